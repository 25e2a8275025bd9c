# Builds host_chunk_check (test infrastructure): the chunker of the host forms
# (nstack_amd/csrc/host_chunk.hpp) in a stand-alone program under AddressSanitizer and UBSan. Host code
# only: no HIP, no GPU, nothing loaded into Python.
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
CXX  ?= g++

$(HERE)host_chunk_check: $(HERE)host_chunk_check.cpp $(HERE)../../nstack_amd/csrc/host_chunk.hpp
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $<

clean:
	rm -f $(HERE)host_chunk_check

.PHONY: clean
