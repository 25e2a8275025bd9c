# Builds mux_plan_check (test infrastructure): the host planning header of one-pass TX multiplexing
# (nstack_amd/csrc/mux_plan.hpp) in a stand-alone program under AddressSanitizer and UBSan. Host code
# only: no HIP, no GPU, nothing loaded into Python.
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
CXX  ?= g++

$(HERE)mux_plan_check: $(HERE)mux_plan_check.cpp $(HERE)../../nstack_amd/csrc/mux_plan.hpp
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $<

clean:
	rm -f $(HERE)mux_plan_check

.PHONY: clean
