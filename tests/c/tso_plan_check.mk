# Builds tso_plan_check (test infrastructure): the host planning header of one-pass TCP segmentation
# (nstack_amd/csrc/tso_plan.hpp, which calls txf_plan.hpp) in a stand-alone program under
# AddressSanitizer and UBSan. Host code only: no HIP, no GPU, nothing loaded into Python.
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
CXX  ?= g++

$(HERE)tso_plan_check: $(HERE)tso_plan_check.cpp $(HERE)../../nstack_amd/csrc/tso_plan.hpp $(HERE)../../nstack_amd/csrc/txf_plan.hpp
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $<

clean:
	rm -f $(HERE)tso_plan_check

.PHONY: clean
