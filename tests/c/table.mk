# Sanitizer build of the host side of encrypted tables (a makefile of its own beside tests/c/Makefile, client.mk, sampler.mk,
# public.mk, fold.mk and lookup.mk, with the same build/ directory, which tests/c/Makefile's `clean` removes):
#                                                                                     make -C tests/c -f table.mk table_asan
#   build/table_harness   table_harness.cpp + the host sources it calls (fbs_error.cpp, fbs_host.cpp) with -DFBS_HOST_ONLY, g++ and
#                         no HIP headers, under AddressSanitizer and UBSan
# tests/test_table_sanitizers.py builds it and runs it as a program of its own.
HERE  := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
ROOT  := $(HERE)../..
CSRC  := $(ROOT)/tfhe_fbs_map_amd/csrc
OUT   := $(HERE)build
SAN   := -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g -O1
SRCS  := $(HERE)table_harness.cpp $(CSRC)/fbs_error.cpp $(CSRC)/fbs_host.cpp

table_asan: $(OUT)/table_harness

$(OUT)/table_harness: $(SRCS) $(wildcard $(CSRC)/*.hpp) $(ROOT)/include/fbs_exec.h
	@mkdir -p $(OUT)
	g++ -std=c++17 $(SAN) -Wall -Wextra -pthread -ffp-contract=off -DFBS_HOST_ONLY -o $@ $(SRCS)

.PHONY: table_asan
