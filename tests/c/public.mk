# Sanitizer build of the public-key encryptor (a makefile of its own beside tests/c/Makefile, client.mk and sampler.mk, with the
# same build/ directory, which tests/c/Makefile's `clean` removes):        make -C tests/c -f public.mk public_asan
#   build/public_harness  public_harness.cpp + the three host sources of libfbspublic.so (fbs_error.cpp, fbs_host.cpp,
#                         fbs_public.cpp) with -DFBS_HOST_ONLY, g++ and no HIP headers, under AddressSanitizer and UBSan
# tests/test_public_sanitizers.py builds it and runs it as a program of its own.
HERE  := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
ROOT  := $(HERE)../..
CSRC  := $(ROOT)/tfhe_fbs_map_amd/csrc
OUT   := $(HERE)build
SAN   := -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g -O1
SRCS  := $(HERE)public_harness.cpp $(CSRC)/fbs_error.cpp $(CSRC)/fbs_host.cpp $(CSRC)/fbs_public.cpp

public_asan: $(OUT)/public_harness

$(OUT)/public_harness: $(SRCS) $(wildcard $(CSRC)/*.hpp) $(ROOT)/include/fbs_exec.h
	@mkdir -p $(OUT)
	g++ -std=c++17 $(SAN) -Wall -Wextra -pthread -ffp-contract=off -DFBS_HOST_ONLY -o $@ $(SRCS)

.PHONY: public_asan
