# Sanitizer build of the rounded-Gaussian sampler (a makefile of its own beside tests/c/Makefile and client.mk, with the same
# build/ directory, which tests/c/Makefile's `clean` removes):        make -C tests/c -f sampler.mk sampler_asan
#   build/sampler_harness  sampler_harness.cpp + csrc/fbs_sampler.hpp (header-only: fbs_chacha.hpp, fbs_field.hpp), with g++ and no
#                          HIP headers, under AddressSanitizer and UBSan with the float-to-integer conversion check, which
#                          -fsanitize=undefined alone leaves out
# tests/test_sampler_sanitizers.py builds and runs it.
HERE  := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
ROOT  := $(HERE)../..
CSRC  := $(ROOT)/tfhe_fbs_map_amd/csrc
OUT   := $(HERE)build
SAN   := -fsanitize=address,undefined -fsanitize=float-cast-overflow -fno-sanitize-recover=undefined,float-cast-overflow -fno-omit-frame-pointer -g -O1

sampler_asan: $(OUT)/sampler_harness

$(OUT)/sampler_harness: $(HERE)sampler_harness.cpp $(CSRC)/fbs_sampler.hpp $(CSRC)/fbs_chacha.hpp $(CSRC)/fbs_field.hpp
	@mkdir -p $(OUT)
	g++ -std=c++17 $(SAN) -Wall -Wextra -ffp-contract=off -o $@ $(HERE)sampler_harness.cpp

.PHONY: sampler_asan
