# Sanitizer build of the client library's sources (a makefile of its own beside tests/c/Makefile, with the same flags and the same
# build/ directory, which that file's `clean` removes):        make -C tests/c -f client.mk client_asan
#   build/client_harness  csrc/fbs_error.cpp + fbs_host.cpp + fbs_client_entries.cpp + fbs_client_capi.cpp, compiled as `make client`
#                         compiles them (FBS_HOST_ONLY, no HIP headers) plus the sanitizers, + client_harness.c, a C program that drives them
#                         through the C ABI alone
# tests/test_client_sanitizers.py builds and runs it.
HERE  := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
ROOT  := $(HERE)../..
CSRC  := $(ROOT)/tfhe_fbs_map_amd/csrc
OUT   := $(HERE)build
SAN   := -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g -O1

client_asan: $(OUT)/client_harness

CLIENT_SRCS := $(CSRC)/fbs_error.cpp $(CSRC)/fbs_host.cpp $(CSRC)/fbs_client_entries.cpp $(CSRC)/fbs_client_capi.cpp
$(OUT)/client_harness: $(HERE)client_harness.c $(CLIENT_SRCS) $(CSRC)/fbs_api_checks.hpp $(CSRC)/fbs_internal.hpp $(CSRC)/fbs_field.hpp $(CSRC)/fbs_select.hpp \
                       $(CSRC)/fbs_chacha.hpp $(CSRC)/fbs_sampler.hpp $(CSRC)/fbs_compact.hpp $(CSRC)/fbs_pack.hpp $(ROOT)/include/fbs_exec.h
	@mkdir -p $(OUT)
	gcc -std=c11 $(SAN) -Wall -Wextra -c -o $(OUT)/client_harness.o $(HERE)client_harness.c
	g++ -std=c++17 $(SAN) -Wall -DFBS_HOST_ONLY -pthread -ffp-contract=off -o $@ $(OUT)/client_harness.o $(CLIENT_SRCS)

.PHONY: client_asan
