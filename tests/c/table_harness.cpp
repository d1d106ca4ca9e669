// Sanitizer harness for the HOST side of encrypted tables (include/fbs_exec.h, "encrypted tables"): csrc/fbs_host.cpp's
// host_table_map, what fbs_table_map answers, into exactly-sized heap buffers, built by tests/c/table.mk with g++ under
// AddressSanitizer and UBSan and run by tests/test_table_sanitizers.py as a program of its own.  No GPU, no HIP call.
//
// At every p in {2, 4, 5, 7, 15, 31}, N in {64, 256, 1024} and spread in {1, 2, 3} that leaves an entry, with len = 1 and
// floor(p / spread), a small and a large base and stride: every entry against the wide-box rule restated here in SIGNED arithmetic
// (the source works in unsigned), spread 1 against host_lookup_map, and the refusals -- which write nothing.
#include <cstdio>
#include <vector>

#include "../../tfhe_fbs_map_amd/csrc/fbs_internal.hpp"

using namespace fbs;

// floor((2 p c + s N) / (2 s N)) for signed c
static int64_t wide_slot(int64_t c, int64_t p, int64_t N, int64_t s) {
    const int64_t num = 2 * p * c + s * N, den = 2 * s * N;
    return num >= 0 ? num / den : -((-num + den - 1) / den);
}

int main() {
    int failures = 0, cases = 0;
    const uint32_t ps[6] = {2, 4, 5, 7, 15, 31}, Ns[3] = {64, 256, 1024};
    for (uint32_t p : ps)
        for (uint32_t N : Ns)
            for (uint32_t s = 1; s <= 3; s++) {
                if (p / s == 0) continue;
                const uint32_t lens[2] = {1, p / s};
                for (uint32_t len : lens) {
                    // (the largest index the map names is base + (len - 1) stride: the last pair puts it at 2^31 - 1)
                    const uint32_t big_stride = 60000000u;
                    const uint32_t pairs[3][2] = {{0, 1}, {12345, 7}, {0x7FFFFFFFu - (len - 1) * big_stride, big_stride}};
                    for (const auto &bs : pairs) {
                        const uint32_t base = bs[0], stride = bs[1];
                        std::vector<uint32_t> map(N);   // exactly N words: one past is the sanitizer's
                        if (host_table_map(p, N, s, len, base, stride, map.data()) != FBS_OK) {
                            printf("FAIL refused p=%u N=%u s=%u len=%u base=%u stride=%u\n", p, N, s, len, base, stride);
                            failures++;
                            continue;
                        }
                        for (uint32_t j = 0; j < N; j++) {
                            const int64_t w = wide_slot(j, p, N, s);
                            const uint32_t want = w < (int64_t)len                                   ? base + (uint32_t)w * stride
                                                  : wide_slot((int64_t)j - (int64_t)N, p, N, s) == 0 ? base | FOLD_MAP_NEG
                                                                                                     : FOLD_MAP_NONE;
                            if (map[j] != want) {
                                printf("FAIL p=%u N=%u s=%u len=%u j=%u: %08x, want %08x\n", p, N, s, len, j, map[j], want);
                                failures++;
                                break;
                            }
                        }
                        if (s == 1) {
                            std::vector<uint32_t> box(N);
                            if (host_lookup_map(p, N, len, base, stride, box.data()) != FBS_OK || box != map) {
                                printf("FAIL p=%u N=%u len=%u: spread 1 is not the box map\n", p, N, len);
                                failures++;
                            }
                        }
                        if (map[0] != base || map[N - 1] != (base | FOLD_MAP_NEG)) {
                            printf("FAIL p=%u N=%u s=%u len=%u: entry 0 does not open and close the polynomial\n", p, N, s, len);
                            failures++;
                        }
                        cases++;
                    }
                }
            }
    // refusals: nothing is written
    std::vector<uint32_t> keep(256, 0x5A5A5A5Au);
    const uint32_t bad[9][6] = {{7, 256, 0, 1, 0, 1}, {7, 256, 2, 0, 0, 1}, {7, 256, 2, 4, 0, 1}, {7, 256, 8, 1, 0, 1}, {7, 256, 0xFFFFFFFFu, 1, 0, 1},
                                {1, 256, 1, 1, 0, 1}, {7, 300, 2, 3, 0, 1}, {7, 256, 2, 3, 0x80000000u, 1}, {7, 256, 2, 3, 0, 0x40000000u}};
    for (const auto &b : bad) {
        if (host_table_map(b[0], b[1], b[2], b[3], b[4], b[5], keep.data()) != FBS_E_INVALID) {
            printf("FAIL accepted p=%u N=%u spread=%u len=%u\n", b[0], b[1], b[2], b[3]);
            failures++;
        }
        for (uint32_t w : keep)
            if (w != 0x5A5A5A5Au) {
                printf("FAIL a refused call wrote\n");
                failures++;
                break;
            }
    }
    if (host_table_map(7, 256, 2, 3, 0, 1, nullptr) != FBS_E_INVALID) {
        printf("FAIL null output accepted\n");
        failures++;
    }
    printf("ok table maps: %d cases\n", cases);
    printf(failures ? "table FAILED\n" : "table ok\n");
    return failures ? 1 : 0;
}
