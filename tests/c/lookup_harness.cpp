// Sanitizer harness for the HOST side of encrypted-index reads (include/fbs_exec.h, "encrypted-index reads"): csrc/fbs_host.cpp's
// host_lookup_map, what fbs_lookup_map answers, into exactly-sized heap buffers, built by tests/c/lookup.mk with g++ under
// AddressSanitizer and UBSan and run by tests/test_lookup_sanitizers.py as a program of its own.  No GPU, no HIP call.
//
// At every p in {2, 7, 15, 31} and N in {256, 1024}, with len = 1, p - 1 and p, a small and a large base and stride: every entry
// against the box rule restated here, the run lengths of the boxes, and the refusals -- which write nothing.
#include <cstdio>
#include <vector>

#include "../../tfhe_fbs_map_amd/csrc/fbs_internal.hpp"

using namespace fbs;

int main() {
    int failures = 0, cases = 0;
    const uint32_t ps[4] = {2, 7, 15, 31}, Ns[2] = {256, 1024};
    for (uint32_t p : ps)
        for (uint32_t N : Ns) {
            const uint32_t lens[3] = {1, p - 1, p};
            for (uint32_t len : lens) {
                // (the largest index the map names is base + (len - 1) stride: the last pair puts it at 2^31 - 1)
                const uint32_t big_stride = 60000000u;
                const uint32_t pairs[3][2] = {{0, 1}, {12345, 7}, {0x7FFFFFFFu - (len - 1) * big_stride, big_stride}};
                for (const auto &bs : pairs) {
                    const uint32_t base = bs[0], stride = bs[1];
                    std::vector<uint32_t> map(N);   // exactly N words: one past is the sanitizer's
                    if (host_lookup_map(p, N, len, base, stride, map.data()) != FBS_OK) {
                        printf("FAIL refused p=%u N=%u len=%u base=%u stride=%u\n", p, N, len, base, stride);
                        failures++;
                        continue;
                    }
                    uint32_t negs = 0;
                    for (uint32_t j = 0; j < N; j++) {
                        const uint64_t x = ((uint64_t)2 * p * j + N) / (2ull * N);
                        const uint32_t want = x < len ? base + (uint32_t)x * stride : x < p ? FOLD_MAP_NONE : base | FOLD_MAP_NEG;
                        if (map[j] != want) {
                            printf("FAIL p=%u N=%u len=%u j=%u: %08x, want %08x\n", p, N, len, j, map[j], want);
                            failures++;
                            break;
                        }
                        negs += x == p;
                    }
                    // the half box below X^N: floor(N / 2p) coefficients (those with 2 p j + N >= 2 p N), and entry 0 opens the polynomial
                    if (negs != N / (2 * p) || map[0] != base) {
                        printf("FAIL p=%u N=%u len=%u: %u coefficients in the half box\n", p, N, len, negs);
                        failures++;
                    }
                    cases++;
                }
            }
        }
    // refusals: nothing is written
    std::vector<uint32_t> keep(256, 0x5A5A5A5Au);
    const uint32_t bad[6][5] = {{7, 256, 0, 0, 1}, {7, 256, 8, 0, 1}, {1, 256, 1, 0, 1}, {7, 300, 3, 0, 1}, {7, 256, 3, 0x80000000u, 1},
                                {7, 256, 3, 0, 0x40000000u}};
    for (const auto &b : bad) {
        if (host_lookup_map(b[0], b[1], b[2], b[3], b[4], keep.data()) != FBS_E_INVALID) {
            printf("FAIL accepted p=%u N=%u len=%u\n", b[0], b[1], b[2]);
            failures++;
        }
        for (uint32_t w : keep)
            if (w != 0x5A5A5A5Au) {
                printf("FAIL a refused call wrote\n");
                failures++;
                break;
            }
    }
    if (host_lookup_map(7, 256, 3, 0, 1, nullptr) != FBS_E_INVALID) {
        printf("FAIL null output accepted\n");
        failures++;
    }
    printf("ok lookup maps: %d cases\n", cases);
    printf(failures ? "lookup FAILED\n" : "lookup ok\n");
    return failures ? 1 : 0;
}
