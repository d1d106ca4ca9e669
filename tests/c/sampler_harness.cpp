// The rounded-Gaussian sampler (csrc/fbs_sampler.hpp) under AddressSanitizer and UBSan, as a program of its own: gauss_sample on the
// planted windows of tests/test_sampler.py -- U = 0, 2^128 - 1, 2^j and 2^j - 1 for every j, t at 0, 2^53 - 1 and every octant
// boundary +- 1 -- and on 2^16 random ones, at sigma = 1, 2^30 and q.  UBSan's float-to-integer and shift checks are the point: the
// leading-zero count, the normalising shifts of U and the conversion of sigma z to an int64.  Every sample is held to the 13.4 sigma
// the header promises, sigma 0 to "no draw", and the dispatch of sample_window to its two samplers.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../tfhe_fbs_map_amd/csrc/fbs_sampler.hpp"

using fbs::FQ;

static int failures = 0;
#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            std::printf("FAIL: " __VA_ARGS__);    \
            std::printf("\n");                    \
            failures++;                           \
        }                                         \
    } while (0)

struct Window {
    uint64_t w[6];
};

static Window make(unsigned __int128 U, uint64_t t, uint64_t fill) {
    return Window{{(uint64_t)(U >> 64), (uint64_t)U, (t << 11) | (fill & 0x7FF), fill, ~fill, fill}};
}

static uint64_t splitmix(uint64_t &s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

int main() {
    std::vector<Window> ws;
    const unsigned __int128 one = 1, all = ~(unsigned __int128)0;
    std::vector<unsigned __int128> Us = {0, all};
    for (int j = 0; j < 128; j++) {
        Us.push_back(one << j);
        Us.push_back((one << j) - 1);
    }
    std::vector<uint64_t> ts = {0, (1ull << 53) - 1, 1, (1ull << 50) - 1};
    for (uint64_t o = 1; o < 8; o++)
        for (int d = -1; d <= 1; d++) ts.push_back((o << 50) + (uint64_t)(int64_t)d);
    for (unsigned __int128 U : Us)
        for (uint64_t t : std::vector<uint64_t>{0, (1ull << 52) + 12345, (3ull << 50) - 1, (1ull << 53) - 1}) ws.push_back(make(U, t, ~0ull));
    for (uint64_t t : ts)
        for (unsigned __int128 U : std::vector<unsigned __int128>{0, one << 127, all, one << 64, (one << 64) - 1, (unsigned __int128)0xB504F333F9DE6484ull << 64})
            ws.push_back(make(U, t, 0));
    const size_t planted = ws.size();
    uint64_t seed = 2024;
    for (int i = 0; i < (1 << 16); i++) {
        Window x;
        for (int j = 0; j < 6; j++) x.w[j] = splitmix(seed);
        ws.push_back(x);
    }
    for (uint64_t sigma : std::vector<uint64_t>{1, 1ull << 30, FQ}) {
        int64_t sum = 0, worst = 0;
        for (size_t i = 0; i < ws.size(); i++) {
            const int64_t x = fbs::gauss_sample(ws[i].w, sigma);
            const int64_t a = x < 0 ? -x : x;
            CHECK((double)a <= 13.4 * (double)sigma, "window %zu at sigma %" PRIu64 ": %" PRId64, i, sigma, x);
            CHECK(fbs::sample_window(fbs::SAMPLER_GAUSS, ws[i].w, sigma) == x, "dispatch, window %zu", i);
            CHECK(fbs::sample_window(fbs::SAMPLER_IRWIN_HALL, ws[i].w, sigma) == fbs::irwin_hall_sample(ws[i].w, sigma), "dispatch 0, window %zu", i);
            CHECK(fbs::gauss_sample(ws[i].w, 0) == 0, "sigma 0, window %zu", i);
            sum += x % 1000003;
            if (a > worst) worst = a;
        }
        std::printf("sigma %" PRIu64 ": %zu windows (%zu planted), largest |x| %" PRId64 ", checksum %" PRId64 "\n", sigma, ws.size(), planted, worst, sum);
    }
    // the two ends of the radius, exactly: U = 0 at angle 0 is rint(sqrt(2 128 ln 2) 2^30), u1 = 1 - 2^-53 at angle 0 is 2^-26 sigma
    const int64_t top = fbs::gauss_sample(make(0, 0, 0).w, 1ull << 30);
    CHECK(top >= 14303179307ll && top <= 14303179309ll, "U = 0: %" PRId64, top);
    CHECK(fbs::gauss_sample(make(all, 0, 0).w, 1ull << 30) == 16, "U = 2^128 - 1");
    CHECK(fbs::gauss_sample(make(all, 1ull << 52, 0).w, 1ull << 30) == -16, "U = 2^128 - 1 at angle pi");
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("sampler ok\n");
    return 0;
}
