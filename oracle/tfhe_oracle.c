/*
 * oracle/tfhe_oracle.c -- TEST INFRASTRUCTURE, NOT PRODUCT CODE (see header).
 *
 * Plain-C restatement of the encrypted functional bootstrap that stands behind
 * one `Bootstrap(src, table)` instruction of the reference's FBS programs
 * (fbs_mapper/fbs_exec_env.py:51-61, cleartext semantics at :218-220) and of
 * the `LinearProd` instruction (:37-49, semantics :215-217).  The reference
 * only ever evaluates those in the clear; the cryptographic algorithm is the
 * published CGGI/TFHE programmable bootstrap in the order the reference's cost
 * model assumes (experiments/concrete.patch:62-74: dot product -> key switch
 * -> PBS), restated from the literature.  Ciphertext-level parity is therefore
 * "unpinned" against any third party; decrypted results ARE pinned against the
 * reference's cleartext goldens (tests/test_oracle_*.py).
 *
 * Deliberately simple: textbook twist + radix-2 cyclic NTT, integer (__int128,
 * Barrett) modular products -- the GPU computes the same residues with FP64 FMAs --, no tricks shared with the HIP kernels, so that agreement between
 * the two is evidence and not an echo.
 */
#include "tfhe_oracle.h"

#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

typedef unsigned __int128 u128;
typedef __int128 i128;
#define Q ORC_Q

/* ------------------------------------------------------------------------ */
/* field Z_q, q = 2^46 - 62*2^13 + 1 = 0x3FFFFFF84001 (prime, 2^14 | q-1)     */
/* ------------------------------------------------------------------------ */
/* branch-free forms: the data are random, so `if` mispredicts half the time */
static inline uint64_t gl_add(uint64_t a, uint64_t b) {
    uint64_t s = a + b; /* < 2^47 */
    return s - (Q & ((uint64_t)0 - (uint64_t)(s >= Q)));
}
static inline uint64_t gl_sub(uint64_t a, uint64_t b) {
    uint64_t d = a - b;
    return d + (Q & ((uint64_t)0 - (uint64_t)(a < b)));
}
static inline uint64_t gl_neg(uint64_t a) { return (Q - a) & ((uint64_t)0 - (uint64_t)(a != 0)); }
/* Barrett: x < q^2 < 2^92, mu = floor(2^92 / q); estimate floor(x/q) from the top bits, fix by <= 2 subtractions */
#define BARRETT_MU ((uint64_t)(((u128)1 << 92) / Q))
static inline uint64_t gl_reduce(u128 x) {
    uint64_t qhat = (uint64_t)(((u128)(uint64_t)(x >> 45) * BARRETT_MU) >> 47);
    uint64_t r = (uint64_t)x - qhat * Q; /* exact mod 2^64: the true remainder estimate is < 3q */
    r -= Q & ((uint64_t)0 - (uint64_t)(r >= Q));
    r -= Q & ((uint64_t)0 - (uint64_t)(r >= Q));
    return r;
}
static inline uint64_t gl_mul(uint64_t a, uint64_t b) { return gl_reduce((u128)a * b); }
/* canonical for every int64: |v| is taken in unsigned arithmetic (INT64_MIN has no negative), and a negative multiple of q is 0, not q */
static inline uint64_t gl_from_i64(int64_t v) {
    if (v >= 0) return (uint64_t)v % Q;
    return gl_neg(((uint64_t)0 - (uint64_t)v) % Q);
}

uint64_t orc_gl_mul(uint64_t a, uint64_t b) { return gl_mul(a % Q, b % Q); }
/* same product by 128-bit division: the unit tests hold the two against each other */
uint64_t orc_gl_mul_slow(uint64_t a, uint64_t b) { return (uint64_t)(((u128)(a % Q) * (b % Q)) % Q); }
uint64_t orc_gl_pow(uint64_t a, uint64_t e) {
    uint64_t r = 1;
    a %= Q;
    while (e) {
        if (e & 1) r = gl_mul(r, a);
        a = gl_mul(a, a);
        e >>= 1;
    }
    return r;
}
static uint64_t gl_inv(uint64_t a) { return orc_gl_pow(a, Q - 2); }

/* ------------------------------------------------------------------------ */
/* textbook negacyclic NTT: twist by psi^j, cyclic radix-2 DIT, natural order */
/* ------------------------------------------------------------------------ */
typedef struct {
    uint32_t log_n, N;
    uint64_t *psi_pow;     /* psi^j           j<N */
    uint64_t *psi_inv_pow; /* psi^-j * N^-1   j<N */
    uint64_t *w_pow;       /* omega^j         j<N/2, omega = psi^2 */
    uint64_t *w_inv_pow;
    uint32_t *brev;
} ntt_plan;

static ntt_plan *plan_new(uint32_t log_n) {
    ntt_plan *pl = calloc(1, sizeof *pl);
    uint32_t N = 1u << log_n;
    pl->log_n = log_n;
    pl->N = N;
    /* 7 generates Z_q^*; psi = 7^((q-1)/2N) is a primitive 2N-th root of unity */
    uint64_t psi = orc_gl_pow(7, (Q - 1) / (2ull * N));
    uint64_t psi_inv = gl_inv(psi);
    uint64_t n_inv = gl_inv(N);
    pl->psi_pow = malloc(N * 8);
    pl->psi_inv_pow = malloc(N * 8);
    pl->w_pow = malloc(N / 2 * 8 + 8);
    pl->w_inv_pow = malloc(N / 2 * 8 + 8);
    pl->brev = malloc(N * 4);
    uint64_t a = 1, b = n_inv;
    for (uint32_t j = 0; j < N; j++) {
        pl->psi_pow[j] = a;
        pl->psi_inv_pow[j] = b;
        a = gl_mul(a, psi);
        b = gl_mul(b, psi_inv);
    }
    uint64_t w = gl_mul(psi, psi), wi = gl_mul(psi_inv, psi_inv);
    a = 1;
    b = 1;
    for (uint32_t j = 0; j < N / 2; j++) {
        pl->w_pow[j] = a;
        pl->w_inv_pow[j] = b;
        a = gl_mul(a, w);
        b = gl_mul(b, wi);
    }
    for (uint32_t j = 0; j < N; j++) {
        uint32_t r = 0;
        for (uint32_t t = 0; t < log_n; t++) r |= ((j >> t) & 1u) << (log_n - 1 - t);
        pl->brev[j] = r;
    }
    return pl;
}
static void plan_free(ntt_plan *pl) {
    if (!pl) return;
    free(pl->psi_pow);
    free(pl->psi_inv_pow);
    free(pl->w_pow);
    free(pl->w_inv_pow);
    free(pl->brev);
    free(pl);
}

static void cyclic_ntt(const ntt_plan *pl, uint64_t *a, const uint64_t *wtab) {
    uint32_t N = pl->N;
    for (uint32_t j = 0; j < N; j++) {
        uint32_t r = pl->brev[j];
        if (j < r) {
            uint64_t t = a[j];
            a[j] = a[r];
            a[r] = t;
        }
    }
    for (uint32_t len = 2; len <= N; len <<= 1) {
        uint32_t half = len >> 1, step = N / len;
        for (uint32_t s = 0; s < N; s += len)
            for (uint32_t j = 0; j < half; j++) {
                uint64_t u = a[s + j], v = gl_mul(a[s + j + half], wtab[j * step]);
                a[s + j] = gl_add(u, v);
                a[s + j + half] = gl_sub(u, v);
            }
    }
}
/* coefficient -> evaluation at psi^(2i+1), natural order */
static void ntt_fwd(const ntt_plan *pl, uint64_t *a) {
    for (uint32_t j = 0; j < pl->N; j++) a[j] = gl_mul(a[j], pl->psi_pow[j]);
    cyclic_ntt(pl, a, pl->w_pow);
}
static void ntt_inv(const ntt_plan *pl, uint64_t *a) {
    cyclic_ntt(pl, a, pl->w_inv_pow);
    for (uint32_t j = 0; j < pl->N; j++) a[j] = gl_mul(a[j], pl->psi_inv_pow[j]);
}

void orc_negacyclic_mul_schoolbook(const uint64_t *a, const uint64_t *b, uint64_t *c, uint32_t N) {
    for (uint32_t i = 0; i < N; i++) c[i] = 0;
    for (uint32_t i = 0; i < N; i++)
        for (uint32_t j = 0; j < N; j++) {
            uint64_t t = gl_mul(a[i] % Q, b[j] % Q);
            uint32_t d = i + j;
            if (d < N) c[d] = gl_add(c[d], t);
            else c[d - N] = gl_sub(c[d - N], t);
        }
}
void orc_negacyclic_mul_ntt(const uint64_t *a, const uint64_t *b, uint64_t *c, uint32_t log_n) {
    ntt_plan *pl = plan_new(log_n);
    uint32_t N = pl->N;
    uint64_t *x = malloc(N * 8), *y = malloc(N * 8);
    for (uint32_t i = 0; i < N; i++) {
        x[i] = a[i] % Q;
        y[i] = b[i] % Q;
    }
    ntt_fwd(pl, x);
    ntt_fwd(pl, y);
    for (uint32_t i = 0; i < N; i++) c[i] = gl_mul(x[i], y[i]);
    ntt_inv(pl, c);
    free(x);
    free(y);
    plan_free(pl);
}

/* ------------------------------------------------------------------------ */
/* ChaCha20 (djb layout: 64-bit block counter, 64-bit stream id)            */
/* ------------------------------------------------------------------------ */
static inline uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
#define QR(a, b, c, d) \
    a += b; d ^= a; d = rotl32(d, 16); \
    c += d; b ^= c; b = rotl32(b, 12); \
    a += b; d ^= a; d = rotl32(d, 8);  \
    c += d; b ^= c; b = rotl32(b, 7)

static void chacha_block(uint64_t seed, uint64_t stream, uint64_t block, uint32_t out[16]) {
    uint32_t in[16], x[16];
    in[0] = 0x61707865u; in[1] = 0x3320646eu; in[2] = 0x79622d32u; in[3] = 0x6b206574u;
    in[4] = (uint32_t)seed; in[5] = (uint32_t)(seed >> 32);
    /* fixed key tail: ASCII "fbs-exec-amd-gfx950-key1" */
    in[6] = 0x2d736266u; in[7] = 0x63657865u; in[8] = 0x646d612du;
    in[9] = 0x7866672du; in[10] = 0x2d303539u; in[11] = 0x3179656bu;
    in[12] = (uint32_t)block; in[13] = (uint32_t)(block >> 32);
    in[14] = (uint32_t)stream; in[15] = (uint32_t)(stream >> 32);
    memcpy(x, in, sizeof x);
    for (int r = 0; r < 10; r++) {
        QR(x[0], x[4], x[8], x[12]);
        QR(x[1], x[5], x[9], x[13]);
        QR(x[2], x[6], x[10], x[14]);
        QR(x[3], x[7], x[11], x[15]);
        QR(x[0], x[5], x[10], x[15]);
        QR(x[1], x[6], x[11], x[12]);
        QR(x[2], x[7], x[8], x[13]);
        QR(x[3], x[4], x[9], x[14]);
    }
    for (int i = 0; i < 16; i++) out[i] = x[i] + in[i];
}
uint64_t orc_rand64(uint64_t seed, uint64_t stream, uint64_t idx) {
    uint32_t o[16];
    chacha_block(seed, stream, idx >> 3, o);
    uint32_t w = (uint32_t)(idx & 7);
    return (uint64_t)o[2 * w] | ((uint64_t)o[2 * w + 1] << 32);
}
/* a whole run of words; cheaper than one block per word */
static void rand_fill(uint64_t seed, uint64_t stream, uint64_t idx0, uint64_t *dst, size_t count) {
    uint32_t o[16];
    uint64_t cur = ~0ull;
    for (size_t i = 0; i < count; i++) {
        uint64_t idx = idx0 + i;
        if ((idx >> 3) != cur) {
            cur = idx >> 3;
            chacha_block(seed, stream, cur, o);
        }
        uint32_t w = (uint32_t)(idx & 7);
        dst[i] = (uint64_t)o[2 * w] | ((uint64_t)o[2 * w + 1] << 32);
    }
}
/* uniform residue from a 64-bit word: keep the top QBITS bits, fold once (bias 2^-27) */
static inline uint64_t to_field(uint64_t r) {
    r >>= 64 - ORC_QBITS;
    return r >= Q ? r - Q : r;
}

/* Irwin-Hall(12) approximation of a centred Gaussian, integer only: twelve
 * 32-bit uniforms (six 64-bit words idx*6 .. idx*6+5), centred, variance 2^64,
 * scaled by sigma/2^32 with round-half-up. */
int64_t orc_noise(uint64_t seed, uint64_t stream, uint64_t idx, uint64_t sigma) {
    if (sigma == 0) return 0;
    uint64_t w[6];
    rand_fill(seed, stream, idx * 6, w, 6);
    i128 s = 0;
    for (int i = 0; i < 6; i++) s += (i128)(w[i] & 0xFFFFFFFFu) + (i128)(w[i] >> 32);
    s -= (i128)6 * 0xFFFFFFFFll;
    i128 v = s * (i128)sigma + ((i128)1 << 31);
    return (int64_t)(v >> 32); /* arithmetic shift = floor */
}

enum { /* stream domains, stream = (domain << 56) | sub */
    DOM_SK_LWE = 1, DOM_SK_GLWE = 2, DOM_BSK_MASK = 3, DOM_BSK_NOISE = 4,
    DOM_KSK_MASK = 5, DOM_KSK_NOISE = 6, DOM_ENC_MASK = 7, DOM_ENC_NOISE = 8
};
#define STREAM(dom, sub) (((uint64_t)(dom) << 56) | ((uint64_t)(sub) & 0x00FFFFFFFFFFFFFFull))

/* ------------------------------------------------------------------------ */
/* context                                                                   */
/* ------------------------------------------------------------------------ */
struct orc_ctx {
    orc_params p;
    uint64_t seed;
    uint32_t N, big_n, rows;   /* rows = (k+1)*l */
    ntt_plan *plan;
    uint64_t *sk_lwe, *sk_glwe, *bsk, *ksk;
    uint64_t *bsk_hat;         /* oracle-internal: rows in natural-order NTT domain */
    uint64_t delta_half;
    uint64_t g[16];            /* gadget factors round(q / B^(l+1)) */
    uint64_t h[64];            /* key-switch factors round(q / 2^(gamma (v+1))) */
};

static uint64_t round_div_q(uint64_t denom_log2) { /* round(q / 2^e) */
    u128 d = (u128)1 << denom_log2;
    return (uint64_t)(((u128)Q + d / 2) / d);
}

orc_ctx *orc_create(const orc_params *p, uint64_t seed) {
    if (!p || p->l_bsk * p->beta_bsk > ORC_QBITS - 2 || p->t_ksk * p->gamma_ksk > ORC_QBITS - 2 || p->l_bsk > 16 || p->t_ksk > 64 ||
        p->log_n_poly < 2 || p->log_n_poly > 14 || p->k < 1 || p->p_msg < 1 || p->bsk_group > 2 || (p->bsk_group == 2 && (p->n & 1)))
        return NULL;
    orc_ctx *c = calloc(1, sizeof *c);
    c->p = *p;
    c->seed = seed;
    c->N = 1u << p->log_n_poly;
    c->big_n = p->k * c->N;
    c->rows = (p->k + 1) * p->l_bsk;
    c->plan = plan_new(p->log_n_poly);
    c->delta_half = (uint64_t)(((u128)Q + 2ull * p->p_msg) / (4ull * p->p_msg));
    for (uint32_t l = 0; l < p->l_bsk; l++) c->g[l] = round_div_q(p->beta_bsk * (l + 1));
    for (uint32_t v = 0; v < p->t_ksk; v++) c->h[v] = round_div_q(p->gamma_ksk * (v + 1));
    return c;
}
void orc_destroy(orc_ctx *c) {
    if (!c) return;
    plan_free(c->plan);
    free(c->sk_lwe);
    free(c->sk_glwe);
    free(c->bsk);
    free(c->ksk);
    free(c->bsk_hat);
    free(c);
}
uint64_t orc_delta_half(const orc_ctx *c) { return c->delta_half; }
const uint64_t *orc_sk_lwe(const orc_ctx *c) { return c->sk_lwe; }
const uint64_t *orc_sk_glwe(const orc_ctx *c) { return c->sk_glwe; }
const uint64_t *orc_bsk(const orc_ctx *c) { return c->bsk; }
const uint64_t *orc_ksk(const orc_ctx *c) { return c->ksk; }

/* GGSW samples in the bootstrapping key: one per key bit, or three per pair of key bits (bsk_group = 2) */
static size_t n_ggsw(const orc_ctx *c) { return c->p.bsk_group == 2 ? (size_t)c->p.n / 2 * 3 : c->p.n; }
/* the bit GGSW sample g encrypts */
static uint64_t ggsw_bit(const orc_ctx *c, size_t g) {
    if (c->p.bsk_group != 2) return c->sk_lwe[g];
    uint64_t s0 = c->sk_lwe[2 * (g / 3)], s1 = c->sk_lwe[2 * (g / 3) + 1];
    switch (g % 3) {
        case 0: return s0 & (1 - s1);
        case 1: return (1 - s0) & s1;
        default: return s0 & s1;
    }
}
static size_t bsk_words(const orc_ctx *c) { return n_ggsw(c) * c->rows * (c->p.k + 1) * c->N; }
static size_t ksk_words(const orc_ctx *c) { return (size_t)c->big_n * c->p.t_ksk * (c->p.n + 1); }

static void alloc_keys(orc_ctx *c) {
    if (c->sk_lwe) return;
    c->sk_lwe = malloc((size_t)c->p.n * 8);
    c->sk_glwe = malloc((size_t)c->big_n * 8);
    c->bsk = malloc(bsk_words(c) * 8);
    c->ksk = malloc(ksk_words(c) * 8);
    c->bsk_hat = malloc(bsk_words(c) * 8);
}
static void transform_bsk(orc_ctx *c) {
    size_t polys = n_ggsw(c) * c->rows * (c->p.k + 1);
    memcpy(c->bsk_hat, c->bsk, bsk_words(c) * 8);
#pragma omp parallel for schedule(static)
    for (long i = 0; i < (long)polys; i++) ntt_fwd(c->plan, c->bsk_hat + (size_t)i * c->N);
}

/* GLWE encryption of the zero polynomial: comps[k+1][N], B = sum A_c*S_c + E */
static void glwe_encrypt_zero(const orc_ctx *c, uint64_t mask_stream, uint64_t noise_stream, uint64_t *comps) {
    uint32_t N = c->N, k = c->p.k;
    uint64_t *tmp = malloc((size_t)N * 8), *body = comps + (size_t)k * N;
    for (uint32_t j = 0; j < N; j++) body[j] = gl_from_i64(orc_noise(c->seed, noise_stream, j, c->p.sigma_glwe));
    for (uint32_t cc = 0; cc < k; cc++) {
        uint64_t *a = comps + (size_t)cc * N;
        rand_fill(c->seed, mask_stream, (uint64_t)cc * N, a, N);
        for (uint32_t j = 0; j < N; j++) a[j] = to_field(a[j]);
        /* binary key: A*S by shift-and-add (exact, independent of the NTT) */
        memset(tmp, 0, (size_t)N * 8);
        const uint64_t *s = c->sk_glwe + (size_t)cc * N;
        for (uint32_t i = 0; i < N; i++) {
            if (!s[i]) continue;
            for (uint32_t j = 0; j < N; j++) {
                uint32_t d = i + j;
                if (d < N) tmp[d] = gl_add(tmp[d], a[j]);
                else tmp[d - N] = gl_sub(tmp[d - N], a[j]);
            }
        }
        for (uint32_t j = 0; j < N; j++) body[j] = gl_add(body[j], tmp[j]);
    }
    free(tmp);
}

void orc_keygen(orc_ctx *c) {
    alloc_keys(c);
    uint32_t N = c->N, k = c->p.k, n = c->p.n, l = c->p.l_bsk, t = c->p.t_ksk;
    for (uint32_t i = 0; i < n; i++) c->sk_lwe[i] = orc_rand64(c->seed, STREAM(DOM_SK_LWE, 0), i) & 1;
    for (uint32_t i = 0; i < c->big_n; i++) c->sk_glwe[i] = orc_rand64(c->seed, STREAM(DOM_SK_GLWE, 0), i) & 1;
    /* BSK_g = GGSW(bit g): row (cc,lv) = GLWE(0) + bit * g_lv on component cc */
    size_t row_words = (size_t)(k + 1) * N;
#pragma omp parallel for schedule(dynamic, 8)
    for (long r = 0; r < (long)(n_ggsw(c) * c->rows); r++) {
        size_t g = (size_t)r / c->rows;
        uint32_t rr = (uint32_t)(r % c->rows);
        uint32_t cc = rr / l, lv = rr % l;
        uint64_t *row = c->bsk + (size_t)r * row_words;
        glwe_encrypt_zero(c, STREAM(DOM_BSK_MASK, r), STREAM(DOM_BSK_NOISE, r), row);
        if (ggsw_bit(c, g)) row[(size_t)cc * N] = gl_add(row[(size_t)cc * N], c->g[lv]);
    }
    /* KSK[j][v] = LWE_small( sk_glwe[j] * h_v ) */
#pragma omp parallel for schedule(dynamic, 64)
    for (long r = 0; r < (long)((size_t)c->big_n * t); r++) {
        uint32_t j = (uint32_t)(r / t), v = (uint32_t)(r % t);
        uint64_t *row = c->ksk + (size_t)r * (n + 1);
        rand_fill(c->seed, STREAM(DOM_KSK_MASK, r), 0, row, n);
        uint64_t b = gl_from_i64(orc_noise(c->seed, STREAM(DOM_KSK_NOISE, r), 0, c->p.sigma_lwe));
        for (uint32_t i = 0; i < n; i++) {
            row[i] = to_field(row[i]);
            if (c->sk_lwe[i]) b = gl_add(b, row[i]);
        }
        if (c->sk_glwe[j]) b = gl_add(b, c->h[v]);
        row[n] = b;
    }
    transform_bsk(c);
}

void orc_set_keys(orc_ctx *c, const uint64_t *sk_lwe, const uint64_t *sk_glwe, const uint64_t *bsk,
                  const uint64_t *ksk) {
    alloc_keys(c);
    memcpy(c->sk_lwe, sk_lwe, (size_t)c->p.n * 8);
    memcpy(c->sk_glwe, sk_glwe, (size_t)c->big_n * 8);
    memcpy(c->bsk, bsk, bsk_words(c) * 8);
    memcpy(c->ksk, ksk, ksk_words(c) * 8);
    transform_bsk(c);
}

/* ------------------------------------------------------------------------ */
/* encrypt / decrypt (big key)                                               */
/* ------------------------------------------------------------------------ */
void orc_encrypt(const orc_ctx *c, const int64_t *msgs, size_t count, uint64_t nonce0, uint64_t *cts) {
    uint32_t d = c->big_n;
    uint64_t delta = 2 * c->delta_half;
    for (size_t i = 0; i < count; i++) {
        uint64_t *ct = cts + i * (d + 1);
        rand_fill(c->seed, STREAM(DOM_ENC_MASK, nonce0 + i), 0, ct, d);
        uint64_t b = gl_from_i64(orc_noise(c->seed, STREAM(DOM_ENC_NOISE, nonce0 + i), 0, c->p.sigma_glwe));
        for (uint32_t j = 0; j < d; j++) {
            ct[j] = to_field(ct[j]);
            if (c->sk_glwe[j]) b = gl_add(b, ct[j]);
        }
        ct[d] = gl_add(b, gl_mul(gl_from_i64(msgs[i]), delta));
    }
}
void orc_phase(const orc_ctx *c, const uint64_t *cts, size_t count, uint64_t *phases) {
    uint32_t d = c->big_n;
    for (size_t i = 0; i < count; i++) {
        const uint64_t *ct = cts + i * (d + 1);
        uint64_t ph = ct[d];
        for (uint32_t j = 0; j < d; j++)
            if (c->sk_glwe[j]) ph = gl_sub(ph, ct[j]);
        phases[i] = ph;
    }
}
void orc_decrypt(const orc_ctx *c, const uint64_t *cts, size_t count, int64_t *msgs) {
    uint64_t two_p = 2ull * c->p.p_msg;
    for (size_t i = 0; i < count; i++) {
        uint64_t ph;
        orc_phase(c, cts + i * (c->big_n + 1), 1, &ph);
        /* m = round(ph * 2p / q) mod 2p */
        u128 v = (u128)ph * two_p + Q / 2;
        msgs[i] = (int64_t)((uint64_t)(v / Q) % two_p);
    }
}

/* ------------------------------------------------------------------------ */
/* test vector: table -> N coefficients (negacyclic contract, map_to_fbs.py:81-98) */
/* ------------------------------------------------------------------------ */
int orc_build_tv(const orc_ctx *c, const int32_t *table, uint32_t len, uint64_t *tv, uint64_t *post_add) {
    uint32_t p = c->p.p_msg, N = c->N;
    if (len == 0 || len > 2 * p) return -1;
    /* values met at x and x+p must sum to one constant `cst`:
     *   f(x+p) = cst - f(x)   <=>   (f - cst/2) is negacyclic.
     * cst=1: the reference's mode1 (:91), 0: mode2 (:93), 2: mode3 (:95). */
    int64_t cst = 0;
    if (len > p) {
        cst = (int64_t)table[0] + table[p];
        for (uint32_t i = 0; i + p < len; i++)
            if ((int64_t)table[i] + table[i + p] != cst) return -1;
    }
    uint64_t dh = c->delta_half;
    uint64_t enc[4096];
    if (p > 4096) return -1;
    for (uint32_t x = 0; x < p; x++) {
        int64_t f = x < len ? table[x] : 0; /* slots never reached: don't care */
        enc[x] = gl_mul(gl_from_i64(2 * f - cst), dh);
    }
    for (uint32_t j = 0; j < N; j++) {
        uint64_t x = ((uint64_t)j * 2 * p + N) / (2ull * N); /* round(j*p/N) */
        tv[j] = x < p ? enc[x] : gl_neg(enc[0]);
    }
    *post_add = gl_mul(gl_from_i64(cst), dh);
    return 0;
}

/* ------------------------------------------------------------------------ */
/* several tables on ONE blind rotation ("multi-value bootstrap": Carpov, Izabachene, Mollimard, "New techniques for
 * multi-value input homomorphic evaluation and applications", CT-RSA 2019, section 3 -- [NOT IN REFERENCE]: the reference
 * emits several tables per linear combination, fbs_mapper/map_to_fbs.py:41-45, and evaluates them in clear).
 * With TV_0 = delta_half * (1 + X + ... + X^(N-1)) and (1 + X + ... + X^(N-1)) (1 - X) = 1 - X^N = 2 in Z[X]/(X^N+1):
 *     TV_F = delta_half * G(X)   (G_j = +-(2 f - cst), orc_build_tv)   =   TV_0 * D_F,   D_F = G (1 - X) / 2,
 * an INTEGER polynomial (all G_j have the parity of cst) that is zero except where the table changes value.  So
 * X^-phase * TV_F = (X^-phase * TV_0) * D_F: one blind rotation of the table-independent TV_0, then per table a product of
 * the accumulator by the small polynomial D_F and a sample extraction.  The output noise variance grows by |D_F|^2. */
/* ------------------------------------------------------------------------ */
void orc_tv0(const orc_ctx *c, uint64_t *tv) {
    for (uint32_t j = 0; j < c->N; j++) tv[j] = c->delta_half;
}

/* diff[N] = D_F (dense, small signed integers), *post_add as orc_build_tv; returns the same error */
int orc_build_tv_diff(const orc_ctx *c, const int32_t *table, uint32_t len, int32_t *diff, uint64_t *post_add) {
    uint32_t p = c->p.p_msg, N = c->N;
    if (len == 0 || len > 2 * p) return -1;
    int64_t cst = 0;
    if (len > p) {
        cst = (int64_t)table[0] + table[p];
        for (uint32_t i = 0; i + p < len; i++)
            if ((int64_t)table[i] + table[i + p] != cst) return -1;
    }
    int64_t *g = malloc((size_t)N * sizeof *g);
    for (uint32_t j = 0; j < N; j++) {
        uint64_t x = ((uint64_t)j * 2 * p + N) / (2ull * N);
        int64_t f = x < p ? (x < len ? table[x] : 0) : (0 < len ? table[0] : 0);
        g[j] = x < p ? 2 * f - cst : -(2 * f - cst);
    }
    /* (G (1 - X))_j = G_j - G_(j-1), and G_0 + G_(N-1) at j = 0 (X^N = -1) */
    for (uint32_t j = 0; j < N; j++) {
        int64_t d = j ? g[j] - g[j - 1] : g[0] + g[N - 1];
        diff[j] = (int32_t)(d / 2); /* exact: see above */
    }
    free(g);
    *post_add = gl_mul(gl_from_i64(cst), c->delta_half);
    return 0;
}

/* ct_out = SampleExtract_0(acc * D_F) + post_add, acc = the (k+1) polynomials the blind rotation of TV_0 left */
void orc_multi_extract(const orc_ctx *c, const uint64_t *acc, const int32_t *diff, uint64_t post_add, uint64_t *ct_big) {
    uint32_t N = c->N, k = c->p.k;
    uint64_t *prod = calloc((size_t)(k + 1) * N, 8);
    for (uint32_t cc = 0; cc <= k; cc++) {
        const uint64_t *a = acc + (size_t)cc * N;
        uint64_t *o = prod + (size_t)cc * N;
        for (uint32_t i = 0; i < N; i++) {
            if (!diff[i]) continue;
            uint64_t d = gl_from_i64(diff[i]);
            for (uint32_t m = 0; m < N; m++) { /* X^i * a: coefficient m is a[m - i], negated when it wrapped */
                uint64_t t = m >= i ? gl_mul(d, a[m - i]) : gl_neg(gl_mul(d, a[m + N - i]));
                o[m] = gl_add(o[m], t);
            }
        }
    }
    orc_sample_extract(c, prod, post_add, ct_big);
    free(prod);
}

/* ------------------------------------------------------------------------ */
/* the path                                                                  */
/* ------------------------------------------------------------------------ */
void orc_lincomb(const orc_ctx *c, const uint64_t *const *srcs, const int64_t *coefs, uint32_t n_src,
                 int64_t const_coef, uint64_t *out) {
    uint32_t d = c->big_n;
    for (uint32_t j = 0; j <= d; j++) out[j] = 0;
    for (uint32_t s = 0; s < n_src; s++) {
        uint64_t cf = gl_from_i64(coefs[s]);
        for (uint32_t j = 0; j <= d; j++) out[j] = gl_add(out[j], gl_mul(cf, srcs[s][j]));
    }
    out[d] = gl_add(out[d], gl_mul(gl_from_i64(const_coef), 2 * c->delta_half));
}

void orc_keyswitch(const orc_ctx *c, const uint64_t *ct_big, uint64_t *ct_small) {
    uint32_t n = c->p.n, t = c->p.t_ksk, gam = c->p.gamma_ksk, d = c->big_n;
    uint32_t tg = t * gam;
    for (uint32_t i = 0; i < n; i++) ct_small[i] = 0;
    ct_small[n] = ct_big[d];
    const int64_t base = 1ll << gam;
    for (uint32_t j = 0; j < d; j++) {
        /* closest multiple of q/2^(t*gamma): top t*gamma bits, rounded, kept mod 2^(t*gamma) (the dropped carry is a
         * multiple of q); then BALANCED digits in [-B/2, B/2), least significant first, carries propagated */
        uint64_t abar = (((ct_big[j] >> (ORC_QBITS - 1 - tg)) + 1) >> 1) & ((1ull << tg) - 1);
        for (uint32_t v = t; v-- > 0;) {
            int64_t dig = (int64_t)(abar & (uint64_t)(base - 1));
            abar >>= gam;
            if (dig >= base / 2 && base > 1) {
                dig -= base;
                abar += 1;
            }
            if (!dig) continue;
            const uint64_t *row = c->ksk + ((size_t)j * t + v) * (n + 1);
            uint64_t df = gl_from_i64(dig);
            for (uint32_t i = 0; i <= n; i++) ct_small[i] = gl_sub(ct_small[i], gl_mul(df, row[i]));
        }
    }
}

/* Mask words are rounded to the closest multiple of 2^46 / 2N (q treated as 2^46, as everywhere).  The rounding errors
 * eps_i of the mask reach the phase as sum_i eps_i s_i through a BINARY key, whose bits have mean 1/2: the evaluator knows
 * every eps_i, so it removes the expected value sum_i eps_i / 2 from the body before rounding it ("mean-compensated"
 * modulus switch).  What is left is sum_i eps_i (s_i - 1/2): variance n/4 roundings instead of n/2
 * (tfhe_fbs_map_amd/params.py, variances).  [NOT IN REFERENCE]; the halving floors. */
void orc_modswitch(const orc_ctx *c, const uint64_t *ct_small, uint32_t *ms) {
    uint32_t sh = ORC_QBITS - c->p.log_n_poly - 1, mask = 2 * c->N - 1, n = c->p.n; /* sh = bits dropped */
    int64_t eps = 0;
    for (uint32_t i = 0; i < n; i++) {
        uint64_t m = ((ct_small[i] >> (sh - 1)) + 1) >> 1;
        eps += (int64_t)ct_small[i] - (int64_t)(m << sh); /* in [-2^(sh-1), 2^(sh-1)) */
        ms[i] = (uint32_t)m & mask;
    }
    uint64_t body = gl_sub(ct_small[n], gl_from_i64(eps >> 1));
    ms[n] = (uint32_t)(((body >> (sh - 1)) + 1) >> 1) & mask;
}

/* out = X^r * in  (r in [0,2N)) in Z_q[X]/(X^N+1) */
static void poly_rotate(const uint64_t *in, uint64_t *out, uint32_t r, uint32_t N) {
    for (uint32_t j = 0; j < N; j++) {
        uint32_t idx = (j + 2 * N - r) & (2 * N - 1);
        out[j] = idx < N ? in[idx] : gl_neg(in[idx - N]);
    }
}

/* Signed balanced digits of the closest multiple of q/B^l of v (mod q); out[lv][j] as field elements.
 * v is a SIGNED representative in (-q, q): the difference of two centred residues, not reduced again.
 * The rounding treats q as 2^46 (a shift), which scales the value by 2^46/q = 1 + 7.2e-9.  Applied to canonical
 * residues in [0, q) that error is always of one sign and adds up coherently through the N/2 key bits (measured: it
 * dominated the bootstrap noise once l*beta >= 24); on representatives symmetric around 0 it averages out.
 * So: round half up to a multiple of 2^s (s = 46 - l*beta), keep the result mod B^l. */
static void decompose_poly(const orc_ctx *c, const int64_t *poly, uint64_t *digits /* l*N */) {
    uint32_t N = c->N, l = c->p.l_bsk, beta = c->p.beta_bsk;
    uint64_t B = 1ull << beta, half = B >> 1;
    const int s = ORC_QBITS - (int)(l * beta);
    for (uint32_t j = 0; j < N; j++) {
        int64_t t = poly[j] + ((int64_t)1 << (s - 1));
        int64_t r = t >= 0 ? t >> s : -((-t + ((int64_t)1 << s) - 1) >> s);   /* floor(t / 2^s) */
        uint64_t abar = (uint64_t)r & ((1ull << (l * beta)) - 1);
        for (int lv = (int)l - 1; lv >= 0; lv--) {
            int64_t dg = (int64_t)(abar & (B - 1));
            abar >>= beta;
            if ((uint64_t)dg >= half) {
                dg -= (int64_t)B;
                abar += 1;
            }
            digits[(size_t)lv * N + j] = gl_from_i64(dg);
        }
    }
}

/* centred representative in [-(q-1)/2, (q-1)/2] */
static inline int64_t centred(uint64_t a) { return a > ORC_Q / 2 ? (int64_t)a - (int64_t)ORC_Q : (int64_t)a; }

/* Two key bits per step ("multi-bit" blind rotation, group size 2):
 *     X^(a0 s0 + a1 s1) - 1 = s0(1-s1)(X^a0 - 1) + (1-s0)s1(X^a1 - 1) + s0 s1 (X^(a0+a1) - 1),
 * so with GGSW samples E0, E1, E2 of the three products,
 *     ACC += [ (X^a0 - 1) E0 + (X^a1 - 1) E1 + (X^(a0+a1) - 1) E2 ]  (x)  ACC :
 * the bundle in brackets is a linear combination of GGSW samples by known polynomials (built here in the NTT domain,
 * where multiplying by a polynomial is pointwise), and ACC ITSELF is decomposed -- there is no rotate-and-subtract.
 * Half as many external products for 1.5x the key; the key-noise term of a step triples. */
static void blind_rotate_pairs(const orc_ctx *c, const uint32_t *ms, const uint64_t *tv, uint64_t *acc) {
    uint32_t N = c->N, k = c->p.k, n = c->p.n, l = c->p.l_bsk;
    uint32_t comps = k + 1, twoN = 2 * N;
    int64_t *cen = malloc((size_t)N * 8);
    uint64_t *dig = malloc((size_t)l * N * 8);
    uint64_t *sum = malloc((size_t)comps * N * 8);
    uint64_t *mono = malloc((size_t)3 * N * 8);
    memset(acc, 0, (size_t)k * N * 8);
    poly_rotate(tv, acc + (size_t)k * N, (twoN - ms[n]) & (twoN - 1), N); /* X^{-b~} * TV */
    for (uint32_t i = 0; i < n / 2; i++) {
        uint32_t e[3] = {ms[2 * i], ms[2 * i + 1], (ms[2 * i] + ms[2 * i + 1]) & (twoN - 1)};
        if (e[0] == 0 && e[1] == 0) continue; /* the bundle is zero */
        for (uint32_t jj = 0; jj < 3; jj++) { /* X^e - 1 as a polynomial, then its transform */
            uint64_t *m = mono + (size_t)jj * N;
            memset(m, 0, (size_t)N * 8);
            if (e[jj]) {
                m[0] = Q - 1;
                uint32_t pos = e[jj] & (N - 1);
                m[pos] = gl_add(m[pos], e[jj] < N ? 1 : Q - 1);
            }
            ntt_fwd(c->plan, m);
        }
        memset(sum, 0, (size_t)comps * N * 8);
        for (uint32_t cc = 0; cc < comps; cc++) {
            for (uint32_t j = 0; j < N; j++) cen[j] = centred(acc[(size_t)cc * N + j]);
            decompose_poly(c, cen, dig);
            for (uint32_t lv = 0; lv < l; lv++) {
                uint64_t *dh = dig + (size_t)lv * N;
                ntt_fwd(c->plan, dh);
                for (uint32_t oc = 0; oc < comps; oc++)
                    for (uint32_t j = 0; j < N; j++) {
                        uint64_t kw = 0;
                        for (uint32_t jj = 0; jj < 3; jj++) {
                            const uint64_t *row = c->bsk_hat + ((((size_t)i * 3 + jj) * c->rows) + cc * l + lv) * comps * N;
                            kw = gl_add(kw, gl_mul(mono[(size_t)jj * N + j], row[(size_t)oc * N + j]));
                        }
                        sum[(size_t)oc * N + j] = gl_add(sum[(size_t)oc * N + j], gl_mul(dh[j], kw));
                    }
            }
        }
        for (uint32_t oc = 0; oc < comps; oc++) {
            uint64_t *s = sum + (size_t)oc * N;
            ntt_inv(c->plan, s);
            for (uint32_t j = 0; j < N; j++) acc[(size_t)oc * N + j] = gl_add(acc[(size_t)oc * N + j], s[j]);
        }
    }
    free(cen);
    free(dig);
    free(sum);
    free(mono);
}

void orc_blind_rotate(const orc_ctx *c, const uint32_t *ms, const uint64_t *tv, uint64_t *acc) {
    if (c->p.bsk_group == 2) {
        blind_rotate_pairs(c, ms, tv, acc);
        return;
    }
    uint32_t N = c->N, k = c->p.k, n = c->p.n, l = c->p.l_bsk;
    uint32_t comps = k + 1, twoN = 2 * N;
    uint64_t *rot = malloc((size_t)N * 8);
    int64_t *diff = malloc((size_t)comps * N * 8);
    uint64_t *dig = malloc((size_t)l * N * 8);
    uint64_t *sum = malloc((size_t)comps * N * 8);
    memset(acc, 0, (size_t)k * N * 8);
    poly_rotate(tv, acc + (size_t)k * N, (twoN - ms[n]) & (twoN - 1), N); /* X^{-b~} * TV */
    for (uint32_t i = 0; i < n; i++) {
        uint32_t r = ms[i];
        if (r == 0) continue; /* X^0*ACC - ACC = 0 */
        for (uint32_t cc = 0; cc < comps; cc++) {
            /* (X^r - 1) * ACC over the centred representatives, as an integer in (-q, q): not reduced again */
            int64_t *dcc = diff + (size_t)cc * N;
            poly_rotate(acc + (size_t)cc * N, rot, r, N);
            for (uint32_t j = 0; j < N; j++) dcc[j] = centred(rot[j]) - centred(acc[(size_t)cc * N + j]);
        }
        memset(sum, 0, (size_t)comps * N * 8);
        for (uint32_t cc = 0; cc < comps; cc++) {
            decompose_poly(c, diff + (size_t)cc * N, dig);
            for (uint32_t lv = 0; lv < l; lv++) {
                uint64_t *dh = dig + (size_t)lv * N;
                ntt_fwd(c->plan, dh);
                const uint64_t *row = c->bsk_hat + (((size_t)i * c->rows) + cc * l + lv) * comps * N;
                for (uint32_t oc = 0; oc < comps; oc++)
                    for (uint32_t j = 0; j < N; j++)
                        sum[(size_t)oc * N + j] = gl_add(sum[(size_t)oc * N + j], gl_mul(dh[j], row[(size_t)oc * N + j]));
            }
        }
        for (uint32_t oc = 0; oc < comps; oc++) {
            uint64_t *s = sum + (size_t)oc * N;
            ntt_inv(c->plan, s);
            for (uint32_t j = 0; j < N; j++) acc[(size_t)oc * N + j] = gl_add(acc[(size_t)oc * N + j], s[j]);
        }
    }
    free(rot);
    free(diff);
    free(dig);
    free(sum);
}

void orc_sample_extract(const orc_ctx *c, const uint64_t *acc, uint64_t post_add, uint64_t *ct_big) {
    uint32_t N = c->N, k = c->p.k;
    for (uint32_t cc = 0; cc < k; cc++) {
        const uint64_t *a = acc + (size_t)cc * N;
        ct_big[(size_t)cc * N] = a[0];
        for (uint32_t j = 1; j < N; j++) ct_big[(size_t)cc * N + j] = gl_neg(a[N - j]);
    }
    ct_big[(size_t)k * N] = gl_add(acc[(size_t)k * N], post_add);
}

void orc_bootstrap(const orc_ctx *c, const uint64_t *ct_in, const uint64_t *tv, uint64_t post_add, uint64_t *ct_out) {
    uint64_t *small = malloc((size_t)(c->p.n + 1) * 8);
    uint32_t *ms = malloc((size_t)(c->p.n + 1) * 4);
    uint64_t *acc = malloc((size_t)(c->p.k + 1) * c->N * 8);
    orc_keyswitch(c, ct_in, small);
    orc_modswitch(c, small, ms);
    orc_blind_rotate(c, ms, tv, acc);
    orc_sample_extract(c, acc, post_add, ct_out);
    free(small);
    free(ms);
    free(acc);
}

int orc_bootstrap_batch(const orc_ctx *c, const uint64_t *cts_in, const uint32_t *tv_idx, const uint64_t *tvs,
                        const uint64_t *post_adds, size_t count, uint64_t *cts_out, int threads) {
    size_t w = (size_t)c->big_n + 1;
    int used = 1;
#ifdef _OPENMP
    if (threads <= 0) threads = omp_get_max_threads();
    used = threads;
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads)
#endif
    for (long i = 0; i < (long)count; i++) {
        uint32_t ti = tv_idx ? tv_idx[i] : 0;
        orc_bootstrap(c, cts_in + (size_t)i * w, tvs + (size_t)ti * c->N, post_adds ? post_adds[ti] : 0,
                      cts_out + (size_t)i * w);
    }
    return used;
}
