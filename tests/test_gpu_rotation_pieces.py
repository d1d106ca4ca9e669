"""The rotated read of a CMUX step where one wave holds a whole polynomial (k_blind_rotate, LL = 6): the rotation amount r splits
into a lane part rl = r mod 64 and a register part rh = r / 64 that is the same for the whole wave.

Host part (no GPU): a numpy replay of the kernel's decomposition -- one address per lane, register offsets and signs per wave, the
guard slot for the lanes that borrow -- against the negacyclic rotation itself, for every amount at N = 256, 512 and 1024.

GPU part: rotation amounts are PLANTED.  The key-switching key comes in through import_keys with one row per input coefficient
replaced, so that a ciphertext whose only non-zero mask word sits at that coefficient leaves the key switch with exactly the chosen
mask, and the modulus switch with exactly the chosen amounts (asserted through the oracle's own key switch and modulus switch).  Every
output word is compared with the oracle's on the same keys.

The launcher picks the instantiation by batch size and nothing else (csrc/fbs_select.cpp): batches of 1, 4 and 5 run, but on the
one-bootstrap-per-CU kernel; the instantiations this file is about are reached at the batch sizes of CASES below, and each case
asserts which kernel ran."""
import numpy as np
import pytest

from oracle import tfhe_oracle as orc
from tests.helpers import CUS

LANES = 64
N_STEPS = 16
TABLES = [[0, 1, 1, 0, 1, 0, 0], [0, 1, 2, 3, 2, 1, 0]]


def planted_amounts(N):
    """0, 1, 63, 64, 65, N-1, N, N+1, 2N-1 and 64 rh + rl for rh in {0, E-1, E, 2E-1}, rl in {0, 1, 62, 63}: every borrow case, the
    register wrap at slot 0, both signs (at N = 1024: 1023, 1024, 1025, 2047 and rh in {0, 15, 16, 31})"""
    E = N // LANES
    out = [0, 1, 63, 64, 65, N - 1, N, N + 1, 2 * N - 1]
    out += [64 * rh + rl for rh in (0, E - 1, E, 2 * E - 1) for rl in (0, 1, 62, 63)]
    return out


# ---- host only -------------------------------------------------------------------------------------------------------------------
def rotate_by_pieces(acc, r):
    """X^r * acc as the kernel reads it: acc[N] in natural order -> the rotated polynomial, plus the LDS words touched"""
    N = len(acc)
    E, loge = N // LANES, (N // LANES).bit_length() - 1
    regs = acc.reshape(E, LANES)                                  # register m of lane t = coefficient t + 64 m
    image = np.concatenate([-regs[E - 1], acc])                   # [guard slot | buffer]: what the wave stores
    rh, rl = r >> 6, r & 63
    first = (-rh) & (2 * E - 1)                                   # wave-uniform: the register (mod 2E) that register 0 reads
    t = np.arange(LANES)
    base = LANES + t - rl                                         # ONE address per lane (inside the guard slot where t < rl)
    out = np.empty_like(regs)
    words = []
    for m in range(E):
        word = base + ((m + first) & (E - 1)) * LANES             # register offset: an immediate of the read
        sign = -1 if ((first + m) >> loge) & 1 else 1             # wave-uniform factor of the subtraction
        out[m] = sign * image[word]
        words.append(word)
    return out.reshape(N), np.array(words)


def negacyclic_rotation(acc, r):
    N = len(acc)
    rolled = np.roll(np.concatenate([acc, -acc]), r)              # coefficient j of X^r * acc is +-acc[(j - r) mod 2N]
    return rolled[:N]


@pytest.mark.parametrize("N", [256, 512, 1024])
def test_lane_and_register_pieces_equal_the_rotation(N):
    rng = np.random.default_rng(N)
    acc = rng.integers(-(1 << 44), 1 << 44, N)
    acc[acc == 0] = 1                                             # a zero would hide a wrong sign
    for r in range(2 * N):
        got, words = rotate_by_pieces(acc, r)
        assert np.array_equal(got, negacyclic_rotation(acc, r)), r
        assert words.min() >= 0 and words.max() < N + LANES, r   # inside the guard slot and the buffer
        # 8-byte reads are banked per 32 lanes over 32 word positions: consecutive words, whatever the amount
        for half in (words[:, :32], words[:, 32:]):
            assert all(len(set(row % 32)) == 32 for row in half), r


def test_planted_amounts_are_the_listed_ones():
    assert planted_amounts(1024) == [0, 1, 63, 64, 65, 1023, 1024, 1025, 2047,
                                     0, 1, 62, 63, 960, 961, 1022, 1023, 1024, 1025, 1086, 1087, 1984, 1985, 2046, 2047]


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
# (log_n, l, beta, count, knobs, kernel): batch sizes that reach each instantiation with a wave per polynomial, and the three small ones
CASES = [
    (10, 3, 7, 4, {}, None),                                      # the batch sizes of one workgroup's worth and around it:
    (10, 3, 7, 5, {}, None),                                      # (the launcher gives these to the one-bootstrap-per-CU kernel)
    (10, 3, 7, 1, {}, None),
    (10, 3, 7, 4 * CUS, {}, "k_blind_rotate<10,6,3,4>"),          # whole-CU workgroups, four bootstraps each
    (10, 3, 7, 4 * CUS - 3, {}, "k_blind_rotate<10,6,3,4>"),      # ... the last one with three dead sub-slots that repeat the last bootstrap
    (10, 3, 7, CUS + 45, dict(br_cu_kernel=0), "k_blind_rotate<10,6,3,2>"),   # two per workgroup, the last one half empty
    (10, 3, 7, 2 * CUS + 88, {}, "k_blind_rotate<10,6,3,1>"),     # one per workgroup: a step with r = 0 is skipped
    (10, 2, 7, 8 * CUS + 60, {}, "k_blind_rotate<10,6,7,1,false>"),   # no priority hand-over (TURNS = false)
    (9, 3, 7, 40, {}, "k_blind_rotate<9,6,3,1>"),                 # E = 8
    (9, 3, 7, CUS + 45, dict(br_cu_kernel=0), "k_blind_rotate<9,6,3,2>"),
    (8, 3, 7, 40, {}, "k_blind_rotate<8,6,3,1>"),                 # E = 4
    (8, 3, 7, CUS + 45, dict(br_cu_kernel=0), "k_blind_rotate<8,6,3,2>"),
]
T_KSK, GAMMA_KSK = 4, 4


@pytest.fixture(scope="module")
def planted():
    """per (log_n, l, beta): context, oracle and the four lists of amounts, on one set of keys with the planted key-switching rows"""
    from tfhe_fbs_map_amd import Params, _native as nat
    made = {}

    def get(log_n, l, beta):
        if (log_n, l, beta) not in made:
            prm = Params(n=N_STEPS, log_n_poly=log_n, l_bsk=l, beta_bsk=beta, t_ksk=T_KSK, gamma_ksk=GAMMA_KSK, p_msg=7,
                         sigma_lwe=1 << 6, sigma_glwe=1 << 4)
            ctx, o = nat.Context(prm, seed=33), orc.Oracle(prm, seed=33)
            N = 1 << log_n
            amounts = planted_amounts(N)
            lists = [[amounts[(N_STEPS * k + i) % len(amounts)] for i in range(N_STEPS)] for k in range(4)]
            keys = ctx.export_keys()
            ksk = keys["ksk"].reshape(N, T_KSK, N_STEPS + 1)
            shift = 46 - log_n - 1                                # the bits the modulus switch drops
            h0 = (orc.Q + (1 << (GAMMA_KSK - 1))) >> GAMMA_KSK    # the gadget's first element, round(q / 2^gamma)
            for k, amounts_k in enumerate(lists):                 # input coefficient k, most significant digit: mask = -amounts
                mask = [(orc.Q - (a << shift)) % orc.Q for a in amounts_k]
                ksk[k, 0, :N_STEPS] = mask
                # a key row stays an encryption (import_keys checks): body = <mask, s> + sk_glwe[k] h_0, without noise
                ksk[k, 0, N_STEPS] = (sum(m for m, bit in zip(mask, keys["sk_lwe"]) if bit) + (h0 if keys["sk_glwe"][k] else 0)) % orc.Q
            keys["ksk"] = ksk.reshape(-1)
            ctx.import_keys(**keys)
            o.set_keys(**keys)
            made[(log_n, l, beta)] = (ctx, o, lists)
        return made[(log_n, l, beta)]

    yield get
    for ctx, _, _ in made.values():
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("log_n,l,beta,count,knobs,kernel", CASES)
def test_planted_rotation_amounts_against_the_oracle(planted, log_n, l, beta, count, knobs, kernel):
    ctx, o, lists = planted(log_n, l, beta)
    N = 1 << log_n
    ctx.tune(br_cu_kernel=1)
    ctx.tune(**knobs)
    rng = np.random.default_rng(count)
    ids = rng.integers(0, len(TABLES), count).astype(np.uint32)
    msgs = np.array([rng.integers(0, len(TABLES[i])) for i in ids])
    cts = ctx.encrypt(msgs, nonce0=5)                             # (the bodies stay; the masks are planted)
    cts[:, :N] = 0
    which = np.arange(count) % 4
    cts[np.arange(count), which] = 1 << (46 - GAMMA_KSK)          # digit 1 at the most significant level, none below
    for f in range(min(count, 4)):                                # the construction itself: these ARE the amounts the steps see
        assert list(o.modswitch(o.keyswitch(cts[f]))[:N_STEPS]) == lists[f % 4]
    ctx.profile(True)
    ctx.profile_read(reset=True)
    got = ctx.bootstrap_batch(ctx.tvset(TABLES), cts, ids)
    launched = ctx.profile_kernels()
    ctx.profile(False)
    if kernel is not None:
        assert kernel in launched, (kernel, sorted(launched))
    # the first two and the last two workgroups of four, whole (every sub-slot, every list of amounts)
    pick = np.arange(count) if count <= 16 else np.concatenate([np.arange(8), np.arange(count - 8, count)])
    ref, _ = o.bootstrap_batch(cts[pick], TABLES, ids[pick])
    assert np.array_equal(got[pick], ref)
    assert got.max() < orc.Q
