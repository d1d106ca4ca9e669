"""Shared by the test modules: fixture loading and an oracle-backed program evaluator."""
import glob
import gzip
import json
import os
import re

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture_names(pattern="*"):
    names = (os.path.basename(p)[:-len(".json.gz")] for p in glob.glob(os.path.join(GOLDEN, pattern + ".json.gz")))
    return sorted(n for n in names if not n.startswith("_"))        # _*.json.gz: collections, not one program each


def _decode(v):
    if "const" in v:
        return int(v["const"])
    if "bits" in v:
        raw = np.frombuffer(bytes.fromhex(v["bits"]), np.uint8)
        return np.unpackbits(raw)[:v["n"]].astype(np.int64)
    return np.asarray(v["ints"], np.int64)


_cache = {}


def load_fixture(name):
    if name not in _cache:
        with gzip.open(os.path.join(GOLDEN, name + ".json.gz"), "rb") as f:
            rec = json.loads(f.read().decode())
        rec["inputs"] = {k: _decode(v) for k, v in rec["inputs"].items()}
        rec["outputs"] = {k: _decode(v) for k, v in rec["outputs"].items()}
        if rec.get("outputs_bitenv"):
            rec["outputs_bitenv"] = {k: _decode(v) for k, v in rec["outputs_bitenv"].items()}
        _cache[name] = rec
    return _cache[name]


def toy_k2(p_msg=7, n=12, beta=21):
    """A toy set of the k = 2 shape (GLWE dimension 2 at N = 1024, one gadget level, two key bits per step): n small enough for
    the CPU oracle to bootstrap in milliseconds, real N so that the kernels are the shipped ones (k_blind_rotate_pairs_k2 and
    the whole-CU k = 2 shape, ct_words = 2049 through k_lincomb and the level calls)."""
    from tfhe_fbs_map_amd import Params
    return Params(n=n, log_n_poly=10, k=2, l_bsk=1, beta_bsk=beta, t_ksk=8, gamma_ksk=2, p_msg=p_msg, sigma_lwe=1 << 8, sigma_glwe=4,
                  bsk_group=2)


def toy_k3(p_msg=7, n=12, beta=18):
    """A toy set of the k = 3 shape the default 128-bit sets for p <= 8 run on (GLWE dimension 3 at N = 512, one gadget level, two key
    bits per step: k_blind_rotate_glwe, ciphertexts of 3 N + 1 = 1537 words, accumulator rows of 4 N)."""
    from tfhe_fbs_map_amd import Params
    return Params(n=n, log_n_poly=9, k=3, l_bsk=1, beta_bsk=beta, t_ksk=8, gamma_ksk=2, p_msg=p_msg, sigma_lwe=1 << 8, sigma_glwe=4,
                  bsk_group=2)


def toy_glwe(k, p_msg=7, n=12):
    """toy_k2 / toy_k3 by GLWE dimension"""
    return toy_k2(p_msg, n) if k == 2 else toy_k3(p_msg, n)


def subsample(rec, T):
    """First T samples of the harness inputs and of the expected outputs."""
    ins = {k: v[:T] for k, v in rec["inputs"].items()}
    outs = {k: (v if isinstance(v, int) else v[:T]) for k, v in rec["outputs"].items()}
    return ins, outs


def assert_outputs_equal(got, expected):
    assert set(got.keys()) == set(expected.keys())
    for k, e in expected.items():
        g = got[k]
        if isinstance(e, int):
            assert isinstance(g, (int, np.integer)) or np.ndim(g) == 0, k
            assert int(g) == e, k
        else:
            assert np.array_equal(np.asarray(g).reshape(-1), e), "output %s differs" % k


def oracle_eval_program(orc, ops, outputs, in_cts, fuse=False):
    """Run a program (oracle.lut_oracle.read_fbs form) on ciphertexts with the C oracle.
    in_cts: {input name: [T][ct_words]}.  Returns {wire name: [T][ct_words]} for all wires.
    fuse: a wire that two or more bootstraps read is rotated once and every table cut out of that accumulator
    (oracle bootstrap_multi) -- what a program loaded with FBS_LOAD_FUSE_TABLES computes."""
    wires = dict(in_cts)
    T = len(next(iter(in_cts.values()))) if in_cts else 1
    readers = {}
    for op in ops:
        if op[0] == "boot":
            readers.setdefault(op[2], []).append(op)
    for op in ops:
        if op[0] == "lin":
            _, name, terms, const = op
            out = np.empty((T, orc.ctw), np.uint64)
            for s in range(T):
                out[s] = orc.lincomb([wires[src][s] for _, src in terms], [c for c, _ in terms], const)
            wires[name] = out
        elif fuse and len(readers[op[2]]) >= 2:
            if op[1] in wires:
                continue                                        # computed with the first gate of its source
            group = readers[op[2]]
            res = orc.bootstrap_multi(wires[op[2]], [g[3] for g in group])
            for g, r in zip(group, res):
                wires[g[1]] = r
        else:
            _, name, src, table = op
            res, _ = orc.bootstrap_batch(wires[src], [table], None)
            wires[name] = res
    return wires


# ---- kernel selection: which parameter set, batch size and knobs reach each instantiation of fbs_kernel_catalog ----
CUS = 256

# what the selection derives DIG from (csrc/fbs_select.cpp): l > 5 -> 0; l = 1 -> 4; l = 2 -> 4 + by_beta; else by_beta,
# by_beta = 3 for beta <= 7, 2 for beta <= 9, 1 otherwise
GADGET_OF_DIG = {0: (6, 4), 1: (3, 10), 2: (3, 8), 3: (3, 7), 4: (1, 20), 5: (2, 10), 6: (2, 8), 7: (2, 7)}


def recipe(name):
    """-> dict(log_n, l, beta, group, count, knobs) that makes the launcher pick `name`"""
    m = re.fullmatch(r"k_blind_rotate<(\d+),(\d+),(\d+),(\d+)(,false)?>", name)
    if m:
        L, LL, dig, fpw = (int(m.group(i)) for i in range(1, 5))
        l, beta = GADGET_OF_DIG[dig]
        main_ll = 6 if L <= 10 else L - 4
        knobs = {}
        if m.group(5):                                    # no priority hand-over: two-level N = 1024 sets beyond two rounds
            count = 8 * CUS + 60
        elif fpw == 4:                                    # whole rounds of the benchmark shape
            count = 4 * CUS
        elif fpw == 2:                                    # between one and two bootstraps per CU, two per workgroup
            count, knobs = CUS + 44, dict(br_cu_kernel=0)
        elif LL != main_ll:                               # N = 1024 / 2048 on four waves per polynomial, generic kernel
            count, knobs = 40, dict(br_cu_kernel=0)
        elif L in (10, 11):                               # main shape: more than two bootstraps per CU (below, the one-per-CU shapes)
            count = 2 * CUS + 88
        else:
            count = 40
        return dict(log_n=L, l=l, beta=beta, group=1, count=count, knobs=knobs)
    m = re.fullmatch(r"k_blind_rotate_pairs<(\d+),(\d+),(\d+)>", name)
    if m:
        L, dig = int(m.group(1)), int(m.group(3))
        l, beta = {4: (1, 20), 3: (2, 7), 0: (2, 10)}[dig]
        # (N = 2048 with two levels goes to the whole-CU kernel whatever the size: the A/B switch brings the generic one back)
        return dict(log_n=L, l=l, beta=beta, group=2, count=CUS + 40 if (L, l) == (11, 1) else 40,
                    knobs=dict(br_cu_kernel=0) if (L, l) == (11, 2) else {})
    if name == "k_blind_rotate_cu_pairs<11,1>":           # two key bits per step on a whole CU: up to one bootstrap per CU
        return dict(log_n=11, l=1, beta=20, group=2, count=CUS - 9, knobs={})
    if name == "k_blind_rotate_cu_pairs<11,2>":           # ... with two gadget levels: every launch, round after round
        return dict(log_n=11, l=2, beta=10, group=2, count=CUS + 21, knobs={})
    m = re.fullmatch(r"k_blind_rotate_pairs_k2<10,(\d)>", name)
    if m:                                                 # GLWE dimension k = 2 on three waves per bootstrap: one, two or four bootstraps per
        fpw = int(m.group(1))                             # workgroup, a ragged last one (up to three per CU the launcher prefers the shape below)
        return dict(log_n=10, l=1, beta=20, group=2, k=2, count={1: 41, 2: CUS + 41, 4: 3 * CUS + 41}[fpw],
                    knobs={} if fpw == 4 else dict(br_k2_shape=3))
    if name == "k_blind_rotate_cu_k2":                    # ... one bootstrap on the twelve waves of a workgroup: two rounds, the second partial
        return dict(log_n=10, l=1, beta=20, group=2, k=2, count=CUS + 41, knobs={})
    m = re.fullmatch(r"k_blind_rotate_glwe<(\d+),(\d),(\d),(\d)>", name)
    if m:                                                 # every other GLWE dimension / size / depth: k + 1 waves per bootstrap, two gadget levels
        L, k1, group, fpw = (int(m.group(i)) for i in (1, 2, 3, 4))   # (k = 2 at N = 1024 with one level and two key bits per step has its own kernels);
        # one bootstrap per workgroup up to one per CU, two up to two, the throughput shape beyond: a ragged last workgroup each time
        return dict(log_n=L, l=2, beta=8, group=group, k=k1 - 1, count={1: 41, 2: CUS + 41}.get(fpw, 2 * CUS + 41), knobs={})
    m = re.fullmatch(r"k_blind_rotate_cu<(\d+),(\d+),(\d+)(,lean)?>", name)
    if m:
        L, nl, first = int(m.group(1)), int(m.group(2)), int(m.group(3))
        beta = {2: 7, 1: 9, 0: 10}[first]
        if nl * beta > 30:
            beta = 30 // nl
        if m.group(4):                                    # two workgroups per CU: between one and two bootstraps per CU
            return dict(log_n=L, l=nl, beta=beta, group=1, count=CUS + 70, knobs=dict(br_cu_lean=1))
        return dict(log_n=L, l=nl, beta=beta, group=1, count=CUS + 3 if nl == 3 or (L, nl) == (11, 2) else 40, knobs=dict(br_cu_lean=0))
    ks = {"k_ks_gemm<2,2> (int8 MFMA)": (40, {}), "k_keyswitch_fp<8,2,8>": (70, dict(ks_mfma=0)),
          "k_keyswitch_lanes<8,2,8>": (70, dict(ks_mfma=0, ks_fp=0)), "k_keyswitch_lanes<8,1,4>": (40, dict(ks_mfma=0)),
          "k_keyswitch<8>": (9, dict(ks_mfma=0))}
    if name in ks:
        count, knobs = ks[name]
        return dict(log_n=9, l=2, beta=8, group=1, count=count, knobs=knobs)
    return None
