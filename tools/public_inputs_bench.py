"""Public-key inputs (include/fbs_exec.h, "public-key inputs"; csrc/fbs_public.hip, k_expand_public) at the shape of adder128's
inputs at its default set: 256 rows of T = 1000 samples, GLWE dimension 2 at N = 1024 -- 256 000 ciphertexts of 2 049 words, 4.2 GB,
from 250 GLWE samples, 6.1 MB.  The context holds no key: the expansion needs none.  Three modes, one JSON line each.

    wall     fbs_state_put_public of the 250 samples against fbs_state_put of the same rows as full ciphertexts (what a server has
             to do with ciphertexts that were expanded elsewhere), alternated `--reps` times: wall time of each call (it ends in a
             device synchronise), the bytes each moves across the bus, and the host encryption rate on this CPU, for information
    kernel   `--launches` launches of one expansion kernel on device buffers, each between two device events: `--kernel public`
             is k_expand_public (fbs_pub_expand_dev), `--kernel seeded` is k_expand_seeded (fbs_expand_seeded_dev) at the same count
             -- the same stores plus the ChaCha20 blocks of the masks, and the yardstick: it exists on the commit before this one,
             whose library `--lib` names.  Talks to the library through ctypes alone, so it runs against either.  Run it under
             `rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/public_inputs_bench.py --mode kernel ...`
             for the kernel's own time
    trace    the median, minimum and maximum of every kernel in a rocprofv3 kernel-trace CSV (`--csv`), warm-up launches included

    python tools/public_inputs_bench.py --mode wall [--rows 256] [--T 1000] [--reps 5] [--out profiles/public_inputs/wall.jsonl]
"""
import argparse
import csv
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
Q = (1 << 46) - 62 * (1 << 13) + 1


def shape_params(n=12):
    """GLWE dimension 2 at N = 1024, as the default 128-bit sets for p <= 15; n does not enter the expansion and stays small, so that
    the seeded yardstick's key generation takes no time"""
    from tfhe_fbs_map_amd import Params
    return Params(n=n, log_n_poly=10, k=2, l_bsk=1, beta_bsk=21, t_ksk=8, gamma_ksk=2, p_msg=15, sigma_lwe=1 << 8, sigma_glwe=4, bsk_group=2)


def emit(record, out):
    line = json.dumps(record)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs)


def wall(args):
    from tfhe_fbs_map_amd import Context, _public_native as pub
    prm = shape_params()
    rows, T, N = args.rows, args.T, prm.N
    count = rows * T
    rng = np.random.default_rng(0)
    mask_key, sk = bytes(rng.integers(0, 256, 32, dtype=np.uint8)), rng.integers(0, 2, prm.k * N).astype(np.uint64)
    enc = pub.Encryptor(prm, mask_key, pub.keygen(prm, mask_key, sk, bytes(32)), bytes(range(32)))
    msgs = rng.integers(0, 2, count)
    t0 = time.perf_counter()
    glwe, _ = enc.encrypt(msgs)
    t_enc = time.perf_counter() - t0
    t0 = time.perf_counter()
    cts = pub.expand(prm, glwe, count)
    t_expand = time.perf_counter() - t0
    ctx = Context(prm, seed=1, keygen=False)
    state = ctx.state(rows, T)
    for _ in range(2):                                            # warm-up: the staging, the kernel's code object
        state.put_public(glwe)
        state.put(cts[:T].reshape(1, T, -1))
    walls = {"put_public": [], "put": []}
    for _ in range(args.reps):
        t0 = time.perf_counter()
        state.put_public(glwe)
        walls["put_public"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        state.put(cts.reshape(rows, T, -1))
        walls["put"].append(time.perf_counter() - t0)
    state.put_public(glwe)
    same = all(np.array_equal(state.fetch(row0=r, rows=1)[0], cts[r * T:(r + 1) * T]) for r in (0, rows // 2, rows - 1))
    assert same, "the device expansion differs from the host's"
    emit(dict(mode="wall", device=ctx.device_info, rows=rows, T=T, k=prm.k, N=N, ciphertexts=count, samples=int(glwe.shape[0]),
              bytes_put_public=int(glwe.nbytes), bytes_put=int(cts.nbytes),
              put_public_s=dict(median=statistics.median(walls["put_public"]), all=walls["put_public"], spread=spread(walls["put_public"])),
              put_s=dict(median=statistics.median(walls["put"]), all=walls["put"], spread=spread(walls["put"])),
              host_encrypt_samples_per_s=glwe.shape[0] / t_enc, host_encrypt_s=t_enc, host_expand_s=t_expand, label=args.label), args.out)


class _Params(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ("n", "log_n_poly", "k", "l_bsk", "beta_bsk", "t_ksk", "gamma_ksk", "p_msg")] + \
               [("sigma_lwe", C.c_uint64), ("sigma_glwe", C.c_uint64), ("bsk_group", C.c_uint32), ("sampler", C.c_uint32)]


def kernel(args):
    import torch                      # (first: its HIP runtime is the one the process uses)
    from dataclasses import asdict
    prm = shape_params()
    lib = C.CDLL(args.lib or os.path.join(ROOT, "tfhe_fbs_map_amd", "libfbsexec.so"))
    vp, sz, u64 = C.c_void_p, C.c_size_t, C.c_uint64
    lib.fbs_last_error.restype = C.c_char_p
    lib.fbs_last_error.argtypes = [vp]
    lib.fbs_ctx_create.argtypes = [C.POINTER(_Params), u64, C.c_int, C.POINTER(vp)]
    lib.fbs_ctx_destroy.argtypes = [vp]
    lib.fbs_keygen_seeded.argtypes = [vp]
    lib.fbs_sync.argtypes = [vp, vp]
    lib.fbs_expand_seeded_dev.argtypes = [vp, vp, sz, u64, vp, vp]
    h = vp()
    cp = _Params(**asdict(prm))

    def check(rc, handle=None):
        if rc:
            raise RuntimeError("%d: %s" % (rc, lib.fbs_last_error(handle).decode()))
    check(lib.fbs_ctx_create(C.byref(cp), 1, 0, C.byref(h)))
    count, N, ctw = args.rows * args.T, prm.N, prm.ct_words
    dev = torch.device("cuda", 0)
    d_cts = torch.empty(count * ctw, dtype=torch.int64, device=dev)
    if args.kernel == "seeded":
        check(lib.fbs_keygen_seeded(h), h)                         # (the entry asks for keys; the kernel reads the mask key only)
        d_src = torch.zeros(count, dtype=torch.int64, device=dev)
        launch = lambda: lib.fbs_expand_seeded_dev(h, d_src.data_ptr(), count, 7, d_cts.data_ptr(), None)      # noqa: E731
        bytes_read = count * 8
    else:
        lib.fbs_pub_expand_dev.argtypes = [vp, vp, sz, vp, vp]
        G = -(-count // N)
        d_src = torch.randint(0, Q, (G * (prm.k + 1) * N,), dtype=torch.int64, device=dev)
        launch = lambda: lib.fbs_pub_expand_dev(h, d_src.data_ptr(), count, d_cts.data_ptr(), None)            # noqa: E731
        bytes_read = G * (prm.k + 1) * N * 8
    for _ in range(3):
        check(launch(), h)
    check(lib.fbs_sync(h, None), h)
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.launches):                                 # the context's stream is a blocking one: ordered with these events
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(launch(), h)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    written = count * ctw * 8
    med = statistics.median(ms)
    emit(dict(mode="kernel", kernel=args.kernel, lib=args.lib or "this tree", rows=args.rows, T=args.T, k=prm.k, N=N, ciphertexts=count,
              launches=args.launches, event_ms=dict(median=med, min=min(ms), max=max(ms)), bytes_written=written, bytes_read=bytes_read,
              written_bytes_per_s_by_events=written / (med * 1e-3), label=args.label), args.out)
    lib.fbs_ctx_destroy(h)


def trace(args):
    per = {}
    with open(args.csv) as f:
        for row in csv.DictReader(f):
            name = row.get("Kernel_Name") or row.get("Name")
            if name is None:
                continue
            per.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6)
    written = args.rows * args.T * (shape_params().ct_words) * 8
    for name, ms in sorted(per.items()):
        if "expand" not in name:
            continue
        med = statistics.median(ms)
        emit(dict(mode="trace", csv=os.path.basename(args.csv), kernel_name=name, launches=len(ms),
                  kernel_ms=dict(median=med, min=min(ms), max=max(ms)), written_bytes_per_s=written / (med * 1e-3), label=args.label), args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("wall", "kernel", "trace"), default="wall")
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=25)
    ap.add_argument("--kernel", choices=("public", "seeded"), default="public")
    ap.add_argument("--lib", default=None, help="the libfbsexec.so to load in kernel mode (default: this tree's)")
    ap.add_argument("--csv", default=None, help="trace mode: a rocprofv3 kernel-trace CSV")
    ap.add_argument("--label", default="", help="a word for the record, e.g. which commit ran")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    {"wall": wall, "kernel": kernel, "trace": trace}[args.mode](args)


if __name__ == "__main__":
    main()
