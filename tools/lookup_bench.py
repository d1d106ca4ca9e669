#!/usr/bin/env python3
"""What an encrypted-index read costs on the GPU, at the default (p, norm2) = (15, 70) set (include/fbs_exec.h, "encrypted-index reads").

    python3 tools/lookup_bench.py [--T 1000] [--reps 3] > profiles/lookup/lookup_T1000.jsonl

T queries, each an encrypted index digit reading a 15-entry table of encrypted values: the tables built by fbs_fold_mapped_dev (one
per query: T N fold positions over 15 T source ciphertexts; and one shared by every query), read by fbs_lookup_dev; beside them
fbs_bootstrap_batch_dev of T ciphertexts through the identity table (the unit: one bootstrap) and fbs_fold_dev of as many fold
positions as ONE pass of the mapped fold reads distinct ciphertexts for.  Medians of --reps timed calls after one warm-up, host clock
around a synchronised call.  One JSON line per figure.  The layers above these entries (resident tables, planes that share a key
switch, digit cascades) are not built and not measured."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(ctx, reps, call):
    call()
    ctx.sync()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ctx.sync()
        out.append(time.perf_counter() - t0)
    return statistics.median(out), out


def main():
    import torch
    from tfhe_fbs_map_amd import Context, _native as nat
    from tfhe_fbs_map_amd.params import choose_params, fold_choice
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    prm = choose_params(15, 70, glwe_dims=(1, 2, 3))
    p, N, T, ctw = prm.p_msg, prm.N, a.T, prm.ct_words
    ctx = Context(prm, seed=7, keygen=False)
    ctx.tune(keys_on_device=1)
    ctx.keygen_seeded()
    t_f, gamma_f = fold_choice(prm, 70)
    ctx.fold_keygen(t_f, gamma_f)
    rng = np.random.default_rng(1)
    entries = rng.integers(0, p, (T, p))
    index = rng.integers(0, p, T)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda()                     # noqa: E731
    d_src = torch.empty((T * p, ctw), dtype=torch.int64, device="cuda")
    d_idx = torch.empty((T, ctw), dtype=torch.int64, device="cuda")
    d_e, d_i = dev(entries.reshape(-1)), dev(index)
    torch.cuda.synchronize()
    ctx.encrypt_dev(d_e.data_ptr(), T * p, d_src.data_ptr(), nonce0=1)
    ctx.encrypt_dev(d_i.data_ptr(), T, d_idx.data_ptr(), nonce0=1 << 20)
    ctx.sync()
    fmap = np.concatenate([nat.lookup_map(p, N, p, base=s * p) for s in range(T)])
    d_map = torch.from_numpy(fmap.view(np.int32)).cuda()
    d_tab = torch.zeros((T, prm.k + 1, N), dtype=torch.int64, device="cuda")
    d_out = torch.zeros((T, ctw), dtype=torch.int64, device="cuda")
    d_zero = torch.zeros(T, dtype=torch.int32, device="cuda")
    tv = ctx.tvset([list(range(p))])
    torch.cuda.synchronize()
    common = dict(T=T, p=p, N=N, k=prm.k, n=prm.n, fold_key=[t_f, gamma_f], reps=a.reps, device=ctx.device_info)

    def emit(name, seconds, runs, **more):
        print(json.dumps(dict(figure=name, seconds=seconds, runs=runs, **more, **common)), flush=True)

    boot, runs = timed(ctx, a.reps, lambda: ctx.bootstrap_batch_dev(tv, d_idx.data_ptr(), 0, T, d_out.data_ptr()))
    emit("bootstrap_batch_dev of T ciphertexts (the unit)", boot, runs)
    build, runs = timed(ctx, a.reps, lambda: ctx.fold_mapped_dev(d_src.data_ptr(), T * p, d_map.data_ptr(), T * N, d_tab.data_ptr()))
    emit("fold_mapped_dev: T tables of p entries", build, runs, in_bootstraps_per_table=build / boot)
    read, runs = timed(ctx, a.reps, lambda: ctx.lookup_dev(d_tab.data_ptr(), T, 0, d_idx.data_ptr(), T, d_out.data_ptr()))
    got = ctx.decrypt(d_out.cpu().numpy().view(np.uint64))
    emit("lookup_dev: T reads, a table each", read, runs, in_bootstraps_per_read=read / boot, decrypt_ok=bool(np.array_equal(got, entries[np.arange(T), index])))
    one, runs = timed(ctx, a.reps, lambda: ctx.fold_mapped_dev(d_src.data_ptr(), p, d_map.data_ptr(), N, d_tab.data_ptr()))
    emit("fold_mapped_dev: one shared table", one, runs)
    shared, runs = timed(ctx, a.reps, lambda: ctx.lookup_dev(d_tab.data_ptr(), 1, d_zero.data_ptr(), d_idx.data_ptr(), T, d_out.data_ptr()))
    got = ctx.decrypt(d_out.cpu().numpy().view(np.uint64))
    emit("lookup_dev: T reads of the shared table", shared, runs, in_bootstraps_per_read=shared / boot, decrypt_ok=bool(np.array_equal(got, entries[0, index])))
    # the plain fold of as many positions as the mapped fold has (T N), from a source array of 8192 ciphertexts a pass would hold
    cnt = min(T * p, 8192)
    d_w = torch.zeros((-(-cnt // N), prm.k + 1, N), dtype=torch.int64, device="cuda")
    plain, runs = timed(ctx, a.reps, lambda: ctx.fold_dev(d_src.data_ptr(), cnt, d_w.data_ptr()))
    emit("fold_dev of one pass of distinct ciphertexts", plain, runs, ciphertexts=cnt, passes_of_the_mapped_fold=-(-T * N // 8192),
         mapped_seconds_per_pass=build / -(-T * N // 8192))
    ctx.close()


if __name__ == "__main__":
    main()
