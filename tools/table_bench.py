#!/usr/bin/env python3
"""What a resident encrypted table costs on the GPU, at the default (p, norm2) = (15, 70) set (include/fbs_exec.h, "encrypted tables").

    python3 tools/table_bench.py [--T 1000] [--reps 3] > profiles/tables/table_T1000.jsonl

T samples, each with a 7-entry table (spread 2) of its own in one `DeviceTable`: the time of fbs_table_create (one mapped fold of T
tables), fbs_table_read, fbs_table_write in add mode and in set mode, beside fbs_bootstrap_batch_dev of T ciphertexts through the
identity table (the unit: one bootstrap).  Medians of --reps timed calls after one warm-up, host clock around a synchronised call;
every write of the timed runs adds 0 or sets the value already there, so the tables decrypt to the same entries at the end, which is
checked.  One JSON line per figure.  `Server.table` and `ResidentTable` above these entries are not timed."""
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
    from tfhe_fbs_map_amd import Context
    from tfhe_fbs_map_amd.params import choose_params, fold_choice
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    prm = choose_params(15, 70, glwe_dims=(1, 2, 3))
    p, T, spread = prm.p_msg, a.T, 2
    length = p // spread
    ctx = Context(prm, seed=7, keygen=False)
    ctx.tune(keys_on_device=1)
    ctx.keygen_seeded()
    t_f, gamma_f = fold_choice(prm, 70)
    ctx.fold_keygen(t_f, gamma_f)
    rng = np.random.default_rng(1)
    entries = rng.integers(0, p, (length, T))
    which = rng.integers(0, length, T)
    rows = ctx.state(length, T).put(ctx.encrypt(entries.reshape(-1), nonce0=1).reshape(length, T, prm.ct_words))
    # row 0: the index (spread * i), row 1: zeros (what the timed adds add), row 2: the entries the index names (what the sets set)
    iv = ctx.state(3, T).put(ctx.encrypt(np.concatenate([spread * which, np.zeros(T, np.int64), entries[which, np.arange(T)]]), nonce0=1 << 20)
                            .reshape(3, T, prm.ct_words))
    d_in = torch.from_numpy(np.ascontiguousarray(iv.fetch()[0]).view(np.int64)).cuda()
    d_out = torch.zeros((T, prm.ct_words), dtype=torch.int64, device="cuda")
    tv = ctx.tvset([list(range(p))])
    torch.cuda.synchronize()
    common = dict(T=T, p=p, N=prm.N, k=prm.k, n=prm.n, entries=length, spread=spread, fold_key=[t_f, gamma_f], reps=a.reps, device=ctx.device_info)

    def emit(name, seconds, runs, **more):
        print(json.dumps(dict(figure=name, seconds=seconds, runs=runs, in_bootstraps_per_table=seconds / boot, **more, **common)), flush=True)

    boot, runs = timed(ctx, a.reps, lambda: ctx.bootstrap_batch_dev(tv, d_in.data_ptr(), 0, T, d_out.data_ptr()))
    emit("bootstrap_batch_dev of T ciphertexts (the unit)", boot, runs)
    made = []

    def create():
        for old in made:
            old.close()
        made[:] = [ctx.table(rows, np.arange(length, dtype=np.uint32)[None], spread)]
    t, runs = timed(ctx, a.reps, create)
    emit("table_create: T tables of %d entries" % length, t, runs)
    tab = made[0]
    out = ctx.state(1, T)
    t, runs = timed(ctx, a.reps, lambda: tab.read(iv, 0, out=out))
    ok = bool(np.array_equal(ctx.decrypt(out.fetch())[0], entries[which, np.arange(T)]))
    emit("table_read: T reads, a table each", t, runs, decrypt_ok=ok)
    t, runs = timed(ctx, a.reps, lambda: tab.write(iv, 0, iv, [1], mode=tab.ADD))
    emit("table_write add: T adds, a table each", t, runs)
    t, runs = timed(ctx, a.reps, lambda: tab.write(iv, 0, iv, [2], mode=tab.SET, identity=tv))
    tab.read(iv, 0, out=out)
    ok = bool(np.array_equal(ctx.decrypt(out.fetch())[0], entries[which, np.arange(T)]))
    emit("table_write set: T sets, a table each", t, runs, decrypt_ok_after_the_writes=ok, writes=tab.stat("writes"),
         table_scratch_words=ctx.stat("table_scratch_words"))
    ctx.close()


if __name__ == "__main__":
    main()
