"""Folded state (include/fbs_exec.h, "folded state"; tfhe_fbs_map_amd/split.py) measured on one box:

  (a) adder128 (129 outputs, its default 128-bit set) at T samples, outputs resident: `fold()` to the host, `fold(device=True)`,
      `restore()` of either, beside `fetch(compact=True)` and the full `fetch()`, ALTERNATED `--reps` times; bytes held per bit.
  (b) the adder8 accumulator at T samples over `--hops` hops, server seconds per hop with its state resident, handed on as compact
      outputs, and folded on the card after every hop and unfolded by the next (the rows are freed in between), alternated too.
  (c) the front kernel alone (fbs_debug_fold_front_dev) on the (a) state's ciphertexts, timed with events on one stream beside a
      device-to-device copy of the same bytes: GB/s of ciphertext read.

    python tools/folded_state_bench.py [--T 1000] [--hops 8] [--reps 5] [--out profiles/folded_state/bench_T1000.jsonl]

One JSON line per figure.  The decrypted outputs of every path are checked equal."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _env(name):
    from tests.helpers import load_fixture
    from tfhe_fbs_map_amd import parse_fbs
    rec = load_fixture(name)
    return parse_fbs(rec["fbs"], inputs=rec["program_inputs"])


def _timed(server, fn):
    server.ctx.sync()
    t0 = time.perf_counter()
    out = fn()
    server.ctx.sync()
    return time.perf_counter() - t0, out


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def bench_outputs(args, emit):
    import torch
    from tfhe_fbs_map_amd import Client, ExecConfig, Server
    env = _env("adder128__search_p15")
    t0 = time.perf_counter()
    client = Client(env, ExecConfig(seed=1), folding=True)
    keygen_s = time.perf_counter() - t0
    server = Server(client.server_key())
    prm, key = client.params, client.server_key()
    rng = np.random.default_rng(0)
    ins = {n: rng.integers(0, 2, args.T) for n in env.lower()["input_names"]}
    res = server.run(env, client.encrypt(ins), resident=True)
    n_out = len(res.output_names)
    paths = dict(fold_host=lambda: res.fold(), fold_device=lambda: res.fold(device=True), fetch_compact=lambda: res.fetch(compact=True),
                 fetch_full=lambda: res.fetch())
    walls, outs = {p: [] for p in paths}, {}
    for p in paths:                                                     # warm-up: scratch, kernels
        paths[p]()
    for _ in range(args.reps):
        for p in paths:
            dt, outs[p] = _timed(server, paths[p])
            walls[p].append(dt)
    want = client.decrypt(outs["fetch_full"])
    for p in ("fold_host", "fold_device", "fetch_compact"):
        _same(client.decrypt(outs[p]), want)
    restores = dict(restore_host=outs["fold_host"], restore_device=outs["fold_device"], restore_full=outs["fetch_full"])
    for p, src in restores.items():
        walls[p] = []
        server.restore(src).close()
    for _ in range(args.reps):
        for p, src in restores.items():
            dt, back = _timed(server, lambda: server.restore(src))
            walls[p].append(dt)
            if p != "restore_full" and len(walls[p]) == 1:
                _same(client.decrypt(back.fetch()), want)
            back.close()
    bits = n_out * args.T
    held = dict(fold_host=outs["fold_host"].words.nbytes, fold_device=outs["fold_device"].words.numel() * 8,
                fetch_compact=outs["fetch_compact"].words.nbytes, fetch_full=outs["fetch_full"].cts.nbytes)
    common = dict(fixture="adder128__search_p15", T=args.T, k=prm.k, N=prm.N, n=prm.n, p=prm.p_msg, n_outputs=n_out,
                  folding=list(client.folding), fold_factor=key.fold_factor, fold_key_bytes=int(key.fold_bodies.nbytes), keygen_s=round(keygen_s, 3))
    for p in walls:
        emit(dict(common, part="outputs", path=p, s_median=float(np.median(walls[p])), s_all=[round(w, 5) for w in walls[p]],
                  bytes_held=held.get(p), bytes_per_bit=None if p not in held else held[p] / bits))
    # (c) the front kernel alone, on the state's own ciphertexts: one pass of 8192 and the whole state in passes, against a copy
    ctx, st = server.ctx, res.state
    count = n_out * args.T
    cols = -(-count // prm.N) * prm.N
    D = prm.k * prm.N
    d_cts = torch.empty(count * (D + 1), dtype=torch.int64, device="cuda")
    d_cts.copy_(torch.from_numpy(st.fetch().reshape(-1).view(np.int64)))
    d_f = torch.empty((D + 2) * cols, dtype=torch.int32, device="cuda")
    d_copy = torch.empty_like(d_cts)
    stream = torch.cuda.current_stream().cuda_stream
    times = {"front": [], "copy": []}
    for rep in range(args.reps + 1):
        for what in times:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            if what == "front":
                ctx.debug_fold_front_dev(d_cts.data_ptr(), count, cols, key.fold_levels * key.fold_base_bits, d_f.data_ptr(), stream)
            else:
                d_copy.copy_(d_cts)
            b.record()
            torch.cuda.synchronize()
            if rep:
                times[what].append(a.elapsed_time(b) * 1e-3)
    read = count * (D + 1) * 8
    for what, ts in times.items():
        moved = read + ((D + 2) * cols * 4 if what == "front" else read)
        emit(dict(common, part="front_kernel", path=what, s_median=float(np.median(ts)), s_all=[round(t, 6) for t in ts], bytes_read=read,
                  bytes_moved=moved, read_GBps=read / float(np.median(ts)) / 1e9, moved_GBps=moved / float(np.median(ts)) / 1e9))
    res.close()
    server.ctx.close()
    client.ctx.close()


def bench_accumulator(args, emit):
    from tfhe_fbs_map_amd import Client, ExecConfig, Server
    env = _env("adder8__search_p15")
    client = Client(env, ExecConfig(seed=1), programs=[env], folding=True)
    server = Server(client.server_key())
    prm = client.params
    T, rng = args.T, np.random.default_rng(1)
    rename = {f"a{i}": f"s{i}" for i in range(8)}
    b_names = [f"b{i}" for i in range(8)]
    first = {**{f"a{i}": rng.integers(0, 2, T) for i in range(8)}, **{n: rng.integers(0, 2, T) for n in b_names}}
    fresh = [client.encrypt({n: rng.integers(0, 2, T) for n in b_names}, names=b_names) for _ in range(args.hops)]

    def chain(link):
        acc = server.run(env, client.encrypt(first, nonce0=1), resident=True)
        state = acc if link == "resident" else acc.fetch(compact=True) if link == "compact" else acc.fold(device=True)
        if link != "resident":
            acc.close()
        server.ctx.sync()
        t0 = time.perf_counter()
        for hop in range(args.hops):
            if link == "compact":
                state = server.run_chain(env, [state, fresh[hop]], rename=rename, compact=True)
                continue
            nxt = server.run_chain(env, [state, fresh[hop]], rename=rename, resident=True)
            if link == "resident":
                state.close()
                state = nxt
            else:
                state = nxt.fold(device=True)
                nxt.close()
        server.ctx.sync()
        dt = (time.perf_counter() - t0) / args.hops
        out = client.decrypt(state.fetch() if link == "resident" else state)
        if link == "resident":
            state.close()
        return dt, out

    links = ("resident", "compact", "folded")
    for link in links:
        chain(link)
    walls, outs = {l: [] for l in links}, {}
    for _ in range(args.reps):
        for link in links:
            dt, outs[link] = chain(link)
            walls[link].append(dt)
    _same(outs["compact"], outs["resident"])
    _same(outs["folded"], outs["resident"])
    per_bit = dict(resident=prm.ct_words * 8, compact=None, folded=-(-9 * T // prm.N) * (prm.k + 1) * prm.N * 8 / (9 * T))
    for link in links:
        emit(dict(part="accumulator", fixture="adder8__search_p15", link=link, T=T, hops=args.hops, k=prm.k, N=prm.N, n=prm.n, p=prm.p_msg,
                  folding=list(client.folding), s_per_hop_median=float(np.median(walls[link])), s_per_hop_all=[round(w, 5) for w in walls[link]],
                  state_bytes_per_bit=per_bit[link]))
    server.ctx.close()
    client.ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--hops", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="outputs,accumulator")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)
        if args.out:                                                    # (written as it goes: a run cut short keeps what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                for ln in lines:
                    f.write(json.dumps(ln) + "\n")

    if "outputs" in args.only:
        bench_outputs(args, emit)
    if "accumulator" in args.only:
        bench_accumulator(args, emit)


if __name__ == "__main__":
    main()
