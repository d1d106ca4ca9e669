"""Chained evaluation (`Server.run_chain`, `fbs_eval_sources`): what keeping state on the server between programs costs.

(a) An accumulator: adder8__search_p15 with a <- the previous sum (s0..s7) and b <- fresh client inputs, over --hops hops at T
    samples, once with full links (`EncryptedOutputs`, kN + 1 words a bit), once with compact links (`CompactOutputs`, refreshed
    on the GPU) and once with resident links (`ResidentOutputs`: the state stays in device memory, nothing crosses the bus but
    the fresh inputs; the clock stops after the last hop has finished on the GPU).  Per link kind, one JSON line: bytes of state per hop, fresh-input bytes per hop, server seconds per hop (median of
    --reps chains, each the mean of its hops), and that the client decrypts the running sum after the last hop.
(b) One adder128__search_p15 hop through compact links (a <- s of an earlier `run_compact`, b fresh) next to the same program's
    own `run_compact` on fresh inputs: the refresh overhead (medians of --reps).
(c) adder128__search_p15 on fresh inputs three ways: `run` (full outputs to the host), `run_compact`, and `run(resident=True)` --
    timed to the end of the evaluation on the GPU -- followed by one `fetch(compact=True)`, timed on its own.

Both at the default 128-bit sets (`ExecConfig()`, one key for the chain: `Client(env, programs=[env])`).

    python tools/chain_bench.py [--T 1000] [--hops 32] [--reps 5] [--out profiles/chain/bench_T1000.jsonl]

The kernels' own times come from a separate run under `rocprofv3 --kernel-trace --stats -f csv`; `--trace <kernel_trace.csv>`
reads that run's trace and prints the refresh's share: every `k_compact_unpack` dispatch and the blind-rotation dispatches right
after it (the identity rotations of the refresh), against all other blind rotations of the run."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summarize_trace(path):
    """dispatches and total ms of the refresh (unpack + the rotations right after it) against the other blind rotations"""
    import csv
    with open(path) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    base = [r["Kernel_Name"].split("(")[0].split("<")[0].replace("void ", "").replace("fbs::", "").strip() for r in rows]
    ms = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows]
    groups = {g: [0, 0.0] for g in ("compact_unpack", "refresh_rotations", "other_rotations", "keyswitch_all")}
    after_unpack = False
    for b, t in zip(base, ms):
        if b == "k_compact_unpack":
            g, after_unpack = "compact_unpack", True
        elif b.startswith("k_blind_rotate"):
            g = "refresh_rotations" if after_unpack else "other_rotations"
        else:
            after_unpack = False
            g = "keyswitch_all" if b in ("k_ks_digits", "k_ks_gemm", "k_ks_gemm_finish", "k_keyswitch", "k_ms_body") else None
        if g:
            groups[g][0] += 1
            groups[g][1] += t
    return {g: dict(dispatches=v[0], ms=round(v[1], 3)) for g, v in groups.items()}


def _env(name):
    from tests.helpers import load_fixture
    from tfhe_fbs_map_amd import parse_fbs
    rec = load_fixture(name)
    return rec, parse_fbs(rec["fbs"], inputs=rec["program_inputs"])


def accumulator(T, hops, reps):
    from oracle import lut_oracle
    from tfhe_fbs_map_amd import Client, ExecConfig, Server
    rec, env = _env("adder8__search_p15")
    client = Client(env, ExecConfig(seed=1), programs=[env])
    server = Server(client.server_key())
    prm = client.params
    rename = {f"a{i}": f"s{i}" for i in range(8)}
    b_names = [f"b{i}" for i in range(8)]
    rng = np.random.default_rng(0)
    first = {n: rng.integers(0, 2, T) for n in env.lower()["input_names"]}
    stream = [{n: rng.integers(0, 2, T) for n in b_names} for _ in range(hops)]
    fresh = [client.encrypt(x, names=b_names) for x in stream]
    clear = lut_oracle.eval_fbs_text(rec["fbs"], first)
    for x in stream:
        clear = lut_oracle.eval_fbs_text(rec["fbs"], {**{f"a{i}": np.broadcast_to(clear[f"s{i}"], (T,)) for i in range(8)}, **x})
    lines = []
    for link in ("full", "compact", "resident"):
        compact, resident = link == "compact", link == "resident"
        start = client.encrypt(first)

        def begin():
            return server.run_compact(env, start) if compact else server.run(env, start, resident=resident)
        warm = server.run_chain(env, [begin(), fresh[0]], rename=rename, compact=compact, resident=resident)   # warm-up: program load, scratch, identity table
        per_hop, state_bytes = [], 0
        for _ in range(reps):
            acc = begin()
            server.ctx.sync()
            t0 = time.perf_counter()
            for f in fresh:
                nxt = server.run_chain(env, [acc, f], rename=rename, compact=compact, resident=resident)
                if resident:
                    acc.close()          # (waits for the hop that reads it)
                acc = nxt
            server.ctx.sync()
            per_hop.append((time.perf_counter() - t0) / hops)
            # what crosses the bus per hop for the eight sum bits
            state_bytes = 0 if resident else int((acc.words if compact else acc.cts)[:8].nbytes)
        got = client.decrypt(acc.fetch() if resident else acc)
        ok = all(np.array_equal(np.broadcast_to(got[k], (T,)), np.broadcast_to(clear[k], (T,))) for k in clear)
        line = dict(bench="adder8_accumulator", link=link, T=T, hops=hops, k=prm.k, N=prm.N, n=prm.n, p=prm.p_msg,
                    bits=getattr(warm, "bits", None), state_bytes_per_hop=state_bytes,
                    state_bytes_per_bit=state_bytes // (8 * T), fresh_input_bytes_per_hop=int(fresh[0].bodies.nbytes),
                    server_s_per_hop_median=float(np.median(per_hop)), server_s_per_hop_all=[round(x, 5) for x in per_hop],
                    decrypts_running_sum=bool(ok))
        print(json.dumps(line), flush=True)
        lines.append(line)
    server.ctx.close()
    client.ctx.close()
    return lines


def adder128_hop(T, reps):
    from tfhe_fbs_map_amd import Client, ExecConfig, Server
    rec, env = _env("adder128__search_p15")
    client = Client(env, ExecConfig(seed=1), programs=[env])
    server = Server(client.server_key())
    prm = client.params
    names = env.lower()["input_names"]
    b_names = [n for n in names if n.startswith("b")]
    rename = {f"a{i}": f"s{i}" for i in range(len(names) - len(b_names))}
    rng = np.random.default_rng(0)
    start = client.encrypt({n: rng.integers(0, 2, T) for n in names})
    fresh = client.encrypt({n: rng.integers(0, 2, T) for n in b_names}, names=b_names)
    state = server.run_compact(env, start)
    server.run_chain(env, [state, fresh], rename=rename, compact=True)   # warm-up
    own, hop = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        server.run_compact(env, start)
        own.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        server.run_chain(env, [state, fresh], rename=rename, compact=True)
        hop.append(time.perf_counter() - t0)
    line = dict(bench="adder128_compact_hop", T=T, k=prm.k, N=prm.N, n=prm.n, p=prm.p_msg, bits=state.bits,
                linked_inputs=len(rename), refreshes=len(rename) * T,
                own_run_compact_s_median=float(np.median(own)), chain_hop_s_median=float(np.median(hop)),
                refresh_overhead_s=float(np.median(hop) - np.median(own)),
                own_all=[round(x, 4) for x in own], hop_all=[round(x, 4) for x in hop],
                state_bytes=int(state.words[:len(rename)].nbytes), full_state_bytes=len(rename) * T * prm.ct_words * 8)
    print(json.dumps(line), flush=True)
    server.ctx.close()
    client.ctx.close()
    return [line]


def adder128_outputs(T, reps):
    from tfhe_fbs_map_amd import Client, ExecConfig, Server
    rec, env = _env("adder128__search_p15")
    client = Client(env, ExecConfig(seed=1), programs=[env])
    server = Server(client.server_key())
    prm = client.params
    rng = np.random.default_rng(0)
    start = client.encrypt({n: rng.integers(0, 2, T) for n in env.lower()["input_names"]})
    want = client.decrypt(server.run_compact(env, start))   # (warm-up too)
    server.run(env, start)
    with server.run(env, start, resident=True) as warm:
        got = client.decrypt(warm.fetch(compact=True))
    ok = all(np.array_equal(got[k], want[k]) for k in want)
    t = dict(run=[], run_compact=[], resident=[], fetch_compact=[])
    for _ in range(reps):
        for name, call in (("run", lambda: server.run(env, start)), ("run_compact", lambda: server.run_compact(env, start))):
            t0 = time.perf_counter()
            call()
            t[name].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        out = server.run(env, start, resident=True)
        server.ctx.sync()
        t["resident"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        words = out.fetch(compact=True)
        t["fetch_compact"].append(time.perf_counter() - t0)
        out.close()
    line = dict(bench="adder128_outputs", T=T, k=prm.k, N=prm.N, n=prm.n, p=prm.p_msg, bits=words.bits,
                full_output_bytes=len(words.output_names) * T * prm.ct_words * 8, compact_output_bytes=int(words.words.nbytes),
                resident_then_fetch_compact_decrypts_as_run_compact=bool(ok),
                **{k + "_s_median": float(np.median(v)) for k, v in t.items()}, **{k + "_all": [round(x, 4) for x in v] for k, v in t.items()})
    print(json.dumps(line), flush=True)
    server.ctx.close()
    client.ctx.close()
    return [line]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--hops", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=("accumulator", "adder128", "outputs"), default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", default=None, help="summarise this rocprofv3 kernel_trace.csv instead of running")
    args = ap.parse_args()
    if args.trace:
        print(json.dumps(summarize_trace(args.trace)))
        return
    lines = []
    if args.only in (None, "accumulator"):
        lines += accumulator(args.T, args.hops, args.reps)
    if args.only in (None, "adder128"):
        lines += adder128_hop(args.T, args.reps)
    if args.only in (None, "outputs"):
        lines += adder128_outputs(args.T, args.reps)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
