"""Sample-axis operations (`fbs_eval_resident_mapped`, `fbs_state_sum_groups`; `ResidentOutputs.samples` / `sum_groups`,
`Server.fold`): what they cost, at adder8's default 128-bit set (`Client(env, programs=[env])`).  Every figure is taken twice.

Wall-clock part (default), one JSON line each into <out-dir>/wall.jsonl:
(a) `sum_groups`: rows = 9, T = 4096, group = 8 over the outputs of one resident adder8 evaluation -- seconds per launch with the
    stream drained before and after a run of launches, and the bytes read per second that makes (rows T (D+1) 8 bytes a launch).
(b) adder8 fold at T = 1000: the sum of 1000 encrypted bytes.  `Server.run(resident=True)` of (x, 0), `Server.fold`, one compact
    fetch of the single result: wall seconds and the bytes that go back to the client.  Against the route there was before: `run_compact` of all
    1000 results (server seconds, bytes), which the client decrypts and adds itself.
(c) gather overhead: one resident adder8 hop at T = 1000 (a <- the state's s rows, b fresh), the state read through the identity
    index (`state.samples(arange(T))`) against the state read as it is: k_wire_load either way, with and without an index word.

Kernel part (`--kernels`, meant to run under `rocprofv3 --kernel-trace --stats -f csv`, a run of its own): the launches of (a), one
unmapped and one identity-mapped adder8 hop over the same T = 4096 state, and into <out-dir>/kernels_run.jsonl the bytes each of
the two state kernels read in that run (both kinds of hop load through k_wire_load: they are accounted for together).  `--stats <kernel_stats.csv>` then divides: <out-dir>/kernel_bandwidth.jsonl.

`--table` prints the README's table from the three files.

    python tools/sample_axis_bench.py [--out-dir profiles/sample_axis]
    rocprofv3 --kernel-trace --stats -f csv -d <dir> -- python tools/sample_axis_bench.py --kernels
    python tools/sample_axis_bench.py --stats <dir>/.../*_kernel_stats.csv
    python tools/sample_axis_bench.py --table"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

A_NAMES, B_NAMES = [f"a{i}" for i in range(8)], [f"b{i}" for i in range(8)]
A_FROM_S, B_FROM_S = {f"a{i}": f"s{i}" for i in range(8)}, {f"b{i}": f"s{i}" for i in range(8)}


def _setup():
    from tests.helpers import load_fixture
    from tfhe_fbs_map_amd import Client, ExecConfig, Server, parse_fbs
    rec = load_fixture("adder8__search_p15")
    env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
    client = Client(env, ExecConfig(seed=1), programs=[env])
    return env, client, Server(client.server_key())


def _bits(x, names):
    return {n: (np.asarray(x) >> i) & 1 for i, n in enumerate(names)}


def _numbers(client, x):
    """the client's inputs for (x, 0): the state a fold starts from is adder8's sum of them"""
    return client.encrypt({**_bits(x, A_NAMES), **_bits(np.zeros(len(x), np.int64), B_NAMES)})


def _value(out):
    return sum(np.asarray(out[f"s{i}"]).astype(np.int64) << i for i in range(8))


def _shape(prm):
    return dict(k=prm.k, N=prm.N, n=prm.n, p=prm.p_msg, ct_words=prm.ct_words)


def sum_groups_wall(client, server, env, T=4096, group=8, launches=20):
    rng = np.random.default_rng(0)
    lines = []
    with server.run(env, _numbers(client, rng.integers(0, 256, T)), resident=True) as state:
        out = state.state.sum_groups(group)          # warm-up; the destination of every timed launch
        read = state.state.rows * T * client.params.ct_words * 8
        for take in range(2):
            server.ctx.sync()
            t0 = time.perf_counter()
            for _ in range(launches):
                state.state.sum_groups(group, out=out)
            server.ctx.sync()
            s = (time.perf_counter() - t0) / launches
            lines.append(dict(bench="sum_groups_wall", take=take, rows=state.state.rows, T=T, group=group, launches=launches,
                              bytes_read_per_launch=read, s_per_launch=s, read_GB_per_s=read / s / 1e9, **_shape(client.params)))
        out.close()
    return lines


def fold_against_compact(client, server, env, T=1000):
    rng = np.random.default_rng(1)
    x = rng.integers(0, 256, T)
    inputs = _numbers(client, x)
    want = int(x.sum()) % 256
    with server.run(env, inputs, resident=True) as state:                                     # warm-up
        server.fold(env, state, A_FROM_S, B_FROM_S).close()
    server.run_compact(env, inputs)
    lines = []
    for take in range(2):
        server.ctx.sync()
        t0 = time.perf_counter()
        with server.run(env, inputs, resident=True) as state, server.fold(env, state, A_FROM_S, B_FROM_S) as total:
            back = total.fetch(compact=True)
        t_fold = time.perf_counter() - t0
        t0 = time.perf_counter()
        every = server.run_compact(env, inputs)
        t_all = time.perf_counter() - t0
        t0 = time.perf_counter()
        summed = int(_value(client.decrypt(every)).sum()) % 256
        t_client = time.perf_counter() - t0
        lines.append(dict(bench="adder8_fold", take=take, T=T, rounds=int(np.ceil(np.log2(T))),
                          fold_server_s=t_fold, fold_bytes_to_client=int(back.words.nbytes), fold_bits=int(back.bits),
                          fold_is_the_sum=bool(int(_value(client.decrypt(back))[0]) == want),
                          run_compact_server_s=t_all, run_compact_bytes_to_client=int(every.words.nbytes), run_compact_bits=int(every.bits),
                          client_decrypt_and_add_s=t_client, client_sum_is_the_sum=bool(summed == want), **_shape(client.params)))
    return lines


def _hops(client, server, env, T, reps, state):
    """seconds of one resident hop over `state`, unmapped and through the identity index, `reps` times each, alternating"""
    rng = np.random.default_rng(2)
    fresh = client.encrypt(_bits(rng.integers(0, 256, T), B_NAMES), names=B_NAMES)
    ident = np.arange(T, dtype=np.uint32)
    t = dict(unmapped=[], identity=[])
    for rep in range(reps + 1):                      # (the first pair is the warm-up)
        for name, src in (("unmapped", state), ("identity", state.samples(ident))):
            server.ctx.sync()
            t0 = time.perf_counter()
            out = server.run_chain(env, [src, fresh], rename=A_FROM_S, resident=True)
            server.ctx.sync()
            if rep:
                t[name].append(time.perf_counter() - t0)
            out.close()
    return t


def gather_overhead(client, server, env, T=1000):
    rng = np.random.default_rng(3)
    with server.run(env, _numbers(client, rng.integers(0, 256, T)), resident=True) as state:
        t = _hops(client, server, env, T, 2, state)
    return [dict(bench="adder8_hop_gather", T=T, linked_inputs=8, unmapped_hop_s=t["unmapped"], identity_index_hop_s=t["identity"],
                 overhead_s=[b - a for a, b in zip(t["unmapped"], t["identity"])], **_shape(client.params))]


def kernels_run(client, server, env, T=4096, group=8, launches=10):
    """what the profiler watches: `launches` group sums twice, and two hops of each kind over the same state"""
    rng = np.random.default_rng(0)
    ctw = client.params.ct_words
    with server.run(env, _numbers(client, rng.integers(0, 256, T)), resident=True) as state:
        out = state.state.sum_groups(group)
        for _ in range(2 * launches - 1):
            state.state.sum_groups(group, out=out)
        out.close()
        _hops(client, server, env, T, 1, state)      # two hops of each kind (one of them the warm-up)
    row = T * ctw * 8
    return [dict(bench="kernels_run", T=T, group=group, **_shape(client.params),
                 bytes_read={"k_state_sum_groups": 2 * launches * 9 * row, "k_wire_load": 4 * 8 * row},
                 bytes_written={"k_state_sum_groups": 2 * launches * 9 * row // group, "k_wire_load": 4 * 8 * row})]


def kernel_bandwidth(stats_csv, run_line):
    lines = []
    with open(stats_csv) as f:
        for r in csv.DictReader(f):
            name = r["Name"].split("(")[0].replace("fbs::", "").replace("void ", "").strip()
            if name in run_line["bytes_read"]:
                total = int(r["TotalDurationNs"])
                lines.append(dict(bench="kernel_bandwidth", kernel=name, calls=int(r["Calls"]), total_ns=total,
                                  min_ns=int(r["MinNs"]), max_ns=int(r["MaxNs"]),
                                  bytes_read=run_line["bytes_read"][name], bytes_written=run_line["bytes_written"][name],
                                  read_GB_per_s=run_line["bytes_read"][name] / total, T=run_line["T"], group=run_line["group"]))
    return lines


def _write(path, lines):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line), flush=True)


def _read(path):
    if not os.path.exists(path):
        return []
    with open(path) as f:
        return [json.loads(line) for line in f if line.strip()]


def table(out_dir):
    rows = ["| what | first take | second take |", "|---|---|---|"]
    wall, band = _read(os.path.join(out_dir, "wall.jsonl")), _read(os.path.join(out_dir, "kernel_bandwidth.jsonl"))
    sg = [x for x in wall if x["bench"] == "sum_groups_wall"]
    if sg:
        rows.append("| `sum_groups` rows 9, T 4096, group 8: wall s per launch (GB/s read) | " +
                    " | ".join("%.6f (%.0f)" % (x["s_per_launch"], x["read_GB_per_s"]) for x in sg) + " |")
    for x in band:
        rows.append("| `%s` under the profiler: %d calls, GB/s read over their total (fastest call ns, slowest) | %.0f (%d, %d) | -- |"
                    % (x["kernel"], x["calls"], x["read_GB_per_s"], x["min_ns"], x["max_ns"]))
    fold = [x for x in wall if x["bench"] == "adder8_fold"]
    if fold:
        rows.append("| adder8 fold of T = 1000, run + fold + compact fetch: server s | " + " | ".join("%.4f" % x["fold_server_s"] for x in fold) + " |")
        rows.append("| ... bytes to the client | " + " | ".join("%d" % x["fold_bytes_to_client"] for x in fold) + " |")
        rows.append("| `run_compact` of all 1000 results: server s | " + " | ".join("%.4f" % x["run_compact_server_s"] for x in fold) + " |")
        rows.append("| ... bytes to the client | " + " | ".join("%d" % x["run_compact_bytes_to_client"] for x in fold) + " |")
        rows.append("| ... the client's decryption and addition: s | " + " | ".join("%.4f" % x["client_decrypt_and_add_s"] for x in fold) + " |")
    for x in wall:
        if x["bench"] == "adder8_hop_gather":
            rows.append("| adder8 hop at T = 1000 over a resident state, no index: s | " + " | ".join("%.5f" % v for v in x["unmapped_hop_s"]) + " |")
            rows.append("| ... through the identity index: s | " + " | ".join("%.5f" % v for v in x["identity_index_hop_s"]) + " |")
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "sample_axis"))
    ap.add_argument("--kernels", action="store_true", help="the run the profiler watches")
    ap.add_argument("--stats", default=None, help="a rocprofv3 kernel_stats.csv of a --kernels run: write kernel_bandwidth.jsonl")
    ap.add_argument("--table", action="store_true")
    args = ap.parse_args()
    if args.table:
        print(table(args.out_dir))
        return
    if args.stats:
        run_line = _read(os.path.join(args.out_dir, "kernels_run.jsonl"))[0]
        _write(os.path.join(args.out_dir, "kernel_bandwidth.jsonl"), kernel_bandwidth(args.stats, run_line))
        return
    env, client, server = _setup()
    if args.kernels:
        _write(os.path.join(args.out_dir, "kernels_run.jsonl"), kernels_run(client, server, env))
    else:
        lines = sum_groups_wall(client, server, env) + fold_against_compact(client, server, env) + gather_overhead(client, server, env)
        _write(os.path.join(args.out_dir, "wall.jsonl"), lines)
    server.ctx.close()
    client.ctx.close()


if __name__ == "__main__":
    main()
