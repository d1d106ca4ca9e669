"""Whole `LutExecEnv.eval` wall with the inputs encrypted and the outputs decrypted on the host (ExecConfig.device_io=False:
ctx.encrypt, Program.eval, ctx.decrypt) against the device (device_io=True: Program.eval_messages), at the default 128-bit sets
and T = 1000.  One warm-up of each, then `--runs` of each alternated; medians.  Both paths must return the same outputs, and
the reference's own.
    python3 tools/device_io_bench.py [--runs 5] [--out profiles/r06/device_io.json] [--programs a,b]
Kernel times of k_encrypt / k_decrypt: run it under `rocprofv3 --kernel-trace --stats` (e.g. --runs 1) in a run of its own."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                                          # noqa: E402

from tests.helpers import load_fixture, subsample                           # noqa: E402
from tfhe_fbs_map_amd import ExecConfig, parse_fbs                          # noqa: E402

PROGRAMS = ("adder128__search_p15", "trivium_stream_short128__search_p15", "mul16__search_p15")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--programs", default=",".join(PROGRAMS))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rows = []
    for name in args.programs.split(","):
        rec = load_fixture(name)
        ins, expect = subsample(rec, args.T)
        env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
        cfg = ExecConfig(seed=1)                     # the default 128-bit set; one context and program for both paths

        def run(device_io):
            cfg.device_io = device_io
            t0 = time.perf_counter()
            out = env.eval(ins, config=cfg)
            return time.perf_counter() - t0, out

        _, ref_host = run(False)
        _, ref_dev = run(True)
        same = ref_host.keys() == ref_dev.keys() and all(np.array_equal(ref_host[k], ref_dev[k]) for k in ref_host)
        golden = all(np.array_equal(np.asarray(ref_dev[k]), np.asarray(v)) for k, v in expect.items())
        walls = {False: [], True: []}
        for _ in range(args.runs):
            for mode in (False, True):
                t, out = run(mode)
                walls[mode].append(t)
                same = same and all(np.array_equal(out[k], ref_host[k]) for k in ref_host)
        ctx = next(iter(cfg._contexts.values()))
        p = ctx.params
        row = dict(program=name, T=args.T, n_inputs=len(rec["program_inputs"]), n_outputs=len(expect),
                   params=dict(n=p.n, N=p.N, k=p.k, l_bsk=p.l_bsk, p_msg=p.p_msg, bsk_group=p.bsk_group), ct_words=p.ct_words,
                   host_io_wall_s=walls[False], device_io_wall_s=walls[True],
                   host_io_median_s=statistics.median(walls[False]), device_io_median_s=statistics.median(walls[True]),
                   outputs_equal=bool(same), outputs_match_reference=bool(golden))
        row["speedup"] = row["host_io_median_s"] / row["device_io_median_s"]
        rows.append(row)
        print(json.dumps({k: row[k] for k in ("program", "host_io_median_s", "device_io_median_s", "speedup", "outputs_equal",
                                              "outputs_match_reference")}), flush=True)
    result = dict(what="LutExecEnv.eval wall, device_io False vs True, medians of alternated runs after one warm-up each",
                  runs=args.runs, programs=rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    if not all(r["outputs_equal"] and r["outputs_match_reference"] for r in rows):
        sys.exit("outputs differ between the two paths or from the reference")


if __name__ == "__main__":
    main()
