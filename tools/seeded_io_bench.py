"""Evaluation without the secret key (tfhe_fbs_map_amd.split): bytes of full and seeded keys and inputs, and the wall of
`Server.run` (seeded inputs expanded on the GPU, full output ciphertexts back) against `LutExecEnv.eval` with device I/O, at the
default 128-bit sets and T = 1000.  One warm-up of each, then `--runs` of each alternated; medians.  The client's encryption and
decryption walls are reported beside them.  Both paths must decrypt to the same outputs, and to the reference's own.
    python3 tools/seeded_io_bench.py [--runs 5] [--out profiles/r07/seeded_io.json] [--programs a,b]
Kernel times of k_expand_seeded (and k_encrypt, from the eval runs): run it under `rocprofv3 --kernel-trace --stats` (e.g.
--runs 1) in a run of its own."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                                          # noqa: E402

from tests.helpers import load_fixture, subsample                           # noqa: E402
from tfhe_fbs_map_amd import Client, ExecConfig, Server, parse_fbs          # noqa: E402

PROGRAMS = ("adder128__search_p15", "trivium_stream_short128__search_p15")


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
        cfg = ExecConfig(seed=1)                     # the default 128-bit set: the client shares its secrets with eval's context
        t0 = time.perf_counter()
        client = Client(env, cfg)
        keygen_s = time.perf_counter() - t0
        key = client.server_key()
        t0 = time.perf_counter()
        server = Server(key)
        import_s = time.perf_counter() - t0
        prm, T = key.params, args.T
        ctx = server.ctx
        sizes = ctx.seeded_key_sizes()
        import ctypes as C
        from tfhe_fbs_map_amd import _native as nat
        full = (C.c_size_t * 4)()
        ctx._check(nat.lib.fbs_key_sizes(ctx._h, C.byref(full)))
        n_in = len(rec["program_inputs"])

        def split_run():
            t0 = time.perf_counter()
            enc = client.encrypt(ins)
            t1 = time.perf_counter()
            outs = server.run(env, enc)
            t2 = time.perf_counter()
            got = client.decrypt(outs)
            return (t1 - t0, t2 - t1, time.perf_counter() - t2), got

        def eval_run():
            t0 = time.perf_counter()
            out = env.eval(ins, config=cfg)
            return time.perf_counter() - t0, out

        _, ref_split = split_run()
        _, ref_eval = eval_run()
        same = ref_split.keys() == ref_eval.keys() and all(np.array_equal(ref_split[k], ref_eval[k]) for k in ref_eval)
        golden = all(np.array_equal(np.asarray(ref_split[k]), np.asarray(v)) for k, v in expect.items())
        walls = dict(encrypt=[], server=[], decrypt=[], eval=[])
        for _ in range(args.runs):
            (te, ts, td), got = split_run()
            walls["encrypt"].append(te), walls["server"].append(ts), walls["decrypt"].append(td)
            t, out = eval_run()
            walls["eval"].append(t)
            same = same and all(np.array_equal(got[k], out[k]) and np.array_equal(out[k], ref_eval[k]) for k in ref_eval)
        row = dict(program=name, T=T, n_inputs=n_in, n_outputs=len(expect), fuse_tables=key.fuse_tables,
                   params=dict(n=prm.n, N=prm.N, k=prm.k, l_bsk=prm.l_bsk, t_ksk=prm.t_ksk, p_msg=prm.p_msg, bsk_group=prm.bsk_group),
                   bytes=dict(bsk_full=int(full[2]) * 8, ksk_full=int(full[3]) * 8, bsk_seeded=sizes[0] * 8, ksk_seeded=sizes[1] * 8,
                              mask_key=32, inputs_full=n_in * T * prm.ct_words * 8, inputs_seeded=n_in * T * 8 + 8,
                              outputs=len(expect) * T * prm.ct_words * 8),
                   client_keygen_s=keygen_s, server_import_s=import_s,
                   walls_s=walls, medians_s={k: statistics.median(v) for k, v in walls.items()},
                   outputs_equal=bool(same), outputs_match_reference=bool(golden))
        rows.append(row)
        print(json.dumps({k: row[k] for k in ("program", "medians_s", "bytes", "outputs_equal", "outputs_match_reference")}), flush=True)
        server.ctx.close()
        client.ctx.close()
    result = dict(what="Server.run wall (seeded inputs in, full ciphertexts out) vs LutExecEnv.eval (device I/O); client encrypt / "
                       "decrypt walls beside them; medians of alternated runs after one warm-up each", runs=args.runs, programs=rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    if not all(r["outputs_equal"] and r["outputs_match_reference"] for r in rows):
        sys.exit("outputs differ between the two paths or from the reference")


if __name__ == "__main__":
    main()
