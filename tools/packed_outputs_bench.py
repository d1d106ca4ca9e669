"""Full, compact and packed outputs of the client / server split (tfhe_fbs_map_amd/split.py): for adder128 (p = 15, the default
k = 2 set) and the AES S-box (p = 3) at T samples, `Server.run`, `Server.run_compact` and `Server.run_packed` on the same seeded
inputs, ALTERNATED `--reps` times (run, compact, packed, run, ...) so that drift of the box lands on all three alike.  Per path one
JSON line: median server wall time (each call blocks until its outputs are on the host), bytes returned, `.npz` size, client
decrypt time.  The decrypted outputs of the three paths are checked equal.

    python tools/packed_outputs_bench.py [--T 1000] [--reps 5] [--out profiles/packed_outputs/bench_T1000.jsonl]

The packing kernels' own times come from a separate run under `rocprofv3 --kernel-trace --stats` (profiles/packed_outputs/README.md):
k_pack_transpose, k_pack_accumulate, k_pack_finish and the key-switch dispatches in front of them."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIXTURES = ("adder128__search_p15", "aes_sbox__search_p3")
PATHS = ("full", "compact", "packed")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--fixtures", default=",".join(FIXTURES))
    args = ap.parse_args()
    from tests.helpers import load_fixture
    from tfhe_fbs_map_amd import Client, ExecConfig, Server, parse_fbs
    lines = []
    for name in args.fixtures.split(","):
        rec = load_fixture(name)
        env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
        t0 = time.perf_counter()
        client = Client(env, ExecConfig(seed=1), packing=True)
        keygen_s = time.perf_counter() - t0
        server = Server(client.server_key())
        run = dict(full=server.run, compact=server.run_compact, packed=server.run_packed)
        rng = np.random.default_rng(0)
        ins = {n: rng.integers(0, 2, args.T) for n in env.lower()["input_names"]}
        inputs = client.encrypt(ins)
        warm = client.encrypt({n: v[:8] for n, v in ins.items()})
        for path in PATHS:                                          # warm-up: program load, scratch, kernels
            run[path](env, warm)
        walls, outs = {p: [] for p in PATHS}, {}
        for _ in range(args.reps):
            for path in PATHS:
                t0 = time.perf_counter()
                outs[path] = run[path](env, inputs)
                walls[path].append(time.perf_counter() - t0)
        decoded = {}
        for path in PATHS:
            out = outs[path]
            data = out.cts if path == "full" else out.words
            with tempfile.TemporaryDirectory() as d:
                f = os.path.join(d, "out.npz")
                out.save(f)
                npz = os.path.getsize(f)
            t0 = time.perf_counter()
            decoded[path] = client.decrypt(out)
            dec_s = time.perf_counter() - t0
            prm = client.params
            line = dict(fixture=name, path=path, T=args.T, k=prm.k, N=prm.N, n=prm.n, p=prm.p_msg, packing=list(client.packing),
                        bits=getattr(out, "bits", None), n_outputs=len(out.output_names), keygen_s=round(keygen_s, 3),
                        packing_key_bytes=int(client.server_key().packing_bodies.nbytes),
                        server_s_median=float(np.median(walls[path])), server_s_all=[round(w, 4) for w in walls[path]],
                        bytes_returned=int(data.nbytes), npz_bytes=int(npz), client_decrypt_s=round(dec_s, 4))
            print(json.dumps(line), flush=True)
            lines.append(line)
        for path in PATHS[1:]:
            assert decoded["full"].keys() == decoded[path].keys()
            for k in decoded["full"]:
                assert np.array_equal(decoded["full"][k], decoded[path][k]), (name, path, k)
        server.ctx.close()
        client.ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
