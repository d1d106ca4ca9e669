"""Full against compact outputs of the client / server split (tfhe_fbs_map_amd/split.py): for adder128 (p = 15, the default k = 2
set) and the AES S-box (p = 3, the default k = 3 set at N = 512) at T samples, `Server.run` and `Server.run_compact` on the same
seeded inputs.  Per path, one JSON line: server wall time (the call blocks until the outputs are on the host), bytes returned, `.npz`
size, client decrypt time.  The decrypted outputs of the two paths are checked equal.

    python tools/compact_outputs_bench.py [--T 1000] [--reps 3] [--out profiles/compact_outputs/bench_T1000.jsonl]

The kernels' own times come from a separate run under `rocprofv3 --kernel-trace --stats -f csv`
(profiles/compact_outputs/README.md); `--trace <kernel_trace.csv>` reads that run's trace and prints what the compaction cost: every `k_compact_pack` dispatch and the
key-switch dispatches right in front of it (the key switch to the small key it packs), against all key switches and all blind
rotations of the run."""
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
KEYSWITCH = ("k_ks_digits", "k_ks_gemm", "k_ks_gemm_finish", "k_keyswitch", "k_ms_body")


def summarize_trace(path):
    """per kernel group, dispatches and total ms of a rocprofv3 kernel trace (csv), compaction separated out"""
    import csv
    with open(path) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    base = [r["Kernel_Name"].split("(")[0].split("<")[0].replace("void ", "").replace("fbs::", "").strip() for r in rows]
    ms = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows]
    groups = {g: [0, 0.0] for g in ("compact_pack", "compact_keyswitch", "keyswitch_all", "blind_rotate_all", "decrypt_compact")}
    for i, (b, t) in enumerate(zip(base, ms)):
        if b == "k_compact_pack":
            groups["compact_pack"][0] += 1
            groups["compact_pack"][1] += t
            j = i - 1
            while j >= 0 and base[j] in KEYSWITCH:             # the key switch whose fields this launch packs
                groups["compact_keyswitch"][0] += 1
                groups["compact_keyswitch"][1] += ms[j]
                j -= 1
        elif b in KEYSWITCH:
            groups["keyswitch_all"][0] += 1
            groups["keyswitch_all"][1] += t
        elif b.startswith("k_blind_rotate"):
            groups["blind_rotate_all"][0] += 1
            groups["blind_rotate_all"][1] += t
        elif b == "k_decrypt_compact":
            groups["decrypt_compact"][0] += 1
            groups["decrypt_compact"][1] += t
    return {g: dict(dispatches=v[0], ms=round(v[1], 3)) for g, v in groups.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--fixtures", default=",".join(FIXTURES))
    ap.add_argument("--trace", default=None, help="summarise this rocprofv3 kernel_trace.csv instead of running")
    args = ap.parse_args()
    if args.trace:
        print(json.dumps(summarize_trace(args.trace)))
        return
    from tests.helpers import load_fixture
    from tfhe_fbs_map_amd import Client, ExecConfig, Server, parse_fbs
    lines = []
    for name in args.fixtures.split(","):
        rec = load_fixture(name)
        env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
        client = Client(env, ExecConfig(seed=1))
        server = Server(client.server_key())
        rng = np.random.default_rng(0)
        ins = {n: rng.integers(0, 2, args.T) for n in env.lower()["input_names"]}
        inputs = client.encrypt(ins)
        server.run_compact(env, client.encrypt({n: v[:8] for n, v in ins.items()}))      # warm-up: program load, scratch, kernels
        server.run(env, client.encrypt({n: v[:8] for n, v in ins.items()}))
        decoded = {}
        for path in ("full", "compact"):
            run = server.run if path == "full" else server.run_compact
            walls = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                out = run(env, inputs)
                walls.append(time.perf_counter() - t0)
            data = out.cts if path == "full" else out.words
            with tempfile.TemporaryDirectory() as d:
                f = os.path.join(d, "out.npz")
                out.save(f)
                npz = os.path.getsize(f)
            t0 = time.perf_counter()
            decoded[path] = client.decrypt(out)
            dec_s = time.perf_counter() - t0
            prm = client.params
            line = dict(fixture=name, path=path, T=args.T, k=prm.k, N=prm.N, n=prm.n, p=prm.p_msg,
                        bits=getattr(out, "bits", None), n_outputs=len(out.output_names),
                        server_s_median=float(np.median(walls)), server_s_all=[round(w, 4) for w in walls],
                        bytes_returned=int(data.nbytes), npz_bytes=int(npz), client_decrypt_s=round(dec_s, 4))
            print(json.dumps(line), flush=True)
            lines.append(line)
        assert decoded["full"].keys() == decoded["compact"].keys()
        for k in decoded["full"]:
            assert np.array_equal(decoded["full"][k], decoded["compact"][k]), (name, k)
        server.ctx.close()
        client.ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
