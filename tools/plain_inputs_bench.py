"""Plaintext server inputs (tfhe_fbs_map_amd/split.py, `PlainInputs`; FBS_SRC_PLAIN in include/fbs_exec.h): adder128 at its default
set, operand a from the client (seeded), operand b from the server, at T samples.  Three paths through the same call,
`Server.run_chain(env, [a, b])`, ALTERNATED `--reps` times so that drift of the box lands on all alike:

    seeded      b seeded too: both operands from the client.  This path exists before plaintext inputs did, so the same tool run on
                the commit before them (`--paths seeded`) gives the figure the other two are held against
    plain       b as a `PlainInputs` with a value per sample: 8 bytes a sample and input cross the bus, as for a seeded body
    broadcast   b as a `PlainInputs` with one value per input for all samples: nothing per sample crosses the bus

Per path one JSON line: the bytes that cross the bus on the way in, the server-call wall time (median, and every repetition), and
the repetitions' spread (max - min over the median).  The decrypted sums are checked against the cleartext adder.

    python tools/plain_inputs_bench.py [--T 1000] [--reps 5] [--paths seeded,plain,broadcast] [--out profiles/plain_inputs/bench_T1000.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIXTURE = "adder128__search_p15"
PATHS = ("seeded", "plain", "broadcast")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--paths", default=",".join(PATHS))
    ap.add_argument("--label", default="", help="a word for the record, e.g. which commit ran")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    paths = [p for p in args.paths.split(",") if p]
    assert set(paths) <= set(PATHS), paths
    from oracle import lut_oracle
    from tests.helpers import load_fixture
    from tfhe_fbs_map_amd import Client, ExecConfig, Server, parse_fbs
    rec = load_fixture(FIXTURE)
    env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
    names = env.lower()["input_names"]
    a_names, b_names = [n for n in names if n.startswith("a")], [n for n in names if n.startswith("b")]
    assert len(a_names) == len(b_names) == 128 and len(names) == 256
    client = Client(env, ExecConfig(seed=1))
    server = Server(client.server_key())
    T = args.T
    rng = np.random.default_rng(0)
    a = {n: rng.integers(0, 2, T) for n in a_names}
    b = {n: rng.integers(0, 2, T) for n in b_names}
    b_once = {n: int(rng.integers(0, 2)) for n in b_names}
    enc_a = client.encrypt(a, names=a_names)

    def sources(path, T_=T, a_=None):
        if path == "seeded":
            return [a_ or enc_a, client.encrypt({n: v[:T_] for n, v in b.items()}, names=b_names)]
        from tfhe_fbs_map_amd.split import PlainInputs
        if path == "plain":
            return [a_ or enc_a, PlainInputs(b_names, T_, {n: v[:T_] for n, v in b.items()})]
        return [a_ or enc_a, PlainInputs(b_names, None, b_once)]

    warm_a = client.encrypt({n: v[:8] for n, v in a.items()}, names=a_names)
    made = {p: sources(p) for p in paths}
    for p in paths:                                                   # warm-up: program load, scratch, kernels
        server.run_chain(env, sources(p, 8, warm_a))
        server.run_chain(env, made[p])
    walls, outs = {p: [] for p in paths}, {}
    for _ in range(args.reps):
        for p in paths:
            t0 = time.perf_counter()
            outs[p] = server.run_chain(env, made[p])
            walls[p].append(time.perf_counter() - t0)
    prm = client.params
    lines = []
    for p in paths:
        b_clear = b if p != "broadcast" else {n: np.full(T, v) for n, v in b_once.items()}
        clear = lut_oracle.eval_fbs_text(rec["fbs"], {**a, **b_clear})
        got = client.decrypt(outs[p])
        for k in clear:
            assert np.array_equal(np.broadcast_to(got[k], (T,)), np.broadcast_to(clear[k], (T,))), (p, k)
        b_bytes = {"seeded": 8 * 128 * T, "plain": 8 * 128 * T, "broadcast": 0}[p]
        med = float(np.median(walls[p]))
        line = dict(fixture=FIXTURE, path=p, label=args.label, T=T, k=prm.k, N=prm.N, n=prm.n, p=prm.p_msg,
                    bytes_in=8 * 128 * T + b_bytes, bytes_in_operand_b=b_bytes, bytes_in_as_full_ciphertexts=256 * T * prm.ct_words * 8,
                    server_s_median=med, server_s_all=[round(w, 4) for w in walls[p]],
                    spread=round((max(walls[p]) - min(walls[p])) / med, 4))
        print(json.dumps(line), flush=True)
        lines.append(line)
    server.ctx.close()
    client.ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
