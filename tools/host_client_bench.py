"""What the client's own work costs, on the host alone and on a GPU context: key generation (`split.Client(...)`: parameter choice,
`keygen_seeded`, the server key) and `Client.encrypt` of one evaluation's inputs, for adder128__search_p15 at T = 1000 by default
-- 256 inputs x 1000 samples = 256 000 seeded ciphertexts, each a ChaCha20 mask of k N words (about 4 GB of masks at k = 2,
N = 1024) folded into one body word.

    python tools/host_client_bench.py --client host      # libfbsclient.so alone; runs on a machine without a GPU
    python tools/host_client_bench.py --client gpu       # a GPU context (libfbsexec.so): keygen on its host, encryption on the device
    python tools/host_client_bench.py --client host --sampler gaussian     # the same with the rounded-Gaussian noise sampler

Each run appends one JSON line to profiles/host_client/<client>.jsonl (--out): seconds per stage (best and median of --repeats
for the encryption), the parameter set, the thread count the host code sized its pool by, and a checksum of the bodies, which is
the same for both clients (the same words).  The figures are recorded, not gated.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--client", choices=("host", "gpu"), required=True)
    ap.add_argument("--fixture", default="adder128__search_p15")
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--sampler", choices=("irwin_hall", "gaussian"), default="irwin_hall", help="the noise sampler of the keys and inputs (ExecConfig.sampler)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from tests.helpers import load_fixture, subsample
    from tfhe_fbs_map_amd import Client, ExecConfig, parse_fbs
    from dataclasses import asdict

    rec = load_fixture(args.fixture)
    env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
    ins, _ = subsample(rec, args.samples)

    t0 = time.perf_counter()
    client = Client(env, ExecConfig(seed=args.seed, sampler=args.sampler), host=args.client == "host")
    t1 = time.perf_counter()
    key = client.server_key()
    t2 = time.perf_counter()

    enc_s, digest = [], None
    for _ in range(max(1, args.repeats)):
        a = time.perf_counter()
        enc = client.encrypt(ins, nonce0=1)          # an explicit first stream: every repeat, and both clients, make the same words
        enc_s.append(time.perf_counter() - a)
        digest = hashlib.sha256(np.ascontiguousarray(enc.bodies).tobytes()).hexdigest()[:16]
    prm = client.params
    line = dict(tool="host_client_bench", client=args.client, sampler=args.sampler, device_info=client.ctx.device_info, fixture=args.fixture,
                samples=args.samples, n_inputs=len(enc.input_names), ciphertexts=int(enc.bodies.size),
                mask_bytes=int(enc.bodies.size) * prm.big_dim * 8, params=asdict(prm),
                keygen_s=round(t1 - t0, 4), server_key_export_s=round(t2 - t1, 4),
                server_key_bytes=int(key.bsk_bodies.nbytes + key.ksk_bodies.nbytes + 32),
                encrypt_s_best=round(min(enc_s), 4), encrypt_s_median=round(statistics.median(enc_s), 4), encrypt_s_all=[round(x, 4) for x in enc_s],
                encrypt_cts_per_s=round(enc.bodies.size / min(enc_s), 1), bodies_sha256_16=digest,
                omp_num_threads=os.environ.get("OMP_NUM_THREADS"), cpu_count=os.cpu_count())
    text = json.dumps(line)
    print(text)
    out = args.out or os.path.join(ROOT, "profiles", "host_client", args.client + ".jsonl")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
