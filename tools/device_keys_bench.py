"""What making the evaluation keys costs, on the host and on the device (knob "keys_on_device", `ExecConfig.device_keys`): wall
times of the three places a user meets key generation, per fixture (default: adder128__search_p15 and adder8__search_p7 at the
128-bit sets `ExecConfig` chooses for them) and per setting of the knob:

    client_s       `Client(env, ExecConfig(seed=5, device_keys=knob), host=False)`: parameter choice, `keygen_seeded`, upload, transform
    server_s       `Server(server_key, device_keys=knob)`: the server key expanded into full keys, uploaded, transformed
    first_eval_s   the first `LutExecEnv.eval` of a fresh `ExecConfig(seed=5, device_keys=knob)` at T = 1000: `keygen`, program load, run
    eval_s         the second `eval` of the same configuration (no keys to make: what the first one is to be set against)

and the two statistics of each context (`keys_made_on_device`, `bsk_upload_bytes`).

    python tools/device_keys_bench.py --label change
    python tools/device_keys_bench.py --label parent      # in a checkout of the parent commit (copy this file there)

A checkout that does not know the knob (`ExecConfig` has no `device_keys`) runs the knob-off legs alone and says so in its lines.
Each run appends one JSON line per (fixture, knob) to profiles/device_keys/<label>.jsonl (--out).  The figures are recorded, not
gated.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--label", default="change", help="names the output file and the lines (change, parent)")
    ap.add_argument("--fixtures", default="adder128__search_p15,adder8__search_p7")
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from dataclasses import asdict, fields
    from tests.helpers import assert_outputs_equal, load_fixture, subsample
    from tfhe_fbs_map_amd import Client, ExecConfig, Server, parse_fbs

    has_knob = "device_keys" in {f.name for f in fields(ExecConfig)}
    out = args.out or os.path.join(ROOT, "profiles", "device_keys", args.label + ".jsonl")
    os.makedirs(os.path.dirname(out), exist_ok=True)

    # the first context of a process pays for loading the GPU runtime and the code objects: a toy one takes that, on the host path
    # and (where there is one) on the device path, so that no timed leg does
    from tfhe_fbs_map_amd import Context, Params
    toy = Params(n=12, log_n_poly=8, k=1, l_bsk=2, beta_bsk=10, t_ksk=8, gamma_ksk=2, p_msg=7, sigma_lwe=1 << 8, sigma_glwe=4)
    for knob in ((False, True) if has_knob else (False,)):
        warm = Context(toy, seed=1, **(dict(device_keys=knob) if has_knob else {}))
        warm.decrypt(warm.bootstrap_batch(warm.tvset([[0, 1]]), warm.encrypt([0, 1], nonce0=1)))
        warm.close()

    def stats(ctx):
        if not has_knob:
            return dict(keys_made_on_device=None, bsk_upload_bytes=None)
        return dict(keys_made_on_device=ctx.stat("keys_made_on_device"), bsk_upload_bytes=ctx.stat("bsk_upload_bytes"))

    for name in args.fixtures.split(","):
        rec = load_fixture(name)
        env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
        ins, outs = subsample(rec, args.samples)
        for knob in ((False, True) if has_knob else (False,)):
            extra = dict(device_keys=knob) if has_knob else {}
            t0 = time.perf_counter()
            client = Client(env, ExecConfig(seed=args.seed, **extra), host=False)
            t1 = time.perf_counter()
            key = client.server_key()
            t2 = time.perf_counter()
            server = Server(key, **extra)
            t3 = time.perf_counter()
            client_stats, server_stats, prm = stats(client.ctx), stats(server.ctx), client.params
            server.ctx.close()
            client.ctx.close()
            del server, client

            cfg = ExecConfig(seed=args.seed, **extra)
            t4 = time.perf_counter()
            got = env.eval(ins, config=cfg)
            t5 = time.perf_counter()
            env.eval(ins, config=cfg)
            t6 = time.perf_counter()
            assert_outputs_equal(got, outs)
            ctx = next(iter(cfg._contexts.values()))
            line = dict(tool="device_keys_bench", label=args.label, knows_knob=has_knob, keys_on_device=int(knob), fixture=name,
                        samples=args.samples, device_info=ctx.device_info, params=asdict(ctx.params), client_params=asdict(prm),
                        client_s=round(t1 - t0, 4), server_key_export_s=round(t2 - t1, 4), server_s=round(t3 - t2, 4),
                        first_eval_s=round(t5 - t4, 4), eval_s=round(t6 - t5, 4),
                        client_stats=client_stats, server_stats=server_stats, eval_stats=stats(ctx),
                        server_key_bytes=int(key.bsk_bodies.nbytes + key.ksk_bodies.nbytes + 32),
                        omp_num_threads=os.environ.get("OMP_NUM_THREADS"), cpu_count=os.cpu_count())
            text = json.dumps(line)
            print(text, flush=True)
            with open(out, "a") as f:
                f.write(text + "\n")


if __name__ == "__main__":
    main()
