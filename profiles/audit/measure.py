"""Wall time of LutExecEnv.audit against LutExecEnv.eval of the same program, inputs and box; the report's margins.
usage (from the repository root): python profiles/audit/measure.py OUT.jsonl [--profile NAME]   (--profile: one all-points audit of NAME only, for a kernel trace)"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from tests.helpers import load_fixture                                    # noqa: E402
from tfhe_fbs_map_amd import ExecConfig, parse_fbs                        # noqa: E402
from tfhe_fbs_map_amd.audit import POINTS                                 # noqa: E402

out_path = sys.argv[1]
profile = sys.argv[3] if len(sys.argv) > 3 and sys.argv[2] == "--profile" else None
names = [profile] if profile else ["aes_sbox__search_p7", "adder128__search_p15"]
T = 1000


def timed(f):
    t0 = time.perf_counter()
    r = f()                                                              # eval and audit both end in a device synchronise
    return r, time.perf_counter() - t0


with open(out_path, "a") as fh:
    for name in names:
        rec = load_fixture(name)
        env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
        ins = {k: v[:T] for k, v in rec["inputs"].items()}
        cfg = ExecConfig(seed=1, nonce0=1000)
        got, first = timed(lambda: env.eval(ins, config=cfg))
        ok = all(np.array_equal(got[k], v[:T] if not isinstance(v, int) else v) for k, v in rec["outputs"].items())
        choice = cfg.last_choice
        prm = choice["params"]
        base = dict(name=name, T=T, stats=env.stats(), fused=choice["fuse_tables"], model_margin=choice["margin_sigmas"], norm2=choice["norm2"],
                    params=dict(n=prm.n, N=prm.N, k=prm.k, p=prm.p_msg, l=prm.l_bsk, beta=prm.beta_bsk, t=prm.t_ksk, gamma=prm.gamma_ksk),
                    eval_matches_golden=bool(ok), first_eval_s=first)
        if profile:
            env.audit(ins, config=cfg, points=POINTS)                    # warm: scratch grows here
            report, dt = timed(lambda: env.audit(ins, config=cfg, points=POINTS))
            fh.write(json.dumps(dict(base, what="profiled audit, all points", s=dt, min_margin=report.min_margin)) + "\n")
            open(out_path.replace(".jsonl", "_report_%s.json" % name), "w").write(report.to_json())
            continue
        env.audit(ins, config=cfg, points=POINTS)                        # warm every shape the timed window uses
        times = dict(eval=[], audit_rotation_input=[], audit_all=[])
        reports = {}
        for rep in range(3):                                             # alternating, so drift of the box hits all three alike
            times["eval"].append(timed(lambda: env.eval(ins, config=cfg))[1])
            r, dt = timed(lambda: env.audit(ins, config=cfg, points=("rotation_input",)))
            times["audit_rotation_input"].append(dt)
            reports["rotation_input"] = r
            r, dt = timed(lambda: env.audit(ins, config=cfg, points=POINTS))
            times["audit_all"].append(dt)
            reports["all"] = r
        for what, r in reports.items():
            same = all(np.array_equal(r.outputs[k], got[k]) for k in got)
            rots = [x for x in r.rows if x.point == "rotation_input"]
            boots = [x for x in r.rows if x.point == "bootstrap"]
            worst = r.worst(1)[0]
            row = dict(base, what="audit " + what, rows=len(r.rows), outputs_equal_eval=bool(same), min_margin=r.min_margin, failures=r.failures,
                       min_rotation_margin=min(x.margin for x in rots), min_rotation_model_margin=min(x.model_margin for x in rots),
                       median_rotation_margin=float(np.median([x.margin for x in rots])),
                       median_rotation_std_over_predicted=float(np.median([x.std / x.predicted_std for x in rots])),
                       max_rotation_std_over_predicted=float(max(x.std / x.predicted_std for x in rots)),
                       max_abs_mean_over_half_box=float(max(abs(x.mean) * 4 * x.p for x in rots)),
                       worst_row=worst.to_dict(), worst_fraction_of_half_box=max(x.worst for x in r.rows))
            if boots:
                q = boots[0].unit
                pooled = (sum(x.sumsq for x in boots) / sum(x.count for x in boots)) ** 0.5 / q
                row.update(bootstrap_pooled_std=pooled, bootstrap_predicted_std=min(x.predicted_std for x in boots))
            fh.write(json.dumps(row) + "\n")
        fh.write(json.dumps(dict(base, what="wall times (s), three alternating repetitions", **times,
                                 best={k: min(v) for k, v in times.items()})) + "\n")
        fh.flush()
        print(name, {k: round(min(v), 3) for k, v in times.items()}, flush=True)
