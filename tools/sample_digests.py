"""One SHA-256 per thing the project encrypts, at fixed seeds: the evidence that a change to the sample generators (csrc/fbs_host.cpp,
csrc/fbs_rows.hpp, csrc/fbs_keygen.hip, csrc/fbs_public.cpp) changes no word.  Run it in two checkouts and compare the files:

    python tools/sample_digests.py --label change
    python tools/sample_digests.py --label parent          # in a checkout of the parent commit (copy this file there)
    python tools/sample_digests.py --label change --host   # the host-only subset: HostContext and libfbspublic, no GPU

Parameter sets: those of tests/test_gpu_device_keys.py and the toy set of tests/test_gpu_device_io.py.  Per set, one line
"<set> <item> <sha256>" for: the full keys and the seeded keys (`device_keys` off and on), the packing key (host and device), the
public key and one public-key encryption, and 70 ciphertexts (more than one round of 64 lanes' worth of waves, not a multiple of
the waves of a workgroup) from `encrypt`, `encrypt_dev`, `encrypt_seeded` and `expand_seeded` (host and device) at one nonce.
Lines go to profiles/sample_rows/digests_<label>[_host].txt (--out) and to the standard output."""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED, NONCE, COUNT = 23, 1000, 70
NOISE_SEED, ENC_SEED = bytes(range(1, 33)), bytes(range(40, 72))


def sets():
    from tests.test_gpu_device_keys import NAMES, _sets
    from tfhe_fbs_map_amd import Params
    out = {name: _sets()[name] for name in NAMES}
    out["toy_io"] = Params(n=12, log_n_poly=10, p_msg=7, sigma_lwe=1 << 8, sigma_glwe=1 << 8)
    return out


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(a if isinstance(a, bytes) else np.ascontiguousarray(a, np.uint64).tobytes())
    return h.hexdigest()


def keys_and_rows(ctx, prm, tag, emit, device_rows):
    """everything one keyed context makes; tag: host | dev0 (device_keys off) | dev1 (on)"""
    from tfhe_fbs_map_amd import _public_native
    msgs = (np.arange(COUNT) * 5 - 17).astype(np.int64)
    ctx.keygen()
    full = ctx.export_keys()
    emit(tag + ".keys", digest(*[full[k] for k in ("sk_lwe", "sk_glwe", "bsk", "ksk")]))
    cts = ctx.encrypt(msgs, nonce0=NONCE)
    emit(tag + ".encrypt", digest(cts))
    ctx.keygen_seeded()
    seeded, expanded = ctx.export_seeded_keys(), ctx.export_keys()
    emit(tag + ".seeded_keys", digest(bytes(seeded["mask_key"]), seeded["bsk_bodies"], seeded["ksk_bodies"]))
    emit(tag + ".seeded_keys_expanded", digest(expanded["bsk"], expanded["ksk"]))
    ctx.packing_keygen(2, 7)
    pk = ctx.export_packing_key(full=True)
    emit(tag + ".packing_key", digest(pk["packing_bodies"], pk["full"]))
    if tag != "dev1":   # (the public key has no device form: once per library)
        pub = _public_native.keygen(prm, seeded["mask_key"], expanded["sk_glwe"], NOISE_SEED)
        emit(tag + ".public_key", digest(pub))
        enc = _public_native.Encryptor(prm, seeded["mask_key"], pub, seed=ENC_SEED)
        emit(tag + ".public_encrypt", digest(enc.encrypt(np.arange(COUNT) % (2 * prm.p_msg), nonce0=NONCE)[0]))
        enc.close()
    host = dict(device=False) if device_rows else {}
    bodies, _ = ctx.encrypt_seeded(msgs, nonce0=NONCE, **host)
    emit(tag + ".encrypt_seeded", digest(bodies))
    emit(tag + ".expand_seeded", digest(ctx.expand_seeded(bodies, NONCE)))
    if device_rows:
        import torch
        d_m = torch.from_numpy(msgs).cuda()
        d_c = torch.empty((COUNT, prm.ct_words), dtype=torch.int64, device="cuda")
        ctx.encrypt_dev(d_m.data_ptr(), COUNT, d_c.data_ptr(), nonce0=NONCE)
        ctx.sync()
        emit(tag + ".encrypt_dev", digest(d_c.cpu().numpy().view(np.uint64)))
        d_bodies, _ = ctx.encrypt_seeded(msgs, nonce0=NONCE, device=True)
        emit(tag + ".encrypt_seeded_dev", digest(d_bodies))
        d_b = torch.from_numpy(np.ascontiguousarray(bodies).view(np.int64)).cuda()
        ctx.expand_seeded_dev(d_b.data_ptr(), COUNT, NONCE, d_c.data_ptr())
        ctx.sync()
        emit(tag + ".expand_seeded_dev", digest(d_c.cpu().numpy().view(np.uint64)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--label", default="change", help="names the output file (change, parent)")
    ap.add_argument("--host", action="store_true", help="the host-only subset: no GPU is touched")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = args.out or os.path.join(ROOT, "profiles", "sample_rows", "digests_%s%s.txt" % (args.label, "_host" if args.host else ""))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    lines = []

    from tfhe_fbs_map_amd import HostContext
    for name, prm in sets().items():
        def emit(item, value):
            lines.append("%s %s %s" % (name, item, value))
            print(lines[-1], flush=True)
        ctx = HostContext(prm, seed=SEED, keygen=False)
        keys_and_rows(ctx, prm, "host", emit, False)
        ctx.close()
        if args.host:
            continue
        from tfhe_fbs_map_amd import Context
        for knob in (False, True):
            ctx = Context(prm, seed=SEED, keygen=False, device_keys=knob)
            keys_and_rows(ctx, prm, "dev%d" % knob, emit, True)
            ctx.close()
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
