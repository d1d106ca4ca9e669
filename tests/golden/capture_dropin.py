#!/usr/bin/env python3
"""Golden calls for tests/test_dropin.py, captured by IMPORTING the reference (a checkout of it, given as the argument).

The reference's map_to_fbs is run with this package's fbs_exec_env shadowing its own (what its `from fbs_exec_env import *`
picks up with the repository root first on sys.path), and every call it makes on the LutExecEnv it maps into is recorded in
order: input / const / linear / bootstrap / output, a node argument as the index of the call that returned it, a numpy scalar
with its dtype.  With the search swapped in (mapper_search.install, the test oracle behind it), every call of
MapToFBSHeur._find_lincomb_coefs_search is recorded with what the reference's own method answers.  Only data is written
(tests/golden/_dropin_traces.json.gz); no reference source.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/capture_dropin.py <reference checkout>
"""
import gzip
import io
import json
import logging
import os
import sys

import numpy as np

REF = sys.argv[1]
REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_dropin_traces.json.gz")
sys.dont_write_bytecode = True
sys.argv = ["capture"]
sys.path.insert(0, REF); sys.path.insert(0, os.path.join(REF, "experiments")); sys.path.insert(0, os.path.join(REF, "fbs_mapper"))
sys.path.insert(0, REPO)                          # our fbs_exec_env shadows fbs_mapper/fbs_exec_env.py
import fbs_exec_env  # noqa: E402
from tfhe_fbs_map_amd import fbs_exec_env as ours  # noqa: E402
assert fbs_exec_env.LutExecEnv is ours.LutExecEnv
import bit_exec_env, map_to_fbs, generate_benchmarks as gb  # noqa: E402,E401

Env = ours.LutExecEnv
traces = {}          # id(env) -> (env, calls, {id(node): index}, keep)


def plain(x):
    if isinstance(x, np.integer):
        return int(x)
    if isinstance(x, (list, tuple, np.ndarray)):
        return [plain(v) for v in x]
    return x


def enc(env, x):
    t = traces[id(env)]
    if isinstance(x, Env.Node) or type(x).__qualname__.startswith("LutExecEnv."):
        return {"node": t[2][id(x)]}
    if isinstance(x, (list, tuple, np.ndarray)):
        return [enc(env, v) for v in x]
    if isinstance(x, np.generic):
        return {"np": x.dtype.name, "v": x.item()}
    assert x is None or isinstance(x, (int, str)), type(x)
    return x


def wrap(name):
    orig = getattr(Env, name)

    def f(self, *args, **kw):
        if id(self) not in traces:
            traces[id(self)] = (self, [], {}, [])
        t = traces[id(self)]
        call = [name, [enc(self, a) for a in args], {k: enc(self, v) for k, v in kw.items()}]
        r = orig(self, *args, **kw)
        t[1].append(call)
        t[3].append(r)
        if r is not None:
            t[2][id(r)] = len(t[1]) - 1
        return r
    setattr(Env, name, f)


for m in ("input", "const", "linear", "bootstrap", "output"):
    wrap(m)
logging.disable(logging.CRITICAL)


def run(gen, mapper, p):
    traces.clear()
    env = bit_exec_env.BitExecEnv(); gb.Bit.set_env(env); getattr(gb, gen)(); env.remove_dangling_nodes()
    m = map_to_fbs.MapToFBSBasic() if mapper == "basic" else map_to_fbs.MapToFBSHeur(fbs_size=p, max_fbs_size=2 * p, max_truth_table_size=16, cone_merger=mapper)
    lut = m.map(env); lut.remove_dangling_nodes()
    s = io.StringIO(); lut.print(os=s, show_outputs=True)
    return traces[id(lut)][1], s.getvalue()


out = {"mappers": {}, "search": {}}
for mapper, p, fixture, gen in [("search", 7, "full_adder__search_p7", "full_adder_bench"), ("naive", 7, "aoi21__naive_p7", "aoi21_bench"),
                                ("search", 15, "aes_sbox__search_p15", "aes_sbox"), ("basic", 2, "ascon_lut__basic_p2", "ascon_lut")]:
    calls, text = run(gen, mapper, p)
    out["mappers"][fixture] = dict(mapper=mapper, p=p, calls=calls)
    print(fixture, len(calls), "calls", len(text), "chars")

# the search swapped in: every call of the replaced method, with what the reference's own method answers
ref_method = map_to_fbs.MapToFBSHeur._find_lincomb_coefs_search
from tfhe_fbs_map_amd import mapper_search  # noqa: E402
from oracle import mapper_search_oracle as mso  # noqa: E402
for p, fixture, gen in [(7, "full_adder__search_p7", "full_adder_bench"), (15, "aes_sbox__search_p15", "aes_sbox")]:
    searches = []

    def stand_in(xy_mvt, r_tt, fbs_size, max_fbs_size, device=0):
        return mso.find_lincomb_coefs_search(xy_mvt[:, 0], xy_mvt[:, 1], r_tt, fbs_size, max_fbs_size)
    mapper_search.find_lincomb_coefs_search = stand_in
    mapper_search.install(map_to_fbs.MapToFBSHeur)
    installed = map_to_fbs.MapToFBSHeur._find_lincomb_coefs_search

    def recording(self, xy_mvt, r_tt):
        ab, mvt = ref_method(self, xy_mvt, r_tt)
        searches.append(dict(xy=plain(np.asarray(xy_mvt)), tt=plain(np.asarray(r_tt)),
                             ab=None if ab is None else plain(ab), mvt=None if mvt is None else plain(np.asarray(mvt))))
        return installed(self, xy_mvt, r_tt)
    map_to_fbs.MapToFBSHeur._find_lincomb_coefs_search = recording
    calls, text = run(gen, "search", p)
    map_to_fbs.MapToFBSHeur._find_lincomb_coefs_search = ref_method
    out["search"][fixture] = dict(p=p, calls=calls, searches=searches)
    print(fixture, len(calls), "calls", len(searches), "searches")

with gzip.GzipFile(OUT, "wb", mtime=0) as f:
    f.write(json.dumps(out, separators=(",", ":"), sort_keys=True).encode())
