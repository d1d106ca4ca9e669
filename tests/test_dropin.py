"""Drop-in checks on the CPU: the module-name shim, and the REFERENCE's own mappers building their programs into this
package's LutExecEnv, byte-identical to what they build into the reference's.

The mappers' side is recorded data (tests/golden/_dropin_traces.json.gz): the reference's map_to_fbs was run with this
package's fbs_exec_env shadowing its own, and every call it made on the LutExecEnv (input / const / linear / bootstrap /
output; a node argument as the index of the call that returned it, a numpy scalar with its dtype) was kept in order -- and, with the search
swapped in, every call of MapToFBSHeur._find_lincomb_coefs_search with what the reference's own method answers.  The
tests replay those calls into the env imported under the reference's module name."""
import gzip
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import GOLDEN, load_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def traces():
    with gzip.open(os.path.join(GOLDEN, "_dropin_traces.json.gz"), "rb") as f:
        return json.loads(f.read().decode())


def replay(calls):
    """The recorded mapper calls on a fresh LutExecEnv of the shim module; -> the program text the mapper's caller prints."""
    from fbs_exec_env import LutExecEnv
    env, made = LutExecEnv(), []

    def arg(v):
        if isinstance(v, dict):
            return made[v["node"]] if "node" in v else np.dtype(v["np"]).type(v["v"])
        return [arg(x) for x in v] if isinstance(v, list) else v
    for name, args, kw in calls:
        made.append(getattr(env, name)(*[arg(a) for a in args], **{k: arg(v) for k, v in kw.items()}))
    assert "tfhe_fbs_map_amd" in type(env).__module__
    env.remove_dangling_nodes()
    s = io.StringIO()
    env.print(os=s, show_outputs=True)
    return s.getvalue()


def test_module_name_shim():
    code = ("import sys; sys.path.insert(0, %r); from fbs_exec_env import *; "
            "e = LutExecEnv(); a = e.input('a'); b = e.input('b'); "
            "m = e.bootstrap(e.linear([1, 2], [a, b]), [0, 1, 1, 0]); e.output('o', m); "
            "import io; s = io.StringIO(); e.print(os=s, show_outputs=True); print(s.getvalue(), end='')" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True).stdout
    assert out == "m1 = 1 * a + 2 * b \nm2 = Bootstrap(m1, [0, 1, 1, 0])\nOutput o = m2\n"


@pytest.mark.parametrize("mapper,p,fixture", [("search", 7, "full_adder__search_p7"), ("naive", 7, "aoi21__naive_p7"),
                                              ("search", 15, "aes_sbox__search_p15"), ("basic", 2, "ascon_lut__basic_p2")])
def test_reference_mappers_build_into_this_env(mapper, p, fixture):
    """The reference's map_to_fbs building into OUR fbs_exec_env (its recorded calls, replayed): the mapped program text
    must equal the fixture the reference produced with its own class."""
    rec = traces()["mappers"][fixture]
    assert (rec["mapper"], rec["p"]) == (mapper, p) and rec["calls"]
    assert replay(rec["calls"]) == load_fixture(fixture)["fbs"]


@pytest.mark.parametrize("p,fixture", [(7, "full_adder__search_p7"), (15, "aes_sbox__search_p15")])
def test_reference_mapper_with_the_search_swapped_in(p, fixture, monkeypatch):
    """`mapper_search.install(MapToFBSHeur)`: the installed method, on every call the reference's mapper made of it, must
    give what the reference's own method gave, and the mapper's calls on the env then map to the same program.  There is
    no GPU here, so the function behind the binding is stood in for by the test oracle (same arguments, same return value);
    on the GPU box tests/test_mapper_search.py holds the kernel itself against the recorded reference results."""
    from tfhe_fbs_map_amd import mapper_search
    from oracle import mapper_search_oracle as mso
    rec = traces()["search"][fixture]
    calls = []

    def stand_in(xy_mvt, r_tt, fbs_size, max_fbs_size, device=0):
        calls.append(len(r_tt))
        return mso.find_lincomb_coefs_search(xy_mvt[:, 0], xy_mvt[:, 1], r_tt, fbs_size, max_fbs_size)

    class MapToFBSHeur:                     # what the installed method reads of the reference's mapper object
        fbs_size, max_fbs_size = p, 2 * p
    monkeypatch.setattr(mapper_search, "find_lincomb_coefs_search", stand_in)
    m = mapper_search.install(MapToFBSHeur)()
    for c in rec["searches"]:
        ab, mvt = m._find_lincomb_coefs_search(np.asarray(c["xy"], np.int64), np.asarray(c["tt"], np.int64))
        if c["ab"] is None:
            assert ab is None and mvt is None
        else:
            assert list(ab) == c["ab"] and np.asarray(mvt).tolist() == c["mvt"]
    assert calls and len(calls) == len(rec["searches"]), 'the replaced method was never reached'
    assert replay(rec["calls"]) == load_fixture(fixture)["fbs"]
