"""Resident state without a GPU (include/fbs_exec.h, "resident state"): the new entries are declared, exported and bound, the ctypes
image of fbs_resident_src has the header's layout, `plan_chain` links a `ResidentOutputs` under the rule of `EncryptedOutputs`
and refuses what it must, and resident outputs cannot be asked for compact."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.test_chain_abi import A_FROM_S, _adder, _key_params, _sources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fbs_state_create", "fbs_state_destroy", "fbs_state_info", "fbs_eval_resident", "fbs_state_fetch", "fbs_state_put")


def test_entries_are_declared_exported_and_bound():
    from tests.test_capi_symbols import declared_symbols
    from tfhe_fbs_map_amd import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in ENTRIES:
        assert name in declared_symbols(), name
        assert hasattr(lib, name), name
        assert name in _native.EXPORTED_SYMBOLS, name
    assert callable(_native.Program.eval_resident) and callable(_native.Context.state)
    for meth in ("fetch", "put", "close", "__enter__", "__exit__"):
        assert callable(getattr(_native.DeviceState, meth)), meth


def test_resident_src_has_the_layout_of_the_header():
    from tfhe_fbs_map_amd import _native
    text = open(os.path.join(ROOT, "include", "fbs_exec.h")).read()
    body = re.search(r"typedef struct fbs_resident_src \{(.*?)\} fbs_resident_src;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(t.strip(), n) for t, n in re.findall(r"([\w \*]+?)\b(\w+);", body)]
    assert fields == [("const fbs_state *", "state"), ("uint32_t", "row"), ("uint32_t", "refresh")]
    want = {"const fbs_state *": ctypes.c_void_p, "uint32_t": ctypes.c_uint32}
    assert [(n, want[t]) for t, n in fields] == list(_native._ResidentSrc._fields_)
    S = _native._ResidentSrc
    assert ctypes.sizeof(S) == 16 and (S.state.offset, S.row.offset, S.refresh.offset) == (0, 8, 12)
    # fbs_input_src is unchanged
    assert ctypes.sizeof(_native._InputSrc) == 32 and _native._InputSrc.nonce0.offset == 16 and _native._InputSrc.data.offset == 24


class _StubState:
    """stands for a DeviceState: plan_chain asks it only whether it is closed"""

    def __init__(self, closed=False):
        self.closed = closed


def _resident(T=4, fp=bytes(8), out_norm2=1.0, closed=False):
    from tfhe_fbs_map_amd.split import ResidentOutputs
    names = [f"s{i}" for i in range(8)] + ["cout"]
    return ResidentOutputs(names, T, fp, None if out_norm2 is None else np.full(9, float(out_norm2)), _StubState(closed))


def test_plan_chain_links_resident_outputs_like_full_ones():
    from tfhe_fbs_map_amd.split import plan_chain
    env = _adder()
    prm, fuse = _key_params(env)
    _, fresh = _sources(prm)
    for o2, refresh in ((1.0, False), (0.0, False), (2.0, True)):
        links, T = plan_chain(prm, fuse, bytes(8), env, [_resident(out_norm2=o2), fresh], rename=A_FROM_S)
        assert T == 4
        for i in range(8):
            assert (links[i].kind, links[i].source, links[i].index, links[i].refresh) == ("state", 0, i, refresh), o2
            assert links[i].noise == (1.0 if refresh else o2) and (links[i].margin is not None) == refresh
            assert (links[8 + i].kind, links[8 + i].source, links[8 + i].index) == ("seeded", 1, i)
        # the same plan as the same ciphertexts on the host, but for the kind
        full, _ = _sources(prm, out_norm2=o2, compact=False)
        host_links, _ = plan_chain(prm, fuse, bytes(8), env, [full, fresh], rename=A_FROM_S)
        for a, b in zip(links, host_links):
            assert (a.name, a.source, a.index, a.refresh, a.noise, a.margin) == (b.name, b.source, b.index, b.refresh, b.noise, b.margin)


def test_plan_chain_refuses_resident_outputs():
    from tfhe_fbs_map_amd.split import plan_chain
    env = _adder()
    prm, fuse = _key_params(env)
    _, fresh = _sources(prm)
    with pytest.raises(ValueError, match="another server key"):
        plan_chain(prm, fuse, bytes(8), env, [_resident(fp=bytes(range(8))), fresh], rename=A_FROM_S)
    with pytest.raises(ValueError, match="T = 4 samples where the others have 5"):
        plan_chain(prm, fuse, bytes(8), env, [_resident(T=5), fresh], rename=A_FROM_S)
    with pytest.raises(ValueError, match="saved without out_norm2"):
        plan_chain(prm, fuse, bytes(8), env, [_resident(out_norm2=None), fresh], rename=A_FROM_S)
    with pytest.raises(ValueError, match="closed"):
        plan_chain(prm, fuse, bytes(8), env, [_resident(closed=True), fresh], rename=A_FROM_S)
    with pytest.raises(ValueError, match="refresh would keep"):
        plan_chain(prm, fuse, bytes(8), env, [_resident(out_norm2=1e4), fresh], rename=A_FROM_S)


def test_resident_and_compact_together_are_refused():
    """resident state is full ciphertexts: the refusal comes before the server or the GPU is touched"""
    from tfhe_fbs_map_amd.split import ResidentOutputs, Server
    server = Server.__new__(Server)
    with pytest.raises(ValueError, match="resident outputs are full ciphertexts"):
        server.run_chain(None, [], resident=True, compact=True)
    closed = _resident(closed=True)
    assert closed.closed
    with pytest.raises(ValueError, match="closed"):
        closed.fetch()
    assert ResidentOutputs(["x"], 1, bytes(8), None, None).closed
