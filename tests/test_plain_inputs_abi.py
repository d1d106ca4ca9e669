"""Plaintext server inputs without a GPU (include/fbs_exec.h, "chained evaluation", FBS_SRC_PLAIN): the kind is defined and the
section's comment names it; `PlainInputs` round-trips through .npz and refuses what it must; `plan_chain` links a plain source
beside a seeded one (noise 0, no refresh, no fingerprint asked), with the ambiguity, T and all-broadcast rules; and a plain link's
noise 0 gives the output factors of a fresh input."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDER = "adder8__search_p7"
A_NAMES = [f"a{i}" for i in range(8)]
B_NAMES = [f"b{i}" for i in range(8)]


def test_the_header_defines_the_kind_and_its_section_names_it():
    text = open(os.path.join(ROOT, "include", "fbs_exec.h")).read()
    assert re.search(r"^#define FBS_SRC_PLAIN 3u\b", text, re.M)
    kinds = dict(re.findall(r"^#define (FBS_SRC_\w+) (\d+)u", text, re.M))
    assert kinds == {"FBS_SRC_SEEDED": "0", "FBS_SRC_FULL": "1", "FBS_SRC_COMPACT": "2", "FBS_SRC_PLAIN": "3"}
    section = text[text.index("/* ---- chained evaluation"):text.index("/* ---- resident state")]
    comment = section[:section.index("*/")]
    assert "FBS_SRC_PLAIN" in comment and "trivial ciphertext" in comment
    resident = text[text.index("/* fbs_eval_sources with two additions."):text.index("int fbs_eval_resident(")]
    assert "FBS_SRC_PLAIN" in resident
    from tfhe_fbs_map_amd import _native
    assert _native.SRC_PLAIN == 3
    assert "fbs_eval_sources" in _native.EXPORTED_SYMBOLS and not any("plain" in s for s in _native.EXPORTED_SYMBOLS)


def test_plain_inputs_round_trip(tmp_path):
    from tfhe_fbs_map_amd.split import EncryptedInputs, PlainInputs
    rng = np.random.default_rng(0)
    per_sample = PlainInputs(B_NAMES, 5, rng.integers(0, 2, (8, 5)))
    broadcast = PlainInputs(B_NAMES, None, rng.integers(0, 2, 8))
    mixed = PlainInputs(["x", "y", "z"], 4, {"z": 1, "x": np.array([0, 1, 1, 0]), "y": 0})
    for obj in (per_sample, broadcast, mixed):
        path = str(tmp_path / "p.npz")
        obj.save(path)
        with np.load(path, allow_pickle=False) as z:
            assert str(z["kind"]) == "plain_inputs" and "fingerprint" not in z.files
        back = PlainInputs.load(path)
        assert back.input_names == obj.input_names and back.T == obj.T
        assert back.values.dtype == np.int64 and np.array_equal(back.values, obj.values) and np.array_equal(back.broadcast, obj.broadcast)
    assert not hasattr(per_sample, "fingerprint")
    assert broadcast.T is None and broadcast.values.shape == (8,) and isinstance(broadcast.row(3), int)
    assert np.array_equal(per_sample.row(2), per_sample.values[2]) and per_sample.row(2).dtype == np.int64
    assert (mixed.row(0).tolist(), mixed.row(1), mixed.row(2)) == ([0, 1, 1, 0], 0, 1)
    assert PlainInputs(B_NAMES, 7, np.ones(8, np.int64)).T == 7      # one value each, T given
    # a file of another kind, and a wrong version, dtype or shape
    path = str(tmp_path / "p.npz")
    EncryptedInputs(B_NAMES, 5, 0, np.zeros((8, 5), np.uint64), bytes(8)).save(path)
    with pytest.raises(ValueError, match="not a saved plain_inputs"):
        PlainInputs.load(path)
    per_sample.save(path)
    with pytest.raises(ValueError, match="not a saved encrypted_inputs"):
        EncryptedInputs.load(path)
    good = dict(kind=np.array("plain_inputs"), format_version=np.array(1), input_names=np.array(B_NAMES), T=np.array(5, np.int64),
                values=np.zeros((8, 5), np.int64), broadcast=np.zeros(8, bool))
    np.savez(path, **good)
    assert PlainInputs.load(path).T == 5
    for change, text in ((dict(format_version=np.array(2)), "format version"),
                         (dict(values=np.zeros((8, 5), np.uint64)), "type uint64"),
                         (dict(values=np.zeros((8, 5), np.float64)), "type float64"),
                         (dict(values=np.zeros((8, 4), np.int64)), r"shape \(8, 4\)"),
                         (dict(values=np.zeros((7, 5), np.int64)), r"shape \(7, 5\)"),
                         (dict(values=np.zeros((8, 5, 1), np.int64)), r"shape \(8, 5, 1\)"),
                         (dict(values=np.zeros(8, np.int64)), "one value each"),
                         (dict(broadcast=np.zeros(8, np.uint8)), "mask of type uint8"),
                         (dict(broadcast=np.zeros(9, bool)), "mask of shape"),
                         (dict(T=np.array(-1, np.int64)), "for 8 inputs of None samples")):
        np.savez(path, **{**good, **change})
        with pytest.raises(ValueError, match=text):
            PlainInputs.load(path)
    # values outside what Client.encrypt admits: inputs are bits
    for bad in (2, -1):
        with pytest.raises(ValueError, match="bits"):
            PlainInputs(B_NAMES, 5, np.full((8, 5), bad))
        with pytest.raises(ValueError, match="bits"):
            PlainInputs(B_NAMES, None, {n: bad for n in B_NAMES})
    with pytest.raises(ValueError, match="integers"):
        PlainInputs(B_NAMES, 5, np.full((8, 5), 0.5))
    with pytest.raises(ValueError, match="other inputs"):
        PlainInputs(B_NAMES, None, {n: 0 for n in A_NAMES})
    with pytest.raises(ValueError, match="need T"):
        PlainInputs(["x"], None, {"x": np.array([0, 1])})
    with pytest.raises(ValueError, match="twice"):
        PlainInputs(["x", "x"], None, [0, 1])


def _adder():
    from tests.helpers import load_fixture
    from tfhe_fbs_map_amd import ExecConfig, parse_fbs
    from tfhe_fbs_map_amd.split import client_choice
    rec = load_fixture(ADDER)
    env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
    assert sorted(env.lower()["input_names"]) == sorted(A_NAMES + B_NAMES)
    return (env,) + tuple(client_choice(env, ExecConfig()))


def _seeded(names, T, fp=bytes(8)):
    from tfhe_fbs_map_amd.split import EncryptedInputs
    return EncryptedInputs(list(names), T, 100, np.zeros((len(names), T), np.uint64), fp)


def test_plan_chain_links_a_plain_source():
    """(fails before PlainInputs exists: plan_chain then raises TypeError for the source)"""
    from tfhe_fbs_map_amd.split import PlainInputs, plan_chain
    env, prm, fuse = _adder()
    fp = bytes(range(8))
    a = _seeded(A_NAMES, 4, fp)
    b = PlainInputs(B_NAMES, 4, np.ones((8, 4), np.int64))
    links, T = plan_chain(prm, fuse, fp, env, [a, b])
    assert T == 4 and [ln.name for ln in links] == env.lower()["input_names"]
    by_name = {ln.name: ln for ln in links}
    for i in range(8):
        la, lb = by_name[f"a{i}"], by_name[f"b{i}"]
        assert (la.kind, la.source, la.index, la.refresh, la.noise) == ("seeded", 0, i, False, 0.0)
        assert (lb.kind, lb.source, lb.index, lb.refresh, lb.noise, lb.margin) == ("plain", 1, i, False, 0.0, None)
    # a name held by both sources is ambiguous
    with pytest.raises(ValueError, match="ambiguous"):
        plan_chain(prm, fuse, fp, env, [_seeded(A_NAMES + ["b3"], 4, fp), b])
    with pytest.raises(ValueError, match="ambiguous"):
        plan_chain(prm, fuse, fp, env, [a, b, PlainInputs(["b0"], None, [1])])
    with pytest.raises(ValueError, match="no source holds"):
        plan_chain(prm, fuse, fp, env, [a, PlainInputs(B_NAMES[:7], 4, np.ones((7, 4), np.int64))])
    # a T mismatch is refused
    with pytest.raises(ValueError, match="T = 5 samples where the others have 4"):
        plan_chain(prm, fuse, fp, env, [a, PlainInputs(B_NAMES, 5, np.ones((8, 5), np.int64))])
    with pytest.raises(ValueError, match="T = 5 samples where the others have 4"):
        plan_chain(prm, fuse, fp, env, [a, PlainInputs(B_NAMES, 5, np.ones(8, np.int64))])
    # a broadcast-only source takes the chain's T, in either order of the sources
    once = PlainInputs(B_NAMES, None, {n: i % 2 for i, n in enumerate(B_NAMES)})
    for sources in ([a, once], [once, a]):
        links, T = plan_chain(prm, fuse, fp, env, sources)
        assert T == 4 and sorted(ln.kind for ln in links) == ["plain"] * 8 + ["seeded"] * 8
    # per-sample plain inputs alone give the chain its T; an all-broadcast chain has none and is refused
    links, T = plan_chain(prm, fuse, fp, env, [PlainInputs(A_NAMES, 3, np.zeros((8, 3), np.int64)), once])
    assert T == 3 and all(ln.kind == "plain" for ln in links)
    with pytest.raises(ValueError, match="has no T"):
        plan_chain(prm, fuse, fp, env, [PlainInputs(A_NAMES, None, np.zeros(8, np.int64)), once])
    # a plain source belongs to no key; the seeded one beside it still has to be the key's
    with pytest.raises(ValueError, match="source 0 was computed under another server key"):
        plan_chain(prm, fuse, bytes(8), env, [a, b])
    # the wording of the TypeError: as before, with the new name at the end
    with pytest.raises(TypeError, match="not EncryptedInputs, EncryptedOutputs, CompactOutputs or ResidentOutputs.*PlainInputs$"):
        plan_chain(prm, fuse, fp, env, [a, {"b0": 1}])


def test_a_plain_link_is_noise_free_like_a_fresh_input():
    from tfhe_fbs_map_amd import parse_fbs
    from tfhe_fbs_map_amd.split import PlainInputs, output_noise_factors, plan_chain
    env, prm, fuse = _adder()
    low, p = env.lower(), prm.p_msg
    fp = bytes(8)
    links, _ = plan_chain(prm, fuse, fp, env, [_seeded(A_NAMES, 2, fp), PlainInputs(B_NAMES, None, np.zeros(8, np.int64))])
    for f in (False, True):
        assert output_noise_factors(low, p, f, [ln.noise for ln in links]) == output_noise_factors(low, p, f)
    # a plain input wired to an output, and one under a linear combination: recorded as noise-free
    through = parse_fbs("m1 = 2 * a + 1 * b\nm2 = Bootstrap(m1, [0, 1, 0, 1])\nOutput pa = a\nOutput s = m1\nOutput t = m2\n", inputs=["a", "b"]).lower()
    assert output_noise_factors(through, p, False, [0.0, 0.0]) == [0.0, 0.0, 1.0] == output_noise_factors(through, p)
    assert output_noise_factors(through, p, False, [0.0, 1.0]) == [0.0, 1.0, 1.0]
