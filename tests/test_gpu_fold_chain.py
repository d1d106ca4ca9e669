"""Folded state through the Python layer on the GPU (tfhe_fbs_map_amd/split.py): a client that keys for folding, a server that
folds resident outputs, links them into the next hop unrefreshed, restores them and hands them over through a file -- the adder8
accumulator of tests/test_gpu_resident.py at its default 128-bit set with its state folded between hops, against the resident
chain and the cleartext."""
import numpy as np
import pytest

from oracle import lut_oracle
from tests.helpers import load_fixture
from tests.test_gpu_resident import A_FROM_S, ADDER, B_NAMES, _hop_inputs, _same

pytestmark = pytest.mark.gpu
_SETUP = {}


def _setup():
    """the adder8 client and server of the resident tests, keyed for folding too; made once per module"""
    if not _SETUP:
        from tfhe_fbs_map_amd import Client, ExecConfig, Server, parse_fbs
        rec = load_fixture(ADDER)
        env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
        client = Client(env, ExecConfig(seed=7), programs=[env], folding=True)
        _SETUP.update(rec=rec, env=env, client=client, server=Server(client.server_key()))
    return _SETUP["rec"], _SETUP["env"], _SETUP["client"], _SETUP["server"]


def test_the_client_keys_for_folding_at_the_choice_of_the_noise_model():
    from tfhe_fbs_map_amd.params import fold_choice, folded_state_factor
    _, env, client, server = _setup()
    prm = client.params
    assert (prm.k, prm.N) == (2, 1024)                                             # adder8's default 128-bit set
    norm2 = env.stats()["norm2_linprod"]
    assert client.folding == fold_choice(prm, norm2, 6.0) and client.folding[0] == 1
    key = client.server_key()
    assert (key.fold_levels, key.fold_base_bits) == client.folding and key.fold_bodies.size == prm.k * prm.N * prm.N
    assert key.fold_factor == folded_state_factor(prm, *client.folding) < 0.03
    assert (server.ctx.stat("fold_key"), server.ctx.stat("fold_levels"), server.ctx.stat("fold_base_bits")) == (1,) + client.folding
    assert server.ctx.stat("has_secret") == 0


def test_adder8_accumulator_with_its_state_folded_between_hops(tmp_path):
    """acc <- acc + b, two hops at T = 16: the state is folded after every evaluation and the rows are freed; the next hop links the
    folded state unrefreshed.  Hop 1 takes it from the card, hop 2 from a file.  Every hop decrypts to what the resident chain
    decrypts to, and to the cleartext."""
    from tfhe_fbs_map_amd.split import FoldedOutputs, ResidentOutputs, folded_words, plan_chain
    T_ = 16
    rec, env, client, server = _setup()
    prm = client.params
    rng = np.random.default_rng(1)
    first = {**{f"a{i}": rng.integers(0, 2, T_) for i in range(8)}, **_hop_inputs(rng, T_)}
    acc = server.run(env, client.encrypt(first), resident=True)                     # the resident chain, beside the folded one
    clear = lut_oracle.eval_fbs_text(rec["fbs"], first)
    folded = acc.fold(device=True)
    assert isinstance(folded, FoldedOutputs) and folded.on_device and folded.words.numel() == folded_words(prm, 9 * T_)
    assert folded.fold_factor == client.server_key().fold_factor and np.array_equal(folded.out_norm2, acc.out_norm2)
    assert np.array_equal(folded.host_words(), acc.fold().words)                    # on the card = through the host
    _same(client.decrypt(folded), clear, T_, "first, folded")
    assert 8 * folded.words.numel() == 24576 and acc.state.rows * T_ * prm.ct_words * 8 == 2360448   # 144 bits: one sample for 2.4 MB of rows
    for hop in range(2):
        fresh = _hop_inputs(rng, T_)
        ins = client.encrypt(fresh, names=B_NAMES)
        links, _ = plan_chain(prm, server.key.fuse_tables, server.key.fingerprint, env, [folded, ins], rename=A_FROM_S)
        assert all(ln.kind == "folded" and not ln.refresh for ln in links[:8])
        alive = server.ctx.stat("states_alive")
        nxt_folded_src = server.run_chain(env, [folded, ins], rename=A_FROM_S, resident=True)
        assert server.ctx.stat("states_alive") == alive + 1                         # the temporary state of the unfold is gone
        nxt = server.run_chain(env, [acc, ins], rename=A_FROM_S, resident=True)
        acc.close()
        acc = nxt
        assert isinstance(nxt_folded_src, ResidentOutputs) and nxt_folded_src.T == T_
        clear = lut_oracle.eval_fbs_text(rec["fbs"], {**{f"a{i}": np.broadcast_to(clear[f"s{i}"], (T_,)) for i in range(8)}, **fresh})
        want = client.decrypt(acc.fetch())
        _same(want, clear, T_, hop)
        _same(client.decrypt(nxt_folded_src.fetch()), want, T_, (hop, "folded link"))
        assert nxt_folded_src.out_norm2.max() >= acc.out_norm2.max()                # the fold's factor is counted in what comes out
        folded = nxt_folded_src.fold(device=(hop == 1))
        nxt_folded_src.close()
        _same(client.decrypt(folded), want, T_, (hop, "folded"))
        if hop == 0:                                                                # handed over through a file
            folded.save(str(tmp_path / "state.npz"))
            folded = FoldedOutputs.load(str(tmp_path / "state.npz"))
            assert not folded.on_device
    # restore: back into rows on the card, from the host words and from the card
    for src in (folded, FoldedOutputs(folded.output_names, T_, folded.host_words(), folded.fingerprint, folded.out_norm2, folded.fold_factor)):
        with server.restore(src) as back:
            assert isinstance(back, ResidentOutputs) and np.allclose(back.out_norm2, folded.out_norm2 + folded.fold_factor)
            _same(client.decrypt(back.fetch()), want, T_, "restored")
    acc.close()
    assert server.ctx.stat("states_alive") == 0


def test_the_temporary_state_is_freed_when_the_evaluation_raises(monkeypatch):
    T_ = 4
    rec, env, client, server = _setup()
    rng = np.random.default_rng(2)
    first = {**{f"a{i}": rng.integers(0, 2, T_) for i in range(8)}, **_hop_inputs(rng, T_)}
    with server.run(env, client.encrypt(first), resident=True) as acc:
        folded = acc.fold()
    assert server.ctx.stat("states_alive") == 0

    def boom(*a, **k):
        raise RuntimeError("on request")
    monkeypatch.setattr(server, "_run_links", boom)
    with pytest.raises(RuntimeError, match="on request"):
        server.run_chain(env, [folded, client.encrypt(_hop_inputs(rng, T_), names=B_NAMES)], rename=A_FROM_S)
    assert server.ctx.stat("states_alive") == 0
    # a server key without a fold key says what is missing
    from tfhe_fbs_map_amd import Client, ExecConfig, Server
    plain_client = Client(env, ExecConfig(seed=7), programs=[env])
    assert plain_client.folding is None and plain_client.server_key().fold_bodies is None
    plain = Server(plain_client.server_key())
    with plain.run(env, plain_client.encrypt(first), resident=True) as acc:
        with pytest.raises(ValueError, match="fold key"):
            acc.fold()
    plain.ctx.close()
    plain_client.ctx.close()
