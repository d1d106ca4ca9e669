"""Audited evaluation on the GPU (include/fbs_exec.h "audited evaluation"; csrc/fbs_audit.hip; tfhe_fbs_map_amd/audit.py): the
errors and the statistics fbs_audit_level_dev returns at its four points, word for word against a numpy / Python-int restatement
made from the exported secret keys and the wire buffer read back; planted errors on both sides of half a box; the rotation input
against the decode of `compact_fields_dev`'s fields; an audited run leaves the evaluation as it was; a wrong expectation is found
where it was planted; the outputs of shared rotations; the refusals; and `LutExecEnv.audit` at a default 128-bit set.

In the hand-made programs every LinearProd and every Bootstrap is also an output: an output keeps its wire slot for good
(fbs_program_io_slots), which is how the restatement finds each audited wire in the buffer without knowing the planner."""
import numpy as np
import pytest

from tests.helpers import COMPACT_WIDE_SETS, load_fixture, subsample, toy_k2, toy_k3

pytestmark = pytest.mark.gpu

POINTS = ("inputs", "lincomb", "rotation_input", "bootstrap")


@pytest.fixture(scope="module")
def nat():
    from tfhe_fbs_map_amd import _native
    return _native


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def modulus():
    from tfhe_fbs_map_amd import MODULUS
    return int(MODULUS)


def delta_of(p):
    q = modulus()
    return 2 * ((q + 2 * p) // (4 * p))          # Delta = 2 delta_half, delta_half = round(q / 4p) (fbs_host.cpp)


def wire_errors(cts, sk_glwe, expected, p):
    """cts [..][D + 1] uint64, expected [..] any integers -> e = centred((b - <a, S> - Delta (expected mod 2p)) mod q), int64 [..]"""
    q = np.uint64(modulus())
    D = cts.shape[-1] - 1
    mask = np.asarray(sk_glwe).astype(bool)
    assert mask.size == D
    s = cts[..., :D][..., mask].sum(-1, dtype=np.uint64) % q        # at most 2048 words below 2^46: no overflow
    phase = (cts[..., D] + q - s) % q
    want = (np.mod(expected, 2 * p).astype(np.uint64) * np.uint64(delta_of(p))) % q
    x = ((phase + q - want) % q).astype(np.int64)
    return np.where(x > (modulus() - 1) // 2, x - modulus(), x)


def field_errors(fields, sk_lwe, expected, p, N):
    """fields [..][n + 1] uint32 at log2(2N) bits -> e = centred((2p ph - 2N m) mod 4pN), ph = body - <mask, s> mod 2N"""
    n = fields.shape[-1] - 1
    mask = np.asarray(sk_lwe).astype(bool)
    assert mask.size == n
    f = fields.astype(np.int64)
    ph = (f[..., n] - f[..., :n][..., mask].sum(-1)) % (2 * N)
    x = (2 * p * ph - 2 * N * np.mod(expected, 2 * p)) % (4 * p * N)
    return np.where(x >= 2 * p * N, x - 4 * p * N, x)


def stats_of(errors, over):
    """Python-int statistics of one row of errors; `over`: the half-box criterion"""
    e = [int(v) for v in errors]
    return dict(count=len(e), over=sum(1 for v in e if over(abs(v))), max_abs=max(abs(v) for v in e), sum=sum(e), sumsq=sum(v * v for v in e))


def wire_over(p):
    return lambda a: 4 * p * a >= modulus()


# ---- programs -------------------------------------------------------------------------------------------------------------------
def two_level_env():
    """a, b, c -> s1 = a + b, s2 = b + 2c | t = B(s1), u = B(s2) -> w = 2t + u + a | v = B(w) -> z = v + c + 1; all of them outputs"""
    from tfhe_fbs_map_amd import LutExecEnv
    env = LutExecEnv()
    a, b, c = env.input("a"), env.input("b"), env.input("c")
    s1, s2 = env.linear([1, 1], [a, b]), env.linear([1, 2], [b, c])
    t, u = env.bootstrap(s1, [0, 1, 1]), env.bootstrap(s2, [0, 1, 1, 0])
    w = env.linear([2, 1, 1], [t, u, a])
    v = env.bootstrap(w, [0, 1, 0, 1, 1])
    z = env.linear([1, 1], [v, c], 1)
    for name, node in (("s1", s1), ("s2", s2), ("t", t), ("u", u), ("w", w), ("v", v), ("z", z)):
        env.output(name, node)
    return env


def three_tables_env():
    """s = a + b + c read by three tables (they share one rotation when fused), u = B(a + 2b) alone on its source; all outputs"""
    from tfhe_fbs_map_amd import LutExecEnv
    env = LutExecEnv()
    a, b, c = env.input("a"), env.input("b"), env.input("c")
    s, r = env.linear([1, 1, 1], [a, b, c]), env.linear([1, 2], [a, b])
    x, y, z = env.bootstrap(s, [0, 1, 0, 1]), env.bootstrap(s, [0, 0, 1, 1]), env.bootstrap(s, [0, 1, 1, 0])
    u = env.bootstrap(r, [0, 1, 1, 0])
    for name, node in (("s", s), ("r", r), ("x", x), ("y", y), ("z", z), ("u", u), ("sum", env.linear([1, 2, 1, 1], [x, y, z, u]))):
        env.output(name, node)
    return env


class Stepped:
    """a loaded program on a wire buffer of torch's, inputs encrypted on the host with pinned nonces"""

    def __init__(self, nat, prm, env, T, fuse=False, seed=6):
        import torch
        from tfhe_fbs_map_amd.audit import cleartext_wires
        self.nat, self.prm, self.T, self.torch = nat, prm, T, torch
        self.ctx = nat.Context(prm, seed=seed)
        self.low = low = env.lower()
        self.prog = nat.Program(self.ctx, self.ctx.tvset(low["tables"]), len(low["input_names"]), low["kind"], low["arg0"], low["arg1"],
                                low["const_coef"], low["term_coef"], low["term_src"], low["out_wire"], fuse_tables=fuse)
        rng = np.random.default_rng(T)
        self.bits = rng.integers(0, 2, (len(low["input_names"]), T))
        self.cts = self.ctx.encrypt(self.bits, nonce0=9)
        self.clear = cleartext_wires(low, self.bits, prm.p_msg)
        keys = self.ctx.export_keys()
        self.sk_glwe, self.sk_lwe = keys["sk_glwe"], keys["sk_lwe"]
        self.slot_of = {i: int(s) for i, s in enumerate(self.prog.in_slot)}
        self.slot_of.update({int(w): int(s) for w, s in zip(low["out_wire"], self.prog.out_slot) if w >= 0})
        self.wires = None

    def load(self):
        torch = self.torch
        self.wires = torch.zeros((self.prog.n_slots, self.T, self.prm.ct_words), dtype=torch.int64, device="cuda")
        self.wires[torch.from_numpy(self.prog.in_slot.astype(np.int64)).cuda()] = torch.from_numpy(self.cts.view(np.int64)).cuda()
        torch.cuda.synchronize()

    def snapshot(self):
        self.ctx.sync()
        return self.wires.cpu().numpy().view(np.uint64)

    def audit(self, L, point, s_begin, s_count, expected=None, errors=True):
        """-> (wire ids, stats, errors) of one point over the sample window; expected: [rows][s_count], default the cleartext values"""
        torch = self.torch
        ids = self.prog.audit_rows(L, POINTS.index(point))
        want = self.clear[ids.astype(np.int64), s_begin:s_begin + s_count] if expected is None else expected
        d_want = torch.from_numpy(np.ascontiguousarray(want, np.int64)).cuda()
        torch.cuda.synchronize()
        stats, err = self.prog.audit_level_dev(L, POINTS.index(point), self.wires.data_ptr(), self.T, s_begin, s_count, d_want.data_ptr(),
                                               errors=errors)
        return ids, stats, err

    def fields_of(self, cts):
        """numpy: the log2(2N)-bit fields `compact_fields_dev` gives for ciphertexts [count][D + 1] (through `compact_dev`)"""
        torch, ctx = self.torch, self.ctx
        count, bits = cts.shape[0], ctx.default_compact_bits
        d_c = torch.from_numpy(np.ascontiguousarray(cts).view(np.int64)).cuda()
        d_w = torch.zeros((count, ctx.compact_words(bits)), dtype=torch.int64, device="cuda")
        d_f = torch.zeros((count, self.prm.n + 1), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.compact_dev(d_c.data_ptr(), count, d_w.data_ptr(), bits)
        ctx.compact_fields_dev(d_w.data_ptr(), count, d_f.data_ptr(), bits)
        ctx.sync()
        return d_f.cpu().numpy().view(np.uint32)

    def check(self, L, point, s_begin, s_count):
        """one point against the restatement, word for word: errors and statistics"""
        p, N = self.prm.p_msg, self.prm.N
        ids, stats, err = self.audit(L, point, s_begin, s_count)
        assert len(ids) == len(stats) == err.shape[0] and err.shape[1] == s_count
        buf = self.snapshot()
        want = self.clear[ids.astype(np.int64), s_begin:s_begin + s_count]
        cts = np.stack([buf[self.slot_of[int(w)], s_begin:s_begin + s_count] for w in ids])
        if point == "rotation_input":
            fields = self.fields_of(cts.reshape(-1, self.prm.ct_words)).reshape(len(ids), s_count, -1)
            ref = field_errors(fields, self.sk_lwe, want, p, N)
            over = lambda a: a >= N                                        # noqa: E731
        else:
            ref = wire_errors(cts, self.sk_glwe, want, p)
            over = wire_over(p)
        assert np.array_equal(err, ref), (point, L)
        for r, st in enumerate(stats):
            assert st == stats_of(ref[r], over), (point, L, r)
        return ids, stats, err

    def run(self, s_begin, s_count, points=POINTS, audited=None):
        """step the program over the window; at every point of `points`, `check`.  -> {(point, L): (ids, stats, errors)}"""
        prog, base, T = self.prog, self.wires.data_ptr(), self.T
        seen = {}

        def at(point, L):
            if point in points:
                seen[(point, L)] = (audited or self.check)(L, point, s_begin, s_count)

        at("inputs", 0)
        for L in range(prog.depth + 1):
            prog.level_lincomb_dev(L, base, T, s_begin, s_count)
            at("lincomb", L)
            if L == prog.depth:
                break
            at("rotation_input", L)
            prog.level_bootstrap_dev(L, base, T, s_begin, s_count, 0, prog.level_width[L] * s_count)
            at("bootstrap", L)
        return seen

    def close(self):
        self.prog.close()
        self.ctx.close()


def toy_set(which, toy_params):
    return {"k1_N1024": toy_params, "k3_N512": toy_k3(), "k2_N1024": toy_k2()}[which]


# ---- the wire kernel and the three wire points, exact ---------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [5, 67])
@pytest.mark.parametrize("which", ["k1_N1024", "k3_N512", "k2_N1024"])
def test_every_point_equals_the_restatement(nat, toy_params, which, T):
    """D = 1024, 1536 and 2048; whole range, a window that starts at 3, one sample; T = 67 puts more than one workgroup of four waves
    on every row and more than 64 samples through the reduction's lanes"""
    prm = toy_set(which, toy_params)
    st = Stepped(nat, prm, two_level_env(), T)
    assert st.prog.depth == 2
    for s_begin, s_count in ((0, T), (3, T - 3), (2, 1)):
        st.load()
        seen = st.run(s_begin, s_count)
        names = {(pt, L): len(v[0]) for (pt, L), v in seen.items()}
        assert names == {("inputs", 0): 3, ("lincomb", 0): 2, ("rotation_input", 0): 2, ("bootstrap", 0): 2, ("lincomb", 1): 1,
                         ("rotation_input", 1): 1, ("bootstrap", 1): 1, ("lincomb", 2): 1}
        # the toy sets are quiet: nothing comes near half a box, and the decode of the outputs is the cleartext
        assert all(s["over"] == 0 for v in seen.values() for s in v[1])
        out = st.ctx.decrypt(st.snapshot()[[st.slot_of[int(w)] for w in st.low["out_wire"]], s_begin:s_begin + s_count])
        assert np.array_equal(out, np.mod(st.clear[st.low["out_wire"], s_begin:s_begin + s_count], 2 * prm.p_msg))
    st.close()


def test_audit_rows_names_the_wires(nat, toy_params):
    st = Stepped(nat, toy_params, two_level_env(), 2)
    low, n_in = st.low, 3
    lin = [n_in + i for i, k in enumerate(low["kind"]) if k == 0]
    boot = [n_in + i for i, k in enumerate(low["kind"]) if k == 1]
    assert st.prog.audit_rows(5, 0).tolist() == [0, 1, 2]                                   # inputs: the level is ignored
    assert [st.prog.audit_rows(L, 1).tolist() for L in range(3)] == [lin[:2], lin[2:3], lin[3:]]
    assert [st.prog.audit_rows(L, 2).tolist() for L in range(2)] == [lin[:2], lin[2:3]]     # the sources
    assert [st.prog.audit_rows(L, 3).tolist() for L in range(2)] == [boot[:2], boot[2:]]
    st.close()


# ---- planted errors ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [7, 4096])
def test_planted_errors_flip_over_exactly_at_half_a_box(nat, toy_params, p):
    """trivial ciphertexts (zero mask) with chosen bodies in the input slots: 0, +-1, +-(q - 1)/2 and the two integers either side of
    4p |e| = q, on both signs; the sum of squares needs its high word; expected values outside [0, 2p) are taken mod 2p"""
    q = modulus()
    prm = toy_params.replace(p_msg=p)
    edge = -(-q // (4 * p))                                                                  # the least |e| with 4p |e| >= q
    errs = [0, 1, -1, (q - 1) // 2, -(q - 1) // 2, edge - 1, edge, -(edge - 1), -edge, 12345, -(1 << 44)]
    T = len(errs)
    st = Stepped(nat, prm, two_level_env(), T)
    st.load()
    msgs = np.array([[(3 * s + 5 * i) % (2 * p) for s in range(T)] for i in range(3)])
    planted = np.array([[e + 7 * i * (e == 12345) for e in errs] for i in range(3)], dtype=object)     # row i differs in one sample
    cts = np.zeros((3, T, prm.ct_words), np.uint64)
    for i in range(3):
        for s in range(T):
            cts[i, s, -1] = (delta_of(p) * int(msgs[i, s]) + int(planted[i, s])) % q
    st.wires[st.torch.from_numpy(st.prog.in_slot.astype(np.int64)).cuda()] = st.torch.from_numpy(cts.view(np.int64)).cuda()
    shifted = msgs + np.array([[2 * p * ((s % 5) - 2) for s in range(T)] for _ in range(3)])      # negative and >= 2p, the same mod 2p
    for want in (msgs, shifted):
        ids, stats, err = st.audit(0, "inputs", 0, T, expected=want)
        assert err.astype(object).tolist() == planted.tolist()
        for i, s in enumerate(stats):
            ref = stats_of(planted[i], wire_over(p))
            assert s == ref, (i, s, ref)
            # over: +-(q - 1)/2, +-edge and -2^44 (beyond half a box at either p); not edge - 1, not 12345
            assert s["over"] == 5 and s["sumsq"] >> 64 > 0 and s["max_abs"] == (q - 1) // 2
    assert 4 * p * (edge - 1) < q <= 4 * p * edge
    # the window: only the two samples either side of the boundary
    _, stats, err = st.audit(0, "inputs", 5, 2, expected=msgs[:, 5:7])
    assert [s["over"] for s in stats] == [1, 1, 1] and err[:, 0].tolist() == [edge - 1] * 3 and err[:, 1].tolist() == [edge] * 3
    st.close()


# ---- the rotation input, exact -------------------------------------------------------------------------------------------------------
def test_rotation_input_at_a_real_key_size_and_planted_expectations(nat):
    """n = 734: 735 fields, eleven passes of 64 lanes and a ragged twelfth; T = 4.  The errors are the decode, under the exported
    small key, of what `compact_fields_dev` returns for the same source ciphertexts; expected values shifted by multiples of 2p
    (negative ones too) give the same errors, and a message off by one moves every error by one box, 2N units."""
    from tfhe_fbs_map_amd import Params
    prm = Params(**COMPACT_WIDE_SETS["n734"])
    p, N, T = prm.p_msg, prm.N, 4
    st = Stepped(nat, prm, two_level_env(), T)
    assert prm.n == 734 and (prm.n + 1) % 64 != 0
    st.load()
    seen = st.run(0, T, points=("rotation_input",))
    (ids, stats, err) = seen[("rotation_input", 0)]
    assert err.shape == (2, T)
    # level 0 again, with other expectations: the audit leaves the wires as they are, so it can be asked twice
    st.load()
    st.prog.level_lincomb_dev(0, st.wires.data_ptr(), T, 0, T)
    want = st.clear[ids.astype(np.int64)]
    shift = np.array([[-2 * p, 4 * p, 0, -6 * p], [2 * p, -4 * p, 8 * p, 0]])
    _, stats2, err2 = st.audit(0, "rotation_input", 0, T, expected=want + shift)
    assert np.array_equal(err2, err) and stats2 == stats
    _, _, err3 = st.audit(0, "rotation_input", 0, T, expected=want + 1)
    box = 4 * p * N
    assert np.array_equal((err3 - err) % box, np.full_like(err, box - 2 * N))
    assert np.all((err3 >= -box // 2) & (err3 < box // 2))
    st.close()


# ---- no disturbance -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["adder8__search_p7", "edge_outputs"])
def test_an_audited_run_is_the_evaluation_and_repeats(nat, toy_params, name):
    """a program whose wire slots are reused (the goldens), audited at all four points: the output ciphertexts are `Program.eval`'s
    word for word, and a second audited run returns the same statistics and errors"""
    from tfhe_fbs_map_amd import parse_fbs
    rec = load_fixture(name)
    T = 6
    env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
    st = Stepped(nat, toy_params, env, T)
    st.bits = np.stack([subsample(rec, T)[0][n] for n in st.low["input_names"]])
    st.cts = st.ctx.encrypt(st.bits, nonce0=9)
    from tfhe_fbs_map_amd.audit import cleartext_wires
    st.clear = cleartext_wires(st.low, st.bits, toy_params.p_msg)
    ref = st.prog.eval(st.cts, T)
    runs = []
    for _ in range(2):
        st.load()
        runs.append(st.run(0, T, audited=lambda L, point, s0, n: st.audit(L, point, s0, n)))
        got = st.snapshot()
        for k, slot in enumerate(st.prog.out_slot.tolist()):
            if slot >= 0:
                assert np.array_equal(got[slot], ref[k]), st.low["out_names"][k]
    assert runs[0].keys() == runs[1].keys() and len(runs[0]) >= 4
    for key in runs[0]:
        (ids0, stats0, err0), (ids1, stats1, err1) = runs[0][key], runs[1][key]
        assert np.array_equal(ids0, ids1) and stats0 == stats1 and np.array_equal(err0, err1), key
        assert all(s["over"] == 0 and s["count"] == T for s in stats0), key
    if name.startswith("adder8"):
        assert st.prog.n_slots < len(st.low["kind"]) + len(st.low["input_names"])      # slots were reused
    st.close()


# ---- a wrong expectation ---------------------------------------------------------------------------------------------------------------
def test_a_wrong_expectation_is_found_where_it_was_planted(nat, toy_params, monkeypatch):
    from tfhe_fbs_map_amd import ExecConfig, audit
    env = two_level_env()
    low = env.lower()
    T, victim, flipped = 9, 3 + 3, (1, 4, 8)                  # wire 6: the second Bootstrap of level 0 ("u")
    assert low["kind"][victim - 3] == 1
    honest = audit.cleartext_wires

    def flipping(low_, bits, p):
        wires = honest(low_, bits, p)
        wires[victim, list(flipped)] += 1                     # the gate's own expectation only: nothing downstream moves
        return wires

    rng = np.random.default_rng(3)
    ins = {n: rng.integers(0, 2, T) for n in low["input_names"]}
    cfg = ExecConfig(fbs_size=7, params=toy_params, seed=4, nonce0=77)
    clean = env.audit(ins, config=cfg, points=POINTS)
    assert clean.failures == 0 and clean.first_failure is None
    monkeypatch.setattr(audit, "cleartext_wires", flipping)
    report = env.audit(ins, config=cfg, points=POINTS)
    bad = [r for r in report.rows if r.over]
    assert len(bad) == 1 and bad[0].over == 3 and bad[0].wire == victim and bad[0].point == "bootstrap" and bad[0].level == 0
    first = report.first_failure
    assert first is bad[0] and first.name == audit.wire_names(env)[victim] and report.failures == 3
    assert first.worst > 1.0 and report.min_margin == first.margin
    for name, v in clean.outputs.items():                      # the evaluation itself is the same
        assert np.array_equal(report.outputs[name], v)


# ---- shared rotations -------------------------------------------------------------------------------------------------------------------
def test_the_outputs_of_a_shared_rotation_are_audited(nat, toy_params):
    """FBS_LOAD_FUSE_TABLES, three tables on one source: one rotation of TV_0, three extractions -- the bootstrap point reports the
    level's own rotation first, then the three cut from the shared one, all equal to the restatement"""
    T = 5
    st = Stepped(nat, toy_params, three_tables_env(), T, fuse=True)
    assert st.prog.fused and st.prog.n_rotations == 2 and st.prog.n_bootstrap == 4
    st.load()
    seen = st.run(0, T)
    ids, stats, _ = seen[("bootstrap", 0)]
    low = st.low
    boots = [3 + i for i, k in enumerate(low["kind"]) if k == 1]                 # x, y, z, u
    assert ids.tolist() == [boots[3]] + boots[:3]
    assert len(seen[("rotation_input", 0)][0]) == 2 and all(s["over"] == 0 and s["count"] == T for s in stats)
    out = st.ctx.decrypt(st.snapshot()[[st.slot_of[int(w)] for w in low["out_wire"]]])
    assert np.array_equal(out, st.clear[low["out_wire"]])
    st.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_working(nat, toy_params):
    import torch
    T = 3
    st = Stepped(nat, toy_params, two_level_env(), T)
    st.load()
    base = st.wires.data_ptr()
    want = torch.zeros((8, T), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def code(*args, **kw):
        with pytest.raises(nat.FbsError) as e:
            st.prog.audit_level_dev(*args, **kw)
        return e.value.code

    depth = st.prog.depth
    assert code(depth + 1, nat.AUDIT_LINCOMB, base, T, 0, T, want.data_ptr()) == -1
    assert code(depth, nat.AUDIT_BOOTSTRAP, base, T, 0, T, want.data_ptr()) == -1            # bootstraps: levels [0, depth)
    assert code(depth, nat.AUDIT_ROTATION_INPUT, base, T, 0, T, want.data_ptr()) == -1
    assert code(0, 7, base, T, 0, T, want.data_ptr()) == -1
    assert code(0, nat.AUDIT_INPUTS, base, T, 2, 2, want.data_ptr()) == -1                   # window past T
    assert code(0, nat.AUDIT_INPUTS, 0, T, 0, T, want.data_ptr()) == -1                      # null pointers with work to do
    assert code(0, nat.AUDIT_INPUTS, base, T, 0, T, 0) == -1
    with pytest.raises(nat.FbsError) as e:
        st.prog.audit_rows(depth + 1, nat.AUDIT_LINCOMB)
    assert e.value.code == -1
    assert st.prog.audit_level_dev(0, nat.AUDIT_INPUTS, 0, T, 0, 0, 0) == ([], None)         # s_count = 0 does nothing
    st.run(0, T)                                                                             # ... and the context works
    st.close()

    # no secret, no audit
    client = nat.Context(toy_params, seed=8, keygen=False)
    client.keygen_seeded()
    server = nat.Context.evaluation_only(toy_params, **client.export_seeded_keys())
    low = two_level_env().lower()
    prog = nat.Program(server, server.tvset(low["tables"]), 3, low["kind"], low["arg0"], low["arg1"], low["const_coef"], low["term_coef"],
                       low["term_src"], low["out_wire"])
    wires = torch.zeros((prog.n_slots, T, toy_params.ct_words), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(nat.FbsError) as e:
        prog.audit_level_dev(0, nat.AUDIT_INPUTS, wires.data_ptr(), T, 0, T, want.data_ptr())
    assert e.value.code == -3
    prog.level_lincomb_dev(0, wires.data_ptr(), T, 0, T)                                     # the evaluation-only context still evaluates
    server.sync()
    prog.close()
    server.close()
    client.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def test_audit_of_a_golden_at_its_default_128_bit_set(nat):
    """`LutExecEnv.audit` of adder8__search_p7 at the set `ExecConfig` chooses, T = 64: the golden outputs, no failure, every
    rotation input further from half a box than the margin asked for would put it at 4 sigma (the measurement is of 64 samples a row:
    it is the model that promises 6), and the pooled noise of the bootstrap outputs (gates x 64 samples) in the band
    tests/test_gpu_parity.py::test_noise_model_holds_for_the_secure_set holds the same quantity to against variances(prm)[0].
    fuse_tables=False: every output is then one blind rotation's, which is what that band is about."""
    from tfhe_fbs_map_amd import ExecConfig, parse_fbs
    from tfhe_fbs_map_amd.params import margin_sigmas, security_bits, variances
    rec = load_fixture("adder8__search_p7")
    T = 64
    ins, expect = subsample(rec, T)
    env = parse_fbs(rec["fbs"], inputs=rec["program_inputs"])
    cfg = ExecConfig(seed=11, nonce0=500, fuse_tables=False)
    report = env.audit(ins, config=cfg, points=("rotation_input", "bootstrap"), chunk=24)      # three chunks, the last ragged
    prm = report.params
    assert security_bits(prm) >= 127.9 and margin_sigmas(prm, env.stats()["norm2_linprod"]) >= 6.0
    for k, v in expect.items():
        assert np.array_equal(report.outputs[k], v), k
    assert report.failures == 0 and report.first_failure is None
    boots = [r for r in report.rows if r.point == "bootstrap"]
    rots = [r for r in report.rows if r.point == "rotation_input"]
    assert len(boots) == env.stats()["nb_bootstrap"] and all(r.count == T for r in report.rows)
    assert len(boots) * T >= 300
    q = modulus()
    pooled = (sum(r.sumsq for r in boots) / sum(r.count for r in boots)) ** 0.5 / q
    predicted = variances(prm)[0] ** 0.5
    print("bootstrap outputs: measured %.4g predicted %.4g; min margin %.2f (model %.2f)" % (
        pooled, predicted, report.min_margin, min(r.model_margin for r in rots)))
    assert 0.5 * predicted < pooled < 1.25 * predicted, (pooled, predicted)
    assert all(r.worst < 1.0 for r in report.rows)
    # the same evaluation as eval's: the same nonces, the same outputs
    got = env.eval(ins, config=cfg)
    for k, v in expect.items():
        assert np.array_equal(got[k], v), k
    assert "min margin" in report.summary() and len(report.worst(10)) == 10
