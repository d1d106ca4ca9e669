"""Audited evaluation: run a program as `LutExecEnv.eval` runs it and MEASURE, gate by gate, the noise the parameter choice is
about (include/fbs_exec.h, "audited evaluation"; DESIGN.md section 4, "Audited evaluation").

Every claim of correctness rests on `params.margin_sigmas`: the phase that enters a blind rotation has variance
norm2 v_br + v_ks + v_ms, and the half box 1/(4p) must lie `min_margin` standard deviations away.  The audit measures that
quantity where it is defined -- on the modulus-switched fields the rotation reads (point "rotation_input") -- and, when asked, on
the big-key ciphertexts of the inputs, of the LinearProds and of the Bootstrap outputs.  The errors are exact integers computed on
the GPU under the secret keys the context keeps there (fbs_audit.hip); only six words of statistics per audited row come back, and
they are accumulated here in Python ints.

Three pieces, the first two of which need neither GPU nor library:
  cleartext_wires      the integer every program wire holds, per sample -- what each ciphertext is compared with
  predicted_variance   the model's variance per wire (`params.variances`)
  run_audit            the stepper behind `LutExecEnv.audit`; returns an `AuditReport`
"""
from __future__ import annotations

import json
import math
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np

from .fbs_exec_env import min_fbs_size, table_fusion_factor, table_is_valid
from .security import MODULUS

POINTS = ("inputs", "lincomb", "rotation_input", "bootstrap")   # FBS_AUDIT_* in this order; also the order within a level


# --------------------------------------------------------------------------------------------
# cleartext semantics
# --------------------------------------------------------------------------------------------
def table_lookup(table, p, x):
    """What one functional bootstrap at plaintext modulus p returns for the integer(s) x -- the contract of the test vector the
    encrypted path builds (`host_build_tv`, fbs_host.cpp): with L = len(table) <= 2p, f(i) = table[i] for i < L and 0 for the
    unreachable slots L <= i < p, and c = table[0] + table[p] when L > p (`table_is_valid`: table[i] + table[i + p] = c throughout)
    and 0 otherwise, the polynomial carries (2 f - c) Delta/2 on box i < p, its negacyclic extension the negative of that on box
    i + p, and c Delta/2 is added after the extraction: y = x mod 2p gives f(y) for y < p and c - f(y - p) for y >= p."""
    if not table_is_valid(table, p):
        raise ValueError("table %s cannot be evaluated by one bootstrap at fbs_size %d" % (list(table), p))
    L = len(table)
    c = int(table[0]) + int(table[p]) if L > p else 0
    f = np.zeros(p, np.int64)
    f[:min(L, p)] = np.asarray(table[:p], np.int64)
    y = np.mod(np.asarray(x, np.int64), 2 * p)
    return np.where(y < p, f[np.minimum(y, p - 1)], c - f[np.maximum(y - p, 0)])


def cleartext_wires(low, bits, p):
    """The integer value of every wire of the lowered program `low` (`LutExecEnv.lower()`) for every sample: bits [n_inputs][T]
    (or a dict name -> array) -> np.ndarray int64 [n_inputs + n_instr][T], wire ids as in fbs_program_desc (inputs, then
    instructions).  LinearProds are plain integer sums (not reduced: a ciphertext holds the value mod 2p, and the audit takes its
    expected values mod 2p); Bootstraps follow `table_lookup`."""
    names = low["input_names"]
    if isinstance(bits, dict):
        cols = [np.asarray(bits[n]).reshape(-1) for n in names]
        T = max((len(c) for c in cols), default=1)
        bits = np.stack([np.broadcast_to(c, (T,)) for c in cols]) if cols else np.zeros((0, T), np.int64)
    bits = np.asarray(bits, np.int64).reshape(len(names), -1)
    T = bits.shape[1]
    wires = np.zeros((len(names) + len(low["kind"]), T), np.int64)
    wires[:len(names)] = bits
    for i, kind in enumerate(low["kind"]):
        a0, a1, w = int(low["arg0"][i]), int(low["arg1"][i]), len(names) + i
        if kind == 0:
            acc = np.full(T, int(low["const_coef"][i]), np.int64)
            for t in range(a0, a0 + a1):
                acc += int(low["term_coef"][t]) * wires[int(low["term_src"][t])]
            wires[w] = acc
        else:
            wires[w] = table_lookup(low["tables"][a1], p, wires[a0])
    return wires


# --------------------------------------------------------------------------------------------
# the model
# --------------------------------------------------------------------------------------------
def wire_noise_factors(low, p, fused=False):
    """Per wire, its noise in units of one blind rotation's output variance v_br, the fresh-input part apart:
    -> (factor [n_wires], fresh [n_wires]) with var(wire) = factor v_br + fresh (sigma_glwe / q)^2.  Inputs (0, 1); a Bootstrap
    output (1, 0), or (`table_fusion_factor`, 0) when the program is fused and several Bootstraps read its source (the rule of
    `split.output_noise_factors`); a LinearProd the sum of c_i^2 times its sources' pairs."""
    n_in = len(low["input_names"])
    readers = {}
    for kind, a0 in zip(low["kind"], low["arg0"]):
        if kind == 1:
            readers[int(a0)] = readers.get(int(a0), 0) + 1
    factor, fresh = [0.0] * n_in, [1.0] * n_in
    for i, kind in enumerate(low["kind"]):
        a0, a1 = int(low["arg0"][i]), int(low["arg1"][i])
        if kind == 1:
            factor.append(float(table_fusion_factor(low["tables"][a1], p)) if fused and readers[a0] >= 2 else 1.0)
            fresh.append(0.0)
        else:
            terms = [(float(low["term_coef"][t]) ** 2, int(low["term_src"][t])) for t in range(a0, a0 + a1)]
            factor.append(sum(c2 * factor[s] for c2, s in terms))
            fresh.append(sum(c2 * fresh[s] for c2, s in terms))
    return np.array(factor), np.array(fresh)


def predicted_variance(low, prm, fused=False):
    """The model's variance of every wire, in torus units: -> (wire [n_wires], rotation_input [n_wires]).
    wire: an input (sigma_glwe / q)^2, the fresh encryption; a Bootstrap output `params.variances(prm)[0]` = v_br, times the
    table's fusion factor when it is cut from a shared rotation (`fused`); a LinearProd sum c_i^2 var(src_i).
    rotation_input[w] = wire[w] + v_ks + v_ms: what the blind rotation of a Bootstrap that reads w sees.
    The sum over a LinearProd's terms ASSUMES INDEPENDENT sources.  Two terms that descend from one ciphertext (a
    reconvergent fan-out, or a LinearProd of LinearProds that share a source when they are not merged) are correlated: their
    noises add as amplitudes, not as variances, and the model is then off in either direction by up to the cross terms."""
    from .params import variances
    v_br, v_ks, v_ms = variances(prm)
    factor, fresh = wire_noise_factors(low, prm.p_msg, fused)
    wire = factor * v_br + fresh * (prm.sigma_glwe / float(MODULUS)) ** 2
    return wire, wire + v_ks + v_ms


# --------------------------------------------------------------------------------------------
# the report
# --------------------------------------------------------------------------------------------
@dataclass
class AuditRow:
    """One audited wire at one point.  `unit`: error units per torus turn (q for wire units, 4pN for field units); count, over,
    max_abs, sum, sumsq: the exact integers of fbs_audit_row, accumulated over the sample chunks."""
    point: str
    level: int
    wire: int
    name: str
    p: int
    unit: int
    predicted_var: float
    norm2: float | None = None     # the reference's statistic: squared norm of the wire over fresh inputs and bootstrap outputs (1 each)
    fan_in: int | None = None      # terms of the LinearProd (None: not one)
    count: int = 0
    over: int = 0
    max_abs: int = 0
    sum: int = 0
    sumsq: int = 0

    def add(self, stats):
        self.count += stats["count"]
        self.over += stats["over"]
        self.max_abs = max(self.max_abs, stats["max_abs"])
        self.sum += stats["sum"]
        self.sumsq += stats["sumsq"]

    @property
    def half_box(self):
        return Fraction(1, 4 * self.p)

    @property
    def mean_exact(self):
        return Fraction(self.sum, self.count * self.unit) if self.count else Fraction(0)

    @property
    def var_exact(self):
        """the samples' variance about their own mean (population form), a Fraction in torus units squared"""
        return Fraction(self.sumsq, self.count * self.unit ** 2) - self.mean_exact ** 2 if self.count else Fraction(0)

    @property
    def mean(self):
        return float(self.mean_exact)

    @property
    def std(self):
        return math.sqrt(float(self.var_exact))

    @property
    def predicted_std(self):
        return math.sqrt(self.predicted_var)

    @property
    def margin(self):
        """(1/(4p) - |mean|) / std: how many measured standard deviations the half box lies from the measured mean"""
        room = float(self.half_box - abs(self.mean_exact))
        return room / self.std if self.std > 0 else math.inf if room > 0 else -math.inf

    @property
    def model_margin(self):
        return float(self.half_box) / self.predicted_std if self.predicted_var > 0 else math.inf

    @property
    def worst(self):
        """the largest |error| seen, as a fraction of the half box"""
        return float(Fraction(self.max_abs, self.unit) / self.half_box)

    def to_dict(self):
        return dict(point=self.point, level=self.level, wire=self.wire, name=self.name, norm2=self.norm2, fan_in=self.fan_in,
                    count=self.count, mean=self.mean, std=self.std, predicted_std=self.predicted_std, margin=self.margin,
                    model_margin=self.model_margin, worst=self.worst, over=self.over)


@dataclass
class AuditReport:
    rows: list
    outputs: dict = field(default_factory=dict)    # what `LutExecEnv.eval` returns for the same inputs
    params: object | None = None
    fused: bool = False
    asked_margin: float | None = None              # ExecConfig.min_margin

    @property
    def min_margin(self):
        return min((r.margin for r in self.rows if r.count), default=math.inf)

    @property
    def failures(self):
        return sum(r.over for r in self.rows)

    @property
    def first_failure(self):
        """the first row with a sample at half a box or beyond: lowest level, then the order the points of a level run in, then row
        order; None when there is none"""
        bad = [(r.level, POINTS.index(r.point), i) for i, r in enumerate(self.rows) if r.over]
        return self.rows[min(bad)[2]] if bad else None

    def worst(self, n=10):
        """the n rows with the least measured margin"""
        return sorted((r for r in self.rows if r.count), key=lambda r: r.margin)[:n]

    def to_json(self):
        first = self.first_failure
        return json.dumps(dict(min_margin=self.min_margin, failures=self.failures, asked_margin=self.asked_margin, fused=self.fused,
                               first_failure=None if first is None else first.to_dict(), rows=[r.to_dict() for r in self.rows]))

    def summary(self, n=10):
        first = self.first_failure
        lines = ["audit: %d rows, min margin %.2f sigma%s, %d samples at half a box or beyond%s" % (
            len(self.rows), self.min_margin, "" if self.asked_margin is None else " (asked: %.1f)" % self.asked_margin, self.failures,
            "" if first is None else "; first at level %d, %s of %s" % (first.level, first.point, first.name))]
        lines.append("%-15s %5s %-12s %8s %8s %11s %11s %7s %7s %6s %5s" % (
            "point", "level", "wire", "norm2", "count", "std", "predicted", "margin", "model", "worst", "over"))
        for r in self.worst(n):
            lines.append("%-15s %5d %-12s %8s %8d %11.3e %11.3e %7.2f %7.2f %6.3f %5d" % (
                r.point, r.level, r.name[:12], "-" if r.norm2 is None else "%.4g" % r.norm2, r.count, r.std, r.predicted_std, r.margin,
                r.model_margin, r.worst, r.over))
        return "\n".join(lines)


def wire_names(env):
    """the name of every program wire, in fbs_program_desc order (`LutExecEnv.lower`: inputs, then the other instructions)"""
    inputs = [i.name for i in env.instructions if isinstance(i, type(env).Input)]
    return inputs + [i.name for i in env.instructions if not isinstance(i, type(env).Input)]


def new_rows(program, low, prm, fused, names, points):
    """the empty rows of a report, keyed (point, level): what `Program.audit_rows` lists, with the model beside each"""
    from . import _native as nat
    p = prm.p_msg
    wire_var, rot_var = predicted_variance(low, prm, fused)
    factor, fresh = wire_noise_factors(low, p, fused)
    n_in = len(low["input_names"])
    rows = {}
    for point in points:
        code = POINTS.index(point)
        levels = [0] if point == "inputs" else range(program.depth + 1) if point == "lincomb" else range(program.depth)
        for L in levels:
            made = []
            for w in program.audit_rows(L, code):
                w = int(w)
                lin = w >= n_in and low["kind"][w - n_in] == 0
                made.append(AuditRow(point, L, w, names[w], p,
                                     unit=4 * p * prm.N if code == nat.AUDIT_ROTATION_INPUT else MODULUS,
                                     predicted_var=float(rot_var[w] if code == nat.AUDIT_ROTATION_INPUT else wire_var[w]),
                                     norm2=float(factor[w] + fresh[w]),
                                     fan_in=int(low["arg1"][w - n_in]) if lin else None))
            rows[(point, L)] = made
    return rows


def chunk_samples(program, T, budget_bytes=None):
    """samples per chunk: what fits a wire budget (default: half of the free device memory) in wire slots, key-switch scratch
    and shared accumulators, at most what one audit call takes"""
    import torch
    from . import _native as nat
    prm = program.ctx.params
    per_sample = program.n_slots * prm.ct_words * 8 + max(1, program.max_sources) * (prm.n + 1) * 4 * 2 + \
        (program.max_width * (prm.k + 1) * prm.N * 8 if program.fused else 0)
    if budget_bytes is None:
        budget_bytes = torch.cuda.mem_get_info(program.ctx.device)[0] // 2
    return int(max(1, min(T, nat.AUDIT_MAX_SAMPLES, budget_bytes // per_sample)))


def run_audit(env, input_values, config=None, points=("rotation_input",), chunk=None):
    """`LutExecEnv.audit`: the parameter choice, the program and the nonces of `LutExecEnv.eval`, stepped level by level on
    torch-owned device memory (the way `distributed.GpuBackend` steps it) in chunks of samples, with the audit of every asked point
    between the steps.  chunk: samples per chunk (None: `chunk_samples`)."""
    import torch
    from . import _native as nat
    cfg = config or env.exec_config
    points = tuple(points)
    for point in points:
        if point not in POINTS:
            raise ValueError("unknown audit point %r (one of %s)" % (point, ", ".join(POINTS)))
    low = env.lower()
    p = cfg.fbs_size or min_fbs_size(low["tables"])
    for t in low["tables"]:
        assert table_is_valid(t, p), "table %s cannot be evaluated by one bootstrap at fbs_size %d" % (t, p)
    names = low["input_names"]
    cols = [np.asarray(input_values[n]).reshape(-1) for n in names]
    T = max((len(c) for c in cols), default=1)
    ctx, fuse = cfg.choose(env, p, samples=T)
    bits = np.stack([np.broadcast_to(c, (T,)) for c in cols]).astype(np.int64) if cols else np.zeros((0, T), np.int64)
    assert bits.size == 0 or (bits.min() >= 0 and bits.max() <= 1), "inputs are bits"
    program = cfg.program_for(ctx, low, fuse)
    prm = ctx.params
    clear = cleartext_wires(low, bits, p)
    rows = new_rows(program, low, prm, fuse, wire_names(env), points)

    nonce0 = cfg.take_nonces(bits.size)
    dev = torch.device("cuda", ctx.device)
    n_in, n_out, ctw = program.n_inputs, program.n_outputs, prm.ct_words
    Tc = chunk_samples(program, T) if chunk is None else int(max(1, min(chunk, T, nat.AUDIT_MAX_SAMPLES)))
    out = np.zeros((n_out, T), np.int64)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        wires = torch.empty((program.n_slots * Tc, ctw), dtype=torch.int64, device=dev)
        d_bits = torch.from_numpy(np.ascontiguousarray(bits)).to(dev)
        d_out = torch.empty((max(1, n_out), Tc), dtype=torch.int64, device=dev)
        base = wires.data_ptr()

        def slot_ptr(slot):
            return base + int(slot) * Tc * ctw * 8

        def audit(point, L, s0, tc):
            made = rows.get((point, L))
            if not made:
                return
            want = np.ascontiguousarray(clear[[r.wire for r in made], s0:s0 + tc])
            d_want = torch.from_numpy(want).to(dev)
            stats, _ = program.audit_level_dev(L, POINTS.index(point), base, Tc, 0, tc, d_want.data_ptr(), stream=stream)
            for r, st in zip(made, stats):
                r.add(st)

        for s0 in range(0, T, Tc):
            tc = min(Tc, T - s0)
            # input i, sample s on stream nonce0 + i T + s, as fbs_eval_messages numbers them; None: streams nobody has used
            for i in range(n_in):
                ctx.encrypt_dev(d_bits.data_ptr() + (i * T + s0) * 8, tc, slot_ptr(program.in_slot[i]),
                                nonce0=None if nonce0 is None else int(nonce0) + i * T + s0, stream=stream)
            audit("inputs", 0, s0, tc)
            for L in range(program.depth + 1):
                program.level_lincomb_dev(L, base, Tc, 0, tc, stream=stream)
                audit("lincomb", L, s0, tc)
                if L == program.depth:
                    break
                audit("rotation_input", L, s0, tc)
                program.level_bootstrap_dev(L, base, Tc, 0, tc, 0, program.level_width[L] * tc, stream=stream)
                audit("bootstrap", L, s0, tc)
            for o in range(n_out):
                if program.out_slot[o] >= 0:
                    ctx.decrypt_dev(slot_ptr(program.out_slot[o]), tc, d_out.data_ptr() + o * Tc * 8, stream=stream)
            ctx.sync(stream)
            out[:, s0:s0 + tc] = d_out[:n_out, :tc].cpu().numpy()
    result = {}
    for k, name in enumerate(low["out_names"]):
        w = low["out_wire"][k]
        result[name] = (-1 - w) if w < 0 else out[k].astype(int)
    ordered = [r for point in POINTS for L in range(program.depth + 1) for r in rows.get((point, L), ())]
    ordered.sort(key=lambda r: (r.level, POINTS.index(r.point)))   # (stable: row order within a point)
    return AuditReport(ordered, result, prm, bool(fuse), cfg.min_margin)
