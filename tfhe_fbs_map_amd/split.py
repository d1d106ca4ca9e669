"""Client / server split: evaluate a program on a GPU that never holds the secret key.

The `Client` picks the parameter set for a program exactly as `ExecConfig.choose` does, keys a context with
`Context.keygen_seeded` and hands out a `ServerKey`: the public mask key and the bodies of the evaluation keys (include/
fbs_exec.h, "seeded keys and inputs").  It encrypts inputs to bodies only (`EncryptedInputs`) and decrypts what comes back.
The `Server` builds an evaluation-only context from the server key, lowers the program itself, expands the input bodies on
the GPU and returns either full output ciphertexts (`run` -> `EncryptedOutputs`, kN + 1 words each) or compact ones
(`run_compact` -> `CompactOutputs`: key-switched to the small key, rounded to a few bits a field and packed, n + 1 fields --
include/fbs_exec.h, "compact outputs").  All four objects save to and load from `.npz` files with `allow_pickle=False`; none of
them holds secret material.

    client = Client(env, ExecConfig())
    client.server_key().save("server_key.npz")             # -> the server, once
    client.encrypt(inputs).save("inputs.npz")              # -> the server, per evaluation
    server = Server(ServerKey.load("server_key.npz"))
    server.run_compact(env, EncryptedInputs.load("inputs.npz")).save("outputs.npz")
    client.decrypt(CompactOutputs.load("outputs.npz"))    # == env.eval(inputs)

Chains.  `Server.run_chain` evaluates a program whose inputs come from any mix of the client's seeded inputs and the full or
compact outputs of earlier evaluations under the same server key, found by name (`rename` maps an input to another source name).
A compact input is refreshed on the GPU -- unpacked and bootstrapped through the identity table, one bootstrap per input and
sample -- and so is a full input whose producer was noisier than a bootstrap output (`out_norm2` > 1).  Every link is held to the
consuming program's margin (`plan_chain`).  One client key serves every program of a chain: `Client(env, config, programs=...)`.

    client = Client(adder8, ExecConfig(), programs=[adder8])
    server = Server(client.server_key())
    acc = server.run_compact(adder8, client.encrypt(first))            # first: {a0..a7, b0..b7: bits}
    a_from_s = {f"a{i}": f"s{i}" for i in range(8)}
    for b in stream:                                                   # acc <- acc + b; the state stays on the server
        fresh = client.encrypt(b, names=[f"b{i}" for i in range(8)])
        acc = server.run_chain(adder8, [acc, fresh], rename=a_from_s, compact=True)
    client.decrypt(acc)

Resident state.  With `resident=True`, `run` and `run_chain` leave the full outputs in the server's device memory and return a
`ResidentOutputs`; it links into the next `run_chain` like an `EncryptedOutputs` (a bootstrap output goes in untouched), with no
copy through the host and no refresh.  The state leaves the card only when asked: `fetch()` -> `EncryptedOutputs`,
`fetch(compact=True)` -> `CompactOutputs` (compacted on the GPU; only the packed words cross the bus); `Server.restore` puts a
fetched `EncryptedOutputs` back.

    acc = server.run(adder8, client.encrypt(first), resident=True)
    for b in stream:
        nxt = server.run_chain(adder8, [acc, client.encrypt(b, names=b_names)], rename=a_from_s, resident=True)
        acc.close()
        acc = nxt
    client.decrypt(acc.fetch(compact=True))

Plaintext inputs.  The server's own data -- a table row, a round key, a counter -- joins a chain as a `PlainInputs`: cleartext bits by
input name, a row per sample or one value for every sample.  They are written on the GPU as trivial ciphertexts (zero mask, body
m * Delta: include/fbs_exec.h, "chained evaluation"), carry no noise and belong to no key; the client never sees them.

    round_key = PlainInputs(b_names, None, {f"b{i}": (k >> i) & 1 for i in range(8)})    # one value for all samples
    server.run(adder8, client.encrypt(query, names=a_names), plain=round_key)

Public-key inputs: three parties.  A data owner who is neither the key holder nor the server -- a sensor, a second company, a user
of a service somebody else keyed -- encrypts under the client's `PublicKey` (`public.PublicEncryptor`, on libfbspublic.so alone: no
secret, no GPU) and sends GLWE samples, k + 1 words a bit (include/fbs_exec.h, "public-key inputs").  The server expands them on
the GPU into resident state and evaluates as ever; their noise, (1 + kN) sigma_glwe^2, is far below a bootstrap output's, so
they enter unrefreshed (`params.public_input_factor`).  IND-CPA only and malleable, like every ciphertext here.

    client.public_key().save("public_key.npz")                                   # key holder -> the data owner, once
    sensor = PublicEncryptor(PublicKey.load("public_key.npz"))                   # the data owner: os.urandom seeds it
    sensor.encrypt(reading, names=a_names).save("reading.npz")                   # -> the server, per evaluation
    out = server.run(adder8, client.encrypt(offset, names=b_names), public=PublicInputs.load("reading.npz"))
    client.decrypt(out)                                                          # the key holder reads the result
"""
from __future__ import annotations

import hashlib
import math
from dataclasses import asdict, dataclass

import numpy as np

from .fbs_exec_env import ExecConfig, min_fbs_size, table_fusion_factor, table_is_valid

__all__ = ["ServerKey", "EncryptedInputs", "PlainInputs", "EncryptedOutputs", "CompactOutputs", "PackedOutputs", "ResidentOutputs", "packed_words", "Client", "Server", "FORMAT_VERSION",
           "mask_key_fingerprint", "seeded_key_sizes", "compact_words", "output_noise_factor", "output_noise_factors",
           "plan_chain", "ChainLink", "client_choice"]

FORMAT_VERSION = 1
_PARAM_FIELDS = ("n", "log_n_poly", "k", "l_bsk", "beta_bsk", "t_ksk", "gamma_ksk", "p_msg", "sigma_lwe", "sigma_glwe",
                 "bsk_group")


def mask_key_fingerprint(mask_key: bytes) -> bytes:
    """8 bytes that name a server key: what inputs and outputs carry so that nobody mixes key sets"""
    return hashlib.sha256(b"tfhe_fbs_map_amd seeded mask key" + bytes(mask_key)).digest()[:8]


def seeded_key_sizes(prm):
    """(bootstrapping-key bodies, key-switching-key bodies) in words for a parameter set: fbs_seeded_key_sizes without a GPU"""
    g = prm.n // 2 * 3 if prm.bsk_group == 2 else prm.n
    return g * (prm.k + 1) * prm.l_bsk * prm.N, prm.k * prm.N * prm.t_ksk


def compact_words(prm, bits):
    """W, the words of one compact ciphertext at width `bits`: fbs_compact_words without a GPU"""
    return ((prm.n + 1) * int(bits) + 63) // 64


def packed_words(prm, count, bits):
    """Words of `count` outputs packed at width `bits` (include/fbs_exec.h, "packed outputs"): fbs_packed_words without a GPU.  A
    full sample is its (k + 1) N fields, a partly filled last one its k N mask fields and `count mod N` body fields; every sample
    starts on a word boundary (k N bits is a multiple of 64)."""
    N, bits = prm.N, int(bits)
    full, rest = divmod(int(count), N)
    mask_words = prm.k * N * bits // 64
    return full * (mask_words + (N * bits + 63) // 64) + ((mask_words + (rest * bits + 63) // 64) if rest else 0)


def output_noise_factor(low, p, fused=False):
    """out_norm2 of `params.compact_output_bits`: the worst output's noise in units of one blind rotation's -- 1 for a bootstrap
    output, `table_fusion_factor` for one cut from a shared rotation (fused programs), the squared norm of the coefficients for a
    linear combination (over its sources' factors), 0 for inputs and constants (fresh or trivial ciphertexts)."""
    return max(output_noise_factors(low, p, fused), default=0.0)


def output_noise_factors(low, p, fused=False, input_noise=None):
    """`output_noise_factor` for each output in output order (a constant: 0).  input_noise: the factor of each input (None: 0, fresh
    ciphertexts; a chained evaluation passes 1 for an input that was refreshed, its producer's factor for a full link)."""
    n_in = len(low["input_names"])
    readers = {}
    for kind, a0 in zip(low["kind"], low["arg0"]):
        if kind == 1:
            readers[int(a0)] = readers.get(int(a0), 0) + 1
    noise = [0.0] * n_in if input_noise is None else [float(x) for x in input_noise]
    assert len(noise) == n_in
    for i, kind in enumerate(low["kind"]):
        a0, a1 = int(low["arg0"][i]), int(low["arg1"][i])
        if kind == 1:
            noise.append(float(table_fusion_factor(low["tables"][a1], p)) if fused and readers[a0] >= 2 else 1.0)
        else:
            noise.append(sum(float(low["term_coef"][t]) ** 2 * noise[int(low["term_src"][t])] for t in range(a0, a0 + a1)))
    return [noise[int(w)] if w >= 0 else 0.0 for w in low["out_wire"]]


def _load_npz(path, kind):
    with np.load(path, allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    if str(d.get("kind", "")) != kind:
        raise ValueError(f"{path} is not a saved {kind}")
    if int(d.get("format_version", -1)) != FORMAT_VERSION:
        raise ValueError(f"{path}: format version {d.get('format_version')} (this library reads {FORMAT_VERSION})")
    return d


def _fingerprint_of(d):
    fp = np.asarray(d["fingerprint"], np.uint8)
    if fp.shape != (8,):
        raise ValueError("a fingerprint has 8 bytes")
    return fp.tobytes()


def _norm2_fields(outputs):
    """the optional out_norm2 record of a saved output set (files written before it existed have none)"""
    return {} if outputs.out_norm2 is None else dict(out_norm2=np.asarray(outputs.out_norm2, np.float64).reshape(-1))


def _norm2_of(d, n_outputs):
    if "out_norm2" not in d:
        return None
    v = np.asarray(d["out_norm2"], np.float64).reshape(-1)
    if v.shape != (n_outputs,) or not np.isfinite(v).all() or (v < 0).any():
        raise ValueError(f"out_norm2 of shape {v.shape} for {n_outputs} outputs")
    return v


@dataclass
class ServerKey:
    """What a server needs to evaluate: the parameter set, whether programs load with shared rotations (`fuse_tables`), the
    public mask key and the key bodies.  No secret."""
    params: object
    fuse_tables: bool
    mask_key: bytes
    bsk_bodies: np.ndarray
    ksk_bodies: np.ndarray
    packing_bodies: np.ndarray | None = None   # [n][t_p][N] bodies of the packing key (packed outputs); None: the key has none
    packing_levels: int = 0                    # t_p
    packing_base_bits: int = 0                 # gamma_p
    fold_bodies: np.ndarray | None = None      # [D][t_f][N] bodies of the fold key (folded state); None: the key has none
    fold_levels: int = 0                       # t_f
    fold_base_bits: int = 0                    # gamma_f

    def __post_init__(self):
        self.mask_key = bytes(self.mask_key)
        if len(self.mask_key) != 32:
            raise ValueError("a mask key has 32 bytes")
        self.bsk_bodies = np.ascontiguousarray(self.bsk_bodies, np.uint64).reshape(-1)
        self.ksk_bodies = np.ascontiguousarray(self.ksk_bodies, np.uint64).reshape(-1)
        want = seeded_key_sizes(self.params)
        for a, w, name in zip((self.bsk_bodies, self.ksk_bodies), want, ("bsk_bodies", "ksk_bodies")):
            if a.size != w:
                raise ValueError(f"{name} has {a.size} words, the parameter set needs {w}")
        self._gadget_key("packing", self.params.n)
        self._gadget_key("fold", self.params.k * self.params.N)

    def _gadget_key(self, noun, rows):
        """normalises and checks the optional `noun` key: `noun`_bodies [rows][t][N], `noun`_levels t, `noun`_base_bits gamma"""
        bodies, t, g = getattr(self, noun + "_bodies"), 0, 0
        if bodies is not None:
            t, g = int(getattr(self, noun + "_levels")), int(getattr(self, noun + "_base_bits"))
            bodies, want = np.ascontiguousarray(bodies, np.uint64).reshape(-1), rows * t * self.params.N
            if t < 1 or g < 1 or t * g > 31:
                raise ValueError(f"a {noun} key of {t} levels of {g} bits")
            if bodies.size != want:
                raise ValueError(f"{noun}_bodies has {bodies.size} words, the parameter set needs {want}")
        setattr(self, noun + "_bodies", bodies)
        setattr(self, noun + "_levels", t)
        setattr(self, noun + "_base_bits", g)

    @property
    def fingerprint(self) -> bytes:
        return mask_key_fingerprint(self.mask_key)

    def save(self, path):
        prm = asdict(self.params)
        np.savez(path, kind=np.array("server_key"), format_version=np.array(FORMAT_VERSION),
                 params=np.array([int(prm[f]) for f in _PARAM_FIELDS], np.int64), fuse_tables=np.array(bool(self.fuse_tables)),
                 mask_key=np.frombuffer(self.mask_key, np.uint8), fingerprint=np.frombuffer(self.fingerprint, np.uint8),
                 bsk_bodies=self.bsk_bodies, ksk_bodies=self.ksk_bodies, **self._gadget_fields("packing"), **self._gadget_fields("fold"),
                 **self._sampler_field())

    def _sampler_field(self):
        """the noise sampler of the parameter set, beside the other parameters (a key of sampler 0 is written exactly as before:
        a file without the field is a sampler-0 key)"""
        sampler = int(getattr(self.params, "sampler", 0))
        return dict(sampler=np.array(sampler, np.int64)) if sampler else {}

    def _gadget_fields(self, prefix):
        """the optional packing or fold key of a saved server key (a key without one is written exactly as before)"""
        bodies = getattr(self, prefix + "_bodies")
        if bodies is None:
            return {}
        return {prefix + "_bodies": bodies, prefix + "_levels": np.array(getattr(self, prefix + "_levels"), np.int64),
                prefix + "_base_bits": np.array(getattr(self, prefix + "_base_bits"), np.int64)}

    @property
    def fold_factor(self):
        """what one fold under this key adds to a ciphertext, in units of a blind rotation's output variance (None: no fold key)"""
        from .params import folded_state_factor
        return None if self.fold_bodies is None else folded_state_factor(self.params, self.fold_levels, self.fold_base_bits)

    @classmethod
    def load(cls, path):
        from ._client_native import Params
        d = _load_npz(path, "server_key")
        vals = np.asarray(d["params"], np.int64)
        if vals.shape != (len(_PARAM_FIELDS),):
            raise ValueError("parameter record has the wrong length")
        prm = Params(sampler=int(d["sampler"]) if "sampler" in d else 0, **{f: int(v) for f, v in zip(_PARAM_FIELDS, vals)})
        if d["bsk_bodies"].dtype != np.uint64 or d["ksk_bodies"].dtype != np.uint64:
            raise ValueError("key bodies are uint64 words")
        gadget = {}
        for prefix in ("packing", "fold"):
            gadget.update(cls._gadget_loaded(d, prefix))
        key = cls(prm, bool(d["fuse_tables"]), np.asarray(d["mask_key"], np.uint8).tobytes(), d["bsk_bodies"], d["ksk_bodies"], **gadget)
        if _fingerprint_of(d) != key.fingerprint:
            raise ValueError("the saved fingerprint is not the mask key's")
        return key

    @staticmethod
    def _gadget_loaded(d, prefix):
        """the fields of `_gadget_fields(prefix)` as constructor arguments ({}: the file has no such key)"""
        if prefix + "_bodies" not in d:
            return {}
        if d[prefix + "_bodies"].dtype != np.uint64:
            raise ValueError("key bodies are uint64 words")
        return {prefix + "_bodies": d[prefix + "_bodies"], prefix + "_levels": int(d[prefix + "_levels"]),
                prefix + "_base_bits": int(d[prefix + "_base_bits"])}


@dataclass
class EncryptedInputs:
    """Seeded input ciphertexts of one evaluation: bodies [n_inputs][T]; input i, sample s on stream nonce0 + i*T + s."""
    input_names: list
    T: int
    nonce0: int
    bodies: np.ndarray
    fingerprint: bytes

    def save(self, path):
        np.savez(path, kind=np.array("encrypted_inputs"), format_version=np.array(FORMAT_VERSION),
                 input_names=np.array(list(self.input_names), dtype=str), T=np.array(self.T, np.int64),
                 nonce0=np.array(self.nonce0, np.uint64), bodies=np.ascontiguousarray(self.bodies, np.uint64),
                 fingerprint=np.frombuffer(self.fingerprint, np.uint8))

    @classmethod
    def load(cls, path):
        d = _load_npz(path, "encrypted_inputs")
        names = [str(n) for n in np.asarray(d["input_names"]).reshape(-1)]
        T = int(d["T"])
        bodies = np.asarray(d["bodies"])
        if bodies.dtype != np.uint64 or bodies.shape != (len(names), T):
            raise ValueError(f"bodies of shape {bodies.shape} for {len(names)} inputs of {T} samples")
        return cls(names, T, int(d["nonce0"]), bodies, _fingerprint_of(d))


@dataclass
class PlainInputs:
    """Cleartext inputs the server supplies itself (`Server.run_chain`): bits by input name, written on the GPU as trivial
    ciphertexts.  values: int64 [n_inputs][T], or [n_inputs] when every input has one value for all samples (T may then be None: the
    chain's T), or a mapping {name: array [T] or int} that may mix the two.  Public data: no fingerprint, no key.  Held to what
    `Client.encrypt` admits for inputs: bits."""
    input_names: list
    T: int | None
    values: object
    broadcast: np.ndarray | None = None   # [n_inputs] bool: the row is one value for all samples (None: by the shape of `values`)

    def __post_init__(self):
        self.input_names = [str(n) for n in self.input_names]
        n = len(self.input_names)
        if len(set(self.input_names)) != n:
            raise ValueError("plain inputs name an input twice")
        self.T = None if self.T is None else int(self.T)
        if self.T is not None and self.T < 1:
            raise ValueError(f"plain inputs of T = {self.T} samples")
        v = self.values
        if hasattr(v, "keys"):
            if sorted(str(k) for k in v.keys()) != sorted(self.input_names):
                raise ValueError("the values name other inputs than input_names")
            v = {str(k): x for k, x in v.items()}
            rows = [self._int64(v[name]) for name in self.input_names]
            self.broadcast = np.array([r.ndim == 0 for r in rows], bool)
            if self.broadcast.all():
                v = np.array([int(r) for r in rows], np.int64).reshape(n)
            else:
                if self.T is None:
                    raise ValueError("plain inputs with a value per sample need T")
                for name, r in zip(self.input_names, rows):
                    if r.ndim and r.shape != (self.T,):
                        raise ValueError(f"plain input {name}: values of shape {r.shape} for {self.T} samples")
                v = np.stack([np.broadcast_to(r, (self.T,)) for r in rows]).astype(np.int64)
        else:
            v = self._int64(v)
            if self.broadcast is None:
                self.broadcast = np.full(n, v.ndim == 1, bool)
        self.broadcast = np.asarray(self.broadcast)
        if self.broadcast.dtype != bool or self.broadcast.shape != (n,):
            raise ValueError(f"a broadcast mask of shape {self.broadcast.shape} and type {self.broadcast.dtype} for {n} plain inputs")
        if v.ndim == 1:
            if v.shape != (n,) or not self.broadcast.all():
                raise ValueError(f"plain values of shape {v.shape} for {n} inputs with one value each")
        elif self.T is None or v.shape != (n, self.T):
            raise ValueError(f"plain values of shape {v.shape} for {n} inputs of {self.T} samples")
        elif (v[self.broadcast] != v[self.broadcast][:, :1]).any():
            raise ValueError("a plain input marked as one value for all samples holds several")
        if v.size and (v.min() < 0 or v.max() > 1):
            raise ValueError("plain inputs are bits, as the inputs a client encrypts")
        self.values = np.ascontiguousarray(v, np.int64)

    @staticmethod
    def _int64(x):
        a = np.asarray(x)
        if a.dtype == bool:
            a = a.astype(np.int64)
        if a.dtype.kind not in "iu":
            raise ValueError(f"plain values of type {a.dtype}: they are integers")
        return a.astype(np.int64)

    def row(self, j):
        """what feeds input j: a python int (one value for all samples) or an int64 array [T]"""
        if self.values.ndim == 1:
            return int(self.values[j])
        return int(self.values[j, 0]) if self.broadcast[j] else self.values[j]

    def save(self, path):
        np.savez(path, kind=np.array("plain_inputs"), format_version=np.array(FORMAT_VERSION),
                 input_names=np.array(list(self.input_names), dtype=str), T=np.array(-1 if self.T is None else self.T, np.int64),
                 values=self.values, broadcast=self.broadcast)

    @classmethod
    def load(cls, path):
        d = _load_npz(path, "plain_inputs")
        names = [str(n) for n in np.asarray(d["input_names"]).reshape(-1)]
        T = int(d["T"])
        values, broadcast = np.asarray(d["values"]), np.asarray(d["broadcast"])
        if values.dtype != np.int64 or values.ndim not in (1, 2) or broadcast.dtype != bool:
            raise ValueError(f"plain values of shape {values.shape} and type {values.dtype}, a mask of type {broadcast.dtype}")
        return cls(names, None if T < 0 else T, values, broadcast)


@dataclass
class EncryptedOutputs:
    """Output ciphertexts of one evaluation: [n_outputs][T][D+1], as `Program.eval` returns them."""
    output_names: list
    T: int
    cts: np.ndarray
    fingerprint: bytes
    out_norm2: np.ndarray | None = None   # [n_outputs] each output's noise factor (output_noise_factors); None: not recorded

    def save(self, path):
        np.savez(path, kind=np.array("encrypted_outputs"), format_version=np.array(FORMAT_VERSION),
                 output_names=np.array(list(self.output_names), dtype=str), T=np.array(self.T, np.int64),
                 cts=np.ascontiguousarray(self.cts, np.uint64), fingerprint=np.frombuffer(self.fingerprint, np.uint8),
                 **_norm2_fields(self))

    @classmethod
    def load(cls, path):
        d = _load_npz(path, "encrypted_outputs")
        names = [str(n) for n in np.asarray(d["output_names"]).reshape(-1)]
        T = int(d["T"])
        cts = np.asarray(d["cts"])
        if cts.dtype != np.uint64 or cts.ndim != 3 or cts.shape[:2] != (len(names), T):
            raise ValueError(f"ciphertexts of shape {cts.shape} for {len(names)} outputs of {T} samples")
        return cls(names, T, cts, _fingerprint_of(d), _norm2_of(d, len(names)))


@dataclass
class CompactOutputs:
    """Compact output ciphertexts of one evaluation (`Server.run_compact`): words [n_outputs][T][W], each ciphertext the output
    key-switched to the small key, rounded to `bits` bits a field and packed (include/fbs_exec.h, "compact outputs")."""
    output_names: list
    T: int
    bits: int
    words: np.ndarray
    fingerprint: bytes
    out_norm2: np.ndarray | None = None   # as EncryptedOutputs.out_norm2

    def save(self, path):
        np.savez(path, kind=np.array("compact_outputs"), format_version=np.array(FORMAT_VERSION),
                 output_names=np.array(list(self.output_names), dtype=str), T=np.array(self.T, np.int64),
                 bits=np.array(self.bits, np.int64), words=np.ascontiguousarray(self.words, np.uint64),
                 fingerprint=np.frombuffer(self.fingerprint, np.uint8), **_norm2_fields(self))

    @classmethod
    def load(cls, path):
        d = _load_npz(path, "compact_outputs")
        names = [str(n) for n in np.asarray(d["output_names"]).reshape(-1)]
        T, bits = int(d["T"]), int(d["bits"])
        words = np.asarray(d["words"])
        if not 1 <= bits <= 31:
            raise ValueError(f"a compact width of {bits} bits")
        if words.dtype != np.uint64 or words.ndim != 3 or words.shape[:2] != (len(names), T):
            raise ValueError(f"compact ciphertexts of shape {words.shape} for {len(names)} outputs of {T} samples")
        return cls(names, T, bits, words, _fingerprint_of(d), _norm2_of(d, len(names)))


@dataclass
class PackedOutputs:
    """Packed output ciphertexts of one evaluation (`Server.run_packed`): the n_outputs * T outputs, flattened [output][sample],
    written N at a time into GLWE samples under the client's big key, rounded to `bits` bits a coefficient and bit-packed
    (include/fbs_exec.h, "packed outputs"); `words` is the flat array `packed_words(params, n_outputs * T, bits)` long.  For the
    client only: a packed result is no source of a chain."""
    output_names: list
    T: int
    bits: int
    words: np.ndarray
    fingerprint: bytes
    out_norm2: np.ndarray | None = None   # as EncryptedOutputs.out_norm2

    def save(self, path):
        np.savez(path, kind=np.array("packed_outputs"), format_version=np.array(FORMAT_VERSION),
                 output_names=np.array(list(self.output_names), dtype=str), T=np.array(self.T, np.int64),
                 bits=np.array(self.bits, np.int64), words=np.ascontiguousarray(self.words, np.uint64),
                 fingerprint=np.frombuffer(self.fingerprint, np.uint8), **_norm2_fields(self))

    @classmethod
    def load(cls, path):
        d = _load_npz(path, "packed_outputs")
        names = [str(n) for n in np.asarray(d["output_names"]).reshape(-1)]
        T, bits = int(d["T"]), int(d["bits"])
        words = np.asarray(d["words"])
        if not 1 <= bits <= 31 or T < 0:
            raise ValueError(f"a packed width of {bits} bits, {T} samples")
        if words.dtype != np.uint64 or words.ndim != 1:
            raise ValueError(f"packed words of shape {words.shape} and type {words.dtype}")
        return cls(names, T, bits, words, _fingerprint_of(d), _norm2_of(d, len(names)))


def folded_words(prm, count):
    """Words of `count` ciphertexts folded (include/fbs_exec.h, "folded state"): ceil(count / N) samples of (k + 1) N words"""
    return -(-int(count) // prm.N) * (prm.k + 1) * prm.N


class FoldedOutputs:
    """Folded state (`ResidentOutputs.fold`): the n_outputs * T output ciphertexts, flattened [output][sample], written N at a time
    into full-precision GLWE samples under the client's big key -- (k + 1) N words for N bits, against (D + 1) N full.  `words` is
    the flat array `folded_words(params, n_outputs * T)` long: a numpy array, or (device=True) an int64 torch tensor that stays on
    the card.  A source of `Server.run_chain` that links in unrefreshed, like a public-key input (`plan_chain`: out_norm2 +
    fold_factor); `Server.restore` turns it back into `ResidentOutputs`, `Client.decrypt` reads it."""

    def __init__(self, output_names, T, words, fingerprint, out_norm2=None, fold_factor=0.0):
        self.output_names, self.T, self.fingerprint = list(output_names), int(T), bytes(fingerprint)
        self.words = words
        self.out_norm2 = None if out_norm2 is None else np.asarray(out_norm2, np.float64).reshape(-1)
        self.fold_factor = float(fold_factor)   # what the fold added, in units of a blind rotation's output variance

    @property
    def on_device(self):
        return not isinstance(self.words, np.ndarray)

    def host_words(self):
        """the words as a numpy array (a device-held one is fetched)"""
        if self.on_device:
            return self.words.cpu().numpy().view(np.uint64)
        return np.ascontiguousarray(self.words, np.uint64).reshape(-1)

    def save(self, path):
        np.savez(path, kind=np.array("folded_outputs"), format_version=np.array(FORMAT_VERSION),
                 output_names=np.array(list(self.output_names), dtype=str), T=np.array(self.T, np.int64), words=self.host_words(),
                 fingerprint=np.frombuffer(self.fingerprint, np.uint8), fold_factor=np.array(self.fold_factor, np.float64),
                 **_norm2_fields(self))

    @classmethod
    def load(cls, path):
        d = _load_npz(path, "folded_outputs")
        names = [str(n) for n in np.asarray(d["output_names"]).reshape(-1)]
        T, words, factor = int(d["T"]), np.asarray(d["words"]), float(d["fold_factor"])
        if T < 0 or not np.isfinite(factor) or factor < 0:
            raise ValueError(f"folded outputs of {T} samples, fold factor {factor}")
        if words.dtype != np.uint64 or words.ndim != 1:
            raise ValueError(f"folded words of shape {words.shape} and type {words.dtype}")
        return cls(names, T, words, _fingerprint_of(d), _norm2_of(d, len(names)), factor)


class ResidentOutputs:
    """Full output ciphertexts of one evaluation that stayed on the server's GPU (`Server.run` / `Server.run_chain` with
    `resident=True`): row o of `state` (a `DeviceState`, [n_outputs][T][D+1]) is output o.  A source of `Server.run_chain` on the
    server that made it, under the link rule of `EncryptedOutputs`; `fetch` brings it to the host, `close()` frees the state."""

    def __init__(self, output_names, T, fingerprint, out_norm2, state, server=None, compact_bits=None):
        self.output_names, self.T, self.fingerprint = list(output_names), int(T), bytes(fingerprint)
        self.out_norm2 = None if out_norm2 is None else np.asarray(out_norm2, np.float64).reshape(-1)
        self.state, self.server = state, server
        self.compact_bits = compact_bits   # the width fetch(compact=True) takes by default: the producer's `Server.compact_bits`
        self.packed_bits = None            # the width fetch(packed=True) takes by default (`Server.packed_bits`)

    @property
    def closed(self):
        return self.state is None or bool(self.state.closed)

    def fetch(self, compact=False, bits=None, packed=False):
        """-> `EncryptedOutputs`, or with compact=True `CompactOutputs` at `bits` (None: the width `Server.compact_bits` picks for
        the program that computed them, or for their noise after a chain); both as `run` / `run_compact` return them.
        packed=True: `PackedOutputs` at `bits` (None: the width `params.packing_choice` gave for them), packed on the GPU with the
        server key's packing key; only the packed words cross the bus."""
        if self.closed:
            raise ValueError("the resident outputs are closed")
        if packed:
            if compact:
                raise ValueError("packed or compact, not both")
            if self.server is None or self.server.key.packing_bodies is None:
                raise ValueError("the server key holds no packing key (Client(..., packing=True))")
            bits = self.packed_bits if bits is None else int(bits)
            if bits is None:
                raise ValueError("no default packed width is recorded for these outputs: pass bits")
            return PackedOutputs(list(self.output_names), self.T, int(bits), self.state.fetch_packed(int(bits)), self.fingerprint, self.out_norm2)
        if not compact:
            return EncryptedOutputs(list(self.output_names), self.T, self.state.fetch(), self.fingerprint, self.out_norm2)
        bits = self.compact_bits if bits is None else int(bits)
        if bits is None:
            raise ValueError("no default compact width is recorded for these outputs: pass bits")
        return CompactOutputs(list(self.output_names), self.T, int(bits), self.state.fetch(bits=int(bits)), self.fingerprint, self.out_norm2)

    def fold(self, device=False) -> "FoldedOutputs":
        """-> `FoldedOutputs`: every row folded on the GPU with the server key's fold key (include/fbs_exec.h, "folded state"), 24
        bytes a bit at k = 2 where the rows hold 16 392.  device=True: the words stay on the card (a torch tensor); else only they
        cross the bus.  The rows themselves are untouched: close them to free their memory."""
        if self.closed:
            raise ValueError("the resident outputs are closed")
        if self.server is None or self.server.key.fold_bodies is None:
            raise ValueError("the server key holds no fold key (Client(..., folding=True))")
        out_norm2 = np.ones(len(self.output_names)) if self.out_norm2 is None else self.out_norm2
        return FoldedOutputs(list(self.output_names), self.T, self.state.fold(device=bool(device)), self.fingerprint, out_norm2,
                             self.server.key.fold_factor)

    # -- sample-axis operations (include/fbs_exec.h): views that read the samples through an index, and sums of runs of samples --
    def samples(self, index, fill=0, names=None) -> "SampleView":
        """A `SampleView`: a source of `Server.run_chain` with T = len(index) whose sample s is sample index[s] of these rows, or,
        where index[s] == SAMPLE_NONE, a ciphertext of `fill` made on the GPU (an int for every row, or {row name: int})."""
        return SampleView(self, index, fill, names)

    def shift(self, d, fill=0, names=None) -> "SampleView":
        """sample s reads sample s - d (d of either sign); samples that fall off either end take `fill`"""
        return self.samples(shift_index(self.T, d), fill, names)

    def broadcast(self, s, T, names=None) -> "SampleView":
        """T samples that all read sample s"""
        if not 0 <= int(s) < self.T:
            raise ValueError("sample %d of %d" % (int(s), self.T))
        return self.samples(np.full(int(T), int(s), np.uint32), 0, names)

    def stride(self, start, step, names=None) -> "SampleView":
        """samples start, start + step, .. below T"""
        if int(step) < 1 or not 0 <= int(start) < self.T:
            raise ValueError("stride(%d, %d) over %d samples" % (int(start), int(step), self.T))
        return self.samples(np.arange(int(start), self.T, int(step), dtype=np.uint32), 0, names)

    def sum_groups(self, group, max_value=1) -> "ResidentOutputs":
        """A new `ResidentOutputs` of T' = ceil(T / group) samples: sample j of every row is the sum of samples [j group, (j + 1) group)
        of that row, added on the GPU (fbs_state_sum_groups) -- how many of a group's bits are set, or the total of values up to
        `max_value`.  Refused (`plan_sum_groups`) when a sum could leave [0, p).  The sums carry `out_norm2 * group`; no default
        fetch width is recorded for them.  A chain that reads them refreshes them first (`plan_chain`: out_norm2 > 1)."""
        if self.closed:
            raise ValueError("the resident outputs are closed")
        T, out_norm2 = plan_sum_groups(self.server.key.params.p_msg, self.T, group, max_value, self.out_norm2)
        return ResidentOutputs(list(self.output_names), T, self.fingerprint, out_norm2, self.state.sum_groups(int(group)), self.server)

    def close(self):
        if self.state is not None:
            self.state.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


SAMPLE_NONE = 0xFFFFFFFF   # FBS_SAMPLE_NONE: a sample of a view that reads no sample of the state, but the view's fill


def shift_index(T, d):
    """the index of `ResidentOutputs.shift`: [T] uint32, s - d where that is a sample, else SAMPLE_NONE"""
    s = np.arange(int(T), dtype=np.int64) - int(d)
    return np.where((s >= 0) & (s < int(T)), s, SAMPLE_NONE).astype(np.uint32)


def plan_sum_groups(p, T, group, max_value=1, out_norm2=None):
    """The pure part of `ResidentOutputs.sum_groups`: -> (T', out_norm2') or ValueError.  T' = ceil(T / group).  The summed samples'
    errors are independent, so their variances add: out_norm2' = out_norm2 * group, as `output_noise_factors` treats a LinearProd
    of `group` unit coefficients.  A sum of `group` values in [0, max_value] must stay in [0, p) -- the range the identity refresh
    and `Client.decrypt` cover -- so group * max_value > p - 1 is refused; so is a group outside [1, 65536] (FBS_MAX_SUM_GROUP)."""
    group, max_value = int(group), int(max_value)
    if not 1 <= group <= 65536:
        raise ValueError("group %d outside [1, 65536]" % group)
    if max_value < 0:
        raise ValueError("max_value %d is negative" % max_value)
    if group * max_value > int(p) - 1:
        raise ValueError("a sum of %d values up to %d reaches %d, above p - 1 = %d: it would not decrypt"
                         % (group, max_value, group * max_value, int(p) - 1))
    return -(-int(T) // group), None if out_norm2 is None else np.asarray(out_norm2, np.float64).reshape(-1) * group


def plan_lookup(params, fold_factor, p, T_table, T_index, n_entries, digits, table_out_norm2, index_out_norm2, axis, min_margin=None):
    """The pure part of an encrypted-index read of resident state (include/fbs_exec.h, "encrypted-index reads"): -> (rounds,
    out_norm2) or ValueError.  `n_entries` entries per plane are read by an index of `digits` digits base p, least significant first,
    as a cascade of one primitive: round r cuts what round r - 1 left (round 0: the entries) into blocks of p and reads every block by
    digit r, so rounds[r] = ceil(n_entries / p^(r + 1)) lookups per plane and sample.  Every round folds its table
    (`fold_factor`: the server key's `fold_factor`, None without a fold key) and rotates it once:
    out_norm2 = `params.lookup_output_norm2(table_out_norm2, fold_factor, digits)`.  axis "rows": a plane's entries are rows of the
    table state, at the index's own sample (T_table == T_index) or shared by every sample (T_table == 1); axis "samples": they are
    the samples of one row, shared by every query, so n_entries == T_table <= p.  Refused: no fold key; no entry, or more than
    p^digits; a table whose T fits neither; an index that the rotation would read with less than `params.refresh_margin_needed(
    params, 1)`, the margin of a program's own bootstraps at norm2 = 1 (a bootstrap output meets it with equality); an output
    that, refreshed by the chain that reads it (out_norm2 > 1: `plan_chain` refreshes it), would keep less than `params.SET_MARGIN`, the 6 standard
    deviations `params.choose_params` and `params.fold_choice` ask of a set by default (a set chosen for another margin: pass it) -- at norm2 = 1 itself nothing that has been through a
    fold and a rotation can stay: 6.60 against 6.61 at the default (15, 70) set.  `min_margin`, when given, stands in for both."""
    from .params import SET_MARGIN, lookup_index_margin, lookup_output_norm2, refresh_margin, refresh_margin_needed
    p, n_entries, digits, T_table, T_index = int(p), int(n_entries), int(digits), int(T_table), int(T_index)
    if fold_factor is None:
        raise ValueError("the server key has no fold key: an encrypted-index read folds its table first")
    if axis not in ("rows", "samples"):
        raise ValueError("axis %r is neither 'rows' nor 'samples'" % (axis,))
    if digits < 1:
        raise ValueError("an index has at least one digit")
    if n_entries == 0:
        raise ValueError("a table has at least one entry")
    if n_entries > p ** digits:
        raise ValueError("%d entries are more than %d digit(s) base %d name (%d)" % (n_entries, digits, p, p ** digits))
    if axis == "rows" and T_table not in (1, T_index):
        raise ValueError("a table of %d samples is neither shared (1) nor the index's own (%d)" % (T_table, T_index))
    if axis == "samples" and (n_entries != T_table or n_entries > p):
        raise ValueError("along the samples a table is its state's %d samples, at most p = %d: %d entries asked" % (T_table, p, n_entries))
    need = refresh_margin_needed(params, 1.0) if min_margin is None else float(min_margin)
    need_out = SET_MARGIN if min_margin is None else float(min_margin)
    index_margin = lookup_index_margin(params, float(np.max(index_out_norm2)))
    if index_margin < need:
        raise ValueError("the index would be read at %.2f standard deviations, below the %.2f needed: refresh it first" % (index_margin, need))
    out_norm2 = lookup_output_norm2(float(np.max(table_out_norm2)), float(fold_factor), digits)
    out_margin = refresh_margin(params, None, out_norm2)
    if out_margin < need_out:
        raise ValueError("the entry read would refresh at %.2f standard deviations, below the %.2f needed: refresh the table first"
                         % (out_margin, need_out))
    return [-(-n_entries // p ** (r + 1)) for r in range(digits)], out_norm2


def plan_table(params, fold_factor, op, spread, n_entries, T_table, T_index=None, table_norm2=1.0, index_out_norm2=1.0, written=False,
               value_norm2=1.0, table_max=None, value_max=None, min_margin=None):
    """The pure part of a resident table (include/fbs_exec.h, "encrypted tables"): -> dict(norm2, max_value, out_norm2) or ValueError.
    op "create": `table_norm2` is the entries' own, and the table carries that and the fold.  op "read": out_norm2 =
    `params.table_read_norm2`.  op "add" / "set": norm2 = `params.table_write_norm2`, max_value the entries' new bound.
    Refused: no fold key; spread < 1, no entry, more than floor(p / spread); an index state that has not the tables' samples, or
    more than one sample writing a shared table; an index read with too little margin -- `params.lookup_index_margin` times spread
    on a table never written, times spread / 2 on a written one and for every write (half of an entry's wide box is what the
    other side's noise may use), against `params.refresh_margin_needed(params, 1)`; an add whose sum could leave [0, p); a write
    after which a read would refresh below `params.SET_MARGIN`.  `min_margin`, when given, stands in for both margins."""
    from .params import (SET_MARGIN, TABLE_ADD, TABLE_SET, lookup_index_margin, refresh_margin, refresh_margin_needed, table_read_norm2,
                         table_write_norm2)
    p, spread, n_entries, T_table = int(params.p_msg), int(spread), int(n_entries), int(T_table)
    if op not in ("create", "read", "add", "set"):
        raise ValueError("op %r is none of 'create', 'read', 'add', 'set'" % (op,))
    if fold_factor is None:
        raise ValueError("the server key has no fold key: a resident table is a fold, and so is every value written")
    if spread < 1:
        raise ValueError("an entry takes at least one box")
    if n_entries < 1:
        raise ValueError("a table has at least one entry")
    if n_entries > p // spread:
        raise ValueError("%d entries of %d boxes each are more than p = %d boxes hold (%d)" % (n_entries, spread, p, p // spread))
    table_norm2 = float(np.max(table_norm2))
    if op == "create":
        return dict(norm2=table_norm2 + float(fold_factor), max_value=table_max, out_norm2=None)
    T_index = int(T_index)
    writing = op != "read"
    if T_table != 1 and T_index != T_table:
        raise ValueError("an index of %d samples for tables of %d" % (T_index, T_table))
    if writing and T_table == 1 and T_index != 1:
        raise ValueError("a shared table is written by an index of one sample, not %d: their writes would have no order" % T_index)
    need = refresh_margin_needed(params, 1.0) if min_margin is None else float(min_margin)
    need_out = SET_MARGIN if min_margin is None else float(min_margin)
    margin = lookup_index_margin(params, float(np.max(index_out_norm2))) * (spread / 2.0 if writing or written else spread)
    if margin < need:
        raise ValueError("the index would be read at %.2f standard deviations, below the %.2f needed: refresh it first" % (margin, need))
    if not writing:
        out_norm2 = table_read_norm2(table_norm2)
        if refresh_margin(params, None, out_norm2) < need_out:
            raise ValueError("the entry read would refresh at %.2f standard deviations, below the %.2f needed: refresh the table first"
                             % (refresh_margin(params, None, out_norm2), need_out))
        return dict(norm2=table_norm2, max_value=table_max, out_norm2=out_norm2)
    if value_max is None or table_max is None:
        raise ValueError("a write needs the bounds of the table's entries and of the values")
    table_max, value_max = int(table_max), int(value_max)
    if value_max < 0:
        raise ValueError("max_value %d is negative" % value_max)
    new_max = value_max if op == "set" else table_max + value_max
    if new_max > p - 1:
        raise ValueError("a sum of entries up to %d and values up to %d reaches %d, above p - 1 = %d: it would not decrypt"
                         % (0 if op == "set" else table_max, value_max, new_max, p - 1))
    norm2 = table_write_norm2(table_norm2, float(np.max(value_norm2)), float(fold_factor), TABLE_SET if op == "set" else TABLE_ADD)
    after = refresh_margin(params, None, table_read_norm2(norm2))
    if after < need_out:
        raise ValueError("a read after this write would refresh at %.2f standard deviations, below the %.2f needed: the table's noise "
                         "budget is spent -- make a new server.table(...) of the refreshed entries()" % (after, need_out))
    return dict(norm2=norm2, max_value=new_max, out_norm2=None)


class ResidentTable:
    """Encrypted tables that stay folded on the server's GPU (`Server.table`; include/fbs_exec.h, "encrypted tables"): one table per
    plane and sample -- or one per plane, shared, where they were made of a state of one sample --, `n_entries` entries each, an entry
    taking `spread` boxes: an index holds spread * i.  `read` returns entries by an encrypted index, `add` and `set` write by one;
    `out_norm2`, `max_value` and `writes`, one figure a table (table (m, s) is number m T + s), follow the tables through their
    writes (`plan_table`): planes written with noisier or larger values age faster than the others."""

    def __init__(self, server, table, planes, n_entries, spread, T, out_norm2, max_value):
        self.server, self.table, self.planes = server, table, list(planes)
        self.n_entries, self.spread, self.T = int(n_entries), int(spread), int(T)
        per_plane = lambda x, dtype: np.repeat(np.broadcast_to(np.asarray(x, dtype), (len(self.planes),)), self.T)   # noqa: E731
        self.out_norm2, self.max_value = per_plane(out_norm2, np.float64), per_plane(max_value, np.int64)
        self.writes = np.zeros(len(self.planes) * self.T, np.int64)
        self.fingerprint = server.key.fingerprint

    def _of(self, m):
        """the tables of plane m"""
        return slice(m * self.T, (m + 1) * self.T)

    @property
    def closed(self):
        return self.table is None or bool(self.table.closed)

    def _index(self, index, index_name):
        if self.closed:
            raise ValueError("the resident table is closed")
        if not isinstance(index, ResidentOutputs) or index.closed:
            raise ValueError("the index is not an open ResidentOutputs")
        if index.server is not self.server or index.fingerprint != self.fingerprint:
            raise ValueError("the index is resident on another server")
        if index_name not in index.output_names:
            raise ValueError("no row named %s" % index_name)
        row = index.output_names.index(index_name)
        return row, 1.0 if index.out_norm2 is None else float(index.out_norm2[row])

    def _plan(self, op, m, T_index, index_norm2, **kw):
        """plane m's tables through `plan_table`"""
        key = self.server.key
        at = self._of(m)
        return plan_table(key.params, None if key.fold_bodies is None else key.fold_factor, op, self.spread, self.n_entries, self.T, T_index,
                          self.out_norm2[at], index_norm2, bool(self.writes[at].any()), table_max=int(self.max_value[at].max()), **kw)

    def read(self, index, index_name, out_names=None) -> "ResidentOutputs":
        """-> a `ResidentOutputs` of one row per plane (`out_names`, or the planes' names): at every sample the entry i of the plane's
        table, spread * i being the encrypted value of row `index_name` of `index` there"""
        row, i2 = self._index(index, index_name)
        out_norm2 = [self._plan("read", m, index.T, i2)["out_norm2"] for m in range(len(self.planes))]
        names = list(self.planes) if out_names is None else list(out_names)
        if len(names) != len(self.planes):
            raise ValueError("%d output names for %d planes" % (len(names), len(self.planes)))
        return ResidentOutputs(names, index.T, self.fingerprint, out_norm2, self.table.read(index.state, row), self.server)

    def _write(self, op, index, index_name, values, value_names, max_value):
        row, i2 = self._index(index, index_name)
        if not isinstance(values, ResidentOutputs) or values.closed or values.server is not self.server:
            raise ValueError("the values are not an open ResidentOutputs of this server")
        value_names = [value_names] if isinstance(value_names, str) else list(value_names)
        missing = [n for n in value_names if n not in values.output_names]
        if missing or len(value_names) != len(self.planes):
            raise ValueError("one value row a plane; no row named %s" % ", ".join(map(str, missing)) if missing else "one value row a plane")
        rows = [values.output_names.index(n) for n in value_names]
        v2 = np.ones(len(rows)) if values.out_norm2 is None else values.out_norm2[rows]
        bounds = np.broadcast_to(np.asarray(max_value, np.int64), (len(rows),))      # one bound, or one a plane
        plans = [self._plan(op, m, index.T, i2, value_norm2=float(v2[m]), value_max=int(bounds[m])) for m in range(len(rows))]
        if values.T != index.T:
            raise ValueError("values of %d samples for an index of %d" % (values.T, index.T))
        self.table.write(index.state, row, values.state, rows, mode=self.table.SET if op == "set" else self.table.ADD)
        for m, plan in enumerate(plans):                                             # (every plane was admitted before any was written)
            self.out_norm2[self._of(m)], self.max_value[self._of(m)] = plan["norm2"], plan["max_value"]
        self.writes += 1
        return self

    def add(self, index, index_name, values, value_names, max_value):
        """entry[i] += value in every table, i named by row `index_name` of `index` as for `read`; plane m's values are row
        value_names[m] of `values`, each at most `max_value` (an int, or one a plane).  Plain integer addition: refused when a sum could reach p."""
        return self._write("add", index, index_name, values, value_names, max_value)

    def set(self, index, index_name, values, value_names, max_value):
        """entry[i] = value: the old entry is read, refreshed and taken off the value, and the difference added"""
        return self._write("set", index, index_name, values, value_names, max_value)

    def entries(self):
        """-> a list of n_entries `ResidentOutputs` (the caller closes them), entry e of every table read out by a trivial index of
        spread * e -- no noise on the index: exact whatever the tables' writes were.  Each has the tables' samples."""
        if self.closed:
            raise ValueError("the resident table is closed")
        from .security import MODULUS
        prm = self.server.key.params
        delta = 2 * ((MODULUS + 2 * prm.p_msg) // (4 * prm.p_msg))
        out = []
        with self.server.ctx.state(1, self.T) as index:
            cts = np.zeros((1, self.T, prm.ct_words), np.uint64)
            for e in range(self.n_entries):
                cts[..., -1] = self.spread * e * delta % MODULUS
                index.put(cts)
                out.append(ResidentOutputs(["%s[%d]" % (pl, e) for pl in self.planes], self.T, self.fingerprint,
                                           [float(self.out_norm2[self._of(m)].max()) + 1.0 for m in range(len(self.planes))],
                                           self.table.read(index, 0), self.server))
        return out

    def fetch(self):
        """the tables' words, uint64 [tables][k+1][N] (table (m, s) is number m T + s)"""
        if self.closed:
            raise ValueError("the resident table is closed")
        return self.table.words()

    def close(self):
        if self.table is not None:
            self.table.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class SampleView:
    """The rows of a `ResidentOutputs` read through a sample map (`ResidentOutputs.samples`): T = len(index) samples, sample s the
    state's sample index[s], or a trivial ciphertext of `fill` where index[s] == SAMPLE_NONE.  A source of `Server.run_chain`
    like the `ResidentOutputs` under it (fbs_eval_resident_mapped gathers on the GPU); gathering changes no ciphertext, so the view
    carries the fingerprint and the per-row `out_norm2` of its state.  names: {row name of the state: its name in the view}, so
    that two views of one state can feed one evaluation.  It owns nothing: closing the state closes its views."""

    def __init__(self, base, index, fill=0, names=None):
        index = np.asarray(index)
        if index.ndim != 1 or index.size < 1 or index.dtype.kind not in "iu":
            raise ValueError("a sample map is a list of at least one sample number")
        bad = (index != SAMPLE_NONE) & ((index < 0) | (index >= base.T))
        if bad.any():
            s = int(np.flatnonzero(bad)[0])
            raise ValueError("sample %d reads sample %d of a state of %d" % (s, int(index[s]), base.T))
        self.base, self.index = base, np.ascontiguousarray(index, np.uint32)
        self.T = int(index.size)
        rows = list(base.output_names)
        names = {str(a): str(b) for a, b in (names or {}).items()}
        fills = fill if isinstance(fill, dict) else {n: fill for n in rows}
        unknown = sorted((set(names) | set(map(str, fills))) - set(rows))
        if unknown:
            raise ValueError("%s are not rows of the state" % unknown)
        self.output_names = [names.get(n, n) for n in rows]
        if len(set(self.output_names)) != len(rows):
            raise ValueError("names gives two rows of the view one name")
        self.fill = [int(fills.get(n, 0)) for n in rows]   # by row, the state's order

    fingerprint = property(lambda self: self.base.fingerprint)
    out_norm2 = property(lambda self: self.base.out_norm2)
    state = property(lambda self: self.base.state)
    server = property(lambda self: self.base.server)
    closed = property(lambda self: self.base.closed)


def client_choice(env, config: ExecConfig, programs=()):
    """The pure part of `Client`: (parameter set, fuse) of the server key.  programs=(): `config.choose_params_fuse` for env at the
    smallest p its tables need.  Otherwise one key for env and every program: p the largest any of them needs (or `fbs_size`),
    `config.params_choice(p, max norm2)`, and shared rotations only when `config.fuse_tables is True`."""
    everything = [env] + [e for e in programs if e is not env]
    lows = [e.lower() for e in everything]
    p = config.fbs_size or max(min_fbs_size(low["tables"]) for low in lows)
    for low in lows:
        for t in low["tables"]:
            if not table_is_valid(t, p):
                raise ValueError("table %s cannot be evaluated by one bootstrap at fbs_size %d" % (t, p))
    if not len(programs):
        return config.choose_params_fuse(env, p)
    fuse = config.fuse_tables is True
    norm2 = max((e.fusion_stats(p) if fuse else e.stats())["norm2_linprod"] for e in everything)
    return config.params_choice(p, norm2), fuse


def _host_client(host):
    """`Client(host=...)` -> bool: None takes the GPU context where its library is there, the host context where only the client
    library is"""
    if host is not None:
        return bool(host)
    import os
    from . import _client_native
    return not os.path.exists(_client_native.gpu_library_path()) and _client_native.client_library_present()


class Client:
    """Holds the secret.  Chooses (parameter set, fuse) for `env` with the rules of `ExecConfig.choose`, keys a context with
    `keygen_seeded`, encrypts inputs to bodies and decrypts outputs.

    programs: further programs the same server key has to evaluate (a chain, `Server.run_chain`).  The key then takes the largest
    p any of them needs and the set `config.params_choice(p, max norm2)` over all of them; tables share rotations only when
    `config.fuse_tables is True`.  With programs=() the choice is `env`'s alone, as before."""

    def __init__(self, env, config: ExecConfig | None = None, programs=(), packing=False, host=None, folding=False):
        """folding=True: the server key also carries a fold key (`ResidentOutputs.fold`, `FoldedOutputs`), at the parameters
        `params.fold_choice` gives for the largest norm2 of env and of every program and the margin the config chose the set for.
        The fold keygen is the GPU library's: with host=True it raises NotImplementedError.
        packing=True: the server key also carries a packing key (`Server.run_packed`, `PackedOutputs`), at the parameters
        `params.packing_choice` gives for the noisiest output of env and of every program; False (default): keys and files are
        what they were without it.
        host: where the client's own work runs.  True: on the host alone, through the client library (`HostContext`: no GPU, no
        ROCm); False: on a GPU context (`Context`), as before there was a choice; None (default): the GPU context where
        libfbsexec.so has been built, the host context where only the client library has.  Keys, inputs and decoded results
        are the same either way, and so are the files.  A host client has no device: it ignores `config.device_keys`."""
        self.env = env
        self.config = cfg = config or ExecConfig()
        self._low = env.lower()
        self.params, self.fuse_tables = client_choice(env, cfg, programs)
        self.host = _host_client(host)
        if folding and self.host:
            raise NotImplementedError("the fold keygen is in the GPU library (libfbsexec.so) only: Client(..., host=False, folding=True)")
        if self.host:
            from ._client_native import HostContext
            self.ctx = HostContext(self.params, seed=cfg.key_seed(), keygen=False)
        else:
            from ._native import Context
            self.ctx = Context(self.params, seed=cfg.key_seed(), device=cfg.device, keygen=False, device_keys=cfg.device_keys)
        self.ctx.keygen_seeded()
        self.packing = self.folding = None
        if packing or folding:
            from .params import fold_choice, packing_choice
            p = self.params.p_msg
            everything = [env] + [e for e in programs if e is not env]
            norm2 = [(e.fusion_stats(p) if self.fuse_tables else e.stats())["norm2_linprod"] for e in everything]
        if packing:
            worst = max(output_noise_factor(e.lower(), p, self.fuse_tables) for e in everything)
            self.packing = packing_choice(self.params, min(norm2), max(worst, 1.0))
            self.ctx.packing_keygen(*self.packing[:2])
        if folding:
            self.folding = fold_choice(self.params, max(norm2), float(getattr(cfg, "min_margin", 6.0)))
            self.ctx.fold_keygen(*self.folding)
        self._server_key = None
        self._public_key = None

    def server_key(self) -> ServerKey:
        if self._server_key is None:
            packing = {}
            if self.packing:
                packing = {k: v for k, v in self.ctx.export_packing_key().items() if k.startswith("packing_")}
            if self.folding:
                packing.update(self.ctx.export_fold_key())
            self._server_key = ServerKey(self.params, self.fuse_tables, **self.ctx.export_seeded_keys(), **packing)
        return self._server_key

    @property
    def fingerprint(self) -> bytes:
        return self.server_key().fingerprint

    def public_key(self):
        """-> `public.PublicKey`: what a third party needs to encrypt inputs for this client's server key (`public.PublicEncryptor`)
        -- the parameter set, the public mask key and k N words of bodies; no secret.  Made on the host (fbs_pub_keygen, from
        whichever library is there) from the exported GLWE key; its noise is drawn under a seed derived from the client's key seed
        under a label of its own, so the same client makes the same key."""
        from . import _public_native
        from .public import PublicKey, public_key_noise_seed
        if self._public_key is None:
            mask_key = self.server_key().mask_key
            sk = self.ctx.export_keys()["sk_glwe"]
            bodies = _public_native.keygen(self.params, mask_key, sk, public_key_noise_seed(self.config.key_seed()))
            sk[:] = 0
            self._public_key = PublicKey(self.params, mask_key, bodies)
        return self._public_key

    def encrypt(self, input_values, nonce0=None, names=None) -> EncryptedInputs:
        """{input name: array-like of bits} (the contract of `LutExecEnv.eval`) -> seeded ciphertexts.  nonce0: the first
        stream (None: the config's `nonce0`, or streams nobody has used).  names: the inputs to encrypt, in this order (None: every
        input of the client's program) -- a chain feeds some inputs of a program from earlier outputs (`Server.run_chain`)."""
        names = self._low["input_names"] if names is None else [str(n) for n in names]
        cols = [np.asarray(input_values[n]).reshape(-1) for n in names]
        T = max((len(c) for c in cols), default=1)
        bits = np.stack([np.broadcast_to(c, (T,)) for c in cols]).astype(np.int64) if cols else np.zeros((0, T), np.int64)
        assert bits.size == 0 or (bits.min() >= 0 and bits.max() <= 1), "inputs are bits"
        bodies, first = self.ctx.encrypt_seeded(bits, nonce0=self.config.nonce0 if nonce0 is None else nonce0)
        return EncryptedInputs(list(names), T, first, bodies.reshape(len(names), T), self.fingerprint)

    def decrypt(self, outputs, env=None):
        """EncryptedOutputs, CompactOutputs, PackedOutputs or FoldedOutputs (expanded on the host first) -> exactly what `LutExecEnv.eval` returns: {output name: np.ndarray of ints},
        constant outputs as python ints.  env: the program that computed them (None: the client's own; any program of a chain)."""
        low = self._low if env is None else env.lower()
        if outputs.fingerprint != self.fingerprint:
            raise ValueError("outputs were computed under another server key")
        if list(outputs.output_names) != list(low["out_names"]):
            raise ValueError("outputs belong to another program")
        if isinstance(outputs, FoldedOutputs):
            from . import _public_native
            count, words = len(low["out_names"]) * int(outputs.T), outputs.host_words()
            if words.size != folded_words(self.params, count):
                raise ValueError(f"{words.size} folded words do not fit this parameter set and {count} outputs")
            cts = _public_native.expand(self.params, words, count) if count else np.zeros((0, self.params.ct_words), np.uint64)
            out = (self.ctx.decrypt(cts) if count else np.zeros(0, np.int64)).reshape(len(low["out_names"]), int(outputs.T))
        elif isinstance(outputs, PackedOutputs):
            bits, count = int(outputs.bits), len(low["out_names"]) * int(outputs.T)
            words = np.ascontiguousarray(outputs.words, np.uint64).reshape(-1)
            if not self.params.log_n_poly + 1 <= bits <= 31 or words.size != packed_words(self.params, count, bits):
                raise ValueError(f"{words.size} packed words at {bits} bits do not fit this parameter set and {count} outputs")
            out = (self.ctx.decrypt_packed(words, count, bits) if count else np.zeros(0, np.int64)).reshape(len(low["out_names"]), int(outputs.T))
        elif isinstance(outputs, CompactOutputs):
            bits, words = int(outputs.bits), outputs.words
            if not self.params.log_n_poly + 1 <= bits <= 31 or words.shape[-1] != compact_words(self.params, bits):
                raise ValueError(f"compact ciphertexts of {words.shape[-1]} words at {bits} bits do not fit this parameter set")
            out = self.ctx.decrypt_compact(words, bits) if words.size else np.zeros(words.shape[:2], np.int64)
        else:
            out = self.ctx.decrypt(outputs.cts) if outputs.cts.size else np.zeros(outputs.cts.shape[:2], np.int64)
        result = {}
        for k, name in enumerate(low["out_names"]):
            w = low["out_wire"][k]
            result[name] = (-1 - w) if w < 0 else out[k].astype(int)
        return result


class Server:
    """Holds evaluation keys only (`Context.evaluation_only`).  Lowers each program itself and evaluates seeded inputs."""

    def __init__(self, server_key: ServerKey, device: int = 0, max_programs: int = 8, device_keys: bool = False):
        """device_keys=True: the server key's bodies are uploaded and expanded into full keys on the GPU, instead of on the host
        (`Context(device_keys=True)`); the evaluation keys, and every result, are the same."""
        from ._native import Context
        self.key = server_key
        self.ctx = Context.evaluation_only(server_key.params, server_key.mask_key, server_key.bsk_bodies, server_key.ksk_bodies,
                                           device=device, device_keys=device_keys)
        if server_key.packing_bodies is not None:
            self.ctx.import_packing_key(server_key.packing_levels, server_key.packing_base_bits, server_key.packing_bodies)
        if server_key.fold_bodies is not None:
            self.ctx.import_fold_key(server_key.fold_levels, server_key.fold_base_bits, server_key.fold_bodies)
        self.max_programs = max_programs
        self._programs = {}

    def program_for(self, env):
        from ._native import Program
        low = env.lower()
        hit = self._programs.get(id(low))
        if hit is not None and hit[1] is low:
            return hit[0], low
        p = self.key.params.p_msg
        for t in low["tables"]:
            if not table_is_valid(t, p):
                raise ValueError("table %s cannot be evaluated by one bootstrap at the server key's p = %d" % (t, p))
        tv = self.ctx.tvset(low["tables"])
        prog = Program(self.ctx, tv, len(low["input_names"]), low["kind"], low["arg0"], low["arg1"], low["const_coef"],
                       low["term_coef"], low["term_src"], low["out_wire"], fuse_tables=self.key.fuse_tables)
        prog._tv = tv
        if len(self._programs) >= max(1, self.max_programs):
            self._programs.pop(next(iter(self._programs)))[0].close()
        self._programs[id(low)] = (prog, low)
        return prog, low

    def run(self, env, inputs: EncryptedInputs, resident=False, plain=None, public=None):
        """-> `EncryptedOutputs`; resident=True: the outputs stay on the GPU (fbs_eval_resident) -> `ResidentOutputs`.
        plain: a `PlainInputs` with the inputs the server supplies in the clear; then `run_chain(env, [inputs, plain])`.
        public: a `public.PublicInputs` (or several) with the inputs a third party encrypted under the client's public key; likewise."""
        if plain is not None or public is not None:
            extra = [] if plain is None else [plain]
            if public is not None:
                extra += list(public) if isinstance(public, (list, tuple)) else [public]
            return self.run_chain(env, [inputs] + extra, resident=resident)
        if inputs.fingerprint != self.key.fingerprint:
            raise ValueError("inputs were encrypted for another server key")
        prog, low = self.program_for(env)
        if list(inputs.input_names) != list(low["input_names"]):
            raise ValueError("inputs belong to another program")
        if resident:
            feed = [("seeded", inputs.bodies[i], inputs.nonce0 + i * inputs.T) for i in range(len(low["input_names"]))]
            return self._resident(env, prog, low, feed, inputs.T, self._out_norm2(low))
        cts = prog.eval_seeded(inputs.bodies, inputs.T, inputs.nonce0)
        return EncryptedOutputs(list(low["out_names"]), inputs.T, cts, self.key.fingerprint, self._out_norm2(low))

    def compact_bits(self, env):
        """The width `run_compact` uses by default: `params.compact_output_bits` for the server key's parameter set, the program's
        norm2 (the statistic its parameter set was chosen for: `stats`, or `fusion_stats` when tables share rotations) and its
        worst output's noise (`output_noise_factor`)."""
        from .params import compact_output_bits
        prm, low = self.key.params, env.lower()
        norm2 = (env.fusion_stats(prm.p_msg) if self.key.fuse_tables else env.stats())["norm2_linprod"]
        return compact_output_bits(prm, norm2, output_noise_factor(low, prm.p_msg, self.key.fuse_tables))

    def run_compact(self, env, inputs: EncryptedInputs, bits=None) -> CompactOutputs:
        """`run` with compact outputs (fbs_eval_seeded_compact): [n_outputs][T][W] words instead of [n_outputs][T][kN + 1];
        bits=None: `compact_bits(env)`."""
        if inputs.fingerprint != self.key.fingerprint:
            raise ValueError("inputs were encrypted for another server key")
        prog, low = self.program_for(env)
        if list(inputs.input_names) != list(low["input_names"]):
            raise ValueError("inputs belong to another program")
        bits = self.compact_bits(env) if bits is None else int(bits)
        words = prog.eval_seeded_compact(inputs.bodies, inputs.T, inputs.nonce0, bits)
        return CompactOutputs(list(low["out_names"]), inputs.T, bits, words, self.key.fingerprint, self._out_norm2(low))

    def packed_bits(self, env, out_norm2=None):
        """The transport width `run_packed` uses by default: the narrowest at which `params.packed_output_margin`, at the server
        key's packing parameters and the outputs' worst noise factor, reaches `params.packed_margin_needed` for the program's
        norm2 (31 when none does)."""
        from .params import packed_margin_needed, packed_output_margin
        prm, low = self.key.params, env.lower()
        if self.key.packing_bodies is None:
            raise ValueError("the server key holds no packing key (Client(..., packing=True))")
        norm2 = (env.fusion_stats(prm.p_msg) if self.key.fuse_tables else env.stats())["norm2_linprod"]
        worst = output_noise_factor(low, prm.p_msg, self.key.fuse_tables) if out_norm2 is None else float(np.asarray(out_norm2).max(initial=0.0))
        need = packed_margin_needed(prm, norm2) * (1.0 - 1e-12)
        for bits in range(prm.log_n_poly + 1, 32):
            if packed_output_margin(prm, self.key.packing_levels, self.key.packing_base_bits, bits, worst) >= need:
                return bits
        return 31

    def run_packed(self, env, inputs: EncryptedInputs, bits=None) -> PackedOutputs:
        """`run` with packed outputs: evaluated resident (the outputs never leave the GPU as ciphertexts), then packed into GLWE
        samples under the client's key (fbs_state_fetch_packed); bits=None: `packed_bits(env)`.  A constant output travels as the
        packing of its trivial ciphertext."""
        if self.key.packing_bodies is None:
            raise ValueError("the server key holds no packing key (Client(..., packing=True))")
        bits = self.packed_bits(env) if bits is None else int(bits)
        with self.run(env, inputs, resident=True) as res:
            return res.fetch(packed=True, bits=bits)

    def _out_norm2(self, low, input_noise=None):
        return np.asarray(output_noise_factors(low, self.key.params.p_msg, self.key.fuse_tables, input_noise), np.float64)

    def _resident(self, env, prog, low, feed, T, out_norm2):
        from .params import compact_output_bits
        prm = self.key.params
        norm2 = (env.fusion_stats(prm.p_msg) if self.key.fuse_tables else env.stats())["norm2_linprod"]
        bits = compact_output_bits(prm, norm2, float(np.asarray(out_norm2).max(initial=0.0)))
        if T < 1 or not len(low["out_names"]):
            raise ValueError("resident outputs need at least one output and one sample")
        state = self.ctx.state(len(low["out_names"]), T)
        try:
            prog.eval_resident(feed, T, 0, state)
        except Exception:
            state.close()
            raise
        res = ResidentOutputs(list(low["out_names"]), T, self.key.fingerprint, out_norm2, state, self, bits)
        if self.key.packing_bodies is not None:
            res.packed_bits = self.packed_bits(env, out_norm2)
        return res

    def restore(self, outputs: EncryptedOutputs, compact_bits=None) -> "ResidentOutputs":
        """An `EncryptedOutputs` (a `ResidentOutputs.fetch()`, possibly saved and loaded) back into device memory
        (fbs_state_put).  compact_bits: the default width of a later fetch(compact=True) (None: it has to be passed then).
        A `FoldedOutputs` is expanded on the GPU by sample extraction (no key; a device-held one without a host copy); the rows
        then carry out_norm2 + fold_factor."""
        if outputs.fingerprint != self.key.fingerprint:
            raise ValueError("outputs were computed under another server key")
        if isinstance(outputs, FoldedOutputs):
            rows, T = len(outputs.output_names), int(outputs.T)
            size = outputs.words.numel() if outputs.on_device else np.asarray(outputs.words).size
            if not rows or T < 1 or size != folded_words(self.key.params, rows * T):
                raise ValueError(f"{size} folded words do not fit the server key's parameter set and {rows} outputs of {T} samples")
            state = self.ctx.state(rows, T)
            try:
                state.unfold(outputs.words if outputs.on_device else outputs.host_words())
            except Exception:
                state.close()
                raise
            out_norm2 = None if outputs.out_norm2 is None else outputs.out_norm2 + outputs.fold_factor
            return ResidentOutputs(list(outputs.output_names), T, self.key.fingerprint, out_norm2, state, self, compact_bits)
        cts = np.ascontiguousarray(outputs.cts, np.uint64)
        if cts.ndim != 3 or cts.shape[:2] != (len(outputs.output_names), outputs.T) or cts.shape[2] != self.key.params.ct_words or not cts.size:
            raise ValueError(f"ciphertexts of shape {cts.shape} do not fit the server key's parameter set")
        state = self.ctx.state(cts.shape[0], cts.shape[1])
        try:
            state.put(cts)
        except Exception:
            state.close()
            raise
        return ResidentOutputs(list(outputs.output_names), outputs.T, self.key.fingerprint, outputs.out_norm2, state, self, compact_bits)

    def run_chain(self, env, sources, rename=None, compact=False, bits=None, resident=False, refresh_public=False):
        """Evaluate `env` with each input taken by name from one of `sources`: the client's `EncryptedInputs` (seeded), the
        `EncryptedOutputs` / `CompactOutputs` of earlier evaluations under this server key, and the server's own `PlainInputs`
        (cleartext bits, written on the GPU as trivial ciphertexts: noise-free, no key) (fbs_eval_sources).  A `public.PublicInputs`
        (a third party's public-key encryptions) is expanded on the GPU into a state of its own (fbs_state_put_public), read like
        any resident row and freed after the evaluation, also when the evaluation raises.  rename: {input name:
        source name} for an input whose source carries another name.  Compact links, and full links whose producer was noisier
        than a bootstrap output, are refreshed on the GPU: one bootstrap each per sample.  compact=True: compact outputs at `bits`
        (None: the width `compact_bits` would pick for the noise these outputs carry).  `plan_chain` says what is refused.
        A source may also be a `ResidentOutputs` of this server (a closed one, or another server's, is refused): its rows are read
        on the GPU; so may a `SampleView` of one (`ResidentOutputs.samples`, `shift`, `broadcast`, `stride`), which reads the
        rows' samples through an index.  resident=True: the outputs stay there too -> `ResidentOutputs` (not with compact=True).
        refresh_public=True: public-key inputs are bootstrapped through the identity table before use even though their noise
        does not ask for it (one bootstrap per input and sample; they then go in with factor 1, as any refreshed link)."""
        from .params import public_input_factor, refresh_margin
        if resident and compact:
            raise ValueError("resident outputs are full ciphertexts: fetch(compact=True) compacts them when they leave the GPU")
        prm, fuse = self.key.params, self.key.fuse_tables
        sources = [sources] if isinstance(sources, _source_types()) else list(sources)
        for k, src in enumerate(sources):
            if isinstance(src, (ResidentOutputs, SampleView)) and not src.closed and (src.server is not self or src.state.ctx is not self.ctx):
                raise ValueError("source %d is resident on another server" % k)
        links, T = plan_chain(prm, fuse, self.key.fingerprint, env, sources, rename)
        if refresh_public:
            for ln in links:
                if ln.kind == "public" and not ln.refresh:
                    ln.refresh, ln.noise, ln.margin = True, 1.0, refresh_margin(prm, None, public_input_factor(prm))
        prog, low = self.program_for(env)
        expanded = {}   # source index -> the temporary state its public-key samples were expanded into
        try:
            for ln in links:
                if ln.kind == "public" and ln.source not in expanded:
                    src = sources[ln.source]
                    expanded[ln.source] = state = self.ctx.state(len(src.input_names), T)
                    state.put_public(src.samples)
                if ln.kind == "folded" and ln.source not in expanded:   # folded state: unfolded into a state of its own, likewise
                    src = sources[ln.source]
                    expanded[ln.source] = state = self.ctx.state(len(src.output_names), T)
                    state.unfold(src.words if src.on_device else src.host_words())
            return self._run_links(env, prog, low, sources, links, T, expanded, compact, bits, resident)
        finally:
            for state in expanded.values():   # (closing waits for the evaluations queued on the context)
                state.close()

    def lookup(self, table: "ResidentOutputs", entries, index: "ResidentOutputs", index_name, out_names=None, axis="rows") -> "ResidentOutputs":
        """Encrypted-index reads of resident state (include/fbs_exec.h, "encrypted-index reads"; fbs_state_lookup): for every sample
        of `index`, entry `i` of each plane of `table`, `i` being the encrypted value of row `index_name` at that sample -- or of
        several rows, digits base p, least significant first.  entries: a list of planes; axis "rows": each plane a list of row
        names of `table` (entry e = name e), read at the query's own sample, or at sample 0 where `table` has one sample (a shared
        table, folded once); axis "samples": each plane one row name, its entries being that row's samples.  Several digits run as
        a cascade of the one primitive: round 0 cuts each plane into blocks of p entries and reads every block by digit 0; the
        results, a temporary resident state, are the entries of round 1, read by digit 1, and so on (`plan_lookup`: ceil(E/p) +
        ceil(E/p^2) + .. lookups per plane and sample).  Temporaries are freed also when a round raises.  An index past the
        entries reads 0.  -> a `ResidentOutputs` of one row per plane (`out_names`, or lookup0, lookup1, ..) carrying
        `params.lookup_output_norm2`; a chain that reads it refreshes it (`plan_chain`: out_norm2 > 1).  `plan_lookup` says what
        is refused; so is a closed state or one resident on another server."""
        for what, res in (("table", table), ("index", index)):
            if not isinstance(res, ResidentOutputs) or res.closed:
                raise ValueError("the %s is not an open ResidentOutputs" % what)
            if res.server is not self or res.state.ctx is not self.ctx or res.fingerprint != self.key.fingerprint:
                raise ValueError("the %s is resident on another server" % what)
        prm = self.key.params
        p = prm.p_msg
        digit_names = [index_name] if isinstance(index_name, str) else list(index_name)
        planes = [list(pl) if axis == "rows" else [pl] for pl in entries]
        if not planes or any(len(pl) != len(planes[0]) for pl in planes):
            raise ValueError("every plane has the same number of entries, and there is at least one plane")

        def rows_of(res, names):
            missing = [n for n in names if n not in res.output_names]
            if missing:
                raise ValueError("no row named %s" % ", ".join(map(str, missing)))
            return [res.output_names.index(n) for n in names]
        digit_rows = rows_of(index, digit_names)
        cur_rows = [rows_of(table, pl) for pl in planes]
        used = sorted({r for pl in cur_rows for r in pl})
        t2 = np.ones(len(table.output_names)) if table.out_norm2 is None else table.out_norm2
        i2 = np.ones(len(index.output_names)) if index.out_norm2 is None else index.out_norm2
        n_entries = table.T if axis == "samples" else len(planes[0])
        fold_factor = None if self.key.fold_bodies is None else self.key.fold_factor
        _, out_norm2 = plan_lookup(prm, fold_factor, p, table.T, index.T, n_entries, len(digit_names), t2[used], i2[digit_rows], axis)
        names = ["lookup%d" % m for m in range(len(planes))] if out_names is None else list(out_names)
        if len(names) != len(planes):
            raise ValueError("%d output names for %d planes" % (len(names), len(planes)))
        cur, temps = table.state, []
        try:
            for r, digit in enumerate(digit_rows):
                if r == 0 and axis == "samples":
                    new = cur.lookup([pl[0] for pl in cur_rows], index.state, digit, axis=1)
                    temps.append(new)
                    cur_rows = [[m] for m in range(len(planes))]
                else:
                    blocks = [(m, pl[b:b + p]) for m, pl in enumerate(cur_rows) for b in range(0, len(pl), p)]
                    order = sorted(range(len(blocks)), key=lambda i: -len(blocks[i][1]))          # whole blocks first, then the tails
                    new = self.ctx.state(len(blocks), index.T)
                    temps.append(new)
                    at = 0
                    while at < len(order):                                                         # one call per block length: two at most
                        group = [i for i in order[at:] if len(blocks[i][1]) == len(blocks[order[at]][1])]
                        cur.lookup([blocks[i][1] for i in group], index.state, digit, out=new, out_row0=at, axis=0)
                        at += len(group)
                    row_of = {i: row for row, i in enumerate(order)}
                    cur_rows = [[row_of[i] for i, (m2, _) in enumerate(blocks) if m2 == m] for m in range(len(planes))]
                if len(temps) > 1:
                    temps.pop(0).close()
                cur = new
            assert all(len(pl) == 1 for pl in cur_rows)
            if [pl[0] for pl in cur_rows] != list(range(len(planes))):                             # (one block a plane: already in order)
                raise AssertionError("the last round leaves one row a plane, in order")
            return ResidentOutputs(names, index.T, self.key.fingerprint, np.full(len(planes), out_norm2), temps.pop(), self)
        finally:
            for st in temps:
                st.close()

    def table(self, state, entries, spread=2, max_value=None, names=None) -> "ResidentTable":
        """Writable encrypted tables of rows of `state` (include/fbs_exec.h, "encrypted tables"; fbs_table_create): `entries` is a list
        of planes, each a list of row names (entry e = name e), as at `lookup`'s axis "rows" -- a table per plane and sample, or one
        shared table per plane where `state` has one sample.  `state` is a `ResidentOutputs` of this server, or `PlainInputs`: the
        server's own cleartext bits (a histogram's zeros), laid out as trivial ciphertexts -- no client ciphertext, no noise; T None
        there is one sample, a shared table.  Folded ONCE, the tables stay on the GPU until the `ResidentTable` is closed; `state`
        itself is not needed afterwards.  An entry takes `spread` boxes (2: a write by a noisy index is safe, `plan_table`), so an
        index holds spread * i and a table floor(p / spread) entries.  max_value: the bound of the entries (None: p - 1, or the
        largest plain value), which `add` holds its sums to.  names: one per plane (plane0, plane1, ..)."""
        plain = isinstance(state, PlainInputs)
        if not plain:
            if not isinstance(state, ResidentOutputs) or state.closed:
                raise ValueError("the table is not an open ResidentOutputs")
            if state.server is not self or state.state.ctx is not self.ctx or state.fingerprint != self.key.fingerprint:
                raise ValueError("the table is resident on another server")
        row_names = state.input_names if plain else state.output_names
        T = (state.T or 1) if plain else state.T
        planes = [list(pl) for pl in entries]
        if not planes or any(len(pl) != len(planes[0]) for pl in planes):
            raise ValueError("every plane has the same number of entries, and there is at least one plane")
        missing = [n for pl in planes for n in pl if n not in row_names]
        if missing:
            raise ValueError("no row named %s" % ", ".join(map(str, missing)))
        rows = [[row_names.index(n) for n in pl] for pl in planes]
        t2 = np.zeros(len(row_names)) if plain else np.ones(len(row_names)) if state.out_norm2 is None else state.out_norm2
        prm = self.key.params
        if max_value is None:
            max_value = int(state.values.max()) if plain and state.values.size else prm.p_msg - 1
        if not 0 <= int(max_value) <= prm.p_msg - 1:
            raise ValueError("max_value %d outside [0, p - 1]" % max_value)
        fold_factor = None if self.key.fold_bodies is None else self.key.fold_factor
        norm2 = [plan_table(prm, fold_factor, "create", spread, len(pl), T, table_norm2=t2[pl], table_max=int(max_value))["norm2"] for pl in rows]
        names = ["plane%d" % m for m in range(len(planes))] if names is None else list(names)
        if len(names) != len(planes):
            raise ValueError("%d names for %d planes" % (len(names), len(planes)))
        if not plain:
            return ResidentTable(self, self.ctx.table(state.state, rows, spread), names, len(planes[0]), spread, T, norm2, max_value)
        from .security import MODULUS
        delta = 2 * ((MODULUS + 2 * prm.p_msg) // (4 * prm.p_msg))
        cts = np.zeros((len(row_names), T, prm.ct_words), np.uint64)   # trivial ciphertexts (0, .., 0, m Delta)
        for j in range(len(row_names)):
            cts[j, :, -1] = np.asarray(state.row(j), np.int64) * delta % MODULUS
        with self.ctx.state(len(row_names), T) as made:
            made.put(cts)
            return ResidentTable(self, self.ctx.table(made, rows, spread), names, len(planes[0]), spread, T, norm2, max_value)

    def fold(self, env, state: "ResidentOutputs", left, right, back=None, fill=0) -> "ResidentOutputs":
        """A tree reduction of the T samples of `state` to one, on the GPU: `env` combines two samples into one, and each round
        runs it resident at ceil(T / 2) samples on two views of the current state -- input `i` of `left` reads row left[i] at
        sample 2j, input `i` of `right` reads row right[i] at sample 2j + 1, or a ciphertext of `fill` (an int, or {row name:
        int}) where there is no such sample.  back: {output name of env: row name} under which the next round finds the rows it
        reads (None: the outputs carry the rows' names already).  -> a `ResidentOutputs` of one sample, its rows named through
        `back`.  Every round's state but the last is closed; `state` itself is left open.  With T = 1 already: a copy.
        ValueError, before anything runs, when left and right do not cover env's inputs exactly once or name a row that `state`
        or a round's renamed outputs do not hold."""
        left, right, back = fold_plan(env.lower(), list(state.output_names), left, right, back)
        if state.closed:
            raise ValueError("the resident outputs are closed")
        if state.T == 1:   # (sum_groups(1): a copy made on the GPU, word for word)
            return ResidentOutputs(list(state.output_names), 1, state.fingerprint, state.out_norm2, state.state.sum_groups(1), self, state.compact_bits)
        cur = state
        while cur.T > 1:
            half = -(-cur.T // 2)
            even, odd = 2 * np.arange(half, dtype=np.int64), 2 * np.arange(half, dtype=np.int64) + 1
            odd[odd >= cur.T] = SAMPLE_NONE
            rows = list(cur.output_names)
            views = [cur.samples(even, 0, {n: n + "@left" for n in rows}), cur.samples(odd, fill, {n: n + "@right" for n in rows})]
            rename = {**{i: r + "@left" for i, r in left.items()}, **{i: r + "@right" for i, r in right.items()}}
            try:
                nxt = self.run_chain(env, views, rename=rename, resident=True)
            finally:
                if cur is not state:
                    cur.close()
            nxt.output_names = [back.get(n, n) for n in nxt.output_names]
            cur = nxt
        return cur

    def _run_links(self, env, prog, low, sources, links, T, expanded, compact, bits, resident):
        from .params import compact_output_bits
        prm, fuse = self.key.params, self.key.fuse_tables
        feed = []
        for ln in links:
            src = sources[ln.source]
            if ln.kind == "seeded":
                feed.append(("seeded", src.bodies[ln.index], src.nonce0 + ln.index * src.T))
            elif ln.kind == "full":
                feed.append(("full", src.cts[ln.index], ln.refresh))
            elif ln.kind == "state":
                feed.append(("state", src.state, ln.index, ln.refresh) + (() if ln.sample_index is None else (ln.sample_index, ln.fill)))
            elif ln.kind in ("public", "folded"):
                feed.append(("state", expanded[ln.source], ln.index, ln.refresh))
            elif ln.kind == "plain":
                feed.append(("plain", src.row(ln.index)))
            else:
                feed.append(("compact", src.words[ln.index], int(src.bits)))
        out_norm2 = self._out_norm2(low, [ln.noise for ln in links])
        names = list(low["out_names"])
        run = prog.eval_resident if any(ln.kind in ("state", "public", "folded") for ln in links) else prog.eval_sources
        if resident:
            return self._resident(env, prog, low, feed, T, out_norm2)
        if not compact:
            return EncryptedOutputs(names, T, run(feed, T, 0), self.key.fingerprint, out_norm2)
        if bits is None:
            norm2 = (env.fusion_stats(prm.p_msg) if fuse else env.stats())["norm2_linprod"]
            bits = compact_output_bits(prm, norm2, float(out_norm2.max(initial=0.0)))
        bits = int(bits)
        return CompactOutputs(names, T, bits, run(feed, T, bits), self.key.fingerprint, out_norm2)


@dataclass
class ChainLink:
    """How one input of a chained evaluation is fed (`plan_chain`)."""
    name: str                     # the program's input
    source: int                   # which of the sources
    index: int                    # its row there (input or output position)
    kind: str                     # "seeded", "full", "compact", "state" (a row of a ResidentOutputs: full ciphertexts on the GPU), "plain", "public"
                                  # or "folded" (a row of a FoldedOutputs: unfolded on the GPU into a temporary state)
    refresh: bool                 # bootstrapped through the identity table before use
    noise: float                  # its noise factor going in: 0 fresh or plain, 1 refreshed, the producer's out_norm2 for a plain full link,
                                  # params.public_input_factor for a public-key input
    margin: float | None = None   # params.refresh_margin of a refreshed link
    sample_index: np.ndarray | None = None   # a "state" link through a `SampleView`: its sample map (uint32 [T]) ..
    fill: int = 0                            # .. and the message of the samples that read none (SAMPLE_NONE)


_SOURCE_TYPES = (EncryptedInputs, EncryptedOutputs, CompactOutputs, ResidentOutputs, SampleView, PlainInputs, FoldedOutputs)


def _source_types():
    from .public import PublicInputs      # (`public` imports this module)
    return _SOURCE_TYPES + (PublicInputs,)


def fold_plan(low, rows, left, right, back=None):
    """The pure part of `Server.fold`: -> (left, right, back) as dicts of str, or ValueError when left and right together do not feed
    every input of the program exactly once, name a row the state does not hold, or name one the outputs renamed through `back` do
    not hold (so that the second round could not run)."""
    left, right = ({str(a): str(b) for a, b in (m or {}).items()} for m in (left, right))
    back = {str(a): str(b) for a, b in (back or {}).items()}
    inputs, outs = list(low["input_names"]), list(low["out_names"])
    both = sorted(set(left) & set(right))
    if both or sorted(set(left) | set(right)) != sorted(inputs):
        raise ValueError("left and right feed inputs %s, the program has %s%s"
                         % (sorted(set(left) | set(right)), sorted(inputs), (" (%s in both)" % both) if both else ""))
    unknown = sorted(set(back) - set(outs))
    if unknown:
        raise ValueError("back names %s, which are not outputs of the program" % unknown)
    after = [back.get(n, n) for n in outs]
    if len(set(after)) != len(after):
        raise ValueError("back gives two outputs one name")
    needed = set(left.values()) | set(right.values())
    for where, have in (("the state", rows), ("the outputs renamed through back", after)):
        missing = sorted(needed - set(have))
        if missing:
            raise ValueError("%s holds no rows %s, which left and right read" % (where, missing))
    return left, right, back


def _names_of(src):
    return list(src.input_names if hasattr(src, "input_names") else src.output_names)


def plan_chain(params, fuse_tables, fingerprint, env, sources, rename=None, min_margin=None):
    """The pure part of `Server.run_chain`: -> ([ChainLink per input of env], T), or ValueError saying why not.

    Refused: a program whose own margin at `params` (`margin_sigmas` at its norm2: `fusion_stats` when tables share rotations) is
    below `min_margin` (None: `ExecConfig().min_margin`) or whose tables are invalid at the key's p; a source of another server
    key or another T; an input that no source, or more than one, names; an output set saved without `out_norm2`; a link whose
    refresh margin (`params.refresh_margin`) is below `params.refresh_margin_needed` at the program's norm2.  A full link whose
    producer's factor is at most 1 (a bootstrap output or a constant) goes in as it is: the program's parameter set assumes
    inputs no noisier than that.  Every other full link and every compact link is refreshed.  A `ResidentOutputs` is a full link
    whose ciphertexts are on the GPU (kind "state"), under the same rule; a closed one is refused.  A `SampleView` is its
    `ResidentOutputs` read through a sample map: the same link with the map and the row's fill attached (`sample_index`, `fill`), the
    same rule by the state's `out_norm2`; it counts with its own T = len(index), under the names it gives its rows.
    A `PlainInputs` is public and belongs to no key: no fingerprint is asked of it, its link is noise-free (kind "plain", noise 0)
    and never refreshed; one without T takes the chain's, and a program fed by such sources alone has no T and is refused.
    A `public.PublicInputs` (public-key encryptions by a third party) is held to the fingerprint and to T like an `EncryptedInputs`;
    its samples must have the shape the parameter set and T give (`public.public_sample_shape`).  Its noise factor is
    `params.public_input_factor`: at most 1, it goes in as it is (kind "public") with that factor as its noise; above, it is
    refreshed under exactly the full-link rule.
    A `FoldedOutputs` is a full link that has been through one fold (kind "folded"): its words must be the
    `folded_words(params, n_outputs T)` of the parameter set.  It goes in as it is, with noise out_norm2 + fold_factor, when its
    producer's factor is at most 1 (the full-link rule) and the program keeps `min_margin` with every such input that much
    noisier -- `margin_sigmas` recomputed with v_br (1 + fold_factor), what `params.fold_choice` chose the fold key for.
    Otherwise it is refreshed like any full link, at out_norm2 + fold_factor."""
    from .params import margin_sigmas, public_input_factor, refresh_margin, refresh_margin_needed, variances
    from .public import PublicInputs, public_sample_shape
    low = env.lower()
    p = params.p_msg
    for t in low["tables"]:
        if not table_is_valid(t, p):
            raise ValueError("table %s cannot be evaluated by one bootstrap at the server key's p = %d" % (t, p))
    norm2 = (env.fusion_stats(p) if fuse_tables else env.stats())["norm2_linprod"]
    floor = ExecConfig().min_margin if min_margin is None else float(min_margin)
    own = margin_sigmas(params, norm2)
    if own < floor - 1e-9:
        raise ValueError("the program's own margin at the server key's parameter set is %.2f sigma (norm2 %g), below %.2f: "
                         "key the chain for it (Client(..., programs=[...]))" % (own, norm2, floor))
    sources = list(sources)
    if not sources and low["input_names"]:
        raise ValueError("no sources for a program with inputs")
    T = None
    for k, src in enumerate(sources):
        if isinstance(src, PackedOutputs):
            raise ValueError("source %d is a PackedOutputs: a packed result is under the client's big key in GLWE form, for the client "
                             "only; link the EncryptedOutputs, CompactOutputs or ResidentOutputs of that evaluation instead" % k)
        if not isinstance(src, _source_types()):
            raise TypeError("source %d is a %s, not EncryptedInputs, EncryptedOutputs, CompactOutputs or ResidentOutputs, or PublicInputs or PlainInputs" % (k, type(src).__name__))
        if isinstance(src, (ResidentOutputs, SampleView)) and src.closed:
            raise ValueError("source %d is resident state that has been closed" % k)
        if not isinstance(src, PlainInputs) and src.fingerprint != fingerprint:
            raise ValueError("source %d was computed under another server key" % k)
        if src.T is None:   # (a PlainInputs of one value per input: the chain's T)
            continue
        if T is not None and src.T != T:
            raise ValueError("source %d has T = %d samples where the others have %d" % (k, src.T, T))
        T = src.T
    if T is None and sources and low["input_names"]:
        raise ValueError("every source is a PlainInputs without T (one value for all samples): the chain has no T; give one of them T")
    rename = {str(a): str(b) for a, b in (rename or {}).items()}
    unknown = sorted(set(rename) - set(low["input_names"]))
    if unknown:
        raise ValueError("rename names %s, which are not inputs of the program" % unknown)
    need = refresh_margin_needed(params, norm2)
    links = []
    for name in low["input_names"]:
        want = rename.get(name, name)
        hits = [(k, j) for k, src in enumerate(sources) for j, n in enumerate(_names_of(src)) if n == want]
        via = name if want == name else "%s (as %s)" % (name, want)
        if not hits:
            raise ValueError("input %s: no source holds it" % via)
        if len(hits) > 1:
            raise ValueError("input %s: ambiguous, held by sources %s" % (via, sorted({k for k, _ in hits})))
        k, j = hits[0]
        src = sources[k]
        if isinstance(src, EncryptedInputs):
            links.append(ChainLink(name, k, j, "seeded", False, 0.0))
            continue
        if isinstance(src, PlainInputs):
            links.append(ChainLink(name, k, j, "plain", False, 0.0))
            continue
        if isinstance(src, PublicInputs):
            shape, want_shape = tuple(np.shape(src.samples)), public_sample_shape(params, len(src.input_names), src.T)
            if shape != want_shape:
                raise ValueError("input %s: public-key samples of shape %s, the server key's parameter set and T = %d need %s"
                                 % (via, shape, src.T, want_shape))
            factor = public_input_factor(params)
            if factor <= 1.0:
                links.append(ChainLink(name, k, j, "public", False, factor))
                continue
            link = ChainLink(name, k, j, "public", True, 1.0, refresh_margin(params, None, factor))
            if link.margin < need * (1.0 - 1e-12):
                raise ValueError("input %s: its refresh would keep %.3f sigma (public-key noise factor %g), below the %.3f the program's "
                                 "bootstraps keep" % (via, link.margin, factor, need))
            links.append(link)
            continue
        if src.out_norm2 is None:
            raise ValueError("input %s: source %d was saved without out_norm2 (before chains existed), so the noise it carries is "
                             "unknown and it cannot be linked; it still decrypts" % (via, k))
        o2 = float(np.asarray(src.out_norm2).reshape(-1)[j])
        if isinstance(src, FoldedOutputs):
            size = src.words.numel() if src.on_device else np.asarray(src.words).size
            if size != folded_words(params, len(src.output_names) * src.T):
                raise ValueError("input %s: %d folded words do not fit the server key's parameter set and %d outputs of %d samples"
                                 % (via, size, len(src.output_names), src.T))
            v_br, v_ks, v_ms = variances(params)
            kept = (1.0 / (4.0 * p)) / math.sqrt(norm2 * v_br * (1.0 + src.fold_factor) + v_ks + v_ms)
            if o2 <= 1.0 and kept >= floor - 1e-9:
                links.append(ChainLink(name, k, j, "folded", False, o2 + src.fold_factor))
                continue
            link = ChainLink(name, k, j, "folded", True, 1.0, refresh_margin(params, None, o2 + src.fold_factor))
            if link.margin < need * (1.0 - 1e-12):
                raise ValueError("input %s: its refresh would keep %.3f sigma (out_norm2 %g, fold factor %g), below the %.3f the "
                                 "program's bootstraps keep" % (via, link.margin, o2, src.fold_factor, need))
            links.append(link)
            continue
        if isinstance(src, CompactOutputs):
            bits = int(src.bits)
            if not params.log_n_poly + 1 <= bits <= 31 or src.words.shape[-1] != compact_words(params, bits):
                raise ValueError("input %s: compact ciphertexts of %d words at %d bits do not fit the server key's parameter set"
                                 % (via, src.words.shape[-1], bits))
            link = ChainLink(name, k, j, "compact", True, 1.0, refresh_margin(params, bits, o2))
        else:
            kind = "state" if isinstance(src, (ResidentOutputs, SampleView)) else "full"
            if kind == "full" and src.cts.shape[-1] != params.ct_words:
                raise ValueError("input %s: ciphertexts of %d words, the server key's set has %d" % (via, src.cts.shape[-1], params.ct_words))
            mapped = {}
            if isinstance(src, SampleView):
                if not 0 <= src.fill[j] < 2 * p:
                    raise ValueError("input %s: fill %d outside [0, 2p) at the server key's p = %d" % (via, src.fill[j], p))
                mapped = dict(sample_index=src.index, fill=src.fill[j])
            if o2 <= 1.0:
                links.append(ChainLink(name, k, j, kind, False, o2, **mapped))
                continue
            link = ChainLink(name, k, j, kind, True, 1.0, refresh_margin(params, None, o2), **mapped)
        if link.margin < need * (1.0 - 1e-12):
            raise ValueError("input %s: its refresh would keep %.3f sigma (out_norm2 %g), below the %.3f the program's bootstraps keep"
                             % (via, link.margin, o2, need))
        links.append(link)
    return links, (T if T is not None else 0)
