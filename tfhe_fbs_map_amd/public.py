"""Public-key inputs: a third party encrypts for a keyed service (include/fbs_exec.h, "public-key inputs").

The key holder (`split.Client`) publishes a `PublicKey` beside the server key: the parameter set, the public mask key and k N
words of bodies -- k GLWE encryptions of zero.  A data owner who holds neither the secret key nor a GPU builds a
`PublicEncryptor` from it and encrypts inputs to `PublicInputs`: GLWE samples of N bits each, k + 1 words a bit on the wire.  The
server expands them on the GPU by sample extraction, straight into resident state (`Server.run_chain`, `Server.run(...,
public=...)`); it needs no key for that.  This module runs on libfbspublic.so alone (`make -C tfhe_fbs_map_amd/csrc public`).

IND-CPA only, and malleable like every ciphertext of this library: nothing proves to the server that a sample is well formed.
The noise and the encryptor's binary u come from the parameter set's sampler and inherit its caveats (`_client_native.
RANDOMNESS_GRADE`, `GAUSSIAN_SAMPLER_GRADE`).  One (seed, nonce) pair must never encrypt twice: the two samples would differ by
the difference of their messages.  `PublicEncryptor` draws its seed from the OS and counts its streams unless told otherwise.
"""
from __future__ import annotations

import hashlib
from dataclasses import asdict, dataclass

import numpy as np

from . import _public_native
from .split import FORMAT_VERSION, _PARAM_FIELDS, _fingerprint_of, _load_npz, mask_key_fingerprint

__all__ = ["PublicKey", "PublicInputs", "PublicEncryptor", "public_key_noise_seed", "public_sample_shape"]


def public_key_noise_seed(key_seed) -> bytes:
    """The 32-byte noise seed of a client's public key: its key seed (`ExecConfig.key_seed()`: an int or 32 bytes) under a label
    no other derivation uses, so that the same client makes the same key and the stream is shared with nothing."""
    raw = b"i" + int(key_seed).to_bytes(8, "little") if isinstance(key_seed, int) else b"b" + bytes(key_seed)
    return hashlib.sha256(b"tfhe_fbs_map_amd public key noise" + raw).digest()


def public_sample_shape(prm, n_inputs, T):
    """[G][k+1][N]: the samples that hold n_inputs * T bits, flattened [input][sample], N to a sample"""
    return (-(-int(n_inputs) * int(T) // prm.N), prm.k + 1, prm.N)


@dataclass
class PublicKey:
    """What an encryptor needs: the parameter set, the public mask key (the server key's) and the bodies [k][N].  No secret."""
    params: object
    mask_key: bytes
    bodies: np.ndarray

    def __post_init__(self):
        self.mask_key = bytes(self.mask_key)
        if len(self.mask_key) != 32:
            raise ValueError("a mask key has 32 bytes")
        self.bodies = np.ascontiguousarray(self.bodies, np.uint64).reshape(-1)
        want = self.params.k * self.params.N
        if self.bodies.size != want:
            raise ValueError(f"public-key bodies have {self.bodies.size} words, the parameter set needs {want}")
        self.bodies = self.bodies.reshape(self.params.k, self.params.N)

    @property
    def fingerprint(self) -> bytes:
        """the fingerprint of the server key it was made beside: inputs encrypted under it carry it"""
        return mask_key_fingerprint(self.mask_key)

    def save(self, path):
        prm = asdict(self.params)
        sampler = int(prm.get("sampler", 0))
        np.savez(path, kind=np.array("public_key"), format_version=np.array(FORMAT_VERSION),
                 params=np.array([int(prm[f]) for f in _PARAM_FIELDS], np.int64), mask_key=np.frombuffer(self.mask_key, np.uint8),
                 fingerprint=np.frombuffer(self.fingerprint, np.uint8), bodies=self.bodies,
                 **(dict(sampler=np.array(sampler, np.int64)) if sampler else {}))

    @classmethod
    def load(cls, path):
        from ._client_native import Params
        d = _load_npz(path, "public_key")
        vals = np.asarray(d["params"], np.int64)
        if vals.shape != (len(_PARAM_FIELDS),):
            raise ValueError("parameter record has the wrong length")
        prm = Params(sampler=int(d["sampler"]) if "sampler" in d else 0, **{f: int(v) for f, v in zip(_PARAM_FIELDS, vals)})
        if d["bodies"].dtype != np.uint64:
            raise ValueError("key bodies are uint64 words")
        key = cls(prm, np.asarray(d["mask_key"], np.uint8).tobytes(), d["bodies"])
        if _fingerprint_of(d) != key.fingerprint:
            raise ValueError("the saved fingerprint is not the mask key's")
        return key


@dataclass
class PublicInputs:
    """Public-key input ciphertexts of one evaluation: samples [G][k+1][N]; bit (input i, sample s) is message i*T + s of the
    batch, at coefficient (i*T + s) mod N of sample (i*T + s) / N."""
    input_names: list
    T: int
    samples: np.ndarray
    fingerprint: bytes

    def save(self, path):
        np.savez(path, kind=np.array("public_inputs"), format_version=np.array(FORMAT_VERSION),
                 input_names=np.array(list(self.input_names), dtype=str), T=np.array(self.T, np.int64),
                 samples=np.ascontiguousarray(self.samples, np.uint64), fingerprint=np.frombuffer(self.fingerprint, np.uint8))

    @classmethod
    def load(cls, path):
        d = _load_npz(path, "public_inputs")
        names = [str(n) for n in np.asarray(d["input_names"]).reshape(-1)]
        T = int(d["T"])
        samples = np.asarray(d["samples"])
        if samples.dtype != np.uint64 or samples.ndim != 3 or T < 1 or samples.shape[0] * samples.shape[2] < len(names) * T:
            raise ValueError(f"samples of shape {samples.shape} and type {samples.dtype} for {len(names)} inputs of {T} samples")
        return cls(names, T, samples, _fingerprint_of(d))


class PublicEncryptor:
    """Encrypts inputs under a `PublicKey`, with no secret and no GPU (libfbspublic.so).  seed: the 32 bytes the encryptor's own
    randomness is expanded from (None: from os.urandom).  Give each encryptor its own seed; one that restarts with the same seed
    must not reuse a nonce."""

    def __init__(self, public_key: PublicKey, seed=None):
        self.key = public_key
        self._enc = _public_native.Encryptor(public_key.params, public_key.mask_key, public_key.bodies, seed)

    def encrypt(self, input_values, names, nonce0=None) -> PublicInputs:
        """{input name: array-like of bits} -> `PublicInputs` for the inputs `names`, in this order.  nonce0: the first stream
        (sample g takes nonce0 + g); None: streams this encryptor has not used."""
        names = [str(n) for n in names]
        cols = [np.asarray(input_values[n]).reshape(-1) for n in names]
        if not cols:
            raise ValueError("no inputs to encrypt")
        T = max(len(c) for c in cols)
        bits = np.stack([np.broadcast_to(c, (T,)) for c in cols]).astype(np.int64)
        if bits.size and (bits.min() < 0 or bits.max() > 1):
            raise ValueError("inputs are bits")
        samples, _ = self._enc.encrypt(bits, nonce0=nonce0)
        return PublicInputs(names, T, samples, self.key.fingerprint)

    def close(self):
        self._enc.close()
