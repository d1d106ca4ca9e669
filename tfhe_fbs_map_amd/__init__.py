"""tfhe_fbs_map_amd -- MI355X-native executor for the FBS programs of ssmiler/tfhe_fbs_map.

`fbs_exec_env.LutExecEnv` (alias `FbsExecEnv`) is the drop-in for the reference's
fbs_mapper/fbs_exec_env.py; `_native` binds libfbsexec.so (C ABI: include/fbs_exec.h), which holds
the hand-written gfx950 kernels.  Importing the package loads the shared library and fails loudly
if it has not been built -- there is no CPU execution path here.

A client without a GPU.  Where libfbsexec.so is missing but the client library libfbsclient.so has been built
(`make -C tfhe_fbs_map_amd/csrc client`), the package imports all the same: `Params`, `params`, `fbs_exec_env` (builder, parsers,
`lower`, `stats`) and `split.Client` (keyed by `_client_native.HostContext`) work, and the first use of anything that needs the
GPU library -- `Context`, `Program`, `TvSet`, `Server`, `LutExecEnv.eval` -- raises the ImportError that the import itself raises
where neither library exists.  Nothing is ever evaluated on the CPU.

A public-key encryptor.  The same holds where only libfbspublic.so has been built (`make -C tfhe_fbs_map_amd/csrc public`): the
package imports, and `public.PublicKey`, `public.PublicEncryptor` and `public.PublicInputs` work on that library alone.
"""
import os as _os
import sys as _sys

from . import _client_native, _public_native

if _os.path.exists(_client_native.gpu_library_path()) or not (_client_native.client_library_present() or _public_native.public_library_present()):
    from . import _native
    from ._native import Context, Program, TvSet
else:   # the client library alone: `_native` becomes a stand-in that raises on the first use of the GPU library
    _native = _sys.modules[__name__ + "._native"] = _client_native.gpu_library_stand_in(__name__ + "._native")
from ._client_native import MODULUS, MODULUS_BITS, FbsError, HostContext, Params
from .fbs_exec_env import ExecConfig, FbsExecEnv, LutExecEnv, min_fbs_size, parse_fbs, parse_lbf, table_is_valid
from .netlist import BitExecEnv, map_basic, parse_blif, parse_bristol
from .params import P1024, P2048, bootstrap_cost, choose_params, margin_sigmas, params_for, security_bits, sigma_min
from .split import Client, EncryptedInputs, EncryptedOutputs, PlainInputs, Server, ServerKey
from .public import PublicEncryptor, PublicInputs, PublicKey


def __getattr__(name):   # (reached with the client library alone: what lives in the GPU binding raises its ImportError on use)
    if name in ("Context", "Program", "TvSet"):
        return getattr(_native, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


__all__ = ["Context", "HostContext", "FbsError", "Params", "Program", "TvSet", "ExecConfig", "FbsExecEnv", "LutExecEnv",
           "min_fbs_size", "parse_fbs", "parse_lbf", "table_is_valid", "P1024", "P2048", "margin_sigmas",
           "params_for", "bootstrap_cost", "choose_params", "security_bits", "sigma_min", "BitExecEnv", "map_basic", "parse_blif", "parse_bristol",
           "Client", "Server", "ServerKey", "EncryptedInputs", "EncryptedOutputs", "PlainInputs",
           "PublicKey", "PublicInputs", "PublicEncryptor"]
