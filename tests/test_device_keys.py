"""Keys on the device, the parts that need no GPU: the option is off by default and reaches every public layer (`ExecConfig`,
`Context`, `Server`, the command line), and the header documents the knob and the two statistics."""
import inspect
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exec_config_leaves_the_keys_on_the_host_by_default():
    from tfhe_fbs_map_amd import ExecConfig
    assert ExecConfig().device_keys is False
    assert ExecConfig(device_keys=True).device_keys is True


def test_command_line_takes_the_option():
    from tfhe_fbs_map_amd.__main__ import build_parser
    ap = build_parser()
    assert ap.parse_args(["x.fbs"]).device_keys is False
    assert ap.parse_args(["x.fbs", "--device-keys"]).device_keys is True


def test_context_server_and_client_carry_the_parameter():
    from tfhe_fbs_map_amd import _native, split
    for fn in (_native.Context.__init__, _native.Context.evaluation_only.__func__, split.Server.__init__):
        param = inspect.signature(fn).parameters["device_keys"]
        assert param.default is False, fn
    assert "device_keys" in inspect.getsource(split.Client.__init__)            # passed on to its GPU context, ignored on the host
    assert "ignores" in split.Client.__init__.__doc__ and "device_keys" in split.Client.__init__.__doc__


def test_header_and_sources_name_the_knob_and_the_statistics():
    header = open(os.path.join(ROOT, "include", "fbs_exec.h")).read()
    for word in ('"keys_on_device" (0)', '"keys_made_on_device"', '"bsk_upload_bytes"'):
        assert word in header, word
    csrc = os.path.join(ROOT, "tfhe_fbs_map_amd", "csrc")
    assert '"keys_on_device"' in open(os.path.join(csrc, "fbs_select.cpp")).read()
    capi = open(os.path.join(csrc, "fbs_capi.cpp")).read()
    assert '"keys_made_on_device"' in capi and '"bsk_upload_bytes"' in capi
    makefile = open(os.path.join(csrc, "Makefile")).read()
    names = makefile.split("NAMES   :=")[1].split("\n")[0].split()
    assert "fbs_keygen.hip" in names
    client = makefile.split("CLIENT_NAMES  :=")[1].split("\n")[0]
    assert "fbs_keygen" not in client                                           # not client code
    for doc in ("DESIGN.md", "README.md"):
        assert "keys_on_device" in open(os.path.join(ROOT, doc)).read(), doc
