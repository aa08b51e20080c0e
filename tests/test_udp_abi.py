"""fpnn_aes_udp_encrypt / _decrypt (include/fpnn_aes.h) without a GPU: the front library exports
and forwards them, the Python layer binds them with the header's signature and the header's
struct layout, and what the calls check before they need a device is reported as the header
says.  (The argument checks that need an engine and key tables are a pure host function,
udp_check_args: tests/test_udp_plan.py runs every case of it; tests/test_gpu_udp.py runs them
again through the C-ABI on a device.)"""
import ctypes as C
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fpnn_aes_udp_encrypt", "fpnn_aes_udp_decrypt")


def test_symbols_exported_and_forwarded():
    import fpnn_amd
    front = C.CDLL(fpnn_amd.LIB_PATH)
    fwd = open(os.path.join(ROOT, "fpnn_amd", "csrc", "front_fwd.inc")).read()
    hdr = open(os.path.join(ROOT, "include", "fpnn_aes.h")).read()
    for name in NAMES + ("fpnn_aes_engine_scratch_bytes",):
        assert hasattr(front, name), name
        assert re.search(r"^FPNN_FWD\([^,]+, %s, " % name, fwd, flags=re.M), f"{name}: run gen_front.py"
        assert re.search(r"\b%s\s*\(" % name, hdr), name


def test_bound_with_the_header_signature_and_struct():
    import fpnn_amd
    from fpnn_amd._lib import SIGNATURES, UdpData
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fpnn_aes.h")).read(), flags=re.S)
    for name in NAMES:
        params = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, hdr, flags=re.S).group(1)
        assert len(params.split(",")) == len(SIGNATURES[name][1]) == 3, name
        assert getattr(fpnn_amd.lib, name).restype is C.c_int
    for name in ("udp_encrypt", "udp_decrypt", "scratch_bytes"):
        assert callable(getattr(fpnn_amd.Engine, name)), name
    # the struct: the header's fields in the header's order, at C's offsets on this ABI
    body = re.search(r"typedef struct \{([^}]*)\} fpnn_aes_udp_data;", hdr).group(1)
    fields = [re.findall(r"\w+", f)[-1] for f in body.split(";") if f.strip()]
    assert fields == [f[0] for f in UdpData._fields_]
    assert [getattr(UdpData, f).offset for f in fields] == [0, 8, 16, 24, 32, 36, 40, 48, 56, 64, 72]
    assert C.sizeof(UdpData) == 80


def test_null_arguments_are_err_arg():
    """No engine, no batch or no fpnn_aes_udp_data: FPNN_AES_ERR_ARG, whatever nconn is."""
    import fpnn_amd
    from fpnn_amd._lib import BatchDesc, UdpData
    for name in NAMES:
        fn = getattr(fpnn_amd.lib, name)
        assert fn(None, None, None) == fpnn_amd.ERR_ARG
        assert fn(None, C.byref(BatchDesc()), C.byref(UdpData())) == fpnn_amd.ERR_ARG
        assert fn(None, C.byref(BatchDesc()), None) == fpnn_amd.ERR_ARG
    assert fpnn_amd.lib.fpnn_aes_engine_scratch_bytes(None) == 0


def test_no_gpu_library_reports_nodev(tmp_path):
    """Fresh process (the front loads the GPU library once): each call returns
    FPNN_AES_ERR_NODEV."""
    code = ("import sys; sys.path.insert(0, %r); import fpnn_amd; l = fpnn_amd.lib; "
            "print(l.fpnn_aes_udp_encrypt(None, None, None), l.fpnn_aes_udp_decrypt(None, None, None), "
            "fpnn_amd.ERR_NODEV)" % ROOT)
    env = dict(os.environ)
    env["FPNN_AES_GPU_LIB"] = str(tmp_path / "no_such_library.so")
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    vals = res.stdout.split()
    assert len(vals) == 3 and len(set(vals)) == 1, vals
