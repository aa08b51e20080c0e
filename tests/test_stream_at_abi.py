"""The one-frame-per-stream and host-frame entry points by key-table slot
(fpnn_aes_stream_encrypt_at / _decrypt_at, fpnn_aes_stream_host_at in include/fpnn_aes.h)
without a GPU: the front library exports and forwards them with no HIP dependency, the
Python layer binds them, and with no GPU library to load each reports FPNN_AES_ERR_NODEV."""
import ctypes as C
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fpnn_aes_stream_encrypt_at", "fpnn_aes_stream_decrypt_at", "fpnn_aes_stream_host_at")


def test_symbols_exported_and_forwarded():
    import fpnn_amd
    front = C.CDLL(fpnn_amd.LIB_PATH)
    fwd = open(os.path.join(ROOT, "fpnn_amd", "csrc", "front_fwd.inc")).read()
    hdr = open(os.path.join(ROOT, "include", "fpnn_aes.h")).read()
    for name in NAMES:
        assert hasattr(front, name), name
        assert re.search(r"^FPNN_FWD\([^,]+, %s, " % name, fwd, flags=re.M), f"{name}: run gen_front.py"
        assert re.search(r"\b%s\s*\(" % name, hdr), name


def test_front_library_has_no_hip_dependency():
    """The library callers link is plain C++: its dynamic section names no HIP / ROCm library."""
    import fpnn_amd
    res = subprocess.run(["readelf", "-d", fpnn_amd.LIB_PATH], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr
    needed = re.findall(r"\(NEEDED\)\s+Shared library: \[([^\]]+)\]", res.stdout)
    assert needed, res.stdout
    assert not [n for n in needed if re.search(r"hip|hsa|roc|amd", n, flags=re.I)], needed


def test_bound_in_lib_with_the_header_signature():
    """Every parameter of the header's prototype has its ctypes entry (a dropped slot_bound
    would shift every pointer behind it)."""
    import fpnn_amd
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fpnn_aes.h")).read(), flags=re.S)
    for name in NAMES:
        assert name in fpnn_amd._lib.SIGNATURES, name
        params = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, hdr, flags=re.S).group(1)
        assert len(params.split(",")) == len(fpnn_amd._lib.SIGNATURES[name][1]), name
        assert getattr(fpnn_amd.lib, name).restype is C.c_int
    for name in ("stream_encrypt_at", "stream_decrypt_at", "stream_host_at"):
        assert callable(getattr(fpnn_amd.Engine, name)), name


def test_no_gpu_library_reports_nodev(tmp_path):
    """Fresh process (the front loads the GPU library once): each call returns
    FPNN_AES_ERR_NODEV."""
    code = ("import sys; sys.path.insert(0, %r); import fpnn_amd; l = fpnn_amd.lib; "
            "print(l.fpnn_aes_stream_encrypt_at(None, None, None, 0, None, None), "
            "l.fpnn_aes_stream_decrypt_at(None, None, None, 0, None, None), "
            "l.fpnn_aes_stream_host_at(None, 1, None, 0, None, 0, None, None), "
            "fpnn_amd.ERR_NODEV)" % ROOT)
    env = dict(os.environ)
    env["FPNN_AES_GPU_LIB"] = str(tmp_path / "no_such_library.so")
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    vals = res.stdout.split()
    assert len(vals) == 4 and len(set(vals)) == 1, vals
