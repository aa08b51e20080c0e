"""The live-key-table entry points (fpnn_aes_keyset_capacity / _set_keys / _clear in
include/fpnn_aes.h, fpnn_ecdh_accept in include/fpnn_ecdh.h) without a GPU: the front
library exports and forwards them, their argument checks come before any device work, and
with no GPU library to load they report what every forwarder reports."""
import ctypes as C
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fpnn_aes_keyset_capacity", "fpnn_aes_keyset_set_keys", "fpnn_aes_keyset_clear", "fpnn_ecdh_accept")


def test_symbols_exported_and_forwarded():
    import fpnn_amd
    front = C.CDLL(fpnn_amd.LIB_PATH)
    fwd = open(os.path.join(ROOT, "fpnn_amd", "csrc", "front_fwd.inc")).read()
    for name in NAMES:
        assert hasattr(front, name), name
        assert re.search(r"^FPNN_FWD\([^,]+, %s, " % name, fwd, flags=re.M), f"{name}: run gen_front.py"
        assert name in fpnn_amd._lib.SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "fpnn_aes.h")).read() + open(os.path.join(ROOT, "include", "fpnn_ecdh.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name


def test_null_table_rejected():
    import fpnn_amd
    lib = fpnn_amd.lib
    assert lib.fpnn_aes_keyset_capacity(None) == 0
    for count in (0, 3):
        assert lib.fpnn_aes_keyset_set_keys(None, 0, count, None, 0, None, None, None) == fpnn_amd.ERR_ARG
        assert lib.fpnn_aes_keyset_clear(None, 0, count, None, 0) == fpnn_amd.ERR_ARG
        # no engine, no private key, no table
        assert lib.fpnn_ecdh_accept(None, 0, None, None, count, None, 0, None, 0, None) == fpnn_amd.ERR_ARG
        assert lib.fpnn_ecdh_accept(None, 0, bytes(32), None, count, None, 0, None, 0, None) == fpnn_amd.ERR_ARG


def test_python_layer_has_the_calls():
    import fpnn_amd
    assert isinstance(fpnn_amd.KeySet.capacity, property)
    assert callable(fpnn_amd.KeySet.set_keys) and callable(fpnn_amd.KeySet.clear)
    assert callable(fpnn_amd.Engine.ecdh_accept)
    assert b"ecdh_accept" in fpnn_amd.lib.fpnn_aes_version()


def test_no_gpu_library_reports_nodev(tmp_path):
    """Fresh process (the front loads the GPU library once): the int calls return
    FPNN_AES_ERR_NODEV, the capacity 0."""
    code = ("import sys; sys.path.insert(0, %r); import fpnn_amd; l = fpnn_amd.lib; "
            "print(l.fpnn_aes_keyset_set_keys(None, 0, 0, None, 0, None, None, None), "
            "l.fpnn_aes_keyset_clear(None, 0, 0, None, 0), "
            "l.fpnn_ecdh_accept(None, 0, None, None, 0, None, 0, None, 0, None), "
            "fpnn_amd.ERR_NODEV, l.fpnn_aes_keyset_capacity(None))" % ROOT)
    env = dict(os.environ)
    env["FPNN_AES_GPU_LIB"] = str(tmp_path / "no_such_library.so")
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    a, b, c, nodev, cap = res.stdout.split()
    assert a == b == c == nodev and cap == "0"
