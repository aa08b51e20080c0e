"""The slot-addressed stream entry points (fpnn_aes_stream_open / _close,
fpnn_aes_stream_encrypt_frames_at / _decrypt_frames_at, fpnn_aes_stream_recv_at in
include/fpnn_aes.h) without a GPU: the front library exports and forwards them, their
argument checks come before any device work, and with no GPU library to load they report
what every forwarder reports."""
import ctypes as C
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fpnn_aes_stream_open", "fpnn_aes_stream_close", "fpnn_aes_stream_encrypt_frames_at",
         "fpnn_aes_stream_decrypt_frames_at", "fpnn_aes_stream_recv_at")


def test_symbols_exported_and_forwarded():
    import fpnn_amd
    front = C.CDLL(fpnn_amd.LIB_PATH)
    fwd = open(os.path.join(ROOT, "fpnn_amd", "csrc", "front_fwd.inc")).read()
    hdr = open(os.path.join(ROOT, "include", "fpnn_aes.h")).read()
    for name in NAMES:
        assert hasattr(front, name), name
        assert re.search(r"^FPNN_FWD\([^,]+, %s, " % name, fwd, flags=re.M), f"{name}: run gen_front.py"
        assert name in fpnn_amd._lib.SIGNATURES
        assert re.search(r"\b%s\s*\(" % name, hdr), name


def test_signatures_match_the_header():
    """Every parameter of the header's prototype has its ctypes entry (a count check: a
    dropped slot_bound would shift every pointer behind it)."""
    import fpnn_amd
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fpnn_aes.h")).read(), flags=re.S)
    for name in NAMES:
        params = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, hdr, flags=re.S).group(1)
        assert len(params.split(",")) == len(fpnn_amd._lib.SIGNATURES[name][1]), name


def test_null_arguments_rejected():
    import fpnn_amd
    lib = fpnn_amd.lib
    for count in (0, 3):
        assert lib.fpnn_aes_stream_open(None, 0, count, None, 0, None, None, None) == fpnn_amd.ERR_ARG
        assert lib.fpnn_aes_stream_close(None, 0, count, None, 0, None, None) == fpnn_amd.ERR_ARG
        # no engine, no batch
        assert lib.fpnn_aes_stream_encrypt_frames_at(None, None, None, count, None, 0, None, None) == fpnn_amd.ERR_ARG
        assert lib.fpnn_aes_stream_decrypt_frames_at(None, None, None, count, None, 0, None, None) == fpnn_amd.ERR_ARG
        assert lib.fpnn_aes_stream_recv_at(None, None, None, 0, None, None, None, 64, count, None, None,
                                           None) == fpnn_amd.ERR_ARG
    # a batch without an engine or a key set
    d = fpnn_amd._lib.BatchDesc()
    d.count = 2
    assert lib.fpnn_aes_stream_encrypt_frames_at(None, C.byref(d), None, 2, None, 0, None, None) == fpnn_amd.ERR_ARG
    assert lib.fpnn_aes_stream_recv_at(None, C.byref(d), None, 0, None, None, None, 64, 4, None, None,
                                       None) == fpnn_amd.ERR_ARG


def test_python_layer_has_the_calls():
    import fpnn_amd
    assert callable(fpnn_amd.KeySet.stream_open) and callable(fpnn_amd.KeySet.stream_close)
    for name in ("stream_encrypt_frames_at", "stream_decrypt_frames_at", "stream_recv_at"):
        assert callable(getattr(fpnn_amd.Engine, name)), name
    v = fpnn_amd.lib.fpnn_aes_version()
    assert b"stream_open" in v and b"frames_at" in v and b"recv_at" in v


def test_no_gpu_library_reports_nodev(tmp_path):
    """Fresh process (the front loads the GPU library once): every call returns
    FPNN_AES_ERR_NODEV."""
    code = ("import sys; sys.path.insert(0, %r); import fpnn_amd; l = fpnn_amd.lib; "
            "print(l.fpnn_aes_stream_open(None, 0, 0, None, 0, None, None, None), "
            "l.fpnn_aes_stream_close(None, 0, 0, None, 0, None, None), "
            "l.fpnn_aes_stream_encrypt_frames_at(None, None, None, 0, None, 0, None, None), "
            "l.fpnn_aes_stream_decrypt_frames_at(None, None, None, 0, None, 0, None, None), "
            "l.fpnn_aes_stream_recv_at(None, None, None, 0, None, None, None, 0, 0, None, None, None), "
            "fpnn_amd.ERR_NODEV)" % ROOT)
    env = dict(os.environ)
    env["FPNN_AES_GPU_LIB"] = str(tmp_path / "no_such_library.so")
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    vals = res.stdout.split()
    assert len(vals) == 6 and len(set(vals)) == 1, vals
