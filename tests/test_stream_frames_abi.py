"""The *_frames entry points of include/fpnn_aes.h without a GPU: argument checks come before
any device work, and with no GPU library to load the front reports FPNN_AES_ERR_NODEV."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_null_arguments_rejected():
    import fpnn_amd
    for fn in (fpnn_amd.lib.fpnn_aes_stream_encrypt_frames, fpnn_amd.lib.fpnn_aes_stream_decrypt_frames):
        assert fn(None, None, None, 0, None, None) == fpnn_amd.ERR_ARG
        assert fn(None, None, None, 3, None, None) == fpnn_amd.ERR_ARG


def test_python_layer_has_the_calls():
    import fpnn_amd
    assert callable(fpnn_amd.Engine.stream_encrypt_frames) and callable(fpnn_amd.Engine.stream_decrypt_frames)
    assert b"stream_encrypt_frames" in fpnn_amd.lib.fpnn_aes_version()


def test_no_gpu_library_reports_nodev(tmp_path):
    """The front library forwards the new symbols like every other: when the GPU library
    cannot be loaded they return FPNN_AES_ERR_NODEV (fresh process: the front loads it once)."""
    code = ("import sys; sys.path.insert(0, %r); import fpnn_amd; l = fpnn_amd.lib; "
            "print(l.fpnn_aes_stream_encrypt_frames(None, None, None, 0, None, None), "
            "l.fpnn_aes_stream_decrypt_frames(None, None, None, 0, None, None), fpnn_amd.ERR_NODEV)" % ROOT)
    env = dict(os.environ)
    env["FPNN_AES_GPU_LIB"] = str(tmp_path / "no_such_library.so")
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    a, b, nodev = res.stdout.split()
    assert a == b == nodev
