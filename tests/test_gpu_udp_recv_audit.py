"""The UDP receive kernels under the address audit (fpnn_amd/csrc/audit.hpp, `make audit`): every
global access of k_udp_walk and k_udp_take names its buffer through FA_AT / FA_SEG, and the audit
build checks each one against the buffer's extent and -- for datagram bytes -- the datagram's own
range.  The front library loads one GPU library per process, so the hostile-bytes, contract-breach
and take-order tests of tests/test_gpu_udp_recv.py run again in a child process with the audit
library: a walk that read one byte outside a datagram, or a take that indexed outside a table,
would come back as FPNN_AES_ERR_DEVICE from the call and fail the test there."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUDIT_LIB = os.path.join(ROOT, "fpnn_amd", "libfpnn_aes_gpu_audit.so")
SELECT = "hostile or ((take_breaches or slot_past or walk_only_then_take or plain_single or families) and 16-32)"


@pytest.mark.gpu
def test_receive_tests_pass_under_the_audit_library():
    blob = open(AUDIT_LIB, "rb").read()
    assert b"udp_walk" in blob and b"udp_take" in blob, "the audit build has no receive kernels"
    env = dict(os.environ, FPNN_AES_GPU_LIB=AUDIT_LIB)
    res = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider",
                          os.path.join(ROOT, "tests", "test_gpu_udp_recv.py"), "-k", SELECT],
                         capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    assert " passed" in res.stdout and "address audit" not in res.stderr, res.stdout[-2000:] + res.stderr[-2000:]
