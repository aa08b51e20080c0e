"""The UDP receive calls' host-only decisions (fpnn_amd/csrc/dispatch_plan.hpp: udp_recv_check_args,
udp_recv_route; scratch_plan.hpp: need_udp_decrypt over the segments) on the CPU: tests/cpp/udp_recv_plan_test.cpp
includes the plan header alone (plain C++, no HIP) and checks every FPNN_AES_ERR_ARG / _ERR_KEYLEN
case of fpnn_aes_udp_recv / _recv_take, which steps each flag combination queues and the scratch
they need, and that fpnn_aes_engine_reserve with the header's bound covers both calls.  The plan
header is host-only code, so the same program also runs under the address and undefined-behaviour
sanitizers, stand-alone.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests/cpp/udp_recv_plan_test.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_udp_recv_plan(tmp_path, flags):
    exe = str(tmp_path / "udp_recv_plan_test")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.startswith("udp_recv_plan ok:"), r.stdout
