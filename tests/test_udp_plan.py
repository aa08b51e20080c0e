"""The UDP calls' host-only decisions (fpnn_amd/csrc/dispatch_plan.hpp: udp_check_args, udp_route;
scratch_plan.hpp: need_udp_decrypt) on the CPU: tests/cpp/udp_plan_test.cpp includes the plan
header alone (plain C++, no HIP) and checks every FPNN_AES_ERR_ARG / _ERR_KEYLEN case of
fpnn_aes_udp_encrypt / _decrypt, the encrypt kernel's route (template arguments, workgroup and
grid on both sides of each step, at 256 CUs and at 8), the scratch the decrypt composition needs,
and that fpnn_aes_engine_reserve(max_segments >= max(count, nsections, nconn), max_blocks) covers
both calls.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_udp_plan(tmp_path):
    exe = str(tmp_path / "udp_plan_test")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests/cpp/udp_plan_test.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.startswith("udp_plan ok:"), r.stdout
