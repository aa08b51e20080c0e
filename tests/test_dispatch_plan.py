"""Which kernel a device batch call runs on (fpnn_amd/csrc/dispatch_plan.hpp) on the CPU:
tests/cpp/dispatch_plan_test.cpp includes that header alone (plain C++, no HIP) and checks the
route of every call kind -- kernel family, layout, key mode, workgroup and grid, length order,
boundary save, scratch need -- against literals, on both sides of every threshold the choice has
(a full chip of chains, more chains than quads, the 2048- and 175-byte max_len bounds, two
blocks per segment, 2^32 blocks per batch, one key against many), at 256 CUs and again at 8.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dispatch_plan(tmp_path):
    exe = str(tmp_path / "dispatch_plan_test")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests/cpp/dispatch_plan_test.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.startswith("dispatch_plan ok:"), r.stdout
