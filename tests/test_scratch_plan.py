"""The engine's scratch sizes (fpnn_amd/csrc/scratch_plan.hpp) on the CPU:
tests/cpp/scratch_plan_test.cpp includes that header alone (plain C++, no HIP) and checks the
capacity policy (1024 elements first, then doubling until the need is covered; no change while
the capacity suffices) and the contract of fpnn_aes_engine_reserve(max_segments, max_blocks):
for every call path, every segment count up to max_segments and block counts up to max_blocks,
each buffer's need is at most what reserve asks for it.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scratch_plan(tmp_path):
    exe = str(tmp_path / "scratch_plan_test")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests/cpp/scratch_plan_test.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.startswith("scratch_plan ok:"), r.stdout
