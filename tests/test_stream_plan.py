"""The chunk planner of the stream-mode host-frame calls (fpnn_amd/csrc/stream_plan.hpp) on
the CPU: tests/cpp/stream_plan_test.cpp includes that header alone (plain C++, no HIP),
drives StreamPlan::next_chunk over random and hand-made frame lists and checks every chunk:
each stream's pieces put together are its frames in array order with every byte once, a
chunk's segments are consecutive from state0, no stream gives more than its quota, a chunk
stops adding streams once it holds chunk_bytes, uniform_len is set exactly when the segment
lengths are equal, the plan ends with nothing left, and the sparse grouping equals the dense.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stream_plan(tmp_path):
    exe = str(tmp_path / "stream_plan_test")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests/cpp/stream_plan_test.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.startswith("stream_plan ok:"), r.stdout
