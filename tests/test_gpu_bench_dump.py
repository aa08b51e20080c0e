"""bench.py on the GPU: a plain run prints the headline line only, `--steps` sets the timed
steps, and `--dump-outputs` writes what the last timed step computed -- checked here against
the oracle on the same synthetic batch, at a size just past the sampling threshold."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_last_step_outputs(tmp_path, oracle):
    import bench
    import workloads as W
    P, L = bench.DUMP_PIECES + 904, 1024  # 5000 packets: more 1 KiB pieces than one array holds
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out_dir = str(tmp_path / "dump")
    cmd = [sys.executable, "-u", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--packets", str(P), "--length", str(L), "--dump-outputs", out_dir]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-3000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "GiB/s" and d["higher_is_better"] is True and d["dtype"] == "u8"
    assert d["ms_per_step"] > 0
    # value is the payload of both directions over the wall time of the timed steps
    # (ms_per_step is printed to 4 decimals: 0.5 % of a 0.01 ms step)
    assert d["ms_per_step"] >= 0.01
    assert d["value"] == pytest.approx(2.0 * P * L / (d["ms_per_step"] * 1e-3) / 2**30, rel=1e-2)
    assert d["full"] is False and not {"roofline", "cpu_baseline", "verify"} & set(d)

    plain = W.synth_bytes(P * L, W.C2["payload_seed"])
    key, iv = W.single_key(W.C2)
    exp = np.empty_like(plain)
    oracle.package_batch(True, plain, exp, P, in_off=np.arange(P, dtype=np.uint64) * L, lens=np.full(P, L, np.uint32),
                         key_slot=np.zeros(P, np.uint32), keys=np.frombuffer(key, np.uint8), keylen=len(key),
                         ivs=np.frombuffer(iv, np.uint8), threads=4)
    idx = bench.dump_sample_index(P * L)
    assert idx is not None and idx.size == bench.DUMP_PIECES * bench.DUMP_PIECE
    cipher = np.load(os.path.join(out_dir, "cipher.npy"))
    back = np.load(os.path.join(out_dir, "decrypted.npy"))
    assert cipher.dtype == np.float32 and back.dtype == np.float32
    assert sorted(os.listdir(out_dir)) == ["cipher.npy", "decrypted.npy"]
    assert np.array_equal(cipher, exp[idx].astype(np.float32))
    assert np.array_equal(back, plain[idx].astype(np.float32))
    assert d["dumped_outputs"]["cipher"] == {"values": int(idx.size), "of": P * L, "sampled": True}
