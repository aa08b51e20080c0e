"""The host-mapped frame pipelines over many small chunks (FPNN_AES_MAP_CHUNK_MB=1): the
four-slot rotation of fpnn_aes_package_host / fpnn_aes_stream_host on registered memory is
passed twice (7-8 chunks), so a slot's staging, descriptor block and events are reused while
the chunks two and three steps back are still in flight.  The other GPU tests stay within
three chunks of the default 32 MiB.

The variable is read once per process, so the checks run in one fresh child process (this
file run as a program), under a time limit of its own; everything is compared with the
oracle byte for byte over the whole destination arena, the gaps between frames included."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CHILD_LIMIT_S = 120


@pytest.mark.gpu
def test_mapped_pipelines_reuse_their_slots():
    env = dict(os.environ, FPNN_AES_MAP_CHUNK_MB="1")
    cmd = ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable]
    if sys.flags.no_user_site:
        cmd.append("-s")
    r = subprocess.run(cmd + [os.path.abspath(__file__)], env=env, capture_output=True, text=True)
    print(r.stdout)
    print(r.stderr, file=sys.stderr)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "chunks ok" in r.stdout


# ---- the child ---------------------------------------------------------------------------

def _arena(held, nbytes, fill):
    import fpnn_amd
    from test_gpu_hostmap import aligned
    a = aligned(nbytes, fill)
    fpnn_amd.host_register(a)
    held.append(a)
    return a


def _package_expected(oracle, src, soffs, doffs, dsize, lens, slots, keys, keylen, ivs, pre):
    exp = np.full(dsize, 0xA5, dtype=np.uint8)
    for i in range(len(lens)):
        s, d, L = int(soffs[i]), int(doffs[i]), int(lens[i])
        if pre:
            exp[d:d + 4] = np.frombuffer(L.to_bytes(4, "little"), dtype=np.uint8)
        exp[d + pre:d + pre + L] = src[s:s + L]
    oracle.package_batch(True, exp.copy(), exp, len(lens), in_off=(doffs + pre).astype(np.uint64), lens=lens,
                         key_slot=slots, keys=keys, keylen=keylen, ivs=ivs, threads=8)
    return exp


def _same(got, exp, what):
    bad = np.nonzero(got != exp)[0]
    assert len(bad) == 0, (what, len(bad), bad[:8])


def _child_package(eng, oracle, held):
    import fpnn_amd
    from test_gpu_hostmap import frames_array, place
    rng = np.random.default_rng(20260)
    nkeys, keylen = 7, 32
    keys = rng.integers(0, 256, nkeys * keylen, dtype=np.uint8)
    ivs = rng.integers(0, 256, nkeys * 16, dtype=np.uint8)
    ks = fpnn_amd.KeySet(eng, keys.tobytes(), keylen, ivs.tobytes())
    lens = np.concatenate([rng.integers(0, 5001, 3000), [0, 1, 15, 16, 17]]).astype(np.uint32)
    rng.shuffle(lens)
    n = len(lens)
    assert int(lens.sum()) > (6 << 20)  # 7-8 chunks of 1 MiB: every slot of the four is used twice
    slots = rng.integers(0, nkeys, n).astype(np.uint32)
    soffs, ssize = place(rng, lens)
    src = _arena(held, ssize, 0)
    src[:] = rng.integers(0, 256, ssize, dtype=np.uint8)
    for pre in (0, 4):
        doffs, dsize = place(rng, lens)
        dst = _arena(held, dsize, 0xA5)
        fr = frames_array(src.ctypes.data, soffs, dst.ctypes.data, doffs, lens, slots)
        exp = _package_expected(oracle, src, soffs, doffs, dsize, lens, slots, keys, keylen, ivs, pre)
        eng.package_host_array(True, fr, ks, wire_prefix=bool(pre))
        assert eng.last_kernel(fpnn_amd.K_HOST) == "host_mapped"
        _same(dst, exp, f"mapped package encrypt, prefix {pre}")
        if pre:
            continue
        # partly mapped: one frame near two thirds of the array leaves registered memory
        out = i_out = None
        for i in range(2 * n // 3, n):
            if lens[i] > 100:
                i_out, out = i, np.full(int(lens[i]), 0x3C, dtype=np.uint8)
                break
        fr2 = fr.copy()
        fr2["dst"][i_out] = out.ctypes.data
        dst[:] = 0xA5
        eng.package_host_array(True, fr2, ks)
        assert eng.last_kernel(fpnn_amd.K_HOST) == "host_mapped+staged"
        d, L = int(doffs[i_out]), int(lens[i_out])
        exp2 = exp.copy()
        exp2[d:d + L] = 0xA5
        _same(dst, exp2, "partly mapped package encrypt")
        _same(out, exp[d:d + L], "partly mapped package encrypt, the frame outside")
        # decrypt in place
        dst[:] = exp
        fr3 = frames_array(dst.ctypes.data, doffs, dst.ctypes.data, doffs, lens, slots)
        eng.package_host_array(False, fr3, ks)
        assert eng.last_kernel(fpnn_amd.K_HOST) == "host_mapped"
        back = exp.copy()
        oracle.package_batch(False, exp.copy(), back, n, in_off=doffs.astype(np.uint64), lens=lens, key_slot=slots,
                             keys=keys, keylen=keylen, ivs=ivs, threads=8)
        assert all(np.array_equal(back[int(doffs[i]):int(doffs[i]) + int(lens[i])],
                                  src[int(soffs[i]):int(soffs[i]) + int(lens[i])]) for i in range(0, n, 50))
        _same(dst, back, "mapped package decrypt in place")
    # uniform frames on the same engine: the dense uniform batch, three chunks
    n, L = 3000, 1024
    lens = np.full(n, L, dtype=np.uint32)
    slots = rng.integers(0, nkeys, n).astype(np.uint32)
    perm = rng.permutation(n).astype(np.int64)
    usrc = _arena(held, n * L, 0)
    usrc[:] = rng.integers(0, 256, n * L, dtype=np.uint8)
    udst = _arena(held, n * L + 64, 0xA5)
    dpos = perm[::-1].copy() * L
    fr = frames_array(usrc.ctypes.data, perm * L, udst.ctypes.data, dpos, lens, slots)
    exp = _package_expected(oracle, usrc, perm * L, dpos, n * L + 64, lens, slots, keys, keylen, ivs, 0)
    eng.package_host_array(True, fr, ks)
    assert eng.last_kernel(fpnn_amd.K_HOST) == "host_mapped"
    _same(udst, exp, "mapped uniform package encrypt")


def _stream_frames(rng):
    """5 streams of about 1.5 MiB in frames of mixed sizes (empty ones at the start, in the
    middle and at the end; one frame longer than two quotas), stream 5 of empty frames only,
    stream 6 without a frame; interleaved in the array, each stream's frames in order."""
    per = []
    for s in range(5):
        target = int(rng.integers(1300 << 10, 1700 << 10))
        ls = [0, 0] if s % 2 == 0 else []
        if s == 1:
            ls.append(500000)  # more than two quotas of ~205 KiB: spans three chunks
        while sum(ls) < target:
            r = rng.random()
            ls.append(0 if r < 0.05 else int(rng.integers(1, 18)) if r < 0.2 else int(rng.integers(18, 5001))
                      if r < 0.97 else int(rng.integers(20000, 90000)))
        ls[-1] -= sum(ls) - target
        if s >= 3:
            ls.append(0)
        per.append(ls)
    per.append([0] * 20)
    labels = np.concatenate([np.full(len(ls), s) for s, ls in enumerate(per)])
    rng.shuffle(labels)
    cur = [0] * len(per)
    lens = []
    for s in labels:
        lens.append(per[s][cur[s]])
        cur[s] += 1
    return np.array(lens, dtype=np.uint32), labels.astype(np.uint32)


def _child_stream(eng, oracle, held):
    import fpnn_amd
    from test_gpu_hostmap import _stream_expected, frames_array, place
    rng = np.random.default_rng(20261)
    S, keylen = 7, 16
    lens, slots = _stream_frames(rng)
    soffs, ssize = place(rng, lens)
    doffs, dsize = place(rng, lens)
    src = _arena(held, ssize, 0x11)
    src[:] = rng.integers(0, 256, ssize, dtype=np.uint8)
    dst = _arena(held, dsize, 0x5A)
    keys = rng.integers(0, 256, S * keylen, dtype=np.uint8)
    ks = fpnn_amd.KeySet(eng, keys.tobytes(), keylen, bytes(16 * S))
    fr = frames_array(src.ctypes.data, soffs, dst.ctypes.data, doffs, lens, slots)
    for encrypt in (True, False):
        iv0 = rng.integers(0, 256, 16 * S, dtype=np.uint8)
        pos0 = rng.integers(0, 16, S).astype(np.uint32)
        dst[:] = 0x5A
        exp, iv_e, pos_e = _stream_expected(oracle, encrypt, keys, keylen, fr, src, dst.copy(), iv0, pos0,
                                            src.ctypes.data, dst.ctypes.data)
        iv, pos = iv0.copy(), pos0.copy()
        eng.stream_host_array(encrypt, fr, ks, iv, pos)
        assert eng.last_kernel(fpnn_amd.K_HOST) == "host_mapped"
        _same(dst, exp, f"mapped stream, encrypt={encrypt}")
        # every stream's state: the ciphered ones, the one of empty frames, the one never named
        assert np.array_equal(iv, iv_e) and np.array_equal(pos, pos_e), encrypt
        assert np.array_equal(iv[16 * 5:], iv0[16 * 5:]) and np.array_equal(pos[5:], pos0[5:]), encrypt


def _child():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), HERE]
    assert os.environ.get("FPNN_AES_MAP_CHUNK_MB") == "1"
    import fpnn_amd
    from pyoracle import Oracle
    oracle = Oracle("port")
    eng = fpnn_amd.Engine(0)
    held = []
    try:
        _child_package(eng, oracle, held)
        _child_stream(eng, oracle, held)
    finally:
        eng.sync()
        for a in held:
            fpnn_amd.host_unregister(a)
        eng.close()
    print("chunks ok")


if __name__ == "__main__":
    _child()
