"""Stream-mode host frames against the live key table (include/fpnn_aes.h:
fpnn_aes_stream_host_at; host_frames.hip): frames[i].key_slot names the table slot, for the key
and for the state, and the state stays in the DEVICE arrays fpnn_aes_stream_open wrote.

Expected bytes and states come from the oracle alone: StreamEncryptor semantics per slot, the
slot's frames in array order (tests/test_gpu_hostmap.py's _stream_expected over oracle.cfb),
starting from (IV of the slot, 0).  Every frame, every byte between the frames and the whole
device state arrays (fill pattern at unnamed and guard entries) are compared bit for bit.

The mapped path is checked in a fresh child process (this file run as a program) under
FPNN_AES_MAP_CHUNK_MB=1 -- the variable is read once per process -- so that streams split across
chunks; the child registers one arena once and carves every buffer out of it.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, os.path.join(ROOT, "oracle"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

IV_FILL, POS_FILL = 0xC3, 0x5A5A5A5A
GUARD = 8
CHILD_LIMIT_S = 150


def many_slots(rng):
    """300 slots, 1-5 frames each, interleaved in array order, 0-5000 bytes (the edge lengths
    among them) -> (lens, slot label per frame)."""
    per = [int(rng.integers(1, 6)) for _ in range(300)]
    labels = np.concatenate([np.full(k, s) for s, k in enumerate(per)])
    rng.shuffle(labels)
    lens = rng.integers(0, 5001, len(labels)).astype(np.uint32)
    lens[:6] = (0, 1, 15, 16, 17, 5000)
    first = {int(s): i for i, s in reversed(list(enumerate(labels)))}
    lens[[first[7], first[8]]] = 0  # slots 7 and 8: at least one empty frame
    for i in np.nonzero(labels == 9)[0]:
        lens[i] = 0                 # slot 9: empty frames only -- its state keeps every bit
    return lens, labels.astype(np.uint32)


def split_slots(rng):
    """40 slots x 1 MiB in 16 frames each, interleaved: more than one 32 MiB chunk, every
    stream split with its state carried by the slot."""
    labels = np.repeat(np.arange(40), 16)
    rng.shuffle(labels)
    return np.full(len(labels), 65536, dtype=np.uint32), labels.astype(np.uint32)


class Life:
    """A reserved table of T slots; the connections live in permuted slots below `bound`
    (set_keys -> stream_open on a send and a receive state pair, device arrays of bound + GUARD
    entries filled with a pattern first)."""

    def __init__(self, eng, rng, nconn, keylen, T, bound):
        import fpnn_amd
        import torch
        from test_gpu_parity import to_dev
        self.eng, self.T, self.bound, self.keylen = eng, T, bound, keylen
        self.slot_of = rng.permutation(bound)[:nconn].astype(np.uint32)
        self.keys = np.zeros((T, keylen), np.uint8)
        self.ivs = np.zeros((T, 16), np.uint8)
        self.keys[self.slot_of] = rng.integers(0, 256, (nconn, keylen), dtype=np.uint8)
        self.ivs[self.slot_of] = rng.integers(0, 256, (nconn, 16), dtype=np.uint8)
        self.ks = fpnn_amd.KeySet.reserve(eng, T, keylen)
        sl = to_dev(self.slot_of.astype(np.int32))
        self.ks.set_keys(to_dev(self.keys[self.slot_of].reshape(-1)), to_dev(self.ivs[self.slot_of].reshape(-1)),
                         slots=sl, slot_bound=T)
        self.state = []
        for _ in range(2):  # send pair, receive pair
            iv_d = torch.full((16 * (bound + GUARD),), IV_FILL, dtype=torch.uint8, device="cuda:0")
            pos_d = torch.full((bound + GUARD,), POS_FILL, dtype=torch.int32, device="cuda:0")
            self.ks.stream_open(iv_d, pos_d, slots=sl, slot_bound=bound)  # (queued: the host call sees it)
            iv_h = np.full((bound + GUARD, 16), IV_FILL, np.uint8)
            pos_h = np.full(bound + GUARD, POS_FILL, np.uint32)
            iv_h[self.slot_of], pos_h[self.slot_of] = self.ivs[self.slot_of], 0
            self.state.append([iv_d, pos_d, iv_h.reshape(-1), pos_h])

    def run(self, oracle, encrypt, fr, src, dst, what, path):
        """One fpnn_aes_stream_host_at call on the send (encrypt) or receive pair against the
        oracle; src / dst: the arenas the frames point into."""
        import fpnn_amd
        from test_gpu_hostmap import _stream_expected
        iv_d, pos_d, iv_h, pos_h = self.state[0 if encrypt else 1]
        exp, iv_e, pos_e = _stream_expected(oracle, encrypt, self.keys.reshape(-1), self.keylen, fr, src, dst.copy(),
                                            iv_h, pos_h, src.ctypes.data, dst.ctypes.data)
        self.eng.stream_host_at(encrypt, fr, self.ks, self.bound, iv_d, pos_d)
        assert self.eng.last_kernel(fpnn_amd.K_HOST) == path, self.eng.last_kernel(fpnn_amd.K_HOST)
        bad = np.nonzero(dst != exp)[0]
        assert len(bad) == 0, (what, "bytes", len(bad), bad[:8])
        got_iv, got_pos = iv_d.cpu().numpy(), pos_d.cpu().numpy().astype(np.uint32)
        assert np.array_equal(got_iv, iv_e) and np.array_equal(got_pos, pos_e), (what, "state")
        self.state[0 if encrypt else 1][2:] = [iv_e, pos_e]
        return exp


def round_trip(eng, oracle, rng, shape, keylen, path, carve):
    """Encrypt the shape's frames on the send pair, decrypt the ciphertext on the receive
    pair; carve(nbytes, fill) hands out the host buffers."""
    from test_gpu_hostmap import frames_array, place
    lens, labels = shape(rng)
    nconn = int(labels.max()) + 1
    life = Life(eng, rng, nconn, keylen, T=nconn + 100, bound=nconn + 60)
    try:
        soffs, ssize = place(rng, lens)
        doffs, dsize = place(rng, lens)
        src = carve(ssize, 0)
        src[:] = rng.integers(0, 256, ssize, dtype=np.uint8)
        dst = carve(dsize, 0x5A)
        back = carve(ssize, 0x3C)
        slots = life.slot_of[labels]
        fr = frames_array(src.ctypes.data, soffs, dst.ctypes.data, doffs, lens, slots)
        life.run(oracle, True, fr, src, dst, "encrypt", path)
        fr2 = frames_array(dst.ctypes.data, doffs, back.ctypes.data, soffs, lens, slots)
        life.run(oracle, False, fr2, dst, back, "decrypt", path)
        for i in range(0, len(lens), 7):
            s, L = int(soffs[i]), int(lens[i])
            assert np.array_equal(back[s:s + L], src[s:s + L]), i
        # the slot of empty frames only kept its opened state; both pairs end alike
        assert np.array_equal(life.state[0][2], life.state[1][2]) and np.array_equal(life.state[0][3], life.state[1][3])
    finally:
        life.ks.close()


def plain_buffer(nbytes, fill):
    return np.full(nbytes, fill, dtype=np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("keylen", [16, 32])
def test_staged_many_slots(engine, oracle, keylen):
    """9. 300 slots, 1-5 frames per slot interleaved in array order, 0-5000 bytes."""
    round_trip(engine, oracle, np.random.default_rng(9000 + keylen), many_slots, keylen, "host_staged", plain_buffer)


@pytest.mark.gpu
@pytest.mark.parametrize("keylen", [16, 32])
def test_staged_chunk_split(engine, oracle, keylen):
    """10. 40 slots x 1 MiB: the call spans more than one 32 MiB chunk, every stream continues
    in the second chunk from the state its slot holds."""
    round_trip(engine, oracle, np.random.default_rng(10000 + keylen), split_slots, keylen, "host_staged", plain_buffer)


@pytest.mark.gpu
def test_bad_slot_in_a_frame(engine, oracle):
    """12. One frame with key_slot == slot_bound (and slot_bound above the capacity):
    FPNN_AES_ERR_ARG before anything is queued -- no state byte and no dst byte changes."""
    import fpnn_amd
    from test_gpu_hostmap import frames_array, place
    rng = np.random.default_rng(12000)
    life = Life(engine, rng, 20, 16, T=64, bound=40)
    try:
        lens = rng.integers(1, 300, 50).astype(np.uint32)
        offs, size = place(rng, lens)
        src = rng.integers(0, 256, size, dtype=np.uint8)
        dst = np.full(size, 0x5A, np.uint8)
        slots = life.slot_of[rng.integers(0, 20, 50)]
        slots[33] = 40
        fr = frames_array(src.ctypes.data, offs, dst.ctypes.data, offs, lens, slots)
        iv_d, pos_d, iv_h, pos_h = life.state[0]
        engine.sync()
        for enc in (True, False):
            with pytest.raises(fpnn_amd.FpnnAesError) as ei:
                engine.stream_host_at(enc, fr, life.ks, 40, iv_d, pos_d)
            assert ei.value.status == fpnn_amd.ERR_ARG
        fr["key_slot"][33] = life.slot_of[0]
        import torch
        wide_iv = torch.zeros(16 * 80, dtype=torch.uint8, device="cuda:0")
        wide_pos = torch.zeros(80, dtype=torch.int32, device="cuda:0")
        with pytest.raises(fpnn_amd.FpnnAesError) as ei:
            engine.stream_host_at(True, fr, life.ks, 65, wide_iv, wide_pos)  # a bound above the capacity (64)
        assert ei.value.status == fpnn_amd.ERR_ARG
        assert not wide_iv.any() and not wide_pos.any()
        engine.sync()
        assert (dst == 0x5A).all()
        assert np.array_equal(iv_d.cpu().numpy(), iv_h) and np.array_equal(pos_d.cpu().numpy().astype(np.uint32), pos_h)
    finally:
        life.ks.close()


@pytest.mark.gpu
def test_mapped_path():
    """11. The same two shapes with every frame in one registered arena, 1 MiB chunks."""
    env = dict(os.environ, FPNN_AES_MAP_CHUNK_MB="1")
    cmd = ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable]
    if sys.flags.no_user_site:
        cmd.append("-s")
    r = subprocess.run(cmd + [os.path.abspath(__file__), "mapped-child"], env=env, capture_output=True, text=True)
    print(r.stdout)
    print(r.stderr, file=sys.stderr)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "mapped ok" in r.stdout


def _mapped_child():
    assert os.environ.get("FPNN_AES_MAP_CHUNK_MB") == "1"
    import fpnn_amd
    from pyoracle import Oracle
    from test_gpu_hostmap import aligned
    oracle = Oracle("port")
    eng = fpnn_amd.Engine(0)
    arena = aligned(160 << 20, 0)  # registered once, never unregistered while in use
    fpnn_amd.host_register(arena)
    try:
        for shape, keylen in ((many_slots, 16), (many_slots, 32), (split_slots, 32)):
            at = [0]

            def carve(nbytes, fill):
                a = arena[at[0]:at[0] + nbytes]
                at[0] += (nbytes + 4095) & ~4095
                assert at[0] <= len(arena)
                a[:] = fill
                return a
            round_trip(eng, oracle, np.random.default_rng(11000 + keylen), shape, keylen, "host_mapped", carve)
    finally:
        eng.sync()
        fpnn_amd.host_unregister(arena)
        eng.close()
    print("mapped ok")


if __name__ == "__main__" and sys.argv[1:] == ["mapped-child"]:
    _mapped_child()
