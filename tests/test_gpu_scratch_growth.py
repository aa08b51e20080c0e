"""The engine's scratch buffers growing under queued work (fpnn_amd/csrc/engine_internal.hpp,
scratch_plan.hpp).

One engine that never calls reserve() runs sequences of device calls whose segment counts
cross a capacity step (the first capacity is 1024 elements, then doubling).  Within a sequence
every input is uploaded first and the calls are then queued back to back with no sync between
them, so a call that grows a buffer does so while the kernels of the call before it may still
read the old one: the old buffer must outlive them (freed behind the stream from the engine's
pool, or kept until the stream is idle when there is no pool).  Every call's whole output
buffer -- and for stream calls the whole state arrays -- is then compared with the oracle,
bit-exact, and the run ends with a sync that reports no device-side fault.

The sequences run twice: as the engine is by default, and with FPNN_AES_POOLS=0, where grown-out
buffers wait on the engine's deferred list.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from test_gpu_parity import keyset, to_dev, to_host  # noqa: E402
from test_gpu_stream_frames import PATTERN, Streams, oracle_rounds  # noqa: E402

pytestmark = pytest.mark.gpu

COUNTS = (900, 1100, 2300)  # below the first capacity (1024 elements), past it, past two doublings
KEYLEN = 16
NKEYS = 3


class Sequence:
    """Calls queued back to back, checked only after the last one is queued."""

    def __init__(self):
        self.calls, self.checks = [], []

    def add(self, call, check):
        self.calls.append(call)
        self.checks.append(check)

    def run(self):
        for call in self.calls:
            call()
        for check in self.checks:
            check()


def expect_equal(dev, exp, what):
    def check():
        got = to_host(dev)
        assert np.array_equal(got, exp), (what, int(np.count_nonzero(got != exp)))
    return check


def expect_all(*checks):
    def check():
        for c in checks:
            c()
    return check


def ragged_layout(rng, n, max_len, min_len=0):
    lens = rng.integers(min_len, max_len + 1, n).astype(np.int32)
    if min_len == 0:
        lens[:4] = (0, 15, 16, 17)
    offs = (np.concatenate([[0], np.cumsum(lens[:-1] + rng.integers(0, 4, n - 1))]) + 1).astype(np.int64)
    return lens, offs, int(offs[-1] + lens[-1]) + 16


class Keys:
    def __init__(self, engine, rng, nkeys=NKEYS):
        self.keys = rng.integers(0, 256, nkeys * KEYLEN, dtype=np.uint8)
        self.ivs = rng.integers(0, 256, nkeys * 16, dtype=np.uint8)
        self.ks = keyset(engine, self.keys, KEYLEN, self.ivs)
        self.n = nkeys


def package_call(seq, eng, oracle, rng, k, encrypt, n, max_len, inplace, what, min_len=0):
    lens, offs, total = ragged_layout(rng, n, max_len, min_len)
    slots = rng.integers(0, k.n, n).astype(np.int32)
    inp = rng.integers(0, 256, total, dtype=np.uint8)
    exp = inp.copy() if inplace else np.full(total, PATTERN, dtype=np.uint8)
    oracle.package_batch(encrypt, inp, exp, n, in_off=offs.astype(np.uint64), lens=lens.astype(np.uint32),
                         key_slot=slots.astype(np.uint32), keys=k.keys, keylen=KEYLEN, ivs=k.ivs, threads=4)
    src = to_dev(inp)
    dst = src if inplace else to_dev(np.full(total, PATTERN, dtype=np.uint8))
    kw = dict(in_off=to_dev(offs), lens=to_dev(lens), key_slot=to_dev(slots))
    fn = eng.package_encrypt if encrypt else eng.package_decrypt
    seq.add(lambda: fn(src, dst, n, k.ks, **kw), expect_equal(dst, exp, what))


def ragged_package(eng, oracle, rng, k):
    """bstart, plan, sink (K1r), perm and the length-order block (K2c in length order)."""
    seq = Sequence()
    for n in COUNTS:
        for inplace in (False, True):
            for encrypt in (False, True):
                package_call(seq, eng, oracle, rng, k, encrypt, n, 80, inplace, ("package", n, inplace, encrypt))
    seq.run()


def stream_call(seq, eng, oracle, rng, k, n, what, uniform=None):
    """One stream_decrypt of n streams (one segment each); uniform = (stride, length): no
    descriptor arrays, so K1r's are materialized in scratch."""
    if uniform:
        stride, length = uniform
        lens = np.full(n, length, dtype=np.int32)
        offs = (np.arange(n) * stride).astype(np.int64)
        total = n * stride + 16
    else:
        lens, offs, total = ragged_layout(rng, n, 80)
    slots = rng.integers(0, k.n, n).astype(np.int32)
    inp = rng.integers(0, 256, total, dtype=np.uint8)
    exp = np.full(total, PATTERN, dtype=np.uint8)
    iv = rng.integers(0, 256, n * 16, dtype=np.uint8)
    pos = rng.integers(0, 16, n).astype(np.uint32)
    iv_d, pos_d = to_dev(iv), to_dev(pos.astype(np.int32))
    oracle.stream_batch(False, inp, exp, n, in_off=offs.astype(np.uint64), out_off=offs.astype(np.uint64),
                        lens=lens.astype(np.uint32), key_slot=slots.astype(np.uint32), keys=k.keys, keylen=KEYLEN,
                        iv_state=iv, pos_state=pos, threads=4)
    src, dst = to_dev(inp), to_dev(np.full(total, PATTERN, dtype=np.uint8))
    kw = dict(key_slot=to_dev(slots))
    if uniform:
        kw.update(stride=stride, uniform_len=length)
    else:
        kw.update(in_off=to_dev(offs), lens=to_dev(lens))
    seq.add(lambda: eng.stream_decrypt(src, dst, n, k.ks, iv_d, pos_d, **kw),
            expect_all(expect_equal(dst, exp, what), expect_equal(iv_d, iv, (what, "iv")),
                       expect_equal(pos_d, pos.astype(np.int32), (what, "pos"))))


def stream_decrypt(eng, oracle, rng, k):
    """The state snapshot (snap_iv, snap_pos)."""
    seq = Sequence()
    for n in COUNTS:
        stream_call(seq, eng, oracle, rng, k, n, ("stream", n))
    seq.run()


def stride_batches(eng, oracle, rng, k):
    """No in_off / len and a partial last block (37 bytes every 48): the layout takes K1r, whose
    descriptor arrays are materialized (desc_off, desc_len)."""
    seq = Sequence()
    for n in COUNTS:
        stream_call(seq, eng, oracle, rng, k, n, ("stride", n), uniform=(48, 37))
    seq.run()


def frame_lens_for(rng, nseg):
    """Streams of 2-4 frames that hold nseg segments in all, lengths 0-80."""
    counts = [2, 3, 4] * (nseg // 9)
    rest = nseg - sum(counts)
    counts += {0: [], 1: [], 2: [2], 3: [3], 4: [4], 5: [2, 3], 6: [2, 4], 7: [3, 4], 8: [4, 4]}[rest]
    assert rest != 1 and sum(counts) == nseg
    counts = [counts[i] for i in rng.permutation(len(counts))]
    lens = [[int(x) for x in rng.integers(0, 81, c)] for c in counts]
    lens[0][:2] = (0, 15)
    lens[1][:2] = (16, 17)
    return lens


def frames_call(seq, eng, oracle, rng, k, nseg, at, inplace, what):
    """stream_decrypt_frames (keys by segment) or, at: _frames_at on a permuted state_slot in a
    table of one key per slot; the whole state arrays are checked."""
    st = Streams(rng, frame_lens_for(rng, nseg), dense=True)
    assert st.count == nseg
    entries = st.S + 5 if at else st.S
    if at:
        k = Keys(eng, rng, entries)
        slot_of_stream = rng.permutation(entries)[:st.S].astype(np.int32)
    else:
        slot_of_stream = rng.integers(0, k.n, st.S).astype(np.int32)
    inp = rng.integers(0, 256, st.total + 8, dtype=np.uint8)
    out_offs = st.offs if inplace else st.offs + 3
    exp = inp.copy() if inplace else np.full(st.total + 8, PATTERN, dtype=np.uint8)
    iv = rng.integers(0, 256, entries * 16, dtype=np.uint8)
    pos = rng.integers(0, 16, entries).astype(np.uint32)
    iv_d, pos_d = to_dev(iv), to_dev(pos.astype(np.int32))
    which = slot_of_stream if at else np.arange(st.S)  # the state entries of the streams
    iv_c = np.ascontiguousarray(iv.reshape(-1, 16)[which]).reshape(-1)
    pos_c = np.ascontiguousarray(pos[which])
    oracle_rounds(oracle, False, st, inp, exp, out_offs, slot_of_stream, k.keys, KEYLEN, iv_c, pos_c)
    iv.reshape(-1, 16)[which] = iv_c.reshape(-1, 16)
    pos[which] = pos_c
    src = to_dev(inp)
    dst = src if inplace else to_dev(np.full(st.total + 8, PATTERN, dtype=np.uint8))
    kw = dict(in_off=to_dev(st.offs), lens=to_dev(st.lens))
    if not inplace:
        kw["out_off"] = to_dev(out_offs)
    first = to_dev(st.first)
    if at:
        slot_d = to_dev(slot_of_stream)
        call = lambda: eng.stream_decrypt_frames_at(src, dst, st.count, k.ks, iv_d, pos_d, first, st.S, slot_d,  # noqa: E731
                                                    entries, **kw)
    else:
        kw["key_slot"] = to_dev(slot_of_stream[st.stream_of])
        call = lambda: eng.stream_decrypt_frames(src, dst, st.count, k.ks, iv_d, pos_d, first, st.S, **kw)  # noqa: E731
    seq.add(call, expect_all(expect_equal(dst, exp, what), expect_equal(iv_d, iv, (what, "iv")),
                             expect_equal(pos_d, pos.astype(np.int32), (what, "pos"))))
    return k


def frames(eng, oracle, rng, k):
    """The per-segment scratch of the *_frames decrypt (sf_*; sf_slot in the _at calls)."""
    seq = Sequence()
    tables = []
    for n in COUNTS:
        frames_call(seq, eng, oracle, rng, k, n, False, False, ("frames", n))
        tables.append(frames_call(seq, eng, oracle, rng, k, n, True, True, ("frames_at", n)))
    seq.run()
    for t in tables:
        t.ks.close()


def onepass_block_map(eng, oracle, rng, k):
    """More segments than the single-workgroup block map takes (16 384): the first use of the
    one-pass block map, whose look-back words must be zero when grown; then a small batch again."""
    seq = Sequence()
    package_call(seq, eng, oracle, rng, k, False, 16500, 32, False, ("onepass", 16500), min_len=1)
    package_call(seq, eng, oracle, rng, k, False, 2300, 80, False, ("after onepass", 2300))
    seq.run()


def dense_inplace(eng, oracle, rng, k):
    """In-place dense uniform decrypt: one saved boundary block per 64-block chunk
    (2 000, 66 000 and 140 000 blocks: 32, 1 032 and 2 188 chunks)."""
    seq = Sequence()
    for count in (1000, 33000, 70000):
        inp = rng.integers(0, 256, 32 * count, dtype=np.uint8)
        exp = inp.copy()
        oracle.package_batch(False, inp, exp, count, stride=32, uniform_len=32, keys=k.keys, keylen=KEYLEN, ivs=k.ivs,
                             threads=4)
        buf = to_dev(inp)
        seq.add(lambda buf=buf, count=count: eng.package_decrypt(buf, buf, count, k.ks, stride=32, uniform_len=32),
                expect_equal(buf, exp, ("dense in place", 2 * count)))
    seq.run()


@pytest.mark.parametrize("mode", ["pools", "deferred"])
def test_scratch_grows_under_queued_work(oracle, monkeypatch, mode):
    import fpnn_amd
    if mode == "deferred":
        monkeypatch.setenv("FPNN_AES_POOLS", "0")  # read when the engine is created
    eng = fpnn_amd.Engine(0)  # (never reserve()d)
    rng = np.random.default_rng(20261020)
    k = Keys(eng, rng)
    one = Keys(eng, rng, 1)
    try:
        ragged_package(eng, oracle, rng, k)
        stream_decrypt(eng, oracle, rng, k)
        frames(eng, oracle, rng, k)
        stride_batches(eng, oracle, rng, k)
        onepass_block_map(eng, oracle, rng, k)
        dense_inplace(eng, oracle, rng, one)
        eng.sync()  # raises unless FPNN_AES_OK: no device-side check failed anywhere above
    finally:
        k.ks.close()
        one.ks.close()
        eng.close()
