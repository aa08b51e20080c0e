"""Many frames of each stream in one device call (fpnn_aes_stream_encrypt_frames /
fpnn_aes_stream_decrypt_frames, include/fpnn_aes.h; k_stream_frames.hip).

The contract: stream j owns segments [first_frame[j], first_frame[j+1]) of the batch, its
frames in order, and the bytes and the final (iv, pos) state equal that many successive
StreamEncryptor::encrypt / decrypt calls (core/Encryptor.cpp:53-70).  So the expected bytes
and states come from the oracle's stream_batch applied ROUND BY ROUND -- round r is every
stream's r-th frame, one segment per stream -- and, for the recorded sequences of
tests/golden/stream_cases.json, from the reference's own bytes.  Everything is bit-exact,
and every byte of the output buffer outside the segments must keep the pattern it was
filled with.

Run as a script (`python tests/test_gpu_stream_frames.py audit-child`) the module runs one
edge-shape case and prints "frames ok"; the audit test starts it in a fresh process with
FPNN_AES_GPU_LIB naming the address-audit build of the GPU library.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from test_gpu_parity import keyset, to_dev, to_host  # noqa: E402

pytestmark = pytest.mark.gpu

AUDIT_LIB = os.path.join(ROOT, "fpnn_amd", "libfpnn_aes_gpu_audit.so")
PATTERN = 0xA5


class Streams:
    """The frames of S streams as one batch: segments ordered by stream; each stream's
    frames laid out in REVERSE memory order, 1-7 bytes apart, at unaligned offsets."""

    def __init__(self, rng, frame_lens, dense=False):
        self.S = len(frame_lens)
        self.counts = np.array([len(f) for f in frame_lens], dtype=np.int64)
        self.first = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int32)
        self.count = int(self.first[-1])
        self.lens = np.array([x for f in frame_lens for x in f], dtype=np.int32)
        self.stream_of = np.repeat(np.arange(self.S), self.counts).astype(np.int32)
        if dense:  # (many streams: vectorised, forward order, 0-3 byte gaps)
            gaps = rng.integers(0, 4, self.count)
            self.offs = (np.concatenate([[0], np.cumsum(self.lens[:-1] + gaps[:-1])]) + 1).astype(np.int64)
            self.total = int(self.offs[-1] + self.lens[-1]) + 16 if self.count else 16
            return
        offs = np.zeros(self.count, dtype=np.int64)
        cur = 1 + int(rng.integers(0, 7))
        for j in range(self.S):
            for k in range(int(self.first[j + 1]) - 1, int(self.first[j]) - 1, -1):
                offs[k] = cur
                cur += int(self.lens[k]) + int(rng.integers(1, 8))
        self.offs = offs
        self.total = cur + 16

    def mask(self, offs, size=None):
        m = np.zeros(self.total + 8 if size is None else size, dtype=bool)
        for o, n in zip(offs, self.lens):
            m[o:o + n] = True
        return m


def oracle_rounds(oracle, encrypt, st, inp, exp, out_offs, slot_of_stream, keys, keylen, iv_h, pos_h):
    """Round r = every stream's r-th frame, one segment per stream, through the oracle's
    stream_batch; iv_h ([S * 16] uint8) and pos_h ([S] uint32) are advanced in place."""
    ivs = iv_h.reshape(st.S, 16)
    for r in range(int(st.counts.max()) if st.S else 0):
        js = np.nonzero(st.counts > r)[0]
        seg = st.first[js].astype(np.int64) + r
        iv_r = np.ascontiguousarray(ivs[js]).reshape(-1)
        pos_r = np.ascontiguousarray(pos_h[js])
        oracle.stream_batch(encrypt, inp, exp, len(js), in_off=np.ascontiguousarray(st.offs[seg].astype(np.uint64)),
                            out_off=np.ascontiguousarray(out_offs[seg].astype(np.uint64)),
                            lens=np.ascontiguousarray(st.lens[seg].astype(np.uint32)),
                            key_slot=np.ascontiguousarray(slot_of_stream[js].astype(np.uint32)), keys=keys,
                            keylen=keylen, iv_state=iv_r, pos_state=pos_r, threads=8)
        ivs[js] = iv_r.reshape(-1, 16)
        pos_h[js] = pos_r


class Session:
    """S streams with their keys and their carried state on the host (the oracle's) and on
    the device."""

    def __init__(self, engine, oracle, rng, S, keylen, per_stream_keys, pos0=None):
        self.engine, self.oracle, self.rng, self.S, self.keylen = engine, oracle, rng, S, keylen
        nkeys = S if per_stream_keys else 1
        self.keys = rng.integers(0, 256, nkeys * keylen, dtype=np.uint8)
        self.ks = keyset(engine, self.keys, keylen, rng.integers(0, 256, nkeys * 16, dtype=np.uint8))
        self.slot_of_stream = (np.arange(S) if per_stream_keys else np.zeros(S)).astype(np.int32)
        self.per_stream_keys = per_stream_keys
        self.iv_h = rng.integers(0, 256, S * 16, dtype=np.uint8)
        self.pos_h = rng.integers(0, 16, S).astype(np.uint32)
        if pos0 is not None:
            for j, p in enumerate(pos0):
                if p is not None:
                    self.pos_h[j] = p
        self.upload_state()

    def upload_state(self):
        self.iv_d, self.pos_d = to_dev(self.iv_h), to_dev(self.pos_h.astype(np.int32))

    def check_state(self, what):
        assert np.array_equal(to_host(self.iv_d), self.iv_h), what
        assert np.array_equal(to_host(self.pos_d).astype(np.uint32), self.pos_h), what

    def frames_call(self, encrypt, frame_lens, inplace, what, dense=False, st=None, data=None):
        """One *_frames call against the oracle's rounds; returns (Streams, input, output).
        st / data: a layout and an input buffer from an earlier call instead of new ones."""
        st = Streams(self.rng, frame_lens, dense) if st is None else st
        inp = self.rng.integers(0, 256, st.total + 8, dtype=np.uint8) if data is None else data
        out_offs = st.offs if inplace else st.offs + 3
        exp = inp.copy() if inplace else np.full(st.total + 8, PATTERN, dtype=np.uint8)
        before_iv, before_pos = self.iv_h.copy(), self.pos_h.copy()
        oracle_rounds(self.oracle, encrypt, st, inp, exp, out_offs, self.slot_of_stream, self.keys, self.keylen,
                      self.iv_h, self.pos_h)
        idle = np.array([int(st.lens[st.first[j]:st.first[j + 1]].sum()) == 0 for j in range(st.S)])
        assert np.array_equal(self.iv_h.reshape(-1, 16)[idle], before_iv.reshape(-1, 16)[idle])
        assert np.array_equal(self.pos_h[idle], before_pos[idle])
        src = to_dev(inp)
        dst = src if inplace else to_dev(np.full(st.total + 8, PATTERN, dtype=np.uint8))
        kw = dict(in_off=to_dev(st.offs), lens=to_dev(st.lens))
        if not inplace:
            kw["out_off"] = to_dev(out_offs)
        if self.per_stream_keys:
            kw["key_slot"] = to_dev(self.slot_of_stream[st.stream_of])
        fn = self.engine.stream_encrypt_frames if encrypt else self.engine.stream_decrypt_frames
        fn(src, dst, st.count, self.ks, self.iv_d, self.pos_d, to_dev(st.first), st.S, **kw)
        self.engine.sync()
        got = to_host(dst)
        assert np.array_equal(got, exp), (what, int(np.count_nonzero(got != exp)))
        self.check_state(what)
        return st, inp, got

    def single_frame_call(self, encrypt, what):
        """The existing one-frame-per-stream call on the same state."""
        S = self.S
        lens = self.rng.integers(0, 60, S).astype(np.int32)
        offs = np.concatenate([[0], np.cumsum(lens[:-1] + 3)]).astype(np.int64)
        inp = self.rng.integers(0, 256, int(offs[-1] + lens[-1]) + 16, dtype=np.uint8)
        exp = inp.copy()
        self.oracle.stream_batch(encrypt, inp, exp, S, in_off=offs.astype(np.uint64), out_off=offs.astype(np.uint64),
                                 lens=lens.astype(np.uint32), key_slot=self.slot_of_stream.astype(np.uint32),
                                 keys=self.keys, keylen=self.keylen, iv_state=self.iv_h, pos_state=self.pos_h, threads=8)
        buf = to_dev(inp)
        kw = dict(in_off=to_dev(offs), lens=to_dev(lens))
        if self.per_stream_keys:
            kw["key_slot"] = to_dev(self.slot_of_stream)
        fn = self.engine.stream_encrypt if encrypt else self.engine.stream_decrypt
        fn(buf, buf, S, self.ks, self.iv_d, self.pos_d, **kw)
        self.engine.sync()
        assert np.array_equal(to_host(buf), exp), what
        self.check_state(what)


# ---------------------------------------------------------------------------------------
# the frame-length rows of the edge-shape test: rng -> (incoming pos or None = random, lengths)


def _split(rng, total, parts):
    cuts = np.sort(rng.integers(0, total + 1, parts - 1))
    return [int(x) for x in np.diff(np.concatenate([[0], cuts, [total]]))]


def _row_to_boundary(blocks):
    def row(rng):
        p0 = int(rng.integers(0, 16))
        return p0, _split(rng, 16 * blocks - p0, 3)  # the state ends at pos == 0
    return row


ROWS = [
    lambda rng: (None, [0, 1, 2, 5, 0, 3, 9]),       # one cipher block spans many frames
    lambda rng: (None, []),                          # no frame at all, between two streams that have some
    lambda rng: (None, [3, 5000, 1, 0, 2]),          # several K1r chunks and interior runs between tiny frames
    lambda rng: (None, [0, 0, 0]),                   # only empty frames
    lambda rng: (3, [2, 4, 1]),                      # no block boundary reached: the state stays iv0-derived
    _row_to_boundary(1),
    _row_to_boundary(2),
    lambda rng: (None, [15, 16, 17]),
    lambda rng: (None, [127, 128, 129, 130]),        # K2c's 8-block step edge
]


def _rows_for(rng, S, first_row):
    rows = [ROWS[(first_row + j) % len(ROWS)](rng) for j in range(S)]
    return [r[1] for r in rows], [r[0] for r in rows]


def run_edge_shapes(engine, oracle, encrypt, keylen, per_stream_keys, inplace, stream_counts=(1, 3, 70)):
    rng = np.random.default_rng(7100 + keylen + 2 * encrypt + 4 * per_stream_keys + 8 * inplace)
    for S in stream_counts:
        # S == 1: every row as a call of its own; S == 3: the rows three at a time; 70: all at once
        starts = range(len(ROWS)) if S == 1 else range(0, len(ROWS), 3) if S == 3 else (0,)
        for first_row in starts:
            lens, pos0 = _rows_for(rng, S, first_row)
            what = (S, first_row)
            ses = Session(engine, oracle, rng, S, keylen, per_stream_keys, pos0)
            ses.frames_call(encrypt, lens, inplace, what + ("frames",))
            # the state carries on: into a second *_frames call, then into the one-frame call
            again = [[int(x) for x in rng.integers(0, 50, int(rng.integers(0, 5)))] for _ in range(S)]
            ses.frames_call(encrypt, again, inplace, what + ("second",))
            ses.single_frame_call(encrypt, what + ("single",))


# ---------------------------------------------------------------------------------------


def test_reference_fixtures(engine, golden):
    """1. Every recorded sequence as one stream whose frames are the recorded frames, all
    sequences of a key length in one call; outputs are the reference's own bytes."""
    import fpnn_amd
    cases = golden("stream_cases.json")
    for keylen in sorted({len(c["key"]) // 2 for c in cases}):
        for encrypt in (True, False):
            cs = [c for c in cases if len(c["key"]) // 2 == keylen and bool(c["encrypt"]) == encrypt]
            if not cs:
                continue
            rng = np.random.default_rng(keylen + encrypt)
            frames = [[bytes.fromhex(f["in"]) for f in c["frames"]] for c in cs]
            st = Streams(rng, [[len(f) for f in fr] for fr in frames])
            inp = np.full(st.total + 8, 0x11, dtype=np.uint8)
            exp = np.full(st.total + 8, PATTERN, dtype=np.uint8)
            k = 0
            for c, fr in zip(cs, frames):
                for f, rec in zip(fr, c["frames"]):
                    inp[st.offs[k]:st.offs[k] + len(f)] = np.frombuffer(f, np.uint8)
                    exp[st.offs[k]:st.offs[k] + len(f)] = np.frombuffer(bytes.fromhex(rec["out"]), np.uint8)
                    k += 1
            keys = np.frombuffer(b"".join(bytes.fromhex(c["key"]) for c in cs), np.uint8)
            ivs = np.frombuffer(b"".join(bytes.fromhex(c["iv"]) for c in cs), np.uint8)
            ks = keyset(engine, keys, keylen, ivs)
            iv_d, pos_d = to_dev(ivs), torch.zeros(len(cs), dtype=torch.int32, device="cuda:0")
            dst = to_dev(np.full(st.total + 8, PATTERN, dtype=np.uint8))
            fn = engine.stream_encrypt_frames if encrypt else engine.stream_decrypt_frames
            fn(to_dev(inp), dst, st.count, ks, iv_d, pos_d, to_dev(st.first), st.S, in_off=to_dev(st.offs),
               lens=to_dev(st.lens), key_slot=to_dev(st.stream_of))
            engine.sync()
            assert np.array_equal(to_host(dst), exp), (keylen, encrypt)
            # and the state the reference's StreamEncryptor is left with
            for j, (c, fr) in enumerate(zip(cs, frames)):
                se = fpnn_amd.StreamEncryptor(engine, bytes.fromhex(c["key"]), bytes.fromhex(c["iv"]))
                for f in fr:
                    se.encrypt(f) if encrypt else se.decrypt(f)
                assert to_host(iv_d)[16 * j:16 * j + 16].tobytes() == se.state[0]
                assert int(to_host(pos_d)[j]) == se.state[1]


@pytest.mark.parametrize("inplace", [False, True], ids=["outofplace", "inplace"])
@pytest.mark.parametrize("per_stream_keys", [False, True], ids=["onekey", "streamkeys"])
@pytest.mark.parametrize("keylen", [16, 24, 32])
@pytest.mark.parametrize("encrypt", [True, False], ids=["encrypt", "decrypt"])
def test_edge_shapes(engine, oracle, encrypt, keylen, per_stream_keys, inplace):
    """2. The frame-length rows above with 1, 3 and 70 streams (70: more than one wave of
    quads), random incoming (ivec, pos), then a second *_frames call and a one-frame call
    on the state the first one left."""
    run_edge_shapes(engine, oracle, encrypt, keylen, per_stream_keys, inplace)


def test_encrypt_reports_its_kernel(engine, oracle):
    import fpnn_amd
    rng = np.random.default_rng(5)
    ses = Session(engine, oracle, rng, 3, 16, True)
    ses.frames_call(True, [[40, 200], [7], [0, 129, 3]], False, "name")
    assert engine.last_kernel(fpnn_amd.K_ENCRYPT) == "cfb_encrypt_stream_frames"


def test_grid_stride_and_large_block_map(engine, oracle):
    """3. 66 000 streams x 3 frames of 0-40 bytes with per-stream keys: more streams than
    the 65 536 quads of a full grid, and more than 16 384 segments (the one-pass block map)."""
    rng = np.random.default_rng(66000)
    S = 66000
    lens = rng.integers(0, 41, (S, 3))
    lens[rng.random(S) < 0.05] = 0
    frame_lens = lens.tolist()
    ses = Session(engine, oracle, rng, S, 16, True)
    iv0, pos0 = ses.iv_h.copy(), ses.pos_h.copy()
    st, plain, cipher = ses.frames_call(True, frame_lens, True, "encrypt", dense=True)
    iv1, pos1 = ses.iv_h.copy(), ses.pos_h.copy()
    # back again from the same incoming state: the plaintext, and (CFB carries ciphertext
    # in both directions) the very state the encrypt call ended in
    ses.iv_h, ses.pos_h = iv0, pos0
    ses.upload_state()
    _, _, back = ses.frames_call(False, None, True, "decrypt", st=st, data=cipher)
    assert np.array_equal(back, plain)
    assert np.array_equal(ses.iv_h, iv1) and np.array_equal(ses.pos_h, pos1)


def _small_batch(engine, oracle, rng):
    ses = Session(engine, oracle, rng, 3, 16, True)
    lens = [[5, 40, 0], [17], [130, 2, 9, 33]]
    st = Streams(rng, lens)
    inp = rng.integers(0, 256, st.total + 8, dtype=np.uint8)
    kw = dict(in_off=to_dev(st.offs), lens=to_dev(st.lens), key_slot=to_dev(ses.slot_of_stream[st.stream_of]))
    return ses, lens, st, inp, kw


def test_arguments(engine, oracle):
    """4a. What the header says is FPNN_AES_ERR_ARG, and the calls that queue nothing."""
    import fpnn_amd
    rng = np.random.default_rng(41)
    ses, _, st, inp, kw = _small_batch(engine, oracle, rng)
    src, dst, first = to_dev(inp), to_dev(inp), to_dev(st.first)
    odd_iv = torch.zeros(16 * st.S + 16, dtype=torch.uint8, device="cuda:0")[1:]
    for fn in (engine.stream_encrypt_frames, engine.stream_decrypt_frames):
        for args, extra in (((ses.iv_d, ses.pos_d, None, st.S), {}),
                            ((None, ses.pos_d, first, st.S), {}),
                            ((ses.iv_d, None, first, st.S), {}),
                            ((odd_iv, ses.pos_d, first, st.S), {}),
                            ((ses.iv_d, ses.pos_d, first, st.S), {"flags": fpnn_amd.F_WIRE_PREFIX})):
            with pytest.raises(fpnn_amd.FpnnAesError) as ei:
                fn(src, dst, st.count, ses.ks, *args, **kw, **extra)
            assert ei.value.status == fpnn_amd.ERR_ARG
        fn(src, dst, st.count, ses.ks, None, None, None, 0, **kw)  # no stream
        fn(src, dst, 0, ses.ks, ses.iv_d, ses.pos_d, first, st.S, **kw)  # no segment
        engine.sync()
        assert np.array_equal(to_host(dst), inp)
        ses.check_state("nothing queued")


@pytest.mark.parametrize("encrypt", [True, False], ids=["encrypt", "decrypt"])
@pytest.mark.parametrize("table", ["past_count", "decreasing"])
def test_bad_table_is_reported_and_stays_in_bounds(engine, oracle, encrypt, table):
    """4b. A first_frame that runs past count, and one that decreases: what the kernels read
    from it is clamped into the batch, so no byte outside the segments changes; the next
    sync reports FPNN_AES_ERR_DEVICE; the following well-formed call is bit-exact."""
    import fpnn_amd
    rng = np.random.default_rng(43 + encrypt)
    ses, lens, st, inp, kw = _small_batch(engine, oracle, rng)
    bad = st.first.copy()
    if table == "past_count":
        bad[-1] = st.count + 5
    else:
        bad[1], bad[2] = bad[2], bad[1]
    out_offs = st.offs + 3
    dst = to_dev(np.full(st.total + 8, PATTERN, dtype=np.uint8))
    fn = engine.stream_encrypt_frames if encrypt else engine.stream_decrypt_frames
    fn(to_dev(inp), dst, st.count, ses.ks, ses.iv_d, ses.pos_d, to_dev(bad), st.S, out_off=to_dev(out_offs), **kw)
    with pytest.raises(fpnn_amd.FpnnAesError) as ei:
        engine.sync()
    assert ei.value.status == fpnn_amd.ERR_DEVICE
    outside = ~st.mask(out_offs)
    assert np.all(to_host(dst)[outside] == PATTERN)
    engine.sync()  # reported once
    ses.upload_state()  # (the bad call's state is invalid)
    ses.frames_call(encrypt, lens, False, "after the bad table")


def test_graph_replay(oracle):
    """5. After reserve: one encrypt-frames and one decrypt-frames call captured as a single
    chain, replayed with new data, lengths and first_frame in the same device arrays."""
    import fpnn_amd
    side = torch.cuda.Stream()
    eng = fpnn_amd.Engine(0, stream=side)
    try:
        S, nseg, cap, keylen = 300, 20000, 20000 * 70, 32  # > 16 384 segments: the one-pass block map
        rng = np.random.default_rng(909)
        keys = rng.integers(0, 256, S * keylen, dtype=np.uint8)
        ks = keyset(eng, keys, keylen, rng.integers(0, 256, S * 16, dtype=np.uint8))
        eng.reserve(nseg, cap // 16 + nseg)
        dev = dict(src=torch.zeros(cap, dtype=torch.uint8, device="cuda:0"),
                   mid=torch.zeros(cap, dtype=torch.uint8, device="cuda:0"),
                   back=torch.zeros(cap, dtype=torch.uint8, device="cuda:0"),
                   off=torch.zeros(nseg, dtype=torch.int64, device="cuda:0"),
                   len=torch.zeros(nseg, dtype=torch.int32, device="cuda:0"),
                   slot=torch.zeros(nseg, dtype=torch.int32, device="cuda:0"),
                   first=torch.zeros(S + 1, dtype=torch.int32, device="cuda:0"),
                   iv_e=torch.zeros(16 * S, dtype=torch.uint8, device="cuda:0"),
                   iv_d=torch.zeros(16 * S, dtype=torch.uint8, device="cuda:0"),
                   pos_e=torch.zeros(S, dtype=torch.int32, device="cuda:0"),
                   pos_d=torch.zeros(S, dtype=torch.int32, device="cuda:0"))

        def load(seed):
            r = np.random.default_rng(seed)
            counts = r.multinomial(nseg, r.dirichlet(np.ones(S)))  # always nseg segments, split anew
            st = Streams(r, [[int(x) for x in r.integers(0, 60, c)] for c in counts], dense=True)
            assert st.count == nseg and st.total + 8 <= cap
            data = r.integers(0, 256, cap, dtype=np.uint8)
            iv_h, pos_h = r.integers(0, 256, 16 * S, dtype=np.uint8), r.integers(0, 16, S).astype(np.uint32)
            with torch.cuda.stream(side):
                for name, a in (("src", data), ("off", st.offs), ("len", st.lens), ("slot", st.stream_of),
                                ("first", st.first), ("iv_e", iv_h), ("iv_d", iv_h), ("pos_e", pos_h.astype(np.int32)),
                                ("pos_d", pos_h.astype(np.int32))):
                    dev[name].copy_(torch.from_numpy(np.ascontiguousarray(a)))
                dev["mid"].fill_(PATTERN)
                dev["back"].fill_(PATTERN)
            exp = np.full(cap, PATTERN, dtype=np.uint8)
            oracle_rounds(oracle, True, st, data, exp, st.offs, np.arange(S), keys, keylen, iv_h, pos_h)
            plain = np.where(st.mask(st.offs, cap), data, PATTERN).astype(np.uint8)
            return exp, plain, iv_h, pos_h

        def run():
            kw = dict(in_off=dev["off"], lens=dev["len"], key_slot=dev["slot"])
            eng.stream_encrypt_frames(dev["src"], dev["mid"], nseg, ks, dev["iv_e"], dev["pos_e"], dev["first"], S, **kw)
            eng.stream_decrypt_frames(dev["mid"], dev["back"], nseg, ks, dev["iv_d"], dev["pos_d"], dev["first"], S, **kw)

        def check(expect, what):
            exp, plain, iv_h, pos_h = expect
            side.synchronize()
            assert np.array_equal(dev["mid"].cpu().numpy(), exp), what
            assert np.array_equal(dev["back"].cpu().numpy(), plain), what
            for iv, pos in ((dev["iv_e"], dev["pos_e"]), (dev["iv_d"], dev["pos_d"])):
                assert np.array_equal(iv.cpu().numpy(), iv_h), what
                assert np.array_equal(pos.cpu().numpy().astype(np.uint32), pos_h), what

        expect = load(1)  # an ordinary call first (code objects loaded, scratch at its final size)
        run()
        check(expect, "ordinary")
        load(2)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side, capture_error_mode="relaxed"):
            run()
        expect = load(3)  # capture does not execute: one replay, on new data
        with torch.cuda.stream(side):
            g.replay()
        check(expect, "replay")
        eng.sync()
        del g
    finally:
        eng.sync()
        eng.close()


def test_audit_library():
    """6. One edge-shape case through the address-audit build of the GPU library, in a fresh
    process: FPNN_AES_OK (no access outside its extent or its segment) and bit-exact."""
    assert os.path.exists(AUDIT_LIB), "make -C fpnn_amd/csrc audit"
    env = dict(os.environ)
    env["FPNN_AES_GPU_LIB"] = AUDIT_LIB
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "audit-child"], capture_output=True, text=True,
                         timeout=240, env=env)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "frames ok" in res.stdout and "address audit" not in res.stderr


def _audit_child():
    import fpnn_amd
    from pyoracle import Oracle
    assert os.environ.get("FPNN_AES_GPU_LIB", "").endswith("libfpnn_aes_gpu_audit.so")
    eng = fpnn_amd.Engine(0)
    oracle = Oracle("port")
    for encrypt in (True, False):
        run_edge_shapes(eng, oracle, encrypt, 16, True, False, stream_counts=(3, 70))
    run_edge_shapes(eng, oracle, True, 32, False, True, stream_counts=(70,))
    eng.sync()
    eng.close()
    print("frames ok")


if __name__ == "__main__":
    if sys.argv[1:] == ["audit-child"]:
        _audit_child()
