"""Stream mode by key-table slot (include/fpnn_aes.h: fpnn_aes_stream_open / _close,
fpnn_aes_stream_encrypt_frames_at / _decrypt_frames_at, fpnn_aes_stream_recv_at;
k_keytable.hip, k_stream_frames.hip).

One index names a connection's key (slot s of the key table) and its state (entry s of the
caller's state arrays).  Expected bytes and states come from the oracle's stream_batch
applied round by round, exactly as in tests/test_gpu_stream_frames.py (whose helpers this
module imports), from the reference's own bytes (tests/golden/stream_cases.json,
framing_cases.json) and from the reference's ECDH outputs (ecdh_cases.json).  Everything is
bit-exact: the whole output buffer (pattern outside the segments) and the WHOLE state arrays
(pattern at every entry a call does not name) are compared.

Run as a script (`python tests/test_gpu_stream_slots.py audit-child`) the module runs one
edge-shape case and prints "slots ok"; the audit test starts it in a fresh process with
FPNN_AES_GPU_LIB naming the address-audit build of the GPU library.
"""
import copy
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from test_gpu_parity import keyset, to_dev, to_host  # noqa: E402
from test_gpu_stream_frames import PATTERN, Streams, oracle_rounds  # noqa: E402

pytestmark = pytest.mark.gpu

AUDIT_LIB = os.path.join(ROOT, "fpnn_amd", "libfpnn_aes_gpu_audit.so")
IV_FILL, POS_FILL = 0xC3, 0x5A5A5A5A  # what state entries hold before anything names them
MAX_FRAMES = 64


def i32(a):
    return to_dev(np.asarray(a).astype(np.int32))


def filled_state(entries):
    """Device state arrays of `entries` slots holding the fill pattern."""
    return (torch.full((16 * entries,), IV_FILL, dtype=torch.uint8, device="cuda:0"),
            torch.full((entries,), POS_FILL, dtype=torch.int32, device="cuda:0"))


def state_of(iv_d, pos_d):
    return to_host(iv_d).reshape(-1, 16), to_host(pos_d).astype(np.uint32)


def live_table(engine, rng, nslots, keylen, written):
    """A reserved table of nslots slots; the slots in `written` get random keys and IVs on
    the device (fpnn_aes_keyset_set_keys), the others are never set.  -> (KeySet, keys, ivs):
    host mirrors [nslots, keylen] / [nslots, 16], zero where never set."""
    import fpnn_amd
    ks = fpnn_amd.KeySet.reserve(engine, nslots, keylen)
    keys = np.zeros((nslots, keylen), np.uint8)
    ivs = np.zeros((nslots, 16), np.uint8)
    written = np.asarray(written)
    keys[written] = rng.integers(0, 256, (len(written), keylen), dtype=np.uint8)
    ivs[written] = rng.integers(0, 256, (len(written), 16), dtype=np.uint8)
    ks.set_keys(to_dev(keys[written].reshape(-1)), to_dev(ivs[written].reshape(-1)), slots=i32(written),
                slot_bound=nslots)
    return ks, keys, ivs


# ---------------------------------------------------------------------------------------
# open and close


def addressing(kind, rng):
    """(first, count, slots or None) in a 64-slot table; every kind leaves slots unnamed."""
    if kind == "contiguous":
        return 10, 20, None
    if kind == "permutation":
        p = rng.permutation(64)[:40]
        if 5 not in p:
            p[0] = 5  # (a never-set slot among them)
        return 0, 40, p
    return 0, 19, 3 + 3 * np.arange(19) + (np.arange(19) % 2)  # sparse: holes of 2 / 1 / 3 slots


@pytest.mark.parametrize("kind", ["contiguous", "permutation", "sparse"])
@pytest.mark.parametrize("keylen", [16, 24, 32])
def test_open_and_close(engine, keylen, kind):
    """1. A 64-slot table with slots 5, 12, 27 and 63 never set.  Open: the named entries
    are (IV of the slot, 0) -- all zero for a never-set slot --, every other entry keeps its
    fill pattern.  Close of half of them: exactly zero, the rest as they were."""
    rng = np.random.default_rng(100 * keylen + len(kind))
    never = np.array([5, 12, 27, 63])
    ks, _, ivs = live_table(engine, rng, 64, keylen, np.setdiff1d(np.arange(64), never))
    try:
        first, count, slots = addressing(kind, rng)
        named = first + np.arange(count) if slots is None else slots
        assert np.intersect1d(named, never).size, "the case must open a never-set slot"
        iv_d, pos_d = filled_state(64)
        kw = {} if slots is None else dict(slots=i32(slots), slot_bound=64)
        ks.stream_open(iv_d, pos_d, first, count, **kw)
        engine.sync()
        exp_iv = np.full((64, 16), IV_FILL, np.uint8)
        exp_pos = np.full(64, POS_FILL, np.uint32)
        exp_iv[named], exp_pos[named] = ivs[named], 0
        assert not exp_iv[never[np.isin(never, named)]].any()
        iv, pos = state_of(iv_d, pos_d)
        assert np.array_equal(iv, exp_iv) and np.array_equal(pos, exp_pos), "open"
        # a position other than 0 first, so that close is seen to write it
        pos_d.fill_(7)
        exp_pos[:] = 7
        half = named[::2]
        if slots is None:
            ks.stream_close(iv_d, pos_d, first, (count + 1) // 2)  # (contiguous: the first half)
            half = named[:(count + 1) // 2]
        else:
            ks.stream_close(iv_d, pos_d, slots=i32(half), slot_bound=64)
        engine.sync()
        exp_iv[half], exp_pos[half] = 0, 0
        iv, pos = state_of(iv_d, pos_d)
        assert np.array_equal(iv, exp_iv) and np.array_equal(pos, exp_pos), "close"
    finally:
        ks.close()


def test_open_ok_gating(engine):
    """2. Entries with ok[i] == 0 write nothing."""
    rng = np.random.default_rng(202)
    ks, _, ivs = live_table(engine, rng, 64, 16, np.arange(64))
    try:
        slots = rng.permutation(64)[:48]
        ok = (rng.random(48) < 0.5).astype(np.uint8)
        ok[:2] = (0, 1)
        iv_d, pos_d = filled_state(64)
        ks.stream_open(iv_d, pos_d, slots=i32(slots), slot_bound=64, ok=to_dev(ok))
        engine.sync()
        exp_iv = np.full((64, 16), IV_FILL, np.uint8)
        exp_pos = np.full(64, POS_FILL, np.uint32)
        exp_iv[slots[ok == 1]], exp_pos[slots[ok == 1]] = ivs[slots[ok == 1]], 0
        iv, pos = state_of(iv_d, pos_d)
        assert np.array_equal(iv, exp_iv) and np.array_equal(pos, exp_pos)
    finally:
        ks.close()


@pytest.mark.parametrize("call", ["open", "close"])
def test_open_close_slot_bound(engine, call):
    """3. slot_bound = 32 in a 64-slot table with one entry naming slot 32 itself: that entry
    writes nothing, the others are written, the guard entries past the bound (the arrays hold
    40) keep their fill, the next sync reports FPNN_AES_ERR_DEVICE once."""
    import fpnn_amd
    rng = np.random.default_rng(303)
    ks, _, ivs = live_table(engine, rng, 64, 16, np.arange(64))
    try:
        engine.sync()
        slots = rng.permutation(32)[:20]
        slots[7] = 32
        iv_d, pos_d = filled_state(40)
        if call == "open":
            ks.stream_open(iv_d, pos_d, slots=i32(slots), slot_bound=32)
        else:
            ks.stream_close(iv_d, pos_d, slots=i32(slots), slot_bound=32)
        with pytest.raises(fpnn_amd.FpnnAesError) as ei:
            engine.sync()
        assert ei.value.status == fpnn_amd.ERR_DEVICE and "slot" in str(ei.value)
        engine.sync()  # reported once
        inb = slots[slots < 32]
        assert len(inb) == 19
        exp_iv = np.full((40, 16), IV_FILL, np.uint8)
        exp_pos = np.full(40, POS_FILL, np.uint32)
        exp_iv[inb], exp_pos[inb] = (ivs[inb] if call == "open" else 0), 0
        iv, pos = state_of(iv_d, pos_d)
        assert np.array_equal(iv, exp_iv) and np.array_equal(pos, exp_pos)
    finally:
        ks.close()


def test_open_close_arguments(engine):
    """4. What the header says is FPNN_AES_ERR_ARG, and the call that does nothing."""
    import fpnn_amd
    rng = np.random.default_rng(404)
    ks, _, _ = live_table(engine, rng, 64, 16, np.arange(64))
    try:
        iv_d, pos_d = filled_state(80)
        odd_iv = torch.zeros(16 * 64 + 16, dtype=torch.uint8, device="cuda:0")[1:]
        slots = i32(np.arange(4))
        bad = [dict(iv=None), dict(pos=None), dict(iv=odd_iv),
               dict(first=60, count=5),                    # first + count above the capacity: never grows
               dict(slots=slots, slot_bound=65, count=4)]
        for fn in (ks.stream_open, ks.stream_close):
            for b in bad:
                kw = {k: v for k, v in b.items() if k in ("slots", "slot_bound")}
                with pytest.raises(fpnn_amd.FpnnAesError) as ei:
                    fn(b.get("iv", iv_d), b.get("pos", pos_d), b.get("first", 0), b.get("count", 4), **kw)
                assert ei.value.status == fpnn_amd.ERR_ARG, b
            fn(None, None, 0, 0)  # count == 0
        assert ks.capacity == 64
        engine.sync()
        iv, pos = state_of(iv_d, pos_d)
        assert (iv == IV_FILL).all() and (pos == POS_FILL).all()
    finally:
        ks.close()


# ---------------------------------------------------------------------------------------
# the slot-addressed frame calls


class SlotTable:
    """A key table of T slots (every slot its own key) with the carried state of every slot
    on the host (the oracle's) and on the device; the device arrays hold `guard` further
    entries past the table that nothing may touch."""

    def __init__(self, engine, oracle, rng, T, keylen, guard=0):
        self.engine, self.oracle, self.rng, self.T, self.keylen = engine, oracle, rng, T, keylen
        self.keys = rng.integers(0, 256, T * keylen, dtype=np.uint8)
        self.ks = keyset(engine, self.keys, keylen, rng.integers(0, 256, T * 16, dtype=np.uint8))
        # (host mirrors of the device arrays: random state everywhere, guards included)
        self.iv_h = rng.integers(0, 256, (T + guard) * 16, dtype=np.uint8)
        self.pos_h = rng.integers(0, 16, T + guard).astype(np.uint32)
        self.upload_state()

    def upload_state(self):
        self.iv_d, self.pos_d = to_dev(self.iv_h), to_dev(self.pos_h.astype(np.int32))

    def check_state(self, what):
        assert np.array_equal(to_host(self.iv_d), self.iv_h), what
        assert np.array_equal(to_host(self.pos_d).astype(np.uint32), self.pos_h), what

    def expect(self, encrypt, st, slots, inp, exp, out_offs):
        """The oracle's rounds on the state of `slots`; the host state advances."""
        slots = np.asarray(slots)
        iv_c = np.ascontiguousarray(self.iv_h.reshape(-1, 16)[slots]).reshape(-1)
        pos_c = np.ascontiguousarray(self.pos_h[slots])
        oracle_rounds(self.oracle, encrypt, st, inp, exp, out_offs, slots, self.keys, self.keylen, iv_c, pos_c)
        self.iv_h.reshape(-1, 16)[slots] = iv_c.reshape(-1, 16)
        self.pos_h[slots] = pos_c

    def at_call(self, encrypt, slots, frame_lens, inplace, what, bound=None, dense=False, st=None, data=None):
        """One *_frames_at call against the oracle's rounds -> (Streams, input, output)."""
        st = Streams(self.rng, frame_lens, dense) if st is None else st
        inp = self.rng.integers(0, 256, st.total + 8, dtype=np.uint8) if data is None else data
        out_offs = st.offs if inplace else st.offs + 3
        exp = inp.copy() if inplace else np.full(st.total + 8, PATTERN, dtype=np.uint8)
        self.expect(encrypt, st, slots, inp, exp, out_offs)
        src = to_dev(inp)
        dst = src if inplace else to_dev(np.full(st.total + 8, PATTERN, dtype=np.uint8))
        kw = dict(in_off=to_dev(st.offs), lens=to_dev(st.lens))
        if not inplace:
            kw["out_off"] = to_dev(out_offs)
        fn = self.engine.stream_encrypt_frames_at if encrypt else self.engine.stream_decrypt_frames_at
        fn(src, dst, st.count, self.ks, self.iv_d, self.pos_d, to_dev(st.first), st.S, i32(slots),
           self.T if bound is None else bound, **kw)
        self.engine.sync()
        got = to_host(dst)
        assert np.array_equal(got, exp), (what, int(np.count_nonzero(got != exp)))
        self.check_state(what)
        return st, inp, got


def parity_shape(rng):
    """37 streams on distinct slots of a 257-slot table (0 and 256 among them), 0-5 frames
    of 0-200 bytes each; stream 11 carries a 2 565-byte frame (more than one 8-block step,
    across K1r's 1 KiB chunks), stream 23 only empty frames, stream 30 no frame."""
    slots = np.concatenate([[0, 256], 1 + rng.permutation(255)[:35]])
    slots = slots[rng.permutation(37)]
    lens = [[int(x) for x in rng.integers(0, 201, int(rng.integers(0, 6)))] for _ in range(37)]
    lens[11] = [40, 2565, 7]
    lens[23] = [0, 0, 0]
    lens[30] = []
    return slots, lens


@pytest.mark.parametrize("inplace", [False, True], ids=["outofplace", "inplace"])
@pytest.mark.parametrize("keylen", [16, 32])
@pytest.mark.parametrize("encrypt", [True, False], ids=["encrypt", "decrypt"])
def test_at_parity(engine, oracle, encrypt, keylen, inplace):
    """5. Bytes, the final state at the named slots, every other state entry and every
    output byte outside the segments; then a second call on other slots and the carried
    state."""
    rng = np.random.default_rng(5000 + keylen + 2 * encrypt + 4 * inplace)
    tab = SlotTable(engine, oracle, rng, 257, keylen)
    try:
        slots, lens = parity_shape(rng)
        before_iv, before_pos = tab.iv_h.copy(), tab.pos_h.copy()
        tab.at_call(encrypt, slots, lens, inplace, "first")
        rest = np.setdiff1d(np.arange(257), slots)
        assert np.array_equal(tab.iv_h.reshape(-1, 16)[rest], before_iv.reshape(-1, 16)[rest])
        assert np.array_equal(tab.pos_h[rest], before_pos[rest])
        assert not np.array_equal(tab.iv_h, before_iv)
        slots2, lens2 = parity_shape(rng)
        tab.at_call(encrypt, slots2, lens2, inplace, "second")
    finally:
        tab.ks.close()


@pytest.mark.parametrize("encrypt", [True, False], ids=["encrypt", "decrypt"])
def test_identity_slots_equal_the_frames_call(engine, oracle, encrypt):
    """6. state_slot = arange over a table whose slot j is stream j's key: the bytes and the
    state of fpnn_aes_stream_*_frames."""
    rng = np.random.default_rng(600 + encrypt)
    S = 37
    tab = SlotTable(engine, oracle, rng, S, 16)
    try:
        _, lens = parity_shape(rng)
        st = Streams(rng, lens)
        inp = rng.integers(0, 256, st.total + 8, dtype=np.uint8)
        iv2, pos2 = tab.iv_d.clone(), tab.pos_d.clone()
        dst = to_dev(np.full(st.total + 8, PATTERN, dtype=np.uint8))
        kw = dict(in_off=to_dev(st.offs), lens=to_dev(st.lens), out_off=to_dev(st.offs + 3))
        fn = engine.stream_encrypt_frames if encrypt else engine.stream_decrypt_frames
        fn(to_dev(inp), dst, st.count, tab.ks, iv2, pos2, to_dev(st.first), S, key_slot=i32(st.stream_of), **kw)
        engine.sync()
        _, _, got = tab.at_call(encrypt, np.arange(S), None, False, "identity", st=st, data=inp)
        assert np.array_equal(got, to_host(dst))
        assert torch.equal(iv2, tab.iv_d) and torch.equal(pos2, tab.pos_d)
    finally:
        tab.ks.close()


def test_large_count_on_permuted_slots(engine, oracle):
    """7. 70 000 streams x one 20-byte frame, slots a random permutation: more streams than
    the quads of a full grid (K2f's grid stride) and more than 16 384 segments (the one-pass
    block map); encrypt, then decrypt from the same incoming state."""
    rng = np.random.default_rng(70000)
    S = 70000
    tab = SlotTable(engine, oracle, rng, S, 16)
    try:
        slots = rng.permutation(S)
        iv0, pos0 = tab.iv_h.copy(), tab.pos_h.copy()
        st, plain, cipher = tab.at_call(True, slots, [[20]] * S, True, "encrypt", dense=True)
        iv1, pos1 = tab.iv_h.copy(), tab.pos_h.copy()
        tab.iv_h, tab.pos_h = iv0, pos0
        tab.upload_state()
        _, _, back = tab.at_call(False, slots, None, True, "decrypt", st=st, data=cipher)
        assert np.array_equal(back, plain)
        assert np.array_equal(tab.iv_h, iv1) and np.array_equal(tab.pos_h, pos1)
    finally:
        tab.ks.close()


@pytest.mark.parametrize("encrypt", [True, False], ids=["encrypt", "decrypt"])
def test_bad_slot_is_reported_and_stays_in_bounds(engine, oracle, encrypt):
    """8. slot_bound = 40 in a 64-slot table whose state arrays hold 48 entries; stream 2
    names slot 43 (inside the arrays' guard entries, whatever a kernel does).  Its state is
    neither read nor written -- the guards keep their bytes --, encrypt writes nothing for
    it, decrypt only inside its own segments; every other stream is exact; the next sync
    reports FPNN_AES_ERR_DEVICE once; the following call is exact."""
    import fpnn_amd
    rng = np.random.default_rng(800 + encrypt)
    tab = SlotTable(engine, oracle, rng, 64, 16, guard=0)
    # (the state arrays: 40 entries the call may name + 8 guard entries = the first 48)
    tab.iv_h, tab.pos_h = tab.iv_h[:16 * 48].copy(), tab.pos_h[:48].copy()
    tab.upload_state()
    try:
        engine.sync()
        lens = [[5, 40, 0], [17], [130, 2, 9, 33], [], [300, 1]]
        slots = np.array([39, 0, 43, 7, 21])
        st = Streams(rng, lens)
        good = copy.copy(st)
        good.counts = st.counts.copy()
        good.counts[2] = 0  # the oracle runs the other streams only
        inp = rng.integers(0, 256, st.total + 8, dtype=np.uint8)
        out_offs = st.offs + 3
        exp = np.full(st.total + 8, PATTERN, dtype=np.uint8)
        # (slot 1 stands in for the bad stream: no other stream names it, the oracle leaves it alone)
        tab.expect(encrypt, good, np.where(slots < 40, slots, 1), inp, exp, out_offs)
        dst = to_dev(np.full(st.total + 8, PATTERN, dtype=np.uint8))
        fn = engine.stream_encrypt_frames_at if encrypt else engine.stream_decrypt_frames_at
        fn(to_dev(inp), dst, st.count, tab.ks, tab.iv_d, tab.pos_d, to_dev(st.first), st.S, i32(slots), 40,
           in_off=to_dev(st.offs), lens=to_dev(st.lens), out_off=to_dev(out_offs))
        with pytest.raises(fpnn_amd.FpnnAesError) as ei:
            engine.sync()
        assert ei.value.status == fpnn_amd.ERR_DEVICE and "slot" in str(ei.value)
        engine.sync()  # reported once
        got = to_host(dst)
        own = np.zeros(st.total + 8, dtype=bool)  # the bad stream's own output bytes
        for k in range(int(st.first[2]), int(st.first[3])):
            own[out_offs[k]:out_offs[k] + st.lens[k]] = True
        if encrypt:
            assert np.array_equal(got, exp)  # (exp holds the pattern there: nothing written)
        else:
            assert np.array_equal(got[~own], exp[~own])
        tab.check_state("bad slot")  # every entry, guards included
        tab.at_call(encrypt, np.array([39, 0, 12, 7, 21]), lens, False, "after the bad slot", bound=40)
    finally:
        tab.ks.close()


def test_frames_at_arguments(engine, oracle):
    """9. FPNN_AES_ERR_ARG: a key_slot, no state_slot, a bound above the table, NULL or
    misaligned state; and the calls that queue nothing."""
    import fpnn_amd
    rng = np.random.default_rng(900)
    tab = SlotTable(engine, oracle, rng, 16, 16)
    try:
        st = Streams(rng, [[5, 40], [17], [130, 2]])
        inp = rng.integers(0, 256, st.total + 8, dtype=np.uint8)
        src, dst, first, slots = to_dev(inp), to_dev(inp), to_dev(st.first), i32([3, 9, 15])
        kw = dict(in_off=to_dev(st.offs), lens=to_dev(st.lens))
        odd_iv = torch.zeros(16 * 16 + 16, dtype=torch.uint8, device="cuda:0")[1:]
        for fn in (engine.stream_encrypt_frames_at, engine.stream_decrypt_frames_at):
            for args, extra in (((tab.iv_d, tab.pos_d, first, st.S, slots, 16), {"key_slot": i32(st.stream_of)}),
                                ((tab.iv_d, tab.pos_d, first, st.S, None, 16), {}),
                                ((tab.iv_d, tab.pos_d, first, st.S, slots, 17), {}),
                                ((tab.iv_d, tab.pos_d, None, st.S, slots, 16), {}),
                                ((None, tab.pos_d, first, st.S, slots, 16), {}),
                                ((tab.iv_d, None, first, st.S, slots, 16), {}),
                                ((odd_iv, tab.pos_d, first, st.S, slots, 16), {}),
                                ((tab.iv_d, tab.pos_d, first, st.S, slots, 16), {"flags": fpnn_amd.F_WIRE_PREFIX})):
                with pytest.raises(fpnn_amd.FpnnAesError) as ei:
                    fn(src, dst, st.count, tab.ks, *args, **kw, **extra)
                assert ei.value.status == fpnn_amd.ERR_ARG, args[2:]
            fn(src, dst, st.count, tab.ks, None, None, None, 0, None, 16, **kw)  # no stream
            fn(src, dst, 0, tab.ks, tab.iv_d, tab.pos_d, first, st.S, slots, 16, **kw)  # no segment
        lib = fpnn_amd.lib
        d = engine._desc(src, dst, st.count, tab.ks, **kw)
        off, ln, scan = engine._scan_buffers(st.count, 4, src.device)
        assert lib.fpnn_aes_stream_recv_at(engine.handle, C.byref(d), None, 16, tab.iv_d.data_ptr(),
                                           tab.pos_d.data_ptr(), None, 4096, 4, off.data_ptr(), ln.data_ptr(),
                                           scan.data_ptr()) == fpnn_amd.ERR_ARG
        engine.sync()
        assert np.array_equal(to_host(dst), inp)
        tab.check_state("nothing queued")
    finally:
        tab.ks.close()


# ---------------------------------------------------------------------------------------
# receive


def test_recv_at_matches_reference_receiver(engine, oracle, scan_mode):
    """10. The stream cases of tests/golden/framing_cases.json, each on its own slot of a
    permuted, larger table: frames, verdicts, consumed bytes, plaintext and the final state
    as test_gpu_framing_golden.py checks them for stream_recv; unnamed state entries keep
    their fill."""
    import fpnn_amd
    from framing_golden import expected, load_cases
    cases_all = [c for c in load_cases() if c["mode"] == "stream"]
    key = lambda c: (c["max_len"], len(c["key"]) // 2)  # noqa: E731
    rng = np.random.default_rng(1000)
    for (max_len, keylen), grp in itertools.groupby(sorted(cases_all, key=key), key=key):
        cases = list(grp)
        n, T = len(cases), len(cases) + 9
        slot_of = rng.permutation(T)[:n]
        keys = rng.integers(0, 256, (T, keylen), dtype=np.uint8)
        keys[slot_of] = [np.frombuffer(bytes.fromhex(c["key"]), np.uint8) for c in cases]
        ks = fpnn_amd.KeySet(engine, keys.tobytes(), keylen, bytes(16 * T))
        iv_d, pos_d = filled_state(T)
        iv_h = to_host(iv_d).reshape(T, 16).copy()
        iv_h[slot_of] = [np.frombuffer(bytes.fromhex(c["iv"]), np.uint8) for c in cases]
        iv_d.copy_(torch.from_numpy(iv_h.reshape(-1)))
        pos_d[torch.from_numpy(slot_of).to("cuda:0")] = 0
        wires = [bytes.fromhex(c["wire"]) for c in cases]
        offs = np.concatenate([[0], np.cumsum([len(w) + 5 for w in wires[:-1]])]).astype(np.int64)
        host = np.zeros(int(offs[-1]) + len(wires[-1]) + 16, dtype=np.uint8)
        for o, w in zip(offs, wires):
            host[o:o + len(w)] = np.frombuffer(w, np.uint8)
        inp = to_dev(host)
        out = torch.zeros_like(inp)
        foff, flen, scan = engine.stream_recv_at(inp, out, n, ks, iv_d, pos_d, i32(slot_of), T, max_len, MAX_FRAMES,
                                                 in_off=to_dev(offs), lens=i32([len(w) for w in wires]))
        engine.sync()
        frames, status, consumed = fpnn_amd.Engine.decode_scan(scan)
        foff, flen, res = to_host(foff), to_host(flen), to_host(out)
        iv, pos = state_of(iv_d, pos_d)
        for i, c in enumerate(cases):
            ef, es, ec, raws = expected(c)
            assert (frames[i], status[i], consumed[i]) == (len(ef), es, ec), c["name"]
            for j, ((o, ln), raw) in enumerate(zip(ef, raws)):
                assert (foff[i * MAX_FRAMES + j], flen[i * MAX_FRAMES + j]) == (o, ln), (c["name"], j)
                if raw is not None:
                    assert res[offs[i] + o:offs[i] + o + ln].tobytes() == raw, (c["name"], j)
            _, iv_end, pos_end = oracle.cfb(bytes.fromhex(c["key"]), False, wires[i], bytes.fromhex(c["iv"]), 0)
            assert (iv[slot_of[i]].tobytes(), int(pos[slot_of[i]])) == (iv_end, pos_end), c["name"]
        rest = np.setdiff1d(np.arange(T), slot_of)
        assert (iv[rest] == IV_FILL).all() and (pos[rest] == POS_FILL).all()
        ks.close()


# ---------------------------------------------------------------------------------------
# the lifecycle on reference data


@pytest.mark.parametrize("keylen", [16, 32])
def test_reference_sequences_from_open_to_close(engine, keylen, golden):
    """11. tests/golden/stream_cases.json: keys and IVs into sparse slots (set_keys), state
    by stream_open, all 12 frames of every sequence in one _at encrypt call against the
    reference's own bytes, back through a second state pair, then stream_close and
    keyset_clear: state and key slots all zero."""
    import fpnn_amd
    cs = [c for c in golden("stream_cases.json") if len(c["key"]) // 2 == keylen]
    assert cs
    rng = np.random.default_rng(1100 + keylen)
    T = 40
    slots = np.array([31, 4, 17, 38])[:len(cs)]
    ks = fpnn_amd.KeySet.reserve(engine, T, keylen)
    try:
        keys = np.frombuffer(b"".join(bytes.fromhex(c["key"]) for c in cs), np.uint8)
        ivs = np.frombuffer(b"".join(bytes.fromhex(c["iv"]) for c in cs), np.uint8)
        ks.set_keys(to_dev(keys), to_dev(ivs), slots=i32(slots), slot_bound=T)
        send, recv = filled_state(T), filled_state(T)
        for iv_d, pos_d in (send, recv):
            ks.stream_open(iv_d, pos_d, slots=i32(slots), slot_bound=T)
        # plaintext and ciphertext of every frame (a recorded decrypt sequence holds them the other way round)
        plain = [[bytes.fromhex(f["in" if c["encrypt"] else "out"]) for f in c["frames"]] for c in cs]
        ciph = [[bytes.fromhex(f["out" if c["encrypt"] else "in"]) for f in c["frames"]] for c in cs]
        assert all(len(p) == 12 for p in plain)
        st = Streams(rng, [[len(f) for f in fr] for fr in plain])
        inp = np.full(st.total + 8, 0x11, dtype=np.uint8)
        exp = np.full(st.total + 8, PATTERN, dtype=np.uint8)
        back_exp = np.full(st.total + 8, PATTERN, dtype=np.uint8)
        k = 0
        for pf, cf in zip(plain, ciph):
            for p, c in zip(pf, cf):
                o = int(st.offs[k])
                inp[o:o + len(p)] = np.frombuffer(p, np.uint8)
                back_exp[o:o + len(p)] = np.frombuffer(p, np.uint8)
                exp[o:o + len(c)] = np.frombuffer(c, np.uint8)
                k += 1
        mid = to_dev(np.full(st.total + 8, PATTERN, dtype=np.uint8))
        back = to_dev(np.full(st.total + 8, PATTERN, dtype=np.uint8))
        kw = dict(in_off=to_dev(st.offs), lens=to_dev(st.lens))
        engine.stream_encrypt_frames_at(to_dev(inp), mid, st.count, ks, send[0], send[1], to_dev(st.first), st.S,
                                        i32(slots), T, **kw)
        engine.stream_decrypt_frames_at(mid, back, st.count, ks, recv[0], recv[1], to_dev(st.first), st.S,
                                        i32(slots), T, **kw)
        engine.sync()
        assert np.array_equal(to_host(mid), exp), "the reference's ciphertext"
        assert np.array_equal(to_host(back), back_exp), "and back"
        # the state the reference's StreamEncryptor is left with, in both pairs; fill elsewhere
        rest = np.setdiff1d(np.arange(T), slots)
        for iv_d, pos_d in (send, recv):
            iv, pos = state_of(iv_d, pos_d)
            for j, (c, pf) in enumerate(zip(cs, plain)):
                se = fpnn_amd.StreamEncryptor(engine, bytes.fromhex(c["key"]), bytes.fromhex(c["iv"]))
                for p in pf:
                    se.encrypt(p)
                assert (iv[slots[j]].tobytes(), int(pos[slots[j]])) == se.state, j
            assert (iv[rest] == IV_FILL).all() and (pos[rest] == POS_FILL).all()
        # the connections close
        never = bytes(ks.schedule(int(rest[0])))
        for iv_d, pos_d in (send, recv):
            ks.stream_close(iv_d, pos_d, slots=i32(slots), slot_bound=T)
        ks.clear(slots=i32(slots), slot_bound=T)
        engine.sync()
        for iv_d, pos_d in (send, recv):
            iv, pos = state_of(iv_d, pos_d)
            assert not iv[slots].any() and not pos[slots].any()
            assert (iv[rest] == IV_FILL).all() and (pos[rest] == POS_FILL).all()
        assert not any(never)  # (a never-set slot of a reserved table: a zero DevKey)
        for s in slots:
            assert bytes(ks.schedule(int(s))) == never, int(s)
        # and an open after the clear gives the all-zero state
        ks.stream_open(send[0], send[1], slots=i32(slots), slot_bound=T)
        engine.sync()
        iv, pos = state_of(*send)
        assert not iv[slots].any() and not pos[slots].any()
    finally:
        ks.close()


@pytest.mark.parametrize("curve,keylen", [("secp256k1", 16), ("secp224r1", 32)])
def test_accept_then_open(engine, curve, keylen):
    """12. fpnn_ecdh_accept on fixture rows, then stream_open with the same ok: the state of
    an accepted row is (the fixture's derived IV, 0), a refused row's keeps its fill."""
    import fpnn_amd
    from test_gpu_keytable import accept_rows
    rng = np.random.default_rng(1200 + keylen)
    rows = accept_rows(curve, keylen)
    T = 128
    ks = fpnn_amd.KeySet.reserve(engine, T, keylen)
    try:
        slot_of_row = rng.permutation(T)[:len(rows)]
        groups = {}
        for i, s in enumerate(rows):
            groups.setdefault(s["private"], []).append(i)
        iv_d, pos_d = filled_state(T)
        for priv, idx in groups.items():
            peers = to_dev(np.frombuffer(b"".join(bytes.fromhex(rows[i]["peer"]) for i in idx), np.uint8))
            sl = i32(slot_of_row[idx])
            ok = engine.ecdh_accept(curve, bytes.fromhex(priv), peers, ks, slots=sl, slot_bound=T)
            ks.stream_open(iv_d, pos_d, slots=sl, slot_bound=T, ok=ok, count=len(idx))
        engine.sync()
        exp_iv = np.full((T, 16), IV_FILL, np.uint8)
        exp_pos = np.full(T, POS_FILL, np.uint32)
        assert any(s["ok"] for s in rows) and not all(s["ok"] for s in rows)
        for i, s in enumerate(rows):
            if s["ok"]:
                exp_iv[slot_of_row[i]] = np.frombuffer(bytes.fromhex(s["iv"]), np.uint8)
                exp_pos[slot_of_row[i]] = 0
        iv, pos = state_of(iv_d, pos_d)
        assert np.array_equal(iv, exp_iv) and np.array_equal(pos, exp_pos)
    finally:
        ks.close()


# ---------------------------------------------------------------------------------------


def test_graph_replay(oracle):
    """13. After reserve: stream_open of two state pairs, encrypt_frames_at and
    decrypt_frames_at captured as one linear chain, replayed with other slots, frames and
    data in the same device arrays."""
    import fpnn_amd
    side = torch.cuda.Stream()
    eng = fpnn_amd.Engine(0, stream=side)
    try:
        T, S, nseg, cap, keylen = 500, 120, 1500, 1500 * 70, 32
        rng = np.random.default_rng(1300)
        keys = rng.integers(0, 256, T * keylen, dtype=np.uint8)
        ivs = rng.integers(0, 256, T * 16, dtype=np.uint8)
        ks = keyset(eng, keys, keylen, ivs)
        eng.reserve(nseg, cap // 16 + nseg)
        z = lambda n, dt: torch.zeros(n, dtype=dt, device="cuda:0")  # noqa: E731
        dev = dict(src=z(cap, torch.uint8), mid=z(cap, torch.uint8), back=z(cap, torch.uint8),
                   off=z(nseg, torch.int64), len=z(nseg, torch.int32), first=z(S + 1, torch.int32),
                   slot=z(S, torch.int32), iv_e=z(16 * T, torch.uint8), iv_d=z(16 * T, torch.uint8),
                   pos_e=z(T, torch.int32), pos_d=z(T, torch.int32))

        def load(seed):
            r = np.random.default_rng(seed)
            counts = r.multinomial(nseg, r.dirichlet(np.ones(S)))
            st = Streams(r, [[int(x) for x in r.integers(0, 60, c)] for c in counts], dense=True)
            assert st.count == nseg and st.total + 8 <= cap
            data = r.integers(0, 256, cap, dtype=np.uint8)
            slots = r.permutation(T)[:S]
            with torch.cuda.stream(side):
                for name, a in (("src", data), ("off", st.offs), ("len", st.lens), ("first", st.first),
                                ("slot", slots.astype(np.int32))):
                    dev[name].copy_(torch.from_numpy(np.ascontiguousarray(a)))
                for name in ("mid", "back"):
                    dev[name].fill_(PATTERN)
                for name in ("iv_e", "iv_d"):
                    dev[name].fill_(IV_FILL)
                for name in ("pos_e", "pos_d"):
                    dev[name].fill_(POS_FILL)
            # the state the chain's own stream_open gives the named slots: (IV, 0)
            iv_c = np.ascontiguousarray(ivs.reshape(T, 16)[slots]).reshape(-1)
            pos_c = np.zeros(S, np.uint32)
            exp = np.full(cap, PATTERN, dtype=np.uint8)
            oracle_rounds(oracle, True, st, data, exp, st.offs, slots, keys, keylen, iv_c, pos_c)
            plain = np.where(st.mask(st.offs, cap), data, PATTERN).astype(np.uint8)
            iv_h = np.full((T, 16), IV_FILL, np.uint8)
            pos_h = np.full(T, POS_FILL, np.uint32)
            iv_h[slots], pos_h[slots] = iv_c.reshape(-1, 16), pos_c
            return exp, plain, iv_h, pos_h

        def run():
            kw = dict(in_off=dev["off"], lens=dev["len"])
            for iv, pos in ((dev["iv_e"], dev["pos_e"]), (dev["iv_d"], dev["pos_d"])):
                ks.stream_open(iv, pos, slots=dev["slot"], slot_bound=T, count=S)
            eng.stream_encrypt_frames_at(dev["src"], dev["mid"], nseg, ks, dev["iv_e"], dev["pos_e"], dev["first"], S,
                                         dev["slot"], T, **kw)
            eng.stream_decrypt_frames_at(dev["mid"], dev["back"], nseg, ks, dev["iv_d"], dev["pos_d"], dev["first"], S,
                                         dev["slot"], T, **kw)

        def check(expect, what):
            exp, plain, iv_h, pos_h = expect
            side.synchronize()
            assert np.array_equal(dev["mid"].cpu().numpy(), exp), what
            assert np.array_equal(dev["back"].cpu().numpy(), plain), what
            for iv, pos in ((dev["iv_e"], dev["pos_e"]), (dev["iv_d"], dev["pos_d"])):
                assert np.array_equal(iv.cpu().numpy().reshape(T, 16), iv_h), what
                assert np.array_equal(pos.cpu().numpy().astype(np.uint32), pos_h), what

        expect = load(1)  # an ordinary call first (code objects loaded, scratch at its final size)
        run()
        check(expect, "ordinary")
        load(2)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side, capture_error_mode="relaxed"):
            run()
        expect = load(3)  # capture does not execute: one replay, on new slots and data
        with torch.cuda.stream(side):
            g.replay()
        check(expect, "replay")
        eng.sync()
        del g
    finally:
        eng.sync()
        eng.close()


def test_audit_library():
    """14. The lifecycle and one edge-shape call per direction through the address-audit
    build of the GPU library, in a fresh process: no access outside its extent or its
    segment, and bit-exact."""
    assert os.path.exists(AUDIT_LIB), "make -C fpnn_amd/csrc audit"
    env = dict(os.environ)
    env["FPNN_AES_GPU_LIB"] = AUDIT_LIB
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "audit-child"], capture_output=True, text=True,
                         timeout=240, env=env)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "slots ok" in res.stdout and "address audit" not in res.stderr


def _audit_child():
    import fpnn_amd
    from pyoracle import Oracle
    assert os.environ.get("FPNN_AES_GPU_LIB", "").endswith("libfpnn_aes_gpu_audit.so")
    eng = fpnn_amd.Engine(0)
    oracle = Oracle("port")
    rng = np.random.default_rng(1400)
    for keylen, inplace in ((16, False), (32, True)):
        tab = SlotTable(eng, oracle, rng, 257, keylen)
        slots, lens = parity_shape(rng)
        # open at the table's edge (state (IV, 0) of slots the call names), then both directions
        tab.ks.stream_open(tab.iv_d, tab.pos_d, slots=i32(slots), slot_bound=257)
        tab.ks.stream_close(tab.iv_d, tab.pos_d, 250, 7)
        eng.sync()
        tab.iv_h, tab.pos_h = to_host(tab.iv_d).copy(), to_host(tab.pos_d).astype(np.uint32)
        for encrypt in (True, False):
            tab.at_call(encrypt, slots, lens, inplace, ("audit", keylen, encrypt))
        # one frame per stream, no first_frame: the receive path's decrypt
        n = 9
        sl = rng.permutation(257)[:n]
        lens1 = rng.integers(0, 90, n)
        st = Streams(rng, [[int(x)] for x in lens1])
        inp = rng.integers(0, 256, st.total + 8, dtype=np.uint8)
        exp = inp.copy()
        tab.expect(False, st, sl, inp, exp, st.offs)
        buf = to_dev(inp)
        eng.stream_recv_at(buf, buf, n, tab.ks, tab.iv_d, tab.pos_d, i32(sl), 257, 4096, 4, in_off=to_dev(st.offs),
                           lens=to_dev(st.lens))
        eng.sync()
        assert np.array_equal(to_host(buf), exp)
        tab.check_state("recv_at")
        tab.ks.close()
    eng.sync()
    eng.close()
    print("slots ok")


if __name__ == "__main__":
    if sys.argv[1:] == ["audit-child"]:
        _audit_child()
