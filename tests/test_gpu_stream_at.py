"""One frame per stream by key-table slot (include/fpnn_aes.h: fpnn_aes_stream_encrypt_at /
_decrypt_at; k_stream_at.hip: the slot forms of K2, K2c and K2h).

Segment i of a call is the one pending frame of the connection in slot state_slot[i]: key and
(iv, pos) both live at that slot.  Expected bytes and states come from the oracle alone
(oracle/aes_oracle.c through pyoracle): one StreamEncryptor restatement per connection -- the
oracle's stream_batch on the state of the named slots, or StreamOracle call by call.  Everything
is bit-exact: the whole output buffer (a fill pattern outside the segments) and the WHOLE state
arrays (a fill pattern at every entry a call does not name, guard entries past the bound
included) are compared.  Every case names the kernel it means to reach and checks it through
fpnn_aes_engine_last_kernel, runs AES-128 and AES-256, and uses permuted slots inside a
slot_bound larger than the stream count.

Run as a script (`python tests/test_gpu_stream_at.py audit-child`) the module runs the small
cases of every kernel form and prints "stream_at ok": the way to run them under the address-audit
build of the GPU library (FPNN_AES_GPU_LIB, as tests/test_gpu_audit.py loads it).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from test_gpu_parity import keyset, to_dev, to_host  # noqa: E402

pytestmark = pytest.mark.gpu

PATTERN = 0xA5
K2, K2C, K2H = "cfb_encrypt_chains_at", "cfb_encrypt_coop_at", "cfb_encrypt_hybrid_at"
K1R = "cfb_decrypt_ragged"
GUARD = 8  # state entries past the bound that nothing may touch


def i32(a):
    return to_dev(np.asarray(a).astype(np.int32))


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def ragged(rng, lens):
    """Segments at increasing offsets with random gaps (unaligned starts) -> (offs, total)."""
    lens = np.asarray(lens, dtype=np.int64)
    gaps = rng.integers(0, 24, len(lens))
    offs = np.concatenate([[0], np.cumsum(lens[:-1] + gaps[:-1])]).astype(np.int64) + 3
    return offs, int(offs[-1] + lens[-1]) + 64


class Table:
    """T slots, every slot its own key and IV; the state of every slot on the host (what the
    oracle carries) and in device arrays of `bound + GUARD` entries (bound <= T).  Before
    anything names them the entries hold a random pattern with pos covering 0..15."""

    def __init__(self, engine, oracle, rng, T, keylen, bound=None):
        self.engine, self.oracle, self.rng, self.T, self.keylen = engine, oracle, rng, T, keylen
        self.bound = T if bound is None else bound
        self.keys = rng.integers(0, 256, T * keylen, dtype=np.uint8)
        self.ivs = rng.integers(0, 256, T * 16, dtype=np.uint8)
        self.ks = keyset(engine, self.keys, keylen, self.ivs)
        n = self.bound + GUARD
        self.iv_h = rng.integers(0, 256, n * 16, dtype=np.uint8)
        self.pos_h = (np.arange(n) % 16).astype(np.uint32)
        rng.shuffle(self.pos_h)
        self.upload()

    def upload(self):
        self.iv_d, self.pos_d = to_dev(self.iv_h), to_dev(self.pos_h.astype(np.int32))

    def pair(self):
        """A second state pair (the receive side) holding what this one holds now."""
        other = object.__new__(Table)
        other.__dict__.update(self.__dict__)
        other.iv_h, other.pos_h = self.iv_h.copy(), self.pos_h.copy()
        other.upload()
        return other

    def check_state(self, what):
        iv, pos = to_host(self.iv_d), to_host(self.pos_d).astype(np.uint32)
        bad = np.nonzero((iv.reshape(-1, 16) != self.iv_h.reshape(-1, 16)).any(axis=1) | (pos != self.pos_h))[0]
        assert len(bad) == 0, (what, "state entries", len(bad), bad[:8])

    def expect(self, encrypt, inp, exp, offs, out_offs, lens, slots):
        """The oracle's StreamEncryptor calls, one per named slot, on the host state."""
        slots = np.asarray(slots, dtype=np.int64)
        assert len(np.unique(slots)) == len(slots)
        iv_c = np.ascontiguousarray(self.iv_h.reshape(-1, 16)[slots]).reshape(-1)
        pos_c = np.ascontiguousarray(self.pos_h[slots])
        self.oracle.stream_batch(encrypt, inp, exp, len(slots), in_off=np.asarray(offs).astype(np.uint64),
                                 out_off=np.asarray(out_offs).astype(np.uint64),
                                 lens=np.asarray(lens).astype(np.uint32), key_slot=slots.astype(np.uint32),
                                 keys=self.keys, keylen=self.keylen, iv_state=iv_c, pos_state=pos_c, threads=8)
        self.iv_h.reshape(-1, 16)[slots] = iv_c.reshape(-1, 16)
        self.pos_h[slots] = pos_c

    def cycle(self, encrypt, slots, lens, what, kernel, *, inplace=False, uniform=None, data=None, offs=None,
              bad=(), max_len=0, sync=True):
        """One fpnn_aes_stream_encrypt_at / _decrypt_at call against the oracle.  lens: per
        segment, or with uniform=(len, stride) a strided batch without descriptor arrays.
        data, offs: the payload and where its segments lie (default: random, at random gaps).
        bad: segment indices whose slot is expected to be refused (their bytes and every state
        stay as they are).  -> (input, (device output, expected output), offs)"""
        import fpnn_amd
        slots = np.asarray(slots)
        n = len(slots)
        if uniform is not None:
            ulen, stride = uniform
            lens = np.full(n, ulen, dtype=np.int64)
            offs, total = np.arange(n, dtype=np.int64) * stride, n * stride + 64
        elif offs is not None:
            total = len(data)
        else:
            offs, total = ragged(self.rng, lens)
        inp = self.rng.integers(0, 256, total, dtype=np.uint8) if data is None else data
        out_offs = offs if (inplace or uniform is not None) else offs + 5
        exp = inp.copy() if inplace else np.full(total + 8, PATTERN, dtype=np.uint8)
        good = np.setdiff1d(np.arange(n), np.asarray(bad, dtype=np.int64))
        self.expect(encrypt, inp, exp, offs[good], out_offs[good], np.asarray(lens)[good], slots[good])
        src = to_dev(inp)
        dst = src if inplace else to_dev(np.full(total + 8, PATTERN, dtype=np.uint8))
        if uniform is not None:
            kw = dict(stride=uniform[1], uniform_len=uniform[0])
        else:
            kw = dict(in_off=to_dev(offs), lens=to_dev(np.asarray(lens).astype(np.int32)))
            if not inplace:
                kw["out_off"] = to_dev(out_offs)
        if max_len:
            kw["max_len"] = max_len
        fn = self.engine.stream_encrypt_at if encrypt else self.engine.stream_decrypt_at
        fn(src, dst, n, self.ks, self.iv_d, self.pos_d, i32(slots), self.bound, **kw)
        which = fpnn_amd.K_ENCRYPT if encrypt else fpnn_amd.K_DECRYPT
        assert self.engine.last_kernel(which) == kernel, (what, self.engine.last_kernel(which))
        if sync:
            self.engine.sync()
            self.verify(dst, exp, what)
        return inp, (dst, exp), offs

    def verify(self, dst, exp, what):
        got = to_host(dst)
        bad = np.nonzero(got != exp)[0]
        assert len(bad) == 0, (what, "bytes", len(bad), bad[:8])
        self.check_state(what)


K2C_LENS = [0, 1, 15, 16, 17, 129, 1000]


def k2c_slots(rng, bound):
    """7 distinct slots in [0, bound) in random order, 0 and bound - 1 among them."""
    s = np.concatenate([[0, bound - 1], 1 + rng.permutation(bound - 2)[:5]])
    return s[rng.permutation(7)]


# ---------------------------------------------------------------------------------------
# 1. K2c form

@pytest.mark.parametrize("inplace", [False, True], ids=["outofplace", "inplace"])
@pytest.mark.parametrize("keylen", [16, 32])
def test_k2c_form(engine, oracle, keylen, inplace):
    """7 streams of 0, 1, 15, 16, 17, 129 and 1000 bytes on permuted slots of a 41-slot table;
    the incoming positions of the 16 rounds cover 0..15 for every length."""
    rng = np.random.default_rng(1000 + keylen + inplace)
    tab = Table(engine, oracle, rng, 41, keylen)
    try:
        for r in range(16):
            slots = k2c_slots(rng, 41)
            tab.pos_h[slots] = (np.arange(7) + r) % 16
            tab.upload()
            tab.cycle(True, slots, K2C_LENS, f"round {r}", K2C, inplace=inplace)
    finally:
        tab.ks.close()


# ---------------------------------------------------------------------------------------
# 2. K2h form, both sessions

def k2h_lens(rng, n):
    """Uniform random 0-300 B, 40 streams of 8-12 KiB (>= 512 blocks: the quad queue), and
    streams at fixed places whose pos + len < 16 (set by the caller: no block boundary)."""
    lens = rng.integers(0, 301, n)
    big = rng.permutation(n)[:40]
    lens[big] = rng.integers(8 << 10, (12 << 10) + 1, 40)
    return lens, big


@pytest.mark.parametrize("keylen", [16, 32])
def test_k2h_form(hybrid_engine, oracle, keylen):
    """CUs x 256 + 1000 streams -- more chains than the grid has quads -- on an engine whose
    quad queue takes chains of 64 blocks and more: the 40 long streams run in the quad session,
    the rest in the lane session; every byte and every state."""
    rng = np.random.default_rng(2000 + keylen)
    n = cu_count() * 256 + 1000
    T = n + 777
    tab = Table(hybrid_engine, oracle, rng, T, keylen)
    try:
        slots = rng.permutation(T)[:n]
        lens, big = k2h_lens(rng, n)
        short = np.setdiff1d(np.arange(n), big)[:6]  # pos + len < 16
        tab.pos_h[slots[short]] = [0, 1, 5, 9, 14, 3]
        lens[short] = [15, 14, 10, 6, 1, 0]
        tab.upload()
        tab.cycle(True, slots, lens, "k2h", K2H)
        # and again on the carried state, in place, other slots active
        slots2 = rng.permutation(T)[:n]
        lens2, _ = k2h_lens(rng, n)
        tab.cycle(True, slots2, lens2, "k2h second", K2H, inplace=True)
    finally:
        tab.ks.close()


# ---------------------------------------------------------------------------------------
# 3. K2 form

@pytest.mark.parametrize("keylen", [16, 32])
def test_k2_form(engine, oracle, keylen):
    """CUs x 1024 streams (one chain per lane of the chip) of uniform 48 B with per-slot keys,
    then 47 B with max_len set on the carried state."""
    rng = np.random.default_rng(3000 + keylen)
    n = cu_count() * 1024
    T = n + 4099
    tab = Table(engine, oracle, rng, T, keylen)
    try:
        slots = rng.permutation(T)[:n]
        tab.cycle(True, slots, None, "48 B", K2, uniform=(48, 48))
        tab.cycle(True, slots[rng.permutation(n)], None, "47 B", K2, uniform=(47, 48), max_len=47)
    finally:
        tab.ks.close()


# ---------------------------------------------------------------------------------------
# 4. three cycles over one table, and the receive side

@pytest.mark.parametrize("keylen", [16, 32])
def test_three_cycles_and_decrypt(engine, oracle, keylen):
    """Each cycle ciphers a different active subset under a fresh permutation; the state
    carries.  fpnn_aes_stream_decrypt_at on a second state pair recovers every plaintext and
    ends in the oracle's receive state."""
    rng = np.random.default_rng(4000 + keylen)
    T = 600
    send = Table(engine, oracle, rng, T, keylen, bound=520)
    recv = send.pair()
    try:
        for c in range(3):
            n = (300, 77, 411)[c]
            slots = rng.permutation(520)[:n]
            lens = rng.integers(0, 700, n)
            lens[:4] = (0, 1, 16, 2500)
            inp, (dst, exp), offs = send.cycle(True, slots, lens, f"cycle {c}", K2C)
            # the receive pair: the ciphertext where the encrypt wrote it (offs + 5), in place
            _, (back, _), _ = recv.cycle(False, slots, lens, f"decrypt {c}", K1R, inplace=True, data=to_host(dst),
                                         offs=offs + 5)
            plain = to_host(back)
            for i in range(n):
                assert np.array_equal(plain[offs[i] + 5:offs[i] + 5 + lens[i]], inp[offs[i]:offs[i] + lens[i]]), (c, i)
            assert np.array_equal(recv.iv_h, send.iv_h) and np.array_equal(recv.pos_h, send.pos_h)
    finally:
        send.ks.close()


# ---------------------------------------------------------------------------------------
# 5. the whole life of a connection on the device

@pytest.mark.parametrize("keylen", [16, 32])
def test_whole_life(engine, oracle, keylen):
    """fpnn_aes_keyset_set_keys -> fpnn_aes_stream_open with an ok[] that refuses two entries ->
    two encrypt_at cycles -> fpnn_aes_keyset_clear + fpnn_aes_stream_close.  The bytes are
    StreamEncryptor(key_i, iv_i) called twice; refused entries keep their fill, closed ones
    are all zero, and a cleared slot holds what a never-set slot holds."""
    import fpnn_amd
    from pyoracle import StreamOracle
    rng = np.random.default_rng(5000 + keylen)
    T, n = 96, 40
    ks = fpnn_amd.KeySet.reserve(engine, T, keylen)
    try:
        slots = rng.permutation(T - 1)[:n]  # (slot T - 1 is never set)
        keys = rng.integers(0, 256, (n, keylen), dtype=np.uint8)
        ivs = rng.integers(0, 256, (n, 16), dtype=np.uint8)
        ks.set_keys(to_dev(keys.reshape(-1)), to_dev(ivs.reshape(-1)), slots=i32(slots), slot_bound=T)
        ok = np.ones(n, np.uint8)
        ok[[3, 17]] = 0
        iv_d = torch.full((16 * (T + GUARD),), 0xC3, dtype=torch.uint8, device="cuda:0")
        pos_d = torch.full((T + GUARD,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
        ks.stream_open(iv_d, pos_d, slots=i32(slots), slot_bound=T, ok=to_dev(ok))
        live = np.nonzero(ok)[0]
        enc = {int(i): StreamOracle(oracle, keys[i].tobytes(), ivs[i].tobytes()) for i in live}
        for c in range(2):
            act = live[rng.permutation(len(live))][:30 + c]
            lens = rng.integers(0, 400, len(act))
            lens[:3] = (0, 7, 33)
            offs, total = ragged(rng, lens)
            inp = rng.integers(0, 256, total, dtype=np.uint8)
            exp = np.full(total, PATTERN, np.uint8)
            for j, i in enumerate(act):
                o, L = int(offs[j]), int(lens[j])
                exp[o:o + L] = np.frombuffer(enc[int(i)].crypt(True, inp[o:o + L].tobytes()), np.uint8)
            dst = to_dev(np.full(total, PATTERN, np.uint8))
            engine.stream_encrypt_at(to_dev(inp), dst, len(act), ks, iv_d, pos_d, i32(slots[act]), T,
                                     in_off=to_dev(offs), lens=to_dev(lens.astype(np.int32)))
            assert engine.last_kernel(fpnn_amd.K_ENCRYPT) == K2C
            engine.sync()
            assert np.array_equal(to_host(dst), exp), c
        exp_iv = np.full((T + GUARD, 16), 0xC3, np.uint8)
        exp_pos = np.full(T + GUARD, 0x5A5A5A5A, np.uint32)
        for i in live:
            exp_iv[slots[i]] = np.frombuffer(enc[int(i)].iv, np.uint8)
            exp_pos[slots[i]] = enc[int(i)].pos
        assert np.array_equal(to_host(iv_d).reshape(-1, 16), exp_iv), "state after two cycles"
        assert np.array_equal(to_host(pos_d).astype(np.uint32), exp_pos)
        gone = slots[live[::2]]
        ks.clear(slots=i32(gone), slot_bound=T)
        ks.stream_close(iv_d, pos_d, slots=i32(gone), slot_bound=T)
        engine.sync()
        exp_iv[gone], exp_pos[gone] = 0, 0
        assert np.array_equal(to_host(iv_d).reshape(-1, 16), exp_iv), "state after close"
        assert np.array_equal(to_host(pos_d).astype(np.uint32), exp_pos)
        assert (exp_iv[slots[[3, 17]]] == 0xC3).all()  # the refused entries were never touched
        never = bytes(ks.schedule(T - 1))
        assert all(bytes(ks.schedule(int(s))) == never for s in gone[:4])
    finally:
        ks.close()


# ---------------------------------------------------------------------------------------
# 6. a slot at the bound

def _bad_slot_case(form, rng):
    """(stream count, lens or None, uniform, kernel, indices of the streams that name the bound)"""
    if form == "k2c":
        return 7, np.array(K2C_LENS)[rng.permutation(7)], None, K2C, [4]
    if form == "k2":
        n = cu_count() * 1024
        return n, None, (48, 48), K2, [n // 3]
    n = cu_count() * 256 + 1000
    lens, big = k2h_lens(rng, n)
    small = int(np.setdiff1d(np.arange(n), big)[100])
    lens[small] = 200
    return n, lens, None, K2H, [int(big[7]), small]  # one in the quad session, one in the lane session


@pytest.mark.parametrize("form", ["k2c", "k2h", "k2"])
@pytest.mark.parametrize("keylen", [16, 32])
def test_slot_at_the_bound(request, oracle, keylen, form):
    """A stream names slot_bound itself (inside the table and inside the arrays' guard
    entries: the documented refusal, no out-of-range access either way).  Its output bytes and
    every state entry keep their fill, every other stream is exact, the next sync reports
    FPNN_AES_ERR_DEVICE once, and the call after that is exact."""
    import fpnn_amd
    eng = request.getfixturevalue("hybrid_engine" if form == "k2h" else "engine")
    rng = np.random.default_rng(6000 + keylen + len(form))
    n, lens, uniform, kernel, bad = _bad_slot_case(form, rng)
    bound = n + 333
    tab = Table(eng, oracle, rng, bound + 16, keylen, bound=bound)
    try:
        eng.sync()
        slots = rng.permutation(bound)[:n]
        slots[bad] = bound
        _, (dst, exp), _ = tab.cycle(True, slots, lens, form, kernel, uniform=uniform, bad=bad, sync=False,
                                     inplace=uniform is not None)
        with pytest.raises(fpnn_amd.FpnnAesError) as ei:
            eng.sync()
        assert ei.value.status == fpnn_amd.ERR_DEVICE and "slot" in str(ei.value)
        eng.sync()  # reported once
        tab.verify(dst, exp, form)
        slots[bad] = np.setdiff1d(np.arange(bound), slots)[:len(bad)]
        tab.cycle(True, slots, lens, form + " after", kernel, uniform=uniform, inplace=uniform is not None)
    finally:
        tab.ks.close()


# ---------------------------------------------------------------------------------------
# 7. argument errors

@pytest.mark.parametrize("encrypt", [True, False], ids=["encrypt", "decrypt"])
def test_argument_errors(engine, oracle, encrypt):
    """What the header says is FPNN_AES_ERR_ARG queues nothing: the state and the output
    keep every bit.  count == 0 is a no-op."""
    import fpnn_amd
    rng = np.random.default_rng(7000 + encrypt)
    tab = Table(engine, oracle, rng, 64, 16)
    try:
        n = 5
        src = to_dev(rng.integers(0, 256, 4096, dtype=np.uint8))
        dst = to_dev(np.full(4096, PATTERN, np.uint8))
        slots = i32(rng.permutation(64)[:n])
        kw = dict(in_off=to_dev(np.arange(n, dtype=np.int64) * 100), lens=i32([0, 1, 16, 17, 90]))
        odd_iv = torch.zeros(16 * 80 + 16, dtype=torch.uint8, device="cuda:0")[1:]
        fn = engine.stream_encrypt_at if encrypt else engine.stream_decrypt_at

        def call(iv=tab.iv_d, pos=tab.pos_d, ss=slots, bound=64, **extra):
            fn(src, dst, n, tab.ks, iv, pos, ss, bound, **dict(kw, **extra))

        bad = [dict(extra=dict(key_slot=slots)),           # a second key addressing
               dict(ss=None),                              # no state_slot
               dict(iv=None), dict(pos=None), dict(iv=odd_iv),
               dict(bound=tab.ks.capacity + 1),            # never grows the table
               dict(extra=dict(flags=fpnn_amd.F_WIRE_PREFIX))]
        for b in bad:
            extra = b.pop("extra", {})
            with pytest.raises(fpnn_amd.FpnnAesError) as ei:
                call(**b, **extra)
            assert ei.value.status == fpnn_amd.ERR_ARG, b
        # a state_slot pointer off the 4-byte grid (through the C-ABI: torch cannot view it)
        d = engine._desc(src, dst, n, tab.ks, **kw)
        cfn = fpnn_amd.lib.fpnn_aes_stream_encrypt_at if encrypt else fpnn_amd.lib.fpnn_aes_stream_decrypt_at
        assert cfn(engine.handle, C.byref(d), C.c_void_p(slots.data_ptr() + 2), 64, C.c_void_p(tab.iv_d.data_ptr()),
                   C.c_void_p(tab.pos_d.data_ptr())) == fpnn_amd.ERR_ARG
        fn(src, dst, 0, tab.ks, None, None, None, 64)  # count == 0
        engine.sync()
        assert (to_host(dst) == PATTERN).all()
        tab.check_state("argument errors")
    finally:
        tab.ks.close()


# ---------------------------------------------------------------------------------------
# 8. graph capture

@pytest.mark.parametrize("n,kernel", [(70000, K2H), (3000, K2C)])
def test_captured_cycle_replays(oracle, n, kernel):
    """After fpnn_aes_engine_reserve a cycle captured on the engine's stream is replayed with
    new lengths, offsets, payloads and slots in the same device arrays (the pattern of
    tests/test_gpu_graph.py); the state carries from replay to replay."""
    import fpnn_amd
    rng = np.random.default_rng(8000 + n)
    side = torch.cuda.Stream()
    eng = fpnn_amd.Engine(0, stream=side)
    try:
        keylen, max_len, T = 32, 600, n + 500
        cap = n * (max_len + 24) + 4096
        tab = Table(eng, oracle, rng, T, keylen)
        eng.reserve(n, cap // 16 + n)
        with torch.cuda.stream(side):
            d_in = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
            d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
            d_off = torch.zeros(n, dtype=torch.int64, device="cuda:0")
            d_len = torch.zeros(n, dtype=torch.int32, device="cuda:0")
            d_slot = torch.zeros(n, dtype=torch.int32, device="cuda:0")
            iv_d, pos_d = tab.iv_d.clone(), tab.pos_d.clone()

        def load(seed):
            r = np.random.default_rng(seed)
            lens = r.integers(0, max_len, n)
            offs, total = ragged(r, lens)
            assert total <= cap
            slots = r.permutation(T)[:n]
            data = r.integers(0, 256, cap, dtype=np.uint8)
            with torch.cuda.stream(side):
                d_off.copy_(torch.from_numpy(offs))
                d_len.copy_(torch.from_numpy(lens.astype(np.int32)))
                d_slot.copy_(torch.from_numpy(slots.astype(np.int32)))
                d_in.copy_(torch.from_numpy(data))
                d_out.zero_()
            exp = np.zeros(cap, dtype=np.uint8)
            tab.expect(True, data, exp, offs, offs, lens, slots)
            return exp

        def run():
            eng.stream_encrypt_at(d_in, d_out, n, tab.ks, iv_d, pos_d, d_slot, T, in_off=d_off, lens=d_len)

        def check(exp, what):
            side.synchronize()
            got = d_out.cpu().numpy()
            assert np.array_equal(got, exp), (what, int(np.count_nonzero(got != exp)))
            assert np.array_equal(iv_d.cpu().numpy(), tab.iv_h), what
            assert np.array_equal(pos_d.cpu().numpy().astype(np.uint32), tab.pos_h), what

        exp = load(1)  # an ordinary call first (code objects loaded, scratch at its final size)
        run()
        assert eng.last_kernel(fpnn_amd.K_ENCRYPT) == kernel
        check(exp, "ordinary")
        g = torch.cuda.CUDAGraph()
        exp = load(2)
        side.synchronize()
        with torch.cuda.graph(g, stream=side, capture_error_mode="relaxed"):
            run()
        for seed in (2, 3):  # capture does not execute: replay once per data set
            if seed != 2:
                exp = load(seed)
            with torch.cuda.stream(side):
                g.replay()
            check(exp, seed)
        eng.sync()
        exp = load(4)
        run()
        check(exp, "after the graph")
        del g
        tab.ks.close()
    finally:
        eng.sync()
        eng.close()


# ---------------------------------------------------------------------------------------
# the small cases of every form in one process (the address-audit run)

def _audit_child():
    import fpnn_amd
    from pyoracle import Oracle
    oracle = Oracle("port")
    rng = np.random.default_rng(99)
    for env, kernel, n in (({}, K2C, 7), ({"FPNN_AES_HYB_FORCE": "1", "FPNN_AES_HYB_LONG": "64", "FPNN_AES_HYB_QW": "3"},
                                           K2H, 3000)):
        os.environ.update(env)
        eng = fpnn_amd.Engine(0)
        for keylen in (16, 32):
            tab = Table(eng, oracle, rng, n + 50, keylen)
            slots = rng.permutation(n + 50)[:n]
            lens = np.array(K2C_LENS) if n == 7 else k2h_lens(rng, n)[0]
            tab.cycle(True, slots, lens, "audit", kernel)
            tab.cycle(True, slots, lens, "audit in place", kernel, inplace=True)
            recv = tab.pair()
            recv.cycle(False, slots, lens, "audit decrypt", K1R)
            tab.ks.close()
        eng.sync()
        eng.close()
    eng = fpnn_amd.Engine(0)
    n = cu_count() * 1024
    tab = Table(eng, oracle, rng, n + 50, 32)
    tab.cycle(True, rng.permutation(n + 50)[:n], None, "audit k2", K2, uniform=(47, 48))
    tab.ks.close()
    eng.sync()
    eng.close()
    print("stream_at ok")


if __name__ == "__main__" and sys.argv[1:] == ["audit-child"]:
    _audit_child()
