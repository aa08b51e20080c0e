"""UDP v2 datagrams with data ("enhanced") encryption in one device call
(include/fpnn_aes.h: fpnn_aes_udp_encrypt / _decrypt; fpnn_amd/csrc/k_udp.hip).

A UDPEncryptor with reinforced data encryption holds two ciphers: a StreamEncryptor under
the data key whose one CFB chain runs through the data sections of the connection's
datagrams, and a PackageEncryptor under the package key that then ciphers every whole
datagram from the connection IV.  Expected bytes are pyoracle's, composed in that order:
oracle.cfb per section (the stream layer, continuing (iv, pos)), then oracle.package per
datagram; decrypt the other way round.  tests/test_oracle.py pins both to the compiled
reference.  Everything is bit-exact: the whole output buffer (a sentinel outside the
datagrams) and the whole state arrays (a fill pattern at every slot no connection names).
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

SENTINEL = 0xA7                        # every byte of a buffer outside the datagrams
IV_FILL, POS_FILL = 0xC3, 0x5A5A5A5A   # state entries no connection names
DGRAM_LENS = (0, 1, 7, 8, 15, 16, 17, 31, 32, 33, 127, 128, 129, 548, 1472)
PAIRS = [(16, 16), (16, 32), (32, 16), (32, 32)]  # (package key length, data key length)


def i32(a):
    return to_dev(np.asarray(a).astype(np.int32))


class Batch:
    """Datagrams of `conns` connections: conns[j] is the list of connection j's datagrams in
    send order, each (length, [(sec_off, sec_len), ...]).  Datagram i lies at offs[i] of the
    buffer, with gaps of 1 - 6 bytes between datagrams unless `offs` is given."""

    def __init__(self, conns, rng, offs=None):
        self.conns = conns
        self.nconn = len(conns)
        self.first_dgram = np.concatenate([[0], np.cumsum([len(c) for c in conns])]).astype(np.int32)
        dgrams = [d for c in conns for d in c]
        self.count = len(dgrams)
        self.lens = np.array([d[0] for d in dgrams], np.int32).reshape(-1)
        self.first_section = np.concatenate([[0], np.cumsum([len(d[1]) for d in dgrams])]).astype(np.int32)
        secs = [s for d in dgrams for s in d[1]]
        self.nsections = len(secs)
        self.sec_off = np.array([s[0] for s in secs], np.int32).reshape(-1)
        self.sec_len = np.array([s[1] for s in secs], np.int32).reshape(-1)
        if offs is None:
            gaps = rng.integers(1, 7, self.count)
            offs = 3 + np.concatenate([[0], np.cumsum(self.lens[:-1].astype(np.int64) + gaps[:-1])]) if self.count \
                else np.zeros(0, np.int64)
        self.offs = np.asarray(offs, np.int64).reshape(-1)
        self.total = int((self.offs + self.lens).max()) + 9 if self.count else 16

    def plaintext(self, rng):
        data = np.full(self.total, SENTINEL, np.uint8)
        for o, n in zip(self.offs, self.lens):
            data[o:o + n] = rng.integers(0, 256, n, dtype=np.uint8)
        return data

    def dev(self):
        z = lambda a: i32(a if len(a) else np.zeros(1, np.int32))  # noqa: E731
        return dict(first_dgram=i32(self.first_dgram), first_section=i32(self.first_section), sec_off=z(self.sec_off),
                    sec_len=z(self.sec_len), in_off=to_dev(self.offs if self.count else np.zeros(1, np.int64)),
                    lens=z(self.lens))


class Tables:
    """A package table and a data table of nslots slots each, with host mirrors."""

    def __init__(self, engine, rng, nslots, pkg_len, data_len):
        self.nslots, self.pkg_len, self.data_len = nslots, pkg_len, data_len
        self.pkeys = rng.integers(0, 256, (nslots, pkg_len), dtype=np.uint8)
        self.pivs = rng.integers(0, 256, (nslots, 16), dtype=np.uint8)
        self.dkeys = rng.integers(0, 256, (nslots, data_len), dtype=np.uint8)
        self.divs = rng.integers(0, 256, (nslots, 16), dtype=np.uint8)
        self.pkg = keyset(engine, self.pkeys.reshape(-1), pkg_len, self.pivs.reshape(-1))
        self.data = keyset(engine, self.dkeys.reshape(-1), data_len, self.divs.reshape(-1))

    def close(self):
        self.pkg.close()
        self.data.close()


def initial_state(rng, entries, slots):
    """State arrays of `entries` slots: the fill pattern, and at the named slots a random iv
    with positions that run through 0 .. 15."""
    iv = np.full((entries, 16), IV_FILL, np.uint8)
    pos = np.full(entries, POS_FILL, np.uint32)
    iv[slots] = rng.integers(0, 256, (len(slots), 16), dtype=np.uint8)
    pos[slots] = np.arange(len(slots)) % 16
    return iv, pos


def reference(oracle, bt, t, slots, data, out0, iv0, pos0, encrypt, skip=()):
    """The reference's bytes and final states: per connection the datagrams in order, per
    datagram the sections in order.  Connections in `skip` are left alone."""
    out, iv, pos = out0.copy(), iv0.copy(), pos0.copy()
    for j, dgrams in enumerate(bt.conns):
        if j in skip:
            continue
        s = int(slots[j])
        pk, piv, dk = t.pkeys[s].tobytes(), t.pivs[s].tobytes(), t.dkeys[s].tobytes()
        civ, cpos, any_byte = iv[s].tobytes(), int(pos[s]) & 15, False
        for k, (n, secs) in enumerate(dgrams):
            o = int(bt.offs[bt.first_dgram[j] + k])
            buf = bytearray(data[o:o + n].tobytes())
            if not encrypt:
                buf = bytearray(oracle.package(pk, piv, False, bytes(buf))) if n else buf
            for so, sn in secs:
                if sn:
                    c, civ, cpos = oracle.cfb(dk, encrypt, bytes(buf[so:so + sn]), civ, cpos)
                    buf[so:so + sn] = c
                    any_byte = True
            if encrypt and n:
                buf = bytearray(oracle.package(pk, piv, True, bytes(buf)))
            out[o:o + n] = np.frombuffer(bytes(buf), np.uint8)
        if any_byte:
            iv[s] = np.frombuffer(civ, np.uint8)
            pos[s] = cpos
    return out, iv, pos


def run(engine, fn, bt, t, slots, src, dst, iv, pos, slot_bound=None, dev=None, with_data=True):
    """One udp_encrypt / udp_decrypt call; src/dst device buffers (the same tensor: in place);
    iv/pos host state arrays.  -> (device iv, device pos)."""
    dev = dev or bt.dev()
    iv_d, pos_d = to_dev(iv.reshape(-1)), to_dev(pos.astype(np.int32))
    fn(src, dst, bt.count, t.pkg, t.data if with_data else None, bt.nconn, dev["first_dgram"], i32(slots),
       t.nslots if slot_bound is None else slot_bound, bt.nsections, dev["first_section"], dev["sec_off"],
       dev["sec_len"], iv_d, pos_d, in_off=dev["in_off"], lens=dev["lens"])
    return iv_d, pos_d


def check_state(iv_d, pos_d, iv, pos, what):
    assert np.array_equal(to_host(iv_d).reshape(-1, 16), iv), what + ": iv_state"
    assert np.array_equal(to_host(pos_d).astype(np.uint32), pos), what + ": pos_state"


def roundtrip(engine, oracle, bt, t, slots, rng, inplace, entries=None):
    """Encrypt against the reference, then decrypt of that ciphertext: plaintext and the same
    final states."""
    entries = entries or t.nslots
    data = bt.plaintext(rng)
    iv0, pos0 = initial_state(rng, entries, slots)
    out0 = data if inplace else np.full(bt.total, SENTINEL, np.uint8)
    exp, iv1, pos1 = reference(oracle, bt, t, slots, data, out0, iv0, pos0, True)
    src = to_dev(data)
    dst = src if inplace else to_dev(out0)
    iv_d, pos_d = run(engine, engine.udp_encrypt, bt, t, slots, src, dst, iv0, pos0)
    engine.sync()
    got = to_host(dst)
    assert np.array_equal(got, exp), ("ciphertext", int(np.count_nonzero(got != exp)))
    check_state(iv_d, pos_d, iv1, pos1, "encrypt")
    # decrypt of the reference's ciphertext
    src = to_dev(exp)
    dst = src if inplace else to_dev(out0)
    iv_d, pos_d = run(engine, engine.udp_decrypt, bt, t, slots, src, dst, iv0, pos0)
    engine.sync()
    got = to_host(dst)
    assert np.array_equal(got, data if inplace else np.where(mask(bt), data, SENTINEL)), \
        ("plaintext", int(np.count_nonzero(got != data)))
    check_state(iv_d, pos_d, iv1, pos1, "decrypt")


def mask(bt):
    m = np.zeros(bt.total, bool)
    for o, n in zip(bt.offs, bt.lens):
        m[o:o + n] = True
    return m


def random_sections(rng, n, k):
    """k ascending, non-overlapping sections inside a datagram of n bytes."""
    cuts = np.sort(rng.integers(0, n + 1, 2 * k))
    return [(int(cuts[2 * i]), int(cuts[2 * i + 1] - cuts[2 * i])) for i in range(k)]


def edge_connections(rng):
    """37 connections of 0 - 4 datagrams; the first ones carry the shapes that must be there."""
    fixed = [
        # a section at byte 0; one ending at the last byte; the realistic layout (8-byte package
        # header + 4-byte section header, data to the end)
        [(33, [(0, 5)]), (129, [(100, 29)]), (1472, [(12, 1460)]), (548, [(12, 536)])],
        # lengths 0, 1, 15, 16, 17; two adjacent sections
        [(128, [(3, 0), (10, 1), (20, 15)]), (127, [(1, 16), (40, 17)]), (548, [(12, 100), (112, 200)])],
        # a section that straddles two, and three, package-layer blocks; whole-datagram section
        [(32, [(14, 4)]), (129, [(15, 18)]), (17, [(0, 17)]), (16, [(0, 16)])],
        # datagrams without sections, a zero-length datagram (with and without a section)
        [(31, []), (0, []), (0, [(0, 0)]), (15, [(7, 8)])],
        [],                      # a connection without datagrams
        [(16, [(4, 0)]), (8, [])],  # sections all empty: the state keeps every bit
        [(1, [(0, 1)]), (7, [(0, 3), (3, 4)]), (1, [(0, 1)])],
    ]
    conns = list(fixed)
    pool = list(DGRAM_LENS)
    while len(conns) < 37:
        c = []
        for _ in range(4 if pool else int(rng.integers(0, 5))):
            n = int(pool.pop()) if pool else int(rng.integers(0, 1500))
            c.append((n, random_sections(rng, n, int(rng.integers(0, 4)))))
        conns.append(c)
    return conns


@pytest.mark.parametrize("inplace", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("pkg_len,data_len", PAIRS)
def test_edges(engine, oracle, pkg_len, data_len, inplace):
    """37 connections at permuted slots of 64-slot tables, gaps between the datagrams: the
    ciphertext, the final (iv, pos) of the named slots, every bit of the others, the sentinel;
    then decrypt back."""
    rng = np.random.default_rng(1000 + pkg_len + 2 * data_len + inplace)
    bt = Batch(edge_connections(rng), rng)
    assert bt.nconn == 37 and set(DGRAM_LENS) <= set(bt.lens.tolist())
    t = Tables(engine, rng, 64, pkg_len, data_len)
    try:
        roundtrip(engine, oracle, bt, t, rng.permutation(64)[:37], rng, inplace)
    finally:
        t.close()


def test_population_300(engine, oracle):
    """300 connections of short datagrams: more than one workgroup's quads."""
    rng = np.random.default_rng(300)
    conns = []
    for _ in range(300):
        c = []
        for _ in range(int(rng.integers(1, 3))):
            n = int(rng.integers(13, 65))
            c.append((n, [(12, n - 12)]))
        conns.append(c)
    bt = Batch(conns, rng)
    t = Tables(engine, rng, 512, 16, 32)
    try:
        roundtrip(engine, oracle, bt, t, rng.permutation(512)[:300], rng, False)
    finally:
        t.close()


def test_population_70000(engine, oracle):
    """70 000 connections x one datagram of at most 64 bytes with one section: more than the
    chip's 65 536 quads, so the grid-stride loop takes a second trip.  (The reference runs
    through the oracle's batch calls: one stream segment per section, then one package
    segment per datagram.)"""
    rng = np.random.default_rng(70000)
    n = 70000
    lens = rng.integers(13, 65, n).astype(np.int32)
    bt = Batch([[(int(x), [(12, int(x) - 12)])] for x in lens], rng)
    t = Tables(engine, rng, n, 16, 32)
    try:
        slots = rng.permutation(n)
        data = bt.plaintext(rng)
        iv0, pos0 = initial_state(rng, n, slots)
        mid = data.copy()
        iv_s, pos_s = np.ascontiguousarray(iv0[slots]).reshape(-1), np.ascontiguousarray(pos0[slots]).astype(np.uint32)
        sec_abs = (bt.offs + 12).astype(np.uint64)
        oracle.stream_batch(True, data, mid, n, in_off=sec_abs, out_off=sec_abs, lens=bt.sec_len.astype(np.uint32),
                            key_slot=slots.astype(np.uint32), keys=t.dkeys.reshape(-1), keylen=32, iv_state=iv_s,
                            pos_state=pos_s, threads=8)
        exp = np.full(bt.total, SENTINEL, np.uint8)
        oracle.package_batch(True, mid, exp, n, in_off=bt.offs.astype(np.uint64), lens=bt.lens.astype(np.uint32),
                             key_slot=slots.astype(np.uint32), keys=t.pkeys.reshape(-1), keylen=16,
                             ivs=t.pivs.reshape(-1), threads=8)
        iv1, pos1 = iv0.copy(), pos0.copy()
        iv1[slots], pos1[slots] = iv_s.reshape(-1, 16), pos_s
        src, dst = to_dev(data), to_dev(np.full(bt.total, SENTINEL, np.uint8))
        iv_d, pos_d = run(engine, engine.udp_encrypt, bt, t, slots, src, dst, iv0, pos0)
        engine.sync()
        assert np.array_equal(to_host(dst), exp), "ciphertext"
        check_state(iv_d, pos_d, iv1, pos1, "encrypt")
        back = to_dev(exp)
        iv_d, pos_d = run(engine, engine.udp_decrypt, bt, t, slots, back, back, iv0, pos0)
        engine.sync()
        assert np.array_equal(to_host(back), data), "plaintext"
        check_state(iv_d, pos_d, iv1, pos1, "decrypt")
    finally:
        t.close()


def test_many_datagrams_and_split_calls(engine, oracle):
    """64 connections x 16 datagrams of 1472 bytes with the section [12, 1472): the data state
    crosses datagram boundaries at every alignment (1460 = 91 * 16 + 4).  The same work split
    into two successive calls of 8 datagrams per connection gives the same bytes and states."""
    rng = np.random.default_rng(6416)
    conns = [[(1472, [(12, 1460)])] * 16 for _ in range(64)]
    bt = Batch(conns, rng)
    t = Tables(engine, rng, 64, 16, 32)
    try:
        slots = rng.permutation(64)
        data = bt.plaintext(rng)
        iv0, pos0 = initial_state(rng, 64, slots)
        out0 = np.full(bt.total, SENTINEL, np.uint8)
        exp, iv1, pos1 = reference(oracle, bt, t, slots, data, out0, iv0, pos0, True)
        src, dst = to_dev(data), to_dev(out0)
        iv_d, pos_d = run(engine, engine.udp_encrypt, bt, t, slots, src, dst, iv0, pos0)
        engine.sync()
        assert np.array_equal(to_host(dst), exp), "one call: ciphertext"
        check_state(iv_d, pos_d, iv1, pos1, "one call")
        back = to_dev(exp)
        iv_d, pos_d = run(engine, engine.udp_decrypt, bt, t, slots, back, back, iv0, pos0)
        engine.sync()
        assert np.array_equal(to_host(back), data), "one call: plaintext"
        check_state(iv_d, pos_d, iv1, pos1, "one call: decrypt")
        # two calls: datagrams 0 - 7 of every connection, then 8 - 15, at the same addresses
        offs = bt.offs.reshape(64, 16)
        halves = [Batch([c[:8] for c in conns], rng, offs[:, :8]), Batch([c[8:] for c in conns], rng, offs[:, 8:])]
        for fn, inp, want, what in ((engine.udp_encrypt, data, exp, "encrypt"), (engine.udp_decrypt, exp, data, "decrypt")):
            src, dst = to_dev(inp), to_dev(out0)
            iv_d, pos_d = to_dev(iv0.reshape(-1)), to_dev(pos0.astype(np.int32))
            for h in halves:
                d = h.dev()
                fn(src, dst, h.count, t.pkg, t.data, 64, d["first_dgram"], i32(slots), 64, h.nsections,
                   d["first_section"], d["sec_off"], d["sec_len"], iv_d, pos_d, in_off=d["in_off"], lens=d["lens"])
            engine.sync()
            got = to_host(dst)
            assert np.array_equal(got, np.where(mask(bt), want, SENTINEL)), "two calls: " + what
            check_state(iv_d, pos_d, iv1, pos1, "two calls: " + what)
    finally:
        t.close()


# ---------------------------------------------------------------------------------------
# contract


def expect_device_error_once(engine):
    import fpnn_amd
    with pytest.raises(fpnn_amd.FpnnAesError) as ei:
        engine.sync()
    assert ei.value.status == fpnn_amd.ERR_DEVICE
    engine.sync()  # reported once


@pytest.mark.parametrize("encrypt", [True, False], ids=["encrypt", "decrypt"])
def test_slot_past_the_bound(engine, oracle, encrypt):
    """One conn_slot >= slot_bound: its state is untouched, encrypt writes no byte for it, the
    other connections are exact, sync reports FPNN_AES_ERR_DEVICE once and then OK."""
    rng = np.random.default_rng(64 + encrypt)
    bt = Batch(edge_connections(rng), rng)
    t = Tables(engine, rng, 64, 16, 32)
    try:
        slots = rng.permutation(60)[:37]
        bad = 2  # (a connection with datagrams and sections)
        slots[bad] = 61
        data = bt.plaintext(rng)
        iv0, pos0 = initial_state(rng, 64, np.delete(slots, bad))
        out0 = np.full(bt.total, SENTINEL, np.uint8)
        exp, iv1, pos1 = reference(oracle, bt, t, slots, data, out0, iv0, pos0, encrypt, skip=(bad,))
        src, dst = to_dev(data), to_dev(out0)
        fn = engine.udp_encrypt if encrypt else engine.udp_decrypt
        iv_d, pos_d = run(engine, fn, bt, t, slots, src, dst, iv0, pos0, slot_bound=60)  # arrays hold 64 entries
        expect_device_error_once(engine)
        got = to_host(dst)
        if not encrypt:  # its own output bytes are unspecified
            own = np.zeros(bt.total, bool)
            for k in range(bt.first_dgram[bad], bt.first_dgram[bad + 1]):
                own[bt.offs[k]:bt.offs[k] + bt.lens[k]] = True
            got[own] = exp[own]
        assert np.array_equal(got, exp), int(np.count_nonzero(got != exp))
        check_state(iv_d, pos_d, iv1, pos1, "state")
    finally:
        t.close()


@pytest.mark.parametrize("encrypt", [True, False], ids=["encrypt", "decrypt"])
def test_section_past_its_datagram(engine, oracle, encrypt):
    """One section with sec_off + sec_len past its datagram: no byte outside that datagram's
    connection changes unduly -- the sentinel and every other connection are exact -- and
    sync reports FPNN_AES_ERR_DEVICE once."""
    rng = np.random.default_rng(640 + encrypt)
    conns = edge_connections(rng)
    bt = Batch(conns, rng)
    good = Batch(conns, rng, bt.offs)
    bad_conn = 2
    s = int(bt.first_section[bt.first_dgram[bad_conn]])  # the first section of its first datagram
    assert bt.sec_len[s] > 0
    bt.sec_len[s] = 5000
    t = Tables(engine, rng, 64, 32, 16)
    try:
        slots = rng.permutation(64)[:37]
        data = bt.plaintext(rng)
        iv0, pos0 = initial_state(rng, 64, slots)
        out0 = np.full(bt.total, SENTINEL, np.uint8)
        exp, iv1, pos1 = reference(oracle, good, t, slots, data, out0, iv0, pos0, encrypt)
        src, dst = to_dev(data), to_dev(out0)
        fn = engine.udp_encrypt if encrypt else engine.udp_decrypt
        iv_d, pos_d = run(engine, fn, bt, t, slots, src, dst, iv0, pos0)
        expect_device_error_once(engine)
        got = to_host(dst)
        own = np.zeros(bt.total, bool)  # the bad connection's datagrams: results invalid
        for k in range(bt.first_dgram[bad_conn], bt.first_dgram[bad_conn + 1]):
            own[bt.offs[k]:bt.offs[k] + bt.lens[k]] = True
        assert np.array_equal(got[~own], exp[~own]), int(np.count_nonzero(got[~own] != exp[~own]))
        others = np.delete(np.arange(64), slots[bad_conn])
        assert np.array_equal(to_host(iv_d).reshape(-1, 16)[others], iv1[others])
        assert np.array_equal(to_host(pos_d).astype(np.uint32)[others], pos1[others])
    finally:
        t.close()


def test_no_sections_is_package_encrypt(engine):
    """A datagram batch with nsections == 0 equals package_encrypt with the expanded key slots
    (with and without a data table), and leaves every bit of state."""
    rng = np.random.default_rng(5)
    bt = Batch([[(int(n), []) for n in rng.choice(DGRAM_LENS, int(rng.integers(0, 5)))] for _ in range(37)], rng)
    t = Tables(engine, rng, 64, 32, 16)
    try:
        slots = rng.permutation(64)[:37]
        data = bt.plaintext(rng)
        dev = bt.dev()
        dg_slot = np.repeat(slots, np.diff(bt.first_dgram))
        src, want = to_dev(data), to_dev(np.full(bt.total, SENTINEL, np.uint8))
        engine.package_encrypt(src, want, bt.count, t.pkg, in_off=dev["in_off"], lens=dev["lens"], key_slot=i32(dg_slot))
        iv0, pos0 = initial_state(rng, 64, slots)
        for with_data in (True, False):
            dst = to_dev(np.full(bt.total, SENTINEL, np.uint8))
            iv_d, pos_d = run(engine, engine.udp_encrypt, bt, t, slots, src, dst, iv0, pos0, dev=dev,
                              with_data=with_data)
            engine.sync()
            assert torch.equal(dst, want), with_data
            check_state(iv_d, pos_d, iv0, pos0, "state")
            back = to_dev(np.full(bt.total, SENTINEL, np.uint8))
            iv_d, pos_d = run(engine, engine.udp_decrypt, bt, t, slots, want, back, iv0, pos0, dev=dev,
                              with_data=with_data)
            engine.sync()
            assert np.array_equal(to_host(back), data), with_data
            check_state(iv_d, pos_d, iv0, pos0, "state")
    finally:
        t.close()


def test_argument_errors(engine):
    """Every FPNN_AES_ERR_ARG / _KEYLEN case of the header, on a real engine; nconn == 0 and
    b->count == 0 are OK and queue nothing."""
    import fpnn_amd
    from fpnn_amd._lib import UdpData, lib
    rng = np.random.default_rng(7)
    t = Tables(engine, rng, 8, 16, 32)
    t24 = Tables(engine, rng, 8, 24, 24)
    other = fpnn_amd.Engine(0)
    foreign = keyset(other, t.dkeys.reshape(-1), 32, t.divs.reshape(-1))
    try:
        buf = torch.zeros(256, dtype=torch.uint8, device="cuda:0")
        words = torch.zeros(64, dtype=torch.int32, device="cuda:0")
        state = torch.zeros(16 * 8 + 16, dtype=torch.uint8, device="cuda:0")
        a16 = state.data_ptr() + (-state.data_ptr() % 16)

        def call(fn, **over):
            d = engine._desc(buf, buf, 2, t.pkg, stride=64, uniform_len=64)
            u = UdpData()
            u.data_keys, u.nconn, u.slot_bound, u.nsections = t.data.handle.value, 2, 8, 2
            u.first_dgram = u.conn_slot = u.first_section = u.sec_off = u.sec_len = u.pos_state = words.data_ptr()
            u.iv_state = a16
            up = C.byref(u)
            for k, v in over.items():
                if k == "u":
                    up = v
                elif hasattr(d, k) and k not in ("nconn",):
                    setattr(d, k, v)
                else:
                    setattr(u, k, v)
            return fn(engine.handle, C.byref(d), up)

        for fn in (lib.fpnn_aes_udp_encrypt, lib.fpnn_aes_udp_decrypt):
            bad = [dict(key_slot=words.data_ptr()), dict(flags=1), dict(u=None),
                   dict(data_keys=None), dict(data_keys=foreign.handle.value), dict(slot_bound=9)]
            for name in ("first_dgram", "conn_slot", "pos_state", "iv_state", "first_section", "sec_off", "sec_len"):
                bad += [{name: None}, {name: words.data_ptr() + 2}]
            bad.append(dict(iv_state=a16 + 4))
            for over in bad:
                assert call(fn, **over) == fpnn_amd.ERR_ARG, over
            assert call(fn, keys=t24.pkg.handle.value) == fpnn_amd.ERR_KEYLEN
            assert call(fn, data_keys=t24.data.handle.value) == fpnn_amd.ERR_KEYLEN
            # nothing to do: OK whatever the arrays are
            assert call(fn, nconn=0, first_dgram=None, conn_slot=None, iv_state=None, pos_state=None) == fpnn_amd.OK
            assert call(fn, count=0) == fpnn_amd.OK
            assert call(fn, nsections=0, data_keys=None, first_section=None, sec_off=None, sec_len=None,
                        nconn=0) == fpnn_amd.OK
        engine.sync()
    finally:
        foreign.close()
        other.close()
        t.close()
        t24.close()


def test_reserve_covers_both_calls(oracle):
    """After reserve(max(count, nsections, nconn), blocks) a call within the bounds grows no
    scratch (fpnn_aes_engine_scratch_bytes stays put) and is exact; an engine that never
    reserved grows its scratch on the same decrypt."""
    import fpnn_amd
    rng = np.random.default_rng(11)
    conns = [[(int(rng.integers(20, 200)), [(12, 8)]) for _ in range(int(rng.integers(1, 4)))] for _ in range(700)]
    bt = Batch(conns, rng)
    for reserved in (True, False):
        eng = fpnn_amd.Engine(0)
        t = Tables(eng, rng, 2048, 16, 32)
        try:
            if reserved:
                eng.reserve(max(bt.count, bt.nsections, bt.nconn), bt.total // 16 + bt.count)
            held = eng.scratch_bytes()
            roundtrip(eng, oracle, bt, t, rng.permutation(2048)[:700], rng, True)
            roundtrip(eng, oracle, bt, t, rng.permutation(2048)[:700], rng, False)
            assert eng.scratch_bytes() == held if reserved else eng.scratch_bytes() > held
        finally:
            eng.sync()
            t.close()
            eng.close()
