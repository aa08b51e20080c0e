"""UDP v2 receive on the device (include/fpnn_aes.h: fpnn_aes_udp_recv / _recv_take;
fpnn_amd/csrc/k_udp_recv.hip): package-decrypt, walk the packages and components, data-decrypt
the sections of the packages taken.

Expected values have two sources.  The tables are tests/udp_wire.py's: a Python restatement of
ARQParser's structural walk, tested by itself in tests/test_udp_wire.py.  The bytes and states are
pyoracle's two ciphers composed as tests/test_gpu_udp.py composes them: the input is
oracle.package(encrypt) of every wire datagram; the output is the wire datagram with every
section the data layer decrypts run through oracle.cfb(decrypt), continuing the connection's
(iv, pos) in the order the packages are taken.  (The sections' bytes are random: the data layer
is a bijection, so "ciphertext" needs no sender.)  Everything is bit-exact: the whole buffer with
a sentinel outside the datagrams, the whole state arrays with a fill at unnamed slots, every
used table entry -- and the unused ones, which must keep the pattern they were given.
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import udp_wire as W  # noqa: E402
from test_gpu_parity import to_dev, to_host  # noqa: E402
from test_gpu_udp import (IV_FILL, PAIRS, POS_FILL, SENTINEL, Tables, check_state, expect_device_error_once, i32,  # noqa: E402
                          initial_state)

pytestmark = pytest.mark.gpu

TABLE_FILL = 0x5B  # every byte of the tables before a call: entries past the used counts keep it
WALK_ONLY, PLAIN = 1, 2
CASES = {c[0]: c for c in W.cases()}


class Batch:
    """Wire datagrams of `conns` connections (conns[j]: connection j's datagrams, bytes, in
    arrival order) at offsets with gaps of 1 - 6 bytes, and their walks."""

    def __init__(self, conns, rng, max_pkgs=4, max_sections=8):
        self.conns, self.nconn = conns, len(conns)
        self.max_pkgs, self.max_sections = max_pkgs, max_sections
        self.first_dgram = np.concatenate([[0], np.cumsum([len(c) for c in conns])]).astype(np.int32)
        self.dgrams = [d for c in conns for d in c]
        self.owner = [j for j, c in enumerate(conns) for _ in c]
        self.count = len(self.dgrams)
        self.lens = np.array([len(d) for d in self.dgrams], np.int32).reshape(-1)
        gaps = rng.integers(1, 7, self.count)
        self.offs = (3 + np.concatenate([[0], np.cumsum(self.lens[:-1].astype(np.int64) + gaps[:-1])])
                     if self.count else np.zeros(0, np.int64)).astype(np.int64)
        self.total = int((self.offs + self.lens).max()) + 9 if self.count else 16
        self.walks = [W.Walk(d, max_pkgs, max_sections) for d in self.dgrams]

    def plain(self):
        """The buffer after the package layer: every wire datagram, the sentinel elsewhere."""
        buf = np.full(self.total, SENTINEL, np.uint8)
        for o, d in zip(self.offs, self.dgrams):
            buf[o:o + len(d)] = np.frombuffer(d, np.uint8)
        return buf

    def wire(self, oracle, t, slots):
        """What arrives: every datagram package-encrypted under its connection's slot."""
        buf = np.full(self.total, SENTINEL, np.uint8)
        for i, (o, d) in enumerate(zip(self.offs, self.dgrams)):
            s = int(slots[self.owner[i]])
            if d:
                buf[o:o + len(d)] = np.frombuffer(oracle.package(t.pkeys[s].tobytes(), t.pivs[s].tobytes(), True, d), np.uint8)
        return buf

    def all_packages(self):
        """Per connection every package of every datagram in array order: (datagram, package)."""
        return [[(i, k) for i in range(self.first_dgram[j], self.first_dgram[j + 1]) for k in range(len(self.walks[i].pkgs))]
                for j in range(self.nconn)]

    def dev(self):
        z = lambda a, dt: to_dev(np.asarray(a if len(a) else np.zeros(1), dt))  # noqa: E731
        return dict(first_dgram=i32(self.first_dgram), in_off=z(self.offs, np.int64), lens=z(self.lens, np.int32))


def data_decrypt(oracle, bt, t, slots, buf, iv, pos, order, skip=()):
    """The data layer on `buf` (package-plaintext) and the states, in place: connection j's
    packages order[j] in that order, their decrypted sections in section order."""
    for j, pkgs in enumerate(order):
        if j in skip:
            continue
        s = int(slots[j])
        dk, civ, cpos, any_byte = t.dkeys[s].tobytes(), iv[s].tobytes(), int(pos[s]) & 15, False
        for i, k in pkgs:
            for off, n in bt.walks[i].decrypted(k):
                if n:
                    a = int(bt.offs[i]) + off
                    p, civ, cpos = oracle.cfb(dk, False, buf[a:a + n].tobytes(), civ, cpos)
                    buf[a:a + n] = np.frombuffer(p, np.uint8)
                    any_byte = True
        if any_byte:
            iv[s] = np.frombuffer(civ, np.uint8)
            pos[s] = cpos


def fresh_tables(bt):
    n = max(bt.count, 1)
    return [to_dev(np.full((n * rows, words), TABLE_FILL * 0x01010101, np.uint32).view(np.int32))
            for rows, words in ((1, 2), (bt.max_pkgs, 4), (bt.max_sections, 4))]


def check_tables(bt, tabs, what=""):
    scan, pkgs, secs = (to_host(x).reshape(-1).view(dt) for x, dt in zip(tabs, (W.SCAN, W.PKG, W.SECTION)))
    e_scan, e_pkgs, e_secs, pu, su = W.tables(bt.walks, bt.max_pkgs, bt.max_sections)
    n = bt.count
    assert np.array_equal(scan[:n], e_scan), (what, "scan", np.flatnonzero(scan[:n] != e_scan)[:5])
    for got, exp, used, name in ((pkgs[:n * bt.max_pkgs], e_pkgs, pu, "pkgs"), (secs[:n * bt.max_sections], e_secs, su, "sections")):
        assert np.array_equal(got[used], exp[used]), (what, name, np.flatnonzero(used)[got[used] != exp[used]][:5],
                                                       got[used][got[used] != exp[used]][:3], exp[used][got[used] != exp[used]][:3])
        assert np.all(got[~used].view(np.uint8) == TABLE_FILL), (what, name, "an entry past the used count was written")


def recv(engine, bt, t, slots, src, dst, iv_d, pos_d, flags=0, tabs=None, slot_bound=None, dev=None, with_data=True):
    dev = dev or bt.dev()
    tabs = tabs or fresh_tables(bt)
    engine.udp_recv(src, dst, bt.count, t.pkg, t.data if with_data else None, bt.nconn, dev["first_dgram"], i32(slots),
                    t.nslots if slot_bound is None else slot_bound, iv_d, pos_d, bt.max_pkgs, bt.max_sections, flags=flags,
                    scan=tabs[0], pkgs=tabs[1], sections=tabs[2], in_off=dev["in_off"], lens=dev["lens"])
    return tabs


def take_lists(bt, order):
    first = np.concatenate([[0], np.cumsum([len(o) for o in order])]).astype(np.int32)
    flat = np.array([i * bt.max_pkgs + k for o in order for i, k in o] or [0], np.int32)
    return first, flat, int(first[-1])


def recv_take(engine, bt, t, slots, buf, iv_d, pos_d, tabs, first, flat, ntake, slot_bound=None, dev=None):
    dev = dev or bt.dev()
    engine.udp_recv_take(buf, buf, bt.count, t.pkg, t.data, bt.nconn, dev["first_dgram"], i32(slots),
                         t.nslots if slot_bound is None else slot_bound, iv_d, pos_d, bt.max_pkgs, bt.max_sections,
                         tabs[0], tabs[1], tabs[2], i32(first), i32(flat), ntake, in_off=dev["in_off"], lens=dev["lens"])


def single_call(engine, oracle, bt, t, slots, rng, inplace, entries=None):
    """One fpnn_aes_udp_recv call against the oracle: tables, bytes, states."""
    iv0, pos0 = initial_state(rng, entries or t.nslots, slots)
    exp, iv1, pos1 = bt.plain(), iv0.copy(), pos0.copy()
    data_decrypt(oracle, bt, t, slots, exp, iv1, pos1, bt.all_packages())
    src = to_dev(bt.wire(oracle, t, slots))
    dst = src if inplace else to_dev(np.full(bt.total, SENTINEL, np.uint8))
    iv_d, pos_d = to_dev(iv0.reshape(-1)), to_dev(pos0.astype(np.int32))
    tabs = recv(engine, bt, t, slots, src, dst, iv_d, pos_d)
    engine.sync()
    check_tables(bt, tabs)
    got = to_host(dst)
    assert np.array_equal(got, exp), ("bytes", np.flatnonzero(got != exp)[:8])
    check_state(iv_d, pos_d, iv1, pos1, "single call")


# ---------------------------------------------------------------------------------------
# 1, 2: the families and the section geometry


@pytest.mark.parametrize("pkg_len,data_len", PAIRS)
def test_families(engine, oracle, pkg_len, data_len):
    """One connection, one datagram of each family, each in a call of its own: the tables, the
    decrypted sections (a discardable or cancelled DATA, and the DATA after a CLOSE, stay as
    they came), the state."""
    rng = np.random.default_rng(100 + pkg_len + 2 * data_len)
    t = Tables(engine, rng, 8, pkg_len, data_len)
    try:
        for k, name in enumerate(W.FAMILIES):
            bt = Batch([[CASES[name][1]]], rng)
            assert bt.walks[0].status == W.OK, name
            single_call(engine, oracle, bt, t, [k % 8], rng, inplace=bool(k & 1))
    finally:
        t.close()


@pytest.mark.parametrize("pkg_len,data_len", PAIRS)
def test_section_geometry(engine, oracle, pkg_len, data_len):
    """Payload lengths 0, 1, 15, 16, 17 and 1460 in three datagrams per connection, 32 connections
    whose chains come in at every position 0 - 15: the state carries from datagram to datagram
    across every alignment.  Whole-package DATA (segmented and not) and COMBINED alternate."""
    rng = np.random.default_rng(200 + pkg_len + 2 * data_len)
    L = (0, 1, 15, 16, 17, 1460)

    def dgram(form, n, seq):
        body = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        if form == 0:
            return W.package(W.DATA, 0, seq, body)
        if form == 1:
            return W.package(W.DATA, W.SEG2, seq, W.data_body(W.SEG2, body, seq & 0xFFFF, seq))
        return W.combined([W.component(W.UNA, 0, b"\0\0\0\1"), W.component(W.DATA, W.SEG1, W.data_body(W.SEG1, body, 7, 3)),
                           W.component(W.DATA, 0, body[:n // 2])], seq=seq)

    conns = [[dgram((j + k) % 3, L[(j + 2 * k) % 6], 10 * j + k) for k in range(3)] for j in range(32)]
    bt = Batch(conns, rng)
    assert {s["len"] for w in bt.walks for s in w.sections} >= set(L)
    t = Tables(engine, rng, 64, pkg_len, data_len)
    try:
        single_call(engine, oracle, bt, t, rng.permutation(64)[:32], rng, inplace=False)
    finally:
        t.close()


# ---------------------------------------------------------------------------------------
# 3: hostile bytes


HOSTILE = [c for c in W.cases() if c[0] not in W.FAMILIES]


@pytest.mark.parametrize("max_pkgs,max_sections", sorted({(c[2], c[3]) for c in HOSTILE}))
def test_hostile_bytes(engine, oracle, max_pkgs, max_sections):
    """Every hostile datagram of udp_wire.cases() as a connection of its own, between two good
    ones: the status, the sections recorded before the rejection (and decrypted: the reference
    has processed them), the state, and no byte outside the datagrams."""
    rng = np.random.default_rng(300 + max_pkgs)
    mine = [c for c in HOSTILE if (c[2], c[3]) == (max_pkgs, max_sections)]
    good = CASES["data"][1]
    conns = [[good]] + [[c[1]] for c in mine] + [[good]]
    bt = Batch(conns, rng, max_pkgs, max_sections)
    for c, w in zip(mine, bt.walks[1:]):
        assert w.status == c[4], c[0]
    t = Tables(engine, rng, 64, 16, 32)
    try:
        single_call(engine, oracle, bt, t, rng.permutation(64)[:bt.nconn], rng, inplace=True)
    finally:
        t.close()


# ---------------------------------------------------------------------------------------
# 4, 5: WALK_ONLY, the host's order, PLAIN


def mixed_connections(rng, nconn, per_conn):
    names = ("data", "data_seg1", "data_seg2", "data_seg4", "combined_mix", "combined_close", "assembled_two",
             "heartbeat8", "cancelled_seg", "acks", "una")
    conns = []
    for j in range(nconn):
        c = []
        for k in range(per_conn):
            d = bytearray(CASES[names[(3 * j + k) % len(names)]][1])
            w = W.Walk(bytes(d))
            for s in w.sections:  # fresh payload bytes, the structure as it is
                d[s["off"]:s["off"] + s["len"]] = rng.integers(0, 256, s["len"], dtype=np.uint8).tobytes()
            c.append(bytes(d))
        conns.append(c)
    return conns


@pytest.mark.parametrize("pkg_len,data_len", PAIRS)
def test_walk_only_then_take(engine, oracle, pkg_len, data_len):
    """40 connections x 5 datagrams.  WALK_ONLY leaves package-plaintext and every bit of state;
    the host then takes each connection's packages in a permuted order and leaves every third
    out: the result is the oracle's run in that order; a second take of the rest completes the
    chain.  Then PLAIN | WALK_ONLY over the package-plaintext: identical tables, no byte changed."""
    rng = np.random.default_rng(40 + pkg_len + 2 * data_len)
    bt = Batch(mixed_connections(rng, 40, 5), rng)
    t = Tables(engine, rng, 64, pkg_len, data_len)
    try:
        slots = rng.permutation(64)[:40]
        iv0, pos0 = initial_state(rng, 64, slots)
        buf = to_dev(bt.wire(oracle, t, slots))
        iv_d, pos_d = to_dev(iv0.reshape(-1)), to_dev(pos0.astype(np.int32))
        tabs = recv(engine, bt, t, slots, buf, buf, iv_d, pos_d, flags=WALK_ONLY)
        engine.sync()
        check_tables(bt, tabs, "WALK_ONLY")
        exp = bt.plain()
        assert np.array_equal(to_host(buf), exp), "WALK_ONLY: package-plaintext"
        check_state(iv_d, pos_d, iv0, pos0, "WALK_ONLY")
        # PLAIN | WALK_ONLY (a datagram back from the disordered cache): the same tables, without a data table too
        again = recv(engine, bt, t, slots, buf, buf, iv_d, pos_d, flags=PLAIN | WALK_ONLY, with_data=False)
        engine.sync()
        for a, b in zip(tabs, again):
            assert torch.equal(a, b), "PLAIN | WALK_ONLY: tables"
        assert np.array_equal(to_host(buf), exp), "PLAIN | WALK_ONLY: bytes"
        check_state(iv_d, pos_d, iv0, pos0, "PLAIN | WALK_ONLY")
        # the host's order
        first_order, rest = [], []
        for pk in bt.all_packages():
            pk = [pk[x] for x in rng.permutation(len(pk))]
            first_order.append([p for x, p in enumerate(pk) if x % 3 != 2])
            rest.append([p for x, p in enumerate(pk) if x % 3 == 2])
        assert sum(map(len, rest)) > 40
        iv1, pos1 = iv0.copy(), pos0.copy()
        for order, what in ((first_order, "first take"), (rest, "second take")):
            data_decrypt(oracle, bt, t, slots, exp, iv1, pos1, order)
            recv_take(engine, bt, t, slots, buf, iv_d, pos_d, tabs, *take_lists(bt, order))
            engine.sync()
            got = to_host(buf)
            assert np.array_equal(got, exp), (what, np.flatnonzero(got != exp)[:8])
            check_state(iv_d, pos_d, iv1, pos1, what)
        check_tables(bt, tabs, "after the takes")
    finally:
        t.close()


@pytest.mark.parametrize("pkg_len,data_len", PAIRS)
def test_plain_single_call(engine, oracle, pkg_len, data_len):
    """PLAIN without WALK_ONLY: walk and data decrypt of package-plaintext in one call."""
    rng = np.random.default_rng(410 + pkg_len + 2 * data_len)
    bt = Batch(mixed_connections(rng, 9, 3), rng)
    t = Tables(engine, rng, 16, pkg_len, data_len)
    try:
        slots = rng.permutation(16)[:9]
        iv0, pos0 = initial_state(rng, 16, slots)
        exp, iv1, pos1 = bt.plain(), iv0.copy(), pos0.copy()
        buf = to_dev(exp)
        data_decrypt(oracle, bt, t, slots, exp, iv1, pos1, bt.all_packages())
        iv_d, pos_d = to_dev(iv0.reshape(-1)), to_dev(pos0.astype(np.int32))
        tabs = recv(engine, bt, t, slots, buf, buf, iv_d, pos_d, flags=PLAIN)
        engine.sync()
        check_tables(bt, tabs)
        assert np.array_equal(to_host(buf), exp)
        check_state(iv_d, pos_d, iv1, pos1, "PLAIN")
    finally:
        t.close()


# ---------------------------------------------------------------------------------------
# 6: equivalence with fpnn_aes_udp_decrypt


@pytest.mark.parametrize("pkg_len,data_len", PAIRS)
def test_equals_udp_decrypt_with_the_sections_supplied(engine, oracle, pkg_len, data_len):
    """Datagrams whose sections are all non-discardable DATA: fpnn_aes_udp_recv gives the bytes
    and states of fpnn_aes_udp_decrypt told where the sections lie."""
    rng = np.random.default_rng(600 + pkg_len + 2 * data_len)
    conns = []
    for j in range(23):
        c = []
        for k in range(int(rng.integers(0, 5))):
            n = int(rng.integers(0, 1461))
            body = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
            c.append(W.package(W.DATA, W.SEG2, k, W.data_body(W.SEG2, body, j, k)) if (j + k) & 1 else
                     W.combined([W.component(W.DATA, 0, body), W.component(W.DATA, W.SEG4, W.data_body(W.SEG4, body[:40], 1, 2))]))
        conns.append(c)
    bt = Batch(conns, rng)
    secs = [[(s["off"], s["len"]) for s in w.sections] for w in bt.walks]
    assert all(w.status == W.OK and all(s["type"] == W.DATA for s in w.sections) for w in bt.walks)
    t = Tables(engine, rng, 32, pkg_len, data_len)
    try:
        slots = rng.permutation(32)[:23]
        iv0, pos0 = initial_state(rng, 32, slots)
        wire = bt.wire(oracle, t, slots)
        dev = bt.dev()
        a, b = to_dev(wire), to_dev(wire)
        iv_a, pos_a = to_dev(iv0.reshape(-1)), to_dev(pos0.astype(np.int32))
        iv_b, pos_b = to_dev(iv0.reshape(-1)), to_dev(pos0.astype(np.int32))
        recv(engine, bt, t, slots, a, a, iv_a, pos_a, dev=dev)
        first_section = np.concatenate([[0], np.cumsum([len(s) for s in secs])]).astype(np.int32)
        flat = [s for d in secs for s in d]
        engine.udp_decrypt(b, b, bt.count, t.pkg, t.data, bt.nconn, dev["first_dgram"], i32(slots), 32, len(flat),
                           i32(first_section), i32([s[0] for s in flat]), i32([s[1] for s in flat]), iv_b, pos_b,
                           in_off=dev["in_off"], lens=dev["lens"])
        engine.sync()
        assert torch.equal(a, b) and torch.equal(iv_a, iv_b) and torch.equal(pos_a, pos_b)
        assert not np.array_equal(to_host(a), bt.plain())  # (the data layer did run)
    finally:
        t.close()


# ---------------------------------------------------------------------------------------
# 7: batch shapes


@pytest.mark.parametrize("pkg_len,data_len", PAIRS)
def test_uneven_connections(engine, oracle, pkg_len, data_len):
    """300 datagrams over 7 connections of uneven counts, two of them empty."""
    rng = np.random.default_rng(700 + pkg_len + 2 * data_len)
    counts = [120, 0, 1, 77, 0, 99, 3]
    pool = mixed_connections(rng, 1, 300)[0]
    conns, at = [], 0
    for n in counts:
        conns.append(pool[at:at + n])
        at += n
    bt = Batch(conns, rng)
    assert bt.count == 300
    t = Tables(engine, rng, 8, pkg_len, data_len)
    try:
        single_call(engine, oracle, bt, t, rng.permutation(8)[:7], rng, inplace=True)
    finally:
        t.close()


@pytest.mark.parametrize("pkg_len,data_len", PAIRS)
def test_nothing_to_do(engine, pkg_len, data_len):
    """nconn == 0 or count == 0: OK, nothing queued -- tables, bytes and state untouched."""
    rng = np.random.default_rng(8)
    t = Tables(engine, rng, 8, pkg_len, data_len)
    try:
        bt = Batch([[CASES["data"][1]]], rng)
        buf = to_dev(bt.plain())
        iv0, pos0 = initial_state(rng, 8, [3])
        iv_d, pos_d = to_dev(iv0.reshape(-1)), to_dev(pos0.astype(np.int32))
        dev = bt.dev()
        for count, nconn in ((0, 1), (1, 0), (0, 0)):
            tabs = fresh_tables(bt)
            engine.udp_recv(buf, buf, count, t.pkg, t.data, nconn, dev["first_dgram"], i32([3]), 8, iv_d, pos_d, 4, 8,
                            scan=tabs[0], pkgs=tabs[1], sections=tabs[2], in_off=dev["in_off"], lens=dev["lens"])
            engine.udp_recv_take(buf, buf, count, t.pkg, t.data, nconn, dev["first_dgram"], i32([3]), 8, iv_d, pos_d, 4, 8,
                                 tabs[0], tabs[1], tabs[2], i32([0, 1]), i32([0]), 1, in_off=dev["in_off"], lens=dev["lens"])
            engine.sync()
            assert all(np.all(to_host(x).view(np.uint8) == TABLE_FILL) for x in tabs)
        # no package taken
        tabs = fresh_tables(bt)
        engine.udp_recv_take(buf, buf, 1, t.pkg, t.data, 1, dev["first_dgram"], i32([3]), 8, iv_d, pos_d, 4, 8,
                             tabs[0], tabs[1], tabs[2], None, None, 0, in_off=dev["in_off"], lens=dev["lens"])
        engine.sync()
        assert np.array_equal(to_host(buf), bt.plain())
        check_state(iv_d, pos_d, iv0, pos0, "nothing to do")
    finally:
        t.close()


def test_more_datagrams_than_the_walk_grid(engine, oracle):
    """300 000 HEARTBEATs of 8 bytes at stride 8, 16 connections: k_udp_walk's grid holds 4
    workgroups of 256 lanes per CU (262 144 on 256 CUs), so its grid-stride loop takes a second
    trip; so does k_udp_take's over the 300 000 (empty) segments.  A package chain's first
    block is plaintext ^ E_k(IV), so the wire bytes are built with numpy from one keystream per
    connection."""
    rng = np.random.default_rng(9)
    n, nconn = 300000, 16
    t = Tables(engine, rng, nconn, 16, 32)
    try:
        seq = np.arange(n, dtype=">u4")
        plain = np.zeros((n, 8), np.uint8)
        plain[:, 0], plain[:, 1], plain[:, 2], plain[:, 3] = 2, W.HEARTBEAT, rng.integers(0, 256, n), rng.integers(0, 256, n)
        plain[:, 4:] = seq.view(np.uint8).reshape(n, 4)
        first_dgram = np.linspace(0, n, nconn + 1).astype(np.int32)
        ks = np.stack([np.frombuffer(oracle.package(t.pkeys[s].tobytes(), t.pivs[s].tobytes(), True, bytes(8)), np.uint8)
                       for s in range(nconn)])
        wire = plain ^ np.repeat(ks, np.diff(first_dgram), axis=0)
        buf = to_dev(wire.reshape(-1))
        iv0, pos0 = initial_state(rng, nconn, np.arange(nconn))
        iv_d, pos_d = to_dev(iv0.reshape(-1)), to_dev(pos0.astype(np.int32))
        tabs = [to_dev(np.full((n * rows, words), TABLE_FILL * 0x01010101, np.uint32).view(np.int32))
                for rows, words in ((1, 2), (1, 4), (1, 4))]
        engine.udp_recv(buf, buf, n, t.pkg, t.data, nconn, i32(first_dgram), i32(np.arange(nconn)), nconn, iv_d, pos_d, 1, 1,
                        scan=tabs[0], pkgs=tabs[1], sections=tabs[2], stride=8, uniform_len=8)
        engine.sync()
        assert np.array_equal(to_host(buf).reshape(n, 8), plain)
        check_state(iv_d, pos_d, iv0, pos0, "no data section: the state keeps every bit")
        scan, pkgs, secs = (to_host(x).reshape(-1).view(dt) for x, dt in zip(tabs, (W.SCAN, W.PKG, W.SECTION)))
        e_scan = np.zeros(n, W.SCAN)
        e_scan["pkgs"], e_scan["sections"], e_scan["version"] = 1, 1, 2
        e_pkgs = np.zeros(n, W.PKG)
        e_pkgs["seq"], e_pkgs["type"], e_pkgs["flag"], e_pkgs["sign"] = np.arange(n), W.HEARTBEAT, plain[:, 2], plain[:, 3]
        e_pkgs["len"], e_pkgs["nsections"] = 8, 1
        e_secs = np.zeros(n, W.SECTION)
        e_secs["type"], e_secs["flag"], e_secs["off"] = W.HEARTBEAT, plain[:, 2], 8
        assert np.array_equal(scan, e_scan) and np.array_equal(pkgs, e_pkgs) and np.array_equal(secs, e_secs)
        w = W.Walk(plain[n - 1].tobytes(), 1, 1)  # (the vectorised rows are the restatement's)
        assert tuple(e_pkgs[n - 1]) == tuple(w.pkgs[0][f] for f in W.PKG.names)
        assert tuple(e_secs[n - 1]) == tuple(w.sections[0][f] for f in W.SECTION.names)
    finally:
        t.close()


# ---------------------------------------------------------------------------------------
# 8: contract breaches


def own_bytes(bt, conns):
    m = np.zeros(bt.total, bool)
    for j in conns:
        for i in range(bt.first_dgram[j], bt.first_dgram[j + 1]):
            m[bt.offs[i]:bt.offs[i] + bt.lens[i]] = True
    return m


@pytest.mark.parametrize("breach", ["first_take_not_monotone", "take_out_of_range", "take_of_another_connection",
                                    "take_of_an_unwalked_package"])
@pytest.mark.parametrize("pkg_len,data_len", PAIRS)
def test_take_breaches(engine, oracle, breach, pkg_len, data_len):
    """A broken take list: the connections it touches are invalid, all others are exact, the
    sentinel is intact, the next sync reports FPNN_AES_ERR_DEVICE once."""
    rng = np.random.default_rng(80 + pkg_len + 2 * data_len)
    bt = Batch(mixed_connections(rng, 12, 3), rng)
    t = Tables(engine, rng, 16, pkg_len, data_len)
    try:
        slots = rng.permutation(16)[:12]
        iv0, pos0 = initial_state(rng, 16, slots)
        buf = to_dev(bt.wire(oracle, t, slots))
        iv_d, pos_d = to_dev(iv0.reshape(-1)), to_dev(pos0.astype(np.int32))
        tabs = recv(engine, bt, t, slots, buf, buf, iv_d, pos_d, flags=WALK_ONLY)
        engine.sync()
        order = bt.all_packages()
        first, flat, ntake = take_lists(bt, order)
        if breach == "first_take_not_monotone":
            first[5] = first[4] - 1   # connection 4 gets an empty range, connection 5 reaches into 3's and 4's entries
            touched = (3, 4, 5)
        elif breach == "take_out_of_range":
            flat[first[5]] = bt.count * bt.max_pkgs + 5
            touched = (5,)
        elif breach == "take_of_another_connection":
            flat[first[5]] = flat[first[7]]
            touched = (5,)
        else:
            i = int(bt.first_dgram[5])
            flat[first[5]] = i * bt.max_pkgs + len(bt.walks[i].pkgs)  # one past the datagram's used rows
            touched = (5,)
        exp, iv1, pos1 = bt.plain(), iv0.copy(), pos0.copy()
        data_decrypt(oracle, bt, t, slots, exp, iv1, pos1, order, skip=touched)
        recv_take(engine, bt, t, slots, buf, iv_d, pos_d, tabs, first, flat, ntake)
        expect_device_error_once(engine)
        got, keep = to_host(buf), ~own_bytes(bt, touched)
        assert np.array_equal(got[keep], exp[keep]), np.flatnonzero(got[keep] != exp[keep])[:8]
        others = np.delete(np.arange(16), slots[list(touched)])
        assert np.array_equal(to_host(iv_d).reshape(-1, 16)[others], iv1[others])
        assert np.array_equal(to_host(pos_d).astype(np.uint32)[others], pos1[others])
    finally:
        t.close()


@pytest.mark.parametrize("flags", [0, PLAIN], ids=["recv", "plain"])
@pytest.mark.parametrize("pkg_len,data_len", PAIRS)
def test_slot_past_the_bound(engine, oracle, flags, pkg_len, data_len):
    """One conn_slot >= slot_bound: its state is untouched, its own bytes are unspecified, every
    other connection, the tables of the others and the sentinel are exact, ERR_DEVICE once."""
    rng = np.random.default_rng(810 + pkg_len + 2 * data_len)
    bt = Batch(mixed_connections(rng, 12, 3), rng)
    t = Tables(engine, rng, 16, pkg_len, data_len)
    try:
        slots = rng.permutation(14)[:12]
        bad = 4
        slots[bad] = 15
        iv0, pos0 = initial_state(rng, 16, np.delete(slots, bad))
        exp, iv1, pos1 = bt.plain(), iv0.copy(), pos0.copy()
        data_decrypt(oracle, bt, t, slots, exp, iv1, pos1, bt.all_packages(), skip=(bad,))
        buf = to_dev(bt.plain() if flags else bt.wire(oracle, t, slots))
        iv_d, pos_d = to_dev(iv0.reshape(-1)), to_dev(pos0.astype(np.int32))
        tabs = recv(engine, bt, t, slots, buf, buf, iv_d, pos_d, flags=flags, slot_bound=14)
        expect_device_error_once(engine)
        got, keep = to_host(buf), ~own_bytes(bt, (bad,))
        assert np.array_equal(got[keep], exp[keep]), np.flatnonzero(got[keep] != exp[keep])[:8]
        check_state(iv_d, pos_d, iv1, pos1, "state")
        if flags:  # (under PLAIN its datagrams are walked as they are: every table entry is exact)
            check_tables(bt, tabs)
    finally:
        t.close()


# ---------------------------------------------------------------------------------------
# 9: reserve


@pytest.mark.parametrize("pkg_len,data_len", PAIRS)
def test_reserve_covers_both_calls(oracle, pkg_len, data_len):
    """After reserve(max(count, nconn, count * max_sections), blocks) neither call grows the
    engine's scratch; an engine that never reserved does."""
    import fpnn_amd
    rng = np.random.default_rng(90 + pkg_len + 2 * data_len)
    bt = Batch(mixed_connections(rng, 150, 4), rng)
    order = bt.all_packages()
    first, flat, ntake = take_lists(bt, order)
    for reserved in (True, False):
        eng = fpnn_amd.Engine(0)
        t = Tables(eng, rng, 256, pkg_len, data_len)
        try:
            if reserved:
                eng.reserve(max(bt.count, bt.nconn, bt.count * bt.max_sections, ntake * bt.max_sections),
                            bt.total // 16 + bt.count)
            held = eng.scratch_bytes()
            slots = rng.permutation(256)[:150]
            single_call(eng, oracle, bt, t, slots, rng, inplace=True)
            single_call(eng, oracle, bt, t, slots, rng, inplace=False)
            iv0, pos0 = initial_state(rng, 256, slots)
            buf = to_dev(bt.wire(oracle, t, slots))
            iv_d, pos_d = to_dev(iv0.reshape(-1)), to_dev(pos0.astype(np.int32))
            tabs = recv(eng, bt, t, slots, buf, buf, iv_d, pos_d, flags=WALK_ONLY)
            recv_take(eng, bt, t, slots, buf, iv_d, pos_d, tabs, first, flat, ntake)
            eng.sync()
            exp, iv1, pos1 = bt.plain(), iv0.copy(), pos0.copy()
            data_decrypt(oracle, bt, t, slots, exp, iv1, pos1, order)
            assert np.array_equal(to_host(buf), exp)
            check_state(iv_d, pos_d, iv1, pos1, "take")
            assert eng.scratch_bytes() == held if reserved else eng.scratch_bytes() > held
        finally:
            eng.sync()
            t.close()
            eng.close()
