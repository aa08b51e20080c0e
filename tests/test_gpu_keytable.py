"""Accept and retire connections in a LIVE key table on the device: fpnn_aes_keyset_set_keys /
_clear (k_keytable.hip) and fpnn_ecdh_accept (ECDH kernel -> engine scratch -> k_set_keys ->
scratch wipe), all queued on the engine stream.

References: the host key expansion (fpnn_aes_setup_encrypt, pinned against the reference by
tests/test_abi.py) for every schedule read back; the oracle (oracle/aes_oracle.c) for every
byte ciphered through the table; tests/golden/ecdh_cases.json and ecdh_edge_cases.json (the
reference's own ECDH outputs) for fpnn_ecdh_accept.  Everything is bit-exact.

Run as a script (`python tests/test_gpu_keytable.py audit-child`) the module runs the new
calls once and prints "keytable ok"; the audit test starts it in a fresh process with
FPNN_AES_GPU_LIB naming the address-audit build of the GPU library.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))

from conftest import load_golden  # noqa: E402
from test_gpu_parity import to_dev, to_host  # noqa: E402

pytestmark = pytest.mark.gpu

AUDIT_LIB = os.path.join(ROOT, "fpnn_amd", "libfpnn_aes_gpu_audit.so")
CAP = 1024


class Mirror:
    """Host copy of what every slot of a table must hold: (key, iv) per slot."""

    def __init__(self, keylen, nslots):
        self.keylen = keylen
        self.keys = np.zeros((nslots, keylen), np.uint8)
        self.ivs = np.zeros((nslots, 16), np.uint8)
        self._sched = {}

    def grow(self, nslots):
        if nslots > len(self.keys):
            add = nslots - len(self.keys)
            self.keys = np.concatenate([self.keys, np.zeros((add, self.keylen), np.uint8)])
            self.ivs = np.concatenate([self.ivs, np.zeros((add, 16), np.uint8)])

    def put(self, slots, keys, ivs=None):
        slots = np.asarray(slots)
        self.grow(int(slots.max()) + 1)
        self.keys[slots] = keys
        self.ivs[slots] = 0 if ivs is None else ivs

    def schedule(self, slot):
        import fpnn_amd
        kb = self.keys[slot].tobytes()
        if kb not in self._sched:
            s = fpnn_amd.setup_encrypt(kb)
            self._sched[kb] = (s.nrounds, list(s.rk[:4 * (s.nrounds + 1)]))
        return self._sched[kb]

    def check_schedules(self, ks, slots, what):
        for s in slots:
            got = ks.schedule(int(s))
            nr, rk = self.schedule(int(s))
            assert got.nrounds == nr and list(got.rk[:len(rk)]) == rk, (what, int(s))


def preload(ks, mirror, rng, nslots):
    """Every slot of [0, nslots) written the old way (host schedules, fpnn_aes_keyset_set)."""
    keys = rng.integers(0, 256, (nslots, mirror.keylen), dtype=np.uint8)
    ivs = rng.integers(0, 256, (nslots, 16), dtype=np.uint8)
    ks.set(0, keys, ivs)
    mirror.put(np.arange(nslots), keys, ivs)


def parity(engine, oracle, ks, mirror, use_slots, rng, what, n=3000, decrypt=True):
    """The shape of test_keyset_writes_refresh_first_keystream_block: mostly 145-byte frames
    (whole waves take block 0 from eiv[]), plus 1, 15, 16, 17 and 1024 bytes; encrypt and
    decrypt through the table against the oracle under the mirror's keys."""
    use_slots = np.asarray(use_slots)
    lens = np.full(n, 145, np.int64)
    pick = rng.random(n) < 0.25
    lens[pick] = rng.choice(np.array([1, 15, 16, 17, 1024]), pick.sum())
    offs = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.int64)
    slots = use_slots[rng.integers(0, len(use_slots), n)].astype(np.int32)
    total = int(offs[-1] + lens[-1] + 16)
    inp = rng.integers(0, 256, total, dtype=np.uint8)
    okw = dict(in_off=offs.astype(np.uint64), lens=lens.astype(np.uint32), key_slot=slots.astype(np.uint32),
               keys=mirror.keys.reshape(-1).copy(), keylen=mirror.keylen, ivs=mirror.ivs.reshape(-1).copy(), threads=8)
    exp = inp.copy()
    oracle.package_batch(True, inp, exp, n, **okw)
    kw = dict(in_off=to_dev(offs), lens=to_dev(lens.astype(np.int32)), key_slot=to_dev(slots))
    src, dst = to_dev(inp), to_dev(inp)
    engine.package_encrypt(src, dst, n, ks, **kw)
    torch.cuda.synchronize()
    got = to_host(dst)
    assert np.array_equal(got, exp), (what, "encrypt")
    if decrypt:
        back = to_dev(got)
        engine.package_decrypt(dst, back, n, ks, **kw)
        torch.cuda.synchronize()
        assert np.array_equal(to_host(back), inp), (what, "decrypt")


def addressing(kind, count, rng):
    """(first, slots or None) for `count` entries in a CAP-slot table."""
    if kind == "contiguous":
        return 300, None
    if kind == "permutation":
        return 0, rng.permutation(CAP)[:count].astype(np.int32)
    return 0, (7 + 3 * np.arange(count) + (np.arange(count) % 2)).astype(np.int32)  # sparse: holes of 2 / 1 / 3 slots


@pytest.mark.parametrize("with_iv", [True, False], ids=["ivs", "null_ivs"])
@pytest.mark.parametrize("kind", ["contiguous", "permutation", "sparse"])
@pytest.mark.parametrize("keylen", [16, 24, 32])
def test_set_keys(engine, oracle, keylen, kind, with_iv):
    """1. Counts at the workgroup edge into a 1024-slot table, three ways of naming the
    slots, IVs present and NULL: every written slot's schedule equals the host expansion,
    the slots beside them (pre-loaded with fpnn_aes_keyset_set) read back unchanged, and
    frames cipher through the whole table as the oracle says (IV and E_k(IV) included)."""
    import fpnn_amd
    rng = np.random.default_rng(1000 * keylen + 10 * len(kind) + with_iv)
    ks = fpnn_amd.KeySet.reserve(engine, CAP, keylen)
    try:
        assert ks.capacity == CAP
        mirror = Mirror(keylen, CAP)
        preload(ks, mirror, rng, CAP)
        for count in (1, 255, 256, 257):
            first, slots = addressing(kind, count, rng)
            keys = rng.integers(0, 256, (count, keylen), dtype=np.uint8)
            ivs = rng.integers(0, 256, (count, 16), dtype=np.uint8) if with_iv else None
            ks.set_keys(to_dev(keys.reshape(-1)), None if ivs is None else to_dev(ivs.reshape(-1)), first=first,
                        slots=None if slots is None else to_dev(slots), slot_bound=None if slots is None else CAP)
            written = first + np.arange(count) if slots is None else slots
            mirror.put(written, keys, ivs)
            beside = np.setdiff1d(np.concatenate([written - 1, written + 1]), written)
            beside = beside[(beside >= 0) & (beside < CAP)]
            mirror.check_schedules(ks, written, ("written", count))
            mirror.check_schedules(ks, beside, ("beside", count))
            assert ks.capacity == CAP and lib_count(ks) == CAP
        parity(engine, oracle, ks, mirror, np.arange(CAP), rng, "after set_keys", n=1500, decrypt=False)
    finally:
        ks.close()


def lib_count(ks):
    import fpnn_amd
    return fpnn_amd.lib.fpnn_aes_keyset_count(ks.handle)


@pytest.mark.parametrize("keylen", [16, 24, 32])
def test_parity_through_the_table(engine, oracle, keylen):
    """2. Encrypt and decrypt against the oracle after set_keys, after rewriting two slots,
    after a grow past the capacity, and after clear plus re-set of a slot."""
    import fpnn_amd
    rng = np.random.default_rng(2200 + keylen)
    ks = fpnn_amd.KeySet.reserve(engine, 8, keylen)
    try:
        mirror = Mirror(keylen, 6)

        def put(slots, first=0):
            n = len(slots)
            keys = rng.integers(0, 256, (n, keylen), dtype=np.uint8)
            ivs = rng.integers(0, 256, (n, 16), dtype=np.uint8)
            contiguous = np.array_equal(slots, first + np.arange(n))
            ks.set_keys(to_dev(keys.reshape(-1)), to_dev(ivs.reshape(-1)), first=first,
                        slots=None if contiguous else to_dev(np.asarray(slots, np.int32)),
                        slot_bound=None if contiguous else ks.count)
            mirror.put(slots, keys, ivs)

        put(np.arange(6))
        assert (ks.capacity, lib_count(ks)) == (8, 6)
        parity(engine, oracle, ks, mirror, np.arange(6), rng, "after set_keys")
        put(np.array([4, 1]))
        parity(engine, oracle, ks, mirror, np.arange(6), rng, "two slots rewritten")
        put(6 + np.arange(6), first=6)  # 12 > 8: the table grows, contents kept
        assert ks.capacity >= 12 and lib_count(ks) == 12
        parity(engine, oracle, ks, mirror, np.arange(12), rng, "after the grow")
        ks.clear(slots=to_dev(np.array([3], np.int32)), slot_bound=12)
        put(np.array([3]), first=3)
        parity(engine, oracle, ks, mirror, np.arange(12), rng, "clear + re-set")
        mirror.check_schedules(ks, np.arange(12), "end")
    finally:
        ks.close()


def test_set_keys_on_a_created_key_set(engine, oracle):
    """The calls work on any key set: one made by fpnn_aes_keyset_create takes a rewrite of
    its slots in place and grows past its count."""
    import fpnn_amd
    rng = np.random.default_rng(77)
    keylen = 16
    k0, i0 = rng.integers(0, 256, (5, keylen), dtype=np.uint8), rng.integers(0, 256, (5, 16), dtype=np.uint8)
    ks = fpnn_amd.KeySet(engine, k0.tobytes(), keylen, i0.tobytes())
    try:
        mirror = Mirror(keylen, 5)
        mirror.put(np.arange(5), k0, i0)
        assert ks.capacity == 5
        k1, i1 = rng.integers(0, 256, (4, keylen), dtype=np.uint8), rng.integers(0, 256, (4, 16), dtype=np.uint8)
        ks.set_keys(to_dev(k1.reshape(-1)), to_dev(i1.reshape(-1)), first=3)  # slots 3..6: grows
        mirror.put(3 + np.arange(4), k1, i1)
        assert ks.capacity >= 7 and lib_count(ks) == 7
        parity(engine, oracle, ks, mirror, np.arange(7), rng, "created key set", n=800)
    finally:
        ks.close()


def test_ok_gating(engine, oracle):
    """3. ok[] of 0 and 1 mixed: slots with 0 keep their schedule and still cipher under the
    old key."""
    import fpnn_amd
    rng = np.random.default_rng(303)
    keylen, n = 32, 300
    ks = fpnn_amd.KeySet.reserve(engine, n, keylen)
    try:
        mirror = Mirror(keylen, n)
        preload(ks, mirror, rng, n)
        keys = rng.integers(0, 256, (n, keylen), dtype=np.uint8)
        ivs = rng.integers(0, 256, (n, 16), dtype=np.uint8)
        ok = (rng.random(n) < 0.5).astype(np.uint8)
        ok[:4] = (0, 1, 1, 0)
        ok[255:258] = (1, 0, 1)
        slots = rng.permutation(n).astype(np.int32)
        ks.set_keys(to_dev(keys.reshape(-1)), to_dev(ivs.reshape(-1)), slots=to_dev(slots), slot_bound=n, ok=to_dev(ok))
        yes = ok == 1
        assert 0 < yes.sum() < n
        mirror.put(slots[yes], keys[yes], ivs[yes])
        mirror.check_schedules(ks, np.arange(n), "ok gating")
        parity(engine, oracle, ks, mirror, np.arange(n), rng, "ok gating", n=1500)
    finally:
        ks.close()


def test_slot_bound(engine, oracle):
    """4. slot_bound = 512 in a 1024-slot table with one entry naming slot 700 (inside the
    allocation whatever the kernel does): that entry writes nothing, every other entry of
    the call is written, the next sync raises FPNN_AES_ERR_DEVICE once, and the engine works
    again afterwards."""
    import fpnn_amd
    rng = np.random.default_rng(404)
    keylen, n = 16, 300
    ks = fpnn_amd.KeySet.reserve(engine, CAP, keylen)
    try:
        mirror = Mirror(keylen, CAP)
        preload(ks, mirror, rng, CAP)
        engine.sync()
        keys = rng.integers(0, 256, (n, keylen), dtype=np.uint8)
        ivs = rng.integers(0, 256, (n, 16), dtype=np.uint8)
        slots = rng.permutation(512)[:n].astype(np.int32)
        slots[130] = 700
        ks.set_keys(to_dev(keys.reshape(-1)), to_dev(ivs.reshape(-1)), slots=to_dev(slots), slot_bound=512)
        with pytest.raises(fpnn_amd.FpnnAesError) as ei:
            engine.sync()
        assert ei.value.status == fpnn_amd.ERR_DEVICE and "slot" in str(ei.value)
        engine.sync()  # reported once
        inb = slots < 512
        assert inb.sum() == n - 1
        mirror.put(slots[inb], keys[inb], ivs[inb])
        mirror.check_schedules(ks, np.arange(CAP), "bound")  # slot 700 and every untouched slot: the old key
        # the engine works again: a well-formed write and frames through the whole table
        k2, i2 = rng.integers(0, 256, (3, keylen), dtype=np.uint8), rng.integers(0, 256, (3, 16), dtype=np.uint8)
        ks.set_keys(to_dev(k2.reshape(-1)), to_dev(i2.reshape(-1)), first=699)
        mirror.put(699 + np.arange(3), k2, i2)
        parity(engine, oracle, ks, mirror, np.arange(CAP), rng, "after the reported error", n=1500)
        engine.sync()
    finally:
        ks.close()


@pytest.mark.parametrize("keylen", [16, 24, 32])
def test_clear(engine, keylen):
    """5. A cleared slot equals a never-set one: by fpnn_aes_keyset_get_schedule, and by the
    bytes frames cipher to through it and through a fresh slot."""
    import fpnn_amd
    rng = np.random.default_rng(505 + keylen)
    ks = fpnn_amd.KeySet.reserve(engine, 16, keylen)
    try:
        keys = rng.integers(0, 256, (8, keylen), dtype=np.uint8)
        ivs = rng.integers(0, 256, (8, 16), dtype=np.uint8)
        ks.set_keys(to_dev(keys.reshape(-1)), to_dev(ivs.reshape(-1)))  # slots 0..7
        ks.set_keys(to_dev(keys[:1].reshape(-1)), to_dev(ivs[:1].reshape(-1)), first=15)  # count 16; 8..14 never set
        ks.clear(slots=to_dev(np.array([5, 2], np.int32)), slot_bound=8)
        ks.clear(first=6, count=1)
        fresh = bytes(ks.schedule(12))
        for s in (2, 5, 6):
            assert bytes(ks.schedule(s)) == fresh, s
        assert bytes(ks.schedule(3)) != fresh and bytes(ks.schedule(7)) != fresh
        n, L = 640, 145  # whole waves on one slot: block 0 from eiv[]
        lens = np.full(n, L, np.int32)
        lens[::9] = 17
        lens[::13] = 1
        offs = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.int64)
        inp = rng.integers(0, 256, int(offs[-1] + lens[-1]), dtype=np.uint8)
        outs = {}
        for s in (2, 5, 6, 12, 3):
            dst = to_dev(inp)
            engine.package_encrypt(to_dev(inp), dst, n, ks, in_off=to_dev(offs), lens=to_dev(lens),
                                   key_slot=to_dev(np.full(n, s, np.int32)))
            torch.cuda.synchronize()
            outs[s] = to_host(dst)
        for s in (2, 5, 6):
            assert np.array_equal(outs[s], outs[12]), s
        assert not np.array_equal(outs[3], outs[12]) and not np.array_equal(outs[12], inp)
    finally:
        ks.close()


# ---- fpnn_ecdh_accept -------------------------------------------------------------------

def accept_rows(curve, keylen):
    """Fixture rows of one curve and key length whose lengths the reference accepts, grouped
    by server private key (one fpnn_ecdh_accept call each); an all-zero peer, which the
    oracle rejects, is added where the rows hold no refused derivation."""
    import ecdh_oracle as E
    c = E.CURVES[curve]
    rows = []
    for name in ("ecdh_cases.json", "ecdh_edge_cases.json"):
        for cv in load_golden(name)["curves"]:
            if cv["curve"] != curve:
                continue
            for s in cv["server"]:
                if len(s["private"]) // 2 == c.private_bytes and len(s["peer"]) // 2 == 2 * c.num_bytes \
                        and s["keylen"] == keylen:
                    rows.append(s)
    assert rows
    if not any(s["ok"] == 0 for s in rows):
        zero = bytes(2 * c.num_bytes)
        eok, _, _ = E.calc_key(curve, bytes.fromhex(rows[0]["private"]), zero, keylen)
        assert not eok
        rows.append(dict(private=rows[0]["private"], peer=zero.hex(), keylen=keylen, ok=0, key="", iv=""))
    return rows


@pytest.mark.parametrize("keylen", [16, 32])
@pytest.mark.parametrize("curve", ["secp256k1", "secp256r1", "secp224r1", "secp192r1"])
def test_accept_rows_hold_a_refused_derivation(curve, keylen):
    rows = accept_rows(curve, keylen)
    assert any(s["ok"] == 0 for s in rows) and any(s["ok"] == 1 for s in rows)


@pytest.mark.parametrize("keylen", [16, 32])
@pytest.mark.parametrize("curve", ["secp256k1", "secp256r1", "secp224r1", "secp192r1"])
def test_ecdh_accept_against_the_reference(engine, oracle, curve, keylen):
    """6. Every fixture row, permuted over the slots of a pre-loaded table: the returned ok
    equals the fixture's, slots with ok == 1 cipher exactly as oracle.package(key, iv, ...)
    with the fixture's key and IV, slots with ok == 0 keep their earlier key."""
    import fpnn_amd
    rng = np.random.default_rng(606 + keylen + len(curve))
    rows = accept_rows(curve, keylen)
    nslots = 512
    ks = fpnn_amd.KeySet.reserve(engine, nslots, keylen)
    try:
        mirror = Mirror(keylen, nslots)
        preload(ks, mirror, rng, nslots)
        slot_of_row = rng.permutation(nslots)[:len(rows)].astype(np.int32)
        groups = {}
        for i, s in enumerate(rows):
            groups.setdefault(s["private"], []).append(i)
        oks = {}
        for priv, idx in groups.items():
            peers = to_dev(np.frombuffer(b"".join(bytes.fromhex(rows[i]["peer"]) for i in idx), np.uint8))
            oks[priv] = engine.ecdh_accept(curve, bytes.fromhex(priv), peers, ks, slots=to_dev(slot_of_row[idx]),
                                           slot_bound=nslots)
        engine.sync()
        for priv, idx in groups.items():
            assert list(to_host(oks[priv])[:len(idx)]) == [rows[i]["ok"] for i in idx], (curve, priv)
        # one frame batch over every row's slot
        lens = np.array([(145, 145, 17, 1, 16, 1024, 145, 15)[i % 8] for i in range(len(rows))], np.int32)
        offs = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.int64)
        inp = rng.integers(0, 256, int(offs[-1] + lens[-1]), dtype=np.uint8)
        dst = to_dev(inp)
        engine.package_encrypt(to_dev(inp), dst, len(rows), ks, in_off=to_dev(offs), lens=to_dev(lens),
                               key_slot=to_dev(slot_of_row))
        torch.cuda.synchronize()
        got = to_host(dst)
        for i, s in enumerate(rows):
            sl = int(slot_of_row[i])
            if s["ok"]:
                key, iv = bytes.fromhex(s["key"]), bytes.fromhex(s["iv"])
            else:
                key, iv = mirror.keys[sl].tobytes(), mirror.ivs[sl].tobytes()
            o, n = int(offs[i]), int(lens[i])
            assert got[o:o + n].tobytes() == oracle.package(key, iv, True, inp[o:o + n].tobytes()), (curve, i, s["ok"])
        assert lib_count(ks) == nslots and ks.capacity == nslots
    finally:
        ks.close()


def test_ecdh_accept_argument_checks(engine):
    import fpnn_amd
    lib = fpnn_amd.lib
    peers = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
    ks24 = fpnn_amd.KeySet.reserve(engine, 4, 24)
    ks16 = fpnn_amd.KeySet.reserve(engine, 4, 16)
    try:
        p = C.c_void_p(peers.data_ptr())
        assert lib.fpnn_ecdh_accept(engine.handle, 0, bytes(32), p, 1, ks24.handle, 0, None, 0, None) == fpnn_amd.ERR_KEYLEN
        assert lib.fpnn_ecdh_accept(engine.handle, 0, bytes(32), None, 1, ks16.handle, 0, None, 0, None) == fpnn_amd.ERR_ARG
        assert lib.fpnn_ecdh_accept(engine.handle, 99, bytes(32), p, 1, ks16.handle, 0, None, 0, None) == fpnn_amd.ERR_ARG
        assert lib.fpnn_ecdh_accept(engine.handle, 0, bytes(32), p, 0, ks16.handle, 0, None, 0, None) == fpnn_amd.OK
        assert lib.fpnn_aes_keyset_set_keys(ks16.handle, 0, 1, None, 0, None, None, None) == fpnn_amd.ERR_ARG
        assert lib.fpnn_aes_keyset_set_keys(ks16.handle, 0xffffffff, 2, None, 0, p, None, None) == fpnn_amd.ERR_RANGE
        assert lib_count(ks16) == 0 and ks16.capacity == 4
    finally:
        ks24.close()
        ks16.close()
        engine.sync()


def test_graph_replay(oracle):
    """7. After reserve: ecdh_accept followed by package_encrypt captured as one chain and
    replayed twice with different peers in the same arrays; parity each time."""
    import ecdh_oracle as E
    import fpnn_amd
    curve, keylen, n, L = "secp256k1", 32, 300, 145
    side = torch.cuda.Stream()
    eng = fpnn_amd.Engine(0, stream=side)
    ks = None
    try:
        rng = np.random.default_rng(707)
        server = bytes(rng.integers(1, 255, 32, dtype=np.uint8))
        ks = fpnn_amd.KeySet.reserve(eng, n, keylen)
        eng.reserve(n, n * 16)
        peers_d = torch.zeros(n * 64, dtype=torch.uint8, device="cuda:0")
        ok_d = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
        slots_d = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        src = torch.zeros(n * L, dtype=torch.uint8, device="cuda:0")
        dst = torch.zeros(n * L, dtype=torch.uint8, device="cuda:0")
        frame_slot = torch.arange(n, dtype=torch.int32, device="cuda:0")

        def load(seed):
            r = np.random.default_rng(seed)
            privs = r.integers(0, 256, (n, 32), dtype=np.uint8)
            privs[:, 0] &= 0x7F
            with torch.cuda.stream(side):
                pub, pok = eng.ecdh_public_keys(curve, torch.from_numpy(privs).to("cuda:0"))
            side.synchronize()
            assert bool(pok.all())
            pp = pub.cpu().numpy().copy()
            pp[5] = 0  # a refused peer: slot keeps what it held
            slots = r.permutation(n).astype(np.int32)
            data = r.integers(0, 256, n * L, dtype=np.uint8)
            with torch.cuda.stream(side):
                peers_d.copy_(torch.from_numpy(pp.reshape(-1)))
                slots_d.copy_(torch.from_numpy(slots))
                src.copy_(torch.from_numpy(data))
                dst.zero_()
            return pp, slots, data

        def run():
            eng.ecdh_accept(curve, server, peers_d, ks, slots=slots_d, slot_bound=n, ok=ok_d, count=n)
            eng.package_encrypt(src, dst, n, ks, stride=L, uniform_len=L, key_slot=frame_slot)

        held = {}  # slot -> (key, iv) as the table must hold it (None: never set)

        def check(loaded, what):
            pp, slots, data = loaded
            side.synchronize()
            out, ok = dst.cpu().numpy(), ok_d.cpu().numpy()
            for i in range(n):
                eok, ek, ei = E.calc_key(curve, server, pp[i].tobytes(), keylen)
                assert bool(ok[i]) == eok, (what, i)
                if eok:
                    held[int(slots[i])] = (ek, ei)
            assert not ok[5]
            for s in list(range(0, n, 23)) + [int(slots[5])]:
                if s in held:
                    exp = oracle.package(held[s][0], held[s][1], True, data[s * L:(s + 1) * L].tobytes())
                    assert out[s * L:(s + 1) * L].tobytes() == exp, (what, s)

        loaded = load(1)  # an ordinary call first (code objects loaded, scratch at its final size)
        with torch.cuda.stream(side):
            run()
        check(loaded, "ordinary")
        load(2)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side, capture_error_mode="relaxed"):
            run()
        for seed in (3, 4):  # capture does not execute: two replays, each on new peers
            loaded = load(seed)
            with torch.cuda.stream(side):
                g.replay()
            check(loaded, f"replay {seed}")
        eng.sync()
        del g
    finally:
        eng.sync()
        if ks is not None:
            ks.close()
        eng.close()


def test_scratch_is_not_re_exposed_by_an_empty_call(engine):
    """8. After ecdh_accept and a sync, a call with count = 0 is a no-op that returns OK and
    leaves table and ok array alone.  (The engine has no read-back of its ECDH scratch, so
    the wipe itself is covered by reading the code: fpnn_ecdh_accept queues ecdh_wipe behind
    k_set_keys.)"""
    import fpnn_amd
    rng = np.random.default_rng(808)
    ks = fpnn_amd.KeySet.reserve(engine, 8, 16)
    try:
        privs = rng.integers(0, 256, (4, 32), dtype=np.uint8)
        privs[:, 0] &= 0x7F
        pub, _ = engine.ecdh_public_keys("secp256k1", to_dev(privs))
        server = bytes(rng.integers(1, 255, 32, dtype=np.uint8))
        ok = engine.ecdh_accept("secp256k1", server, pub, ks)
        engine.sync()
        before = [bytes(ks.schedule(s)) for s in range(4)]
        assert list(to_host(ok)[:4]) == [1, 1, 1, 1]
        ok2 = torch.full((4,), 7, dtype=torch.uint8, device="cuda:0")
        engine.ecdh_accept("secp256k1", server, pub, ks, ok=ok2, count=0)
        engine.sync()
        assert list(to_host(ok2)) == [7, 7, 7, 7]
        assert [bytes(ks.schedule(s)) for s in range(4)] == before and lib_count(ks) == 4
    finally:
        ks.close()


# ---- the address-audit build ----------------------------------------------------------------

def test_audit_library():
    """9. The new calls through the address-audit build of the GPU library, in a fresh
    process: FPNN_AES_OK (no access of k_set_keys / k_clear_slots outside its extent) and
    bit-exact."""
    assert os.path.exists(AUDIT_LIB), "make -C fpnn_amd/csrc audit"
    env = dict(os.environ)
    env["FPNN_AES_GPU_LIB"] = AUDIT_LIB
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "audit-child"], capture_output=True, text=True,
                         timeout=240, env=env)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "keytable ok" in res.stdout and "address audit" not in res.stderr


def _audit_child():
    import fpnn_amd
    from pyoracle import Oracle
    assert os.environ.get("FPNN_AES_GPU_LIB", "").endswith("libfpnn_aes_gpu_audit.so")
    eng = fpnn_amd.Engine(0)
    oracle = Oracle("port")
    rng = np.random.default_rng(909)
    for keylen in (16, 24, 32):
        ks = fpnn_amd.KeySet.reserve(eng, CAP, keylen)
        mirror = Mirror(keylen, CAP)
        preload(ks, mirror, rng, CAP)
        for kind in ("contiguous", "permutation", "sparse"):
            first, slots = addressing(kind, 257, rng)
            keys = rng.integers(0, 256, (257, keylen), dtype=np.uint8)
            ivs = rng.integers(0, 256, (257, 16), dtype=np.uint8)
            ok = np.ones(257, np.uint8)
            ok[100] = 0
            ks.set_keys(to_dev(keys.reshape(-1)), to_dev(ivs.reshape(-1)), first=first,
                        slots=None if slots is None else to_dev(slots), slot_bound=None if slots is None else CAP,
                        ok=to_dev(ok))
            written = first + np.arange(257) if slots is None else slots
            mirror.put(written[ok == 1], keys[ok == 1], ivs[ok == 1])
        k2 = rng.integers(0, 256, (CAP, keylen), dtype=np.uint8)
        ks.set_keys(to_dev(k2.reshape(-1)), None, first=CAP)  # grows: the last slot of the new table
        mirror.put(CAP + np.arange(CAP), k2)
        ks.clear(first=2 * CAP - 1, count=1)
        ks.set_keys(to_dev(k2[:1].reshape(-1)), None, first=2 * CAP - 1)
        mirror.put(np.array([2 * CAP - 1]), k2[:1])
        parity(eng, oracle, ks, mirror, np.arange(2 * CAP), rng, "audit", n=1000)
        ks.close()
    rows = accept_rows("secp256k1", 32)
    priv = rows[-1]["private"]
    grp = [s for s in rows if s["private"] == priv]
    ks = fpnn_amd.KeySet.reserve(eng, 64, 32)
    peers = to_dev(np.frombuffer(b"".join(bytes.fromhex(s["peer"]) for s in grp), np.uint8))
    ok = eng.ecdh_accept("secp256k1", bytes.fromhex(priv), peers, ks, first=64 - len(grp))
    eng.sync()
    assert list(to_host(ok)[:len(grp)]) == [s["ok"] for s in grp]
    ks.close()
    eng.close()
    print("keytable ok")


if __name__ == "__main__":
    if sys.argv[1:] == ["audit-child"]:
        _audit_child()
