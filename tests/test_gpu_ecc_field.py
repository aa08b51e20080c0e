"""The device field and point arithmetic of the ECDH key derivation (fpnn_amd/csrc/ecc_field.hpp),
run function by function through the probe library (k_ecdh_probe.hip, libfpnn_ecc_probe.so) and
compared exactly with Python big integers -- on the structured operands of tests/ecc_vectors.py,
which take the folds' rare branches (tests/test_field_folds.py asserts which), on all-carry
operands, and in launches of 256 Ki lanes so that several waves per SIMD run the asm carry
chains at once.  Then the edges of the real entry points: lanes past the count, and the
reference's answers for edge scalars and peers (tests/golden/ecdh_edge_cases.json) through
all three device routes.

The whole-ladder tests on random inputs are tests/test_gpu_ecdh.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ecdh_oracle as E  # noqa: E402
import ecc_vectors as V  # noqa: E402

PROBE_LIB = os.path.join(ROOT, "fpnn_amd", "libfpnn_ecc_probe.so")
CURVE_ID = {"secp256k1": 0, "secp256r1": 1, "secp224r1": 2, "secp192r1": 3}  # ecc.hpp ECC_*
# lanes of a field-op launch (vectors repeated to fill it): 4 096 waves, 4 for each of the
# 1 024 SIMDs, so that every SIMD interleaves several waves' carry chains
LANES = 1 << 18
PAD_ROWS = 8        # canary rows behind every output
CANARY = 0xA5
# k_ecdh_probe.hip: op -> (code, a row, b row, out row) in field elements; "t"/"T": 1 / 2*NW limbs
OPS = {
    "MUL": (0, "e", "e", "e"), "SQR": (1, "e", "", "e"),
    "DUAL_MM": (2, "ee", "ee", "ee"), "DUAL_MS": (3, "ee", "ee", "ee"), "DUAL_SM": (4, "ee", "ee", "ee"),
    "DUAL_SS": (5, "ee", "ee", "ee"), "DUAL_SS_ALIAS": (6, "ee", "", "ee"), "DUAL_MM_ALIAS": (7, "ee", "e", "ee"),
    "ADD": (8, "e", "e", "e"), "SUB": (9, "e", "e", "e"), "HALF": (10, "e", "", "e"), "REDUCE": (11, "et", "", "e"),
    "INV": (12, "e", "", "e"), "FOLD": (13, "T", "", "e"), "DBL": (14, "eee", "", "eee"),
    "APPLYZ": (15, "ee", "e", "ee"), "XYCZ_ADD": (16, "eeee", "", "eeee"), "XYCZ_ADDC": (17, "eeee", "", "eeee"),
}


def _sizes(spec, nw):
    return [{"e": nw, "t": 1, "T": 2 * nw}[ch] for ch in spec]


def _pack(rows, sizes):
    """rows of integers -> uint32 [n, sum(sizes)], each integer as sizes[k] little-endian limbs"""
    buf = b"".join(int(v).to_bytes(4 * sz, "little") for row in rows for v, sz in zip(row, sizes))
    return np.frombuffer(buf, dtype=np.uint32).reshape(len(rows), sum(sizes))


def _unpack_row(row, sizes):
    out, at = [], 0
    for sz in sizes:
        out.append(V.value(row[at:at + sz]))
        at += sz
    return out


@pytest.fixture(scope="module")
def probe(engine):
    """fpnn_ecc_probe of libfpnn_ecc_probe.so (built by fpnn_amd/csrc/Makefile's `all`)."""
    assert os.path.exists(PROBE_LIB), "fpnn_amd/libfpnn_ecc_probe.so missing: run __graft_entry__.build()"
    fn = C.CDLL(PROBE_LIB).fpnn_ecc_probe
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return fn


def _dev_u32(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).to(DEV)


def run_op(probe, curve, op, a_rows, b_rows=None, lanes=0, n=None):
    """Run `op` on the rows (repeated cyclically up to `lanes` lanes) -> (uint32 [n, out limbs],
    row index of every lane).  The output buffer carries PAD_ROWS canary rows, checked here."""
    nw = V.NW[curve]
    code, sa, sb, so = OPS[op]
    a = _pack(a_rows, _sizes(sa, nw))
    idx = np.arange(max(lanes, len(a))) % len(a)
    if n is not None:
        idx = idx[:n]
    n = len(idx)
    da = _dev_u32(a[idx])
    db = None
    if sb:
        b = _pack(b_rows, _sizes(sb, nw))
        assert len(b) == len(a)
        db = _dev_u32(b[idx])
    ow = sum(_sizes(so, nw))
    out = torch.full(((n + PAD_ROWS) * ow * 4,), CANARY, dtype=torch.uint8, device=DEV)
    rc = probe(CURVE_ID[curve], code, n, da.data_ptr(), db.data_ptr() if db is not None else None, out.data_ptr(), None)
    assert rc == 0, (curve, op, rc)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[n * ow * 4:] == CANARY).all(), f"{curve} {op}: bytes past row {n} written"
    return o[:n * ow * 4].view(np.uint32).reshape(n, ow), idx


def check_op(probe, curve, op, a_rows, b_rows, exp_rows, lanes=LANES):
    """Every lane's result equals exp_rows[its row] exactly; returns the device results."""
    nw = V.NW[curve]
    got, idx = run_op(probe, curve, op, a_rows, b_rows, lanes)
    so = _sizes(OPS[op][3], nw)
    exp = _pack(exp_rows, so)[idx]
    if not np.array_equal(got, exp):
        lane = int(np.nonzero((got != exp).any(axis=1))[0][0])
        r = int(idx[lane])
        nbad = int((got != exp).any(axis=1).sum())
        pytest.fail(f"{curve} {op}: {nbad} of {len(idx)} lanes differ; first lane {lane} (row {r}): "
                    f"a = {[hex(v) for v in a_rows[r]]}, b = {[hex(v) for v in b_rows[r]] if b_rows else None}, "
                    f"got {[hex(v) for v in _unpack_row(got[lane], so)]}, want {[hex(v) for v in exp_rows[r]]}")
    return got


def _pairs(curve):
    """Operand pairs (a, b < p): the structured pairs, 4 096 random pairs, all-carry operands
    with one another."""
    ac = V.all_carry(curve)
    ra, rb = V.random_below(curve, 4096, "a"), V.random_below(curve, 4096, "b")
    pairs = list(V.product_pairs(curve)) + list(zip(ra, rb)) + [(a, b) for a in ac for b in ac]
    assert len(pairs) <= LANES
    return pairs


@pytest.mark.parametrize("curve", V.CURVES)
def test_mul_sqr(probe, curve):
    """fmul and fsqr (product scan + sqr_finish + fold): a * b and a^2 mod p; SQR(a) = MUL(a, a)."""
    p = V.P[curve]
    pairs = _pairs(curve)
    check_op(probe, curve, "MUL", [(a,) for a, _ in pairs], [(b,) for _, b in pairs], [(a * b % p,) for a, b in pairs])
    sq = sorted(set(V.operands(curve)) | set(V.all_carry(curve)) | set(V.random_below(curve, 4096, "sq")))
    rows = [(a,) for a in sq]
    exp = [(a * a % p,) for a in sq]
    m = check_op(probe, curve, "MUL", rows, rows, exp)
    s = check_op(probe, curve, "SQR", rows, None, exp)
    assert np.array_equal(m, s)


@pytest.mark.parametrize("curve", V.CURVES)
def test_dual(probe, curve):
    """fdual in its four SQ1 / SQ2 forms and with the argument aliasing of xycz_add /
    xycz_addc: each half equals the single fmul / fsqr on the device, and the big-integer value."""
    p = V.P[curve]
    h1 = _pairs(curve)
    h2 = h1[7919:] + h1[:7919]  # the second product of a row: another pair
    a_rows = [(x[0], y[0]) for x, y in zip(h1, h2)]
    b_rows = [(x[1], y[1]) for x, y in zip(h1, h2)]
    single = {}
    for half, h in ((0, h1), (1, h2)):
        single[half, False] = check_op(probe, curve, "MUL", [(a,) for a, _ in h], [(b,) for _, b in h],
                                       [(a * b % p,) for a, b in h])
        single[half, True] = check_op(probe, curve, "SQR", [(a,) for a, _ in h], None, [(a * a % p,) for a, _ in h])
    for op, sq1, sq2 in (("DUAL_MM", False, False), ("DUAL_MS", False, True), ("DUAL_SM", True, False),
                         ("DUAL_SS", True, True), ("DUAL_SS_ALIAS", True, True)):
        exp = [((a1 * a1 if sq1 else a1 * b1) % p, (a2 * a2 if sq2 else a2 * b2) % p)
               for (a1, a2), (b1, b2) in zip(a_rows, b_rows)]
        got = check_op(probe, curve, op, a_rows, b_rows if OPS[op][2] else None, exp)
        assert np.array_equal(got, np.hstack([single[0, sq1], single[1, sq2]])), (curve, op)
    # fdual(X1, X1, t5, X2, X2, t5): both products share the second operand
    b1_rows = [(b1,) for b1, _ in b_rows]
    exp = [(a1 * b1 % p, a2 * b1 % p) for (a1, a2), (b1,) in zip(a_rows, b1_rows)]
    got = check_op(probe, curve, "DUAL_MM_ALIAS", a_rows, b1_rows, exp)
    assert np.array_equal(got[:, :V.NW[curve]], single[0, False])


@pytest.mark.parametrize("curve", V.CURVES)
def test_fold(probe, curve):
    """fold_nf on raw 2*NW-limb words t < p^2 (extreme limbs) and on the products' words."""
    p = V.P[curve]
    ts = [V.value(w) for w in V.raw_words(curve)] + [a * b for a, b in _pairs(curve)]
    ts += [(p - 1) ** 2, (p - 1) * (p - 2), 0, 1, p, p - 1, p * p - 1]
    assert max(ts) < p * p and len(ts) <= LANES
    check_op(probe, curve, "FOLD", [(t,) for t in ts], None, [(t % p,) for t in ts])


def _addsub_pairs(curve):
    p, top = V.P[curve], 1 << (32 * V.NW[curve])
    ops, ac = V.operands(curve), V.all_carry(curve)
    pairs = list(V.product_pairs(curve)) + [(a, b) for a in ac for b in ac]
    pairs += [(0, b) for b in ops[::7]] + [(a, 0) for a in ops[::7]] + [(a, a) for a in ops] + [(a, p - 1) for a in ops]
    d = top - p
    for x in (1, 2, d - 1, d, d + 1, p >> 1, (p >> 1) + 1, p - 2, p - 1):
        for s in (p - 1, p, p + 1, top - 1, top, top + 1, 2 * p - 2):  # sums around p and 2^bits
            if 0 <= s - x < p:
                pairs.append((x, s - x))
    sums = [a + b for a, b in pairs]
    for cls in (lambda s: s < p, lambda s: s == p, lambda s: p < s < top, lambda s: s == top, lambda s: s > top):
        assert any(cls(s) for s in sums)
    assert any(a == b for a, b in pairs) and any(a < b for a, b in pairs) and any(a > b for a, b in pairs)
    assert len(pairs) <= LANES
    return pairs


@pytest.mark.parametrize("curve", V.CURVES)
def test_add_sub_half_reduce(probe, curve):
    """fadd, fsub, fhalf, reduce_once: sums below p, in [p, 2^bits) and from 2^bits up, a = b,
    a = 0, b = p - 1; halves of even and odd values, with and without a carry out of a + p;
    reduce_once over [0, 2p) as (t, top)."""
    p, nw = V.P[curve], V.NW[curve]
    top = 1 << (32 * nw)
    pairs = _addsub_pairs(curve)
    a_rows, b_rows = [(a,) for a, _ in pairs], [(b,) for _, b in pairs]
    check_op(probe, curve, "ADD", a_rows, b_rows, [((a + b) % p,) for a, b in pairs])
    check_op(probe, curve, "SUB", a_rows, b_rows, [((a - b) % p,) for a, b in pairs])
    hs = sorted(set(V.operands(curve)) | set(V.all_carry(curve)) | set(V.random_below(curve, 4096, "half"))
                | {0, 1, 2, p - 1, p - 2, top - p, top - p + 1, top - p - 1})
    assert all(0 <= a < p for a in hs)
    assert any(a & 1 and a + p >= top for a in hs) and any(a & 1 and a + p < top for a in hs)
    assert any(not a & 1 for a in hs)
    check_op(probe, curve, "HALF", [(a,) for a in hs], None, [(a * ((p + 1) // 2) % p,) for a in hs])
    rng_v = V.random_below(curve, 4096, "reduce")
    vs = list(V.operands(curve)) + [x + p for x in V.operands(curve)] + rng_v + [x + p for x in rng_v]
    vs += [v for v in (0, p - 1, p, p + 1, top - 1, top, top + 1, 2 * p - 2, 2 * p - 1) if v < 2 * p]
    assert any(p <= v < top for v in vs) and any(v >= top for v in vs) and max(vs) < 2 * p
    check_op(probe, curve, "REDUCE", [(v % top, v >> (32 * nw)) for v in vs], None, [(v % p,) for v in vs])


@pytest.mark.parametrize("curve", V.CURVES)
def test_inv(probe, curve):
    """finv: the inversion chain against pow(a, p - 2, p); 0 gives 0."""
    p = V.P[curve]
    vals = [0, 1, 2, p - 1, p - 2] + V.random_below(curve, 64, "inv")
    check_op(probe, curve, "INV", [(a,) for a in vals], None, [(pow(a, p - 2, p),) for a in vals], lanes=0)


def _coz_inputs(curve):
    """(X1, Y1, X2, Y2): random, and the degenerate co-Z pairs a ladder meets at infinity."""
    p = V.P[curve]
    r = V.random_below(curve, 4 * 1024, "coz")
    rows = [tuple(r[i:i + 4]) for i in range(0, len(r), 4)]
    deg = []
    for x1, y1, x2, y2 in rows[:8]:
        deg += [(x1, y1, x1, y2), (x1, y1, x2, y1), (x1, y1, x2, p - y1), (x1, y1, x1, y1), (x1, y1, x1, p - y1),
                (0, y1, x2, y2), (x1, 0, x2, y2), (x1, y1, 0, y2), (x1, y1, x2, 0), (0, 0, x2, y2), (x1, y1, 0, 0),
                (x1, 0, x1, 0), (0, y1, 0, y2), (p - 1, y1, 1, y2)]
    return rows + deg + [(0, 0, 0, 0), (1, 1, 1, 1), (p - 1, p - 1, p - 1, p - 1)]


@pytest.mark.parametrize("curve", V.CURVES)
def test_point_formulas(probe, curve):
    """dbl_jacobian, apply_z, xycz_add, xycz_addc against the oracle's _double_jacobian,
    _apply_z, _add, _add_c: random inputs and the degenerate ones."""
    c, p = E.CURVES[curve], V.P[curve]
    assert c.p == p
    r = V.random_below(curve, 3 * 1024, "dbl")
    rows = [tuple(r[i:i + 3]) for i in range(0, len(r), 3)]
    x, y, z = rows[0]
    rows += [(x, y, 1), (x, 0, z), (0, y, z), (0, 0, z), (x, y, p - 1), (p - 1, p - 1, p - 1), (1, 1, 1), (x, p - y, z)]
    assert all(row[2] != 0 for row in rows)  # (z = 0 is the caller's case: EccPoint_mult starts from z = 1)
    check_op(probe, curve, "DBL", rows, None, [E._double_jacobian(c, *row) for row in rows], lanes=0)
    rows += [(x, y, 0), (0, 0, 0)]
    check_op(probe, curve, "APPLYZ", [row[:2] for row in rows], [row[2:] for row in rows],
             [E._apply_z(p, *row) for row in rows], lanes=0)
    coz = _coz_inputs(curve)
    check_op(probe, curve, "XYCZ_ADD", coz, None, [E._add(p, *row) for row in coz], lanes=0)
    check_op(probe, curve, "XYCZ_ADDC", coz, None, [E._add_c(p, *row) for row in coz], lanes=0)


COUNTS = (1, 63, 64, 65, 255, 256, 257)


@pytest.mark.parametrize("curve", V.CURVES)
def test_probe_lanes_past_count(probe, curve):
    """The probe kernel with counts around the wave and block sizes: rows below n right, bytes
    past n rows untouched (run_op checks the canary rows)."""
    p = V.P[curve]
    pairs = _pairs(curve)[:257]
    coz = _coz_inputs(curve)[:257]
    for n in COUNTS:
        got, _ = run_op(probe, curve, "MUL", [(a,) for a, _ in pairs], [(b,) for _, b in pairs], n=n)
        assert np.array_equal(got, _pack([(a * b % p,) for a, b in pairs[:n]], [V.NW[curve]]))
        got, _ = run_op(probe, curve, "XYCZ_ADDC", coz, None, n=n)
        assert np.array_equal(got, _pack([E._add_c(p, *row) for row in coz[:n]], [V.NW[curve]] * 4))


def _canary(rows, width):
    return torch.full((rows + PAD_ROWS, width), CANARY, dtype=torch.uint8, device=DEV)


def _tail_clean(t, n):
    return bool((t[n:] == CANARY).all())


@pytest.mark.parametrize("curve", V.CURVES)
def test_batch_entry_points_lanes_past_count(engine, curve):
    """fpnn_ecdh_public_keys, fpnn_ecdh_calc_keys and fpnn_ecdh_calc_keys_client with counts
    around the wave and block sizes into over-allocated outputs: rows below n equal the
    257-row run (itself sampled against the oracle), every byte past n rows keeps its canary."""
    from fpnn_amd.engine import _ptr, check, lib
    c, cv = E.CURVES[curve], engine.ecdh_curve(curve)
    pb, nb, nmax = c.private_bytes, c.num_bytes, max(COUNTS)
    rng = np.random.default_rng(257 + nb)
    privs_h = rng.integers(0, 256, (nmax, pb), dtype=np.uint8)
    privs = torch.from_numpy(privs_h).to(DEV)
    server = bytes(rng.integers(1, 255, pb, dtype=np.uint8))

    def public(n):
        pub, ok = _canary(nmax, 2 * nb), _canary(nmax, 1)
        check(lib.fpnn_ecdh_public_keys(engine._h, cv, _ptr(privs), n, _ptr(pub), _ptr(ok)), "ecdh_public_keys")
        torch.cuda.synchronize()
        return pub, ok

    pub_full, ok_full = public(nmax)
    assert _tail_clean(pub_full, nmax) and _tail_clean(ok_full, nmax)
    for i in (0, 1, 63, 64, 255, 256):
        eok, epub = E.public_key(c, privs_h[i].tobytes())
        assert eok and ok_full[i, 0] == 1 and pub_full[i].cpu().numpy().tobytes() == epub, (curve, i)
    peers = pub_full[:nmax].contiguous()
    eok, server_pub = E.public_key(c, server)
    assert eok

    def server_side(n):
        keys, ivs, ok = _canary(nmax, 32), _canary(nmax, 16), _canary(nmax, 1)
        check(lib.fpnn_ecdh_calc_keys(engine._h, cv, server, _ptr(peers), n, 32, _ptr(keys), _ptr(ivs), _ptr(ok)),
              "ecdh_calc_keys")
        torch.cuda.synchronize()
        return keys, ivs, ok

    def client_side(n):
        keys, ivs, ok = _canary(nmax, 16), _canary(nmax, 16), _canary(nmax, 1)
        check(lib.fpnn_ecdh_calc_keys_client(engine._h, cv, _ptr(privs), server_pub, n, 16, _ptr(keys), _ptr(ivs),
                                             _ptr(ok)), "ecdh_calc_keys_client")
        torch.cuda.synchronize()
        return keys, ivs, ok

    full = {"public": (pub_full, ok_full), "server": server_side(nmax), "client": client_side(nmax)}
    for i in (0, 64, 256):
        eok, ek, ei = E.calc_key(curve, server, pub_full[i].cpu().numpy().tobytes(), 32)
        keys, ivs, ok = full["server"]
        assert eok and ok[i, 0] == 1 and keys[i].cpu().numpy().tobytes() == ek and ivs[i].cpu().numpy().tobytes() == ei
        eok, ek, ei = E.calc_key(curve, privs_h[i].tobytes(), server_pub, 16)
        keys, ivs, ok = full["client"]
        assert eok and ok[i, 0] == 1 and keys[i].cpu().numpy().tobytes() == ek and ivs[i].cpu().numpy().tobytes() == ei
    for n in COUNTS:
        for name, fn in (("public", public), ("server", server_side), ("client", client_side)):
            for got, ref in zip(fn(n), full[name]):
                assert torch.equal(got[:n], ref[:n]), (curve, name, n)
                assert _tail_clean(got, n), f"{curve} {name}: bytes past row {n} written"


def _edge_rows(golden, curve):
    for cv in golden("ecdh_edge_cases.json")["curves"]:
        if cv["curve"] == curve:
            return cv["server"]
    raise AssertionError(curve)


def _dev_bytes(b: bytes) -> torch.Tensor:
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(DEV)


def _same(s, ok, key, iv):
    """one device answer against one fixture row (key / iv only where the reference succeeds)"""
    return int(ok) == s["ok"] and (not s["ok"] or (bytes(key).hex(), bytes(iv).hex()) == (s["key"], s["iv"]))


@pytest.mark.parametrize("curve", V.CURVES)
def test_edge_cases_server_route(engine, golden, curve):
    """Every edge row through fpnn_ecdh_calc_keys: grouped by private key (the uniform,
    host-regularized scalar), the peers as one batch."""
    groups = {}
    for s in _edge_rows(golden, curve):
        groups.setdefault((s["private"], s["keylen"]), []).append(s)
    for (priv, kl), cases in groups.items():
        peers = _dev_bytes(b"".join(bytes.fromhex(s["peer"]) for s in cases))
        keys, ivs, ok = engine.ecdh_calc_keys(curve, bytes.fromhex(priv), peers, kl)
        torch.cuda.synchronize()
        keys, ivs, ok = keys.cpu().numpy(), ivs.cpu().numpy(), ok.cpu().numpy()
        for i, s in enumerate(cases):
            assert _same(s, ok[i], keys[i].tobytes(), ivs[i].tobytes()), (curve, s)


@pytest.mark.parametrize("curve", V.CURVES)
def test_edge_cases_client_route(engine, golden, curve):
    """Every edge row through fpnn_ecdh_calc_keys_client: grouped by peer, the private keys as
    per-lane scalars -- the device's own regularize (k + n, k + 2n, the select) on 0, 1, n - 1,
    n, n + 1, 2^bits - 1, ..."""
    groups = {}
    for s in _edge_rows(golden, curve):
        groups.setdefault((s["peer"], s["keylen"]), []).append(s)
    for (peer, kl), cases in groups.items():
        privs = _dev_bytes(b"".join(bytes.fromhex(s["private"]) for s in cases))
        keys, ivs, ok = engine.ecdh_calc_keys_client(curve, privs, bytes.fromhex(peer), kl)
        torch.cuda.synchronize()
        keys, ivs, ok = keys.cpu().numpy(), ivs.cpu().numpy(), ok.cpu().numpy()
        for i, s in enumerate(cases):
            assert _same(s, ok[i], keys[i].tobytes(), ivs[i].tobytes()), (curve, s)


@pytest.mark.parametrize("curve", V.CURVES)
def test_edge_cases_single_call_route(engine, golden, curve):
    """Every edge row through fpnn_ecdh_calc_key_host (ECCKeyExchange::init + calcKey)."""
    for s in _edge_rows(golden, curve):
        ok, key, iv = engine.ecdh_calc_key_host(curve, bytes.fromhex(s["private"]), bytes.fromhex(s["peer"]),
                                                s["keylen"])
        assert (int(ok), key.hex(), iv.hex()) == (s["ok"], s["key"], s["iv"]), (curve, s)


@pytest.mark.parametrize("curve", V.CURVES)
def test_public_keys_edge_scalars(engine, curve):
    """fpnn_ecdh_public_keys on the per-lane scalars 0, 1, 2, n - 1, n, n + 1, 2^bits - 1 against
    the oracle's public_key (ok and, where ok, the point)."""
    c = E.CURVES[curve]
    ks = [0, 1, 2, c.n - 1, c.n, c.n + 1, (1 << (8 * c.private_bytes)) - 1]
    kb = [k.to_bytes(c.private_bytes, "big") for k in ks]
    pub, ok = engine.ecdh_public_keys(curve, _dev_bytes(b"".join(kb)))
    torch.cuda.synchronize()
    pub, ok = pub.cpu().numpy(), ok.cpu().numpy()
    exp = [E.public_key(c, b) for b in kb]
    assert any(e[0] for e in exp) and not all(e[0] for e in exp)
    for i, (eok, epub) in enumerate(exp):
        assert bool(ok[i]) == eok and (not eok or pub[i].tobytes() == epub), (curve, hex(ks[i]))
