"""Pin the oracle before trusting it (CPU only).

1. Published known answers: FIPS-197 appendix C.1/C.3 and NIST SP 800-38A F.3.13 /
   F.3.17 (independent of the reference; the reference reproduces them too).
2. Golden fixtures produced by the compiled reference (oracle/gen_golden.py).
3. Live randomized comparison with oracle/_ref when it is built (this container).
"""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIPS_C1 = ("000102030405060708090a0b0c0d0e0f", "00112233445566778899aabbccddeeff", "69c4e0d86a7b0430d8cdb78070b4c55a")
FIPS_C3 = ("000102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f", "00112233445566778899aabbccddeeff",
           "8ea2b7ca516745bfeafc49904b496089")
SP_PT = ("6bc1bee22e409f96e93d7e117393172aae2d8a571e03ac9c9eb76fac45af8e51"
         "30c81c46a35ce411e5fbc1191a0a52eff69f2445df4f9b17ad2b417be66c3710")
SP_F313 = ("2b7e151628aed2a6abf7158809cf4f3c",
           "3b3fd92eb72dad20333449f8e83cfb4ac8a64537a0b3a93fcde3cdad9f1ce58b"
           "26751f67a3cbb140b1808cf187a4f4dfc04b05357c5d1c0eeac4c66f9ff7f2e6")
SP_F317 = ("603deb1015ca71be2b73aef0857d77811f352c073b6108d72d9810a30914dff4",
           "dc7e84bfda79164b7ecd8486985d386039ffed143b28b1c832113c6331e5407b"
           "df10132415e54b92a13ed0a8267ae2f975a385741ab9cef82031623d55b1e471")
IV = bytes(range(16))


@pytest.mark.parametrize("kat", [FIPS_C1, FIPS_C3])
def test_fips197_ecb(oracle, kat):
    key, pt, ct = (bytes.fromhex(x) for x in kat)
    assert oracle.encrypt_block(key, pt) == ct


@pytest.mark.parametrize("kat", [SP_F313, SP_F317])
def test_sp800_38a_cfb128(oracle, kat):
    key, ct = bytes.fromhex(kat[0]), bytes.fromhex(kat[1])
    pt = bytes.fromhex(SP_PT)
    assert oracle.cfb(key, True, pt, IV)[0] == ct
    assert oracle.cfb(key, False, ct, IV)[0] == pt
    # split calls exercise the (ivec, pos) carry
    out1, iv1, n1 = oracle.cfb(key, True, pt[:23], IV)
    out2, _, _ = oracle.cfb(key, True, pt[23:], iv1, n1)
    assert out1 + out2 == ct


def test_golden_kat(oracle, golden):
    g = golden("kat.json")
    for v in g["ecb"]:
        assert oracle.encrypt_block(bytes.fromhex(v["key"]), bytes.fromhex(v["in"])).hex() == v["out"], v["name"]
    for v in g["cfb"]:
        out = oracle.cfb(bytes.fromhex(v["key"]), True, bytes.fromhex(v["in"]), bytes.fromhex(v["iv"]))[0]
        assert out.hex() == v["out"], v["name"]


def test_golden_cfb_cases(oracle, golden):
    cases = golden("cfb_cases.json")
    assert len(cases) >= 200
    for c in cases:
        out, iv, pos = oracle.cfb(bytes.fromhex(c["key"]), c["encrypt"], bytes.fromhex(c["in"]), bytes.fromhex(c["iv"]),
                                  c["pos"])
        assert (out.hex(), iv.hex(), pos) == (c["out"], c["iv_out"], c["pos_out"])


def test_golden_package_cases(oracle, golden):
    for c in golden("package_cases.json"):
        key, iv, data = (bytes.fromhex(c[k]) for k in ("key", "iv", "in"))
        assert oracle.package(key, iv, True, data).hex() == c["encrypt"]
        assert oracle.package(key, iv, False, data).hex() == c["decrypt"]
        assert oracle.package_frame(key, iv, data).hex() == c["frame"]


def test_golden_stream_cases(oracle, golden):
    from pyoracle import StreamOracle
    for c in golden("stream_cases.json"):
        s = StreamOracle(oracle, bytes.fromhex(c["key"]), bytes.fromhex(c["iv"]))
        for fr in c["frames"]:
            assert s.crypt(c["encrypt"], bytes.fromhex(fr["in"])).hex() == fr["out"]


def test_package_batch_matches_single_calls(oracle):
    rng = np.random.default_rng(3)
    n = 50
    lens = rng.integers(0, 300, n).astype(np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1].astype(np.uint64) + 3)]).astype(np.uint64)
    total = int(offs[-1] + lens[-1] + 16)
    inp = rng.integers(0, 256, total, dtype=np.uint8)
    out = np.zeros_like(inp)
    keys = rng.integers(0, 256, 3 * 32, dtype=np.uint8)
    ivs = rng.integers(0, 256, 3 * 16, dtype=np.uint8)
    slots = (np.arange(n) % 3).astype(np.uint32)
    oracle.package_batch(True, inp, out, n, in_off=offs, lens=lens, key_slot=slots, keys=keys, keylen=32, ivs=ivs,
                         threads=4)
    for i in range(n):
        k = keys[32 * slots[i]: 32 * slots[i] + 32].tobytes()
        v = ivs[16 * slots[i]: 16 * slots[i] + 16].tobytes()
        seg = inp[offs[i]: offs[i] + lens[i]].tobytes()
        assert out[offs[i]: offs[i] + lens[i]].tobytes() == oracle.package(k, v, True, seg)


def test_live_reference_random(oracle, ref_oracle):
    rng = np.random.default_rng(99)
    for t in range(1500):
        kl = (16, 24, 32)[t % 3]
        key, iv = rng.bytes(kl), rng.bytes(16)
        data = rng.bytes(int(rng.integers(0, 700)))
        pos = int(rng.integers(0, 16))
        enc = bool(t & 1)
        assert oracle.cfb(key, enc, data, iv, pos) == ref_oracle.cfb(key, enc, data, iv, pos)
        if kl != 24:
            assert oracle.package_frame(key, iv, data) == ref_oracle.package_frame(key, iv, data)


def test_port_speed_tracks_reference(oracle, ref_oracle):
    """the restatement runs the same algorithm (T-tables, per-frame key
    setup, byte-loop CFB), so one core of it should time close to the compiled reference
    (measured here: within ~12%).  The bound is loose so that a loaded CI host cannot
    flake it; it catches an accidentally de-optimised oracle."""
    n, L = 2048, 1024
    a = np.random.default_rng(5).integers(0, 256, n * L, dtype=np.uint8)
    t, o = np.empty_like(a), np.empty_like(a)
    key, iv = bytes(range(32)), bytes(16)
    best = {}
    for _ in range(3):
        for name, orc in (("port", oracle), ("reference", ref_oracle)):
            dt = orc.time_package_roundtrip(a, t, o, n, L, key, iv, 1, 1)
            best[name] = min(best.get(name, 1e9), dt)
    ratio = best["reference"] / best["port"]  # port speed relative to the reference
    assert 0.6 < ratio < 1.7, ratio


def test_framing_restatement_known_answers():
    """The framing restatement on hand-built inputs whose verdicts follow from the
    reference's code (core/EncryptedPackageReceiver.cpp:62-81,
    core/EncryptedStreamReceiver.cpp:8-15,87-110, proto/FPMessage.cpp:27-44)."""
    import struct
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import pyoracle as P
    pk = struct.pack("<I", 3) + b"abc" + struct.pack("<I", 0) + struct.pack("<I", 5) + b"xy"
    assert P.scan_package(pk, 100, 8) == ([(4, 3), (11, 0)], P.SCAN_OK, 11)
    assert P.scan_package(pk, 100, 1) == ([(4, 3)], P.SCAN_FULL, 7)
    assert P.scan_package(struct.pack("<I", 101) + bytes(200), 100, 8) == ([], P.SCAN_TOO_LARGE, 0)
    assert P.scan_package(b"\x01\x00", 100, 8) == ([], P.SCAN_OK, 0)

    def msg(mtype, ss, psize, body=None):
        h = b"FPNN" + bytes([1, 0x80, mtype, ss]) + struct.pack("<I", psize)
        return h + (bytes(body) if body is not None else b"")
    two = msg(1, 3, 5, 5 + 3 + 4)   # TWOWAY: psize + ss + seq
    ans = msg(2, 9, 5, 5 + 4)       # ANSWER: psize + seq (ss = status, not counted)
    one = msg(0, 3, 5, 5 + 3)       # ONEWAY: psize + ss
    st = two + ans + one
    assert P.scan_stream(st, 1 << 23, 8) == ([(0, 24), (24, 21), (45, 20)], P.SCAN_OK, 65)
    assert P.scan_stream(st[:-1], 1 << 23, 8) == ([(0, 24), (24, 21)], P.SCAN_OK, 45)
    assert P.scan_stream(b"GET " + bytes(8), 1 << 23, 8)[1] == P.SCAN_BAD_MAGIC
    assert P.scan_stream(msg(3, 0, 0), 1 << 23, 8)[1] == P.SCAN_BAD_MTYPE
    assert P.scan_stream(msg(0, 0, 0), 1 << 23, 8)[1] == P.SCAN_BAD_LENGTH          # length 0 is rejected
    assert P.scan_stream(msg(0, 0, 0x80000000), 1 << 23, 8)[1] == P.SCAN_BAD_LENGTH  # (int) < 0
    assert P.scan_stream(msg(2, 0, 0xFFFFFFFF, 3), 1 << 23, 8) == ([(0, 15)], P.SCAN_OK, 15)  # uint32 wrap
    assert P.scan_stream(msg(0, 0, 100), 111, 8)[1] == P.SCAN_TOO_LARGE             # 12 + 100 > 111
    assert P.scan_stream(msg(0, 0, 100, 100), 112, 8) == ([(0, 112)], P.SCAN_OK, 112)


def test_framing_restatement_vs_reference_receivers(oracle):
    """The framing restatement (ao_scan_package / ao_scan_stream) against the reference's
    own receivers (tests/golden/framing_cases.json, oracle/_ref/framing_ref): the same
    frames, verdicts and consumed bytes, and the oracle's decryption of each frame equals
    the plaintext the reference receiver decoded."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import pyoracle as P
    from framing_golden import expected, load_cases
    cases = load_cases()
    assert {c["expect"] for c in cases} == {"ok", "too_large", "bad_magic", "bad_mtype", "bad_length"}
    for c in cases:
        key, iv, wire = bytes.fromhex(c["key"]), bytes.fromhex(c["iv"]), bytes.fromhex(c["wire"])
        frames, status, consumed, raws = expected(c)
        if c["mode"] == "package":
            got = P.scan_package(wire, c["max_len"], 64)
            plain = [oracle.package(key, iv, False, wire[o:o + n]) for o, n in frames]
        else:
            stream = oracle.cfb(key, False, wire, iv, 0)[0]
            got = P.scan_stream(stream, c["max_len"], 64)
            plain = [stream[o:o + n] for o, n in frames]
        assert got == (frames, status, consumed), c["name"]
        for j, (p, r) in enumerate(zip(plain, raws)):
            assert r is None or p == r, (c["name"], j)


def test_openssl_comparator_matches_oracle(oracle):
    """The bench's OpenSSL EVP cfb128 comparator (oracle/openssl_cfb.c) computes the same
    package-mode bytes as the restatement (so its timing is of the same work)."""
    import ctypes as C
    lib_path = os.path.join(ROOT, "oracle", "libossl_cfb.so")
    if not os.path.exists(lib_path):
        pytest.skip("oracle/libossl_cfb.so not built (make -C oracle ossl; needs libcrypto)")
    lib = C.CDLL(lib_path)
    f = lib.ossl_time_package_roundtrip
    u8 = C.POINTER(C.c_uint8)
    f.argtypes = [u8, u8, u8, C.c_uint32, C.c_uint32, C.c_char_p, C.c_size_t, C.c_char_p, C.c_int, C.c_int]
    f.restype = C.c_double
    rng = np.random.default_rng(77)
    for keylen, L in ((16, 1000), (24, 17), (32, 1024)):
        n = 300
        key, iv = rng.bytes(keylen), rng.bytes(16)
        inp = rng.integers(0, 256, n * L, dtype=np.uint8)
        tmp, out = np.empty_like(inp), np.empty_like(inp)
        assert f(inp.ctypes.data_as(u8), tmp.ctypes.data_as(u8), out.ctypes.data_as(u8), n, L, key, keylen, iv,
                 4, 1) > 0
        exp = inp.copy()
        oracle.package_batch(True, inp, exp, n, stride=L, uniform_len=L, keys=np.frombuffer(key, np.uint8).copy(),
                             keylen=keylen, ivs=np.frombuffer(iv, np.uint8).copy())
        assert np.array_equal(tmp, exp)
        assert np.array_equal(out, inp)


def test_golden_modes_cases(oracle, golden):
    """The rest of rijndael.h restated (oracle/aes_oracle.c ao_setup_decrypt, ao_decrypt_block,
    ao_cbc_*, ao_ofb) against the reference's outputs in tests/golden/modes_cases.json."""
    g = golden("modes_cases.json")
    for c in g["setup_decrypt"]:
        ctx = oracle.setup_decrypt(bytes.fromhex(c["key"]))
        assert ctx.nrounds == c["nrounds"] and list(ctx.rk[:len(c["rk"])]) == c["rk"]
    for c in g["ecb_decrypt"]:
        assert oracle.decrypt_block(bytes.fromhex(c["key"]), bytes.fromhex(c["in"])).hex() == c["out"]
    for c in g["cbc"]:
        out, iv = oracle.cbc(bytes.fromhex(c["key"]), c["encrypt"], bytes.fromhex(c["in"]), bytes.fromhex(c["iv"]),
                             c["len"])
        assert out.hex() == c["out"] and iv.hex() == c["iv_out"]
    for c in g["ofb"]:
        out, iv, pos = oracle.ofb(bytes.fromhex(c["key"]), bytes.fromhex(c["in"]), bytes.fromhex(c["iv"]), c["pos"])
        assert (out.hex(), iv.hex(), pos) == (c["out"], c["iv_out"], c["pos_out"])
    # FIPS-197 C.1 / C.3 inverse cipher
    assert g["ecb_decrypt"][0]["out"] == "00112233445566778899aabbccddeeff"
    assert g["ecb_decrypt"][1]["out"] == "00112233445566778899aabbccddeeff"


def test_ecdh_restatement_vs_reference():
    """oracle/ecdh_oracle.py against core/KeyExchange.cpp + core/micro-ecc run by
    oracle/_ref/ecdh_ref (tests/golden/ecdh_cases.json): client public keys, the keys and
    IVs both sides derive, degenerate scalars and malformed peers on all four curves."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ecdh_oracle as E
    with open(os.path.join(ROOT, "tests", "golden", "ecdh_cases.json")) as f:
        g = json.load(f)
    assert {c["curve"] for c in g["curves"]} == set(E.CURVES)
    fails = 0
    for cv in g["curves"]:
        c = E.CURVES[cv["curve"]]
        for cl in cv["clients"]:
            ok, pub = E.public_key(c, bytes.fromhex(cl["private"]))
            assert ok and pub.hex() == cl["public"], cv["curve"]
            ok, key, iv = E.calc_key(cv["curve"], bytes.fromhex(cl["private"]), bytes.fromhex(cv["server_public"]),
                                     cl["keylen"])
            assert (int(ok), key.hex(), iv.hex()) == (cl["ok"], cl["key"], cl["iv"]), cv["curve"]
        for s in cv["server"]:
            ok, key, iv = E.calc_key(cv["curve"], bytes.fromhex(s["private"]), bytes.fromhex(s["peer"]), s["keylen"])
            assert (int(ok), key.hex(), iv.hex()) == (s["ok"], s["key"], s["iv"]), (cv["curve"], s)
            fails += 1 - s["ok"]
    assert fails >= 4 * 5  # zero point, short peer, bad keylen, private 1, short private per curve


def test_ecdh_restatement_vs_reference_edge_cases():
    """oracle/ecdh_oracle.py against the reference on edge scalars and peers
    (tests/golden/ecdh_edge_cases.json, written by oracle/_ref/ecdh_ref): scalars 0, 1, 2, 3,
    n - 2 .. n + 1, (n +- 1) / 2, 2^bits - 1, 2^(bits - 1), 2^bits - n; peer coordinates 0, 1, 2,
    p - 2 .. p + 1, 2^bits - 1, 2^(bits - 1), 2^96 - 1 in both positions; on-curve points with
    tiny or near-p x, their negatives, and x not reduced.  Every row, failures included."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ecdh_oracle as E
    with open(os.path.join(ROOT, "tests", "golden", "ecdh_edge_cases.json")) as f:
        g = json.load(f)
    assert {c["curve"] for c in g["curves"]} == set(E.CURVES)
    for cv in g["curves"]:
        c = E.CURVES[cv["curve"]]
        p, n, top = c.p, c.n, 1 << (8 * c.num_bytes)
        assert len(cv["server"]) >= 100
        for s in cv["server"]:
            ok, key, iv = E.calc_key(cv["curve"], bytes.fromhex(s["private"]), bytes.fromhex(s["peer"]), s["keylen"])
            assert (int(ok), key.hex(), iv.hex()) == (s["ok"], s["key"], s["iv"]), (cv["curve"], s)
        # the fixture holds what it is meant to hold
        scalars = {int(s["private"], 16) for s in cv["server"]}
        assert scalars >= {0, 1, 2, 3, n - 2, n - 1, n, n + 1, (n - 1) // 2, (n + 1) // 2, top - 1, top >> 1, top - n}
        coords = {0, 1, 2, p - 2, p - 1, p, p + 1, top - 1, top >> 1, (1 << 96) - 1}
        nb2 = 2 * c.num_bytes
        assert {int(s["peer"][:nb2], 16) for s in cv["server"]} >= coords
        assert {int(s["peer"][nb2:], 16) for s in cv["server"]} >= coords
        assert {s["keylen"] for s in cv["server"]} == {16, 32}
        assert 0 < sum(s["ok"] for s in cv["server"]) < len(cv["server"])


def _ref_exe(name):
    p = os.path.join(ROOT, "oracle", "_ref", name)
    if not os.access(p, os.X_OK):
        pytest.skip(f"oracle/_ref/{name} not built (needs /root/reference)")
    return p


def test_c1_echo_reference_reproduces_fixture():
    """oracle/_ref/io_echo_ref (the reference's SendBuffer + encrypted receivers on its own
    Encryptor, C1's encrypted echo) reproduces tests/golden/c1_cases.json -- the fixture the
    drop-in build is checked against on the GPU (tests/test_gpu_dropin.py)."""
    import json
    import subprocess
    exe = _ref_exe("io_echo_ref")
    with open(os.path.join(ROOT, "tests", "golden", "c1_cases.json")) as f:
        cases = json.load(f)["echo"]
    for g in cases[1:]:  # the small cases (C1 itself is 10 000 quests)
        out = subprocess.run([exe, "1" if g["mode"] == "stream" else "0", str(g["keylen"]), str(g["quests"]),
                              str(g["payload"]), str(g["window"])], capture_output=True, text=True, check=True,
                             timeout=120).stdout
        d = json.loads(out.strip().splitlines()[-1])
        assert d["answers_ok"]
        assert [d[k] for k in ("wire_c2s_fnv", "wire_s2c_fnv")] == [g["wire_c2s_fnv"], g["wire_s2c_fnv"]], g


def _multi_cases():
    import json
    with open(os.path.join(ROOT, "tests", "golden", "multi_cases.json")) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("case", _multi_cases(), ids=lambda c: c["name"])
def test_collect_patch_keeps_reference_wire_bytes_on_cpu(case):
    """INTEGRATION.md 2a applied to the reference's IO plumbing (oracle/collect_patch.py:
    SendBuffer::encryptData and EncryptedPackageReceiver::fetch queue their cipher calls in
    a collect phase, the IO loop flushes once per cycle and direction) -- here over the
    REFERENCE cipher through a CPU stand-in queue (oracle/_ref/io_multi_cpucollect).  The
    patched plumbing's wire bytes equal the unpatched reference build's
    (tests/golden/multi_cases.json), so the deferral and ordering are right independently
    of the GPU; tests/test_gpu_dropin.py runs the same plumbing on EncryptorBatch."""
    import json
    import subprocess
    exe = _ref_exe("io_multi_cpucollect")
    out = subprocess.run([exe, "1" if case["mode"] == "stream" else "0", str(case["keylen"]), str(case["conns"]),
                          str(case["quests_per_conn"]), str(case["payload"]), str(case["window"]),
                          str(case["threads"]), "1", "1" if case.get("first_clear") else "0"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert d["build"] == "cpucollect" and d["ok"] and d["answers_ok"], d
    assert d["flushes"] > 0
    for k in ("wire_c2s_bytes", "wire_c2s_fnv", "wire_s2c_bytes", "wire_s2c_fnv"):
        assert d[k] == case[k], (k, d[k], case[k])


def test_udp_encryptor_reference_reproduces_fixture():
    """oracle/_ref/udp_v2_ref -- the reference's UDPEncryptor (core/UDP.v2/UDPCommon.v2.cpp)
    on its own Encryptor and KeyExchange -- reproduces tests/golden/udp_cases.json, the
    fixture the drop-in build is checked against on the GPU (tests/test_gpu_dropin.py)."""
    import json
    import subprocess
    exe = _ref_exe("udp_v2_ref")
    with open(os.path.join(ROOT, "tests", "golden", "udp_cases.json")) as f:
        cases = json.load(f)["cases"]
    for c in cases:
        out = subprocess.run([exe], input=c["input"] + "\n", capture_output=True, text=True, check=True,
                             timeout=120).stdout
        d = json.loads([x for x in out.splitlines() if x.startswith("{")][-1])
        d.pop("seconds")
        assert d == c["expect"]


def test_udp_dropin_binds_cipher_and_key_exchange_to_libfpnn_aes():
    """The drop-in build of UDPCommon.v2.cpp (oracle/Makefile `udp`) defines neither cipher
    nor key exchange: PackageEncryptor / StreamEncryptor and ECCKeyExchange::init / calcKey
    are undefined symbols resolved from libfpnn_aes.so (no core/Encryptor.cpp,
    core/KeyExchange.cpp, micro-ecc or base/rijndael.c linked), and UDPEncryptor itself is
    the reference's code."""
    import subprocess
    exe = _ref_exe("udp_v2_dropin")
    ldd = subprocess.run(["ldd", exe], capture_output=True, text=True, check=True).stdout
    assert "libfpnn_aes.so" in ldd, ldd
    syms = subprocess.run(["nm", "-C", exe], capture_output=True, text=True, check=True).stdout.splitlines()
    defined = [s for s in syms if " T " in s or " t " in s]
    assert any("fpnn::UDPEncryptor::createPair" in s for s in defined)
    assert not [s for s in defined if "rijndael_" in s or "uECC_" in s or "Encryptor::encrypt" in s
                or "Encryptor::decrypt" in s or "ECCKeyExchange::calcKey" in s]
    undef = [s.split(" U ")[-1] for s in syms if " U " in s]
    for want in ("fpnn::ECCKeyExchange::calcKey", "fpnn::ECCKeyExchange::init", "fpnn::encryptor_serial()",
                 "rijndael_setup_encrypt"):
        assert any(want in u for u in undef), want
    # the Encryptor methods are reached through the vtables, whose key functions live in
    # libfpnn_aes.so: the executable holds copy-relocated vtables bound at load time
    dyn = subprocess.run(["nm", "-DC", exe], capture_output=True, text=True, check=True).stdout
    assert "vtable for fpnn::PackageEncryptor" in dyn and "vtable for fpnn::StreamEncryptor" in dyn


def test_dropin_builds_bind_the_cipher_to_libfpnn_aes():
    """The drop-in builds of the reference callers (oracle/Makefile `dropin`) define no
    cipher of their own: every Encryptor method and rijndael_* call they make is an
    undefined symbol resolved from libfpnn_aes.so (core/Encryptor.cpp and base/rijndael.c
    are not linked), and the receivers' objects were compiled against include/Encryptor.h
    (PackageEncryptor carries this header's _ctx member: the layout differs from
    core/Encryptor.h, so a wrong header would not link against these symbols consistently)."""
    import subprocess
    for name in ("framing_dropin", "io_echo_dropin", "io_multi_dropin", "io_multi_batched"):
        exe = _ref_exe(name)
        ldd = subprocess.run(["ldd", exe], capture_output=True, text=True, check=True).stdout
        assert "libfpnn_aes.so" in ldd, ldd
        syms = subprocess.run(["nm", "-C", exe], capture_output=True, text=True, check=True).stdout.splitlines()
        defined = [s for s in syms if " T " in s or " t " in s]
        assert not [s for s in defined if "rijndael_" in s or "Encryptor::encrypt" in s or "Encryptor::decrypt" in s]
        undef = [s.split(" U ")[-1] for s in syms if " U " in s]
        assert "fpnn::encryptor_serial()" in undef  # only include/Encryptor.h's constructor calls this
        if name == "io_multi_batched":  # the patched call sites queue into the product's collector
            assert "fpnn::EncryptorBatch::flush()" in undef
        else:
            assert any("fpnn::PackageEncryptor::decrypt" in u for u in undef)
