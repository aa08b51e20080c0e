"""The kernel choice of the package calls at its edges, on the device (the CPU side of the same
rules: tests/test_dispatch_plan.py).  With F = one chain per GPU lane (CUs x 1024), one batch of
F frames of 1-175 bytes at unaligned offsets over 1000 AES-256 keyed connections is ciphered at
F and F - 1 frames, under length bounds of 175, 176 and 2049 bytes and without one, and at F / 4
and F / 4 + 1 frames (as many chains as the chip has quads, and one more); uniform 16-byte packets
at F - 1 and F.  Every call must run the kernel fpnn_aes.h promises for that shape -- last_kernel
-- and give the oracle's bytes, with every byte outside the call's frames left alone.  Only the
public Python API is used; the oracle runs twice for the whole module.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEYLEN, NK = 32, 1000


def to_dev(a):
    return torch.from_numpy(np.array(a, copy=True)).to(DEV)


class Edge:
    pass


@pytest.fixture(scope="module")
def edge(engine, oracle):
    import fpnn_amd
    e = Edge()
    rng = np.random.default_rng(20261)
    e.F = F = torch.cuda.get_device_properties(0).multi_processor_count * 1024
    lens = rng.integers(1, 176, F).astype(np.int64)
    pick = rng.random(F)
    lens[pick < 0.2] = 145  # FPNN's quests
    lens[(pick >= 0.2) & (pick < 0.3)] = 16 * rng.integers(1, 11, int(((pick >= 0.2) & (pick < 0.3)).sum()))
    lens[[0, F // 4 - 1, F // 4, F - 2, F - 1]] = (175, 1, 175, 16, 175)
    gaps = rng.integers(0, 3, F)
    e.offs = np.concatenate([[0], np.cumsum(lens[:-1] + gaps[:-1])]).astype(np.int64) + 1
    e.lens = lens
    e.total = int(e.offs[-1] + lens[-1] + 16)
    slots = rng.integers(0, NK, F).astype(np.int32)
    keys = rng.integers(0, 256, NK * KEYLEN, dtype=np.uint8)
    ivs = rng.integers(0, 256, NK * 16, dtype=np.uint8)
    e.ks = fpnn_amd.KeySet(engine, keys.tobytes(), KEYLEN, ivs.tobytes())
    e.data = rng.integers(0, 256, e.total, dtype=np.uint8)  # plaintext of the encrypts, ciphertext of the decrypts
    e.fill = rng.integers(0, 256, e.total, dtype=np.uint8)  # what the destination holds before a call
    okw = dict(in_off=e.offs.astype(np.uint64), lens=lens.astype(np.uint32), key_slot=slots.astype(np.uint32),
               keys=keys, keylen=KEYLEN, ivs=ivs, threads=8)
    e.exp = {}
    for encrypt in (True, False):
        out = e.data.copy()
        oracle.package_batch(encrypt, e.data, out, F, **okw)
        e.exp[encrypt] = out
    # bytes inside some frame (the frames never overlap and lie in index order)
    d = np.zeros(e.total + 1, np.int32)
    np.add.at(d, e.offs, 1)
    np.add.at(d, e.offs + lens, -1)
    e.inside = np.cumsum(d[:-1]) > 0
    # uniform 16-byte packets under key slot 0
    e.udata = rng.integers(0, 256, 16 * F, dtype=np.uint8)
    e.uexp = e.udata.copy()
    oracle.package_batch(True, e.udata, e.uexp, F, stride=16, uniform_len=16, keys=keys, keylen=KEYLEN, ivs=ivs, threads=8)
    e.src = to_dev(e.data)
    e.usrc = to_dev(e.udata)
    e.kw = dict(in_off=to_dev(e.offs), lens=to_dev(lens.astype(np.int32)), key_slot=to_dev(slots))
    for a in (e.offs, e.lens, e.data, e.fill, e.inside, e.udata, e.uexp, e.exp[True], e.exp[False]):
        a.setflags(write=False)
    return e


def expected(e, encrypt, n):
    """The destination after a call on the first n frames: theirs from the oracle, every other byte kept."""
    end = int(e.offs[n - 1] + e.lens[n - 1])
    exp = e.fill.copy()
    exp[:end] = np.where(e.inside[:end], e.exp[encrypt][:end], e.fill[:end])
    return exp


def run(engine, e, encrypt, n, bound, kernel):
    import fpnn_amd
    dst = to_dev(e.fill)
    fn = engine.package_encrypt if encrypt else engine.package_decrypt
    fn(e.src, dst, n, e.ks, max_len=bound, **e.kw)
    torch.cuda.synchronize()
    got = engine.last_kernel(fpnn_amd.K_ENCRYPT if encrypt else fpnn_amd.K_DECRYPT)
    print(f"encrypt={encrypt} n={n} (F={e.F}) max_len={bound}: {got}")
    assert got == kernel
    bad = np.nonzero(dst.cpu().numpy() != expected(e, encrypt, n))[0]
    assert len(bad) == 0, f"{len(bad)} bytes differ, first at {bad[:8]}"


@pytest.mark.parametrize("dn,bound,kernel", [
    (0, 175, "cfb_encrypt_frames"),    # K2s-DB: the bound within 175 bytes, one chain per lane
    (-1, 175, "cfb_encrypt_hybrid"),   # one chain short of it
    (0, 176, "cfb_encrypt_chains"),    # one byte past the whole-frame bound: K2
    (0, 2049, "cfb_encrypt_hybrid"),   # one byte past K2's bound
])
def test_encrypt_bound_edges(engine, edge, dn, bound, kernel):
    run(engine, edge, True, edge.F + dn, bound, kernel)


@pytest.mark.parametrize("dn,kernel", [(0, "cfb_encrypt_coop"), (1, "cfb_encrypt_hybrid")])
def test_encrypt_quads_edge(engine, edge, dn, kernel):
    """Without a bound: K2c while every chain gets a quad of its own, K2h from one more on."""
    run(engine, edge, True, edge.F // 4 + dn, 0, kernel)


@pytest.mark.parametrize("dn,kernel", [(-1, "cfb_encrypt_coop"), (0, "cfb_encrypt_chains")])
def test_encrypt_uniform_full_chip_edge(engine, edge, dn, kernel):
    import fpnn_amd
    e = edge
    n = e.F + dn
    dst = torch.zeros_like(e.usrc)
    engine.package_encrypt(e.usrc, dst, n, e.ks, stride=16, uniform_len=16)
    torch.cuda.synchronize()
    got = engine.last_kernel(fpnn_amd.K_ENCRYPT)
    print(f"uniform 16 B n={n} (F={e.F}): {got}")
    assert got == kernel
    exp = e.uexp.copy()
    exp[16 * n:] = 0
    assert np.array_equal(dst.cpu().numpy(), exp)


@pytest.mark.parametrize("dn,bound,kernel", [
    (0, 175, "cfb_decrypt_frames"),   # D2s
    (-1, 175, "cfb_decrypt_ragged"),  # one frame short of one per lane: K1r
    (0, 176, "cfb_decrypt_ragged"),   # one byte past the bound
])
def test_decrypt_bound_edges(engine, edge, dn, bound, kernel):
    run(engine, edge, False, edge.F + dn, bound, kernel)
