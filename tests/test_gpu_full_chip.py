"""Uniform batches at full-chip size: K2 chains without a `len` array, and dense decrypt steps
past a wave's first.

Two kernel families have forms that only a batch as large as the chip reaches:

* K2 (`k_cfb_encrypt_chains`) takes a uniform or array-free batch only from one chain per GPU
  lane on (F = CUs x 1024, dispatch_plan.hpp); below that the batch is K2c's.  Part A encrypts
  F + F // 4 + 37 chains, so a quarter of the lanes run a second chain one grid stride later and
  the last wave of that pass is partial, at lengths and strides where the line-alignment head
  (`mis` / `h`, k_encrypt.hip) takes every value 0..7, chunks run on unaligned pointers, the last
  chunk's prefetch reads the key table, singles and a partial block follow the chunks, keys are
  per lane (4-block chunks, the E_k(IV) table, the round keys kept over a grid stride) and, in
  stream mode, a position head comes before the alignment singles.
* The dense decrypt kernels (k_decrypt.hip) launch min(ceil(nchunks / 64), CUs) workgroups of 16
  waves; a wave takes a second and a third step of U chunks (the ping-pong prefetch into the
  second buffer and back into the first, the hand-over to the overhanging tail step,
  `boundary[c0]` beyond the first sweep in place, K1's grid-stride loop) only when the batch has
  more than 2 * U * nwaves + U chunks.  Part A's decrypts and part B's decrypt-only batches are
  sized for that.

Every size comes from the device's CU count, and every case asserts by arithmetic, before the
call, that its batch reaches the route and the step it is meant for, and afterwards that the
kernel it names ran: on a chip with another CU count a case fails loudly instead of testing
nothing.  The sizes are not a workload's; they are the smallest at which the route or the step
exists (256 CUs: 85-99 MB per round trip, 17-34 MB per decrypt-only case).

Bit-exact against the oracle; every destination is pre-filled with a pattern, and the gaps
between strides, the bytes before the batch (stream cases) and the 64 guard bytes behind it must
keep it.  Only the public Python layer is used.  The oracle runs once per shape.
"""
import time

import numpy as np
import pytest
import torch

from test_gpu_parity import keyset, to_dev, to_host

pytestmark = pytest.mark.gpu

GUARD = 64
LEAD = 5  # stream cases: the device buffers start this many bytes past a 128-byte line

# 64-block chunks per wave step of the decrypt kernel each shape runs (k_decrypt.hip, dec_launch)
U = {
    "R1": 4,   # K1d unaligned (nb = 17), one key
    "R2": 4,   # K1, LAYOUT_UNIFORM (partial last block per packet)
    "R3": 4,   # K1, strided LAYOUT_FULL
    "R4a": 1,  # K1k: one chunk per step, per-lane keys
    "R4b": 1,
    "D1": 4,   # K1d aligned, one key (fenced)
    "D2": 4,   # K1d keyed, 4 chunks per packet
    "D3": 2,   # K1d keyed, 2 chunks per packet
    "D4": 1,   # K1d keyed, 3 chunks per packet
}


class Chip:
    pass


@pytest.fixture(scope="module")
def chip():
    """The device's sizes, and the bytes every case draws from: random data (plaintext of the
    round trips, ciphertext of the decrypt-only cases) and the pattern the destinations hold
    before a call.  Read-only."""
    c = Chip()
    c.CUS = torch.cuda.get_device_properties(0).multi_processor_count
    c.F = c.CUS * 1024
    c.COUNT = c.F + c.F // 4 + 37
    n = max(c.COUNT * 301, (128 * c.CUS + 64) * 1024) + 4096
    c.data = np.random.default_rng(20270).integers(0, 256, n, dtype=np.uint8)
    c.pattern = np.resize(np.arange(1, 252, dtype=np.uint8), n)
    c.data.setflags(write=False)
    c.pattern.setflags(write=False)
    print(f"CUs={c.CUS} F={c.F} COUNT={c.COUNT}")
    return c


def ceil_div(a, b):
    return -(-a // b)


def dense_plan(chip, count, nb):
    """The plan's constants for a dense decrypt of count packets of nb blocks (decrypt_route)."""
    total_blocks = nb * count
    nchunks = ceil_div(total_blocks, 64)
    want = ceil_div(nchunks, 64)
    nwaves = min(want, chip.CUS) * 16
    return total_blocks, nchunks, want, nwaves


def third_step(chip, case, count, nb):
    """Some wave takes a third step: the second buffer is used and then the first again."""
    total_blocks, nchunks, want, nwaves = dense_plan(chip, count, nb)
    return nchunks > 2 * U[case] * nwaves + U[case]


def assert_steps(chip, case, count, nb, tail=False):
    total_blocks, nchunks, want, nwaves = dense_plan(chip, count, nb)
    u = U[case]
    print(f"{case}: count={count} nb={nb} total_blocks={total_blocks} nchunks={nchunks} nwaves={nwaves} U={u} "
          f"bound={2 * u * nwaves + u} nchunks%U={nchunks % u} total_blocks%64={total_blocks % 64}")
    assert total_blocks < 2 ** 32
    assert nchunks > 2 * u * nwaves + u
    if tail:
        assert nchunks % u != 0 or total_blocks % 64 != 0


def assert_full_chip(chip, case, count):
    print(f"{case}: count={count} F={chip.F} second chains={count - chip.F}")
    assert count >= chip.F and count - chip.F >= 64


def assert_kernel(engine, which, name, case):
    got = engine.last_kernel(which)
    print(f"{case}: {got}")
    assert got == name


def assert_same(got_t, exp, what, stride, lead=0):
    got = to_host(got_t)
    assert got.shape == exp.shape
    if np.array_equal(got, exp):
        return
    bad = np.nonzero(got != exp)[0]
    o = int(bad[0]) - lead
    pytest.fail(f"{what}: {len(bad)} bytes differ, first at offset {o + lead}: chain {o // stride}, "
                f"byte {o % stride} (block {(o % stride) // 16}) of its stride")


def plain_image(chip, count, length, stride, total):
    """The destination after a decrypt: every packet's plaintext, every other byte the pattern."""
    exp = chip.pattern[:total].copy()
    exp[:count * stride].reshape(count, stride)[:, :length] = chip.data[:count * stride].reshape(count, stride)[:, :length]
    return exp


def run_decrypt(engine, chip, case, src, exp, count, ks, kw, kernel, inplace, stride):
    import fpnn_amd
    dst = src.clone() if inplace else to_dev(chip.pattern[:len(exp)])
    engine.package_decrypt(dst if inplace else src, dst, count, ks, **kw)
    torch.cuda.synchronize()
    assert_kernel(engine, fpnn_amd.K_DECRYPT, kernel, case)
    assert_same(dst, exp, f"{case} decrypt {'in place' if inplace else 'out of place'}", stride)


def package_round_trip(engine, oracle, chip, case, keylen, length, stride, nkeys, slot_rule, dec_kernel, *,
                       inplace=False, arrays=False):
    import fpnn_amd
    count = chip.COUNT
    assert_full_chip(chip, case, count)
    nb = ceil_div(length, 16)
    assert_steps(chip, case, count, nb, tail=True)
    rng = np.random.default_rng(sum(map(ord, case)) * 100 + keylen)
    total = count * stride + GUARD
    keys = rng.integers(0, 256, nkeys * keylen, dtype=np.uint8)
    ivs = rng.integers(0, 256, nkeys * 16, dtype=np.uint8)
    slots = None
    if slot_rule == "random":
        slots = rng.integers(0, nkeys, count).astype(np.int32)
    elif slot_rule == "modulo":
        # every lane's second chain has its first chain's slot: the grid stride is a multiple of nkeys
        assert chip.F % nkeys == 0
        slots = (np.arange(count) % nkeys).astype(np.int32)
    ks = keyset(engine, keys, keylen, ivs)
    data = chip.data[:total]
    exp_c = chip.pattern[:total].copy()
    t0 = time.perf_counter()
    oracle.package_batch(True, data, exp_c, count, stride=stride, uniform_len=length,
                         key_slot=None if slots is None else slots.astype(np.uint32), keys=keys, keylen=keylen,
                         ivs=ivs, threads=8)
    print(f"{case}: oracle encrypt of {count * length} bytes {time.perf_counter() - t0:.2f} s")
    src = to_dev(data)
    assert src.data_ptr() % 128 == 0  # chain s then starts 16 * (17 * s % 8) bytes into a line (272-byte strides)
    kw = dict(stride=stride, uniform_len=length)
    if slots is not None:
        kw["key_slot"] = to_dev(slots)
    cipher = to_dev(chip.pattern[:total])
    engine.package_encrypt(src, cipher, count, ks, **kw)
    torch.cuda.synchronize()
    assert_kernel(engine, fpnn_amd.K_ENCRYPT, "cfb_encrypt_chains", case)
    assert_same(cipher, exp_c, f"{case} encrypt", stride)
    if arrays:  # offsets as a device array, no len: still K2, LAYOUT_GENERAL with KEY_UNIFORM
        assert slots is None and stride == length
        again = to_dev(chip.pattern[:total])
        engine.package_encrypt(src, again, count, ks, uniform_len=length,
                               in_off=to_dev(np.arange(count, dtype=np.int64) * stride))
        torch.cuda.synchronize()
        assert_kernel(engine, fpnn_amd.K_ENCRYPT, "cfb_encrypt_chains", case + " in_off")
        assert_same(again, exp_c, f"{case} encrypt by in_off", stride)
        del again
    del src
    exp_p = plain_image(chip, count, length, stride, total)
    for ip in ((False, True) if inplace else (False,)):
        run_decrypt(engine, chip, case, cipher, exp_p, count, ks, kw, dec_kernel, ip, stride)


# --------------------------------------------------------------------------------------
# A. round trips at F + F // 4 + 37 chains


@pytest.mark.parametrize("keylen", [16, 24, 32])
def test_r1_line_heads_dense(engine, oracle, chip, keylen):
    """272-byte packets back to back under one key.  Encrypt: LAYOUT_UNIFORM, fenced, 8-block
    chunks; chain s starts 16 * (s % 8) bytes into a 128-byte line, so the head runs 0..7 single
    blocks; of the 17 blocks, heads of 0 and 1 leave two chunks (the prefetch of a real next
    chunk, then of the key table), the others one chunk and singles.  AES-256 once more with the
    offsets as a device array and no `len`.  Decrypt: K1d unaligned, U = 4, prefetched, partial
    last chunk, out of place and in place (the saved boundary blocks beyond the first sweep)."""
    package_round_trip(engine, oracle, chip, "R1", keylen, 272, 272, 1, None, "cfb_decrypt_dense", inplace=True,
                       arrays=keylen == 32)


@pytest.mark.parametrize("keylen", [16, 32])
def test_r2_every_residue_tail(engine, oracle, chip, keylen):
    """301-byte packets back to back: the chains start at every residue mod 16 (no head, chunks on
    unaligned pointers), 18 blocks and a 13-byte tail.  Decrypt: K1 on LAYOUT_UNIFORM, several
    grid strides."""
    package_round_trip(engine, oracle, chip, "R2", keylen, 301, 301, 1, None, "cfb_decrypt_blocks")


def test_r3_stride_gaps(engine, oracle, chip):
    """R1's packets 288 bytes apart (AES-192): the gaps must keep the pattern.  Decrypt: K1 on
    strided LAYOUT_FULL."""
    package_round_trip(engine, oracle, chip, "R3", 24, 272, 288, 1, None, "cfb_decrypt_blocks")


@pytest.mark.parametrize("keylen", [16, 24, 32])
def test_r4a_lane_keys(engine, oracle, chip, keylen):
    """R1's packets with one of 1000 keys each, random slots.  Encrypt: LAYOUT_GENERAL with per-lane
    keys, 4-block chunks, block 0 from the E_k(IV) table, the key reloaded for the second chain.
    Decrypt: K1k beyond the grid cap, out of place and in place."""
    package_round_trip(engine, oracle, chip, "R4a", keylen, 272, 272, 1000, "random", "cfb_decrypt_lanekey",
                       inplace=True)


def test_r4b_lane_keys_kept(engine, oracle, chip):
    """As R4a with 1024 AES-256 keys and slot = s % 1024: 1024 divides the grid stride, so every
    lane's second chain has its first chain's slot and keeps the round keys it holds."""
    package_round_trip(engine, oracle, chip, "R4b", 32, 272, 272, 1024, "modulo", "cfb_decrypt_lanekey")


@pytest.mark.parametrize("keylen", [16, 32])
@pytest.mark.parametrize("per_stream_keys", [False, True])
def test_r5_stream_round_trip(engine, oracle, chip, keylen, per_stream_keys):
    """One 272-byte frame of each of F + F // 4 + 37 streams, by stride / uniform_len, from a
    random (iv, pos) per stream: K2's stream forms (one key, then one key per stream).  The buffers
    start 5 bytes into a line, so the streams at position 5 are 16-byte aligned after their
    position head and run alignment singles before their chunks; the others chunk unaligned.
    The decrypt starts from the same state on whichever kernel the plan picks.  Output and the
    (iv, pos) arrays after each call against the oracle."""
    import fpnn_amd
    case = f"R5[{keylen}{',keyed' if per_stream_keys else ''}]"
    count, length = chip.COUNT, 272
    assert_full_chip(chip, case, count)
    rng = np.random.default_rng(5000 + keylen + per_stream_keys)
    nkeys = count if per_stream_keys else 1
    keys = rng.integers(0, 256, nkeys * keylen, dtype=np.uint8)
    ks = keyset(engine, keys, keylen, rng.integers(0, 256, nkeys * 16, dtype=np.uint8))
    iv0 = rng.integers(0, 256, 16 * count, dtype=np.uint8)
    pos0 = rng.integers(0, 16, count).astype(np.uint32)
    assert np.count_nonzero(pos0 == LEAD) >= 64 and np.count_nonzero(pos0 == 0) >= 64
    offs = np.arange(count, dtype=np.uint64) * length
    lens = np.full(count, length, dtype=np.uint32)
    slots = np.arange(count, dtype=np.uint32) if per_stream_keys else None
    total = count * length
    plain = chip.data[:total]
    okw = dict(in_off=offs, out_off=offs, lens=lens, key_slot=slots, keys=keys, keylen=keylen, threads=8)
    exp, state = {}, {}
    t0 = time.perf_counter()
    for encrypt, inp in ((True, plain), (False, None)):
        inp = exp[True][LEAD:LEAD + total] if inp is None else inp
        image = chip.pattern[:LEAD + total + GUARD].copy()
        iv, pos = iv0.copy(), pos0.copy()
        oracle.stream_batch(encrypt, inp, image[LEAD:], count, iv_state=iv, pos_state=pos, **okw)
        exp[encrypt], state[encrypt] = image, (iv, pos)
    print(f"{case}: oracle encrypt + decrypt of {total} bytes {time.perf_counter() - t0:.2f} s")
    assert np.array_equal(exp[False][LEAD:LEAD + total], plain)  # (the oracle's own round trip)

    kw = dict(stride=length, uniform_len=length)
    if per_stream_keys:
        kw["key_slot"] = to_dev(slots.astype(np.int32))
    src_image = chip.pattern[:LEAD + total + GUARD].copy()
    src_image[LEAD:LEAD + total] = plain
    src = to_dev(src_image)
    assert src.data_ptr() % 128 == 0
    for encrypt in (True, False):
        dst = to_dev(chip.pattern[:LEAD + total + GUARD])
        iv_d, pos_d = to_dev(iv0), to_dev(pos0.astype(np.int32))
        fn = engine.stream_encrypt if encrypt else engine.stream_decrypt
        fn(src[LEAD:], dst[LEAD:], count, ks, iv_d, pos_d, **kw)
        torch.cuda.synchronize()
        if encrypt:
            assert_kernel(engine, fpnn_amd.K_ENCRYPT, "cfb_encrypt_chains", case)
        else:
            print(f"{case}: decrypt on {engine.last_kernel(fpnn_amd.K_DECRYPT)}")
        what = f"{case} {'encrypt' if encrypt else 'decrypt'}"
        assert_same(dst, exp[encrypt], what, length, LEAD)
        bad = np.nonzero((to_host(iv_d) != state[encrypt][0]).reshape(count, 16).any(axis=1))[0]
        assert len(bad) == 0, f"{what}: iv of {len(bad)} streams differs, first {bad[:8]}, pos in {pos0[bad[:8]]}"
        bad = np.nonzero(to_host(pos_d).astype(np.uint32) != state[encrypt][1])[0]
        assert len(bad) == 0, f"{what}: pos of {len(bad)} streams differs, first {bad[:8]}"
        src = dst  # the decrypt reads the ciphertext just written


# --------------------------------------------------------------------------------------
# B. decrypt-only batches sized in sweeps (fewer packets than F)


@pytest.mark.parametrize("case,length,nkeys,keylen", [
    ("D1", 1024, 1, 16), ("D1", 1024, 1, 24),    # K1d aligned, one key (the C2 kernel), tail step
    ("D2", 4096, 97, 16), ("D2", 4096, 97, 24),  # K1d keyed, U = 4
    ("D3", 2048, 97, 32),                        # K1d keyed, U = 2
    ("D4", 3072, 97, 24),                        # K1d keyed, U = 1, beyond the grid cap
])
def test_dense_decrypt_steps(engine, oracle, chip, case, length, nkeys, keylen):
    """Dense whole-chunk packets, the smallest count at which a wave takes a third step: the
    ping-pong prefetch loads the second buffer and then the first again.  D1's count is 3 mod 4,
    so the overhanging tail step (three chunks, the last recomputed) follows the full-step loop
    on the wave it falls to.  D4 (one chunk per step) also asks for more workgroups than CUs.
    Random ciphertext against the oracle's decrypt, out of place and in place (the saved boundary
    blocks of chunks beyond the first sweep); the guard bytes keep the pattern."""
    nb = length // 16
    assert nb % 64 == 0

    def fits(n):
        if not third_step(chip, case, n, nb):
            return False
        if case == "D1":
            return n % 4 == 3
        if case == "D4":
            return dense_plan(chip, n, nb)[2] > chip.CUS
        return True

    count = next(n for n in range(1, chip.F) if fits(n))
    assert count < chip.F
    assert_steps(chip, case, count, nb, tail=case == "D1")
    assert dense_plan(chip, count, nb)[2] >= chip.CUS  # one workgroup per CU: the waves grid-stride
    rng = np.random.default_rng(sum(map(ord, case)) * 100 + keylen)
    total = count * length + GUARD
    keys = rng.integers(0, 256, nkeys * keylen, dtype=np.uint8)
    ivs = rng.integers(0, 256, nkeys * 16, dtype=np.uint8)
    slots = rng.integers(0, nkeys, count).astype(np.int32) if nkeys > 1 else None
    ks = keyset(engine, keys, keylen, ivs)
    data = chip.data[:total]
    exp = chip.pattern[:total].copy()
    oracle.package_batch(False, data, exp, count, stride=length, uniform_len=length,
                         key_slot=None if slots is None else slots.astype(np.uint32), keys=keys, keylen=keylen,
                         ivs=ivs, threads=8)
    kw = dict(stride=length, uniform_len=length)
    if slots is not None:
        kw["key_slot"] = to_dev(slots)
    # in place the 64 bytes behind the batch are the source's own: the pattern there too
    image = chip.pattern[:total].copy()
    image[:count * length] = data[:count * length]
    src = to_dev(image)
    for inplace in (False, True):
        run_decrypt(engine, chip, case, src, exp, count, ks, kw, "cfb_decrypt_dense", inplace, length)
