"""Operand sets for the ECDH field arithmetic, shared by the CPU coverage test
(tests/test_field_folds.py) and the device tests (tests/test_gpu_ecc_field.py).

A special-prime fold takes its rare branches (a final carry, a result in [p, 2^bits), a
top word at the end of its range) with a chance of 2^-32 .. 2^-189 per random product, so
random operands never reach them.  Structured operands do: values one off a power of two,
one off p minus a power of two, p shifted down, and single all-ones limbs, multiplied with
one another.  Everything here is deterministic (seeded), so the branch coverage that
test_field_folds.py asserts for these vectors is the coverage the device tests get.

Plain module (no fixtures), as tests/framing_golden.py."""
import functools
import random

M = 1 << 32
P = {
    "secp256k1": (1 << 256) - (1 << 32) - 977,
    "secp256r1": (1 << 256) - (1 << 224) + (1 << 192) + (1 << 96) - 1,
    "secp224r1": (1 << 224) - (1 << 96) + 1,
    "secp192r1": (1 << 192) - (1 << 64) - 1,
}
NW = {"secp256k1": 8, "secp256r1": 8, "secp224r1": 7, "secp192r1": 6}
CURVES = sorted(P)
PARTNERS = 12       # sampled partners per operand (plus itself, p - 1 and p - 2)
RAW_WORDS = 8192    # raw 2*NW-limb words t < p^2 per curve


def limbs(x, n):
    return [(x >> (32 * i)) & (M - 1) for i in range(n)]


def value(u):
    return sum(int(w) << (32 * i) for i, w in enumerate(u))


@functools.lru_cache(maxsize=None)
def operands(curve):
    """The structured operand set, sorted, every value in [0, p): 2^k + d, p - 2^k + d and
    (p >> k) + d for every bit k and d in {-1, 0, 1}; each single all-ones limb and its
    complement (reduced mod p)."""
    p, nw = P[curve], NW[curve]
    top = 1 << (32 * nw)
    ops = set()
    for k in range(32 * nw + 1):
        for base in (1 << k, p - (1 << k), p >> k):
            for d in (-1, 0, 1):
                if 0 <= base + d < p:
                    ops.add(base + d)
    for i in range(nw):
        ones = (M - 1) << (32 * i)
        ops.add(ones % p)
        ops.add((top - 1 - ones) % p)
    return tuple(sorted(ops))


@functools.lru_cache(maxsize=None)
def product_pairs(curve):
    """(a, b) pairs, a and b < p: every structured operand with PARTNERS sampled partners,
    itself, p - 1 and p - 2."""
    p = P[curve]
    ops = operands(curve)
    rng = random.Random("ecc_vectors pairs " + curve)
    pairs = []
    for a in ops:
        for b in rng.sample(ops, PARTNERS) + [a, p - 1, p - 2]:
            pairs.append((a, b))
    return tuple(pairs)


@functools.lru_cache(maxsize=None)
def raw_words(curve):
    """Raw 2*NW-limb words t < p^2 (as limb lists) with limbs drawn from {0, 1, 2^32 - 1,
    random}: inputs of a fold that no product of two operands below p need equal."""
    p, nw = P[curve], NW[curve]
    rng = random.Random("ecc_vectors raw " + curve)
    out = []
    while len(out) < RAW_WORDS:
        ws = [rng.choice((0, M - 1, M - 1, 1, rng.randrange(M))) for _ in range(2 * nw)]
        if value(ws) < p * p:
            out.append(ws)
    return tuple(tuple(w) for w in out)


@functools.lru_cache(maxsize=None)
def all_carry(curve):
    """Operands whose sums and products carry at every limb: every limb 2^32 - 1 (reduced
    mod p), p - 1, p - 2, each single-limb pattern and its complement, and limbs that
    alternate between 2^32 - 1 and 0."""
    p, nw = P[curve], NW[curve]
    top = 1 << (32 * nw)
    vals = {(top - 1) % p, p - 1, p - 2, 1, top - p, (top - p) - 1}
    for i in range(nw):
        ones = (M - 1) << (32 * i)
        vals |= {ones % p, (top - 1 - ones) % p, (1 << (32 * i)) % p, ((1 << (32 * i + 31)) % p)}
    alt = value([(M - 1) if i % 2 == 0 else 0 for i in range(nw)])
    vals |= {alt % p, (top - 1 - alt) % p}
    return tuple(sorted(vals))


def random_below(curve, count, seed):
    p = P[curve]
    rng = random.Random(f"ecc_vectors random {curve} {seed}")
    return [rng.randrange(p) for _ in range(count)]
