"""The adversarial addend sets of the exact accumulator (beifong_amd/csrc/bf_sum.h), shared by tests/test_exact_sum_host.py and
tests/test_gpu_exact_sum.py: the smallest inputs at which a fixed-point accumulator and its one rounding can go wrong.  Every set
is (name, cell uint32[n], value float32[n], n_cells); the ones whose result can be written down by hand carry it in EXPECTED."""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
TINY = 2.0 ** -149      # the smallest subnormal: one unit of the accumulator


def _one_cell(values):
    v = np.asarray(values, dtype=np.float64).astype(np.float32)
    assert np.array_equal(v.astype(np.float64), np.asarray(values, dtype=np.float64)), "an addend of a set is not an fp32 number"
    return np.zeros(v.size, np.uint32), v, 1


# name -> (addends, the correctly rounded sum, by hand)
EXPECTED = {
    "cancel_to_tiny": ([FLT_MAX, TINY, -FLT_MAX], TINY),
    "tie_even": ([2.0 ** 24, 1.0], 2.0 ** 24),
    "tie_odd": ([2.0 ** 24 + 2.0, 1.0], 2.0 ** 24 + 4.0),
    "tie_broken": ([2.0 ** 24, 1.0, TINY], 2.0 ** 24 + 2.0),
    "mantissa_carry": ([16777215.0, 0.5, 0.5], 2.0 ** 24),
    "borrow_through": ([2.0 ** 100, -TINY, -2.0 ** 100], -TINY),
    "subnormal_result": ([2.0 ** -126, -TINY], 2.0 ** -126 - TINY),
    "below_overflow": ([FLT_MAX, 2.0 ** 102], FLT_MAX),
    "overflow": ([FLT_MAX, 2.0 ** 103], float("inf")),
}


def _straddle(signs):
    """(2 - 2^-23) 2^k for every k in -126..127: a full mantissa straddles a limb boundary at 23 of every 32 exponents"""
    return [s * (2.0 - 2.0 ** -23) * 2.0 ** k for k in range(-126, 128) for s in signs]


def sets():
    out = [(name, *_one_cell(vals)) for name, (vals, _) in EXPECTED.items()]
    both = _straddle((1.0, -1.0))
    out.append(("straddle_one_cell", *_one_cell(both)))
    c, v, _ = _one_cell(both)
    out.append(("straddle_alternating", (np.arange(v.size, dtype=np.uint32) % 2).astype(np.uint32), v, 2))
    # (alternating cells: cell 0 takes every positive term, cell 1 every negative one)
    out.append(("straddle_positive", *_one_cell(_straddle((1.0,)))))
    n = 1 << 22
    v = np.full(n, FLT_MAX, np.float32)
    v[1::2] = -FLT_MAX
    out.append(("headroom", np.zeros(n, np.uint32), v, 1))
    return out


def orders(cell, value, seed=7):
    """the set as given, reversed and shuffled"""
    p = np.random.default_rng(seed).permutation(value.size)
    return [("given", cell, value), ("reversed", cell[::-1].copy(), value[::-1].copy()), ("shuffled", cell[p], value[p])]


def shuffles(cell, value, n=3, seed=11):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        p = rng.permutation(value.size)
        out.append((cell[p], value[p]))
    return out


def random_bits(rng, n, sign=None):
    """n finite fp32 numbers of uniformly random bit patterns (every exponent, subnormals included); sign: +1, -1 or None (mixed)"""
    bits = rng.integers(0, 1 << 31, size=n, dtype=np.uint64).astype(np.uint32)
    bits = np.where((bits >> np.uint32(23)) == 0xff, bits & np.uint32(0x7f7fffff), bits).astype(np.uint32)      # no inf / nan
    if sign is None:
        bits |= rng.integers(0, 2, size=n, dtype=np.uint64).astype(np.uint32) << np.uint32(31)
    elif sign < 0:
        bits |= np.uint32(0x80000000)
    return bits.view(np.float32)
