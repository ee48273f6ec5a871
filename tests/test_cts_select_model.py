"""The model of k_cts_row's select (ctsselref.select_top: 6-bit digits aligned to the top of the range,
exit on a bin of one, at most six passes) against sorted(v)[m // 2], and the exits it is expected to
take; the 8-bit variant that the probe compares it with runs through the same checks."""
import numpy as np
import pytest

import ctsselref

RANGES = [0, 1, 2**8 - 1, 2**8, 2**16, 2**24, 2**32 - 1]
SIZES = [1, 2, 255, 256]


def _check(v, k=None):
    v = [int(x) for x in v]
    k = len(v) // 2 if k is None else k
    bits = (max(v) - min(v)).bit_length()
    for digit in (8, ctsselref.DIGIT):
        got, trail = ctsselref.select_top(v, k, digit)
        assert got == sorted(v)[k], (digit, got, sorted(v)[k], trail)
        assert trail["passes"] <= -(-bits // digit) <= ctsselref.max_passes(digit)
        assert trail["exit"] in ("range0", "one", "shift0")
    return trail


@pytest.mark.parametrize("m", SIZES)
@pytest.mark.parametrize("rng_max", RANGES)
def test_random_multisets_of_every_range(m, rng_max):
    rng = np.random.default_rng(1000 * m + rng_max % 997)
    for rep in range(20):
        base = int(rng.integers(0, 2**32 - rng_max))
        v = base + rng.integers(0, rng_max + 1, m, dtype=np.uint64).astype(object)
        if m >= 2:   # the range is exactly rng_max
            v[0], v[1] = base, base + rng_max
        trail = _check(v)
        if rng_max == 0 or m == 1:
            assert trail["exit"] == "range0" and trail["passes"] == 0
        elif rng_max < 2**ctsselref.DIGIT:
            assert trail["passes"] == 1
        for k in (0, m - 1):
            _check(v, k)


@pytest.mark.parametrize("m", SIZES)
def test_all_equal(m):
    for x in (0, 1, 2**31, 2**32 - 1):
        assert _check([x] * m)["exit"] == "range0"


@pytest.mark.parametrize("m", [2, 255, 256])
@pytest.mark.parametrize("rng_max", RANGES[1:])
def test_duplicates_straddling_rank_k(m, rng_max):
    """count_less <= k < count_less_or_equal with several copies of the answer on both sides of k."""
    rng = np.random.default_rng(m + rng_max % 991)
    k = m // 2
    for dup in (2, 3, m // 2 + 1):
        dup = min(dup, m)
        x = int(rng.integers(0, rng_max + 1))
        first = max(0, min(k - dup // 2, m - dup))   # the copies sit at sorted ranks first .. first + dup - 1, k among them
        below = rng.integers(0, x + 1, first) if first else np.zeros(0, np.int64)
        above = rng.integers(x, rng_max + 1, m - dup - first, dtype=np.uint64) if m - dup - first else np.zeros(0, np.int64)
        v = [int(b) for b in below] + [x] * dup + [int(a) for a in above]
        rng.shuffle(v)
        got, trail = ctsselref.select_top(v, k)
        assert got == x == sorted(v)[k], (got, x, trail)
        if (max(v) - min(v)) >= 2**ctsselref.DIGIT:   # copies of the answer share every bin: no exit on a bin of one
            assert trail["exit"] == "shift0"


def test_exit_on_a_bin_of_one_and_the_last_digit():
    # 14-bit range, distinct top digits: one pass, exit "one"
    v = [i << 8 | 7 for i in range(64)]
    assert _check(v)["exit"] == "one" and _check(v)["passes"] == 1
    # a 22-bit range takes digits of 6, 6, 6 and 4 bits; equal values down to the last digit
    v = [0, 2**22 - 1] + [2**21 + 5] * 100 + [2**21 + 6] * 100
    t = _check(v)
    assert t["exit"] == "shift0" and t["passes"] == 4
    # full 32 bits, every digit needed: six passes (6, 6, 6, 6, 6, 2)
    v = [0, 2**32 - 1] + [2**31 + 1] * 3 + [2**31] * 3
    t = _check(v)
    assert t["exit"] == "shift0" and t["passes"] == 6


def test_against_the_low_aligned_model():
    rng = np.random.default_rng(5)
    for bits in (3, 9, 17, 22, 30, 32):
        v = [int(x) for x in rng.integers(0, 2**bits, 200, dtype=np.uint64)]
        a, ta = ctsselref.select_top(v, 100, 8)
        b, tb = ctsselref.select_low(v, 100)
        assert a == b == sorted(v)[100]
        assert ta["passes"] <= tb["passes"]
