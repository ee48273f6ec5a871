"""Python models of the wave-wide 32-bit selects of hgx_device.h, control flow included.

select_top models wave_select_kth32_top's walk: values rebased to their minimum, digits of `digit`
bits (6 in the kernel) aligned to the top of the range (the last digit takes what is left), the exit
as soon as the chosen bin holds one value, at most ceil(32 / digit) passes. select_low models wave_select_kth32 (digits
aligned to bit 0, no early exit). Both return (value, trail): trail["exit"] names the way out
("range0", "one", "shift0"), trail["passes"] counts histogram passes, trail["active"] lists the values
still active after each pass and trail["maxbin"] the largest count of one bin in each pass (the
degree to which that pass's LDS atomics serialise).

The tests (test_cts_select_model.py) hold select_top against sorted(v)[k]; tools/probe/cts_select_passes.py
runs both over the offsets of a trace.
"""
import numpy as np

DIGIT = 6   # the kernel's: 64 bins, one per lane


def _pass(d, act, shift, mask, k):
    """One histogram pass over the active values: (bucket, values below it, its count, largest bin)."""
    dig = (d[act] >> shift) & mask
    hist = np.bincount(dig, minlength=mask + 1)
    incl = np.cumsum(hist)
    bucket = int(np.searchsorted(incl, k, side="right"))
    below = int(incl[bucket] - hist[bucket])
    return bucket, below, int(hist[bucket]), int(hist.max())


def max_passes(digit=DIGIT):
    return (32 + digit - 1) // digit


def select_top(vals, k, digit=DIGIT):
    v = np.asarray(vals, dtype=np.uint64)
    assert v.size and 0 <= k < v.size and int(v.max()) < 1 << 32
    lo, hi = int(v.min()), int(v.max())
    trail = {"passes": 0, "active": [], "maxbin": [], "exit": None}
    if hi <= lo:
        trail["exit"] = "range0"
        return lo, trail
    d = (v - np.uint64(lo)).astype(np.int64)
    top = (hi - lo).bit_length()
    act = np.ones(v.size, bool)
    prefix = 0
    for _ in range(max_passes(digit)):
        shift = top - digit if top > digit else 0
        mask = (1 << (top - shift)) - 1
        bucket, below, cnt, mx = _pass(d, act, shift, mask, k)
        trail["passes"] += 1
        trail["maxbin"].append(mx)
        k -= below
        prefix |= bucket << shift
        top = shift
        act &= ((d >> shift) & mask) == bucket
        trail["active"].append(int(act.sum()))
        if shift == 0:
            trail["exit"] = "shift0"
            return lo + prefix, trail
        if cnt == 1:
            trail["exit"] = "one"
            return int(v[act][0]), trail
    raise AssertionError("select_top: the digits cover 32 bits")


def select_low(vals, k):
    v = np.asarray(vals, dtype=np.uint64)
    assert v.size and 0 <= k < v.size and int(v.max()) < 1 << 32
    lo, hi = int(v.min()), int(v.max())
    trail = {"passes": 0, "active": [], "maxbin": [], "exit": None}
    if hi == lo:
        trail["exit"] = "range0"
        return lo, trail
    d = (v - np.uint64(lo)).astype(np.int64)
    bits = (hi - lo).bit_length()
    act = np.ones(v.size, bool)
    prefix = 0
    for shift in range(((bits - 1) // 8) * 8, -1, -8):
        bucket, below, _, mx = _pass(d, act, shift, 255, k)
        trail["passes"] += 1
        trail["maxbin"].append(mx)
        k -= below
        prefix |= bucket << shift
        act &= ((d >> shift) & 255) == bucket
        trail["active"].append(int(act.sum()))
    trail["exit"] = "shift0"
    return lo + prefix, trail
