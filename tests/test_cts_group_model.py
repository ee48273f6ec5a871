"""ctsgroupref.select_group (the model of group8_select_kth32_top) against sorted(v)[k] per event and
against ctsselref.select_top: same value, same exit, same passes per event; the common loop runs as long
as its slowest event."""
import numpy as np
import pytest

import ctsgroupref
import ctsselref


def _check(events, vpl=32):
    res, tr = ctsgroupref.select_group(events, vpl)
    worst = 0
    for i, (v, mem) in enumerate(events):
        v = np.asarray(v, dtype=np.uint64)
        mv = v if mem is None else v[np.asarray(mem, bool)]
        if mv.size == 0:
            assert res[i] is None and tr["passes"][i] == 0
            continue
        k = mv.size // 2
        assert res[i] == int(np.sort(mv)[k]), (i, tr)
        want, wt = ctsselref.select_top(mv, k)
        assert res[i] == want
        assert tr["passes"][i] == wt["passes"] and tr["exit"][i] == wt["exit"], (i, tr, wt)
        worst = max(worst, wt["passes"])
    assert tr["loops"] == worst
    return tr


@pytest.mark.parametrize("vpl,nvals", [(32, 256), (32, 201), (16, 100), (8, 64), (8, 33)])
def test_events_of_different_ranges_side_by_side(vpl, nvals):
    """Ranges of 0 to 32 bits inside one group: per-event shift, width and exit, 0 to 6 passes."""
    rng = np.random.default_rng(vpl * 1000 + nvals)
    seen = set()
    for rep in range(40):
        events = []
        for _ in range(8):
            bits = int(rng.integers(0, 33))
            base = int(rng.integers(0, 2**32 - (2**bits - 1)))
            v = base + rng.integers(0, 2**bits, nvals, dtype=np.uint64).astype(np.int64)
            if rng.random() < 0.5:   # two values: no bin of one, ceil(bits / 6) passes
                v = base + np.where(rng.random(nvals) < 0.5, 0, 2**bits - 1).astype(np.int64)
            mem = rng.random(nvals) < rng.choice([0.3, 0.8, 1.0])
            mem[int(rng.integers(nvals))] = True
            events.append((v, mem))
        tr = _check(events, vpl)
        seen.update(tr["passes"])
    assert seen == set(range(7)), seen


def test_absent_events_and_short_groups():
    rng = np.random.default_rng(5)
    v = rng.integers(0, 2**32, 256, dtype=np.uint64).astype(np.int64)
    none = np.zeros(256, bool)
    tr = _check([(v, none), (v, None), (v, none), (v[:7], None), (v[:1], None)])
    assert tr["passes"][0] == tr["passes"][2] == 0 and tr["passes"][4] == 0
    res, tr = ctsgroupref.select_group([(v, none)] * 8)
    assert res == [None] * 8 and tr["loops"] == 0


def test_duplicates_around_the_rank_and_full_range():
    """No exit on a bin of one when the median is repeated; the range 2^32 - 1, where a value that still
    counts equals the 0xffffffff that marks those that do not."""
    rng = np.random.default_rng(9)
    q = (rng.integers(0, 16, 256) << 12).astype(np.int64) + 2**31
    full = rng.integers(0, 2**32, 256, dtype=np.uint64).astype(np.int64)
    full[0], full[1] = 0, 2**32 - 1
    hi = np.full(256, 2**32 - 1, np.int64)
    hi[:100] = 0
    one_hi = np.zeros(256, np.int64)
    one_hi[:129] = 2**32 - 1     # the median is the largest value
    mem = rng.random(256) < 0.5
    mem[:2] = True
    tr = _check([(q, None), (full, None), (hi, None), (one_hi, None), (full, mem), (q, mem)])
    assert tr["exit"][0] == "shift0" and tr["passes"][1] >= 1


@pytest.mark.parametrize("r", [1, 2**5, 2**6, 2**11, 2**12, 2**23, 2**30, 2**31 - 1, 2**31])
def test_two_valued_offsets_beside_a_spread_event(r):
    """The alt shapes of test_gpu_cts_select.py ({0, R}: the digit boundaries) beside a 23-bit event."""
    rng = np.random.default_rng(r % 1000)
    alt = np.where(rng.random(200) < 0.5, 0, r).astype(np.int64) + 2**31 - r // 2
    spread = 2**31 + rng.integers(0, 2**23, 200)
    _check([(alt, None), (spread, None)] * 4)


def test_form_groups_is_the_kernels_mapping():
    pos = np.arange(200)
    tile, grp, slot = ctsgroupref.form_groups(pos)
    assert (tile * 64 + grp + 8 * slot == pos).all()
    assert set(zip(grp[:64].tolist(), slot[:64].tolist())) == {(g, s) for g in range(8) for s in range(8)}
