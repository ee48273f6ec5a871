"""k_cts_row's select (wave_select_kth32_top, hgx_device.h): 6-bit digits aligned to the top of the
range, one bin per lane, the exit on a bin of one, at most six passes.

A gossip trace's timestamps are rewritten so that the offsets ts(FD[x][d]) - ts(x) of an event land
on chosen branches (rr does not depend on the timestamps; the CPU oracle gives the expected medians),
the kernel is forced with set_cts_kernel("row") and every output is compared bit for bit with the
oracle at n = 40 (NPAD 64, four waves, 8 silent peers: every event has non-member chains), n = 100
(NPAD 128) and n = 256; then row against tile at n = 256 on every shape, and two chunked cases
(absent events, short first tiles). An event of an alt shape sees the offsets {0, R} or {-R, 0}, a range
of R. The shapes alt5, alt6, alt11, alt12 and mod61 put the range on and next to the boundaries of 6-bit
digits (6 | 7 and 12 | 13 bits; alt23 has 24 bits, four whole digits); they run at n = 40 and 100 only.

What the shapes reach, counted on the CPU with the model (ctsselref.select_top) over the offsets of
the 5 725 events of gossip(40, 6000, 3, n_silent=8) that all 32 live chains have reached (each of them
counted as a member, firstDescendants by the closed form); the oracle runs every trace (it receives
5 082, 8 948 and 9 370 events at n = 40, 100 and 256). Exits and passes per event:
    equal    range0 5725                    0 passes
    alt5     shift0 5725                    1 pass   (a 6-bit range: one digit)
    alt6     shift0 5725                    2 passes (7 bits: digits of 6 and 1)
    alt7     shift0 5725                    2 passes (8 bits)
    alt11    shift0 5725                    2 passes (12 bits: two whole digits)
    alt12    shift0 5725                    3 passes (13 bits)
    alt15    shift0 5725                    3 passes (16 bits)
    alt23    shift0 5725                    4 passes (24 bits: four whole digits)
    alt30    shift0 5725                    6 passes (31 bits: 6, 6, 6, 6, 6, 1)
    altmax   shift0 5725                    6 passes (31 bits; 2 863 events hold an offset of exactly INT32_MAX)
    alt31    2 863 events in 64 bits (an offset of +2^31), 2 862 in 32 bits (-2^31 fits; shift0, 6 passes):
             even and odd gids alternate along a chain, so the waves of a block meet both kinds
    quant    shift0 5725                    3 passes (equal values around the median: no exit on a bin of one)
    mod251   one 2854, shift0 2871          1 pass 2 854, 2 passes 2 871 (8 bits)
    mod61    shift0 5725                    1 pass
    wide3    every event holds an offset beyond 32 bits (each meets a shifted member): the 64-bit path alone;
             the mix of both kinds inside a block is alt31's
    jitter   one 5725                       1 pass 3 460, 2 passes 2 238, 3 passes 27
    gossip   one 5725 (the plain trace)     1 pass 1 825, 2 passes 3 900
(At 256 chains the plain trace takes 2 passes on 98 % of its events and 3 on the rest:
profiles/r11_cts_select/select_passes.txt.)
"""
import functools

import numpy as np
import pytest

import hgref
from babble_amd import trace as gtrace

pytestmark = pytest.mark.gpu

KT0 = 1_500_000_000_000_000_000


def _alt(r):
    return lambda ts, g: KT0 + (g & 1) * np.int64(r)


SHAPES = {
    "equal": lambda ts, g: np.full(g.size, KT0, np.int64),
    "alt5": _alt(2**5), "alt6": _alt(2**6), "alt11": _alt(2**11), "alt12": _alt(2**12),
    "alt7": _alt(2**7), "alt15": _alt(2**15), "alt23": _alt(2**23), "alt30": _alt(2**30),
    "altmax": _alt(2**31 - 1),      # offsets {-INT32_MAX, 0, INT32_MAX}
    "alt31": _alt(2**31),           # +2^31 does not fit 32 bits, -2^31 does
    "quant": lambda ts, g: KT0 + ((g // 64) << np.int64(12)),
    "mod251": lambda ts, g: KT0 + g % 251,
    "mod61": lambda ts, g: KT0 + g % 61,
    "wide3": lambda ts, g: np.where(g % 3 == 0, ts + (g << np.int64(44)), ts),
    "jitter": lambda ts, g: ts + np.random.default_rng(7).integers(-2**29, 2**29, g.size),
    "gossip": lambda ts, g: ts,
}

SMALL_ONLY = ("alt5", "alt6", "alt11", "alt12", "mod61")   # the 6-bit digit boundaries: n = 40 and 100

# n, E, seed, silent peers
GRAPHS = {40: (40, 6000, 3, 8), 100: (100, 12000, 11, 0), 256: (256, 20000, 16, 0)}


@functools.lru_cache(maxsize=None)
def _trace(n, shape):
    n, E, seed, silent = GRAPHS[n]
    t = gtrace.gossip(n, E, seed, n_silent=silent)
    t.ts = np.ascontiguousarray(SHAPES[shape](np.asarray(t.ts).astype(np.int64), np.arange(E, dtype=np.int64)), np.int64)
    return t


def _run(t, cts, chunk=None):
    from babble_amd.hashgraph import Hashgraph
    h = Hashgraph(t.n, capacity=max(64, t.E))
    try:
        h.set_cts_kernel(cts)
        for lo in range(0, t.E, chunk or t.E):
            h.insert_trace(t, lo, min(t.E, lo + (chunk or t.E)))
            h.RunConsensus()
        return h.results(), h.phase_times()
    finally:
        h.close()


def _compare(a, b):
    for k in ("round", "witness", "famous", "rr", "cts"):
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if not np.array_equal(x, y):
            bad = np.nonzero(x != y)[0][:10]
            raise AssertionError(f"{k} differs at gids {bad.tolist()}: gpu {x[bad].tolist()} expected {y[bad].tolist()}")
    assert list(a["order"]) == list(b["order"]), "consensus order"
    for k in ("last_round", "undecided", "lcr", "lcre", "consensus_tx", "pending_loaded"):
        assert a[k] == b[k], k


@functools.lru_cache(maxsize=None)
def _row(n, shape):
    res, ph = _run(_trace(n, shape), "row")
    assert ph["cts_row"] > 0, "the lane = event timestamp kernel did not run"
    return res


@pytest.mark.parametrize("n,shape", [(n, sh) for n in sorted(GRAPHS) for sh in sorted(SHAPES)
                                     if n < 256 or sh not in SMALL_ONLY])
def test_row_against_oracle(n, shape):
    res = _row(n, shape)
    assert (np.asarray(res["rr"]) >= 0).sum() > GRAPHS[n][1] // 3
    _compare(res, hgref.oracle_run(_trace(n, shape)).results())


@pytest.mark.parametrize("shape", [sh for sh in sorted(SHAPES) if sh not in SMALL_ONLY])
def test_row_equals_tile_at_256_chains(shape):
    tile, ph = _run(_trace(256, shape), "tile")
    assert ph["cts_row"] == 0
    _compare(_row(256, shape), tile)


@pytest.mark.parametrize("shape", ["alt31", "jitter"])
def test_row_chunked_calls(shape):
    """RunConsensus every 1 000 events with the kernel forced: a call receives a few events per chain, so
    most members of a group are absent, and first tiles start off a 32-position boundary."""
    t = _trace(100, shape)
    res, ph = _run(t, "row", chunk=1000)
    assert ph["cts_row"] > 0
    _compare(res, hgref.oracle_run(t, chunk=1000).results())
