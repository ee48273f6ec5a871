"""k_cts_row's phase 2 selects eight events per wave (group8_select_kth32_top, hgx_device.h): groups whose
events differ.

test_gpu_cts_select.py and test_gpu_cts_row.py hold every branch of one select against the oracle, but all
events of a group there are of one kind: a group is the events e = vw + 8s of a tile of 64 positions, which
have the same gid parity. The shapes here change the offset range along a chain instead, so that the eight
events of a group need different numbers of passes, finish at different times, and sit beside events that
need 64 bits (done one wave per event) or have a range of 0:
    ramp   ts = KT0 + ((g & 1) << (5 + (g // 4n) % 28)): the range changes every four positions of a chain
           through 6 .. 33 bits (1 to 6 passes; 2^31 fits as -2^31 only, 2^32 never)
    holes  the same with a constant shift of 20, and all timestamps equal where g // 4n is even
    steep  ramp with g // n for g // 4n: the range changes at every position of a chain and runs through all
           its 28 steps several times at every n (ramp does not get there at n = 100 and 256, see below)
The graphs are test_gpu_cts_select.py's (n = 40 with 8 silent peers: NPAD 64, two groups per wave; n = 100;
n = 256), the kernel is forced with set_cts_kernel("row") and every output is compared bit for bit with the
CPU oracle; then row against tile at n = 256, and ramp at n = 100 in calls of 1 000 events (absent events,
short first tiles, member counts that differ inside a group).

Before the GPU comparison of ramp at n = 40 and 100 and of steep at every n, the model
(ctsgroupref.select_group) runs over the groups exactly as the kernel forms them in one call
(ctsgroupref.form_groups over the positions of a chain; at n = 256 the groups of the first 32 chains), on
the offsets of the events the oracle received, every chain that has reached an event counted as a member
(firstDescendants by the closed form), and has to find
  - two or more different pass counts in at least a quarter of the groups with two or more received events;
  - at least 20 groups that hold both a 64-bit and a 32-bit event.
Counted with the project's traces (groups with >= 2 received events / of them with >= 2 pass counts / groups
with a 64-bit and a 32-bit event; events per pass count 1..6 and in 64 bits):
    ramp  n = 40     749 /   602 /   298    142 1469  994  885  913  252    427
    ramp  n = 100  1 559 / 1 217 /     0    196 1917 2305 2316 2141   73      0
    steep n = 40     749 /   741 /   605    404  525 1041  960  899  352    901
    steep n = 100  1 559 / 1 267 / 1 476      3  452 1639 1769 1719  398  2 968
    steep n = 256    256 /   228 /   246      0   35  168  304  194   32    348   (32 chains)
    holes n = 40: 4 passes on 4 960 events, range 0 on 122; n = 100: 4 passes on all 8 948
ramp's ranges follow g // 4n, and the oracle receives the events below gid 9 000 or so at n = 100 (g // 4n <= 22:
ranges up to 28 bits) and below 9 400 at n = 256 (g // 4n <= 9): no offset there needs 64 bits, so ramp mixes
64-bit and 32-bit events at n = 40 only (a stand-in that counted every event as received found such groups at
n = 100 too: the issue's estimate for this shape was wrong there). ramp's second condition is asserted on its
own at n = 40; at n = 100 it holds only over ramp's two graphs together, that is through n = 40, and steep, which
holds both conditions at every n on its own, is what mixes the two kinds at NPAD 128 and 256.
"""
import functools

import numpy as np
import pytest

import ctsgroupref
import hgref
from babble_amd import trace as gtrace

pytestmark = pytest.mark.gpu

KT0 = 1_500_000_000_000_000_000

# n, E, seed, silent peers (test_gpu_cts_select.py's graphs)
GRAPHS = {40: (40, 6000, 3, 8), 100: (100, 12000, 11, 0), 256: (256, 20000, 16, 0)}


def _ramp(g, n):
    return KT0 + ((g & 1) << (5 + (g // (4 * n)) % 28))


def _holes(g, n):
    return KT0 + np.where((g // (4 * n)) % 2 == 1, (g & 1) << np.int64(20), 0)


def _steep(g, n):
    return KT0 + ((g & 1) << (5 + (g // n) % 28))


SHAPES = {"ramp": _ramp, "holes": _holes, "steep": _steep}


@functools.lru_cache(maxsize=None)
def _trace(n, shape):
    n, E, seed, silent = GRAPHS[n]
    t = gtrace.gossip(n, E, seed, n_silent=silent)
    t.ts = np.ascontiguousarray(SHAPES[shape](np.arange(E, dtype=np.int64), n), np.int64)
    return t


@functools.lru_cache(maxsize=None)
def _oracle(n, shape, chunk=None):
    return hgref.oracle_run(_trace(n, shape), chunk=chunk).results()


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


def _first_descendants(t):
    """FDg[x][d]: gid of chain d's first event that has x among its ancestors, -1 = none yet."""
    E, n = t.E, t.n
    cr, idx = np.asarray(t.creator), np.asarray(t.index)
    LA = np.full((E, n), -1, np.int32)
    for x in range(E):
        row = LA[x]
        if t.sp[x] >= 0:
            np.maximum(row, LA[t.sp[x]], out=row)
        if t.op[x] >= 0:
            np.maximum(row, LA[t.op[x]], out=row)
        row[cr[x]] = idx[x]
    chains = [np.nonzero(cr == c)[0] for c in range(n)]
    FDg = np.full((E, n), -1, np.int64)
    for d in range(n):
        if chains[d].size == 0:
            continue
        for c in range(n):
            xs = chains[c]
            col = LA[chains[d], c]              # non-decreasing along chain d
            k = np.searchsorted(col, idx[xs], side="left")
            FDg[xs, d] = np.where(k < col.size, chains[d][np.minimum(k, col.size - 1)], -1)
    return FDg


@functools.lru_cache(maxsize=None)
def group_census(n, shape, chains=None):
    """The model over the kernel's groups of a one-call run (of the first `chains` chains, None = all):
    (groups with >= 2 received events, those of them with >= 2 different pass counts, groups with a 64-bit
    and a 32-bit event, events per pass count)."""
    t = _trace(n, shape)
    rr = np.asarray(_oracle(n, shape)["rr"])
    ts = np.asarray(t.ts).astype(np.int64)
    FDg = _first_descendants(t)
    cr, idx = np.asarray(t.creator), np.asarray(t.index)
    tile, grp, slot = ctsgroupref.form_groups(idx)
    groups = {}
    for x in np.nonzero((rr >= 0) & (cr < (chains or n)))[0]:
        groups.setdefault((int(cr[x]), int(tile[x]), int(grp[x])), []).append(int(x))
    vpl = (64 if n <= 64 else 128 if n <= 128 else 256) // 8
    multi = mixed = both = 0
    per_pass = {}
    for xs in groups.values():
        narrow, wide = [], 0
        for x in xs:
            mem = FDg[x] >= 0
            off = ts[FDg[x][mem]] - ts[x]
            if off.min() < -2**31 or off.max() >= 2**31:
                wide += 1
            else:
                narrow.append((off + 2**31, None))
        passes = []
        if narrow:
            res, tr = ctsgroupref.select_group(narrow, vpl)
            for (u, _), r in zip(narrow, res):
                assert r == int(np.sort(u)[u.size // 2])
            passes = tr["passes"]
            assert tr["loops"] == max(passes)
            for p in passes:
                per_pass[p] = per_pass.get(p, 0) + 1
        per_pass["64-bit"] = per_pass.get("64-bit", 0) + wide
        if len(xs) >= 2:
            multi += 1
            mixed += len(set(passes)) >= 2
        both += bool(wide and narrow)
    return multi, mixed, both, per_pass


@pytest.mark.parametrize("n,shape", [(n, sh) for n in sorted(GRAPHS) for sh in sorted(SHAPES)])
def test_row_against_oracle(n, shape):
    if shape == "steep" or (shape == "ramp" and n < 256):
        multi, mixed, both, per_pass = group_census(n, shape, 32 if n == 256 else None)
        print(f"n={n} {shape}: {mixed} of {multi} groups with >= 2 received events hold >= 2 pass counts; "
              f"{both} groups hold a 64-bit and a 32-bit event; events per pass count {per_pass}")
        assert 4 * mixed >= multi > 0
        assert sum(per_pass.get(p, 0) > 0 for p in (1, 2, 3, 4, 5, 6)) >= 5, per_pass
        if shape == "ramp" and n == 100:
            # this graph has none of its own (see the docstring), so the condition holds for ramp only over
            # its two graphs together, that is through n = 40; steep is what mixes the two kinds at this n
            both += group_census(40, shape)[2]
        assert both >= 20
    res = _row(n, shape)
    assert (np.asarray(res["rr"]) >= 0).sum() > GRAPHS[n][1] // 3
    _compare(res, _oracle(n, shape))


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_row_equals_tile_at_256_chains(shape):
    tile, ph = _run(_trace(256, shape), "tile")
    assert ph["cts_row"] == 0
    _compare(_row(256, shape), tile)


@pytest.mark.parametrize("shape", ["ramp", "steep"])
def test_row_chunked_calls(shape):
    """RunConsensus every 1 000 events with the kernel forced: a call receives a few events per chain, so most
    events of a group are absent, first tiles start off a 32-position boundary and the member counts of
    the events of a group differ."""
    t = _trace(100, shape)
    res, ph = _run(t, "row", chunk=1000)
    assert ph["cts_row"] > 0
    _compare(res, _oracle(100, shape, 1000))
