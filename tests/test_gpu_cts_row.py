"""The lane = event consensus-timestamp kernel (k_cts_row, hgx_cts.hip; set_cts_kernel "row" / "row1").

Every output against the CPU oracle with the kernel forced (phase_times cts_row tells that it
ran, so a silent fall-back to k_cts_tile fails the test): the three chain paddings, both coordinate
types, the global-memory membership path ("row1": one staged WLAT row, so every tile spanning more
than one round takes it), chunked calls (unaligned first tiles, chains that receive nothing, chains
that went quiet off a tile boundary),
timestamp offsets beyond 32 bits (the 64-bit reselect), timestamps that are not monotone along a
chain, batched graphs; then row against tile at the headline's chain count, and the auto rule.
"""
import functools

import numpy as np
import pytest

import hgref
from babble_amd import trace as gtrace

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _trace(n, E, seed, silent=0, stale=0.0, depth=1):
    return gtrace.gossip(n, E, seed, n_silent=silent, stale_prob=stale, stale_depth=depth)


@functools.lru_cache(maxsize=None)
def _oracle(n, E, seed, silent=0, stale=0.0, depth=1, chunk=None):
    """Oracle results of an unmodified gossip trace, computed once and shared (read only)."""
    return hgref.oracle_run(_trace(n, E, seed, silent, stale, depth), chunk=chunk).results()


def _run(t, cts, chunk=None, coord32=False, graphs=1):
    """(results of every graph, phase_times) of a context that is closed before returning."""
    from babble_amd.hashgraph import Hashgraph
    h = Hashgraph(t.n, capacity=max(64, t.E), n_graphs=graphs)
    try:
        if coord32:
            h.set_coord_storage(1)
        if cts is not None:
            h.set_cts_kernel(cts)
        rows = 0
        for lo in range(0, t.E, chunk or t.E):
            h.insert_trace(t, lo, min(t.E, lo + (chunk or t.E)))
            h.RunConsensus()
            rows = h.phase_times()["cts_row"]
        return [h.results(g) for g in range(graphs)], h.phase_times(), rows
    finally:
        h.close()


def _compare(a, b):
    for k in ("round", "witness", "famous", "rr", "cts"):
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if not np.array_equal(x, y):
            bad = np.nonzero(x != y)[0][:10]
            raise AssertionError(f"{k} differs at gids {bad.tolist()}: gpu {x[bad].tolist()} oracle {y[bad].tolist()}")
    assert list(a["order"]) == list(b["order"]), "consensus order"
    for k in ("last_round", "undecided", "lcr", "lcre", "consensus_tx", "pending_loaded"):
        assert a[k] == b[k], k


@pytest.mark.parametrize("n,E,seed,silent,stale,depth,coord32,compact", [
    (34, 6000, 3, 0, 0.0, 1, False, 1),      # just above k_cts_small, NPAD 64 with padding, compact
    (33, 6000, 5, 0, 0.0, 1, False, 0),      # odd n: int32 coordinates by the storage rule
    (64, 12000, 10, 21, 0.2, 4, False, 1),
    (100, 15000, 11, 0, 0.0, 1, False, 1),   # NPAD 128, n not a multiple of 64
    (130, 15000, 12, 0, 0.0, 1, False, 1),   # NPAD 256 with padding
    (256, 20000, 16, 0, 0.0, 1, False, 1),
    (64, 12000, 10, 21, 0.2, 4, True, 0)])   # int32 on an even n
def test_row_against_oracle(n, E, seed, silent, stale, depth, coord32, compact):
    res, ph, _ = _run(_trace(n, E, seed, silent, stale, depth), "row", coord32=coord32)
    assert ph["cts_row"] > 0, "the lane = event timestamp kernel did not run"
    assert ph["compact"] == compact
    _compare(res[0], _oracle(n, E, seed, silent, stale, depth))


@pytest.mark.parametrize("n,E,seed", [(40, 8000, 4), (256, 20000, 16)])
def test_row1_global_membership_path(n, E, seed):
    """One staged WLAT row: 64 positions span 6.4 and 3.5 rounds on average on these traces, so
    most events read their membership row from global memory."""
    res, ph, _ = _run(_trace(n, E, seed), "row1")
    assert ph["cts_row"] > 0
    _compare(res[0], _oracle(n, E, seed))


def test_row_chunked_calls():
    """RunConsensus every 1 000 events: first tiles that start off a 32-position boundary, short
    tiles, chains with no received event in a call."""
    res, ph, _ = _run(_trace(128, 20000, 12), "row", chunk=1000)
    assert ph["cts_row"] > 0
    _compare(res[0], _oracle(128, 20000, 12, chunk=1000))


def _quiet_trace(n, E, seed, stops):
    """Gossip like hgx_trace_gossip's (an event's other-parent is the head of a random other peer), in
    which peer c of `stops` creates no event after its chain holds stops[c] events; the others keep
    gossiping, with its head still among their other-parents."""
    rng = np.random.default_rng(seed)
    t = gtrace.GossipTrace(
        n=n, creator=np.zeros(E, np.int32), index=np.zeros(E, np.int64), sp=np.full(E, -1, np.int64),
        op=np.full(E, -1, np.int64), ts=1_500_000_000_000_000_000 + 1000 * np.arange(E, dtype=np.int64),
        hash=rng.integers(0, 256, (E, 32), dtype=np.uint8), s=rng.integers(0, 256, (E, 32), dtype=np.uint8),
        ntx=np.zeros(E, np.int32), txnil=np.zeros(E, np.int32), tx_seq=np.full(E, -1, np.int64))
    head, length = [-1] * n, [0] * n
    t.txnil[:n] = 1
    for e in range(E):
        if e < n:
            to, op = e, -1
        else:
            to = int(rng.integers(n))
            while length[to] >= stops.get(to, E):
                to = int(rng.integers(n))
            frm = int(rng.integers(n - 1))
            frm += frm >= to
            op = head[frm]
        t.creator[e], t.index[e], t.sp[e], t.op[e] = to, length[to], head[to], op
        head[to], length[to] = e, length[to] + 1
    return t


def test_row_chains_that_stop_off_a_tile_boundary():
    """Peers that go quiet with 33, 45 and 95 events: once their last events are received, every later
    call finds nothing new on those chains at an fu that is no multiple of 32. Such a chain's first
    block holds no event and must load nothing (the positions past a chain's end hold no
    firstDescendants)."""
    stops = {3: 33, 17: 45, 40: 95}
    t = _quiet_trace(64, 12000, 77, stops)
    res, ph, _ = _run(t, "row", chunk=1000)
    assert ph["cts_row"] > 0
    o = hgref.oracle_run(t, chunk=1000).results()
    _compare(res[0], o)
    rr = np.asarray(o["rr"])
    for c in stops:   # the quiet chains are received in full well before the end: many calls run on them empty
        mine = np.nonzero(t.creator == c)[0]
        assert len(mine) == stops[c] and (rr[mine] >= 0).all() and rr[mine].max() < rr.max() - 3


def _wide(t, step_log2, every=1):
    ts = t.ts.copy()
    g = np.arange(t.E, dtype=np.int64)
    sel = (g % every) == 0
    ts[sel] = ts[sel] + (g[sel] << np.int64(step_log2))
    t.ts = ts
    return t


@pytest.mark.parametrize("n,E,seed,step,every", [
    (64, 12000, 201, 46, 1),     # every offset beyond 32 bits: the 64-bit reselect on every event
    (256, 20000, 204, 44, 3)])   # mixed
def test_row_wide_timestamps(n, E, seed, step, every):
    t = _wide(gtrace.gossip(n, E, seed, stale_prob=0.1, stale_depth=3), step, every)
    res, ph, _ = _run(t, "row")
    assert ph["cts_row"] > 0
    _compare(res[0], hgref.oracle_run(t).results())


def test_row_timestamps_not_monotone_along_chains():
    """Monotone firstDescendants and timestamps may serve locality only, never correctness."""
    t = gtrace.gossip(64, 12000, 21)
    t.ts = t.ts + np.random.default_rng(7).integers(-5_000_000, 5_000_000, t.E)
    res, ph, _ = _run(t, "row")
    assert ph["cts_row"] > 0
    _compare(res[0], hgref.oracle_run(t).results())


def test_row_batched_graphs():
    traces = [gtrace.gossip(64, 6000, 30 + g, stale_prob=0.1 * g, stale_depth=3) for g in range(3)]
    res, ph, _ = _run(gtrace.concat_graphs(traces), "row", graphs=3)
    assert ph["cts_row"] > 0
    off = 0
    for g, t in enumerate(traces):
        o = hgref.oracle_run(t).results()
        a = res[g]
        sl = slice(off, off + t.E)
        for k in ("round", "witness", "famous", "rr", "cts"):
            assert np.array_equal(np.asarray(a[k])[sl], np.asarray(o[k])), (g, k)
        assert list(np.asarray(a["order"]) - off) == list(o["order"]), g
        assert a["undecided"] == o["undecided"] and a["lcr"] == o["lcr"] and a["last_round"] == o["last_round"], g
        off += t.E


@pytest.fixture(scope="module")
def c3_shaped():
    """n = 256, 200 000 events in one call under each setting: (rr, cts, order, FindOrders on the row kernel)."""
    from babble_amd.hashgraph import Hashgraph
    t = gtrace.gossip(256, 200_000, 1)
    out = {}
    for mode in (None, "tile", "row"):
        h = Hashgraph(256, capacity=t.E)
        try:
            if mode:
                h.set_cts_kernel(mode)
            h.insert_trace(t)
            h.RunConsensus()
            rr, cts = h.received()
            out[mode] = (rr.copy(), cts.copy(), h.ConsensusEvents().copy(), h.phase_times()["cts_row"])
        finally:
            h.close()
    return out


def test_row_equals_tile_at_256_chains(c3_shaped):
    tile, row = c3_shaped["tile"], c3_shaped["row"]
    assert tile[3] == 0 and row[3] == 1
    assert (tile[0] >= 0).sum() > 150_000
    for k in range(3):
        assert np.array_equal(tile[k], row[k]), ("rr", "cts", "order")[k]


def test_auto_runs_the_row_kernel_on_a_batch_call(c3_shaped):
    auto, row = c3_shaped[None], c3_shaped["row"]
    assert auto[3] == 1
    for k in range(3):
        assert np.array_equal(auto[k], row[k]), ("rr", "cts", "order")[k]


def test_auto_keeps_the_tile_kernel_on_small_calls():
    """1 000 events per call over 256 chains: a handful of received events per chain."""
    _, ph, rows = _run(_trace(256, 20000, 16), None, chunk=1000)
    assert ph["cts_row"] == 0 and rows == 0
