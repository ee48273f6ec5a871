"""hgx_insert_and_run32 with the device kept fed between its phases: the pipelined
ingest's copier goes on with the payload right behind the last structure piece, the payload's first
columns are committed inside DivideRounds (ahead of the rounds, not between the recurrence and
DecideFame), DecideFame's device pass is launched from DivideRounds' bookkeeping, and the host loops
over the rounds are single passes over raw rows. None of it may change a result: every output equals
the serial path, the two-call path and the oracle; a failed check leaves no early payload write and no
copier behind; a reused context shows nothing of the previous trace's S or staging columns."""
import numpy as np
import pytest

import hgref
from babble_amd import trace as gtrace
from test_gpu_ingest_pipeline import _cols, _hg
from test_gpu_insert_and_run import _same
from test_gpu_parity import compare

pytestmark = pytest.mark.gpu


def _mixed(t, every=7):
    """Body.Transactions == nil on every 7th event (ntx = -1 in the compact columns) and a zero coin
    byte (byte 16 of the event id) on every third: the generator alone gives neither."""
    nil, ntx, h = t.txnil.copy(), t.ntx.copy(), t.hash.copy()
    k = np.arange(0, t.E, every)
    nil[k], ntx[k] = 1, 0
    h[np.arange(0, t.E, 3), 16] = 0
    return gtrace.GossipTrace(**{**t.__dict__, "txnil": nil, "ntx": ntx, "hash": h})


def _trace(n, E, seed, **kw):
    kw = {"stale_prob": 0.2, "stale_depth": 3, **kw}
    return _mixed(gtrace.gossip(n, E, seed, **kw))


def _run32(h, cols, pieces):
    assert h.insert_and_run32(cols) == len(cols["creator"])
    ph = h.phase_times()
    assert ph["ingest_pieces"] == pieces, ph
    return h


_ORACLE = {}


def _oracle(key, t):
    """One oracle run per trace, shared by the tests that use the trace."""
    if key not in _ORACLE:
        _ORACLE[key] = hgref.oracle_run(t)
    return _ORACLE[key]


@pytest.mark.parametrize("n,E,pieces,la,seed", [(32, 80000, 4, 8, 41), (64, 120001, 2, None, 42), (16, 70000, 3, 8, 43)])
def test_piped_equals_serial_and_oracle(n, E, pieces, la, seed):
    """n = 16: equal consensus timestamps are common, so the sort's S tie-break reads the S column the
    copier wrote straight into the store."""
    t = _trace(n, E, seed)
    cols = _cols(t)
    assert 0 < int(cols["coin"].sum()) < E and int((cols["ntx"] < 0).sum()) > 0
    a = _run32(_hg(n, E, pieces, la), cols, pieces)
    b = _run32(_hg(n, E, 0, la), cols, 0)
    _same(a, b)
    compare(a, _oracle((n, E, seed), t), t, hashes=False)


@pytest.mark.parametrize("frac", [0.9, 0.05])
def test_failed_check_leaves_nothing_behind(frac):
    """A bad other-parent in the last piece and in the first: error, accepted prefix and the consensus
    over it are a serial context's; after clear() the same context runs a clean trace like a fresh one."""
    from babble_amd._lib import HgxError
    n, E, la, pieces = 32, 80000, 8, 4
    k0 = int(E * frac)
    t = _trace(n, E, 44)
    cols = _cols(t)
    bad = {**cols, "op": cols["op"].copy()}
    bad["op"][k0] = -2   # HGX_UNKNOWN_PARENT
    a, b = _hg(n, E, pieces, la), _hg(n, E, 0, la)
    errs = []
    for h in (a, b):
        with pytest.raises(HgxError) as ei:
            h.insert_and_run32(bad)
        errs.append((ei.value.msg, ei.value.code, ei.value.inserted))
        assert h.num_events() == k0 and h.phase_times()["ingest_pieces"] == 0
        h.RunConsensus()
    assert errs[0] == errs[1] == ("CheckOtherParent: Other-parent not known", errs[1][1], k0)
    _same(a, b)
    t2 = _trace(n, E, 45)
    c2 = _cols(t2)
    a.clear()
    _run32(a, c2, pieces)
    _same(a, _run32(_hg(n, E, pieces, la), c2, pieces))


def test_reused_context_after_a_longer_trace():
    """The store's S column and the staging columns beyond the new batch still hold the longer
    trace's values: none may show."""
    n, la, pieces = 32, 8, 4
    ta, tb = _trace(n, 120000, 46), _trace(n, 80000, 47)
    tb = gtrace.GossipTrace(**{**tb.__dict__, "ts": tb.ts + 777})   # (the generator's timestamps do not depend on the seed)
    assert not np.array_equal(ta.s[:tb.E], tb.s) and not np.array_equal(ta.ts[:tb.E], tb.ts)
    a = _run32(_hg(n, ta.E, pieces, la), _cols(ta), pieces)
    a.clear()
    _run32(a, _cols(tb), pieces)
    _same(a, _run32(_hg(n, ta.E, pieces, la), _cols(tb), pieces))


def test_pinned_and_pageable_columns():
    from babble_amd.hashgraph import pinned_columns
    n, E, pieces = 64, 120001, 4
    t = _trace(n, E, 42)
    cols = _cols(t)
    pc = pinned_columns(cols)
    a = _run32(_hg(n, E, pieces), {k: v for k, v in pc.items() if k != "_buffers"}, pieces)
    _same(a, _run32(_hg(n, E, pieces), cols, pieces))
    compare(a, _oracle((n, E, 42), t), t, hashes=False)


def test_split_path_without_the_pipeline():
    """The commit moved into DivideRounds and the rewritten layout timestamps on the split path: one
    graph, and a batch of graphs (which never takes the pipeline)."""
    n, E = 32, 80000
    cols = _cols(_trace(n, E, 48))
    a = _run32(_hg(n, E, 0), cols, 0)
    b = _hg(n, E, 0)
    assert b.insert_events32(cols) == E
    b.RunConsensus()
    _same(a, b)
    from babble_amd.hashgraph import Hashgraph
    G = 8
    t = _mixed(gtrace.concat_graphs([gtrace.gossip(16, 16384, 90 + g, stale_prob=0.2, stale_depth=3) for g in range(G)]))
    cols = _cols(t)
    a, b = Hashgraph(16, capacity=t.E, n_graphs=G), Hashgraph(16, capacity=t.E, n_graphs=G)
    _run32(a, cols, 0)
    assert b.insert_events32(cols) == t.E
    b.RunConsensus()
    _same(a, b, graphs=G)


@pytest.mark.parametrize("calls", [1, 4])
def test_bookkeeping_with_an_undecided_tail(calls):
    """10 of 32 peers silent (the super-majority needs every live one) and 30 % stale other-parents:
    rounds stay undecided at the end. The undecided queue, LastConsensusRound, LastCommitedRoundEvents,
    every witness' fame, the blocks and the counters equal the oracle fed the same way."""
    n, E = 32, 80000
    t = _mixed(gtrace.gossip(n, E, 49, n_silent=10, stale_prob=0.3, stale_depth=3))
    cols = _cols(t)
    a = _hg(n, E, 4, 8)
    o = hgref.Oracle(n)
    for k in range(calls):
        lo, hi = E * k // calls, E * (k + 1) // calls
        assert a.insert_and_run32(cols, lo, hi) == hi - lo
        o.insert_trace(t, lo, hi)
        o.run_consensus()
    assert a.phase_times()["ingest_pieces"] == (4 if calls == 1 else 0)
    assert len(a.UndecidedRounds()) > 0
    compare(a, o, t, hashes=False)
    assert a.LastConsensusRound() == o.last_consensus_round() and a.UndecidedRounds() == o.undecided_rounds()
