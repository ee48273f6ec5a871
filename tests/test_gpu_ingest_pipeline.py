"""The pipelined ingest of hgx_insert_and_run32: on an empty context the creator
column crosses PCIe first and gives the layout plan, the other structure columns follow in pieces
cut at time-segment boundaries, and each piece is inserted, laid out and its segments'
lastAncestors main pass started while the later pieces are still being copied. Every output must
equal a context that took the serial path on the same columns (and the oracle where n <= 64); a
failed check in any piece gives the serial path's error, accepted prefix and later consensus; a
reused context must not read the previous trace's positions; and the cases the path does not take
stay serial. phase_times()["ingest_pieces"] tells which path ran."""
import numpy as np
import pytest

import hgref
from babble_amd import trace as gtrace
from test_gpu_insert_and_run import _same
from test_gpu_parity import compare

pytestmark = pytest.mark.gpu


def _hg(n, cap, pieces, la=None):
    from babble_amd.hashgraph import Hashgraph
    h = Hashgraph(n, capacity=cap)
    h.set_ingest_pipeline(pieces, 0)
    if la is not None:
        h.set_la_kernel(la)
    return h


def _cols(t):
    from babble_amd.hashgraph import compact_columns
    return compact_columns(t)


def _both(t, pieces, la=None, cols=None, want_pieces=None):
    """The trace through the pipeline and through the serial path; returns the two contexts."""
    cols = _cols(t) if cols is None else cols
    a = _hg(t.n, t.E, pieces, la)
    assert a.insert_and_run32(cols) == t.E
    pa = a.phase_times()
    assert pa["ingest_pieces"] == (pieces if want_pieces is None else want_pieces), pa
    assert pa["la_wave"] == 1 and pa["la_wave_fallbacks"] == 0
    b = _hg(t.n, t.E, 0, la)
    assert b.insert_and_run32(cols) == t.E
    pb = b.phase_times()
    assert pb["ingest_pieces"] == 0
    # (without a forced count the pipeline may take more, shorter time segments than a serial rebuild)
    assert pa["compact"] == pb["compact"] and pa["la_wave_segs"] >= pb["la_wave_segs"] > 1
    assert la is None or pa["la_wave_segs"] == pb["la_wave_segs"] == la
    _same(a, b)
    return a, b


@pytest.mark.parametrize("n,E,la,pieces,seed", [(32, 80000, 8, 4, 31), (64, 120001, None, 2, 32),
                                                (256, 200000, None, 4, 33)])
def test_pipeline_equals_serial_and_oracle(n, E, la, pieces, seed):
    t = gtrace.gossip(n, E, seed, stale_prob=0.2, stale_depth=3)
    a, _ = _both(t, pieces, la)
    if la is not None:
        assert a.phase_times()["la_wave_segs"] == la
    if n <= 64:
        compare(a, hgref.oracle_run(t), t, hashes=False)


def test_int32_coordinates():
    """An odd n keeps int32 coordinates (4-byte column blocks)."""
    t = gtrace.gossip(31, 80000, 34, stale_prob=0.2, stale_depth=3)
    a, _ = _both(t, 4, 8)
    assert a.phase_times()["compact"] == 0
    compare(a, hgref.oracle_run(t), t, hashes=False)


def test_silent_chains():
    """Chains without events: zeros in the histogram, empty slots in the plan."""
    t = gtrace.gossip(32, 80000, 35, n_silent=5, stale_prob=0.2, stale_depth=3)
    a, _ = _both(t, 4, 8)
    compare(a, hgref.oracle_run(t), t, hashes=False)


def test_reused_context_ignores_the_previous_trace():
    """After clear() the positions above a piece's rows still hold trace A's gids: the segment
    bounds of trace B's pieces must not search them."""
    n = 32
    ta = gtrace.gossip(n, 100000, 1, stale_prob=0.2, stale_depth=3)
    tb = gtrace.gossip(n, 70000, 2, stale_prob=0.2, stale_depth=3)
    a = _hg(n, ta.E, 4, 8)
    assert a.insert_and_run32(_cols(ta)) == ta.E
    assert a.phase_times()["ingest_pieces"] == 4
    a.clear()
    assert a.insert_and_run32(_cols(tb)) == tb.E
    assert a.phase_times()["ingest_pieces"] == 4
    b = _hg(n, ta.E, 0, 8)
    assert b.insert_and_run32(_cols(tb)) == tb.E
    _same(a, b)
    compare(a, hgref.oracle_run(tb), tb, hashes=False)


@pytest.mark.parametrize("where", ["inside_piece_0", "first_of_piece_2", "last_event"])
def test_insert_error_is_the_serial_paths(where):
    """A bad other-parent in any piece: message, accepted prefix and the consensus over the prefix
    are those of the two-call path (the pipeline redoes the batch serially)."""
    from babble_amd._lib import HgxError
    n, E, la, pieces = 32, 100000, 8, 4
    k0 = {"inside_piece_0": 12345, "first_of_piece_2": E * 4 // 8, "last_event": E - 1}[where]
    t = gtrace.gossip(n, E, 36, stale_prob=0.2, stale_depth=3)
    cols = _cols(t)
    good_op = cols["op"].copy()
    cols["op"][k0] = -2   # HGX_UNKNOWN_PARENT
    a = _hg(n, E, pieces, la)
    with pytest.raises(HgxError) as ei:
        a.insert_and_run32(cols)
    assert ei.value.msg == "CheckOtherParent: Other-parent not known" and ei.value.inserted == k0
    assert a.num_events() == k0
    assert a.phase_times()["ingest_pieces"] == 0
    a.RunConsensus()
    b = _hg(n, E, 0, la)
    assert b.insert_events32({**cols, "op": good_op}, 0, k0) == k0
    b.RunConsensus()
    _same(a, b)


def test_serial_path_where_the_pipeline_does_not_apply():
    n, E = 32, 160000
    t = gtrace.gossip(n, E, 37, stale_prob=0.2, stale_depth=3)
    cols = _cols(t)
    ref = _hg(n, E, 0, 8)
    assert ref.insert_and_run32(cols) == E
    assert ref.phase_times()["ingest_pieces"] == 0
    # a context that already holds events
    a = _hg(n, E, 4, 8)
    assert a.insert_events32(cols, 0, 70000) == 70000
    assert a.insert_and_run32(cols, 70000, E) == E - 70000
    assert a.phase_times()["ingest_pieces"] == 0
    _same(a, ref)
    # per-kernel timing on
    b = _hg(n, E, 4, 8)
    b.set_kernel_timing(True)
    assert b.insert_and_run32(cols) == E
    assert b.phase_times()["ingest_pieces"] == 0
    _same(b, ref)


def test_page_locked_columns():
    from babble_amd.hashgraph import pinned_columns
    t = gtrace.gossip(64, 120001, 38, stale_prob=0.2, stale_depth=3)
    pc = pinned_columns(_cols(t))
    _both(t, 4, None, cols={k: v for k, v in pc.items() if k != "_buffers"})
