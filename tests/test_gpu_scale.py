"""Parity at the headline configuration's shape and on the paths small traces never reach.

* C3-shaped: 256 peers, 200k events (chains ~780 long, 57 rounds), compact uint16
  coordinates, the n <= 256 round step, k_cts_tile at n = 256 -- every output against the
  oracle (the oracle needs ~1 min here; bench.py --full adds the full-size property checks).
* Timestamps so far apart that the (graph, rr, cts - min) sort key needs more than 64 bits
  (two-pass sort, hgx_engine.cpp find_order) and the consensus-timestamp offsets overflow
  32 bits (k_cts_tile's 64-bit reselect), alone and mixed with ordinary events.
"""
import numpy as np
import pytest

import hgref
from babble_amd import trace as gtrace

pytestmark = pytest.mark.gpu


def _run(t, cap=None, cts=None):
    from babble_amd.hashgraph import Hashgraph
    h = Hashgraph(t.n, capacity=cap or t.E)
    if cts:
        h.set_cts_kernel(cts)
    h.insert_trace(t)
    h.RunConsensus()
    return h


def _compare(h, o):
    a, b = h.results(), o.results()
    for k in ("round", "witness", "famous", "rr", "cts"):
        if not np.array_equal(np.asarray(a[k]), np.asarray(b[k])):
            bad = np.nonzero(np.asarray(a[k]) != np.asarray(b[k]))[0][:10]
            raise AssertionError(f"{k} differs at gids {bad.tolist()}")
    assert list(a["order"]) == list(b["order"]), "consensus order"
    for k in ("last_round", "undecided", "lcr", "lcre", "consensus_tx", "pending_loaded"):
        assert a[k] == b[k], k
    assert [(x["rr"], x["ntx"], x["tx_nil"]) for x in a["blocks"]] == [(x[0], x[1], x[2]) for x in b["blocks"]]
    return b


def _block_hashes(h, t):
    """Go-JSON block hashes (SHA256(json(Block)), block.go:26-53) of the GPU's blocks, with the
    transactions of the GPU's own order (hgx_block_hash)."""
    from babble_amd.hashgraph import block_hash
    order = h.ConsensusEvents()
    out = []
    for b in h.Blocks():
        txs = []
        for g in order[b["first"]:b["first"] + b["n_events"]]:
            txs.extend(t.txs(int(g)) or [])
        out.append(block_hash(b["rr"], txs, b["tx_nil"]))
    return out


def test_c3_shaped_long_chains():
    t = gtrace.gossip(256, 200_000, 1)
    h = _run(t)
    assert h.phase_times()["compact"] == 1
    b = _compare(h, hgref.oracle_run(t))
    assert b["last_round"] >= 50 and len(b["order"]) > 150_000
    assert _block_hashes(h, t) == [x[4] for x in b["blocks"]], "block hashes"


def test_c5_shaped_341_silent_peers_live():
    """BASELINE configs[4] names 1/3 silent peers: at n = 1024, 341 = n - SM silent peers is the
    most that still lets rounds advance: every StronglySee then needs all 683
    active coordinates, so a round takes ~20k events. bench.py's c5 line runs 300 silent; this
    is the 341 case. Oracle parity on a 25k-event prefix (rounds 0-2; the oracle's n^3 loops
    take ~30 s there), then 400k events on the GPU alone: rounds must stay live, fame must
    decide and events must be ordered, with bench.py's full-size order properties."""
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    tp = gtrace.gossip(1024, 25_000, 5, n_silent=341)
    _compare(_run(tp), hgref.oracle_run(tp))
    t = gtrace.gossip(1024, 400_000, 5, n_silent=341)
    h = _run(t)
    lr, lcr = h.LastRound(), h.LastConsensusRound()
    assert lr >= 15, lr
    assert lcr is not None and lcr >= lr - 6, (lr, lcr)
    assert len(h.ConsensusEvents()) > 200_000
    assert bench.full_size_checks(h, t, 1)["result"] == "pass"


def _wide(t, step_log2, every=1):
    ts = t.ts.copy()
    g = np.arange(t.E, dtype=np.int64)
    sel = (g % every) == 0
    ts[sel] = ts[sel] + (g[sel] << np.int64(step_log2))
    t.ts = ts
    return t


@pytest.mark.parametrize("n,E,seed,step,every", [
    (64, 12000, 201, 46, 1),    # ~60-bit cts range: key > 64 bits, every offset > 32 bits
    (64, 12000, 202, 40, 97),   # mixed: a few far-future events among ordinary ones
    (16, 4000, 203, 46, 1),     # n <= 32 (k_cts_small) with the two-pass sort
    (256, 20000, 204, 44, 3)])  # n = 256 tile path
def test_wide_timestamps(n, E, seed, step, every):
    t = _wide(gtrace.gossip(n, E, seed, stale_prob=0.1, stale_depth=3), step, every)
    h = _run(t)
    b = _compare(h, hgref.oracle_run(t))
    rr = np.asarray(b["rr"])
    cts = np.asarray(b["cts"])[rr >= 0]
    span = int(cts.max()) - int(cts.min()) if cts.size else 0
    assert len(b["order"]) > 0
    if every == 1:
        assert span.bit_length() + int(rr.max()).bit_length() > 64 or span.bit_length() > 56


@pytest.mark.parametrize("n,E,seed,step,every", [(64, 12000, 201, 46, 1), (256, 20000, 204, 44, 3)])
def test_wide_timestamps_pipelined_cts(n, E, seed, step, every):
    """The pipelined timestamp kernel's 64-bit redo pass (k_cts_redo) on offsets beyond 32 bits."""
    t = _wide(gtrace.gossip(n, E, seed, stale_prob=0.1, stale_depth=3), step, every)
    _compare(_run(t, cts="pipe"), hgref.oracle_run(t))
