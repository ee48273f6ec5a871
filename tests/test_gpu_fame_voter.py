"""k_fame_voter (the default DecideFame kernel: lane = voter, votes and decisions by ballot) against the
CPU oracle and against the other fame kernels: word and slice boundaries, holes in the witness sets,
word counts that are no power of two, batched graphs, resumed calls, graphs too short to decide."""
import functools

import numpy as np
import pytest

import famemodel
import hgref
from babble_amd import trace as gtrace
from test_gpu_parity import _hg, compare, run_gpu

pytestmark = pytest.mark.gpu

KEYS = ("round", "witness", "famous", "rr", "cts")


@functools.lru_cache(maxsize=None)
def _trace(n, E, seed, silent=0, stale=0.0):
    return gtrace.gossip(n, E, seed, n_silent=silent, stale_prob=stale, stale_depth=4)


@functools.lru_cache(maxsize=None)
def _oracle(n, E, seed, silent=0, stale=0.0):
    return hgref.oracle_run(_trace(n, E, seed, silent, stale))


def _same(a, b, what):
    for k in KEYS:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), f"{what}: {k}"
    assert list(a["order"]) == list(b["order"]), f"{what}: order"
    for k in ("last_round", "undecided", "lcr", "lcre", "consensus_tx"):
        assert a[k] == b[k], f"{what}: {k}"


def _rerun(h, t, tally):
    h.clear()
    h.set_fame_tally(tally)
    h.insert_trace(t)
    h.RunConsensus()
    return h.results()


# a round spans about 14 n events: every case has several decided rounds and two undecided at the end
@pytest.mark.parametrize("n,E,seed", [(1, 300, 1), (2, 300, 1), (3, 600, 2), (4, 1024, 2), (5, 800, 3),
                                      (63, 7000, 4), (64, 7000, 5), (65, 7000, 6), (127, 14000, 7),
                                      (128, 14000, 8), (129, 14000, 9), (192, 22000, 10), (255, 30000, 11),
                                      (256, 30000, 12)])
def test_word_and_slice_boundaries(n, E, seed):
    """n around every multiple of 64 (a wave's last lane, a word's last bit, a slice's last x). n = 2 and 4
    reach coin rounds ((j - i) % n == 0; counted with the CPU model of the same mapping); no trace does at
    n = 3 (tests/test_fame_voter_model.py::test_model_n3_trace says why), and n = 1 decides nothing."""
    t, o = _trace(n, E, seed), _oracle(n, E, seed)
    compare(run_gpu(t), o, t, hashes=False)
    if n in (2, 4):
        LR, wit, wstat, S, see, coin = famemodel.inputs_from_oracle(o, t)
        _, coin_rounds = famemodel.model_fame(n, LR, wstat, S, see, coin, int(o.L.hgo_super_majority(o.h)))
        assert coin_rounds > 0
    if n >= 5:
        assert (o.results()["famous"] == 1).any()


@pytest.mark.parametrize("n,E,seed,silent", [(100, 9000, 21, 33), (256, 30000, 22, 85)])
def test_holes_in_the_witness_sets(n, E, seed, silent):
    """silent peers (chains that never have a witness) and stale other-parents (witnesses that come late)"""
    t, o = _trace(n, E, seed, silent, 0.4), _oracle(n, E, seed, silent, 0.4)
    compare(run_gpu(t), o, t, hashes=False)


@pytest.mark.parametrize("n,seed,Ep", [(300, 31, 12000), (520, 32, 22000)])
def test_word_counts_that_are_no_power_of_two(n, seed, Ep):
    """5 and 9 words per row, one third silent ((n - 1) // 3: one more and no round ever ends, the chains
    that gossip being fewer than the super-majority): the per-round kernel (tally 1) and the witness-tiled
    kernel (tally 3) over all 40 000 events on the same context, the oracle on a prefix. With exactly a
    super-majority gossiping a round takes about 5 000 (n = 300) to 8 000 events, so the prefixes are about
    the shortest with a decided round (at n = 520, 20 000 events decide none)."""
    E, silent = 40000, (n - 1) // 3
    t = _trace(n, E, seed, silent, 0.2)
    h = _hg(n, cap=E)
    got = _rerun(h, t, "popc")
    assert got["last_round"] >= 3 and (got["famous"] == 1).any()
    _same(got, _rerun(h, t, "vote"), "tally 1")
    _same(got, _rerun(h, t, "tile"), "tally 3")
    tp = _trace(n, Ep, seed, silent, 0.2)
    assert np.array_equal(tp.hash, t.hash[:Ep]), "a shorter trace of the same seed is a prefix"
    o = hgref.oracle_run(tp)
    assert (o.results()["famous"] == 1).any()
    compare(run_gpu(tp), o, tp, hashes=False)


@pytest.mark.parametrize("G,n,Es", [(40, 16, 1500), (3, 100, 8000)])
def test_batched_graphs(G, n, Es):
    """the (graph, round, slice) block mapping over a batched context; every graph has its own last round"""
    traces = [gtrace.gossip(n, Es - 37 * g, 400 + g, n_silent=(g % 3) * (n // 8), stale_prob=0.1 * (g % 4),
                            stale_depth=3) for g in range(G)]
    cat = gtrace.concat_graphs(traces)
    h = _hg(n, cap=cat.E, graphs=G)
    h.insert_trace(cat)
    h.RunConsensus()
    _, _, fam = h.rounds()
    off = 0
    for g, t in enumerate(traces):
        o = hgref.oracle_run(t).results()
        assert np.array_equal(fam[off:off + t.E], o["famous"]), g
        assert list(h.ConsensusEvents(g) - off) == list(o["order"]), g
        assert h.UndecidedRounds(g) == o["undecided"], g
        assert h.LastConsensusRound(g) == o["lcr"], g
        off += t.E


def test_resumed_calls():
    """RunConsensus after every 1 000 events: DecideFame starts at the first undecided round with the
    earlier rounds' fame kept. Fame equals the one-shot run's and the oracle's."""
    n, E, seed = 64, 20000, 41
    t = _trace(n, E, seed, 5, 0.2)
    one = run_gpu(t).results()
    h = run_gpu(t, chunk=1000)
    _same(one, h.results(), "chunked")
    compare(h, hgref.oracle_run(t, chunk=1000), t, hashes=False)
    assert np.array_equal(one["famous"], _oracle(n, E, seed, 5, 0.2).results()["famous"])


@pytest.mark.parametrize("n,E", [(4, 10), (16, 120), (64, 700), (130, 1500)])
def test_fewer_than_three_rounds(n, E):
    """no round i has an i + 2: every fame stays undefined"""
    t = _trace(n, E, 51)
    o = hgref.oracle_run(t)
    h = run_gpu(t)
    assert h.LastRound() < 2
    assert not h.results()["famous"].any()
    compare(h, o, t, hashes=False)


@pytest.mark.parametrize("shape", ["256", "40x16"])
def test_all_four_tallies_agree(shape):
    if shape == "256":
        t = _trace(256, 30000, 12)
        h = _hg(256, cap=t.E)
    else:
        t = gtrace.concat_graphs([gtrace.gossip(16, 1500, 600 + g, stale_prob=0.1 * (g % 5), stale_depth=3)
                                  for g in range(40)])
        h = _hg(16, cap=t.E, graphs=40)
    res = {m: _rerun(h, t, m) for m in (0, 1, 2, 3)}
    assert (res[0]["famous"] == 1).any()
    for m in (1, 2, 3):
        for k in KEYS:
            assert np.array_equal(res[0][k], res[m][k]), (m, k)
        assert list(res[0]["order"]) == list(res[m]["order"]), m
