"""The lane = voter mapping of k_fame_voter (tests/famemodel.py: vote words by ballot, the witness
mask of round j - 1, coin rounds, per-wave decisions merged lowest chain first) gives the oracle's
fame. Runs without a GPU."""
import numpy as np
import pytest

import famemodel
import hgref
from babble_amd import trace as gtrace


def _check(n, E, seed, silent=0, stale=0.0, XS=64, want_coin=False):
    t = gtrace.gossip(n, E, seed, n_silent=silent, stale_prob=stale, stale_depth=4)
    o = hgref.oracle_run(t)
    LR, wit, wstat, S, see, coin = famemodel.inputs_from_oracle(o, t)
    sm = int(o.L.hgo_super_majority(o.h))
    got, coin_rounds = famemodel.model_fame(n, LR, wstat, S, see, coin, sm, XS=XS)
    want = famemodel.oracle_fame(o, wit)
    assert LR >= 3, "the trace must have rounds that can decide"
    assert np.array_equal(got, want), np.argwhere(got != want)[:10].tolist()
    if want_coin:
        assert coin_rounds > 0, "no coin round reached"
    return want


# n = 2 and 4: (j - i) % n == 0 is reached before every witness is decided
@pytest.mark.parametrize("n,E,seed,stale", [(2, 300, 1, 0.0), (4, 1024, 2, 0.0), (4, 1024, 4, 0.6)])
def test_model_small_n_reaches_coin_rounds(n, E, seed, stale):
    _check(n, E, seed, 0, stale, want_coin=True)


@pytest.mark.parametrize("seed,stale", [(2, 0.3), (7, 0.8)])
def test_model_n3_trace(seed, stale):
    """No trace reaches a coin round at n = 3: the super-majority is 3, so a witness of round i + 1 strongly
    sees (and so sees) all three witnesses of round i and votes yes for each, and a witness of round i + 2
    strongly sees all three of those votes: every x is decided famous at j = i + 2 < i + 3. The coin round of
    n = 3 is covered by test_model_random_inputs instead."""
    want = _check(3, 600, seed, 0, stale)
    assert not (want == 2).any()


@pytest.mark.parametrize("n,R,seed", [(3, 12, 1), (3, 12, 2), (4, 14, 3), (5, 14, 4), (70, 6, 5), (130, 5, 6)])
def test_model_random_inputs(n, R, seed):
    """Arrays that no trace gives: witnesses missing at random, deciders of a round that disagree (the lowest
    chain must win), and coin rounds at n = 3."""
    # (at large n a voter reaches the super-majority only if nearly every chain is a witness and strongly seen)
    wstat, S, see, coin = famemodel.random_inputs(n, R, seed, *((0.85, 0.7) if n < 64 else (0.97, 0.92)))
    sm = 2 * n // 3 + 1
    for LR in (R - 3, R - 1):
        got, _ = famemodel.model_fame(n, LR, wstat, S, see, coin, sm, XS=64 if seed % 2 else 16)
        want, coin_rounds = famemodel.plain_fame(n, LR, wstat, S, see, coin, sm)
        assert np.array_equal(got, want), np.argwhere(got != want)[:10].tolist()
    if n <= 4:
        assert coin_rounds > 0, "no coin round reached"
    assert (want != 0).any(), "nothing decided"


@pytest.mark.parametrize("n,E", [(5, 600), (16, 1500), (64, 5000), (65, 5000), (100, 7000)])
def test_model_word_boundaries(n, E):
    want = _check(n, E, 10 + n)
    assert (want == 1).any(), "no famous witness decided"


@pytest.mark.parametrize("n,E", [(16, 1500), (65, 4000), (100, 6000)])
def test_model_one_third_silent(n, E):
    _check(n, E, 20 + n, silent=n // 3)


@pytest.mark.parametrize("n,E", [(5, 800), (16, 2000), (65, 6000)])
def test_model_stale_other_parents(n, E):
    _check(n, E, 30 + n, stale=0.5)


@pytest.mark.parametrize("XS", [16, 32])
def test_model_narrow_slices(XS):
    """the slice width only splits the x of a round over blocks"""
    _check(65, 4000, 41, silent=5, stale=0.2, XS=XS)
