"""Batched ECDSA P-256 verify on the GPU (hgx_p256_verify_batch, Event.Verify event.go:142-152)
against libcrypto's answers (tests/golden/p256_vectors.txt, oracle/p256_ref.c): valid
signatures, malleated s, digests 0 / N / 2^256-1, single-bit corruptions of digest, r and s,
the wrong key, r or s out of [1, N-1], and public keys that are not curve points; and against
the constructed vectors of tests/golden/p256_edge_vectors.txt (tests/p256ref.py), which reach the
branches no random signature does, at several batch sizes, orders and key layouts."""
import numpy as np
import pytest

from test_p256_fixtures import load_vectors

pytestmark = pytest.mark.gpu


def _batch(rows):
    keys, kid, cols = [], [], ([], [], [])
    for pub, dg, r, s, *_ in rows:
        if pub not in keys:
            keys.append(pub)
        kid.append(keys.index(pub))
        for c, v in zip(cols, (dg, r, s)):
            c.append(np.frombuffer(v, np.uint8))
    return (np.stack([np.frombuffer(k, np.uint8) for k in keys]), np.array(kid, np.int32),
            *[np.stack(c) for c in cols])


def _expected(rows):
    return np.array([e if kok else 2 for _, _, _, _, e, kok, _ in rows], np.uint8)


def test_verify_matches_libcrypto():
    from babble_amd.hashgraph import p256_verify
    rows = load_vectors()
    got = p256_verify(*_batch(rows))
    exp = _expected(rows)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, [(int(i), rows[i][6], int(got[i]), int(exp[i])) for i in bad[:20]]


def test_verify_large_batch_and_bench_entry():
    """Many signatures over few keys (a sync batch), shuffled; the bench entry's results too."""
    from babble_amd.hashgraph import p256_verify, p256_verify_bench
    rows = load_vectors()
    rng = np.random.default_rng(7)
    sel = rng.integers(0, len(rows), 20000)
    big = [rows[i] for i in sel]
    cols = _batch(big)
    exp = _expected(big)
    assert np.array_equal(p256_verify(*cols), exp)
    r = p256_verify_bench(*cols, warmup=1, iters=2)
    assert np.array_equal(r["out"], exp) and r["ms_per_launch"] > 0


@pytest.fixture(scope="module")
def edge():
    """The constructed vectors (tests/golden/p256_edge_vectors.txt; tests/test_p256_edge_fixtures.py
    checks on the CPU that each takes the branch of the kernel its tag names)."""
    from test_p256_edge_fixtures import EDGE
    rows = load_vectors(EDGE)
    return rows, _batch(rows), _expected(rows)


def _check(got, exp, rows, idx):
    bad = np.nonzero(got != exp)[0]
    by_tag = {}
    for i in bad:
        print(f"vector {int(idx[i])} {rows[idx[i]][6]}: got {int(got[i])}, expected {int(exp[i])}")
        by_tag[rows[idx[i]][6]] = by_tag.get(rows[idx[i]][6], 0) + 1
    assert bad.size == 0, f"{bad.size} of {len(exp)} differ, by class: {by_tag}"


def test_edge_vectors_match_reference(edge):
    """The doubling and opposite branches of the mixed addition, the restart from infinity, the final
    infinity, the second compare and its two guards, degenerate keys, every table position alone,
    the ends of the scalar ranges: the whole file in one batch."""
    from babble_amd.hashgraph import p256_verify
    rows, cols, exp = edge
    _check(p256_verify(*cols), exp, rows, np.arange(len(rows)))


@pytest.mark.parametrize("count", [1, 127, 128, 129])
def test_edge_vectors_any_batch_size_and_position(edge, count):
    """A lane's answer depends neither on its neighbours nor on its block (128 lanes, early returns
    per lane): windows of the file at the block size and one either side of it, and for count 1 the
    first vector of every class alone."""
    from babble_amd.hashgraph import p256_verify
    rows, (keys, kid, dg, r, s), exp = edge
    if count == 1:
        first = {}
        for i, row in enumerate(rows):
            first.setdefault(row[6], i)
        wins = [np.array([i]) for i in first.values()]
    else:
        wins = [np.arange(lo, lo + count) for lo in (0, 5, len(rows) - count)]
    for w in wins:
        _check(p256_verify(keys, kid[w], dg[w], r[w], s[w]), exp[w], rows, w)


def test_edge_vectors_reversed(edge):
    from babble_amd.hashgraph import p256_verify
    rows, (keys, kid, dg, r, s), exp = edge
    w = np.arange(len(rows))[::-1]
    _check(p256_verify(keys, kid[w], dg[w], r[w], s[w]), exp[w], rows, w)


def test_key_index_edges(edge):
    from babble_amd.hashgraph import p256_verify
    rows, (keys, kid, dg, r, s), exp = edge
    nk = keys.shape[0]
    idx = np.arange(len(rows))
    # an index below or past the keys is 2 (past the keys lies G's own table), the other lanes keep their answers
    k2, e2 = kid.copy(), exp.copy()
    k2[[0, 130]], e2[[0, 130]] = -1, 2
    k2[[1, 127, len(rows) - 1]], e2[[1, 127, len(rows) - 1]] = nk, 2
    _check(p256_verify(keys, k2, dg, r, s), e2, rows, idx)
    # no keys at all
    assert np.array_equal(p256_verify(np.zeros((0, 65), np.uint8), kid, dg, r, s), np.full(len(rows), 2, np.uint8))
    # the same keys twice: the same answers through either copy
    both = np.concatenate([keys, keys])
    alt = kid + nk * (idx % 2).astype(np.int32)
    _check(p256_verify(both, alt, dg, r, s), exp, rows, idx)
    # one key that is no curve point among the others: 2 for its lanes, nothing else changes
    victim = int(kid[len(rows) // 2])
    assert exp[kid == victim].max() == 1
    bad = keys.copy()
    bad[victim, 64] ^= 1
    _check(p256_verify(bad, kid, dg, r, s), np.where(kid == victim, 2, exp).astype(np.uint8), rows, idx)


def test_empty_and_bad_key_index():
    from babble_amd.hashgraph import p256_verify
    rows = load_vectors()[:4]
    keys, kid, dg, r, s = _batch(rows)
    kid = kid.copy()
    kid[0] = 99   # no such key
    out = p256_verify(keys, kid, dg, r, s)
    assert out[0] == 2
