"""k_seg_sort's register network (hgx_kernels.hip) on buckets of chosen sizes, through the test entry
hgx_seg_sort_check (the production kernels on caller-given buckets): every length around the boundaries
of the network -- a thread's elements, a wave, the wave and the 1 024-thread kernels, EPT 8 -- and key
patterns that make every stage matter, on the one-word path and forced onto the (key, value) path.
The expectation is numpy's lexsort by (key, S bytes) per bucket. The public path is held against the
radix sort and the oracle as tests/test_gpu_sort_seg.py does."""
import numpy as np
import pytest

import hgref
import segsortref as ref
from babble_amd import trace as gtrace

pytestmark = pytest.mark.gpu

WAVE_LENS = [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512]
GROUP_LENS = WAVE_LENS + [513, 1023, 1024, 1025, 2047, 2049, 4095, 4096]
EPT8_LENS = GROUP_LENS + [4097, 8192]
LAUNCHES = {"wave": WAVE_LENS, "group": GROUP_LENS, "ept8": EPT8_LENS}
PATTERNS = ["random", "sorted", "reversed", "equal", "pairs", "topbit", "bit0"]


def _keys(pattern, n, rng):
    if pattern == "random":
        return rng.integers(0, 2**64, n, dtype=np.uint64)
    if pattern == "sorted":
        return np.sort(rng.integers(0, 2**64, n, dtype=np.uint64))
    if pattern == "reversed":
        return np.sort(rng.integers(0, 2**64, n, dtype=np.uint64))[::-1].copy()
    if pattern == "equal":   # one run the size of the bucket
        return np.full(n, 5, np.uint64)
    if pattern == "pairs":
        return rng.permutation(np.arange(n, dtype=np.uint64) // np.uint64(2))
    if pattern == "topbit":
        return rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63)
    if pattern == "bit0":
        return np.uint64(0x1234567800000000) | rng.integers(0, 2, n, dtype=np.uint64)
    raise ValueError(pattern)


def _buckets(lens, keyfn, seed):
    """Buckets of the given lengths in a shuffled order: segoff, keys, vals (a permutation: the S rows), S."""
    rng = np.random.default_rng(seed)
    lens = [lens[i] for i in rng.permutation(len(lens))]
    segoff = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint32)
    m = int(sum(lens))
    keys = np.concatenate([keyfn(n, rng) for n in lens]).astype(np.uint64)
    vals = rng.permutation(m).astype(np.uint32)
    S = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    S[::3, :8] = 7     # equal 8-byte prefixes: the full compare decides
    S[::6, 8:26] = 9   # ... on the last bytes
    assert len({r.tobytes() for r in S}) == m
    return lens, segoff, keys, vals, S


def _expected(lens, segoff, keys, vals, S):
    out = np.empty_like(vals)
    for o, n in zip(segoff.astype(np.int64), lens):
        v, k = vals[o:o + n], keys[o:o + n]
        rows = S[v]
        order = np.lexsort(tuple(rows[:, b] for b in range(31, -1, -1)) + (k,))
        out[o:o + n] = v[order]
    return out


def _check(lens, keyfn, seed, expect_packed=None):
    from babble_amd.hashgraph import seg_sort_check
    lens, segoff, keys, vals, S = _buckets(lens, keyfn, seed)
    want = _expected(lens, segoff, keys, vals, S)
    cap = ref.launch_cap(max(lens))
    key_bits = int(np.bitwise_or.reduce(keys)).bit_length()
    packs = ref.packs(cap, key_bits)
    if expect_packed is not None:
        assert packs == expect_packed
    for force_kv in (False, True):
        got, packed = seg_sort_check(segoff, keys, vals, S, force_kv=force_kv)
        assert packed == (packs and not force_kv), (force_kv, cap, key_bits)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (force_kv, bad[:8], np.searchsorted(segoff, bad[:8], side="right") - 1, lens)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("launch", list(LAUNCHES))
def test_bucket_lengths_and_key_patterns(launch, pattern):
    _check(LAUNCHES[launch], lambda n, rng: _keys(pattern, n, rng), 1300 + 10 * PATTERNS.index(pattern) + len(launch))


@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("launch", list(LAUNCHES))
def test_index_packing_boundary(launch, extra):
    """Keys of exactly 64 - log2 CAP bits, where the index just fits beside them, and of one bit more,
    where the one-word path must not be taken; duplicates among them, so the runs are found on the word."""
    lens = LAUNCHES[launch]
    bits = 64 - (ref.geometry(ref.launch_cap(max(lens)))[2].bit_length() - 1) + extra

    def keyfn(n, rng):
        k = rng.integers(0, 2**(bits - 1), n, dtype=np.uint64) | np.uint64(1 << (bits - 1))
        k[1::4] = k[0::4][:len(k[1::4])]   # (equal keys)
        k[2::8] = np.uint64(2**bits - 1)   # (every key bit set)
        return k

    _check(lens, keyfn, 1400 + bits, expect_packed=extra == 0)


def _run(t, sort="auto", graphs=1, n=None):
    from babble_amd.hashgraph import Hashgraph
    h = Hashgraph(n or t.n, capacity=max(64, t.E), n_graphs=graphs)
    h.set_sort_kernel(sort)
    h.insert_trace(t)
    h.RunConsensus()
    return h


def _same(a, b):
    ra, rb = a.results(), b.results()
    for k in ("round", "witness", "famous", "rr", "cts"):
        assert np.array_equal(np.asarray(ra[k]), np.asarray(rb[k])), k
    assert list(ra["order"]) == list(rb["order"]), "consensus order"


def test_public_path_many_graphs():
    n, G = 16, 32
    traces = [gtrace.gossip(n, 3000 + 100 * g, 1310 + g, stale_prob=0.1 * (g % 3), stale_depth=3) for g in range(G)]
    t = gtrace.concat_graphs(traces)
    hs, hr = _run(t, graphs=G, n=n), _run(t, "radix", graphs=G, n=n)
    assert hs.phase_times()["sort_seg"] >= 1, "the segmented sort did not run"
    assert hr.phase_times()["sort_seg"] == 0
    _same(hs, hr)
    off = 0
    for g, tg in enumerate(traces[:3]):
        o = hgref.oracle_run(tg).results()
        assert list(hs.ConsensusEvents(g) - off) == list(o["order"]), g
        off += tg.E


def test_public_path_256_peers():
    t = gtrace.gossip(256, 60000, 1303, stale_prob=0.0, stale_depth=3)
    hs, hr = _run(t), _run(t, "radix")
    assert hs.phase_times()["sort_seg"] >= 1, "the segmented sort did not run"
    assert hr.phase_times()["sort_seg"] == 0
    _same(hs, hr)
    assert list(hs.results()["order"]) == list(hgref.oracle_run(t).results()["order"])
