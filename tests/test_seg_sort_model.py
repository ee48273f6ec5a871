"""The schedule of k_seg_sort's register network (segsortref): for every bucket size P = 2 .. 8 192 and
every instantiation (GS, EPT) that can meet it, the stages are the bitonic network's, each is done where
the kernel does it (registers, lanes of a wave, LDS across waves), and applying them sorts."""
import numpy as np
import pytest

import segsortref as ref

CAPS = [2 << b for b in range(13)]   # 2 .. 8 192
CASES = [(P, cap) for cap in CAPS if cap >= 64 for P in CAPS if P <= cap]


def _bitonic(P):
    out, k = [], 2
    while k <= P:
        j = k >> 1
        while j:
            out.append((k, j))
            j >>= 1
        k <<= 1
    return out


def test_geometry_of_every_cap():
    for cap in CAPS:
        gs, ept, full = ref.geometry(cap)
        assert gs in ref.GROUPS and ept in (1, 2, 4, 8)
        assert full == max(cap, 64) and full == gs * ept
        assert (gs == 64) == (cap <= 512)
    assert ref.geometry(4096) == (1024, 4, 4096) and ref.geometry(8192) == (1024, 8, 8192)
    assert ref.geometry(512) == (64, 8, 512) and ref.geometry(128) == (64, 2, 128)
    assert [ref.launch_cap(n) for n in (0, 1, 2, 3, 512, 513, 4096, 4097)] == [2, 2, 2, 4, 512, 1024, 4096, 8192]


def test_pack_threshold():
    assert ref.packs(4096, 52) and not ref.packs(4096, 53)
    assert ref.packs(8192, 51) and not ref.packs(8192, 52)
    assert ref.packs(2, 58) and not ref.packs(2, 59)   # (a wave's index takes 6 bits even at a smaller cap)


@pytest.mark.parametrize("P,cap", CASES)
def test_stages_are_the_bitonic_network(P, cap):
    gs, ept, _ = ref.geometry(cap)
    sch = ref.schedule(P, gs, ept)
    assert [(k, j) for k, j, _ in sch] == _bitonic(P)
    for k, j, kd in sch:
        if j < ept:
            assert kd == "thread"
        elif j < 64 * ept:
            assert kd == "wave" and j // ept in (1, 2, 4, 8, 16, 32)
        else:
            assert kd == "lds" and gs == 1024 and j // (64 * ept) in (1, 2, 4, 8)
        # both partners where the stage's kind says: same thread, same wave, another wave
        i = np.arange(P)
        p = ref.partner(i, j)
        assert np.array_equal(np.sort(p), i) and np.array_equal(ref.partner(p, j), i) and np.all(np.abs(p - i) == j)
        same_thread, same_wave = (i // ept) == (p // ept), (i // (64 * ept)) == (p // (64 * ept))
        assert np.all(same_thread == (kd == "thread")) and np.all(same_wave == (kd != "lds"))
        if kd == "wave":
            assert np.all(((i // ept) % 64) ^ (j // ept) == (p // ept) % 64) and np.all(i % ept == p % ept)
        # one partner of a pair keeps the minimum, the other the maximum
        assert np.all(ref.keeps_min(i, k, j) != ref.keeps_min(p, k, j))
        assert np.all(ref.keeps_min(i, k, j) == (((i & k) == 0) == (i < p)))
    if gs == 64:
        assert all(kd != "lds" for _, _, kd in sch)


def test_cross_wave_stages_at_c3():
    sch = ref.schedule(4096, 1024, 4)
    lds = [(k, j) for k, j, kd in sch if kd == "lds"]
    assert len(sch) == 78 and len(lds) == 10
    assert sorted({j for _, j in lds}) == [256, 512, 1024, 2048] and min(k for k, _ in lds) == 512


@pytest.mark.parametrize("P,cap", CASES)
def test_network_sorts(P, cap):
    gs, ept, _ = ref.geometry(cap)
    rng = np.random.default_rng(P * 31 + cap)
    for n in sorted({P, P - 1, P // 2 + 1}):
        if n < 2 or (P > 2 and n <= P // 2):
            continue
        w = rng.integers(0, 2**64, n, dtype=np.uint64)
        got = ref.apply(w, P, gs, ept)
        assert np.array_equal(got[:n], np.sort(w))
        assert np.all(got[n:] == np.iinfo(np.uint64).max)
        # few distinct keys: the (key, value) path keeps every pair and sorts the keys
        keys = rng.integers(0, 4, n, dtype=np.uint64)
        gk, gv = ref.apply_kv(keys, np.arange(n), P, gs, ept)
        assert np.array_equal(gk[:n], np.sort(keys))
        assert np.array_equal(np.sort(gv[:n]), np.arange(n)) and np.array_equal(keys[gv[:n]], gk[:n])
