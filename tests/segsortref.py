"""A model of k_seg_sort's network schedule (babble_amd/csrc/hgx_kernels.hip): thread t of a group of GS
threads owns the EPT = CAP / GS consecutive elements i = EPT t + e of a bucket padded to the launch's
CAP; a bucket of P <= CAP elements runs the bitonic stages (k, j) of P. A stage is done between a
thread's own registers (j < EPT), between lanes of one wave at distance j / EPT (EPT <= j < 64 EPT) or
through LDS between waves (j >= 64 EPT, 1 024-thread groups only)."""
import numpy as np

WAVE = 64
GROUPS = (64, 1024)       # a wave per bucket (cap <= 512), a workgroup per bucket above
WAVE_CAP_MAX = 512
SORT_CAP = 8192           # kSegSortCap


def launch_cap(max_len):
    """launch_sort_seg's cap: the largest bucket rounded up to a power of two (at least 2)."""
    cap = 2
    while cap < max_len:
        cap <<= 1
    return cap


def geometry(cap):
    """(GS, EPT, CAP) of the instantiation a launch with this cap takes."""
    gs = 64 if cap <= WAVE_CAP_MAX else 1024
    ept = max(1, cap // gs)
    return gs, ept, gs * ept


def packs(cap, key_bits):
    """The one-word path: the key bits that vary in a bucket and the index (log2 CAP bits) fit 64."""
    return key_bits + (geometry(cap)[2].bit_length() - 1) <= 64


def kind(j, ept):
    return "thread" if j < ept else ("wave" if j < WAVE * ept else "lds")


def schedule(P, gs, ept):
    """The stages in the kernel's order: (k, j, kind), for merges k = 2 .. P of a CAP = gs * ept layout."""
    out = []
    logcap = (gs * ept).bit_length() - 1
    for lk in range(logcap):
        k = 2 << lk
        if k <= P:
            for jj in range(lk + 1):
                j = (k >> 1) >> jj
                out.append((k, j, kind(j, ept)))
    return out


def partner(i, j):
    return i ^ j


def keeps_min(i, k, j):
    """The lower element of a pair keeps the minimum in ascending blocks ((i & k) == 0)."""
    return ((i & j) == 0) == ((i & k) == 0)


def apply(words, P, gs, ept):
    """The network on `words` (len <= P), padded with the largest word to CAP as the kernel pads."""
    cap = gs * ept
    a = np.full(cap, np.iinfo(np.uint64).max, np.uint64)
    a[:len(words)] = words
    i = np.arange(cap)
    for k, j, _ in schedule(P, gs, ept):
        b = a[partner(i, j)]
        a = np.where(keeps_min(i, k, j), np.minimum(a, b), np.maximum(a, b))
    return a


def apply_kv(keys, vals, P, gs, ept):
    """The (key, value) path: a pair is replaced by its partner's only on a strict inequality of the keys."""
    cap = gs * ept
    a = np.full(cap, np.iinfo(np.uint64).max, np.uint64)
    v = np.zeros(cap, np.int64)
    a[:len(keys)] = keys
    v[:len(vals)] = vals
    i = np.arange(cap)
    for k, j, _ in schedule(P, gs, ept):
        p = partner(i, j)
        b, vb = a[p], v[p]
        take = np.where(keeps_min(i, k, j), b < a, b > a)
        a, v = np.where(take, b, a), np.where(take, vb, v)
    return a, v
