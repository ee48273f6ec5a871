"""Dev probe (CPU): what does the radix select of the consensus timestamps do per event?

The timestamp of x is the upper median of ts(FD[x][d]) - ts(x) over the member chains d. This takes a
c3-shaped trace (256 peers, seed 1) of the project's generator, computes lastAncestors and, by the
closed form, firstDescendants, and runs the models of tests/ctsselref.py over the offsets of every
event that all chains have reached (every chain counted as a member): the select aligned to bit 0
(wave_select_kth32) and the ones aligned to the top of the range with the exit on a bin of one, with
8-bit digits and with 6-bit digits (wave_select_kth32_top). Per variant: passes per event, values still active after each pass, and
the largest count of one bin per pass (how far that pass's LDS atomics serialise). Then the same on
wall-clock-like timestamps: the trace's with a random jitter of +-2^29 ns.

    python tools/probe/cts_select_passes.py [E]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
import ctsselref  # noqa: E402
from babble_amd import trace  # noqa: E402

n = 256
E = int(sys.argv[1]) if len(sys.argv) > 1 else 60000
_, _, _, silent, stale, depth, _ = bench.CONFIGS["c3"]
t = trace.gossip(n, E, 1, n_silent=silent, stale_prob=stale, stale_depth=depth)
cr = np.asarray(t.creator)
idx = np.asarray(t.index)
LA = np.full((E, n), -1, np.int32)
for x in range(E):
    row = LA[x]
    if t.sp[x] >= 0:
        np.maximum(row, LA[t.sp[x]], out=row)
    if t.op[x] >= 0:
        np.maximum(row, LA[t.op[x]], out=row)
    row[cr[x]] = idx[x]
chains = [np.nonzero(cr == c)[0] for c in range(n)]
# firstDescendants by the closed form, as gids: FDg[x][d] = chain d's first event whose LA[.][cr(x)] >= Index(x)
FDg = np.full((E, n), -1, np.int64)
for c in range(n):
    xs = chains[c]
    for d in range(n):
        col = LA[chains[d], c]              # non-decreasing along chain d
        k = np.searchsorted(col, idx[xs], side="left")
        FDg[xs, d] = np.where(k < len(col), chains[d][np.minimum(k, len(col) - 1)], -1)
full = np.nonzero((FDg >= 0).all(axis=1))[0]
print(f"E={E} n={n}: {full.size} events reached by every chain")


def report(name, ts):
    off = ts[FDg[full]] - ts[full][:, None]
    assert off.min() >= -2**31 and off.max() < 2**31
    u = (off + 2**31).astype(np.uint64)
    bits = np.array([int(r.max() - r.min()).bit_length() for r in u])
    print(f"## {name}: range bits of an event's offsets: min {bits.min()} median {int(np.median(bits))} max {bits.max()}")
    for label, fn in (("low-aligned (wave_select_kth32)", ctsselref.select_low),
                      ("top-aligned 8-bit digits, exit on a bin of one", lambda r, k: ctsselref.select_top(r, k, 8)),
                      ("top-aligned 6-bit digits, exit on a bin of one (wave_select_kth32_top)",
                       lambda r, k: ctsselref.select_top(r, k, 6))):
        passes, act, mx, exits = [], [[] for _ in range(6)], [[] for _ in range(6)], {}
        for r in u:
            want = np.sort(r)[n // 2]
            got, tr = fn(r, n // 2)
            assert got == want
            passes.append(tr["passes"])
            exits[tr["exit"]] = exits.get(tr["exit"], 0) + 1
            for p in range(tr["passes"]):
                act[p].append(tr["active"][p])
                mx[p].append(tr["maxbin"][p])
        passes = np.asarray(passes)
        dist = {int(p): int((passes == p).sum()) for p in np.unique(passes)}
        print(f"{label}: passes per event {dist} (mean {passes.mean():.3f}), exits {exits}")
        for p in range(6):
            if act[p]:
                a, m = np.asarray(act[p]), np.asarray(mx[p])
                print(f"   pass {p + 1} ({a.size} events): active after it median {int(np.median(a))} p99 "
                      f"{int(np.percentile(a, 99))} max {a.max()}; largest bin median {int(np.median(m))} p99 "
                      f"{int(np.percentile(m, 99))} max {m.max()}")


ts = np.asarray(t.ts).astype(np.int64)
report("the trace's timestamps", ts)
report("wall-clock-like: + jitter of +-2^29 ns", ts + np.random.default_rng(11).integers(-2**29, 2**29, E))
