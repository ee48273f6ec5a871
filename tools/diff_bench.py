"""Dev tool: measurements of hgx_diff_wire on one GPU.

  python tools/diff_bench.py call [--n 256] [--events 200000 2000000] [--behind 1000] [--reps 50]
                                  [--repeats 3] [--out file.json]
  python tools/diff_bench.py once [--n 256] [--events 2000000] [--calls 20]   (run it under
                                  rocprofv3 --kernel-trace --stats: the kernels' device time)

call: host clock around the bare C calls (each ends in a device synchronise) of three ways to answer
      the same SyncRequest, a `known` vector `behind` events back, alternating in one process:
        diff_wire    hgx_diff_wire with all twelve columns;
        parent_cold  the route without it, the host mirror dropped by a one-event hgx_insert_events
                     just before: hgx_known + n x hgx_participant_events + a host sort +
                     hgx_wire_info over the gid range + hgx_get_event per event (there is no bulk
                     getter for S and the ids, so this route returns less);
        parent_warm  the same again with the mirror in place.
      Every repeat inserts one event (so the diff grows by one); the order of the new call and the
      parent's route flips every repeat. The whole measurement runs `repeats` times: the spread of
      the medians is the run-to-run spread. The answers are compared once per size.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from babble_amd import _lib  # noqa: E402
from babble_amd import trace as gtrace  # noqa: E402
from babble_amd._lib import hgx_error, ptr  # noqa: E402
from babble_amd.hashgraph import Hashgraph  # noqa: E402

BYTES_PER_RESIDENT_EVENT = 16   # creator and Index (4 + 4 bytes), read by k_diff_count and by k_diff_gather


def build(t, E, cap, chunk=1 << 18):
    h = Hashgraph(t.n, capacity=cap)
    for lo in range(0, E, chunk):
        h.insert_trace(t, lo, min(E, lo + chunk))
    return h


def known_behind(t, E, behind):
    k = np.full(t.n, -1, np.int32)
    np.maximum.at(k, t.creator[:max(E - behind, 0)], t.index[:max(E - behind, 0)].astype(np.int32))
    return k


class DiffCall:
    """hgx_diff_wire through the bare binding on arrays allocated once"""

    def __init__(self, h, rows):
        self.h = h
        self.rows = rows
        self.cols = {nm: np.zeros((rows,) + shp, dt) for nm, dt, shp in _lib.WIRE_OUT_COLUMNS}
        self.out = _lib.hgx_wire_out(**{nm: ptr(a) for nm, a in self.cols.items()})
        self.cnt, self.over, self.err = C.c_int64(), C.c_int32(), hgx_error()

    def __call__(self, known):
        t0 = time.perf_counter()
        rc = self.h.L.hgx_diff_wire(self.h.ctx, 0, ptr(known), -1, C.byref(self.out), self.rows, C.byref(self.cnt),
                                    C.byref(self.over), C.byref(self.err))
        ms = (time.perf_counter() - t0) * 1e3
        _lib.check(rc, self.err)
        return ms, self.cnt.value


class ParentRoute:
    """What a shim does without hgx_diff_wire, through the bare binding"""

    def __init__(self, h, rows, E_max):
        self.h, self.n = h, h.n
        self.own = np.zeros(h.n, np.int32)
        self.gids = np.zeros(rows, np.int64)
        self.spi, self.opc, self.opi = (np.zeros(E_max, np.int32) for _ in range(3))
        self.ts = np.zeros(rows, np.int64)
        self.ntx, self.nil = np.zeros(rows, np.int32), np.zeros(rows, np.int32)

    def __call__(self, known):
        L, ctx, err = self.h.L, self.h.ctx, hgx_error()
        cnt = C.c_int64()
        ts, nt, nil = C.c_int64(), C.c_int32(), C.c_int32()
        t0 = time.perf_counter()
        L.hgx_known(ctx, 0, ptr(self.own))
        m = 0
        for p in range(self.n):
            rc = L.hgx_participant_events(ctx, p, int(known[p]), ptr(self.gids[m:]), len(self.gids) - m, C.byref(cnt),
                                          C.byref(err))
            _lib.check(rc, err)
            m += cnt.value
        g = np.sort(self.gids[:m])
        if m:
            first, count = int(g[0]), int(g[-1] - g[0] + 1)
            rc = L.hgx_wire_info(ctx, first, count, ptr(self.spi), ptr(self.opc), ptr(self.opi))
            assert rc == 0
        for k in range(m):
            rc = L.hgx_get_event(ctx, int(g[k]), None, None, None, None, C.byref(ts), C.byref(nt), C.byref(nil), C.byref(err))
            _lib.check(rc, err)
            self.ts[k], self.ntx[k], self.nil[k] = ts.value, nt.value, nil.value
        ms = (time.perf_counter() - t0) * 1e3
        self.g = g
        return ms, m


def insert_one(h, t, k):
    h.insert_trace(t, k, k + 1)


def stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def measure(a, E):
    extra = a.repeats * (a.reps + a.warmup) + 8
    t = gtrace.gossip(a.n, E + extra, a.seed)
    h = build(t, E, E + extra)
    known = known_behind(t, E, a.behind)
    rows = a.behind + extra + a.n
    new, old = DiffCall(h, rows), ParentRoute(h, rows, E + extra)
    nxt = E
    # the answers agree (gids, wire indices, timestamp, ntx, tx_nil)
    insert_one(h, t, nxt)
    nxt += 1
    _, m = new(known)
    _, m2 = old(known)
    assert m == m2 and np.array_equal(new.cols["gid"][:m], old.g)
    g0 = int(old.g[0])
    for nm, ref in (("self_parent_index", old.spi), ("other_parent_creator", old.opc), ("other_parent_index", old.opi)):
        assert np.array_equal(new.cols[nm][:m], ref[old.g - g0]), nm
    assert np.array_equal(new.cols["timestamp_ns"][:m], old.ts[:m]) and np.array_equal(new.cols["ntx"][:m], old.ntx[:m])
    runs = []
    for rep_all in range(a.repeats):
        d, c, w = [], [], []
        for rep in range(a.reps + a.warmup):
            insert_one(h, t, nxt)
            nxt += 1
            if rep % 2:
                dm, m = new(known)
                cm, _ = old(known)
                wm, _ = old(known)
            else:
                cm, _ = old(known)
                wm, _ = old(known)
                dm, m = new(known)
            if rep >= a.warmup:
                d.append(dm)
                c.append(cm)
                w.append(wm)
        runs.append(dict(diff_wire_ms=stats(d), parent_cold_ms=stats(c), parent_warm_ms=stats(w), rows_last=m))
    h.close()
    med = lambda k: [r[k]["median"] for r in runs]
    dw, pc, pw = med("diff_wire_ms"), med("parent_cold_ms"), med("parent_warm_ms")
    return dict(n=a.n, resident=E, behind=a.behind, reps=a.reps, warmup=a.warmup, repeats=runs,
                diff_wire_median_ms=float(np.median(dw)), diff_wire_spread_ms=float(max(dw) - min(dw)),
                parent_cold_median_ms=float(np.median(pc)), parent_cold_spread_ms=float(max(pc) - min(pc)),
                parent_warm_median_ms=float(np.median(pw)), parent_warm_spread_ms=float(max(pw) - min(pw)),
                cold_over_diff=float(np.median(pc) / np.median(dw)), warm_over_diff=float(np.median(pw) / np.median(dw)),
                beats_cold_by_more_than_the_spread=bool(min(pc) - max(dw) > 0))


def mode_call(a):
    return {f"resident_{E}": measure(a, E) for E in a.events}


def mode_once(a):
    E = a.events[-1]
    t = gtrace.gossip(a.n, E, a.seed)
    h = build(t, E, E)
    known = known_behind(t, E, a.behind)
    call = DiffCall(h, a.behind + a.n)
    ms = [call(known)[0] for _ in range(a.calls)]
    h.close()
    return dict(n=a.n, resident=E, behind=a.behind, calls=a.calls, rows=call.cnt.value, call_ms_under_profiler=stats(ms),
                bytes_read_per_kernel=E * BYTES_PER_RESIDENT_EVENT // 2, bytes_read_per_call=E * BYTES_PER_RESIDENT_EVENT)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["call", "once"])
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--events", type=int, nargs="+", default=[200_000, 2_000_000])
    ap.add_argument("--behind", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"call": mode_call, "once": mode_once}[a.mode](a)
    txt = json.dumps(res, indent=1, default=float)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
