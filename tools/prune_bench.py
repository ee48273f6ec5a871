"""Dev tool: measurements of hgx_prune_to_frame on one GPU.

  python tools/prune_bench.py call   [--n 256] [--events 2000000] [--reps 5] [--out file.json]
  python tools/prune_bench.py rooted [--n 256] [--events 2000000] [--syncs 20] [--out file.json]
  python tools/prune_bench.py once   [--n 256] [--events 2000000]     (one prune: run it under rocprofv3)

call:   wall time of hgx_prune_to_frame against the host route on an identical context
        (hgx_get_frame + hgx_reset + hgx_set_root_others + hgx_insert_events from the caller's host
        arrays; the caller's own remap of the parents is timed apart). The two alternate in one
        process; before every repeat the context is cleared and rebuilt (insert of the trace through
        hgx_events, one RunConsensus); one warm-up repeat first.
rooted: ms per step (1 000-event insert + RunConsensus) of the syncs that follow, on the pruned
        context and on an unpruned context holding the same events.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ctypes as C  # noqa: E402

from babble_amd import _lib  # noqa: E402
from babble_amd import trace as gtrace  # noqa: E402
from babble_amd._lib import hgx_error, hgx_events, ptr  # noqa: E402
from babble_amd.hashgraph import Hashgraph  # noqa: E402

ROOT_Y, ROOT_OTHER = -3, -4


def build(h, t, E, chunk=1 << 18):
    h.clear()
    for lo in range(0, E, chunk):
        h.insert_trace(t, lo, min(E, lo + chunk))
    h.RunConsensus()


def host_remap(t, ev, oth_ev):
    """The frame's events with the parents InsertEvent expects after Reset(frame roots), vectorised."""
    new = np.full(t.E, -1, np.int64)
    new[ev] = np.arange(len(ev))
    sp, op = t.sp[ev], t.op[ev]
    sp_new = np.where(sp >= 0, new[np.maximum(sp, 0)], -1)
    op_kept = np.where(op >= 0, new[np.maximum(op, 0)], -1)
    first = sp_new < 0
    op_new = np.where(op < 0, -1, np.where(op_kept >= 0, op_kept, np.where(first, ROOT_Y, ROOT_OTHER)))
    cols = [np.ascontiguousarray(x) for x in (t.creator[ev], t.index[ev], sp_new, op_new, t.ts[ev], t.hash[ev],
                                              t.s[ev], t.ntx[ev], t.txnil[ev])]
    return cols, np.ascontiguousarray(t.hash[np.sort(oth_ev)])


def raw_prune(h, buf):
    """hgx_prune_to_frame through the bare binding (the clock holds the call alone)."""
    err, nk = hgx_error(), C.c_int64()
    t0 = time.perf_counter()
    rc = h.L.hgx_prune_to_frame(h.ctx, ptr(buf), buf.size, C.byref(nk), C.byref(err))
    ms = (time.perf_counter() - t0) * 1e3
    _lib.check(rc, err)
    return ms, buf[:nk.value]


def host_route(h, t, bufs):
    """The four library calls of the host route, each through the bare binding; the caller's remap
    (numpy) is timed apart."""
    L = h.L
    ev, oe, op, rx, ry, ri, rr = bufs
    err, ne, no, ins = hgx_error(), C.c_int64(), C.c_int64(), C.c_int64()
    t0 = time.perf_counter()
    rc = L.hgx_get_frame(h.ctx, ptr(ev), ev.size, C.byref(ne), ptr(rx), ptr(ry), ptr(ri), ptr(rr), ptr(oe), ptr(op),
                         oe.size, C.byref(no), C.byref(err))
    t1 = time.perf_counter()
    _lib.check(rc, err)
    cols, keys = host_remap(t, ev[:ne.value], oe[:no.value])
    yev = np.ascontiguousarray(ry != -1, np.int32)
    evs = hgx_events(*[ptr(c) for c in cols])
    t2 = time.perf_counter()
    rc = L.hgx_reset(h.ctx, ptr(ri), ptr(rr), ptr(yev), C.byref(err))
    if rc == 0 and no.value:
        rc = L.hgx_set_root_others(h.ctx, ptr(keys), keys.shape[0], C.byref(err))
    if rc == 0:
        rc = L.hgx_insert_events(h.ctx, C.byref(evs), ne.value, C.byref(ins), C.byref(err))
    t3 = time.perf_counter()
    _lib.check(rc, err)
    return dict(lib_ms=((t1 - t0) + (t3 - t2)) * 1e3, get_frame_ms=(t1 - t0) * 1e3, remap_ms=(t2 - t1) * 1e3,
                kept=ne.value, others=no.value)


def stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), all=[round(float(x), 3) for x in v])


def mode_call(a):
    t = gtrace.gossip(a.n, a.events, a.seed)
    hA, hB = Hashgraph(a.n, capacity=a.events), Hashgraph(a.n, capacity=a.events)
    dev, lib, gf, remap, info = [], [], [], [], {}
    E1 = a.events + 1
    old_buf = np.zeros(E1, np.int64)
    bufs = [np.zeros(E1, np.int64) for _ in range(3)] + [np.zeros(a.n, np.int64), np.zeros(a.n, np.int64),
                                                          np.zeros(a.n, np.int32), np.zeros(a.n, np.int32)]
    for rep in range(a.reps + 1):
        build(hA, t, a.events)
        d, old = raw_prune(hA, old_buf)
        build(hB, t, a.events)
        r = host_route(hB, t, bufs)
        assert len(old) == r["kept"] == hA.num_events() == hB.num_events()
        assert list(hA.Known()) == list(hB.Known())
        if rep:   # (repeat 0 warms both up)
            dev.append(d)
            lib.append(r["lib_ms"])
            gf.append(r["get_frame_ms"])
            remap.append(r["remap_ms"])
        info = dict(kept=r["kept"], others=r["others"])
    return dict(n=a.n, resident=a.events, **info, prune_to_frame_ms=stats(dev), host_route_library_calls_ms=stats(lib),
                host_route_get_frame_ms=stats(gf), host_route_caller_remap_ms=stats(remap),
                ratio_host_over_device=float(np.median(lib) / np.median(dev)))


def mode_rooted(a):
    step = 1000
    total = a.events + a.syncs * step
    t = gtrace.gossip(a.n, total, a.seed)
    hP, hU = Hashgraph(a.n, capacity=total), Hashgraph(a.n, capacity=total)
    build(hP, t, a.events)
    build(hU, t, a.events)
    old = hP.PruneToFrame()
    hP.RunConsensus()
    new = np.full(total, -1, np.int64)
    new[old] = np.arange(len(old))
    new[a.events:] = len(old) + np.arange(total - a.events)
    ms_p, ms_u = [], []
    for lo in range(a.events, total, step):
        sl = slice(lo, lo + step)
        sp, op = t.sp[sl], t.op[sl]
        sp_n = np.where(sp >= 0, new[np.maximum(sp, 0)], -1)
        op_n = np.where(op >= 0, new[np.maximum(op, 0)], -1)
        assert (sp_n[sp >= 0] >= 0).all() and (op_n[op >= 0] >= 0).all(), "a parent was pruned away"
        t0 = time.perf_counter()
        hP.insert_arrays(t.creator[sl], t.index[sl], sp_n, op_n, t.ts[sl], t.hash[sl], t.s[sl], t.ntx[sl], t.txnil[sl])
        hP.RunConsensus()
        t1 = time.perf_counter()
        hU.insert_trace(t, lo, lo + step)
        hU.RunConsensus()
        t2 = time.perf_counter()
        ms_p.append((t1 - t0) * 1e3)
        ms_u.append((t2 - t1) * 1e3)
    return dict(n=a.n, resident_before=a.events, kept=len(old), syncs=a.syncs, events_per_sync=step,
                last_consensus_round=[hP.LastConsensusRound(), hU.LastConsensusRound()],
                last_round=[hP.LastRound(), hU.LastRound()],
                pruned_ms_per_step=stats(ms_p), unpruned_ms_per_step=stats(ms_u),
                pruned_phases_last=hP.phase_times(), unpruned_phases_last=hU.phase_times())


def mode_once(a):
    t = gtrace.gossip(a.n, a.events, a.seed)
    h = Hashgraph(a.n, capacity=a.events)
    build(h, t, a.events)
    old = h.PruneToFrame()
    return dict(n=a.n, resident=a.events, kept=len(old), others=len(h.GetRootOthers()))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["call", "rooted", "once"])
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--events", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--syncs", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"call": mode_call, "rooted": mode_rooted, "once": mode_once}[a.mode](a)
    txt = json.dumps(res, indent=1, default=float)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
