"""Dev tool: measurements of hgx_get_frame_bodies on one GPU.

  python tools/frame_bench.py call [--n 256] [--events 2000000] [--reps 5] [--out file.json]
  python tools/frame_bench.py once [--n 256] [--events 2000000]      (one call: run it under rocprofv3)

call: wall time of hgx_get_frame_bodies (the sizing call + the fill) against the route that gives the
      same data without it: hgx_get_frame, then hgx_get_event_id for every root, Others pair, event
      and parent, hgx_get_event per event, and hgx_get_event_bodies (sizing + fill). A host clock
      around the bare C calls, which end in a synchronise; the two routes alternate in one process
      on one context, one warm-up repeat first. The context is gossip(n, events), signed once on a
      scratch context (hgx_sign_insert_event_bodies), taken with the bodies kept in syncs of 20 000
      events through hgx_insert_event_bodies_claimed, each followed by RunConsensus.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from babble_amd import _lib  # noqa: E402
from babble_amd import trace as gtrace  # noqa: E402
from babble_amd._lib import hgx_error, ptr  # noqa: E402
from babble_amd.hashgraph import Hashgraph, body_columns, p256_public_keys  # noqa: E402

SYNC = 20000


def resident(n, E, seed):
    """A context holding gossip(n, E) with ids, signatures and bodies, after one RunConsensus."""
    import signref
    d = signref.priv_bytes(n)
    t = gtrace.gossip(n, E, seed)
    pub = p256_public_keys(d)
    txs = [t.txs(i) for i in range(E)]
    s = Hashgraph(n, capacity=E)   # a scratch context signs the chain once
    s.set_participant_keys(pub)
    s.set_signing_keys(d)
    r, sg, ids, k = s.sign_insert_event_bodies(body_columns(t.creator, t.index, t.sp, t.op, t.ts, None, None, txs))
    s.close()
    assert k == E
    cols = body_columns(t.creator, t.index, t.sp, t.op, t.ts, r, sg, txs)
    h = Hashgraph(n, capacity=E)
    h.set_participant_keys(pub)
    h.KeepBodies(0, 0)
    for lo in range(0, E, SYNC):   # syncs as a node takes them: insert with the claimed ids, then consensus
        hi = min(E, lo + SYNC)
        assert h.insert_bodies_claimed(cols, ids, lo=lo, hi=hi) == hi - lo
        h.RunConsensus()
    return h


def new_route(h):
    """hgx_get_frame_bodies twice: the sizing call (a body column makes the body totals count), the fill."""
    C_ = h.n
    spec = dict(_lib.FRAME_OUT_FIELDS)
    t0 = time.perf_counter()
    rc, err, (ne, no, nt, nb) = h.get_frame_bodies_raw(dict(sig_r=np.zeros((1, 32), np.uint8)))
    assert rc == 103, err.msg
    rows = {nm: C_ for nm in _lib.FRAME_ROOT_COLUMNS}
    rows.update({nm: no for nm in _lib.FRAME_OTHERS_COLUMNS})
    rows.update({nm: ne for nm in _lib.FRAME_EVENT_COLUMNS})
    rows.update(tx_off=nt + 1, tx_bytes=nb)
    arr = {nm: np.empty((max(1, m),) + spec[nm][1], spec[nm][0]) for nm, m in rows.items()}
    rc, err, _ = h.get_frame_bodies_raw(arr, ne, no, nt, nb)
    ms = (time.perf_counter() - t0) * 1e3
    _lib.check(rc, err)
    nbytes = sum(arr[nm][:m].nbytes for nm, m in rows.items())
    return ms, dict(events=ne, others=no, n_tx=nt, tx_bytes=nb, bytes_returned=nbytes), arr


def old_route(h, bufs):
    """The same data through the entries that existed before: per-root, per-pair and per-event getters."""
    L, ctx = h.L, h.ctx
    ev, oe, op, rx, ry, ri, rr = bufs
    err, ne, no = hgx_error(), C.c_int64(), C.c_int64()
    t0 = time.perf_counter()
    rc = L.hgx_get_frame(ctx, ptr(ev), ev.size, C.byref(ne), ptr(rx), ptr(ry), ptr(ri), ptr(rr), ptr(oe), ptr(op),
                         oe.size, C.byref(no), C.byref(err))
    _lib.check(rc, err)
    t1 = time.perf_counter()
    ne, no = ne.value, no.value
    ids = np.zeros((ne, 32), np.uint8)
    spid, opid = np.zeros((ne, 32), np.uint8), np.zeros((ne, 32), np.uint8)
    rid = np.zeros((2 * h.n, 32), np.uint8)
    oid = np.zeros((2 * max(1, no), 32), np.uint8)
    cols = np.zeros((ne, 7), np.int64)

    def get_id(gid, row):
        if gid >= 0:
            _lib.check(L.hgx_get_event_id(ctx, int(gid), row.ctypes.data_as(C.c_void_p), C.byref(err)), err)

    for p in range(h.n):
        get_id(rx[p], rid[2 * p])
        get_id(ry[p], rid[2 * p + 1])
    for j in range(no):
        get_id(oe[j], oid[2 * j])
        get_id(op[j], oid[2 * j + 1])
    cr, nt, nil = C.c_int32(), C.c_int32(), C.c_int32()
    ix, sp, opp, ts = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    for k in range(ne):
        g = int(ev[k])
        _lib.check(L.hgx_get_event(ctx, g, C.byref(cr), C.byref(ix), C.byref(sp), C.byref(opp), C.byref(ts), C.byref(nt),
                                   C.byref(nil), C.byref(err)), err)
        cols[k] = (cr.value, ix.value, sp.value, opp.value, ts.value, nt.value, nil.value)
        get_id(g, ids[k])
        get_id(sp.value, spid[k])
        get_id(opp.value, opid[k])
    t2 = time.perf_counter()
    gids = np.ascontiguousarray(ev[:ne])
    n_tx, n_by = C.c_int64(), C.c_int64()
    rc = L.hgx_get_event_bodies(ctx, ptr(gids), ne, None, None, None, 0, None, 0, C.byref(n_tx), C.byref(n_by), C.byref(err))
    assert rc == 103, err.msg
    R, ntx = np.zeros((ne, 32), np.uint8), np.zeros(ne, np.int32)
    off, by = np.zeros(n_tx.value + 1, np.int64), np.zeros(max(1, n_by.value), np.uint8)
    rc = L.hgx_get_event_bodies(ctx, ptr(gids), ne, ptr(R), ptr(ntx), ptr(off), n_tx.value, ptr(by), n_by.value,
                                C.byref(n_tx), C.byref(n_by), C.byref(err))
    _lib.check(rc, err)
    t3 = time.perf_counter()
    # (S has no getter of its own before this call: the old route cannot return it at all)
    return dict(total_ms=(t3 - t0) * 1e3, get_frame_ms=(t1 - t0) * 1e3, per_event_ms=(t2 - t1) * 1e3,
                bodies_ms=(t3 - t2) * 1e3), dict(ids=ids, spid=spid, opid=opid, R=R, off=off, by=by[:n_by.value], gid=gids)


def stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), all=[round(float(x), 3) for x in v])


def mode_call(a):
    h = resident(a.n, a.events, a.seed)
    E1 = a.events + 1
    bufs = [np.zeros(E1, np.int64) for _ in range(3)] + [np.zeros(a.n, np.int64), np.zeros(a.n, np.int64),
                                                          np.zeros(a.n, np.int32), np.zeros(a.n, np.int32)]
    new, old, parts, info = [], [], {}, {}
    for rep in range(a.reps + 1):
        ms, info, arr = new_route(h)
        o, got = old_route(h, bufs)
        ne = info["events"]
        assert np.array_equal(arr["gid"][:ne], got["gid"]) and np.array_equal(arr["id32"][:ne], got["ids"])
        assert np.array_equal(arr["self_parent_id32"][:ne], got["spid"])
        assert np.array_equal(arr["other_parent_id32"][:ne], got["opid"])
        assert np.array_equal(arr["sig_r"][:ne], got["R"]) and np.array_equal(arr["tx_off"], got["off"])
        assert np.array_equal(arr["tx_bytes"][:info["tx_bytes"]], got["by"])
        if rep:   # (repeat 0 warms both up)
            new.append(ms)
            old.append(o["total_ms"])
            for k, v in o.items():
                parts.setdefault(k, []).append(v)
    return dict(n=a.n, resident=a.events, **info, get_frame_bodies_ms=stats(new), old_route_ms=stats(old),
                old_route_parts_ms={k: stats(v) for k, v in parts.items()},
                ratio_old_over_new=float(np.median(old) / np.median(new)))


def mode_once(a):
    h = resident(a.n, a.events, a.seed)
    ms, info, _ = new_route(h)
    return dict(n=a.n, resident=a.events, ms=ms, **info)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["call", "once"])
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--events", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=5)
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
