"""Dev tool: measurements of hgx_insert_wire_bodies on one GPU.

  python tools/wire_bodies_bench.py sign [--n 256] [--events 200000 2000000]     (CPU only: signs the syncs
                                         of every size into bench_out/, where `call` and `once` find them)
  python tools/wire_bodies_bench.py call [--n 256] [--events 200000 2000000] [--sync 1000] [--reps 50]
                                         [--repeats 3] [--out file.json]
  python tools/wire_bodies_bench.py once [--n 256] [--events 2000000] [--calls 20]   (run it under
                                         rocprofv3 --kernel-trace --stats: the kernels' device time)

call: host clock around the bare C calls (each ends in a device synchronise) of three ways to take the
      same signed `sync`-event SyncResponse on contexts in the same state, alternating in one process:
        wire   hgx_insert_wire_bodies, all three output columns;
        gid    hgx_insert_event_bodies with the parents already gids (the ceiling: wire - gid is what
               resolution costs);
        shim   the route without the call: hgx_read_wire_info per event for the resident parents (the
               batch's own events from a dict), then hgx_insert_event_bodies.
      Before every sync each context takes the node's own new event through a one-event
      hgx_insert_event_bodies, which drops the host mirror: the shim's first lookup rebuilds it.
      The order of the routes flips every repeat. The whole measurement runs `repeats` times: the spread
      of the medians is the run-to-run spread. The ids of the three routes are compared once per size.
The resident events are a gossip trace inserted with the trace's ids; the syncs are the trace's next
events, signed on the CPU (tests/bodyref.py's way) over their parents' ids.
"""
import argparse
import ctypes as C
import hashlib
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


def stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def tail_events(a):
    return a.repeats * (a.reps + a.warmup) * (a.sync + 1) + a.sync + 1


def signed_path(a, E):
    return os.path.join(ROOT, "bench_out", f"wire_sync_n{a.n}_E{E}_x{tail_events(a)}_s{a.seed}.npz")


def sign_tail(t, E):
    """Keys, R, S and ids of events [E, t.E) whose resident parents' ids are the trace's hash column"""
    import bodyref
    import hgref
    m = t.E - E
    level, nl = bodyref.py_levels(t.sp[E:], t.op[E:], base=E)
    keys, _, _ = hgref.sign_batch(t.n, [0], np.zeros((1, 32), np.uint8))
    ids, dig = np.zeros((m, 32), np.uint8), np.zeros((m, 32), np.uint8)
    r, s = np.zeros((m, 32), np.uint8), np.zeros((m, 32), np.uint8)
    pid = lambda g: None if g < 0 else bytes(t.hash[g]) if g < E else bytes(ids[g - E])
    txs = [t.txs(E + k) for k in range(m)]
    for l in range(nl):
        ks = np.nonzero(level == l)[0]
        for k in ks:
            g = E + k
            bj = bodyref.body_json(txs[k], pid(t.sp[g]), pid(t.op[g]), bytes(keys[t.creator[g]]), int(t.ts[g]), int(t.index[g]))
            dig[k] = np.frombuffer(hashlib.sha256(bj).digest(), np.uint8)
        _, r[ks], s[ks] = hgref.sign_batch(t.n, t.creator[E + ks], dig[ks])
        for k in ks:
            g = E + k
            js = hgref.go_event_json(txs[k], bodyref.hex_id(pid(t.sp[g])), bodyref.hex_id(pid(t.op[g])),
                                     bytes(keys[t.creator[g]]), int(t.ts[g]), int(t.index[g]), bytes(r[k]), bytes(s[k]))
            ids[k] = np.frombuffer(hashlib.sha256(js).digest(), np.uint8)
    return keys, r, s, ids


def signed(a, E, t):
    p = signed_path(a, E)
    if os.path.exists(p):
        z = np.load(p)
        return z["keys"], z["r"], z["s"], z["ids"]
    keys, r, s, ids = sign_tail(t, E)
    os.makedirs(os.path.dirname(p), exist_ok=True)
    np.savez(p, keys=keys, r=r, s=s, ids=ids)
    return keys, r, s, ids


def setup(a, E, contexts):
    """The trace, the signed tail as body / wire columns, and `contexts` contexts holding the residents"""
    from babble_amd.hashgraph import Hashgraph, body_columns, wire_body_columns
    total = E + tail_events(a)
    t = gtrace.gossip(a.n, total, a.seed)
    keys, r, s, ids = signed(a, E, t)
    sel = np.arange(E, total)
    sp, op = t.sp[sel], t.op[sel]
    txs = [t.txs(int(g)) for g in sel]
    body = body_columns(t.creator[sel], t.index[sel], sp, op, t.ts[sel], r, s, txs)
    rows = dict(creator_id=t.creator[sel], index=t.index[sel],
                self_parent_index=np.where(sp >= 0, t.index[np.maximum(sp, 0)], -1),
                other_parent_creator=np.where(op >= 0, t.creator[np.maximum(op, 0)], -1),
                other_parent_index=np.where(op >= 0, t.index[np.maximum(op, 0)], -1), timestamp_ns=t.ts[sel], sig_s=s)
    wire = wire_body_columns(rows, r, txs)
    hs = []
    for _ in range(contexts):
        h = Hashgraph(a.n, capacity=total)
        h.set_participant_keys(keys)
        for lo in range(0, E, 1 << 18):
            h.insert_trace(t, lo, min(E, lo + (1 << 18)))
        hs.append(h)
    return t, ids, body, wire, hs


class Routes:
    def __init__(self, a, E, body, wire):
        self.a, self.E, self.body, self.wire = a, E, body, wire
        m = a.sync
        self.ids = np.zeros((m, 32), np.uint8)
        self.sp, self.op = np.zeros(m, np.int64), np.zeros(m, np.int64)
        self.err, self.n_ins = hgx_error(), C.c_int64()

    def own(self, h, k):
        """the node's own new event (tail position k) through a one-event hgx_insert_event_bodies"""
        from babble_amd.hashgraph import _event_bodies_of
        _, ev = _event_bodies_of(self.body, k, k + 1)
        _lib.check(h.L.hgx_insert_event_bodies(h.ctx, C.byref(ev), 1, None, C.byref(self.n_ins), C.byref(self.err)), self.err)

    def wire_route(self, h, lo):
        from babble_amd.hashgraph import _wire_bodies_of
        _, ev = _wire_bodies_of(self.wire, lo, lo + self.a.sync)
        t0 = time.perf_counter()
        rc = h.L.hgx_insert_wire_bodies(h.ctx, C.byref(ev), self.a.sync, ptr(self.ids), ptr(self.sp), ptr(self.op),
                                        C.byref(self.n_ins), C.byref(self.err))
        ms = (time.perf_counter() - t0) * 1e3
        _lib.check(rc, self.err)
        return ms

    def gid_route(self, h, lo):
        from babble_amd.hashgraph import _event_bodies_of
        _, ev = _event_bodies_of(self.body, lo, lo + self.a.sync)
        t0 = time.perf_counter()
        rc = h.L.hgx_insert_event_bodies(h.ctx, C.byref(ev), self.a.sync, ptr(self.ids), C.byref(self.n_ins), C.byref(self.err))
        ms = (time.perf_counter() - t0) * 1e3
        _lib.check(rc, self.err)
        return ms

    def shim_route(self, h, lo):
        from babble_amd.hashgraph import _event_bodies_of, _wire_bodies_of
        m, L = self.a.sync, h.L
        w, _ = _wire_bodies_of(self.wire, lo, lo + m)
        b, _ = _event_bodies_of(self.body, lo, lo + m)
        cr, ix = w["creator_id"].tolist(), w["index"].tolist()
        spi, opc, opi = w["self_parent_index"].tolist(), w["other_parent_creator"].tolist(), w["other_parent_index"].tolist()
        sp, op = np.zeros(m, np.int64), np.zeros(m, np.int64)
        gs, go = C.c_int64(), C.c_int64()
        t0 = time.perf_counter()
        base = L.hgx_num_events(h.ctx)
        mine = {}   # (creator, Index) -> gid of the batch's own events
        for k in range(m):
            s = mine.get((cr[k], spi[k]), None) if spi[k] >= 0 else -1
            o = mine.get((opc[k], opi[k]), None) if opi[k] >= 0 else -1
            if s is None or o is None:
                rc = L.hgx_read_wire_info(h.ctx, cr[k], spi[k] if s is None else -1, opc[k], opi[k] if o is None else -1,
                                          C.byref(gs), C.byref(go), C.byref(self.err))
                _lib.check(rc, self.err)
                s = gs.value if s is None else s
                o = go.value if o is None else o
            sp[k], op[k] = s, o
            mine[(cr[k], ix[k])] = base + k
        b["sp"], b["op"] = sp, op
        ev = _lib.hgx_event_bodies(*[ptr(b[x]) for x in ("creator", "index", "sp", "op", "ts", "r", "s", "ntx", "tx_off",
                                                         "tx_bytes")])
        rc = L.hgx_insert_event_bodies(h.ctx, C.byref(ev), m, ptr(self.ids), C.byref(self.n_ins), C.byref(self.err))
        ms = (time.perf_counter() - t0) * 1e3
        _lib.check(rc, self.err)
        return ms


def measure(a, E):
    t, ids, body, wire, (hw, hg, hs) = setup(a, E, 3)
    R = Routes(a, E, body, wire)
    m = a.sync
    # one sync on every route: the same ids, the chain's
    pos = 0
    for h, route in ((hw, R.wire_route), (hg, R.gid_route), (hs, R.shim_route)):
        R.own(h, pos)
        route(h, pos + 1)
        assert np.array_equal(R.ids, ids[pos + 1:pos + 1 + m]), route.__name__
    assert np.array_equal(R.sp, t.sp[E + 1:E + 1 + m])
    pos += m + 1
    runs = []
    for _ in range(a.repeats):
        w, g, s = [], [], []
        for rep in range(a.reps + a.warmup):
            for h in (hw, hg, hs):
                R.own(h, pos)
            order = ((hw, R.wire_route, w), (hg, R.gid_route, g), (hs, R.shim_route, s))
            for h, route, dst in (order if rep % 2 else order[::-1]):
                ms = route(h, pos + 1)
                if rep >= a.warmup:
                    dst.append(ms)
            pos += m + 1
        runs.append(dict(wire_ms=stats(w), gid_ms=stats(g), shim_ms=stats(s)))
    for h in (hw, hg, hs):
        h.close()
    med = lambda k: [r[k]["median"] for r in runs]
    mw, mg, ms_ = med("wire_ms"), med("gid_ms"), med("shim_ms")
    return dict(n=a.n, resident=E, sync=m, reps=a.reps, warmup=a.warmup, repeats=runs,
                wire_median_ms=float(np.median(mw)), wire_range_ms=[min(mw), max(mw)],
                gid_median_ms=float(np.median(mg)), gid_range_ms=[min(mg), max(mg)],
                shim_median_ms=float(np.median(ms_)), shim_range_ms=[min(ms_), max(ms_)],
                resolution_cost_ms=float(np.median(mw) - np.median(mg)),
                shim_over_wire=float(np.median(ms_) / np.median(mw)),
                beats_shim_by_more_than_the_spread=bool(min(ms_) - max(mw) > 0))


def mode_call(a):
    return {f"resident_{E}": measure(a, E) for E in a.events}


def once_args(a):
    b = argparse.Namespace(**vars(a))
    b.repeats, b.reps, b.warmup, b.events = 1, a.calls, 0, a.events[-1:]
    return b


def mode_once(a):
    a = once_args(a)
    E = a.events[-1]
    t, ids, body, wire, (h,) = setup(a, E, 1)
    R = Routes(a, E, body, wire)
    ms = []
    for k in range(a.calls):
        R.own(h, k * (a.sync + 1))
        ms.append(R.wire_route(h, k * (a.sync + 1) + 1))
    h.close()
    return dict(n=a.n, resident=E, sync=a.sync, calls=a.calls, call_ms_under_profiler=stats(ms), bytes_read_by_window=8 * E)


def mode_sign(a):
    out = {}
    for b in (a, once_args(a)):   # the syncs of `call` at every size, and of `once` at the last
        for E in b.events:
            t0 = time.time()
            t = gtrace.gossip(b.n, E + tail_events(b), b.seed)
            signed(b, E, t)
            out[signed_path(b, E)] = time.time() - t0
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["call", "once", "sign"])
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--events", type=int, nargs="+", default=[200_000, 2_000_000])
    ap.add_argument("--sync", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"call": mode_call, "once": mode_once, "sign": mode_sign}[a.mode](a)
    txt = json.dumps(res, indent=1, default=float)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
