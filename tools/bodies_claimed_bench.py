"""The flat id pass against the level pass; prints one JSON object.

  python tools/bodies_claimed_bench.py [--legs sync bulk ckpt] [--out profiles/bodies_claimed.json]

Both routes insert the same signed chain: gossip(n, E) signed once by hgx_sign_insert_event_bodies on a
scratch context (derived keys), whose R, S and ids are then the events' columns and claimed ids.

sync  §3.10's shape (a): a 1 000-event sync at n = 256 into 4 000 resident events. Per repeat and route a
      fresh context takes the 4 000 events (untimed), then the timed call; the routes alternate in one
      process. Wall clock of the call (it ends in a device synchronise), median [min, max].
bulk  §3.10's shape (b): 262 144 events at n = 64 in one call on an empty context, the same way; with the
      number of dependency levels the level route walks.
ckpt  hgx_save_bodies of a keeping context and hgx_bootstrap of that file on a fresh keeping context,
      seconds each, the file's size and the restored store's counts, on the first --ckpt-events events of
      (b)'s chain. Not at (b)'s full size: a consensus run that orders some 65 000 events or more in one call
      on a keeping context is refused by hgx_find_order's block hashing ("block hashes: invalid argument",
      on the level route as well), and Bootstrap runs consensus once over the whole file. A refusal is
      recorded in the result, not raised.
--only ROUTE  one timed sync call of one route and nothing else (for a kernel trace of its own).
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from babble_amd import trace as gtrace  # noqa: E402
from babble_amd.hashgraph import Hashgraph, batch_levels, body_columns, p256_public_keys  # noqa: E402

CHUNK = 65536   # hgx_bodies.h kBodyChunkEvents


def stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def signed_chain(n, E, seed):
    """(keys, columns with the device's R and S, ids) of gossip(n, E, seed)."""
    import signref
    d = signref.priv_bytes(n)
    pub = p256_public_keys(d)
    t = gtrace.gossip(n, E, seed)
    txs = [t.txs(i) for i in range(t.E)]
    h = Hashgraph(n, capacity=t.E)
    h.set_participant_keys(pub)
    h.set_signing_keys(d)
    r, s, ids, k = h.sign_insert_event_bodies(body_columns(t.creator, t.index, t.sp, t.op, t.ts, None, None, txs))
    h.close()
    assert k == t.E
    return pub, t, body_columns(t.creator, t.index, t.sp, t.op, t.ts, r, s, txs), ids


def timed_call(n, pub, cols, ids, resident, hi, route, keep=False):
    h = Hashgraph(n, capacity=hi)
    h.set_participant_keys(pub)
    if keep:
        h.KeepBodies(0, 0)
    if resident:
        h.insert_bodies_claimed(cols, ids, lo=0, hi=resident)
    t0 = time.perf_counter()
    if route == "claimed":
        k = h.insert_bodies_claimed(cols, ids, lo=resident, hi=hi)
    else:
        k = len(h.insert_bodies(cols, resident, hi))
    dt = time.perf_counter() - t0
    assert k == hi - resident and h.event_id(hi - 1) == ids[hi - 1].tobytes()
    return dt, h


def compare(n, pub, cols, ids, resident, hi, repeats):
    secs = dict(level=[], claimed=[])
    for rep in range(repeats + 1):   # (the first round is the warm-up)
        for route in ("level", "claimed"):
            dt, h = timed_call(n, pub, cols, ids, resident, hi, route)
            h.close()
            if rep:
                secs[route].append(dt)
    m = hi - resident
    out = {r: dict(seconds=stats(v), events_per_s=m / float(np.median(v))) for r, v in secs.items()}
    out["speedup_median"] = float(np.median(secs["level"]) / np.median(secs["claimed"]))
    return out


def levels_of(t, lo, hi):
    total = 0
    for a in range(lo, hi, CHUNK):
        b = min(hi, a + CHUNK)
        total += batch_levels(t.sp[a:b], t.op[a:b], base=a)[1]
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", nargs="+", default=["sync", "bulk", "ckpt"], choices=["sync", "bulk", "ckpt"])
    ap.add_argument("--only", default=None, choices=["level", "claimed"])
    ap.add_argument("--sync-n", type=int, default=256)
    ap.add_argument("--sync-resident", type=int, default=4000)
    ap.add_argument("--sync-events", type=int, default=1000)
    ap.add_argument("--bulk-n", type=int, default=64)
    ap.add_argument("--bulk-events", type=int, default=262144)
    ap.add_argument("--ckpt-events", type=int, default=32768)
    ap.add_argument("--sync-repeats", type=int, default=9)
    ap.add_argument("--bulk-repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}

    def keep():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")

    if a.only or "sync" in a.legs:
        hi = a.sync_resident + a.sync_events
        pub, t, cols, ids = signed_chain(a.sync_n, hi, a.seed)
        if a.only:
            timed_call(a.sync_n, pub, cols, ids, a.sync_resident, hi, a.only)[1].close()   # warm-up
            dt, h = timed_call(a.sync_n, pub, cols, ids, a.sync_resident, hi, a.only)
            h.close()
            print(json.dumps(dict(route=a.only, seconds=dt)))
            return
        res["sync"] = dict(n=a.sync_n, resident=a.sync_resident, events=a.sync_events, repeats=a.sync_repeats,
                           levels=levels_of(t, a.sync_resident, hi),
                           **compare(a.sync_n, pub, cols, ids, a.sync_resident, hi, a.sync_repeats))
        keep()
    if "bulk" in a.legs or "ckpt" in a.legs:
        E = a.bulk_events
        pub, t, cols, ids = signed_chain(a.bulk_n, E, a.seed)
        if "bulk" in a.legs:
            res["bulk"] = dict(n=a.bulk_n, events=E, repeats=a.bulk_repeats, levels=levels_of(t, 0, E),
                               **compare(a.bulk_n, pub, cols, ids, 0, E, a.bulk_repeats))
            keep()
        if "ckpt" in a.legs:
            from babble_amd._lib import HgxError
            Ec = min(E, a.ckpt_events)
            _, h = timed_call(a.bulk_n, pub, cols, ids, 0, Ec, "claimed", keep=True)
            b = Hashgraph(a.bulk_n, capacity=Ec)
            b.KeepBodies(0, 0)
            res["ckpt"] = dict(n=a.bulk_n, events=Ec)
            try:
                h.RunConsensus()
                with tempfile.TemporaryDirectory() as d:
                    p = os.path.join(d, "bodies.ckpt")
                    t0 = time.perf_counter()
                    h.save_bodies(p)
                    t_save = time.perf_counter() - t0
                    size = os.path.getsize(p)
                    t0 = time.perf_counter()
                    b.Bootstrap(p)
                    t_boot = time.perf_counter() - t0
                assert b.BodiesState() == h.BodiesState() and b.event_id(Ec - 1) == ids[Ec - 1].tobytes()
                assert list(b.ConsensusEvents()) == list(h.ConsensusEvents())
                res["ckpt"].update(file_bytes=size, save_bodies_seconds=t_save, bootstrap_seconds_incl_consensus=t_boot,
                                   store=b.BodiesState(), blocks=len(b.Blocks()))
            except HgxError as e:
                res["ckpt"].update(error=e.msg, resident=b.num_events(), store=b.BodiesState())
            h.close()
            b.close()
            keep()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
