"""The signer's two measurements; prints one JSON object.

  python tools/sign_bench.py [--count 1000000] [--keys 256] [--n 256] [--events 200000] [--cpu-events N]
                             [--legs batch chain cpu] [--out FILE]

batch  `count` digests under `keys` derived keys through hgx_p256_sign_batch: signatures/s from the wall
       clock of the call, which INCLUDES the base point's table build and the copies in and out (a warm-up
       call of the same shape comes first; `repeats` timed calls). Beside it hgx_p256_verify_bench on the
       same count in the same process, over the signatures just made: device time per verify launch from
       HIP events (no copies, key tables built before the window), so the two figures are not like for
       like; both are printed for what they are.
chain  gossip(n, events) signed and inserted through hgx_sign_insert_event_bodies on an empty context:
       seconds (host clock around the call, which ends in a device synchronise) and events/s, the number
       of dependency levels the call walks (summed over its internal chunks of 65 536 events) and the mean
       time per level: one workgroup walks a graph's levels, so the call is bound by the DAG's depth times
       one signature's latency, not by throughput.
cpu    the CPU route for the first `cpu-events` events of the same trace (default: all), tools/
       wire_bodies_bench.py sign's way on the same machine: level by level, body JSON from the oracle's
       encoder, SHA-256, one oracle/p256_ref sign process per level, the event's JSON and its id.
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from babble_amd import trace as gtrace  # noqa: E402
from babble_amd.hashgraph import (Hashgraph, batch_levels, body_columns, p256_public_keys, p256_sign,  # noqa: E402
                                  p256_verify_bench)

CHUNK = 65536   # hgx_bodies.h kBodyChunkEvents


def stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def derived_keys(n):
    import signref
    return signref.priv_bytes(n)


def leg_batch(a):
    d = derived_keys(a.keys)
    rng = np.random.default_rng(a.seed)
    dig = rng.integers(0, 256, (a.count, 32), dtype=np.uint8)
    idx = (np.arange(a.count) % a.keys).astype(np.int32)
    p256_sign(d, idx[:a.count], dig)   # warm-up: code objects, allocations
    secs = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        r, s = p256_sign(d, idx, dig)
        secs.append(time.perf_counter() - t0)
    pub = p256_public_keys(d)
    v = p256_verify_bench(pub, idx, dig, r, s, warmup=1, iters=a.repeats)
    assert (v["out"] == 1).all(), "the device's verify rejects a device signature"
    med = float(np.median(secs))
    return dict(count=a.count, keys=a.keys, repeats=a.repeats,
                sign_call_seconds=stats(secs), sign_per_s_wall_incl_table_and_copies=a.count / med,
                verify_ms_per_launch_device=v["ms_per_launch"],
                verify_per_s_device_launch_only=a.count / (v["ms_per_launch"] * 1e-3),
                command=f"python tools/sign_bench.py --legs batch --count {a.count} --keys {a.keys}")


def chain_levels(t):
    total = 0
    for lo in range(0, t.E, CHUNK):
        hi = min(t.E, lo + CHUNK)
        total += batch_levels(t.sp[lo:hi], t.op[lo:hi], base=lo)[1]
    return total


def leg_chain(a, t):
    d = derived_keys(a.n)
    pub = p256_public_keys(d)
    cols = body_columns(t.creator, t.index, t.sp, t.op, t.ts, None, None, [t.txs(i) for i in range(t.E)])
    secs = []
    for rep in range(a.chain_repeats + 1):   # (the first call is the warm-up)
        h = Hashgraph(a.n, capacity=t.E)
        h.set_participant_keys(pub)
        h.set_signing_keys(d)
        t0 = time.perf_counter()
        r, s, ids, k = h.sign_insert_event_bodies(cols)
        dt = time.perf_counter() - t0
        assert k == t.E
        h.close()
        if rep:
            secs.append(dt)
    levels = chain_levels(t)
    med = float(np.median(secs))
    return dict(n=a.n, events=t.E, repeats=a.chain_repeats, seconds=stats(secs), events_per_s=t.E / med, levels=levels,
                mean_ms_per_level=1e3 * med / levels, last_id=bytes(ids[-1]).hex(),
                command=f"python tools/sign_bench.py --legs chain --n {a.n} --events {t.E}"), (r, s, ids)


def leg_cpu(a, t, m):
    """wire_bodies_bench.py sign's route over events [0, m)."""
    import bodyref
    import hgref
    t0 = time.perf_counter()
    level, nl = bodyref.py_levels(t.sp[:m], t.op[:m])
    keys, _, _ = hgref.sign_batch(t.n, [0], np.zeros((1, 32), np.uint8))
    ids, dig = np.zeros((m, 32), np.uint8), np.zeros((m, 32), np.uint8)
    r, s = np.zeros((m, 32), np.uint8), np.zeros((m, 32), np.uint8)
    pid = lambda g: None if g < 0 else bytes(ids[g])
    txs = [t.txs(k) for k in range(m)]
    order = np.argsort(level, kind="stable")
    cuts = np.searchsorted(level[order], np.arange(nl + 1))
    for l in range(nl):
        ks = order[cuts[l]:cuts[l + 1]]
        for k in ks:
            bj = bodyref.body_json(txs[k], pid(t.sp[k]), pid(t.op[k]), bytes(keys[t.creator[k]]), int(t.ts[k]), int(t.index[k]))
            dig[k] = np.frombuffer(hashlib.sha256(bj).digest(), np.uint8)
        _, r[ks], s[ks] = hgref.sign_batch(t.n, t.creator[ks], dig[ks])
        for k in ks:
            js = hgref.go_event_json(txs[k], bodyref.hex_id(pid(t.sp[k])), bodyref.hex_id(pid(t.op[k])),
                                     bytes(keys[t.creator[k]]), int(t.ts[k]), int(t.index[k]), bytes(r[k]), bytes(s[k]))
            ids[k] = np.frombuffer(hashlib.sha256(js).digest(), np.uint8)
    dt = time.perf_counter() - t0
    return dict(events=m, levels=int(nl), seconds=dt, events_per_s=m / dt,
                route="tools/wire_bodies_bench.py sign's: one oracle/p256_ref sign process per level, JSON per event")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=1_000_000)
    ap.add_argument("--keys", type=int, default=256)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--events", type=int, default=200_000)
    ap.add_argument("--cpu-events", type=int, default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--chain-repeats", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--legs", nargs="+", default=["batch", "chain", "cpu"], choices=["batch", "chain", "cpu"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}

    def keep():   # (a leg that runs long does not lose the ones before it)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")

    if "batch" in a.legs:
        res["batch"] = leg_batch(a)
        keep()
    t = gtrace.gossip(a.n, a.events, a.seed) if ("chain" in a.legs or "cpu" in a.legs) else None
    if "chain" in a.legs:
        res["chain"], _ = leg_chain(a, t)
        keep()
    if "cpu" in a.legs:
        res["cpu_route"] = leg_cpu(a, t, min(t.E, a.cpu_events or t.E))
        keep()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
