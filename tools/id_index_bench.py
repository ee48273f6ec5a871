"""The event-id index against its parent-equivalent paths; prints one JSON object.

  python tools/id_index_bench.py [--legs overhead find by_id] [--out profiles/r17_id_index/id_index.json]

One signed chain: gossip(n, resident + events) signed once by hgx_sign_insert_event_bodies on a scratch
context (derived keys), whose R, S and ids are then the events' columns and claimed ids.

overhead  what keeping the index costs an insert: the same batches (`resident` events, then `batches`
          syncs of events / batches each, through hgx_insert_event_bodies_claimed) on a fresh context that
          keeps the index and on one that does not, alternating in one process. Wall clock of the sync
          calls (each ends in a device synchronise), median [min, max] over the repeats; the resident
          load is timed apart (it contains the index's one large launch).
find      hgx_find_events over all resident ids in shuffled order plus as many absent ids, one call:
          queries per second, wall clock of the call (copies included).
by_id     a sync of `events` events into `resident` resident ones: hgx_insert_events_by_id (parents as
          ids, resolved on the device) against hgx_insert_event_bodies_claimed fed by a Python dict from
          id bytes to gid (the dict's lookups are inside the timed region: it is the work the index
          takes over; its filling from the resident ids is timed apart as dict_fill_seconds).

Every figure of a leg is stated against the same job's other route: index not kept, or _claimed with
host-resolved gids.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from babble_amd.hashgraph import Hashgraph  # noqa: E402
from bodies_claimed_bench import signed_chain, stats  # noqa: E402


def fresh(n, pub, cap, keep):
    h = Hashgraph(n, capacity=cap)
    h.set_participant_keys(pub)
    if keep:
        h.KeepIdIndex()
    return h


def parents_as_ids(t, ids):
    m = len(t.sp)
    sp_ids, op_ids = np.zeros((m, 32), np.uint8), np.zeros((m, 32), np.uint8)
    has_sp, has_op = t.sp >= 0, t.op >= 0
    sp_ids[has_sp] = ids[t.sp[has_sp]]
    op_ids[has_op] = ids[t.op[has_op]]
    return sp_ids, op_ids, (has_sp.astype(np.uint8) | (has_op.astype(np.uint8) << 1))


def leg_overhead(n, pub, cols, ids, resident, events, batches, repeats):
    hi = resident + events
    step = events // batches
    secs = dict(off=[], kept=[])
    load = dict(off=[], kept=[])
    for rep in range(repeats + 1):   # (the first round is the warm-up)
        for route in ("off", "kept"):
            h = fresh(n, pub, hi, route == "kept")
            t0 = time.perf_counter()
            h.insert_bodies_claimed(cols, ids, lo=0, hi=resident)
            t_load = time.perf_counter() - t0
            t0 = time.perf_counter()
            for lo in range(resident, hi, step):
                h.insert_bodies_claimed(cols, ids, lo=lo, hi=min(hi, lo + step))
            dt = time.perf_counter() - t0
            assert h.num_events() == hi
            if route == "kept":
                st = h.IdIndexState()
                assert st["kept"] == 1 and st["entries"] == hi
            h.close()
            if rep:
                secs[route].append(dt / batches)
                load[route].append(t_load)
    return dict(resident=resident, events=events, batches=batches, batch_events=step, repeats=repeats,
                seconds_per_batch={r: stats(v) for r, v in secs.items()},
                overhead_per_batch_us=(float(np.median(secs["kept"])) - float(np.median(secs["off"]))) * 1e6,
                kept_over_off_median=float(np.median(secs["kept"]) / np.median(secs["off"])),
                load_seconds={r: stats(v) for r, v in load.items()}, index_state=st)


def leg_find(n, pub, cols, ids, resident, repeats):
    h = fresh(n, pub, resident, True)
    h.insert_bodies_claimed(cols, ids, lo=0, hi=resident)
    rng = np.random.default_rng(7)
    perm = rng.permutation(resident)
    q = np.concatenate([ids[perm], rng.integers(0, 256, (resident, 32), dtype=np.uint8)])
    want = np.concatenate([perm, np.full(resident, -1)])
    secs = []
    for rep in range(repeats + 1):
        t0 = time.perf_counter()
        got = h.FindEvents(q)
        secs.append(time.perf_counter() - t0)
        assert np.array_equal(got, want)
    # the dict a caller would keep instead, over the same queries
    t0 = time.perf_counter()
    by = {ids[g].tobytes(): g for g in range(resident)}
    t_fill = time.perf_counter() - t0
    t0 = time.perf_counter()
    got = [by.get(r.tobytes(), -1) for r in q]
    t_dict = time.perf_counter() - t0
    assert np.array_equal(np.asarray(got), want)
    st = h.IdIndexState()
    h.close()
    return dict(resident=resident, queries=len(q), repeats=repeats, seconds=stats(secs[1:]),
                queries_per_s=len(q) / float(np.median(secs[1:])), python_dict_fill_seconds=t_fill,
                python_dict_lookup_seconds=t_dict, python_dict_queries_per_s=len(q) / t_dict, index_state=st)


def leg_by_id(n, pub, t, cols, ids, resident, events, repeats):
    hi = resident + events
    sp_ids, op_ids, flags = parents_as_ids(t, ids)
    secs = dict(claimed_dict=[], by_id=[])
    fill = []
    for rep in range(repeats + 1):
        for route in ("claimed_dict", "by_id"):
            h = fresh(n, pub, hi, route == "by_id")
            h.insert_bodies_claimed(cols, ids, lo=0, hi=resident)
            if route == "by_id":
                t0 = time.perf_counter()
                k, sp, op = h.insert_events_by_id(cols, ids, sp_ids, op_ids, flags, resident, hi)
                dt = time.perf_counter() - t0
                assert np.array_equal(sp, t.sp[resident:hi]) and np.array_equal(op, t.op[resident:hi])
            else:
                t0 = time.perf_counter()
                by = {ids[g].tobytes(): g for g in range(resident)}   # the shim's map of the resident events
                t_fill = time.perf_counter() - t0
                t0 = time.perf_counter()
                sp, op = np.full(hi, -1, np.int64), np.full(hi, -1, np.int64)
                for g in range(resident, hi):   # one lookup per present parent, the batch's own events added as they go
                    if flags[g] & 1:
                        sp[g] = by.get(sp_ids[g].tobytes(), -2)
                    if flags[g] & 2:
                        op[g] = by.get(op_ids[g].tobytes(), -2)
                    by[ids[g].tobytes()] = g
                k = h.insert_bodies_claimed(dict(cols, sp=sp, op=op), ids, lo=resident, hi=hi)
                dt = time.perf_counter() - t0
                if rep:
                    fill.append(t_fill)
            assert k == events and h.event_id(hi - 1) == ids[hi - 1].tobytes()
            h.close()
            if rep:
                secs[route].append(dt)
    out = {r: dict(seconds=stats(v), events_per_s=events / float(np.median(v))) for r, v in secs.items()}
    out.update(resident=resident, events=events, repeats=repeats, dict_fill_seconds=stats(fill),
               by_id_over_claimed_dict_median=float(np.median(secs["by_id"]) / np.median(secs["claimed_dict"])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", nargs="+", default=["overhead", "find", "by_id"], choices=["overhead", "find", "by_id"])
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--resident", type=int, default=100000)
    ap.add_argument("--events", type=int, default=8000)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    hi = a.resident + a.events
    pub, t, cols, ids = signed_chain(a.n, hi, a.seed)
    res = dict(n=a.n)

    def keep():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")

    if "overhead" in a.legs:
        res["overhead"] = leg_overhead(a.n, pub, cols, ids, a.resident, a.events, a.batches, a.repeats)
        keep()
    if "find" in a.legs:
        res["find"] = leg_find(a.n, pub, cols, ids, a.resident, a.repeats)
        keep()
    if "by_id" in a.legs:
        res["by_id"] = leg_by_id(a.n, pub, t, cols, ids, a.resident, a.events, a.repeats)
        keep()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
