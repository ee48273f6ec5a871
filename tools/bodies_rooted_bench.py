"""Dev tool: wall time of one hgx_insert_event_bodies sync on a pruned (rooted) context against an
unrooted context taking the same events, on one GPU.

  python tools/bodies_rooted_bench.py [--n 256] [--resident 20000] [--sync 1000] [--reps 7]
                                      [--parent-lib libhgx_parent.so] [--rounds 2] [--out file.json]

The driver signs a gossip trace of resident + sync events on the CPU (tests/bodyref.py), keeps it in
bench_out/, and starts one child process per measurement. A child builds two contexts before every
repeat: P takes the first `resident` events through the body path, runs consensus and prunes to its
frame; U takes them and stays unpruned. The timed call is the next `sync` events through
hgx_insert_event_bodies (bare binding; the call ends in a device synchronise), parents remapped to
P's gids for P. P and U alternate inside a repeat; the first two repeats warm up. Every returned id
is checked against the CPU chain.
--parent-lib: a library built from the parent commit, placed next to libhgx.so. Its children measure
U alone (the parent refuses a rooted context) and alternate with this build's children, `rounds`
processes each.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CACHE = os.path.join(ROOT, "bench_out", "bodies_rooted_chain.npz")
TRACE_COLS = ("creator", "index", "sp", "op", "ts", "ntx", "txnil", "tx_seq")


def stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), all=[round(float(x), 3) for x in v])


def sign_chain(a):
    import bodyref
    from babble_amd import trace as gtrace
    t = gtrace.gossip(a.n, a.resident + a.sync, a.seed)
    c = bodyref.build(t, [t.txs(i) for i in range(t.E)])
    os.makedirs(os.path.dirname(CACHE), exist_ok=True)
    np.savez(CACHE, keys=c.keys, r=c.r, s=c.t.s, ids=c.ids, **{k: getattr(t, k) for k in TRACE_COLS})
    return int(c.level[a.resident:].max() - c.level[a.resident:].min() + 1)


def child(a):
    from babble_amd import _lib
    from babble_amd import trace as gtrace
    from babble_amd._lib import hgx_error, ptr
    from babble_amd.hashgraph import Hashgraph, _event_bodies_of, body_columns
    z = np.load(CACHE)
    R0, E = a.resident, a.resident + a.sync
    tx = lambda i: None if z["txnil"][i] else ([gtrace.payload(int(z["creator"][i]), int(z["tx_seq"][i]))] if z["ntx"][i] else [])
    txs = [tx(i) for i in range(E)]
    col = lambda sl, sp, op: body_columns(z["creator"][sl], z["index"][sl], sp, op, z["ts"][sl], z["r"][sl], z["s"][sl],
                                          txs[sl])
    head = col(slice(0, R0), z["sp"][:R0], z["op"][:R0])
    tail = slice(R0, E)
    L = _lib.lib()

    def timed(h, cols):
        keep, ev = _event_bodies_of(cols, 0, a.sync)
        ids = np.zeros((a.sync, 32), np.uint8)
        err, n_ins = hgx_error(), C.c_int64(0)
        t0 = time.perf_counter()
        rc = L.hgx_insert_event_bodies(h.ctx, C.byref(ev), a.sync, ptr(ids), C.byref(n_ins), C.byref(err))
        ms = (time.perf_counter() - t0) * 1e3
        _lib.check(rc, err)
        assert np.array_equal(ids, z["ids"][tail])
        return ms

    def fresh():
        h = Hashgraph(a.n, capacity=E)
        h.set_participant_keys(z["keys"])
        h.insert_bodies(head)
        h.RunConsensus()
        return h

    ms_p, ms_u, info = [], [], {}
    for rep in range(a.reps + 2):
        hU = fresh()
        hP = None
        if not a.skip_rooted:
            hP = fresh()
            old = hP.PruneToFrame()
            hP.RunConsensus()
            new = np.full(E, -1, np.int64)
            new[old] = np.arange(len(old))
            new[R0:] = len(old) + np.arange(a.sync)
            sp, op = z["sp"][tail], z["op"][tail]
            sp_n = np.where(sp >= 0, new[np.maximum(sp, 0)], -1)
            op_n = np.where(op >= 0, new[np.maximum(op, 0)], -1)
            assert (sp_n[sp >= 0] >= 0).all() and (op_n[op >= 0] >= 0).all(), "a parent was pruned away"
            roots = [hP.GetRoot(p) for p in range(a.n)]
            info = dict(kept=len(old), others=len(hP.GetRootOthers()), roots_with_round=sum(r["Round"] >= 0 for r in roots),
                        roots_with_y=sum(r["Y"] != -1 for r in roots))
            assert info["roots_with_round"] > 0, "the pruned context is not rooted: raise --resident"
            cols_p = col(tail, sp_n, op_n)
        cols_u = col(tail, z["sp"][tail], z["op"][tail])
        order = [("P", hP), ("U", hU)] if rep % 2 == 0 else [("U", hU), ("P", hP)]
        for name, h in order:
            if h is None:
                continue
            ms = timed(h, cols_p if name == "P" else cols_u)
            if rep >= 2:
                (ms_p if name == "P" else ms_u).append(ms)
        hU.close()
        if hP is not None:
            hP.close()
    res = dict(lib=os.path.basename(_lib.LIB_PATH), unrooted_resident=R0, unrooted_ms=stats(ms_u))
    if ms_p:
        res.update(rooted=info, rooted_resident=info["kept"], rooted_ms=stats(ms_p))
    print("RESULT " + json.dumps(res))


def run_child(a, lib, skip_rooted):
    env = dict(os.environ)
    if lib:
        env["HGX_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--n", str(a.n), "--resident", str(a.resident),
           "--sync", str(a.sync), "--reps", str(a.reps)] + (["--skip-rooted"] if skip_rooted else [])
    out = subprocess.run(cmd, env=env, check=True, stdout=subprocess.PIPE, text=True, timeout=600).stdout
    return json.loads(next(l for l in out.splitlines() if l.startswith("RESULT "))[7:])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--resident", type=int, default=20000)
    ap.add_argument("--sync", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--skip-rooted", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        child(a)
        sys.exit(0)
    levels = sign_chain(a)
    runs = []
    for _ in range(a.rounds):
        if a.parent_lib:
            runs.append(run_child(a, a.parent_lib, True))
        runs.append(run_child(a, None, False))
    res = dict(n=a.n, events_per_sync=a.sync, levels_of_the_sync=levels, repeats_per_process=a.reps, processes=runs)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
