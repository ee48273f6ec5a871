"""Dev tool: what the resident body store (hgx_keep_bodies) costs and saves, on one GPU.

  python tools/bodies_kept_bench.py [--n 256] [--resident 4000] [--sync 1000] [--reps 15] [--warmup 3]
                                    [--diff-resident 200000 2000000] [--blocks-n 64] [--out FILE]
                                    [--vs-parent FILE ...] [--kernel-stats CSV]
  python tools/bodies_kept_bench.py --only insert_off [--tree DIR --label NAME] --out FILE
  rocprofv3 --kernel-trace --stats ... -- python tools/bodies_kept_bench.py --only find_order_loop

Host clock around the bare C calls (each ends in a device synchronise; every array is allocated and every
sizing call made before the clock starts), medians with ranges, the compared paths alternating in one
process (the order flips every repetition):
  insert      hgx_insert_event_bodies of a `sync`-event batch into `resident` events (§3.10(a)'s shape),
              keeping on against off (the append's price);
  find_order  one hgx_find_order over everything inserted, keeping on against off (the eager block hashes), at
              --blocks-n participants (the same event counts decide no round at n = 256: no block is made);
  blocks      hgx_block_transactions + hgx_get_block_hash of every block against hgx_consensus_events + a host
              gather + hgx_block_hash (what a caller without the store does);
  diff        hgx_diff_wire_bodies for the last `sync` rows against hgx_diff_wire plus a numpy gather of R and
              the bytes from host arrays keyed by gid, at `resident` events and at every --diff-resident size.
--only insert_off measures the keeping-off insert alone and imports babble_amd from --tree (a build of another
commit): processes of the two builds run alternately, and --vs-parent puts their results beside the rest.
--only find_order_loop runs `reps` keeping-on hgx_find_order calls and nothing else, for a kernel trace of its
own; --kernel-stats reads that trace's per-kernel statistics (the body-store and block-encoder kernels).
The events are a gossip trace signed on the CPU (tests/bodyref.py), since the store holds only what came
through the body paths: 0.1 to 0.6 ms per event, minutes at 2 000 000 events.
"""
import argparse
import csv
import ctypes as C
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(v):
    return dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)), reps=len(v))


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def host_store(c, E):
    """What a caller without the store keeps on the host: the bytes of every event in one array, by gid."""
    off = np.zeros(E + 1, np.int64)
    np.cumsum([sum(len(x) for x in (t or [])) for t in c.txs[:E]], out=off[1:])
    flat = np.frombuffer(b"".join(x for t in c.txs[:E] for x in (t or [])) + b"\0", np.uint8)
    return off, flat


def bench_diff(h, c, E, rows, a, lib):
    """The last `rows` events of E resident ones, as a sync response with R and the bytes: one
    hgx_diff_wire_bodies against hgx_diff_wire + a numpy gather from the host arrays."""
    _lib, hgx_error, ptr = lib
    known = np.full(a.n, -1, np.int32)
    np.maximum.at(known, np.asarray(c.t.creator[:E - rows]), np.asarray(c.t.index[:E - rows], np.int32))
    off_h, flat = host_store(c, E)
    r_host = np.ascontiguousarray(c.r[:E])

    def columns():
        cols = {nm: np.zeros((rows,) + shp, dt) for nm, dt, shp in _lib.WIRE_OUT_COLUMNS}
        return cols, _lib.hgx_wire_out(**{nm: ptr(x) for nm, x in cols.items()})

    cols_d, out_d = columns()
    cols_h, out_h = columns()
    cnt, over, nt, nb, err = C.c_int64(0), C.c_int32(0), C.c_int64(0), C.c_int64(0), hgx_error()
    rc = h.L.hgx_diff_wire_bodies(h.ctx, 0, ptr(known), -1, C.byref(out_d), None, rows, C.byref(cnt), C.byref(nt),
                                  C.byref(nb), C.byref(over), C.byref(err))
    assert rc in (0, 103) and cnt.value == rows, (rc, err.msg, cnt.value)
    r = np.zeros((rows, 32), np.uint8)
    off, by = np.zeros(nt.value + 1, np.int64), np.zeros(max(nb.value, 1), np.uint8)
    body = _lib.hgx_wire_body_out(ptr(r), ptr(off), nt.value, ptr(by), nb.value)
    got = {}

    def device():
        rc = h.L.hgx_diff_wire_bodies(h.ctx, 0, ptr(known), -1, C.byref(out_d), C.byref(body), rows, C.byref(cnt),
                                      C.byref(nt), C.byref(nb), C.byref(over), C.byref(err))
        assert rc == 0, err.msg

    def host():
        rc = h.L.hgx_diff_wire(h.ctx, 0, ptr(known), -1, C.byref(out_h), rows, C.byref(cnt), C.byref(over),
                               C.byref(err))
        assert rc == 0, err.msg
        g = cols_h["gid"]
        lo, ln = off_h[g], off_h[g + 1] - off_h[g]
        at = np.cumsum(ln) - ln
        got["r"] = r_host[g]
        got["bytes"] = flat[np.repeat(lo - at, ln) + np.arange(int(ln.sum()))]

    device()
    host()
    assert np.array_equal(got["r"], r) and np.array_equal(got["bytes"], by[:nb.value])
    td, th = [], []
    for rep in range(a.warmup + a.reps):
        for dev in ((True, False) if rep % 2 == 0 else (False, True)):
            x = timed(device if dev else host)
            if rep >= a.warmup:
                (td if dev else th).append(x)
    return dict(resident=E, rows=rows, n_tx=nt.value, n_bytes=nb.value, device=stats(td), host_gather=stats(th))


def kernel_stats(path):
    """rocprofv3 --kernel-trace --stats' per-kernel table: the kernels this change adds to hgx_find_order."""
    res = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            m = re.search(r"\b(k_(?:body|blk)_\w+)", row.get("Name", ""))
            if m:
                short = m.group(1)
                res[short] = dict(calls=int(row["Calls"]), average_us=float(row["AverageNs"]) / 1e3,
                                  min_us=float(row["MinNs"]) / 1e3, max_us=float(row["MaxNs"]) / 1e3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--resident", type=int, default=4000)
    ap.add_argument("--sync", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=9)
    ap.add_argument("--diff-resident", type=int, nargs="*", default=[200000, 2000000])
    ap.add_argument("--blocks-n", type=int, default=64, help="participants of the find_order / blocks shape")
    ap.add_argument("--only", choices=("all", "insert_off", "find_order_loop"), default="all")
    ap.add_argument("--tree", default=ROOT, help="import babble_amd from this checkout (insert_off)")
    ap.add_argument("--label", default="this change", help="the build's name in the result (insert_off)")
    ap.add_argument("--vs-parent", nargs="*", default=[], help="results of --only insert_off runs to include")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3's kernel statistics of a find_order_loop run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bodies_kept.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.abspath(a.tree))
    import bodyref
    from babble_amd import _lib
    from babble_amd._lib import hgx_error, ptr
    from babble_amd.hashgraph import Hashgraph, _event_bodies_of
    R, E = a.resident, a.resident + a.sync
    ids = np.zeros((a.sync, 32), np.uint8)

    def run_shape(n, modes):
        """The sync into R resident events, then one hgx_find_order, per repetition on fresh contents."""
        c = bodyref.chain(n, E, a.seed)
        ctx = {}
        for keep in modes:
            h = Hashgraph(n, capacity=E)
            h.set_participant_keys(c.keys)
            ctx[keep] = h
        _, ev = _event_bodies_of(c.cols, R, E)
        t_ins, t_fo = {False: [], True: []}, {False: [], True: []}
        for rep in range(a.warmup + a.reps):
            for keep in (modes if rep % 2 == 0 else modes[::-1]):
                h = ctx[keep]
                h.clear()
                if keep:
                    h.KeepBodies(0, 0)
                h.insert_bodies(c.cols, 0, R)
                err, n_ins = hgx_error(), C.c_int64(0)
                dt = timed(lambda: h.L.hgx_insert_event_bodies(h.ctx, C.byref(ev), a.sync, ptr(ids), C.byref(n_ins),
                                                               C.byref(err)))
                assert n_ins.value == a.sync, err.msg
                h.DivideRounds()
                h.DecideFame()
                df = timed(lambda: h.L.hgx_find_order(h.ctx, C.byref(err)))
                assert err.code == 0, err.msg
                if rep >= a.warmup:
                    t_ins[keep].append(dt)
                    t_fo[keep].append(df)
        return c, ctx, t_ins, t_fo

    res = dict(n=a.n, resident=R, sync=a.sync)
    if a.only == "insert_off":
        res.update(build=a.label, insert_off=stats(run_shape(a.n, (False,))[2][False]))
    if a.only == "find_order_loop":
        res.update(n=a.blocks_n, find_order_on=stats(run_shape(a.blocks_n, (True,))[3][True]))
    if a.only != "all":
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res))
        return
    lib = (_lib, hgx_error, ptr)
    c, ctx, t_ins, _ = run_shape(a.n, (False, True))
    res["insert"] = {name: stats(t_ins[keep]) for keep, name in ((False, "off"), (True, "on"))}
    if a.vs_parent:   # keeping off, this build against a build of the parent commit, processes alternating
        res["insert"]["off_by_build"] = [json.load(open(p)) for p in a.vs_parent]
    res["diff"] = [bench_diff(ctx[True], c, E, a.sync, a, lib)]
    for k in ctx.values():
        k.close()
    # hgx_find_order and the block consumers at --blocks-n participants: E events decide no round at n = 256,
    # so no block would be made there
    c, ctx, _, t_fo = run_shape(a.blocks_n, (False, True))
    res["find_order"] = {name: stats(t_fo[keep]) for keep, name in ((False, "off"), (True, "on"))}
    res["find_order"]["n"] = a.blocks_n
    h, p = ctx[True], ctx[False]
    blocks = h.Blocks()
    assert blocks, "no block was made: choose a smaller --blocks-n"
    res["find_order"]["blocks"] = len(blocks)
    res["find_order"]["block_events"] = [b["n_events"] for b in blocks]
    res["find_order"]["block_tx"] = [b["ntx"] for b in blocks]
    if a.kernel_stats:
        res["find_order"]["kernels"] = kernel_stats(a.kernel_stats)
    # every block's transactions and hash: the bare calls, buffers sized beforehand on both sides
    nb_blk = len(blocks)
    n_order = int(p.L.hgx_consensus_events_count(p.ctx, 0))
    order = np.zeros(max(n_order, 1), np.int64)
    off_h, flat = host_store(c, E)
    raw = flat.tobytes()
    tx_at = np.zeros(E + 1, np.int64)   # the host store's transaction table
    np.cumsum([len(t or []) for t in c.txs[:E]], out=tx_at[1:])
    tx_lo = np.zeros(int(tx_at[E]) + 1, np.int64)
    np.cumsum([len(x) for t in c.txs[:E] for x in (t or [])], out=tx_lo[1:])
    max_tx = max([b["ntx"] for b in blocks] + [1])
    sizes = []
    for b in range(nb_blk):
        nt, nby, err = C.c_int64(0), C.c_int64(0), hgx_error()
        h.L.hgx_block_transactions(h.ctx, 0, b, None, 0, None, 0, C.byref(nt), C.byref(nby), C.byref(err))
        sizes.append((nt.value, nby.value))
    offs = [np.zeros(t + 1, np.int64) for t, _ in sizes]
    bys = [np.zeros(max(y, 1), np.uint8) for _, y in sizes]
    dev_hash, host_hash = np.zeros((max(nb_blk, 1), 32), np.uint8), np.zeros((max(nb_blk, 1), 32), np.uint8)
    ptrs, lens = (C.c_char_p * max_tx)(), (C.c_int64 * max_tx)()

    def dev_blocks():
        nt, nby, err = C.c_int64(0), C.c_int64(0), hgx_error()
        for b in range(nb_blk):
            rc = h.L.hgx_block_transactions(h.ctx, 0, b, ptr(offs[b]), sizes[b][0], ptr(bys[b]), sizes[b][1],
                                            C.byref(nt), C.byref(nby), C.byref(err))
            assert rc == 0, err.msg
            rc = h.L.hgx_get_block_hash(h.ctx, 0, b, ptr(dev_hash[b]), C.byref(err))
            assert rc == 0, err.msg

    def host_blocks():
        rc = p.L.hgx_consensus_events(p.ctx, 0, 0, n_order, ptr(order))
        assert rc == 0
        for b, blk in enumerate(blocks):
            k = 0
            for g in order[blk["first"]:blk["first"] + blk["n_events"]]:
                for j in range(tx_at[g], tx_at[g + 1]):
                    lo, hi = tx_lo[j], tx_lo[j + 1]
                    ptrs[k] = raw[lo:hi]
                    lens[k] = hi - lo
                    k += 1
            p.L.hgx_block_hash(blk["rr"], k, C.cast(ptrs, C.c_void_p), C.cast(lens, C.c_void_p),
                               1 if blk["tx_nil"] else 0, ptr(host_hash[b]))

    dev_blocks()
    host_blocks()
    assert np.array_equal(dev_hash, host_hash)
    tb, thb = [], []
    for rep in range(a.warmup + a.reps):
        for dev in ((True, False) if rep % 2 == 0 else (False, True)):
            x = timed(dev_blocks if dev else host_blocks)
            if rep >= a.warmup:
                (tb if dev else thb).append(x)
    res["blocks"] = dict(n=a.blocks_n, blocks=nb_blk, device=stats(tb), host=stats(thb))
    for k in ctx.values():
        k.close()

    def write():   # (after every resident size: a large one that runs out of time loses only itself)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)

    write()
    for big in a.diff_resident:   # a resident set of its own: signed on the CPU first (progress on stdout)
        t0 = time.perf_counter()
        cb = bodyref.chain(a.n, big, a.seed + 1)
        print(f"signed {big} events in {time.perf_counter() - t0:.0f} s", flush=True)
        hb = Hashgraph(a.n, capacity=big)
        hb.set_participant_keys(cb.keys)
        hb.KeepBodies(0, 0)
        for lo in range(0, big, 20000):
            hb.insert_bodies(cb.cols, lo, min(big, lo + 20000))
        res["diff"].append(bench_diff(hb, cb, big, a.sync, a, lib))
        hb.close()
        print(json.dumps(res["diff"][-1]), flush=True)
        del cb, hb
        write()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
