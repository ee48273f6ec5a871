"""hgx_diff_wire: a SyncRequest answered on the device (node.processSyncRequest's OverSyncLimit,
Core.Diff and ToWire, node/node.go:214-270, node/core.go:147-188) against the oracle and the trace.

Expected values never come from the new call: the gids are {g : index[g] > known[creator[g]]} in
ascending order, the wire indices hgref.Oracle.wire(g), and timestamp, S, id, ntx and tx_nil the
trace columns. The device works in chunks of 2 048 gids (kDiffChunk, hgx_diff.hip): the shapes sit
on both sides of one and two chunk boundaries. Every context opened here is closed."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

import hgref
from babble_amd import _lib
from babble_amd import trace as gtrace
from babble_amd._lib import HgxError, hgx_error, ptr
from hgref import ROOT_OTHER, ROOT_Y, UNKNOWN

pytestmark = pytest.mark.gpu

NAMES = [nm for nm, _, _ in _lib.WIRE_OUT_COLUMNS]
SPEC = {nm: (dt, shp) for nm, dt, shp in _lib.WIRE_OUT_COLUMNS}
SENTINEL = 0x5A


@contextlib.contextmanager
def _ctx(n, cap, graphs=1, shard_devices=None):
    from babble_amd.hashgraph import Hashgraph
    h = Hashgraph(n, capacity=max(cap, 16), n_graphs=graphs, shard_devices=shard_devices)
    try:
        yield h
    finally:
        h.close()


@functools.lru_cache(maxsize=None)
def _traced(n, E, seed, n_silent=0):
    """A gossip trace and the oracle's wire indices of every event, computed once per shape. The wire
    indices of an event depend on its parents alone, so they hold for every prefix of the trace."""
    t = gtrace.gossip(n, E, seed, n_silent=n_silent, stale_prob=0.1, stale_depth=2)
    o = hgref.Oracle(n)
    o.insert_trace(t)
    wire = np.array([o.wire(g) for g in range(E)], np.int64).reshape(E, 3)
    wire.setflags(write=False)
    return t, wire


def _known_of(t, E, n):
    """Hashgraph.Known() of the first E events of trace t"""
    k = np.full(n, -1, np.int64)
    np.maximum.at(k, t.creator[:E], t.index[:E])
    return k


def _select(t, E, known, c0=0):
    n = len(known)
    g = np.arange(E)
    cr = t.creator[:E].astype(np.int64) - c0
    inside = (cr >= 0) & (cr < n)
    return g[inside & (t.index[:E] > np.asarray(known, np.int64)[np.clip(cr, 0, n - 1)])]


def _expected(t, wire, gids, c0=0, wire_off=0, root=None):
    """The twelve columns of events `gids` of trace t; wire[g - wire_off] = the oracle's wire indices.
    root: root_parent codes per event (default none)."""
    g = np.asarray(gids, np.int64)
    w = wire[g - wire_off] if len(g) else np.zeros((0, 3), np.int64)
    return dict(gid=g, creator_id=t.creator[g] - c0, index=t.index[g], self_parent_index=w[:, 0],
                other_parent_creator=w[:, 1], other_parent_index=w[:, 2], timestamp_ns=t.ts[g], hash=t.hash[g],
                sig_s=t.s[g], ntx=t.ntx[g], tx_nil=t.txnil[g],
                root_parent=np.zeros(len(g), np.uint8) if root is None else np.asarray(root, np.uint8)[g])


def _same(cols, want, names=NAMES):
    for nm in names:
        got, exp = np.asarray(cols[nm]), np.asarray(want[nm]).astype(SPEC[nm][0])
        assert got.dtype == SPEC[nm][0] and got.shape == exp.shape, (nm, got.shape, exp.shape)
        assert np.array_equal(got, exp), (nm, np.nonzero(got != exp)[0][:5])


def _raw(h, known, cap, names=NAMES, sync_limit=-1, graph=0, alloc=None, null=()):
    """hgx_diff_wire itself on sentinel-filled arrays of `alloc` rows: (rc, message, count, over, arrays)"""
    alloc = max(cap, 0) + 8 if alloc is None else alloc
    cols = {nm: np.full((alloc,) + SPEC[nm][1] + (np.dtype(SPEC[nm][0]).itemsize,), SENTINEL, np.uint8)
            .view(SPEC[nm][0]).reshape((alloc,) + SPEC[nm][1]) for nm in names}   # every byte the sentinel
    out = _lib.hgx_wire_out(**{nm: ptr(a) for nm, a in cols.items()})
    kn = np.ascontiguousarray(known, np.int32)
    cnt, over, err = C.c_int64(-77), C.c_int32(-77), hgx_error()
    rc = h.L.hgx_diff_wire(None if "ctx" in null else h.ctx, graph, None if "known" in null else ptr(kn), sync_limit,
                           None if "out" in null else C.byref(out), cap, None if "count" in null else C.byref(cnt),
                           C.byref(over), C.byref(err))
    return rc, err.msg.decode(errors="replace"), cnt.value, over.value, cols


def _untouched(cols, first=0):
    return all((np.asarray(a[first:]).view(np.uint8) == SENTINEL).all() for a in cols.values())


# ---- 1. the boundaries of the geometry --------------------------------------------------------
@pytest.mark.parametrize("E", [0, 1, 2047, 2048, 2049, 4097])
def test_chunk_boundaries(E):
    n = 4
    t, wire = _traced(n, 4097, 31)
    own = _known_of(t, E, n)
    cases = {"everything": np.full(n, -1), "nothing": own.copy()}
    if E:
        last = own.copy()
        last[t.creator[E - 1]] -= 1            # exactly the last resident gid
        cases["last gid only"] = last
        above = np.full(n, -1)
        above[t.creator[0]] = own[t.creator[0]] + 3   # known > last on one chain: that chain gives nothing
        cases["known above last"] = above
    if E > 2048:
        for x in (2047, 2048):                 # from the last gid of chunk 0 / the first of chunk 1 on, one chain
            k = own.copy()
            k[t.creator[x]] = t.index[x] - 1
            cases[f"chain of gid {x}"] = k
    with _ctx(n, E) as h:
        if E:
            h.insert_trace(t, 0, E)
        assert list(h.Known()) == list(own)
        for name, known in cases.items():
            sel = _select(t, E, known)
            cols, count, over = h.DiffWire(known)
            assert count == len(sel) and not over, name
            _same(cols, _expected(t, wire, sel))
            if name == "everything":
                assert count == E
            if name == "nothing":
                assert count == 0
            if name == "last gid only":
                assert list(cols["gid"]) == [E - 1]   # E = 2048: the last gid of chunk 0; 2049, 4097: the first of a chunk
            if name == "known above last":
                assert count == E - np.count_nonzero(t.creator[:E] == t.creator[0])
            if name.startswith("chain of gid"):
                assert cols["gid"][0] == int(name.split()[-1])


# ---- 2. shapes --------------------------------------------------------------------------------
@pytest.mark.parametrize("n,n_silent", [(3, 0), (64, 0), (256, 0), (1024, 341)])
def test_shapes_random_known(n, n_silent):
    E = 6000
    t, wire = _traced(n, E, 40 + n, n_silent)
    own = _known_of(t, E, n)
    with _ctx(n, E) as h:
        h.insert_trace(t)
        for seed in (1, 2, 3):
            rng = np.random.default_rng(seed * 1000 + n)
            known = rng.integers(-1, own + 1)   # per chain in [-1, last]
            sel = _select(t, E, known)
            cols, count, over = h.DiffWire(known)
            assert count == len(sel) and 0 < count < E and not over
            _same(cols, _expected(t, wire, sel))


def test_row_sharded_context():
    """A row-sharded rank holds the whole DAG: the same answer."""
    n, E = 16, 3000
    t, wire = _traced(n, E, 47)
    known = _known_of(t, E - 700, n)
    with _ctx(n, E) as h:
        h.set_shard(1, 2)
        h.insert_trace(t)
        cols, count, _ = h.DiffWire(known)
        sel = _select(t, E, known)
        assert count == len(sel) > 0
        _same(cols, _expected(t, wire, sel))


# ---- 3. cap and columns -----------------------------------------------------------------------
def test_cap_and_columns():
    n, E = 8, 5000
    t, wire = _traced(n, E, 52)
    known = _known_of(t, E - 1300, n)
    sel = _select(t, E, known)
    total = len(sel)
    assert total > 1000
    with _ctx(n, E) as h:
        h.insert_trace(t)
        for cap in (0, 1, total - 1, total, total + 5):
            rc, msg, count, over, cols = _raw(h, known, cap, alloc=total + 8)
            assert rc == 0 and count == total and over == 0, (cap, msg)
            m = min(cap, total)
            _same({nm: a[:m] for nm, a in cols.items()}, _expected(t, wire, sel[:m]))
            assert _untouched(cols, first=m), cap
        full, _, _ = h.DiffWire(known)
        only, count, _ = h.DiffWire(known, columns=["gid"])
        assert list(only) == ["gid"] and count == total and np.array_equal(only["gid"], full["gid"])
        some, _, _ = h.DiffWire(known, cap=10, columns=["sig_s", "other_parent_index", "root_parent"])
        _same(some, _expected(t, wire, sel[:10]), names=list(some))
        with pytest.raises(ValueError):
            h.DiffWire(known, columns=["nope"])


# ---- 4. the sync limit ------------------------------------------------------------------------
def test_sync_limit():
    n, E = 8, 3000
    t, wire = _traced(n, E, 53)
    own = _known_of(t, E, n)
    known = _known_of(t, E - 900, n)
    known[2] = own[2] + 4                       # ahead of us on one chain: counts as nothing
    unknown = int(np.maximum(own - known, 0).sum())
    sel = _select(t, E, known)
    assert unknown == len(sel) > 0
    with _ctx(n, E) as h:
        h.insert_trace(t)
        rc, msg, count, over, cols = _raw(h, known, unknown + 8, sync_limit=unknown)
        assert rc == 0 and over == 0 and count == unknown, msg
        _same({nm: a[:unknown] for nm, a in cols.items()}, _expected(t, wire, sel))
        rc, msg, count, over, cols = _raw(h, known, unknown + 8, sync_limit=unknown - 1)
        assert rc == 0 and over == 1 and count == unknown and _untouched(cols), msg
        cols, count, over = h.DiffWire(known, sync_limit=unknown - 1)
        assert over and count == unknown and all(len(a) == 0 for a in cols.values())
        cols, count, over = h.DiffWire(known, sync_limit=0)
        assert over
        cols, count, over = h.DiffWire(own, sync_limit=0)   # nothing unknown: not over a limit of 0
        assert not over and count == 0


# ---- 5. errors and refusals -------------------------------------------------------------------
def test_too_late_like_participant_events():
    n, E = 4, 600
    t, _ = _traced(n, 4097, 31)
    with _ctx(n, E) as h:
        h.insert_trace(t, 0, E)
        with pytest.raises(HgxError) as want:
            h.ParticipantEvents(1, -2)
        assert want.value.code == 2 and want.value.msg == "\x03, Too Late"
        known = np.full(n, -1)
        known[1] = -2
        rc, msg, count, over, cols = _raw(h, known, E)
        assert (rc, msg) == (2, want.value.msg) and count == -77 and over == -77 and _untouched(cols)
        known[3] = -5                           # two failing chains: the lower id's error (the same string)
        rc, msg, count, over, cols = _raw(h, known, E)
        assert (rc, msg) == (2, want.value.msg) and count == -77 and _untouched(cols)
        with pytest.raises(HgxError) as got:
            h.DiffWire(known)
        assert got.value.code == 2 and got.value.msg == want.value.msg
        # OverSyncLimit comes first, as in processSyncRequest
        rc, msg, count, over, cols = _raw(h, known, E, sync_limit=10)
        assert rc == 0 and over == 1 and _untouched(cols)


def test_refusals_change_nothing():
    from babble_amd.hashgraph import compact_columns
    n, E = 4, 600
    t, wire = _traced(n, 4097, 31)
    known = np.full(n, -1)
    with _ctx(n, E) as h:
        h.insert_trace(t, 0, E)
        for kw in (dict(null=("ctx",)), dict(null=("known",)), dict(null=("out",)), dict(null=("count",)),
                   dict(graph=-1), dict(graph=1), dict(cap=-1)):
            cap = kw.pop("cap", E)
            rc, msg, count, over, cols = _raw(h, known, cap, alloc=E + 8, **kw)
            assert rc == 102 and msg.startswith("hgx_diff_wire:"), (kw, rc, msg)
            assert count == -77 and over == -77 and _untouched(cols), kw
        cols, count, _ = h.DiffWire(known)      # and the context still answers
        assert count == E
    with _ctx(16, 1000, shard_devices=[0, 0]) as hs:   # a chain-sharded context
        rc, msg, count, over, cols = _raw(hs, np.full(16, -1), 8)
        assert rc == 102 and "chain-sharded" in msg and count == -77 and _untouched(cols)
    with _ctx(n, E) as hc:                      # no ids: hash is refused, the rest works
        hc.insert_events32(compact_columns(t), 0, E)
        rc, msg, count, over, cols = _raw(hc, known, E)
        assert rc == 102 and "ids are not known" in msg and count == -77 and _untouched(cols)
        rest = [nm for nm in NAMES if nm != "hash"]
        rc, msg, count, over, cols = _raw(hc, known, E, names=rest)
        assert rc == 0 and count == E, msg
        _same({nm: a[:E] for nm, a in cols.items()}, _expected(t, wire, np.arange(E)), names=rest)
        got, count, _ = hc.DiffWire(known)      # the wrapper's default leaves hash out there
        assert sorted(got) == sorted(rest) and count == E


# ---- 6. after a prune -------------------------------------------------------------------------
def test_after_prune_to_frame():
    from test_gpu_prune import _concat
    n, cap, sync = 8, 2000, 200
    t = gtrace.gossip(n, 3200, 88)
    o = hgref.Oracle(n)
    with _ctx(n, cap) as h:
        lo = 0
        while lo + sync <= cap:                 # run up to capacity
            for x in (h, o):
                x.insert_trace(t, lo, lo + sync)
            h.RunConsensus()
            assert not o.run_consensus()[0]
            lo += sync
        f = o.get_frame()
        sub, new = hgref.remap_after_reset(t, f["events"], f)
        assert (sub.sp != UNKNOWN).all() and (sub.op != UNKNOWN).all()
        assert list(h.PruneToFrame()) == f["events"] and len(f["events"]) + 2 * sync <= cap
        o.reset(*hgref.frame_root_arrays(f))
        o.insert_trace(sub)
        h.RunConsensus()
        assert not o.run_consensus()[0]
        res = sub
        for _ in range(2):                      # two more syncs on the rooted context
            part, new = hgref.remap_after_reset(t, list(range(lo, lo + sync)), f, new)
            assert (part.sp != UNKNOWN).all() and (part.op != UNKNOWN).all()
            for x in (h, o):
                x.insert_trace(part)
            h.RunConsensus()
            assert not o.run_consensus()[0]
            res = _concat(res, part)
            lo += sync
        E = res.E
        assert h.num_events() == E
        coded = res.op < -1
        assert (res.op[coded] == ROOT_Y).any() or (res.op[coded] == ROOT_OTHER).any()
        root = np.where(res.op == ROOT_Y, 1, np.where(res.op == ROOT_OTHER, 2, 0))
        wire = np.array([o.wire(g) for g in range(E)], np.int64)   # (a root-coded other-parent: -1 / -1)
        assert (wire[coded, 1:] == -1).all()
        root_index = np.array([r[2] for r in f["roots"]])
        assert [h.GetRoot(p)["Index"] for p in range(n)] == list(root_index) and (root_index >= 0).any()
        for known in (root_index.copy(), _known_of(res, E - 300, n).clip(min=root_index)):
            sel = _select(res, E, known)
            cols, count, over = h.DiffWire(known)
            assert count == len(sel) > 0 and not over
            _same(cols, _expected(res, wire, sel, root=root))
            assert ((cols["other_parent_creator"] == -1) & (cols["other_parent_index"] == -1))[cols["root_parent"] > 0].all()
            # the existing host route on the same context
            spi, opc, opi = h.wire_info()
            assert np.array_equal(cols["self_parent_index"], spi[sel]) and np.array_equal(cols["other_parent_creator"], opc[sel])
            assert np.array_equal(cols["other_parent_index"], opi[sel])
        cols, count, _ = h.DiffWire(root_index)
        assert count == E and (cols["root_parent"] > 0).sum() == coded.sum() > 0
        for p in range(n):                      # every chain's first row: SelfParentIndex = Root.Index
            rows = np.nonzero(cols["creator_id"] == p)[0]
            assert len(rows) and cols["self_parent_index"][rows[0]] == root_index[p] == cols["index"][rows[0]] - 1
        p = int(np.argmax(root_index))
        late = root_index.copy()
        late[p] -= 1                            # one below the oldest kept Index minus one
        with pytest.raises(HgxError) as ei:
            h.DiffWire(late)
        assert ei.value.code == 2 and ei.value.msg == "\x03, Too Late"


# ---- 7. a batched context ---------------------------------------------------------------------
def test_batched_context_graph_ids():
    n, E0, E1 = 4, 2500, 2300
    t0, w0 = _traced(n, E0, 61)
    t1, w1 = _traced(n, E1, 62)
    tb = gtrace.concat_graphs([t0, t1])
    with _ctx(n, E0 + E1, graphs=2) as h:
        h.insert_trace(tb)
        for g, (tg, wg, off) in enumerate(((t0, w0, 0), (t1, w1, E0))):
            known = _known_of(tg, tg.E - 500, n)
            sel = _select(tb, tb.E, known, c0=g * n)
            assert len(sel) > 0 and (sel >= off).all() and (sel < off + tg.E).all()
            cols, count, over = h.DiffWire(known, graph=g)
            assert count == len(sel) and not over
            _same(cols, _expected(tb, wg, sel, c0=g * n, wire_off=off))
            assert cols["creator_id"].max() < n and cols["other_parent_creator"].max() < n
            assert list(h.Known(g)) == list(_known_of(tg, tg.E, n))


# ---- 8. straight after a split insert ---------------------------------------------------------
@pytest.mark.parametrize("compact", [False, True])
def test_after_split_insert_payload_is_joined(compact):
    """hgx_insert_and_run copies the payload columns beside DivideRounds (the compact form lands S
    straight in the store, after the call's other work): the gather must see them complete."""
    from babble_amd.hashgraph import compact_columns
    n, E = 64, 70000
    t = gtrace.gossip(n, E, 71)
    names = ["gid", "timestamp_ns", "sig_s", "ntx", "tx_nil"]
    with _ctx(n, E) as h:
        if compact:
            h.insert_and_run32(compact_columns(t))
        else:
            h.insert_and_run(t)
        cols, count, _ = h.DiffWire(np.full(n, -1), columns=names)
    assert count == E and np.array_equal(cols["gid"], np.arange(E))
    assert np.array_equal(cols["timestamp_ns"], t.ts) and np.array_equal(cols["sig_s"], t.s)
    assert np.array_equal(cols["ntx"], t.ntx) and np.array_equal(cols["tx_nil"], t.txnil)


# ---- 9. the playbooks -------------------------------------------------------------------------
def test_core_playbooks_served_by_diff_wire(plays):
    """node/core_test.go's playbooks with every Core on its own context: each sync is
    DiffWire(receiver.Known()) on the sender fed straight into insert_wire on the receiver, then the
    new head and RunConsensus. Must equal the oracle-backed Core simulation, and serving requests
    leaves the sender's results as they were."""
    from babble_amd.hashgraph import Hashgraph
    for fx in ("core_consensus", "core_ff"):
        p = plays[fx]
        n = p["n"]
        fac = hgref.EventFactory(fx, n)
        so = hgref.CoreSim(fx, n, lambda m: hgref.Oracle(m))
        hexes = {}
        cores = [dict(h=Hashgraph(n, capacity=4096), hexes=[], pool=[], head="", seq=0) for _ in range(n)]
        try:
            def make(c, index, sp_hex, op_hex, txs):
                e = fac.make(c, index, sp_hex, op_hex, txs, f"ev{len(hexes)}")
                hexes[e["hex"]] = e
                return e

            def insert_local(core, e, sp, op):
                core["h"].insert_arrays([e["creator"]], [e["index"]], [sp], [op], [e["ts"]],
                                        np.frombuffer(e["hash"], np.uint8).reshape(1, 32),
                                        np.frombuffer(e["s"], np.uint8).reshape(1, 32), [len(e["txs"] or [])],
                                        [1 if e["txs"] is None else 0])
                core["hexes"].append(e["hex"])

            for i in range(n):
                e = make(i, 0, "", "", None)
                insert_local(cores[i], e, -1, -1)
                cores[i]["head"] = e["hex"]
            served = 0
            for frm, to, pl in p["playbook"]:
                src, dst = cores[frm], cores[to]
                w, count, over = src["h"].DiffWire(dst["h"].Known())
                assert not over and count == len(w["gid"])
                if count:
                    # the body store is keyed by gid: the ids must be the events' own
                    es = [hexes[src["hexes"][int(g)]] for g in w["gid"]]
                    assert [e["hash"] for e in es] == [w["hash"][k].tobytes() for k in range(count)]
                    assert not w["root_parent"].any()
                    dst["h"].insert_wire(w["creator_id"], w["index"], w["self_parent_index"], w["other_parent_creator"],
                                         w["other_parent_index"], w["timestamp_ns"], w["hash"], w["sig_s"], w["ntx"],
                                         w["tx_nil"])
                    dst["hexes"].extend(e["hex"] for e in es)
                    served += count
                dst["pool"].extend(x.encode() for x in pl)
                if count or dst["pool"]:
                    other = dst["hexes"][-1] if count else ""
                    ne = make(to, dst["seq"] + 1, dst["head"], other, list(dst["pool"]))
                    insert_local(dst, ne, dst["hexes"].index(dst["head"]), dst["hexes"].index(other) if other else -1)
                    dst["head"], dst["seq"], dst["pool"] = ne["hex"], dst["seq"] + 1, []
                dst["h"].RunConsensus()
                so.sync_and_run(frm, to, [x.encode() for x in pl])
            assert served > n
            for c in range(n):
                h = cores[c]["h"]
                got = [cores[c]["hexes"][int(x)] for x in h.ConsensusEvents()]
                assert got == so.consensus_hex(c), (fx, c)
                assert h.LastConsensusRound() == so.backends[c].last_consensus_round()
                before = h.results()
                _, count, _ = h.DiffWire(np.full(n, -1))
                assert count == h.num_events()
                after = h.results()
                for k in ("round", "witness", "famous", "rr", "cts", "order"):
                    assert np.array_equal(np.asarray(before[k]), np.asarray(after[k])), k
                for k in ("last_round", "undecided", "lcr", "lcre", "consensus_tx", "pending_loaded", "blocks"):
                    assert before[k] == after[k], k
        finally:
            for c in cores:
                c["h"].close()
