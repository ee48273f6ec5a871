"""hgx_insert_wire_bodies: a SyncResponse inserted from its wire fields alone (no hash, parents as
(creator id, Index)): parents resolved, ids hashed, signatures verified and events inserted on the device.

Expected values never come from the new call: ids are the chain's (tests/bodyref.py, libcrypto
signatures), parent gids the trace's own or tests/wireref.py's restatement of ReadWireInfo, consensus
the oracle's. The window kernel works in chunks of 2 048 gids (kWireChunk, hgx_wire.hip): the resident
sets sit on both sides of one and two chunk boundaries. Every context opened here is closed."""
import ctypes as C
import functools

import numpy as np
import pytest

import bodyref
import hgref
import wireref
from babble_amd import _lib
from babble_amd import trace as gtrace
from babble_amd._lib import HgxError, hgx_error, ptr
from babble_amd.hashgraph import Hashgraph, body_columns, compact_columns, wire_body_columns

pytestmark = pytest.mark.gpu

SELF_PARENT = "CheckSelfParent: Self-parent not last known event by creator"
_OPEN = []


@pytest.fixture(autouse=True)
def _close_contexts():
    yield
    while _OPEN:
        _OPEN.pop().close()


def _hg(c, cap=None, keys=True, **kw):
    h = Hashgraph(c.n, capacity=max(cap or c.t.E, 16), **kw)
    _OPEN.append(h)
    if keys:
        h.set_participant_keys(c.keys)
    return h


def _same_consensus(h, t):
    a, b = h.results(), hgref.oracle_run(t).results()
    for k in ("round", "witness", "famous", "rr", "cts"):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    assert list(a["order"]) == list(b["order"])
    assert a["lcr"] == b["lcr"] and a["undecided"] == b["undecided"]


def _wire(h, c, w, lo, hi):
    """One call on chain events [lo, hi) of the whole-chain wire columns w: ids and parents as the chain's"""
    ids, sp, op = h.insert_wire_bodies(w, lo, hi)
    assert np.array_equal(ids, c.ids[lo:hi]), np.nonzero((ids != c.ids[lo:hi]).any(axis=1))[0][:5]
    assert np.array_equal(sp, c.t.sp[lo:hi]) and np.array_equal(op, c.t.op[lo:hi])


@functools.lru_cache(maxsize=None)
def _chain64():
    return bodyref.chain(64, 4200, 9)


@functools.lru_cache(maxsize=None)
def _wire_of(n, E, seed):
    c = bodyref.chain(n, E, seed)
    return c, wireref.wire_cols(c)


# ---- 1. whole traces from an empty context in several syncs ------------------------------------
@pytest.mark.parametrize("n,E,seed,calls", [(2, 150, 3, 3), (4, 200, 1, 4), (16, 600, 2, 5), (128, 1024, 4, 3)])
def test_whole_trace_in_several_syncs(n, E, seed, calls):
    c, w = _wire_of(n, E, seed)
    # the restatement of the resolution rule gives the trace's own parents
    sp, op, m, code, _ = wireref.resolve(wireref.Store(n), w)
    assert (m, code) == (E, 0) and sp == list(c.t.sp) and op == list(c.t.op)
    h = _hg(c)
    cuts = [E * k // calls + (7 * k) % 5 for k in range(calls)] + [E]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        _wire(h, c, w, lo, hi)
        assert h.num_events() == hi
    for g in (0, 1, E // 2, E - 1):
        assert h.event_id(g) == bytes(c.ids[g])
    h.RunConsensus()
    _same_consensus(h, c.t)


# ---- 2. window edges ---------------------------------------------------------------------------
@pytest.mark.parametrize("R", [0, 1, 2047, 2048, 2049, 4097])
def test_window_edges(R):
    """R resident events (inserted with their ids), the next 100 as wire bodies, then hand-made events of
    four different creators whose other-parents sit on the chunk boundary, at a chain's Index 0 (the
    deepest window) and at a chain's head."""
    c = _chain64()
    t, w = c.t, wireref.wire_cols(c, np.arange(R, R + 100))
    h = _hg(c)
    if R:
        h.insert_trace(t, 0, R)
    ids, sp, op = h.insert_wire_bodies(w)
    assert np.array_equal(ids, c.ids[R:R + 100])
    assert np.array_equal(sp, t.sp[R:R + 100]) and np.array_equal(op, t.op[R:R + 100])
    E0 = R + 100
    if R < 2047:
        assert h.num_events() == E0
        return
    # the first event after E0 of four creators (their self-parents are resident, they are independent)
    nxt = {}
    for k in range(E0, t.E):
        if t.sp[k] < E0:
            nxt.setdefault(int(t.creator[k]), k)
    ks = sorted(nxt.values())[:4]
    cr0 = int(t.creator[0])
    head = max(g for g in range(E0) if t.creator[g] not in [t.creator[k] for k in ks])
    targets = [0, head, 2047, 2048][:len(ks)]   # (R = 4 097 leaves three events: gid 2 048 is the others' case)
    assert t.index[0] == 0 and int(t.creator[0]) == cr0 and len(ks) >= 3
    r, s, want = c.r.copy(), t.s.copy(), []
    for k, g in zip(ks, targets):
        r[k], s[k], i = wireref.resigned(c, k, int(t.sp[k]), g)
        want.append(i)
    x = wireref.wire_cols(c, ks, r=r, s=s, other_parent_creator=t.creator[targets].astype(np.int32),
                          other_parent_index=t.index[targets].astype(np.int64))
    ids, sp, op = h.insert_wire_bodies(x)
    assert np.array_equal(ids, np.array(want)) and list(sp) == [int(t.sp[k]) for k in ks] and list(op) == targets
    assert h.num_events() == E0 + len(ks) and h.event_id(E0 + 2) == bytes(want[2])


@pytest.mark.parametrize("n,n_silent,E,R", [(3, 1, 400, 250), (1024, 341, 1500, 1000)])
def test_silent_creators_have_empty_windows(n, n_silent, E, R):
    """A third of the creators never speak: their windows are empty; n = 1 024 fills the LDS table."""
    t = gtrace.gossip(n, E, 50 + n, n_silent=n_silent, stale_prob=0.1, stale_depth=2)
    c = bodyref.build(t, [t.txs(i) for i in range(E)])
    assert len(set(c.t.creator.tolist())) <= n - n_silent
    h = _hg(c)
    h.insert_trace(c.t, 0, R)
    _wire(h, c, wireref.wire_cols(c), R, E)
    h.RunConsensus()
    _same_consensus(h, c.t)


# ---- 3. purely in-batch parents ----------------------------------------------------------------
def test_in_batch_parents_only():
    c, w = _wire_of(4, 200, 1)
    h = _hg(c)
    _wire(h, c, w, 0, 200)   # an empty context: nothing resident, no window
    # on a context with residents: a batch that names none of them (four more creators' first events)
    c8 = bodyref.manual(8, [0, 1, 2, 3, 0, 4, 5, 6, 7, 5, 4], [-1, -1, -1, -1, 0, -1, -1, -1, -1, 6, 5],
                        [-1, -1, -1, -1, 1, -1, -1, -1, -1, 8, 9], [[b"t%d" % k] for k in range(11)])
    h8 = _hg(c8)
    w8 = wireref.wire_cols(c8)
    _wire(h8, c8, w8, 0, 5)
    _wire(h8, c8, w8, 5, 11)


def test_forked_batch_wider_than_a_workgroup():
    """test_gpu_event_bodies' construction: 1 500 events without parents at n = 4, one level wider than
    the id pass's workgroup; the fifth event is a fork."""
    E = 1500
    none = np.full(E, -1, np.int64)
    c = bodyref.manual(4, np.arange(E) % 4, none, none, [[]] * E)
    h = _hg(c)
    with pytest.raises(HgxError) as ei:
        h.insert_wire_bodies(wireref.wire_cols(c))
    assert ei.value.msg == SELF_PARENT and ei.value.inserted == 4 and np.array_equal(ei.value.ids, c.ids[:4])
    assert list(ei.value.self_parent) == [-1] * 4 and h.num_events() == 4


# ---- 4. errors ---------------------------------------------------------------------------------
R4 = 100   # resident events of the error cases


def _fails(h, c, w, p, code, msg, lo=R4, hi=200):
    """The batch [lo, hi) fails at batch position p: the prefix is kept, the good tail completes."""
    with pytest.raises(HgxError) as ei:
        h.insert_wire_bodies(w, lo, hi)
    e = ei.value
    assert (e.code, e.msg, e.inserted) == (code, msg, p), (e.code, e.msg, e.inserted)
    assert h.num_events() == lo + p and np.array_equal(e.ids, c.ids[lo:lo + p])
    assert np.array_equal(e.self_parent, c.t.sp[lo:lo + p]) and np.array_equal(e.other_parent, c.t.op[lo:lo + p])
    if p:
        assert h.event_id(lo + p - 1) == bytes(c.ids[lo + p - 1])
    _wire(h, c, wireref.wire_cols(c), lo + p, c.t.E)
    h.RunConsensus()
    assert list(h.ConsensusEvents()) == list(hgref.oracle_run(c.t).results()["order"])


def _resident(c):
    h = _hg(c)
    h.insert_bodies(c.cols, 0, R4)
    return h


def _with(c, **repl):
    rows = wireref.wire_rows(c.t)
    for nm, (k, v) in repl.items():
        rows[nm] = rows[nm].copy()
        rows[nm][k] = v
    return wire_body_columns(rows, c.r, c.txs), rows


def test_not_found_above_the_head():
    c = bodyref.chain(4, 200, 1)
    t = c.t
    k = next(k for k in range(130, 200) if t.op[k] >= 0)
    oc = int(t.creator[t.op[k]])
    above = int(max(t.index[g] for g in range(k) if t.creator[g] == oc)) + 1
    w, rows = _with(c, other_parent_index=(k, above))
    _, _, m, code, msg = wireref.resolve(wireref.store_of(t, R4), rows, R4, 200)
    assert (m, code, msg) == (k - R4, 1, wireref.rune(above) + ", Not Found")
    _fails(_resident(c), c, w, k - R4, code, msg)


def test_not_found_for_a_parent_at_a_later_position():
    c = bodyref.chain(4, 200, 1)
    t = c.t
    k = next(k for k in range(130, 190) if t.op[k] >= 0)
    q = next(q for q in range(k + 1, 200) if t.creator[q] != t.creator[k])   # the first later event of another creator
    w, rows = _with(c, other_parent_creator=(k, int(t.creator[q])), other_parent_index=(k, int(t.index[q])))
    _, _, m, code, msg = wireref.resolve(wireref.store_of(t, R4), rows, R4, 200)
    assert (m, code, msg) == (k - R4, 1, wireref.rune(int(t.index[q])) + ", Not Found")
    _fails(_resident(c), c, w, k - R4, code, msg)


def test_both_panics():
    c = bodyref.chain(4, 200, 1)
    k = next(k for k in range(130, 200) if c.t.op[k] >= 0)
    for cid in (4, -1):
        w, _ = _with(c, creator_id=(k, cid))
        _fails(_resident(c), c, w, k - R4, 300, wireref.PANIC_CREATOR)
    for cid in (4, -1):
        w, _ = _with(c, other_parent_creator=(k, cid))
        _fails(_resident(c), c, w, k - R4, 300, wireref.PANIC_OTHER)
    # an other-parent creator that is not read (index < 0) panics nothing
    k2 = next(k for k in range(R4, 200) if c.t.op[k] < 0) if (c.t.op[R4:] < 0).any() else None
    if k2 is not None:
        w, _ = _with(c, other_parent_creator=(k2, 77))
        _wire(_resident(c), c, w, R4, 200)


@pytest.mark.parametrize("what", ["tx", "ts", "opi"])
def test_tampered_event_fails_verify(what):
    c = bodyref.chain(4, 200, 1)
    t = c.t
    k0 = next(k for k in range(110, t.E) if t.ntx[k] > 0 and t.op[k] >= 0)
    if what == "tx":
        txs = list(c.txs)
        txs[k0] = [bytes([txs[k0][0][0] ^ 1]) + txs[k0][0][1:]]
        w = wireref.wire_cols(c, txs=txs)
    elif what == "ts":
        w, _ = _with(c, timestamp_ns=(k0, int(t.ts[k0]) + 1))
    else:   # another resident event of the same creator: resolves, but it is not what was signed
        assert t.index[t.op[k0]] > 0
        w, _ = _with(c, other_parent_index=(k0, int(t.index[t.op[k0]]) - 1))
    _fails(_resident(c), c, w, k0 - R4, 104, "Invalid signature")


def test_good_signature_wrong_self_parent():
    """Event k0 names its creator's last-but-one event as self-parent and is signed that way: Verify
    passes, CheckSelfParent rejects it."""
    c = bodyref.chain(4, 200, 1)
    t = c.t
    k0 = next(k for k in range(120, 200) if t.sp[k] >= 0 and t.sp[t.sp[k]] >= 0)
    j = int(t.sp[t.sp[k0]])
    r, s = c.r.copy(), t.s.copy()
    r[k0], s[k0], _ = wireref.resigned(c, k0, j, int(t.op[k0]))
    rows = wireref.wire_rows(t)
    rows["self_parent_index"] = rows["self_parent_index"].copy()
    rows["self_parent_index"][k0] = t.index[j]
    rows["sig_s"] = s
    _fails(_resident(c), c, wire_body_columns(rows, r, c.txs), k0 - R4, 100, SELF_PARENT)


def test_the_earlier_failure_wins():
    c = bodyref.chain(4, 200, 1)
    t = c.t
    a = next(k for k in range(120, 150) if t.op[k] >= 0)
    b = next(k for k in range(160, 200) if t.op[k] >= 0)
    for sig_at, res_at in ((a, b), (b, a)):
        rows = wireref.wire_rows(t)
        rows["other_parent_index"] = rows["other_parent_index"].copy()
        rows["other_parent_index"][res_at] = 1000   # Not Found
        r = c.r.copy()
        r[sig_at, 7] ^= 4                           # Invalid signature
        w = wire_body_columns(rows, r, c.txs)
        if sig_at < res_at:
            _fails(_resident(c), c, w, sig_at - R4, 104, "Invalid signature")
        else:
            _fails(_resident(c), c, w, res_at - R4, 1, wireref.rune(1000) + ", Not Found")


# ---- 5. equality with the gid route -----------------------------------------------------------
@pytest.mark.parametrize("fail", [False, True])
def test_equals_the_gid_route(fail):
    c = bodyref.chain(16, 600, 2)
    t = c.t
    ts = t.ts.copy()
    if fail:
        ts[470] += 1
    rows = wireref.wire_rows(t)
    rows["timestamp_ns"] = ts
    w, b = wire_body_columns(rows, c.r, c.txs), c.columns(ts=ts)
    out = []
    for wire in (True, False):
        h = _hg(c)
        h.insert_bodies(c.cols, 0, 300)
        try:
            ids = h.insert_wire_bodies(w, 300, 600)[0] if wire else h.insert_bodies(b, 300, 600)
            got = (ids.tobytes(), 300, "")
        except HgxError as e:
            got = (e.ids.tobytes(), e.inserted, f"{e.code} {e.msg}")
        h.RunConsensus()
        res = h.results()
        out.append((got, h.num_events(), h.event_id(h.num_events() - 1), list(h.Known()),
                    {k: np.asarray(v).tolist() if k in ("round", "witness", "famous", "rr", "cts", "order") else v
                     for k, v in res.items()}))
    assert out[0] == out[1]
    assert out[0][0][1:] == ((170, "104 Invalid signature") if fail else (300, ""))


# ---- 6. rooted contexts -----------------------------------------------------------------------
def test_pruned_context_keeps_syncing():
    """test_gpu_bodies_rooted's long run (capacity 400, syncs of 100, a prune before each sync that would
    not fit) with every sync through the wire route; and Too Late below a pruned chain's oldest Index."""
    from test_gpu_bodies_rooted import SHAPES, chain_of, oracle_run
    from test_gpu_parity import compare
    c, run = chain_of(4), oracle_run(4)
    assert run["n_prunes"] >= 3
    w = wireref.wire_cols(c)
    h = _hg(c, SHAPES[4][4])
    late_checked = 0
    pending_late = None
    for x in run["steps"]:
        if x["kind"] == "prune":
            assert list(h.PruneToFrame()) == x["events"]
            h.RunConsensus()
            pending_late = x
            continue
        part, sel = x["part"], x["sel"]
        lo, hi = int(sel[0]), int(sel[-1]) + 1
        if pending_late is not None:   # the first sync after a prune: first a batch that reaches below a chain
            root_index = [r[2] for r in pending_late["roots"]]
            p = int(np.argmax(root_index))
            k = next((k for k in range(lo, hi) if c.t.op[k] >= 0), None)
            if root_index[p] >= 0 and k is not None:
                rows = wireref.wire_rows(c.t, sel)
                rows["other_parent_creator"][k - lo], rows["other_parent_index"][k - lo] = p, root_index[p]
                bad = wire_body_columns(rows, c.r[sel], [c.txs[int(i)] for i in sel])
                before = h.num_events()
                with pytest.raises(HgxError) as ei:
                    h.insert_wire_bodies(bad)
                assert (ei.value.code, ei.value.msg) == (2, wireref.rune(root_index[p]) + ", Too Late")
                assert ei.value.inserted == k - lo and np.array_equal(ei.value.ids, c.ids[lo:k])
                assert list(ei.value.self_parent) == list(part.sp[:k - lo]) and h.num_events() == before + k - lo
                late_checked += 1
                lo = k
            pending_late = None
        ids, sp, op = h.insert_wire_bodies(w, lo, hi)
        assert np.array_equal(ids, c.ids[lo:hi])
        assert np.array_equal(sp, part.sp[lo - int(sel[0]):]) and np.array_equal(op, part.op[lo - int(sel[0]):])
        h.RunConsensus()
    assert late_checked >= 2 and h.num_events() == run["resident"].E
    compare(h, run["oracle"], run["resident"], hashes=False)


def test_fast_forward_join_prints_root_x():
    """Reset + SetRootIds, then wire events whose self-parent index is < 0: creators 0, 1 and 2 continue on
    roots with an id (Root.X = g3, g4, g2), creator 3 on a genesis root; g9's self-parent index resolves."""
    creator = [0, 1, 2, 0, 1, 2, 0, 3, 1, 2]
    sp = [-1, -1, -1, 0, 1, 2, 3, -1, 4, 5]
    op = [-1, -1, -1, 1, 3, -1, 5, -1, 7, 8]
    c = bodyref.manual(4, creator, sp, op, [[b"a"], [], None, [b"bc", b""], [], [b"d"], None, [b"e"], [], [b"f"]])
    hid = lambda g: None if g is None else c.ids[g].tobytes()
    sel = np.arange(5, 10)
    rows = wireref.wire_rows(c.t, sel)
    assert list(rows["self_parent_index"]) == [0, 1, -1, 1, 1]
    rows["self_parent_index"][[0, 1, 3]] = -1   # the parents that are Root.X now
    w = wire_body_columns(rows, c.r[sel], [c.txs[int(i)] for i in sel])
    h = _hg(c, 16)
    h.Reset([1, 1, 0, -1], [0, 0, 0, -1], [0, 0, 0, 0])
    with pytest.raises(HgxError) as ei:   # roots without ids
        h.insert_wire_bodies(w)
    assert ei.value.code == 102 and "hgx_set_root_ids" in ei.value.msg and h.num_events() == 0
    h.SetRootIds([hid(3), hid(4), hid(2), None], [None] * 4, [])
    ids, gsp, gop = h.insert_wire_bodies(w)
    assert np.array_equal(ids, c.ids[sel])
    assert list(gsp) == [-1, -1, -1, -1, 0] and list(gop) == [-1, 0, -1, 2, 3]
    assert bodyref.hex_id(hid(3)).encode() in c.json[6] and b'"Parents":["",""]' in c.json[7]
    # without the roots' ids the same events hash to something else
    h2 = _hg(c, 16)
    h2.Reset([1, 1, 0, -1], [0, 0, 0, -1], [0, 0, 0, 0])
    h2.SetRootIds([None] * 4, [None] * 4, [])
    with pytest.raises(HgxError) as ei:
        h2.insert_wire_bodies(w)
    assert ei.value.msg == "Invalid signature" and ei.value.inserted == 0


# ---- 7. the sync loop -------------------------------------------------------------------------
def test_two_contexts_gossip_end_to_end():
    c = bodyref.chain(16, 600, 2)
    t, E = c.t, 600
    A, B = _hg(c), _hg(c)
    A.insert_bodies(c.cols)
    _wire(B, c, wireref.wire_cols(c), 0, 100)
    rounds = 0
    while B.num_events() < E:
        rows, count, over = A.DiffWire(B.Known(), sync_limit=1000, cap=130)
        assert not over and count == E - B.num_events() and len(rows["gid"]) == min(130, count)
        g = rows["gid"]
        assert np.array_equal(rows["hash"], c.ids[g])   # (A's body store is keyed by gid)
        ids, sp, op = B.insert_wire_bodies(wire_body_columns(rows, c.r[g], [c.txs[int(i)] for i in g]))
        assert np.array_equal(ids, c.ids[g]) and np.array_equal(sp, t.sp[g]) and np.array_equal(op, t.op[g])
        B.RunConsensus()
        rounds += 1
    assert rounds == 4
    _, count, _ = A.DiffWire(B.Known())
    assert count == 0
    b, o = B.results(), hgref.oracle_run(t, chunk=None).results()
    A.RunConsensus()
    a = A.results()
    for k in ("round", "witness", "famous", "rr", "cts", "order"):
        assert np.array_equal(np.asarray(b[k]), np.asarray(o[k])), k
        assert np.array_equal(np.asarray(a[k]), np.asarray(o[k])), k
    assert [B.event_id(g) for g in (0, 99, 100, 599)] == [bytes(c.ids[g]) for g in (0, 99, 100, 599)]


def test_core_playbooks_through_wire_bodies(plays):
    """node/core_test.go's playbooks with every Core on its own context and real signatures: each sync is
    DiffWire(receiver.Known()) on the sender, R and the transactions from the body store by gid, then
    insert_wire_bodies on the receiver, the new head through insert_bodies, RunConsensus. Every Core also
    feeds an oracle of its own; the consensus orders must agree."""
    import hashlib
    ordered = 0
    for fx in ("core_consensus", "core_ff"):
        p = plays[fx]
        n = p["n"]
        keys, _, _ = hgref.sign_batch(n, [0], np.zeros((1, 32), np.uint8))
        events = []   # global: dict(creator, index, sp, op (global ids), ts, txs, r, s, id)

        def make(creator, index, sp_g, op_g, txs):
            pid = lambda g: events[g]["id"] if g >= 0 else None
            ts = hgref.T0_NS + 1000 * len(events)
            bj = bodyref.body_json(txs, pid(sp_g), pid(op_g), bytes(keys[creator]), ts, index)
            d = np.frombuffer(hashlib.sha256(bj).digest(), np.uint8)
            _, r, s = hgref.sign_batch(n, [creator], d[None, :])
            js = hgref.go_event_json(txs, bodyref.hex_id(pid(sp_g)), bodyref.hex_id(pid(op_g)), bytes(keys[creator]),
                                     ts, index, bytes(r[0]), bytes(s[0]))
            events.append(dict(creator=creator, index=index, sp=sp_g, op=op_g, ts=ts, txs=txs, r=r[0], s=s[0],
                               id=hashlib.sha256(js).digest()))
            return len(events) - 1

        cores = []
        for i in range(n):
            h = Hashgraph(n, capacity=4096)
            _OPEN.append(h)
            h.set_participant_keys(keys)
            cores.append(dict(h=h, o=hgref.Oracle(n), local=[], g2l={}, head=-1, seq=0, pool=[]))

        def took(core, g, sp_l, op_l):
            e = events[g]
            rc = core["o"].insert(e["creator"], e["index"], sp_l, op_l, e["ts"], e["id"], bytes(e["s"]), e["txs"])
            assert not rc[0], rc
            core["g2l"][g] = len(core["local"])
            core["local"].append(g)

        def insert_own(core, g):
            e = events[g]
            sp_l = core["g2l"][e["sp"]] if e["sp"] >= 0 else -1
            op_l = core["g2l"][e["op"]] if e["op"] >= 0 else -1
            ids = core["h"].insert_bodies(body_columns([e["creator"]], [e["index"]], [sp_l], [op_l], [e["ts"]],
                                                       e["r"][None, :], e["s"][None, :], [e["txs"]]))
            assert ids[0].tobytes() == e["id"]
            took(core, g, sp_l, op_l)
            core["head"], core["seq"] = g, e["index"]

        for i in range(n):
            insert_own(cores[i], make(i, 0, -1, -1, None))
        served = 0
        for frm, to, pl in p["playbook"]:
            src, dst = cores[frm], cores[to]
            w, count, over = src["h"].DiffWire(dst["h"].Known())
            assert not over
            gs = [src["local"][int(x)] for x in w["gid"]]
            if count:
                assert [events[g]["id"] for g in gs] == [w["hash"][k].tobytes() for k in range(count)]
                want_sp = [dst["g2l"].get(events[g]["sp"], None) if events[g]["sp"] >= 0 else -1 for g in gs]
                ids, sp, op = dst["h"].insert_wire_bodies(
                    wire_body_columns(w, np.array([events[g]["r"] for g in gs]), [events[g]["txs"] for g in gs]))
                assert [x.tobytes() for x in ids] == [events[g]["id"] for g in gs]
                for k, g in enumerate(gs):   # parents in the receiver's own gids, known before the call or in it
                    e = events[g]
                    sp_l = dst["g2l"][e["sp"]] if e["sp"] >= 0 else -1
                    op_l = dst["g2l"][e["op"]] if e["op"] >= 0 else -1
                    assert (int(sp[k]), int(op[k])) == (sp_l, op_l) and want_sp[k] in (None, sp_l)
                    took(dst, g, sp_l, op_l)
                served += count
            dst["pool"].extend(x.encode() for x in pl)
            if count or dst["pool"]:
                insert_own(dst, make(to, dst["seq"] + 1, dst["head"], gs[-1] if count else -1, list(dst["pool"])))
                dst["pool"] = []
            dst["h"].RunConsensus()
            rc = dst["o"].run_consensus()
            assert not rc[0], rc
        assert served > n
        for core in cores:
            assert list(core["h"].ConsensusEvents()) == list(core["o"].consensus_events()), fx
            assert core["h"].LastConsensusRound() == core["o"].last_consensus_round()
        ordered += sum(len(core["h"].ConsensusEvents()) for core in cores)
        while _OPEN:
            _OPEN.pop().close()
    assert ordered > 0


# ---- 8. the mirror ----------------------------------------------------------------------------
def test_straight_after_an_insert_that_dropped_the_mirror():
    c, w = _wire_of(4, 200, 1)
    t = c.t
    h = _hg(c)
    h.insert_bodies(c.cols, 0, 100)
    assert h.ParticipantEvents(1, -1)          # builds the host mirror ...
    h.insert_bodies(c.cols, 100, 101)          # ... and the node's own new event drops it
    _wire(h, c, w, 101, 160)
    # the store views answer from a mirror rebuilt on demand
    st = wireref.store_of(t, 160)
    for p in range(4):
        assert list(h.ParticipantEvents(p, -1)) == st.items[p]
        assert h.ParticipantEvent(p, st.last[p]) == st.items[p][-1]
    spi, opc, opi = h.wire_info()
    rows = wireref.wire_rows(t, np.arange(160))
    assert np.array_equal(spi, rows["self_parent_index"]) and np.array_equal(opi, rows["other_parent_index"])
    k = next(k for k in range(150, 160) if t.op[k] >= 0)
    assert h.ReadWireInfo(int(t.creator[k]), int(rows["self_parent_index"][k]), int(rows["other_parent_creator"][k]),
                          int(rows["other_parent_index"][k])) == (int(t.sp[k]), int(t.op[k]))
    _wire(h, c, w, 160, 200)                   # and again with the mirror present
    h.RunConsensus()
    pt = h.phase_times()
    assert pt["rounds"] > 0 and pt["coords_ms"] >= 0
    _same_consensus(h, t)


# ---- 9. refusals ------------------------------------------------------------------------------
def test_refusals_change_nothing():
    c, w = _wire_of(4, 200, 1)
    from babble_amd.hashgraph import _wire_bodies_of, _WIRE_BODY_FIELDS
    a, full = _wire_bodies_of(w, 50, 200)

    def refused(h, ev, why, count=150, ctx=True):
        ids, sp, op = np.full((150, 32), 0x5A, np.uint8), np.full(150, 77, np.int64), np.full(150, 78, np.int64)
        before = h.num_events()
        err, n_ins = hgx_error(), C.c_int64(9)
        rc = h.L.hgx_insert_wire_bodies(h.ctx if ctx else None, C.byref(ev), count, ptr(ids), ptr(sp), ptr(op),
                                        C.byref(n_ins), C.byref(err))
        msg = err.msg.decode()
        assert rc == 102 and msg.startswith("hgx_insert_wire_bodies: ") and why in msg, msg
        assert n_ins.value == 0 and (ids == 0x5A).all() and (sp == 77).all() and (op == 78).all()
        assert h.num_events() == before

    h = _hg(c)
    h.insert_bodies(c.cols, 0, 50)
    for nm in _WIRE_BODY_FIELDS[:-1]:
        refused(h, _lib.hgx_wire_bodies(*[None if x == nm else ptr(a[x]) for x in _WIRE_BODY_FIELDS]), "null column")
    bad = dict(a, ntx=np.where(np.arange(150) == 9, -2, a["ntx"]).astype(np.int32))
    refused(h, _lib.hgx_wire_bodies(*[ptr(bad[x]) for x in _WIRE_BODY_FIELDS]), "ntx below -1")
    refused(h, full, "bad arguments", count=-1)
    refused(h, full, "bad arguments", ctx=False)
    _wire(h, c, w, 50, 200)                     # and the context still takes the batch
    refused(_hg(c, keys=False), full, "participant keys not set")
    h32 = _hg(c)
    h32.insert_events32(compact_columns(c.t), 0, 50)
    refused(h32, full, "ids not known")
    hr = _hg(c)
    hr.Reset([3] * 4, [1] * 4, [0] * 4)
    refused(hr, full, "hgx_reset")
    hb = _hg(c, keys=False, n_graphs=2)
    refused(hb, full, "batched")
    hs = Hashgraph(16, capacity=1000, shard_devices=[0, 0])
    _OPEN.append(hs)
    refused(hs, full, "chain-sharded")
    hw = _hg(c)
    hw.set_shard(1, 2)
    refused(hw, full, "row-sharded")
