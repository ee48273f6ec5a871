"""The event-id index on the device (hgx_keep_id_index, hgx_id_index_state, hgx_find_events,
hgx_insert_events_by_id) against tests/idindexref.py, the sequential Python model of the
table, and against hgx_insert_event_bodies_claimed fed with the parent codes a host map produces.

Shapes: 4 participants, 64 events, capacity 64, so 128 slots at load 0.5: the smallest table in which
clusters, displacement and wrap-around all occur. The chain is tests/signref.py's: bodyref.chain's trace and
Chain, signed with RFC 6979 nonces, so its ids are the same in every process (bodyref.chain signs with
libcrypto's random nonces: its ids, and with them the table's shape, differ from run to run). The seed was
chosen with the model so that the table wraps (asserted below, so the fixture cannot lose the property)."""
import numpy as np
import pytest

import bodyref
import hgref
import idindexref
import signref
import wireref
from babble_amd._lib import HgxError
from babble_amd.hashgraph import Hashgraph, compact_columns
from hgref import ROOT_OTHER, ROOT_Y, UNKNOWN
from test_gpu_prune import remap_frame

pytestmark = pytest.mark.gpu

N, E, SEED, CAP = 4, 64, 2, 64
HGX_ERR_INVALID = 102

_OPEN = []   # the contexts a test made


@pytest.fixture(autouse=True)
def _close_contexts():
    yield
    while _OPEN:
        _OPEN.pop().close()


def chain():
    return signref.chain(N, E, SEED)


def _hg(c, keep=True, cap=CAP, bodies=False, n_graphs=1):
    h = Hashgraph(c.n // n_graphs, capacity=cap, n_graphs=n_graphs)
    _OPEN.append(h)
    if bodies:
        h.KeepBodies(0, 0)
    h.set_participant_keys(c.keys)
    if keep:
        h.KeepIdIndex()
    return h


def test_fixture_wraps():
    st = idindexref.model_of(chain().ids, CAP).state()
    print("fixture", st)
    assert st["slots"] == 128 and st["entries"] == E
    assert st["wrapped"] >= 1 and st["total_displacement"] >= 16, st


def absent_queries(ids, model, rng):
    """Ids no resident event has: random ones, a resident id with its last byte flipped, forged ids that
    share home and tag with a resident one, and forged ids whose home is the last slot."""
    ids = np.asarray(ids, np.uint8)
    q = [rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(8)]
    for k in rng.choice(len(ids), 8, replace=False):
        f = ids[k].copy()
        f[31] ^= 1
        q.append(f)
        q.append(idindexref.forge_same_home_and_tag(ids[k]))
    q += [idindexref.forge_home(model.slots - 1, salt) for salt in range(4)]
    q = np.stack(q)
    assert all(model.find(r) == -1 for r in q)
    return q


def check_index(h, ids, cap=CAP, seed=1):
    """The state equals the model over `ids` (gid order) in all five fields; every id is found under its
    gid in shuffled order; absent ids are not found."""
    ids = np.asarray(ids, np.uint8).reshape(-1, 32)
    model = idindexref.model_of(ids, cap)
    st = h.IdIndexState()
    print("state", st, "model", model.state())
    assert st == model.state()
    rng = np.random.default_rng(seed)
    perm = rng.permutation(len(ids))
    want = np.asarray([model.find(ids[k]) for k in perm], np.int64)
    assert np.array_equal(want, perm)   # (the chain's ids are distinct)
    assert np.array_equal(h.FindEvents(ids[perm]), want)
    q = absent_queries(ids, model, rng)
    assert (h.FindEvents(q) == -1).all()
    # present and absent in one call
    mix = np.concatenate([q[:5], ids[perm[:7]], q[5:9]])
    assert list(h.FindEvents(mix)) == [-1] * 5 + list(perm[:7]) + [-1] * 4
    assert h.FindEvents(np.zeros((0, 32), np.uint8)).shape == (0,)


# ----------------------------------------------------------------------------- state and find
def test_state_and_find():
    c = chain()
    h = _hg(c)
    assert h.IdIndexState() == dict(kept=1, slots=128, entries=0, total_displacement=0, wrapped=0)
    assert (h.FindEvents(c.ids[:3]) == -1).all()
    # a lone lane, a wave that is not full, the rest
    for lo, hi in ((0, 1), (1, 64), (64, E)):
        if hi > lo:
            assert np.array_equal(h.insert_bodies(c.cols, lo, hi), c.ids[lo:hi])
    check_index(h, c.ids)
    h.KeepIdIndex()   # idempotent
    check_index(h, c.ids, seed=2)


def test_keep_after_the_fact():
    c = chain()
    h = _hg(c, keep=False)
    assert h.IdIndexState()["kept"] == 0
    with pytest.raises(HgxError) as ei:
        h.FindEvents(c.ids[:1])
    assert ei.value.code == HGX_ERR_INVALID and ei.value.msg == "hgx_find_events: id index not kept"
    h.insert_bodies(c.cols, 0, 40)
    h.KeepIdIndex()
    check_index(h, c.ids[:40])
    h.insert_bodies(c.cols, 40, E)
    check_index(h, c.ids)


# ----------------------------------------------------------------------------- every id-carrying path
@pytest.mark.parametrize("path", ["wide", "claimed", "sign", "wire", "bootstrap"])
def test_every_id_carrying_path(path, tmp_path):
    c = chain()
    ids = c.ids
    if path == "wide":
        h = _hg(c)
        assert h.insert_trace(c.t, 0, 30) == 30 and h.insert_trace(c.t, 30, E) == E - 30
    elif path == "claimed":
        h = _hg(c)
        assert h.insert_bodies_claimed(c.cols, c.ids, lo=0, hi=30) == 30
        assert h.insert_bodies_claimed(c.cols, c.ids, lo=30) == E - 30
    elif path == "sign":
        h = _hg(c)
        h.set_signing_keys(signref.priv_bytes(N))
        a = dict(creator=c.t.creator, index=c.t.index, sp=c.t.sp, op=c.t.op, ts=c.t.ts, r=None, s=None, txs=c.txs)
        from babble_amd.hashgraph import body_columns
        _, _, ids, k = h.sign_insert_event_bodies(body_columns(**a))
        assert k == E and np.array_equal(ids, c.ids)
    elif path == "wire":
        h = _hg(c)
        w = wireref.wire_cols(c)
        got = h.insert_wire_bodies(w, 0, 30)
        assert np.array_equal(got[0], c.ids[:30])
        got = h.insert_wire_bodies(w, 30, E)
        assert np.array_equal(got[0], c.ids[30:])
    else:
        src = _hg(c, keep=False, bodies=True)
        src.insert_bodies(c.cols)
        src.RunConsensus()
        p = str(tmp_path / "ck.hgx")
        src.save_bodies(p)
        h = _hg(c)
        h.insert_bodies(c.cols, 0, 10)   # (Bootstrap runs on an empty context: the table is emptied, then rebuilt)
        h.clear()
        h.Bootstrap(p)
        assert h.num_events() == E
    check_index(h, ids)


# ----------------------------------------------------------------------------- invalidation
def test_insert_without_ids_invalidates_until_clear():
    c = chain()
    h = _hg(c)
    h.insert_bodies(c.cols, 0, 20)
    assert h.insert_events32(compact_columns(c.t), 20, 40) == 20
    st = h.IdIndexState()
    assert st["kept"] == 2 and st["slots"] == 128
    with pytest.raises(HgxError) as ei:
        h.FindEvents(c.ids[:4])
    assert ei.value.code == HGX_ERR_INVALID and "ids not known" in ei.value.msg
    assert ei.value.msg.startswith("hgx_find_events: ")
    sp_ids, op_ids, flags = parents_as_ids(c)
    with pytest.raises(HgxError) as ei:
        h.insert_events_by_id(c.cols, c.ids, sp_ids, op_ids, flags, 40, 50)
    assert ei.value.code == HGX_ERR_INVALID and "ids not known" in ei.value.msg and h.num_events() == 40
    h.clear()
    assert h.IdIndexState() == dict(kept=1, slots=128, entries=0, total_displacement=0, wrapped=0)
    assert (h.FindEvents(c.ids[:4]) == -1).all()
    h.set_participant_keys(c.keys)
    h.insert_bodies(c.cols)
    check_index(h, c.ids)


def test_refusals():
    c = chain()
    hb = Hashgraph(2, capacity=CAP, n_graphs=2)
    _OPEN.append(hb)
    with pytest.raises(HgxError) as ei:
        hb.KeepIdIndex()
    assert (ei.value.code, ei.value.msg) == (HGX_ERR_INVALID, "hgx_keep_id_index: not available on a batched context")
    assert hb.IdIndexState()["kept"] == 0
    h = _hg(c, keep=False)
    sp_ids, op_ids, flags = parents_as_ids(c)
    with pytest.raises(HgxError) as ei:
        h.insert_events_by_id(c.cols, c.ids, sp_ids, op_ids, flags)
    assert (ei.value.code, ei.value.msg) == (HGX_ERR_INVALID, "hgx_insert_events_by_id: id index not kept")
    assert ei.value.inserted == 0 and h.num_events() == 0
    h.KeepIdIndex()
    with pytest.raises(HgxError) as ei:   # a flag names a column that is not there
        h.insert_events_by_id(c.cols, c.ids, sp_ids, None, flags)
    assert (ei.value.code, ei.value.msg) == (HGX_ERR_INVALID, "hgx_insert_events_by_id: null parent id column")
    assert h.num_events() == 0
    # ... and a column nobody names may be missing
    n, sp, op = h.insert_events_by_id(c.cols, c.ids, None, None, np.zeros(E, np.uint8), 0, 1)
    assert (n, list(sp), list(op)) == (1, [-1], [-1])


# ----------------------------------------------------------------------------- prune
def pruned(c, h):
    """RunConsensus and PruneToFrame on a context holding the chain; the old gid of each new gid."""
    h.RunConsensus()
    old = np.asarray(h.PruneToFrame(), np.int64)
    assert 0 < len(old) < E   # (something was pruned)
    return old


def test_prune_rebuilds_the_index_under_the_new_gids():
    c = chain()
    h = _hg(c)
    h.insert_bodies(c.cols)
    old = pruned(c, h)
    want = np.full(E, -1, np.int64)
    want[old] = np.arange(len(old))
    assert np.array_equal(h.FindEvents(c.ids), want)
    check_index(h, c.ids[old])
    h.RunConsensus()
    check_index(h, c.ids[old], seed=3)


# ----------------------------------------------------------------------------- insert by id
def parents_as_ids(c, t=None):
    """Body.Parents of the chain's events as a Go Event holds them: the parents' ids and the flags."""
    t = c.t if t is None else t
    m = len(t.sp)
    sp_ids, op_ids, flags = np.zeros((m, 32), np.uint8), np.zeros((m, 32), np.uint8), np.zeros(m, np.uint8)
    for k in range(m):
        if t.sp[k] >= 0:
            sp_ids[k], flags[k] = c.ids[t.sp[k]], flags[k] | 1
        if t.op[k] >= 0:
            op_ids[k], flags[k] = c.ids[t.op[k]], flags[k] | 2
    return sp_ids, op_ids, flags


def host_codes(resident, E0, claimed, sp_ids, op_ids, flags):
    """The parent codes a host map (hex id -> gid, filled event after event) produces on an unrooted
    context: resident first, then the lowest earlier batch position, else UNKNOWN."""
    seen, sp, op = {}, [], []

    def look(row):
        b = bytes(row)
        return resident[b] if b in resident else E0 + seen[b] if b in seen else UNKNOWN
    for k in range(len(flags)):
        sp.append(look(sp_ids[k]) if flags[k] & 1 else -1)
        op.append(look(op_ids[k]) if flags[k] & 2 else -1)
        seen.setdefault(bytes(claimed[k]), k)
    return np.asarray(sp, np.int64), np.asarray(op, np.int64)


def same_resident(a, b, m):
    assert a.num_events() == b.num_events() == m
    for g in range(m):
        assert a.event_id(g) == b.event_id(g), g


@pytest.mark.parametrize("split", [(0, E), (0, 20, E)])
def test_by_id_equals_claimed(split):
    c = chain()
    sp_ids, op_ids, flags = parents_as_ids(c)
    a, b = _hg(c, keep=False), _hg(c)
    for lo, hi in zip(split, split[1:]):
        na = a.insert_bodies_claimed(c.cols, c.ids, lo=lo, hi=hi)
        nb, sp, op = b.insert_events_by_id(c.cols, c.ids, sp_ids, op_ids, flags, lo, hi)
        assert na == nb == hi - lo
        assert np.array_equal(sp, c.t.sp[lo:hi]) and np.array_equal(op, c.t.op[lo:hi])
    same_resident(a, b, E)
    check_index(b, c.ids)
    a.RunConsensus()
    b.RunConsensus()
    ra, rb = a.results(), b.results()
    for k in ("round", "witness", "famous", "rr", "cts"):
        assert np.array_equal(np.asarray(ra[k]), np.asarray(rb[k])), k
    assert list(ra["order"]) == list(rb["order"])
    want = hgref.oracle_run(c.t).results()
    assert list(rb["order"]) == list(want["order"]) and np.array_equal(np.asarray(rb["round"]), want["round"])


def _with_other_parent(c, k):
    """The first event at or after k that has an other-parent."""
    return next(j for j in range(k, E) if c.t.op[j] >= 0)


def _failure_case(c, how):
    """(cols, claimed, sp_ids, op_ids, flags, k): the chain with event k made to fail."""
    sp_ids, op_ids, flags = parents_as_ids(c)
    claimed, cols = c.ids.copy(), c.cols
    k = _with_other_parent(c, 30)
    if how == "unknown_other_parent":      # an id nobody holds
        op_ids[k] = np.arange(32, dtype=np.uint8) ^ 0x5C
    elif how == "later_other_parent":      # a later batch position
        op_ids[k] = c.ids[k + 5]
    elif how == "claimed_id_of_another":   # event k's claimed id is event j's
        claimed[k] = c.ids[k - 7]
    else:                                  # one body byte: the timestamp's last digit; the claimed id follows the text
        assert how == "body_byte"
        ts = c.t.ts.copy()
        ts[k] += 1
        cols = c.columns(ts=ts)
        t = c.t
        js = hgref.go_event_json(c.txs[k], bodyref.hex_id(bytes(c.ids[t.sp[k]]) if t.sp[k] >= 0 else None),
                                 bodyref.hex_id(bytes(c.ids[t.op[k]])), bytes(c.keys[t.creator[k]]), int(ts[k]),
                                 int(t.index[k]), bytes(c.r[k]), bytes(c.t.s[k]))
        import hashlib
        claimed[k] = np.frombuffer(hashlib.sha256(js).digest(), np.uint8)
    return cols, claimed, sp_ids, op_ids, flags, k


@pytest.mark.parametrize("resident", [0, 20])
@pytest.mark.parametrize("how,code,msg", [
    ("unknown_other_parent", 101, "CheckOtherParent: Other-parent not known"),
    ("later_other_parent", 101, "CheckOtherParent: Other-parent not known"),
    ("claimed_id_of_another", HGX_ERR_INVALID, "FN: event K: the claimed id is not the event's hash"),
    ("body_byte", 104, "Invalid signature"),
])
def test_by_id_failures_equal_claimed(how, code, msg, resident):
    c = chain()
    cols, claimed, sp_ids, op_ids, flags, k = _failure_case(c, how)
    a, b = _hg(c, keep=False), _hg(c)
    if resident:
        a.insert_bodies(c.cols, 0, resident)
        b.insert_bodies(c.cols, 0, resident)
    res = {bytes(c.ids[g]): g for g in range(resident)}
    sl = slice(resident, E)
    sp, op = host_codes(res, resident, claimed[sl], sp_ids[sl], op_ids[sl], flags[sl])
    assert op[k - resident] == UNKNOWN if how.endswith("other_parent") else op[k - resident] == c.t.op[k]
    full_sp, full_op = c.t.sp.copy(), c.t.op.copy()
    full_sp[sl], full_op[sl] = sp, op
    with pytest.raises(HgxError) as ea:
        a.insert_bodies_claimed(dict(cols, sp=full_sp, op=full_op), claimed, lo=resident)
    with pytest.raises(HgxError) as eb:
        b.insert_events_by_id(cols, claimed, sp_ids, op_ids, flags, resident, E)
    ea, eb = ea.value, eb.value
    print(how, "claimed:", ea.code, ea.msg, ea.inserted, "by id:", eb.code, eb.msg, eb.inserted)
    assert np.array_equal(eb.sp, sp) and np.array_equal(eb.op, op)
    assert ea.code == eb.code == code and ea.inserted == eb.inserted == k - resident
    assert ea.msg == msg.replace("FN", "hgx_insert_event_bodies_claimed").replace("K", str(k - resident))
    assert eb.msg == msg.replace("FN", "hgx_insert_events_by_id").replace("K", str(k - resident))
    same_resident(a, b, k)
    check_index(b, c.ids[:k])


# ----------------------------------------------------------------------------- rooted
def test_by_id_on_a_rooted_context_equals_the_codes():
    """The chain is pruned to its frame (the oracle's), and the frame joins two fresh contexts after
    Reset(frame roots) and SetRootIds: A by the codes remap_frame computes (self-parent -1 = Root.X,
    ROOT_Y, ROOT_OTHER with the entry's id), B by the parents' ids alone. Then the rest of a longer
    chain, whose parents are the frame's events, on both."""
    c = signref.chain(N, 96, SEED)
    t = c.t
    pre = type(t)(t.n, **{k: getattr(t, k)[:E].copy() for k in
                          ("creator", "index", "sp", "op", "ts", "hash", "s", "ntx", "txnil", "tx_seq")})
    o = hgref.Oracle(N)
    o.insert_trace(pre)
    rc, msg = o.run_consensus()
    assert not rc, msg
    f = o.get_frame()
    ev = [int(g) for g in f["events"]]
    sub = remap_frame(pre, f)
    assert (sub.sp != UNKNOWN).all() and (sub.op != UNKNOWN).all() and len(ev) < E
    # the parents cover Root.X with an id, Root.Y and a Root.Others entry
    first = [k for k in range(sub.E) if sub.sp[k] == -1]
    assert any(t.sp[ev[k]] >= 0 for k in first) and (sub.op == ROOT_Y).any() and (sub.op == ROOT_OTHER).any()
    hid = lambda g: bytes(c.ids[g]) if g >= 0 else None
    xs = [hid(r[0]) for r in f["roots"]]
    ys = [hid(r[1]) for r in f["roots"]]
    others = sorted((hid(g), hid(op)) for g, op in f["others"].items())
    roots = hgref.frame_root_arrays(f)
    sel = np.asarray(ev, np.int64)
    from babble_amd.hashgraph import body_columns
    cols = body_columns(t.creator[sel], t.index[sel], sub.sp, sub.op, t.ts[sel], c.r[sel], t.s[sel],
                        [c.txs[g] for g in ev])
    opi = np.zeros((len(ev), 32), np.uint8)
    for k in np.nonzero(sub.op == ROOT_OTHER)[0]:
        opi[k] = c.ids[f["others"][ev[k]]]
    sp_all, op_all, fl_all = parents_as_ids(c)
    cap = len(ev) + t.E - E   # the frame and the rest (a table of its own size: 256 slots)
    a, b = _hg(c, keep=False, cap=cap), _hg(c, cap=cap)
    for h in (a, b):
        h.Reset(*roots)
        h.SetRootIds(xs, ys, others)
    na = a.insert_bodies_claimed(cols, c.ids[sel], other_parent_id32=opi)
    nb, sp, op = b.insert_events_by_id(cols, c.ids[sel], sp_all[sel], op_all[sel], fl_all[sel])
    print("frame", len(ev), "codes", list(sp), list(op))
    assert na == nb == len(ev)
    assert np.array_equal(sp, sub.sp) and np.array_equal(op, sub.op)
    same_resident(a, b, len(ev))
    check_index(b, c.ids[sel], cap=cap)
    # the rest of the longer chain: every parent a resident frame event or an earlier event of the batch
    g2c = {g: k for k, g in enumerate(ev)}
    rest = np.arange(E, t.E)
    for g in rest:
        g2c[int(g)] = len(g2c)
    rsp = np.asarray([g2c[int(x)] if x >= 0 else -1 for x in t.sp[rest]], np.int64)
    rop = np.asarray([g2c.get(int(x), UNKNOWN) if x >= 0 else -1 for x in t.op[rest]], np.int64)
    rcols = body_columns(t.creator[rest], t.index[rest], rsp, rop, t.ts[rest], c.r[rest], t.s[rest],
                         [c.txs[int(g)] for g in rest])
    unknown = np.nonzero(rop == UNKNOWN)[0]
    m = int(unknown[0]) if len(unknown) else len(rest)   # (an other-parent the prune dropped ends both calls alike)
    assert m >= 8
    out = []
    for h, call in ((a, lambda: a.insert_bodies_claimed(rcols, c.ids[rest])),
                    (b, lambda: b.insert_events_by_id(rcols, c.ids[rest], sp_all[rest], op_all[rest], fl_all[rest]))):
        try:
            r = call()
            out.append((0, "", r if h is a else r[0]))
            if h is b:
                assert np.array_equal(r[1], rsp) and np.array_equal(r[2], rop)
        except HgxError as e:
            out.append((e.code, e.msg, e.inserted))
            if h is b:
                # a dropped other-parent is ROOT_OTHER by id (the device's Root.Others check refuses it)
                assert np.array_equal(e.sp, rsp) and np.array_equal(np.where(e.op == ROOT_OTHER, UNKNOWN, e.op), rop)
    print("rest", out)
    assert out[0] == out[1] and out[0][2] == m
    same_resident(a, b, len(ev) + m)
    check_index(b, np.concatenate([c.ids[sel], c.ids[rest[:m]]]), cap=cap)
    a.RunConsensus()
    b.RunConsensus()
    ra, rb = a.results(), b.results()
    for k in ("round", "witness", "famous", "rr", "cts"):
        assert np.array_equal(np.asarray(ra[k]), np.asarray(rb[k])), k
    assert list(ra["order"]) == list(rb["order"])
