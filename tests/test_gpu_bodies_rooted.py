"""Event bodies on rooted contexts (hgx_insert_event_bodies_ext, hgx_set_root_ids):
the device builds the Go-JSON of events whose parents lie outside the store, printing the roots' ids
(Root.X for self-parent -1, Root.Y for HGX_ROOT_Y, the supplied id for HGX_ROOT_OTHER).
  * a node that syncs through the body path, prunes and syncs on, past several times its capacity;
  * a first event whose self-parent is a Root.X with an id, installed by the caller;
  * a fast-forward join: Reset(frame roots), SetRootIds, the frame through the body path, then on;
  * the Root.Others value check, the order of errors at one event, the refusals.

The reference for every id is the chain of tests/bodyref.py over the whole unpruned trace: an id is
the SHA-256 of the event's Go-JSON with its real parents' hex ids, whatever the store still holds, so
equal ids imply equal texts. The oracle runs on the signed trace (hash = the chain's ids, s = the
signatures' S: the coin bit and the sort's tie-break depend on them)."""
import functools

import numpy as np
import pytest

import bodyref
import hgref
from babble_amd import trace as gtrace
from babble_amd._lib import HgxError
from babble_amd.hashgraph import Hashgraph, body_columns
from hgref import ROOT_OTHER, ROOT_Y, UNKNOWN
from test_gpu_parity import compare
from test_gpu_prune import _concat, _sub, remap_frame

pytestmark = pytest.mark.gpu

# (n, events of the gossip trace, seed, sync, cap) of test_gpu_prune.LONG, and the prefix used here
SHAPES = {4: (4, 6000, 85, 100, 400, 2000), 16: (16, 12000, 86, 200, 1000, 3000)}


@functools.lru_cache(maxsize=None)
def chain_of(n):
    """The signed chain of the shape's trace prefix (read-only, shared)."""
    n, E, seed, _, _, K = SHAPES[n]
    t = gtrace.gossip(n, E, seed)
    cut = gtrace.GossipTrace(n, **{k: getattr(t, k)[:K].copy() for k in
                                   ("creator", "index", "sp", "op", "ts", "hash", "s", "ntx", "txnil", "tx_seq")})
    return bodyref.build(cut, [cut.txs(i) for i in range(K)])


def long_run(c, sync, cap, start=None):
    """The oracle's side of a long run over the chain's signed trace (the driver of
    test_gpu_prune.oracle_long_run, taking a trace): the steps (insert: the part with its parents
    in resident gids and its trace gids; prune: the frame) and the final oracle. Root ids are
    tracked as trace gids (None = ""). start = (oracle, resident trace, src, rx, ry, others, lo):
    continue a run whose state the caller built (the fast-forward join)."""
    t = c.t
    n, K = t.n, t.E
    if start is None:
        o, cur, src, rx_id, ry_id, oth_id, lo0 = hgref.Oracle(n), None, [], [None] * n, [None] * n, {}, 0
    else:
        o, cur, src, rx_id, ry_id, oth_id, lo0 = start
        src, rx_id, ry_id, oth_id = list(src), list(rx_id), list(ry_id), dict(oth_id)
    g2c = {s: k for k, s in enumerate(src)}
    steps, n_prunes = [], 0
    for lo in range(lo0, K, sync):
        hi = min(K, lo + sync)
        if len(src) + hi - lo > cap:   # the sync would not fit: prune first
            f = o.get_frame()
            ev = f["events"]
            sub = remap_frame(cur, f)
            # the two conditions the oracle alone must meet
            assert (sub.sp != UNKNOWN).all() and (sub.op != UNKNOWN).all()
            assert len(ev) + sync <= cap, (len(ev), sync, cap)
            first = {}
            for g in ev:
                first.setdefault(int(cur.creator[g]), g)
            others = {}
            for g, op in f["others"].items():
                others[src[g]] = src[op] if op >= 0 else oth_id[src[g]]
            for p, (x, y, _, _) in enumerate(f["roots"]):
                if x >= 0:
                    rx_id[p] = src[x]
                if y >= 0:
                    ry_id[p] = src[y]
                elif y == -1:
                    ry_id[p] = None
                elif y == ROOT_OTHER:
                    ry_id[p] = oth_id[src[first[p]]]
            oth_id = others
            roots = hgref.frame_root_arrays(f)
            o.reset(*roots)
            o.insert_trace(sub)
            rc, msg = o.run_consensus()
            assert not rc, msg
            src = [src[g] for g in ev]
            g2c = {s: k for k, s in enumerate(src)}
            cur = sub
            n_prunes += 1
            steps.append(dict(kind="prune", events=ev, roots=f["roots"], root_arrays=roots, sub=sub,
                              known=o.known().copy(), src=list(src), rx=list(rx_id), ry=list(ry_id),
                              others=dict(oth_id), next_lo=lo))
        sel = np.arange(lo, hi)
        for k in range(lo, hi):
            g2c[k] = len(src)
            src.append(k)
        sp = [g2c[int(x)] if x >= 0 else -1 for x in t.sp[sel]]
        op = [g2c.get(int(x), UNKNOWN) if x >= 0 else -1 for x in t.op[sel]]
        part = _sub(t, sel, sp, op)
        assert (part.op != UNKNOWN).all()
        o.insert_trace(part)
        rc, msg = o.run_consensus()
        assert not rc, msg
        cur = _concat(cur, part)
        steps.append(dict(kind="insert", part=part, sel=sel))
    return dict(steps=steps, oracle=o, resident=cur, n_prunes=n_prunes)


@functools.lru_cache(maxsize=None)
def oracle_run(n):
    _, _, _, sync, cap, _ = SHAPES[n]
    return long_run(chain_of(n), sync, cap)


def cols_of(c, sel, sp, op, r=None, s=None):
    """hgx_event_bodies columns of the chain's events `sel` with the given parents (r, s: other
    signature columns than the chain's)."""
    sel = np.asarray(sel, np.int64)
    return body_columns(c.t.creator[sel], c.t.index[sel], sp, op, c.t.ts[sel], (c.r if r is None else r)[sel],
                        (c.t.s if s is None else s)[sel], [c.txs[int(i)] for i in sel])


def hid(c, g):
    return None if g is None else c.ids[g].tobytes()


def root_ids_of(c, x):
    """SetRootIds arguments / GetRootIds and GetRootOthers answers of a prune step."""
    return ([hid(c, g) for g in x["rx"]], [hid(c, g) for g in x["ry"]],
            sorted((hid(c, k), hid(c, v)) for k, v in x["others"].items()))


def check_root_ids(h, c, x):
    xs, ys, oth = root_ids_of(c, x)
    for p in range(c.n):
        assert h.GetRootIds(p) == dict(X=xs[p], Y=ys[p]), p
    assert h.GetRootOthers() == oth


_OPEN = []   # the contexts a test made


@pytest.fixture(autouse=True)
def _close_contexts():
    """No context outlives its test: each holds a HIP stream, and with few hardware queues a stream
    left open changes how later tests' streams share them (the chain-sharded rehearsal needs its two
    launches co-scheduled)."""
    yield
    while _OPEN:
        _OPEN.pop().close()


def _hg(c, cap, n_graphs=1):
    h = Hashgraph(c.n if c is not None else 4, capacity=cap, n_graphs=n_graphs)
    _OPEN.append(h)
    if c is not None:
        h.set_participant_keys(c.keys)
    return h


def replay(h, c, steps, on_prune=None):
    """The GPU side of long_run: every sync through insert_bodies, every returned id against the
    chain, every prune against the oracle's frame."""
    for x in steps:
        if x["kind"] == "insert":
            part, sel = x["part"], x["sel"]
            ids = h.insert_bodies(cols_of(c, sel, part.sp, part.op))
            assert np.array_equal(ids, c.ids[sel]), int(sel[0])
            h.RunConsensus()
            continue
        old = h.PruneToFrame()
        assert list(old) == x["events"]
        for p in range(c.n):
            r = h.GetRoot(p)
            assert (r["X"], r["Y"], r["Index"], r["Round"]) == \
                (-1, -1 if x["roots"][p][1] == -1 else ROOT_Y, x["roots"][p][2], x["roots"][p][3]), p
        assert list(h.Known()) == list(x["known"])
        assert h.num_events() == len(old)
        if on_prune:
            on_prune(h, x)
        h.RunConsensus()


# ----------------------------------------------------------------------------- 1: sync, prune, sync
@functools.lru_cache(maxsize=None)
def pruned_run(n):
    """The whole run of a shape on one context (computed once; the context is closed at the end):
    every id and every prune checked on the way, the final state against the oracle's. Returns what
    the context reported as its root ids at every prune."""
    c, run = chain_of(n), oracle_run(n)
    seen = []
    h = Hashgraph(n, capacity=SHAPES[n][4])
    try:
        h.set_participant_keys(c.keys)
        replay(h, c, run["steps"],
               on_prune=lambda h, x: seen.append(([h.GetRootIds(p) for p in range(n)], h.GetRootOthers())))
        assert h.num_events() == run["resident"].E
        compare(h, run["oracle"], run["resident"], hashes=False)
    finally:
        h.close()
    return seen


@pytest.mark.parametrize("n", [4, 16])
def test_sync_prune_sync_through_the_body_path(n):
    """Every sync through insert_bodies, PruneToFrame before each sync that would not fit: every id
    equals the chain's and the final state is the oracle's. Without the feature the first sync after
    the first prune is refused ("not after hgx_reset")."""
    run = oracle_run(n)
    assert run["n_prunes"] >= 3
    assert len(pruned_run(n)) == run["n_prunes"]


# ----------------------------------------------------------------------------- 2: Root.X with an id
def _hand_made():
    """Four creators; the caller's roots cut the DAG after g4: creator 0's Root.X is g3, creator 2's
    Root.X is g2 and its Root.Y g4, creator 1's Root.X is g4, creator 3 has a genesis root."""
    creator = [0, 1, 2, 0, 1, 2, 0, 3, 1]
    sp = [-1, -1, -1, 0, 1, 2, 3, -1, 4]
    op = [-1, -1, -1, 1, 3, 4, 5, -1, 7]
    txs = [[b"a"], [], None, [b"bc", b""], [], [b"d"], None, [b"e"], []]
    return bodyref.manual(4, creator, sp, op, txs)


def test_first_event_on_a_root_x_with_an_id():
    c = _hand_made()
    h = _hg(c, 16)
    h.Reset([1, 1, 0, -1], [0, 0, 0, -1], [0, 0, 1, 0])
    x = [hid(c, 3), hid(c, 4), hid(c, 2), None]
    y = [None, None, hid(c, 4), None]
    h.SetRootIds(x, y, [])
    for p in range(4):
        assert h.GetRootIds(p) == dict(X=x[p], Y=y[p])
    # g5: self-parent Root.X (g2), other-parent Root.Y (g4); g6: self-parent Root.X (g3), other-parent
    # g5; g7: a genesis root's "" next to the table; g8: Root.X (g4) and g7
    sel = [5, 6, 7, 8]
    ids = h.insert_bodies(cols_of(c, sel, [-1, -1, -1, -1], [ROOT_Y, 0, -1, 2]))
    assert np.array_equal(ids, c.ids[sel])
    for k, g in enumerate(sel):
        assert h.event_id(k) == hid(c, g)
    assert bodyref.hex_id(hid(c, 3)).encode() in c.json[6] and b'"Parents":["",""]' in c.json[7]
    # the same events without the table's ids hash to something else: the ids above came from the table
    h2 = _hg(c, 16)
    h2.Reset([1, 1, 0, -1], [0, 0, 0, -1], [0, 0, 1, 0])
    h2.SetRootIds([None] * 4, [None, None, hid(c, 4), None], [])
    with pytest.raises(HgxError) as ei:
        h2.insert_bodies(cols_of(c, sel, [-1, -1, -1, -1], [ROOT_Y, 0, -1, 2]))
    assert ei.value.msg == "Invalid signature" and ei.value.inserted == 0


# ----------------------------------------------------------------------------- 3: fast-forward join
def _join_step(n):
    """The first prune of the shape's run whose frame holds an Others entry and a ROOT_Y event."""
    run = oracle_run(n)
    prunes = [x for x in run["steps"] if x["kind"] == "prune"]
    j = next(j for j, x in enumerate(prunes) if (x["sub"].op == ROOT_OTHER).any() and (x["sub"].op == ROOT_Y).any())
    return j, prunes[j]


def _frame_inputs(c, x, flip=None):
    """The frame of prune step x as insert_bodies arguments: columns with the codes, and the ids of
    the HGX_ROOT_OTHER other-parents (flip: that position's id with one bit altered)."""
    sub = x["sub"]
    opi = np.zeros((sub.E, 32), np.uint8)
    for k in np.nonzero(sub.op == ROOT_OTHER)[0]:
        opi[k] = c.ids[x["others"][x["src"][k]]]
    if flip is not None:
        opi[flip, 7] ^= 0x10
    return cols_of(c, x["src"], sub.sp, sub.op), opi


def _joined(c, x, cap):
    """A fresh context after Reset(frame roots) and SetRootIds(ids from the chain)."""
    h = _hg(c, cap)
    h.Reset(*x["root_arrays"])
    h.SetRootIds(*root_ids_of(c, x))
    return h


@functools.lru_cache(maxsize=None)
def joined_oracle_run(n):
    """A fresh oracle joining at the step of _join_step, then the rest of the trace."""
    c = chain_of(n)
    _, x = _join_step(n)
    o = hgref.Oracle(n)
    o.reset(*x["root_arrays"])
    o.insert_trace(x["sub"])
    rc, msg = o.run_consensus()
    assert not rc, msg
    _, _, _, sync, cap, _ = SHAPES[n]
    return long_run(c, sync, cap, start=(o, x["sub"], x["src"], x["rx"], x["ry"], x["others"], x["next_lo"]))


def test_fast_forward_join():
    n = 16
    c = chain_of(n)
    j, x = _join_step(n)
    sub = x["sub"]
    assert (sub.op == ROOT_OTHER).sum() >= 1 and (sub.op == ROOT_Y).sum() >= 1 and len(x["others"]) >= 1
    h = _joined(c, x, SHAPES[n][4])
    cols, opi = _frame_inputs(c, x)
    ids = h.insert_bodies(cols, other_parent_ids=opi)
    assert np.array_equal(ids, c.ids[x["src"]])
    # the root ids are what the context that pruned its way here reports
    seen = pruned_run(n)
    assert ([h.GetRootIds(p) for p in range(n)], h.GetRootOthers()) == seen[j]
    check_root_ids(h, c, x)
    h.RunConsensus()
    run = joined_oracle_run(n)
    assert run["n_prunes"] >= 1
    replay(h, c, run["steps"], on_prune=lambda h, y: check_root_ids(h, c, y))
    assert h.num_events() == run["resident"].E
    compare(h, run["oracle"], run["resident"], hashes=False)


# ----------------------------------------------------------------------------- 4: the value check
def _signed_with_other_parent(c, g, op_id):
    """(r, s) of the chain's event g signed over another other-parent id (its creator's key)."""
    import hashlib
    t = c.t
    sp = int(t.sp[g])
    bj = bodyref.body_json(c.txs[g], hid(c, sp) if sp >= 0 else None, op_id, bytes(c.keys[t.creator[g]]), int(t.ts[g]),
                           int(t.index[g]))
    d = np.frombuffer(hashlib.sha256(bj).digest(), np.uint8)
    _, r, s = hgref.sign_batch(c.n, [int(t.creator[g])], d[None, :])
    return r[0], s[0]


@pytest.mark.parametrize("how", ["bit", "entry", "none"])
def test_others_value_check(how):
    """CheckOtherParent's error at an Others event's position, the prefix resident:
      bit    its supplied other-parent id differs from the roots' entry by one bit. The id is part of
             the event's text, so the event is signed over the altered id (with the chain's signature
             Event.Verify fails first, here as in the reference: test_invalid_signature_comes_first);
      entry  the roots' entry for it differs from the supplied id by one bit (the event, its text and
             its id are the chain's: the key is found, the value is not equal);
      none   the batch comes without the column."""
    n = 16
    c = chain_of(n)
    _, x = _join_step(n)
    others = np.nonzero(x["sub"].op == ROOT_OTHER)[0]
    k0 = int(others[0]) if how == "none" else int(others[len(others) // 2])
    g0 = x["src"][k0]
    cols, opi = _frame_inputs(c, x, flip=k0 if how == "bit" else None)
    if how == "bit":
        r, s = c.r.copy(), c.t.s.copy()
        r[g0], s[g0] = _signed_with_other_parent(c, g0, opi[k0].tobytes())
        cols = cols_of(c, x["src"], x["sub"].sp, x["sub"].op, r=r, s=s)
    if how == "entry":
        h = _hg(c, SHAPES[n][4])
        h.Reset(*x["root_arrays"])
        xs, ys, oth = root_ids_of(c, x)
        bad = bytes([opi[k0, 0] ^ 1]) + opi[k0, 1:].tobytes()
        h.SetRootIds(xs, ys, [(k, bad if k == hid(c, g0) else v) for k, v in oth])
        assert dict(h.GetRootOthers())[hid(c, g0)] == bad
    else:
        h = _joined(c, x, SHAPES[n][4])
    with pytest.raises(HgxError) as ei:
        h.insert_bodies(cols, other_parent_ids=None if how == "none" else opi)
    assert (ei.value.code, ei.value.msg) == (101, "CheckOtherParent: Other-parent not known")
    assert ei.value.inserted == k0 and h.num_events() == k0
    assert np.array_equal(ei.value.ids, c.ids[x["src"][:k0]])
    if k0:
        assert h.event_id(k0 - 1) == hid(c, x["src"][k0 - 1])
    if how != "entry":   # the caller resends the tail as the chain has it
        cols, good = _frame_inputs(c, x)
        tail = h.insert_bodies(cols, k0, x["sub"].E, other_parent_ids=good)
        assert np.array_equal(tail, c.ids[x["src"][k0:]])


# ----------------------------------------------------------------------------- 5: order of errors
def test_invalid_signature_comes_first():
    n = 4
    c, run = chain_of(n), oracle_run(n)
    h = _hg(c, SHAPES[n][4])
    # replay up to the first sync after the first prune
    steps = run["steps"]
    first = next(i for i, x in enumerate(steps) if x["kind"] == "prune") + 1
    assert steps[first]["kind"] == "insert"
    replay(h, c, steps[:first])
    part, sel = steps[first]["part"], steps[first]["sel"]
    e0 = h.num_events()
    r = c.r.copy()
    r[sel[0], 9] ^= 4
    with pytest.raises(HgxError) as ei:
        h.insert_bodies(cols_of(c, sel, part.sp, part.op, r=r))
    assert (ei.value.code, ei.value.msg, ei.value.inserted) == (104, "Invalid signature", 0) and h.num_events() == e0
    assert np.array_equal(h.insert_bodies(cols_of(c, sel, part.sp, part.op)), c.ids[sel])
    # an Others event with a bad signature and a bad entry: Verify comes first (hashgraph.go:356-363)
    c16 = chain_of(16)
    _, x = _join_step(16)
    k0 = int(np.nonzero(x["sub"].op == ROOT_OTHER)[0][0])
    r = c16.r.copy()
    r[x["src"][k0], 9] ^= 4
    cols, opi = _frame_inputs(c16, x, flip=k0)
    cols = cols_of(c16, x["src"], x["sub"].sp, x["sub"].op, r=r)
    h = _joined(c16, x, SHAPES[16][4])
    with pytest.raises(HgxError) as ei:
        h.insert_bodies(cols, other_parent_ids=opi)
    assert (ei.value.msg, ei.value.inserted) == ("Invalid signature", k0)


# ----------------------------------------------------------------------------- 6: refusals
def _ids_unknown(h):
    for call in (lambda: h.GetRootIds(0), h.GetRootOthers):
        with pytest.raises(HgxError) as ei:
            call()
        assert ei.value.msg == "root ids not known"


def test_refusals_and_set_root_ids_argument_errors():
    n = 16
    c = chain_of(n)
    _, x = _join_step(n)
    xs, ys, oth = root_ids_of(c, x)
    cols, opi = _frame_inputs(c, x)
    h = _hg(c, SHAPES[n][4])
    h.Reset(*x["root_arrays"])
    with pytest.raises(HgxError) as ei:
        h.insert_bodies(cols, other_parent_ids=opi)
    assert ei.value.code == 102 and "hgx_reset" in ei.value.msg and ei.value.inserted == 0
    assert h.num_events() == 0 and [h.GetRoot(p)["Index"] for p in range(n)] == [r[2] for r in x["roots"]]
    _ids_unknown(h)

    def refused(x_, y_, o_, word):
        with pytest.raises(HgxError) as ei:
            h.SetRootIds(x_, y_, o_)
        assert ei.value.code == 102 and word in ei.value.msg, ei.value.msg
        _ids_unknown(h)

    p = next(p for p in range(n) if ys[p] is not None)
    refused(xs, [None if q == p else v for q, v in enumerate(ys)], oth, "has_y")
    q = next(q for q in range(n) if ys[q] is None) if any(v is None for v in ys) else None
    if q is not None:
        refused(xs, [xs[0] if r == q else v for r, v in enumerate(ys)], oth, "has_y")
    refused(xs, ys, oth + [(oth[0][0], oth[-1][1])], "twice")
    # events resident: one event through the plain insert, then the ids come too late
    k = next(k for k in range(x["sub"].E) if x["sub"].op[k] in (-1, ROOT_Y))
    assert k == 0
    h.insert_trace(x["sub"], 0, 1)
    refused(xs, ys, oth, "resident")
    assert h.num_events() == 1
    # a batch context has no roots
    hb = _hg(None, 64, n_graphs=2)
    with pytest.raises(HgxError) as ei:
        hb.SetRootIds([None] * 8, [None] * 8, [])
    assert ei.value.code == 102


# ----------------------------------------------------------------------------- 7: a further prune
def test_a_further_prune_carries_the_installed_ids():
    """Join at the first prune of the n = 4 run, sync on through the next prunes: the ids the caller
    installed are carried like the ones a prune gathered."""
    n = 4
    c, run = chain_of(n), oracle_run(n)
    _, _, _, sync, cap, _ = SHAPES[n]
    x = next(s for s in run["steps"] if s["kind"] == "prune")
    o = hgref.Oracle(n)
    o.reset(*x["root_arrays"])
    o.insert_trace(x["sub"])
    rc, msg = o.run_consensus()
    assert not rc, msg
    rest = long_run(c, sync, cap, start=(o, x["sub"], x["src"], x["rx"], x["ry"], x["others"], x["next_lo"]))
    assert rest["n_prunes"] >= 2
    h = _joined(c, x, cap)
    cols, opi = _frame_inputs(c, x)
    assert np.array_equal(h.insert_bodies(cols, other_parent_ids=opi), c.ids[x["src"]])
    h.RunConsensus()
    seen = []
    replay(h, c, rest["steps"], on_prune=lambda h, y: (check_root_ids(h, c, y), seen.append(len(y["others"]))))
    assert len(seen) == rest["n_prunes"]
    compare(h, rest["oracle"], rest["resident"], hashes=False)
