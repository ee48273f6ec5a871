"""hgx_prune_to_frame: the resident hashgraph cut down to its last frame on the device
(GetFrame -> Reset(frame.Roots) -> re-insert of frame.Events, hashgraph.go:879-1002, in one call
with no event crossing PCIe), against the oracle doing the same by hand:
  * a node that keeps running past several times its capacity, pruning whenever the next sync
    would not fit (rooted contexts pruned again, silent chains whose root is carried over);
  * the same state as the host route (GetFrame / Reset / insert) on a second context;
  * the ids of the new roots (hgx_get_root_ids / hgx_get_root_others) over two prunes;
  * refusals that leave the context untouched;
  * payloads and checkpoints of a pruned context.

The scan behind the renumbering works in chunks of 2 048 events (kScanChunk, hgx_kernels.hip): the
shapes cover a resident set under one chunk and one above three chunks with a remainder."""
import functools

import numpy as np
import pytest

import hgref
from babble_amd import trace as gtrace
from hgref import ROOT_OTHER, ROOT_Y, UNKNOWN
from test_gpu_parity import compare

pytestmark = pytest.mark.gpu

COLS = ("creator", "index", "sp", "op", "ts", "hash", "s", "ntx", "txnil", "tx_seq")


def _hg(n, cap):
    from babble_amd.hashgraph import Hashgraph
    return Hashgraph(n, capacity=cap)


def _sub(t, sel, sp, op):
    """Events `sel` of trace t with the given parents, as a trace of their own."""
    sel = np.asarray(sel, np.int64)
    cols = {k: getattr(t, k)[sel] for k in COLS if k not in ("sp", "op") and hasattr(t, k)}
    cols["sp"], cols["op"] = np.asarray(sp, np.int64), np.asarray(op, np.int64)
    if hasattr(t, "tx_seq"):
        return type(t)(t.n, **cols)
    return hgref.Trace(n=t.n, txs=[t.txs[int(x)] for x in sel], names=[t.names[int(x)] for x in sel] if t.names else [],
                       **cols)


def remap_frame(cur, frame):
    """The frame's events (gids of the resident trace `cur`, whose parents may already be the codes
    of a rooted context) as the trace to insert after Reset(frame roots), parents resolved like
    InsertEvent (hashgraph.go:404-445): kept -> new gid; the self-parent equal to Root.X -> -1; an
    other-parent equal to Root.Y of an event whose self-parent is Root.X -> ROOT_Y; else the
    event's Root.Others entry -> ROOT_OTHER; anything else UNKNOWN. (Root.Y is tested only for the
    creator's first event: a later event whose outside other-parent happens to equal Root.Y is an
    Others entry.)"""
    new = {g: k for k, g in enumerate(frame["events"])}
    sp_new, op_new = [], []
    for g in frame["events"]:
        rx, ry = frame["roots"][int(cur.creator[g])][:2]
        sp, op = int(cur.sp[g]), int(cur.op[g])
        sp_new.append(new[sp] if sp in new else (-1 if sp == rx else UNKNOWN))
        if op == -1:
            op_new.append(-1)
        elif op in new:
            op_new.append(new[op])
        elif op == ry and sp == rx:
            op_new.append(ROOT_Y)
        elif frame["others"].get(g) == op:
            op_new.append(ROOT_OTHER)
        else:
            op_new.append(UNKNOWN)
    return _sub(cur, frame["events"], sp_new, op_new)


def _concat(a, b):
    if a is None:
        return b
    return type(a)(a.n, **{k: np.concatenate([getattr(a, k), getattr(b, k)]) for k in COLS})


@functools.lru_cache(maxsize=None)
def oracle_long_run(n, E, seed, sync, cap, n_silent, max_prunes=None):
    """The oracle's side of a long run, computed once per shape: the list of steps (("insert", part)
    with the part's parents in resident gids, ("prune", info)) and the final results. Root ids are
    tracked as trace gids (None = "")."""
    t = gtrace.gossip(n, E, seed, n_silent=n_silent)
    o = hgref.Oracle(n)
    cur, src, g2c = None, [], {}
    rx_id, ry_id, oth_id = [None] * n, [None] * n, {}
    steps, n_prunes = [], 0
    for lo in range(0, E, sync):
        hi = min(E, lo + sync)
        if len(src) + hi - lo > cap:   # the sync would not fit: prune first
            if max_prunes is not None and n_prunes == max_prunes:
                break
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
            o.reset(*hgref.frame_root_arrays(f))
            o.insert_trace(sub)
            rc, msg = o.run_consensus()
            assert not rc, msg
            src = [src[g] for g in ev]
            g2c = {s: k for k, s in enumerate(src)}
            cur = sub
            n_prunes += 1
            steps.append(("prune", dict(events=ev, roots=f["roots"], known=o.known().copy(), src=list(src),
                                        rx=list(rx_id), ry=list(ry_id), others=dict(oth_id),
                                        n_others=len(f["others"]))))
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
        steps.append(("insert", part))
    return dict(t=t, steps=steps, oracle=o, resident=cur, n_prunes=n_prunes)


def replay(run, cap, on_prune=None):
    """The GPU side of oracle_long_run: the same steps on a context of `cap` events, every prune
    checked against the oracle's frame."""
    t = run["t"]
    h = _hg(t.n, cap)
    for kind, x in run["steps"]:
        if kind == "insert":
            h.insert_trace(x)
            h.RunConsensus()
            continue
        old = h.PruneToFrame()
        assert list(old) == x["events"]
        for p in range(t.n):
            r = h.GetRoot(p)
            assert (r["X"], r["Y"], r["Index"], r["Round"]) == \
                (-1, -1 if x["roots"][p][1] == -1 else ROOT_Y, x["roots"][p][2], x["roots"][p][3]), p
        assert list(h.Known()) == list(x["known"])
        assert h.num_events() == len(old)
        for k in range(len(old)):
            assert h.event_id(k) == t.hash[x["src"][k]].tobytes(), k
        if on_prune:
            on_prune(h, x)
        h.RunConsensus()
    return h


LONG = [(4, 6000, 81, 100, 1000, 0), (4, 6000, 82, 100, 1000, 1), (4, 6000, 85, 100, 400, 0),
        (16, 12000, 83, 400, 3000, 0), (16, 12000, 86, 200, 1000, 0), (64, 30000, 84, 1000, 8000, 8)]


@pytest.mark.parametrize("n,E,seed,sync,cap,n_silent", LONG)
def test_long_run_past_capacity(n, E, seed, sync, cap, n_silent):
    """A context of `cap` events takes E = 3.75 to 15 times cap events, pruning before every sync
    that would not fit (4 to 19 prunes); every prune and the final state match the oracle doing
    GetFrame / Reset / re-insert. Without hgx_prune_to_frame the context answers "context capacity
    exceeded" at the first sync that does not fit."""
    run = oracle_long_run(n, E, seed, sync, cap, n_silent)
    assert run["n_prunes"] >= 4
    h = replay(run, cap)
    assert h.num_events() == run["resident"].E
    compare(h, run["oracle"], run["resident"], hashes=False)


def _results_equal(a, b):
    for k in ("round", "witness", "famous", "rr", "cts", "order"):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    for k in ("last_round", "undecided", "lcr", "lcre", "consensus_tx", "pending_loaded", "blocks"):
        assert a[k] == b[k], k


def _same_getters(a, b, n):
    _results_equal(a.results(), b.results())
    assert a.num_events() == b.num_events() and list(a.Known()) == list(b.Known())
    for p in range(n):
        assert a.GetRoot(p) == b.GetRoot(p)
        assert a.LastFrom(p) == b.LastFrom(p)
    for g in sorted({0, a.num_events() // 2, a.num_events() - 1}):
        assert a.GetEvent(g) == b.GetEvent(g) and a.event_id(g) == b.event_id(g)


def _prune_both(t, chunks, nxt=None):
    """Context A pruned on the device, context B through GetFrame / Reset / insert, the oracle
    likewise; returns (A, B, oracle, the frame trace, the frame). nxt: a trace event not inserted
    yet whose self-parent is in the frame, for the Root.Others refusal."""
    from babble_amd._lib import HgxError
    A, B, o = _hg(t.n, t.E + 8), _hg(t.n, t.E + 8), hgref.Oracle(t.n)
    for lo, hi in chunks:
        for x in (A, B, o):
            x.insert_trace(t, lo, hi)
        A.RunConsensus()
        B.RunConsensus()
        o.run_consensus()
    f = o.get_frame()
    assert B.GetFrame() == f
    sub = remap_frame(t, f)
    assert (sub.sp != UNKNOWN).all() and (sub.op != UNKNOWN).all()
    assert list(A.PruneToFrame()) == f["events"]
    roots = hgref.frame_root_arrays(f)
    B.Reset(*roots, others=hgref.frame_others_keys(t, f))
    B.insert_trace(sub)
    o.reset(*roots)
    o.insert_trace(sub)
    _same_getters(A, B, t.n)
    # an event that claims a Root.Others parent without being a key is refused alike
    if nxt is None:
        return A, B, o, sub, f
    bogus = _sub(t, [nxt], [f["events"].index(int(t.sp[nxt]))], [ROOT_OTHER])
    msgs = []
    for x in (A, B):
        e0 = x.num_events()
        with pytest.raises(HgxError) as ei:
            x.insert_trace(bogus)
        msgs.append((ei.value.code, ei.value.msg))
        assert x.num_events() == e0
    assert msgs[0] == msgs[1] == (101, "CheckOtherParent: Other-parent not known")
    return A, B, o, sub, f


def test_same_state_as_the_host_route_gossip():
    n, E, K = 16, 6000, 3000
    t = gtrace.gossip(n, E, 72)
    A, B, o, sub, f = _prune_both(t, [(0, K // 2), (K // 2, K)], nxt=K)
    for x in (A, B, o):
        x.run_consensus() if x is o else x.RunConsensus()
    new = {g: k for k, g in enumerate(f["events"])}
    res = sub
    for lo in range(K, E, 1000):
        sel = np.arange(lo, min(E, lo + 1000))
        for g in sel:
            new[int(g)] = len(new)
        sp = [new[int(x)] for x in t.sp[sel]]
        op = [new.get(int(x), UNKNOWN) if x >= 0 else -1 for x in t.op[sel]]
        part = _sub(t, sel, sp, op)
        assert (part.op != UNKNOWN).all()
        for x in (A, B, o):
            x.insert_trace(part)
            x.run_consensus() if x is o else x.RunConsensus()
        res = _concat(res, part)
    _same_getters(A, B, n)
    compare(A, o, res, hashes=False)
    compare(B, o, res, hashes=False)
    assert o.results()["last_round"] > max(r[3] for r in f["roots"]) + 2


def test_events_without_a_round_yet_equal_the_host_route():
    """Events inserted after the last RunConsensus have no round yet; the frame takes them as the
    tails of their chains. The device route and the host route agree on that state too (the two
    contexts only: the oracle computes rounds on demand)."""
    n, E, K, U = 16, 6000, 3000, 300
    t = gtrace.gossip(n, E, 72)
    A, B = _hg(n, E), _hg(n, E)
    for x in (A, B):
        x.insert_trace(t, 0, K)
        x.RunConsensus()
        x.insert_trace(t, K, K + U)
    f = B.GetFrame()
    assert max(f["events"]) == K + U - 1
    sub = remap_frame(t, f)
    assert list(A.PruneToFrame()) == f["events"]
    B.Reset(*hgref.frame_root_arrays(f), others=hgref.frame_others_keys(t, f))
    B.insert_trace(sub)
    new = {g: k for k, g in enumerate(f["events"])}
    sel = np.arange(K + U, E)
    for g in sel:
        new[int(g)] = len(new)
    rest = _sub(t, sel, [new[int(x)] for x in t.sp[sel]], [new.get(int(x), UNKNOWN) if x >= 0 else -1 for x in t.op[sel]])
    assert (rest.op != UNKNOWN).all()
    for x in (A, B):
        x.RunConsensus()
        x.insert_trace(rest)
        x.RunConsensus()
    _same_getters(A, B, n)
    assert A.LastRound() > max(r[3] for r in f["roots"]) + 2


def test_same_state_as_the_host_route_fixture():
    t = hgref.fixture_trace("consensus_hashgraph")
    A, B, o, sub, f = _prune_both(t, [(0, t.E)])
    assert list(A.Known()) == [8, 7, 7]
    for x in (A, B, o):
        x.run_consensus() if x is o else x.RunConsensus()
    assert A.LastConsensusRound() == 1
    _same_getters(A, B, t.n)
    compare(A, o, sub, hashes=False)


def test_root_ids_over_two_prunes():
    """hgx_get_root_ids / hgx_get_root_others after the first and the second prune equal the trace
    hashes of the oracle frames' Root.X / Root.Y / Others (mapped to trace gids through the old_gid
    history); "" comes back as has = 0. After a plain Reset the ids are not known."""
    from babble_amd._lib import HgxError
    run = oracle_long_run(4, 6000, 81, 100, 1000, 0, max_prunes=2)
    t = run["t"]
    seen = []

    def check(h, x):
        hid = lambda g: None if g is None else t.hash[g].tobytes()
        for p in range(t.n):
            assert h.GetRootIds(p) == dict(X=hid(x["rx"][p]), Y=hid(x["ry"][p])), p
        want = sorted((hid(k), hid(v)) for k, v in x["others"].items())
        assert h.GetRootOthers() == want and len(want) == x["n_others"]
        seen.append((len(want), sum(v is None for v in x["rx"] + x["ry"])))

    h = replay(run, 1000, on_prune=check)
    assert len(seen) == 2 and seen[0][0] > 0 and seen[1][0] > 0
    fresh = _hg(t.n, 64)
    assert fresh.GetRootIds(0) == dict(X=None, Y=None) and fresh.GetRootOthers() == []
    f = h.GetFrame()
    h.Reset(*hgref.frame_root_arrays(f))
    for call in (lambda: h.GetRootIds(0), h.GetRootOthers):
        with pytest.raises(HgxError) as ei:
            call()
        assert ei.value.msg == "root ids not known"


def test_refusals_leave_the_context_untouched():
    from babble_amd._lib import HgxError
    from babble_amd.hashgraph import Hashgraph, compact_columns
    n, E = 4, 1024
    t = gtrace.gossip(n, E, 1)
    o = hgref.oracle_run(t)

    def refused(h, code_msg):
        e0, k0 = h.num_events(), list(h.Known())
        with pytest.raises(HgxError) as ei:
            h.PruneToFrame()
        assert code_msg(ei.value), (ei.value.code, ei.value.msg)
        assert h.num_events() == e0 and list(h.Known()) == k0

    # before any consensus: the text of GetFrame
    h = _hg(n, E)
    h.insert_trace(t)
    with pytest.raises(HgxError) as ei:
        h.GetFrame()
    assert ei.value.msg == "0, Not Found"
    refused(h, lambda e: e.msg == "0, Not Found" and e.code == 1)
    h.RunConsensus()
    compare(h, o, t, hashes=False)
    # a batch context
    hb = Hashgraph(n, capacity=2 * E, n_graphs=2)
    tb = gtrace.concat_graphs([t, t])
    hb.insert_trace(tb)
    hb.RunConsensus()
    before = hb.results(1)
    refused(hb, lambda e: e.code == 102)
    hb.RunConsensus()
    _results_equal(hb.results(1), before)
    # no ids
    hc = _hg(n, E)
    hc.insert_and_run32(compact_columns(t))
    refused(hc, lambda e: e.code == 102 and "ids" in e.msg)
    hc.RunConsensus()
    compare(hc, o, t, hashes=False)


def test_payloads_and_checkpoint_of_a_pruned_context(tmp_path):
    n, E = 16, 6000
    t = gtrace.gossip(n, E, 61, stale_prob=0.1, stale_depth=2)
    pay = [gtrace.payload(int(t.creator[i]), int(t.tx_seq[i])) if t.ntx[i] else b"" for i in range(E)]
    h = _hg(n, E)
    h.insert_trace(t)
    h.RunConsensus()
    p = str(tmp_path / "node.ckpt")
    h.save_with_payloads(p, pay)
    h2 = _hg(n, E)
    h2.Bootstrap(p)
    old = h2.PruneToFrame()
    assert 0 < len(old) < E and len(old) == h2.num_events()
    for k, g in enumerate(old):
        assert h2.event_payload(k) == pay[int(g)]
        if k % 64 == 0:
            assert h2.event_id(k) == t.hash[int(g)].tobytes()
    h2.RunConsensus()
    # a pruned context round-trips through the rooted checkpoint format
    p2 = str(tmp_path / "pruned.ckpt")
    h2.save(p2)
    h3 = _hg(n, E)
    h3.Bootstrap(p2)
    _results_equal(h3.results(), h2.results())
    assert list(h3.Known()) == list(h2.Known())
    for q in range(n):
        assert h3.GetRoot(q) == h2.GetRoot(q)
    p3 = str(tmp_path / "pruned2.ckpt")
    h3.save(p3)
    assert open(p3, "rb").read() == open(p2, "rb").read()
