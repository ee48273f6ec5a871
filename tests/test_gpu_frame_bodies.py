"""hgx_get_frame_bodies: Hashgraph.GetFrame served complete from the device, the
frame's roots, ids, parents as ids and bodies in one call that changes nothing.
  1. signed chains with bodies kept: at every prune of a long run the frame just before PruneToFrame
     (a) and, on the now rooted context, just after the prune and RunConsensus (b);
  2. a fast-forward between two contexts from served data alone, by positions and codes (A) and by
     ids and flags (B);
  3. structure only: more than one scan chunk, silent chains, no bodies;
  4. capacities (all or nothing) and refusals.

Every expected value comes from hgref.Oracle and the bodyref chain over the unpruned trace, never from
the library: an id is the SHA-256 of the event's Go-JSON with its real parents' ids, whatever the
store still holds."""
import functools

import numpy as np
import pytest

import hgref
from babble_amd import _lib
from babble_amd import trace as gtrace
from babble_amd._lib import HgxError
from babble_amd.hashgraph import Hashgraph, body_columns, compact_columns
from hgref import ROOT_OTHER, ROOT_Y, UNKNOWN
from test_gpu_bodies_rooted import (SHAPES, _OPEN, _close_contexts, _hg, _join_step, chain_of, cols_of,  # noqa: F401
                                    joined_oracle_run, long_run, replay)
from test_gpu_parity import compare
from test_gpu_prune import COLS, LONG, _concat, _sub, oracle_long_run, remap_frame

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------- the oracle's side
def frame_info(o, cur, src, rx_id, ry_id, oth_id):
    """The oracle's frame at this moment, with everything a served frame must say, and nothing of the
    caller's state changed. cur: the resident trace (parents as resident gids or stored codes), src:
    its events' trace gids, rx_id / ry_id / oth_id: the current roots' ids as trace gids (None: "")."""
    f = o.get_frame()
    ev = f["events"]
    sub = remap_frame(cur, f)
    first = {}
    for g in ev:
        first.setdefault(int(cur.creator[g]), g)
    others = {src[g]: (src[op] if op >= 0 else oth_id[src[g]]) for g, op in f["others"].items()}
    rx, ry = list(rx_id), list(ry_id)
    for p, (x, y, _, _) in enumerate(f["roots"]):
        if x >= 0:
            rx[p] = src[x]
        if y >= 0:
            ry[p] = src[y]
        elif y == -1:
            ry[p] = None
        elif y == ROOT_OTHER:
            ry[p] = oth_id[src[first[p]]]
    stored = dict(other=sum(int(cur.op[g]) == ROOT_OTHER for g in ev), y=sum(int(cur.op[g]) == ROOT_Y for g in ev),
                  x=sum(int(cur.sp[g]) == -1 and rx_id[int(cur.creator[g])] is not None for g in ev))
    return dict(events=ev, roots=f["roots"], root_arrays=hgref.frame_root_arrays(f), sub=sub, src=[src[g] for g in ev],
                rx=rx, ry=ry, others=others, stored=stored)


@functools.lru_cache(maxsize=None)
def frame_run(n):
    """test_gpu_bodies_rooted.long_run with the oracle's frame recorded twice at every prune: (a) the
    frame the prune keeps, (b) the frame of the oracle that went Reset + re-insert + consensus."""
    _, _, _, sync, cap, K = SHAPES[n]
    t = chain_of(n).t
    o, cur, src, rx, ry, oth = hgref.Oracle(n), None, [], [None] * n, [None] * n, {}
    g2c, steps = {}, []
    for lo in range(0, K, sync):
        hi = min(K, lo + sync)
        if len(src) + hi - lo > cap:
            a = frame_info(o, cur, src, rx, ry, oth)
            assert len(a["events"]) + sync <= cap
            o.reset(*a["root_arrays"])
            o.insert_trace(a["sub"])
            rc, msg = o.run_consensus()
            assert not rc, msg
            cur, src, rx, ry, oth = a["sub"], list(a["src"]), a["rx"], a["ry"], a["others"]
            g2c = {s: k for k, s in enumerate(src)}
            b = frame_info(o, cur, src, rx, ry, oth)
            steps.append(dict(kind="prune", a=a, b=b, known=o.known().copy(), next_lo=lo))
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
    return dict(steps=steps, oracle=o, resident=cur)


def _prunes(n):
    return [x for x in frame_run(n)["steps"] if x["kind"] == "prune"]


# ----------------------------------------------------------------------------- the checks
def _parent_ids(ids, par):
    """Body.Parents of events with trace parents `par` (-1: "") as (rows, present)."""
    par = np.asarray(par, np.int64)
    rows = np.zeros((len(par), 32), np.uint8)
    rows[par >= 0] = ids[par[par >= 0]]
    return rows, par >= 0


def check_structure(fb, info, t, ids):
    """Every column but the bodies' of a served frame against the oracle's frame `info`, the unpruned
    trace t and its events' ids."""
    src = np.asarray(info["src"], np.int64)
    sub = info["sub"]
    assert (sub.sp != UNKNOWN).all() and (sub.op != UNKNOWN).all()
    assert list(fb["gid"]) == info["events"]
    assert np.array_equal(fb["creator"], t.creator[src]) and np.array_equal(fb["index"], t.index[src])
    assert np.array_equal(fb["timestamp_ns"], t.ts[src])
    assert np.array_equal(fb["ntx"], np.where(t.txnil[src] != 0, -1, t.ntx[src]))
    assert np.array_equal(fb["id32"], ids[src]) and np.array_equal(fb["sig_s"], t.s[src])
    assert np.array_equal(fb["self_parent"], sub.sp) and np.array_equal(fb["other_parent"], sub.op)
    sp_rows, has_sp = _parent_ids(ids, t.sp[src])
    op_rows, has_op = _parent_ids(ids, t.op[src])
    assert np.array_equal(fb["parent_flags"], has_sp.astype(np.uint8) | (has_op.astype(np.uint8) << 1))
    assert np.array_equal(fb["self_parent_id32"], sp_rows) and np.array_equal(fb["other_parent_id32"], op_rows)
    rid = lambda g: None if g is None else ids[g].tobytes()
    for p, r in enumerate(info["roots"]):
        assert fb["roots"][p] == dict(Index=r[2], Round=r[3], X=rid(info["rx"][p]), Y=rid(info["ry"][p])), p
    assert fb["others"] == sorted((rid(k), rid(v)) for k, v in info["others"].items())


def check_bodies(fb, info, c):
    src = info["src"]
    assert np.array_equal(fb["sig_r"], c.r[np.asarray(src, np.int64)])
    flat = [b for g in src if c.txs[g] for b in c.txs[g]]
    assert list(fb["tx_off"]) == list(np.cumsum([0] + [len(b) for b in flat]))
    assert fb["tx_bytes"].tobytes() == b"".join(flat)


def served_txs(fb):
    """Body.Transactions of every served event, from ntx / tx_off / tx_bytes."""
    out, k = [], 0
    by = fb["tx_bytes"].tobytes()
    for m in fb["ntx"]:
        if m < 0:
            out.append(None)
            continue
        out.append([by[int(fb["tx_off"][k + j]):int(fb["tx_off"][k + j + 1])] for j in range(int(m))])
        k += int(m)
    return out


def served_columns(fb):
    return body_columns(fb["creator"], fb["index"], fb["self_parent"], fb["other_parent"], fb["timestamp_ns"],
                        fb["sig_r"], fb["sig_s"], served_txs(fb))


def served_roots(fb):
    """Reset and SetRootIds arguments from a served frame."""
    r = fb["roots"]
    return ([x["Index"] for x in r], [x["Round"] for x in r], [0 if x["Y"] is None else 1 for x in r]), \
        ([x["X"] for x in r], [x["Y"] for x in r], fb["others"])


def _keeping(c, cap):
    h = _hg(c, cap)
    h.KeepBodies()
    return h


def _sync(h, c, x):
    ids = h.insert_bodies(cols_of(c, x["sel"], x["part"].sp, x["part"].op))
    assert np.array_equal(ids, c.ids[x["sel"]])
    h.RunConsensus()


# ----------------------------------------------------------------------------- 1: signed chains
def test_the_oracle_runs_exercise_every_source():
    """Conditions on the oracle's data alone, so that test 1 cannot pass vacuously."""
    p16, p4 = _prunes(16), _prunes(4)
    assert len(p16) == 4 and len(p4) == 6
    for x in p16:
        b, a = x["b"], x["a"]
        assert b["stored"]["other"] >= 1 and b["stored"]["y"] >= 1 and b["stored"]["x"] >= 1, b["stored"]
        assert len(a["others"]) >= 1 and (a["sub"].op == ROOT_Y).sum() >= 1
    assert sum(x["b"]["stored"]["other"] >= 1 for x in p4) >= 3
    for x in p16 + p4:
        for f in (x["a"], x["b"]):
            assert (f["sub"].sp != UNKNOWN).all() and (f["sub"].op != UNKNOWN).all()
        assert x["a"]["stored"]["other"] == 0 and x["a"]["stored"]["y"] == 0   # (that is why (b) is required)


@pytest.mark.parametrize("n", [4, 16])
def test_frames_of_a_pruning_run_with_bodies(n):
    c, run = chain_of(n), frame_run(n)
    h = _keeping(c, SHAPES[n][4])
    for x in run["steps"]:
        if x["kind"] == "insert":
            _sync(h, c, x)
            continue
        fa = h.GetFrameBodies()
        check_structure(fa, x["a"], c.t, c.ids)
        check_bodies(fa, x["a"], c)
        old = h.PruneToFrame()
        assert np.array_equal(old, fa["gid"])
        assert [h.GetRootIds(p) for p in range(n)] == [dict(X=r["X"], Y=r["Y"]) for r in fa["roots"]]
        assert h.GetRootOthers() == fa["others"]
        assert list(h.Known()) == list(x["known"])
        h.RunConsensus()
        fb = h.GetFrameBodies()
        check_structure(fb, x["b"], c.t, c.ids)
        check_bodies(fb, x["b"], c)
    assert h.num_events() == run["resident"].E
    compare(h, run["oracle"], run["resident"], hashes=False)   # the call changed nothing on the way


# ----------------------------------------------------------------------------- 2: fast-forward
def _served(n, j):
    """A serving context run up to prune j of the shape: its frames (a) and (b) there."""
    c = chain_of(n)
    h = _keeping(c, SHAPES[n][4])
    seen = 0
    for x in frame_run(n)["steps"]:
        if x["kind"] == "insert":
            _sync(h, c, x)
            continue
        if seen < j:
            h.PruneToFrame()
            h.RunConsensus()
            seen += 1
            continue
        fa = h.GetFrameBodies()
        h.PruneToFrame()
        h.RunConsensus()
        return fa, h.GetFrameBodies(), x


def test_fast_forward_from_served_data_alone():
    n = 16
    c = chain_of(n)
    cap = SHAPES[n][4]
    j, xj = _join_step(n)
    fa, fb, x = _served(n, j)
    assert x["a"]["events"] == xj["events"] and x["next_lo"] == xj["next_lo"]
    # A: positions and codes, the served other-parent ids at the HGX_ROOT_OTHER rows
    reset_a, ids_a = served_roots(fa)
    others = np.nonzero(fa["other_parent"] == ROOT_OTHER)[0]
    assert len(others) >= 1
    opi = np.zeros_like(fa["other_parent_id32"])
    opi[others] = fa["other_parent_id32"][others]
    A = _keeping(c, cap)
    A.Reset(*reset_a)
    A.SetRootIds(*ids_a)
    assert A.insert_bodies_claimed(served_columns(fa), fa["id32"], opi) == len(fa["gid"])
    A.RunConsensus()
    run = joined_oracle_run(n)
    replay(A, c, run["steps"])
    assert A.num_events() == run["resident"].E
    compare(A, run["oracle"], run["resident"], hashes=False)
    # one bit of one served other-parent id of an Others event: the insert fails at that event
    k0 = int(others[len(others) // 2])
    bad = opi.copy()
    bad[k0, 7] ^= 0x10
    A2 = _keeping(c, cap)
    A2.Reset(*reset_a)
    A2.SetRootIds(*ids_a)
    with pytest.raises(HgxError) as ei:
        A2.insert_bodies_claimed(served_columns(fa), fa["id32"], bad)
    assert ei.value.inserted == k0 and A2.num_events() == k0
    # B: ids and flags, from the frame the rooted context served
    b = x["b"]
    assert b["stored"]["other"] >= 1 and b["stored"]["y"] >= 1 and b["stored"]["x"] >= 1
    reset_b, ids_b = served_roots(fb)
    B = _keeping(c, cap)
    B.KeepIdIndex()
    B.Reset(*reset_b)
    B.SetRootIds(*ids_b)
    m, sp, op = B.insert_events_by_id(served_columns(fb), fb["id32"], fb["self_parent_id32"], fb["other_parent_id32"],
                                      fb["parent_flags"])
    assert m == len(fb["gid"])
    assert np.array_equal(sp, fb["self_parent"]) and np.array_equal(op, fb["other_parent"])
    B.RunConsensus()
    o = hgref.Oracle(n)
    o.reset(*b["root_arrays"])
    o.insert_trace(b["sub"])
    rc, msg = o.run_consensus()
    assert not rc, msg
    rest = long_run(c, SHAPES[n][3], cap, start=(o, b["sub"], b["src"], b["rx"], b["ry"], b["others"], x["next_lo"]))
    assert rest["n_prunes"] >= 1
    replay(B, c, rest["steps"])
    assert B.num_events() == rest["resident"].E
    compare(B, rest["oracle"], rest["resident"], hashes=False)


# ----------------------------------------------------------------------------- 3: structure only
def test_structure_only_beyond_one_scan_chunk_with_silent_chains():
    shape = LONG[5]
    n, E, seed, sync, cap, n_silent = shape
    assert (n, n_silent, cap) == (64, 8, 8000)
    run = oracle_long_run(*shape)
    t = run["t"]
    assert run["n_prunes"] == 4
    h = Hashgraph(n, capacity=cap)
    _OPEN.append(h)
    cur, src, nxt, seen = None, [], 0, 0
    for kind, x in run["steps"]:
        if kind == "insert":
            h.insert_trace(x)
            h.RunConsensus()
            src += list(range(nxt, nxt + x.E))   # (the syncs take the trace in order)
            nxt += x.E
            cur = _concat(cur, x)
            continue
        # the oracle's frame in resident gids, from the recorded step: an event is an Others key iff
        # the oracle recorded its trace gid as one
        ev = x["events"]
        frame = dict(events=ev, roots=x["roots"], others={g: int(cur.op[g]) for g in ev if src[g] in x["others"]})
        info = dict(events=ev, roots=x["roots"], sub=remap_frame(cur, frame), src=x["src"], rx=x["rx"], ry=x["ry"],
                    others=x["others"])
        assert [src[g] for g in ev] == x["src"] and len(frame["others"]) == x["n_others"]
        if seen == 0:
            assert len(ev) > 2048 and len(src) > 6144 and x["n_others"] >= 1, (len(ev), len(src))
        silent = [p for p in range(n) if not (t.creator == p).any()]
        assert len(silent) == n_silent
        before = h.num_events()
        fb = h.GetFrameBodies(bodies=False)
        check_structure(fb, info, t, np.asarray(t.hash, np.uint8).reshape(-1, 32))
        for p in silent:
            assert fb["roots"][p] == dict(Index=-1, Round=-1, X=None, Y=None)
        # a body column on a context that keeps none: refused, nothing written
        r = np.full((len(ev), 32), 0xA5, np.uint8)
        g = np.full(len(ev), -77, np.int64)
        rc, err, cnt = h.get_frame_bodies_raw(dict(sig_r=r, gid=g), events_cap=len(ev))
        assert (rc, err.msg) == (102, b"hgx_get_frame_bodies: bodies not known") and cnt == (0, 0, 0, 0)
        assert (r == 0xA5).all() and (g == -77).all() and h.num_events() == before
        old = h.PruneToFrame()
        assert np.array_equal(old, fb["gid"])
        h.RunConsensus()
        cur, src, seen = info["sub"], list(x["src"]), seen + 1
    assert seen == 4
    compare(h, run["oracle"], run["resident"], hashes=False)


# ----------------------------------------------------------------------------- 4: capacities, refusals
SENT = 0xA5


def _sentinel_arrays(C_, ne, no, nt, nb):
    spec = dict(_lib.FRAME_OUT_FIELDS)
    rows = {nm: C_ for nm in _lib.FRAME_ROOT_COLUMNS}
    rows.update({nm: no for nm in _lib.FRAME_OTHERS_COLUMNS})
    rows.update({nm: ne for nm in _lib.FRAME_EVENT_COLUMNS})
    rows.update(tx_off=nt + 1, tx_bytes=nb)
    arr = {}
    for nm, m in rows.items():
        a = np.zeros((max(1, m),) + spec[nm][1], spec[nm][0])
        a.view(np.uint8)[...] = SENT
        arr[nm] = a
    return arr


def _untouched(arr):
    return all((a.view(np.uint8) == SENT).all() for a in arr.values())


def test_capacities_and_refusals():
    n, K = 4, 300
    c = chain_of(n)
    t = c.t
    o = hgref.Oracle(n)
    o.insert_trace(t, 0, K)
    rc, msg = o.run_consensus()
    assert not rc, msg
    sel = np.arange(K)
    h = _keeping(c, 1000)
    # before any DivideRounds: hgx_get_frame's text
    h.insert_bodies(cols_of(c, sel, t.sp[sel], t.op[sel]))
    rc, err, cnt = h.get_frame_bodies_raw({})
    assert (rc, err.code, err.msg, cnt) == (1, 1, b"0, Not Found", (0, 0, 0, 0))
    h.RunConsensus()
    info = frame_info(o, _sub(t, sel, t.sp[sel], t.op[sel]), list(range(K)), [None] * n, [None] * n, {})
    # the sizing call: the totals, nothing touched (a body column makes the body totals count)
    rc, err, cnt0 = h.get_frame_bodies_raw({})
    assert rc == 103 and cnt0[0] == len(info["events"]) and cnt0[1] == len(info["others"]) and cnt0[2:] == (0, 0)
    probe = np.full((1, 32), SENT, np.uint8)
    rc, err, cnt = h.get_frame_bodies_raw(dict(sig_r=probe))
    ne, no, nt, nb = cnt
    flat = [b for g in info["src"] if c.txs[g] for b in c.txs[g]]
    assert rc == 103 and (ne, no) == cnt0[:2] and nt == len(flat) >= 1 and nb == sum(len(b) for b in flat) >= 1
    assert no >= 1 and (probe == SENT).all()
    # each capacity one short in turn: the totals, the sentinels intact
    for short in range(4):
        caps = [ne, no, nt, nb]
        caps[short] -= 1
        arr = _sentinel_arrays(n, ne, no, nt, nb)
        rc, err, got = h.get_frame_bodies_raw(arr, *caps)
        assert rc == 103 and err.code == 103 and got == cnt and _untouched(arr), short
    # exact capacities fill; capacities + 5 leave the tail rows untouched
    spec = dict(_lib.FRAME_OUT_FIELDS)
    exact = _sentinel_arrays(n, ne, no, nt, nb)
    rc, err, got = h.get_frame_bodies_raw(exact, ne, no, nt, nb)
    assert rc == 0 and got == cnt
    wide = _sentinel_arrays(n, ne + 5, no + 5, nt + 5, nb + 5)
    rc, err, got = h.get_frame_bodies_raw(wide, ne + 5, no + 5, nt + 5, nb + 5)
    assert rc == 0 and got == cnt
    used = {nm: ne for nm in _lib.FRAME_EVENT_COLUMNS}
    used.update({nm: no for nm in _lib.FRAME_OTHERS_COLUMNS})
    used.update({nm: n for nm in _lib.FRAME_ROOT_COLUMNS})
    used.update(tx_off=nt + 1, tx_bytes=nb)
    for nm, m in used.items():
        assert np.array_equal(wide[nm][:m], exact[nm][:m]), nm
        assert (wide[nm][m:].view(np.uint8) == SENT).all(), nm
    fb = h.GetFrameBodies()
    for nm in _lib.FRAME_EVENT_COLUMNS + ("tx_off", "tx_bytes"):
        assert np.array_equal(fb[nm], exact[nm][:used[nm]]), nm
    check_structure(fb, info, t, c.ids)
    check_bodies(fb, info, c)

    def refused(hh, word, arrays=None):
        e0 = hh.num_events()
        arr = _sentinel_arrays(hh.n * hh.G, 8, 8, 8, 8) if arrays is None else arrays
        rc, err, got = hh.get_frame_bodies_raw(arr, 8, 8, 8, 8)
        assert rc == 102 and err.msg.startswith(b"hgx_get_frame_bodies: ") and word in err.msg, err.msg
        assert got == (0, 0, 0, 0) and _untouched(arr) and hh.num_events() == e0

    # between hgx_find_order_begin and _end
    part = np.arange(K, K + 100)
    h.insert_bodies(cols_of(c, part, t.sp[part], t.op[part]))
    h.DivideRounds()
    h.DecideFame()
    h._call(h.L.hgx_find_order_begin)
    refused(h, b"FindOrder")
    h._call(h.L.hgx_find_order_end)
    # ... and afterwards the context takes a sync and agrees with the oracle
    K1, K2 = K + 100, K + 200
    nxt = np.arange(K1, K2)
    h.insert_bodies(cols_of(c, nxt, t.sp[nxt], t.op[nxt]))
    h.RunConsensus()
    for lo in (K, K1):
        o.insert_trace(t, lo, lo + 100)
        rc, msg = o.run_consensus()
        assert not rc, msg
    compare(h, o, _sub(t, np.arange(K2), t.sp[:K2], t.op[:K2]), hashes=False)
    # the oracle of the next two contexts: K events, consensus, a sync of 100, consensus
    o2 = hgref.Oracle(n)
    for lo, hi in ((0, K), (K, K1)):
        o2.insert_trace(t, lo, hi)
        rc, msg = o2.run_consensus()
        assert not rc, msg
    tk, tk1 = _sub(t, sel, t.sp[sel], t.op[sel]), _sub(t, np.arange(K1), t.sp[:K1], t.op[:K1])
    # a batch context: refused, then a sync into both graphs; each graph agrees with the oracle
    G = 2
    hb = _hg(None, G * K1, n_graphs=G)
    hb.insert_trace(gtrace.concat_graphs([tk] * G))
    hb.RunConsensus()
    refused(hb, b"single-graph")
    part = np.arange(K, K1)
    gid_of = lambda g, x: np.where(x < 0, x, np.where(x < K, x + g * K, G * K + g * 100 + (x - K)))   # trace gid -> batch gid
    for g in range(G):
        sync = _sub(t, part, gid_of(g, t.sp[part]), gid_of(g, t.op[part]))
        sync = type(sync)(n, **{k: getattr(sync, k) + (g * n if k == "creator" else 0) for k in COLS})
        hb.insert_trace(sync)
    hb.RunConsensus()
    want = o2.results()
    for g in range(G):
        back = {int(gid_of(g, np.int64(x))): x for x in range(K1)}
        assert [back[int(x)] for x in hb.ConsensusEvents(g)] == list(want["order"]), g
        assert hb.UndecidedRounds(g) == want["undecided"] and hb.LastConsensusRound(g) == want["lcr"]
        assert hb.ConsensusTransactions(g) == want["consensus_tx"]
        assert [(b["rr"], b["ntx"], b["tx_nil"]) for b in hb.Blocks(g)] == [(b[0], b[1], b[2]) for b in want["blocks"]]
    # events without their ids: refused, then a sync
    hc = _hg(None, K1)
    hc.insert_and_run32(compact_columns(tk))
    refused(hc, b"ids not known")
    hc.insert_and_run32(compact_columns(_sub(t, part, t.sp[part], t.op[part])))
    compare(hc, o2, tk1, hashes=False)
    # the caller's own Reset with roots, before SetRootIds; with them the served frame joins
    reset_args, ids_args = served_roots(fb)
    assert any(r >= 0 for r in reset_args[1])
    hr = _keeping(c, 1000)
    hr.Reset(*reset_args)
    refused(hr, b"root ids not known")
    hr.SetRootIds(*ids_args)
    opi = fb["other_parent_id32"]
    assert hr.insert_bodies_claimed(served_columns(fb), fb["id32"], opi) == ne
    hr.RunConsensus()
    oj = hgref.Oracle(n)
    oj.reset(*info["root_arrays"])
    oj.insert_trace(info["sub"])
    rc, msg = oj.run_consensus()
    assert not rc, msg
    compare(hr, oj, info["sub"], hashes=False)
