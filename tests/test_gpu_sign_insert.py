"""hgx_sign_insert_event_bodies / hgx_set_signing_keys on the device: Event.Sign, the
text, the id and the verified insert of a batch in one call. The expected R, S and ids are those of
tests/signref.py's chain (pure Python, RFC 6979 nonces), bit for bit."""
import os

import numpy as np
import pytest

import hgref
import signref
from babble_amd import trace as gtrace
from babble_amd._lib import HgxError
from babble_amd.hashgraph import Hashgraph, body_columns
from hgref import ROOT_OTHER, ROOT_Y
from p256ref import N
from test_sign_ref import ref_check

pytestmark = pytest.mark.gpu

INVALID = 102
SIGN_BLOCK = 64   # lanes per workgroup of the signing kernels (hgx_kernels.h kSignBlock)
_OPEN = []


@pytest.fixture(autouse=True)
def _close_contexts():
    yield
    while _OPEN:
        _OPEN.pop().close()


def _hg(c, cap=None, n=None, n_graphs=1, sign=True, keep=False):
    h = Hashgraph(n or c.n, capacity=cap or c.t.E, n_graphs=n_graphs)
    _OPEN.append(h)
    if keep:
        h.KeepBodies(0, 0)
    h.set_participant_keys(c.keys)
    if sign:
        h.set_signing_keys(signref.priv_bytes(len(c.keys)))
    return h


def unsigned(c, lo=0, hi=None, **repl):
    """body_columns of the chain's events [lo, hi) without signatures."""
    hi = c.t.E if hi is None else hi
    a = dict(creator=c.t.creator[lo:hi], index=c.t.index[lo:hi], sp=c.t.sp[lo:hi], op=c.t.op[lo:hi], ts=c.t.ts[lo:hi],
             r=None, s=None, txs=c.txs[lo:hi])
    a.update(repl)
    return body_columns(**a)


def _same(got, c, lo=0, hi=None):
    r, s, ids, k = got
    hi = c.t.E if hi is None else hi
    assert k == hi - lo
    for name, a, b in (("r", r, c.r[lo:hi]), ("s", s, c.t.s[lo:hi]), ("id", ids, c.ids[lo:hi])):
        bad = np.nonzero((a != b).any(axis=1))[0]
        assert len(bad) == 0, (name, bad[:8] + lo)


def _same_consensus(h, t):
    a, b = h.results(), hgref.oracle_run(t).results()
    for k in ("round", "witness", "famous", "rr", "cts"):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    assert list(a["order"]) == list(b["order"])


# ----------------------------------------------------------------------------- chains
@pytest.mark.parametrize("n,E,seed", [(4, 200, 1), (2, 150, 3), (16, 300, 2)])
def test_chain_signed_in_one_call(n, E, seed):
    c = signref.chain(n, E, seed)
    h = _hg(c)
    got = h.sign_insert_event_bodies(unsigned(c))
    _same(got, c)
    assert h.num_events() == E and h.event_id(E - 1) == bytes(c.ids[E - 1])
    h.RunConsensus()
    _same_consensus(h, c.t)
    # anyone's verified insert accepts the returned columns, with the same ids
    h2 = _hg(c, sign=False)
    assert np.array_equal(h2.insert_bodies(c.columns(r=got[0], s=got[1])), got[2])


def test_store_parents_and_one_event_per_call():
    c = signref.chain(4, 200, 1)
    h = _hg(c)
    _same(h.sign_insert_event_bodies(unsigned(c, 0, 80)), c, 0, 80)
    _same(h.sign_insert_event_bodies(unsigned(c, 80, 190)), c, 80, 190)   # parents' ids from the store
    for k in range(190, 200):   # Core.SignAndInsertSelfEvent's shape
        _same(h.sign_insert_event_bodies(unsigned(c, k, k + 1)), c, k, k + 1)
    assert h.num_events() == 200
    h.RunConsensus()
    _same_consensus(h, c.t)


def test_manual_dag_transaction_shapes():
    """nil, empty and multi-transaction events; g5 and g6 have both parents in the batch."""
    creator = [0, 1, 2, 0, 1, 2, 0, 3, 1]
    sp = [-1, -1, -1, 0, 1, 2, 3, -1, 4]
    op = [-1, -1, -1, 1, 3, 4, 5, -1, 7]
    txs = [[b"a"], [], None, [b"bc", b""], [], [b"d" * 1000, b"e", b"fgh"], None, [b"e"], []]
    c = signref.manual(4, creator, sp, op, txs)
    assert b'"Transactions":null' in c.json[2] and b'"Transactions":[]' in c.json[1]
    h = _hg(c, cap=16)
    _same(h.sign_insert_event_bodies(unsigned(c)), c)


def test_batched_context():
    """3 graphs x 4 participants, interleaved: each graph's chain equals the single-graph result."""
    a = gtrace.gossip(4, 90, 5)
    n, G = 4, 3
    E = G * a.E
    creator = np.empty(E, np.int32)
    sp, op = np.empty(E, np.int64), np.empty(E, np.int64)
    for g in range(G):
        creator[g::G] = a.creator + g * n
        sp[g::G] = np.where(a.sp >= 0, G * a.sp + g, -1)
        op[g::G] = np.where(a.op >= 0, G * a.op + g, -1)
    txs = [[b"tx %d" % (k // G)] if (k // G) % 3 else [] for k in range(E)]
    c = signref.manual(G * n, creator, sp, op, txs)
    h = _hg(c, cap=E, n=n, n_graphs=G)
    _same(h.sign_insert_event_bodies(unsigned(c)), c)
    # graph 0 alone on a single-graph context (same keys 0..3, same events): the same chain
    one = signref.manual(n, a.creator, a.sp, a.op, txs[0::G])
    h1 = _hg(one, cap=a.E)
    r, s, ids, _ = h1.sign_insert_event_bodies(body_columns(one.t.creator, one.t.index, one.t.sp, one.t.op,
                                                            c.t.ts[0::G], None, None, one.txs))
    assert np.array_equal(ids, c.ids[0::G]) and np.array_equal(r, c.r[0::G]) and np.array_equal(s, c.t.s[0::G])


def test_level_wider_than_a_workgroup(tmp_path):
    """SIGN_BLOCK + 76 first events in one level: the workgroup strides over it."""
    E = SIGN_BLOCK + 76
    none = np.full(E, -1, np.int64)
    c = signref.manual(E, np.arange(E), none, none, [[b"w%d" % k] for k in range(E)])
    assert c.level.max() == 0
    h = _hg(c, cap=E)
    r, s, ids, k = h.sign_insert_event_bodies(unsigned(c))
    assert k == E == h.num_events()
    ref_check([(bytes(c.keys[i]), bytes(c.dig[i]), bytes(r[i]), bytes(s[i])) for i in range(E)], tmp_path)
    for i in range(E):   # (every position: the first and last of the level, and both sides of lane 64)
        assert (bytes(r[i]), bytes(s[i]), bytes(ids[i])) == (bytes(c.r[i]), bytes(c.t.s[i]), bytes(c.ids[i])), i


def test_chunk_boundary():
    """40 first events of 1 MiB of text each fill more than one internal chunk; the events of the second
    chunk name parents in the first."""
    big = bytes(range(256)) * (3 << 10)
    creator = list(range(40)) + list(range(10))
    sp = [-1] * 40 + list(range(10))
    op = [-1] * 40 + [(k + 7) % 40 for k in range(9)] + [48]
    txs = [[big[k:]] for k in range(40)] + [[b"a"], None, [], [b"bc", b""]] * 2 + [[b"d"], []]
    c = signref.manual(64, creator, sp, op, txs)
    assert sum(map(len, c.json[:32])) > 32 << 20
    h = _hg(c)
    _same(h.sign_insert_event_bodies(unsigned(c)), c)


# ----------------------------------------------------------------------------- rooted context
def test_rooted_context_root_x_and_root_other():
    """A node signs its way to a prune; a second context joins at that frame (Reset, SetRootIds with the
    ids the pruned context reports) and signs the frame's events again: self-parent -1 prints Root.X,
    HGX_ROOT_Y prints Root.Y, HGX_ROOT_OTHER the supplied id. The nonces are deterministic, so the ids
    are the chain's."""
    import test_gpu_bodies_rooted as tr
    K, sync, cap = 600, 100, 400
    t = gtrace.gossip(4, 6000, 85)
    cut = gtrace.GossipTrace(4, **{k: getattr(t, k)[:K].copy() for k in
                                   ("creator", "index", "sp", "op", "ts", "hash", "s", "ntx", "txnil", "tx_seq")})
    c = signref.build(cut, [cut.txs(i) for i in range(K)])
    run = tr.long_run(c, sync, cap)
    A = _hg(c, cap=cap)
    x = None
    for st in run["steps"]:
        if st["kind"] == "insert":
            part, sel = st["part"], st["sel"]
            got = A.sign_insert_event_bodies(body_columns(part.creator, part.index, part.sp, part.op, part.ts, None, None,
                                                          [c.txs[int(i)] for i in sel]))
            assert np.array_equal(got[2], c.ids[sel]) and np.array_equal(got[0], c.r[sel])
            A.RunConsensus()
        elif x is None:
            assert list(A.PruneToFrame()) == st["events"]
            A.RunConsensus()
            x = st
            xs, ys, oth = tr.root_ids_of(c, x)
            assert [A.GetRootIds(p) for p in range(4)] == [dict(X=xs[p], Y=ys[p]) for p in range(4)]
            sub = x["sub"]
            assert (sub.op == ROOT_OTHER).any() and any(v is not None for v in xs) and (sub.sp == -1).any()
            B = _hg(c, cap=cap)
            B.Reset(*x["root_arrays"])
            B.SetRootIds(xs, ys, oth)
            src = np.asarray(x["src"], np.int64)
            opi = np.zeros((sub.E, 32), np.uint8)
            for k in np.nonzero(sub.op == ROOT_OTHER)[0]:
                opi[k] = c.ids[x["others"][x["src"][k]]]
            got = B.sign_insert_event_bodies(body_columns(sub.creator, sub.index, sub.sp, sub.op, sub.ts, None, None,
                                                          [c.txs[int(i)] for i in src]), opi)
            assert got[3] == sub.E
            assert np.array_equal(got[2], c.ids[src]) and np.array_equal(got[0], c.r[src]) and \
                np.array_equal(got[1], c.t.s[src])
        else:
            break
    assert x is not None


# ----------------------------------------------------------------------------- body store
def test_body_store_keeps_the_devices_r():
    c = signref.chain(4, 200, 1)
    A = _hg(c, keep=True)
    r, s, ids, _ = A.sign_insert_event_bodies(unsigned(c))
    got = A.EventBodies(np.arange(200))
    assert np.array_equal(got["sig_r"], r) and np.array_equal(r, c.r)
    rows, count, over = A.DiffWireBodies(np.full(4, -1, np.int32))
    assert count == 200 and not over and np.array_equal(rows["sig_s"], s)
    resp = dict(creator_id=rows["creator_id"], index=rows["index"], self_parent_index=rows["self_parent_index"],
                other_parent_creator=rows["other_parent_creator"], other_parent_index=rows["other_parent_index"],
                timestamp_ns=rows["timestamp_ns"], sig_r=rows["sig_r"], sig_s=rows["sig_s"],
                ntx=np.where(rows["tx_nil"] != 0, -1, rows["ntx"]).astype(np.int32), tx_off=rows["tx_off"],
                tx_bytes=np.concatenate([rows["tx_bytes"], np.zeros(1, np.uint8)]))
    B = _hg(c, sign=False)
    ids2, _, _ = B.insert_wire_bodies(resp)
    assert np.array_equal(ids2, c.ids[rows["gid"]]) and B.num_events() == 200


# ----------------------------------------------------------------------------- failures and refusals
def test_failure_parity_wrong_self_parent():
    c = signref.chain(4, 200, 1)
    t = c.t
    k0 = 120
    j = next(g for g in range(k0 - 1, -1, -1) if t.creator[g] != t.creator[k0])
    sp = t.sp.copy()
    sp[k0] = j
    op0 = int(t.op[k0])
    rb, sb, _, _, _ = signref.event(c.txs[k0], bytes(c.ids[j]), bytes(c.ids[op0]) if op0 >= 0 else None,
                                    signref.priv(int(t.creator[k0])), int(t.ts[k0]), int(t.index[k0]))
    r, s = c.r.copy(), t.s.copy()
    r[k0], s[k0] = np.frombuffer(rb, np.uint8), np.frombuffer(sb, np.uint8)
    ref = _hg(c, sign=False)
    with pytest.raises(HgxError) as want:
        ref.insert_bodies(c.columns(sp=sp, r=r, s=s))
    h = _hg(c)
    with pytest.raises(HgxError) as ei:
        h.sign_insert_event_bodies(unsigned(c, sp=sp))
    assert (ei.value.code, ei.value.msg, ei.value.inserted) == (want.value.code, want.value.msg, want.value.inserted)
    assert ei.value.msg == "CheckSelfParent: Self-parent not last known event by creator" and ei.value.inserted == k0
    assert h.num_events() == ref.num_events() == k0
    assert np.array_equal(ei.value.ids, c.ids[:k0]) and np.array_equal(ei.value.r, c.r[:k0]) and \
        np.array_equal(ei.value.s, t.s[:k0])


def test_refusals_and_key_clearing():
    c = signref.chain(4, 200, 1)
    cols = unsigned(c)

    def refused(h, why, cols=cols, fn="hgx_sign_insert_event_bodies: "):
        before = h.num_events()
        with pytest.raises(HgxError) as ei:
            h.sign_insert_event_bodies(cols)
        assert ei.value.code == INVALID and ei.value.msg.startswith(fn) and why in ei.value.msg, ei.value.msg
        assert h.num_events() == before

    h = _hg(c, sign=False)
    refused(h, "signing keys not set")
    d = signref.priv_bytes(4)
    # a creator without a signing key
    part = d.copy()
    part[2] = 0
    h.set_signing_keys(part)
    refused(h, "creator 2 has no signing key")
    only2 = np.nonzero(c.t.creator[:4] != 2)[0]   # (its other events are signed: the first events of 0, 1, 3)
    k = h.sign_insert_event_bodies(body_columns(c.t.creator[only2], c.t.index[only2], c.t.sp[only2], c.t.op[only2],
                                                c.t.ts[only2], None, None, [c.txs[int(i)] for i in only2]))[3]
    assert k == len(only2) == h.num_events()
    # a key that does not match the participant's, and d >= N: nothing changes (creator 2 still has none)
    swapped = d.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    for bad, why in ((swapped, "hgx_set_signing_keys: key 0 does not match participant 0's public key"), ):
        with pytest.raises(HgxError) as ei:
            h.set_signing_keys(bad)
        assert (ei.value.code, ei.value.msg) == (INVALID, why)
    for v in (N, N + 5, 2 ** 256 - 1):
        big = d.copy()
        big[3] = np.frombuffer(v.to_bytes(32, "big"), np.uint8)
        with pytest.raises(HgxError) as ei:
            h.set_signing_keys(big)
        assert ei.value.code == INVALID and "key 3 is not below N" in ei.value.msg
    refused(h, "creator 2 has no signing key")
    # bad columns come first, even without keys
    h3 = _hg(c, sign=False)
    bad_cols = dict(cols, ntx=np.full(200, -2, np.int32))
    refused(h3, "ntx below -1", bad_cols)
    h3.set_signing_keys(d)
    refused(h3, "ntx below -1", bad_cols)
    # key clearing
    _same(h3.sign_insert_event_bodies(unsigned(c, 0, 50)), c, 0, 50)
    h3.set_signing_keys(None)
    refused(h3, "signing keys not set", unsigned(c, 50, 200))
    h3.set_signing_keys(d)
    _same(h3.sign_insert_event_bodies(unsigned(c, 50, 200)), c, 50, 200)
    # no participant keys: the signing keys are refused, and so is the call
    h4 = Hashgraph(4, capacity=200)
    _OPEN.append(h4)
    with pytest.raises(HgxError) as ei:
        h4.set_signing_keys(d)
    assert ei.value.code == INVALID and "participant keys not set" in ei.value.msg
    refused(h4, "participant keys not set")
    # a chain-sharded context
    hs = Hashgraph(4, capacity=256, shard_devices=[0, 0])
    _OPEN.append(hs)
    refused(hs, "chain-sharded")


def test_checkpoint_holds_no_private_key(tmp_path):
    c = signref.chain(4, 200, 1)
    h = _hg(c, keep=True)
    h.sign_insert_event_bodies(unsigned(c))
    h.RunConsensus()
    path = os.path.join(str(tmp_path), "ck.hgx")
    h.save(path)
    with open(path, "rb") as f:
        blob = f.read()
    assert len(blob) > 200 * 32
    assert bytes(c.ids[7]) in blob          # (the search finds what is there)
    for k in range(4):
        assert signref.priv(k).to_bytes(32, "big") not in blob
