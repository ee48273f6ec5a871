"""Events that arrive with their ids (hgx_insert_event_bodies_claimed): one flat hash pass
proves every claimed id instead of hashing level after level; and the checkpoint built on it: hgx_save_bodies
writes a version-3 file with the event bodies, hgx_bootstrap proves every id and signature in it and restores
the body store.

Expected values never come from the code under test: ids, R, S and the transactions are the
bodyref.Chain's (hashlib and the oracle's signer on the CPU), consensus results the CPU oracle's."""
import functools
import hashlib
import os

import numpy as np
import pytest

import bodyref
import hgref
import wireref
from babble_amd import checkpoint
from babble_amd._lib import HgxError
from babble_amd.hashgraph import Hashgraph
from test_gpu_bodies_kept import (_OPEN, _ListTrace, _chain_own, _check, _close_contexts, _counts,   # noqa: F401 (fixture)
                                  _expected, _hg)

pytestmark = pytest.mark.gpu

INVALID, SIGNATURE = 102, 104
KEYS = ("round", "witness", "famous", "rr", "cts", "order")


def _mismatch(k):
    return f"hgx_insert_event_bodies_claimed: event {k}: the claimed id is not the event's hash"


def _chain():
    """n = 4, E = 300 over the test's own lists (nil / [] / 1 / 3 transactions, every length of LENS)."""
    c = _chain_own(4, 300, 11)
    assert int(c.level.max()) + 1 > 50   # deep: the level path would run that many rounds
    return c


@functools.lru_cache(maxsize=None)
def _oracle_results():
    """The CPU oracle over the chain with its explicit transaction lists, one consensus run at the end."""
    c = _chain()
    o = hgref.Oracle(c.n)
    o.insert_trace(_ListTrace(c), 0, c.t.E)
    rc, msg = o.run_consensus()
    assert not rc, msg
    return o.results()


def _same_as_oracle(h):
    h.RunConsensus()
    got, want = h.results(), _oracle_results()
    for k in KEYS:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k


def _ids_are(h, ids, lo=0):
    for g in range(lo, lo + len(ids)):
        assert h.event_id(g) == ids[g - lo].tobytes(), g


# ---- 1. flat equals level ----------------------------------------------------------------------------
@pytest.mark.parametrize("cuts", [(0, 300), (0, 90, 200, 300)])
def test_flat_equals_level(cuts):
    """One call, and three calls: a later call's parents come from the store's id column, parents inside a
    call from the claimed column."""
    c = _chain()
    if len(cuts) > 2:   # the split has parents on both sides of a cut
        assert any(c.t.sp[k] < 90 or c.t.op[k] < 90 for k in range(90, 200))
        assert any(c.t.sp[k] >= 90 or c.t.op[k] >= 90 for k in range(91, 200))
    h, ref = _hg(c), _hg(c)
    for lo, hi in zip(cuts, cuts[1:]):
        assert h.insert_bodies_claimed(c.cols, c.ids, lo=lo, hi=hi) == hi - lo
        assert h.num_events() == hi
    _ids_are(h, c.ids)
    ref.insert_bodies(c.cols)
    assert h.BodiesState() == ref.BodiesState() == _counts(c, range(300))
    _check(h, np.arange(300), c)
    a, b = h.EventBodies(np.arange(300)), ref.EventBodies(np.arange(300))
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    _same_as_oracle(h)


def test_flat_on_a_batched_context():
    import dataclasses
    from babble_amd import trace as gtrace
    a, b = bodyref.chain(4, 200, 1), bodyref.chain(4, 200, 5)
    t = dataclasses.replace(gtrace.concat_graphs([a.t, b.t]), n=8)
    c = bodyref.build(t, a.txs + b.txs)
    h = Hashgraph(4, capacity=400, n_graphs=2)
    _OPEN.append(h)
    h.set_participant_keys(c.keys)
    h.KeepBodies(0, 0)
    assert h.insert_bodies_claimed(c.cols, c.ids) == 400
    _ids_are(h, c.ids)
    _check(h, np.arange(400)[::-1], c)
    ref = Hashgraph(4, capacity=400, n_graphs=2)
    _OPEN.append(ref)
    ref.set_participant_keys(c.keys)
    ref.insert_bodies(c.cols)
    h.RunConsensus()
    ref.RunConsensus()
    for g in range(2):
        assert np.array_equal(h.ConsensusEvents(g), ref.ConsensusEvents(g)) and len(h.Blocks(g)) >= 3
        assert h.Blocks(g) == ref.Blocks(g)


# ---- 2. a wrong claimed id ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 150, 299])
def test_wrong_claimed_id(k):
    c = _chain()
    if k == 150:   # an event whose descendants are in the same call
        assert (c.t.sp[151:] == 150).any() or (c.t.op[151:] == 150).any()
    ids = c.ids.copy()
    ids[k, 13] ^= 0x20
    h = _hg(c)
    with pytest.raises(HgxError) as ei:
        h.insert_bodies_claimed(c.cols, ids)
    assert (ei.value.code, ei.value.msg, ei.value.inserted) == (INVALID, _mismatch(k), k)
    assert h.num_events() == k
    _ids_are(h, c.ids[:k])
    assert h.BodiesState() == _counts(c, range(k))
    _check(h, np.arange(k), c)
    assert h.insert_bodies_claimed(c.cols, c.ids, lo=k) == 300 - k
    _ids_are(h, c.ids)
    _check(h, np.arange(300), c)
    _same_as_oracle(h)


# ---- 3. a tampered body under untouched ids ----------------------------------------------------------
def test_tampered_body_is_a_mismatch_not_a_signature_error():
    c = _chain()
    k = next(k for k in range(100, 300) if c.txs[k] and any(len(b) for b in c.txs[k]))
    txs = list(c.txs)
    j = next(j for j, b in enumerate(txs[k]) if len(b))
    b = bytearray(txs[k][j])
    b[len(b) // 2] ^= 1
    txs[k] = txs[k][:j] + [bytes(b)] + txs[k][j + 1:]
    h = _hg(c)
    with pytest.raises(HgxError) as ei:
        h.insert_bodies_claimed(c.columns(txs=txs), c.ids)
    assert (ei.value.code, ei.value.msg, ei.value.inserted) == (INVALID, _mismatch(k), k)
    assert h.num_events() == k


# ---- 4. an invalid signature under consistent ids ----------------------------------------------------
def _resigned_from(c, j):
    """The chain with event j signed under another participant's key and every later event rebuilt on the
    new ids with the oracle's encoder (and signed by its own creator): r, s, ids."""
    t = c.t
    r, s, ids = c.r.copy(), t.s.copy(), c.ids.copy()
    pid = lambda g: bytes(ids[g]) if g >= 0 else None
    for k in range(j, t.E):
        key = bytes(c.keys[t.creator[k]])
        bj = bodyref.body_json(c.txs[k], pid(t.sp[k]), pid(t.op[k]), key, int(t.ts[k]), int(t.index[k]))
        d = np.frombuffer(hashlib.sha256(bj).digest(), np.uint8)
        signer = (int(t.creator[k]) + 1) % c.n if k == j else int(t.creator[k])
        _, rk, sk = hgref.sign_batch(c.n, [signer], d[None, :])
        r[k], s[k] = rk[0], sk[0]
        js = hgref.go_event_json(c.txs[k], bodyref.hex_id(pid(t.sp[k])), bodyref.hex_id(pid(t.op[k])), key, int(t.ts[k]),
                                 int(t.index[k]), bytes(r[k]), bytes(s[k]))
        ids[k] = np.frombuffer(hashlib.sha256(js).digest(), np.uint8)
    return r, s, ids


def test_invalid_signature_under_consistent_ids():
    c = _chain()
    j, m = 120, 200
    r, s, ids = _resigned_from(c, j)
    assert not np.array_equal(ids[j], c.ids[j]) and np.array_equal(ids[:j], c.ids[:j])
    cols = c.columns(r=r, s=s)
    h = _hg(c)
    with pytest.raises(HgxError) as ei:
        h.insert_bodies_claimed(cols, ids)
    assert (ei.value.code, ei.value.msg, ei.value.inserted) == (SIGNATURE, "Invalid signature", j)
    assert h.num_events() == j
    _ids_are(h, c.ids[:j])
    # a wrong claimed id behind it in the same call: the proven prefix's own failure still comes first
    bad = ids.copy()
    bad[m, 0] ^= 1
    h2 = _hg(c)
    with pytest.raises(HgxError) as ei:
        h2.insert_bodies_claimed(cols, bad)
    assert (ei.value.code, ei.value.msg, ei.value.inserted) == (SIGNATURE, "Invalid signature", j)
    # at the same position the mismatch wins
    bad = ids.copy()
    bad[j, 0] ^= 1
    h3 = _hg(c)
    with pytest.raises(HgxError) as ei:
        h3.insert_bodies_claimed(cols, bad)
    assert (ei.value.code, ei.value.msg, ei.value.inserted) == (INVALID, _mismatch(j), j)


# ---- 5. the byte seam --------------------------------------------------------------------------------
def test_byte_seam():
    """test_chunk_seam's batch: two internal chunks (events 0..30 | 31..49); the ten small events' parents
    sit in the first chunk, which the second chunk reads from the store's id column."""
    big = bytes(range(256)) * (3 << 10)
    creator = list(range(40)) + list(range(10))
    sp = [-1] * 40 + list(range(10))
    op = [-1] * 40 + [(k + 7) % 40 for k in range(9)] + [48]
    txs = [[big[k:]] for k in range(40)] + [[b"a"], None, [], [b"bc", b""]] * 2 + [[b"d"], []]
    c = bodyref.manual(64, creator, sp, op, txs)
    assert sum(map(len, c.json[:32])) > 32 << 20 > sum(map(len, c.json[:31]))
    assert all(s < 31 for s in sp[40:]) and all(o < 31 for o in op[40:49]) and op[49] == 48
    h = _hg(c, keep=(0, 0))
    assert h.insert_bodies_claimed(c.cols, c.ids) == 50
    _ids_are(h, c.ids)
    assert h.BodiesState() == _counts(c, range(50))
    _check(h, np.arange(50)[::-1], c)
    # a wrong claimed id in the second chunk: the first chunk stays, the position counts from the call's start
    ids = c.ids.copy()
    ids[45, 31] ^= 0x80
    h2 = _hg(c, keep=(0, 0))
    with pytest.raises(HgxError) as ei:
        h2.insert_bodies_claimed(c.cols, ids)
    assert (ei.value.msg, ei.value.inserted, h2.num_events()) == (_mismatch(45), 45, 45)
    assert h2.BodiesState() == _counts(c, range(45))


# ---- checkpoints with event bodies (hgx_save_bodies, version 3) ---------------------------------------
def _v2_bytes(c):
    """What hgx_save writes for the chain: checkpoint.encode over the chain's own columns."""
    t = c.t
    return checkpoint.encode(c.n, 1, t.creator, t.index, t.sp, t.op, t.ts, t.s, c.ids[:, 16] != 0, t.ntx, t.txnil,
                             ids=c.ids, keys=c.keys)


def _v3_bytes(c, txs=None):
    t = c.t
    return checkpoint.encode(c.n, 1, t.creator, t.index, t.sp, t.op, t.ts, t.s, c.ids[:, 16] != 0, t.ntx, t.txnil,
                             ids=c.ids, keys=c.keys, bodies=(c.r, c.txs if txs is None else txs))


def _reencode(r, **repl):
    """checkpoint.encode of what checkpoint.read returned for a version-3 file, with some arguments replaced."""
    off, by = r["tx_off"], r["tx_bytes"]
    flat = [by[int(off[j]):int(off[j + 1])] for j in range(len(off) - 1)]
    txs, j = [], 0
    for k in range(r["E"]):
        txs.append(None if r["tx_nil"][k] else flat[j:j + int(r["ntx"][k])])
        j += int(r["ntx"][k])
    a = dict(roots=r["roots"], others=r["others"], kept=r["kept"], ids=r["ids"], keys=r["keys"], bodies=(r["sig_r"], txs),
             root_ids=r["root_ids"], kept_hashes=r["kept_hashes"])
    a.update(repl)
    return checkpoint.encode(r["n"], r["graphs"], r["creator"], r["index"], r["self_parent"], r["other_parent"],
                             r["timestamp_ns"], r["sig_s"], r["coin"], r["ntx"], r["tx_nil"], **a)


def _patched(data, pos, new):
    """The file with bytes [pos, pos + len(new)) replaced and a valid checksum again."""
    body = data[:pos] + new + data[pos + len(new):-8]
    return body + np.array([checkpoint.fnv1a(body)], "<u8").tobytes()


def _write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return str(path)


def _refused(h, path, why):
    with pytest.raises(HgxError) as ei:
        h.Bootstrap(path)
    assert (ei.value.code, ei.value.msg) == (INVALID, "hgx_bootstrap: " + why)
    assert h.num_events() == 0


# ---- 6. keeping context round trip -------------------------------------------------------------------
def test_keeping_context_round_trip(tmp_path):
    c = _chain()
    h = _hg(c)
    h.insert_bodies(c.cols)
    h.RunConsensus()
    p = str(tmp_path / "bodies.ckpt")
    h.save_bodies(p)
    data = open(p, "rb").read()
    assert data == _v3_bytes(c)   # every section, byte for byte, from the chain's own columns
    r = checkpoint.read(p)
    want_r, _, want_off, want_by = _expected(c, range(300))
    assert r["version"] == 3 and r["flags"] == 2 | 4 | 16
    assert np.array_equal(r["sig_r"], want_r) and np.array_equal(r["tx_off"], want_off) and r["tx_bytes"] == want_by
    assert data == _reencode(r)
    b = _hg(c)
    b.Bootstrap(p)
    assert b.BodiesState() == h.BodiesState() == _counts(c, range(300))
    _check(b, np.arange(300), c)
    _ids_are(b, c.ids)
    blocks = h.Blocks()
    assert b.Blocks() == blocks and len(blocks) >= 3
    for k in range(len(blocks)):
        assert b.BlockTransactions(k) == h.BlockTransactions(k), k
        assert b.BlockHash(k) == h.BlockHash(k), k
    got, want = b.results(), _oracle_results()
    for k in KEYS:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k
    p2 = str(tmp_path / "again.ckpt")
    b.save_bodies(p2)
    assert open(p2, "rb").read() == data
    # a context that keeps no bodies verifies the same file and stays as it is
    q = _hg(c, keep=None)
    q.Bootstrap(p)
    assert q.BodiesState()["state"] == 0
    _ids_are(q, c.ids)
    got = q.results()
    for k in KEYS:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k
    # hgx_save of the keeping context is the version-2 file it always was
    p3 = str(tmp_path / "plain.ckpt")
    h.save(p3)
    assert open(p3, "rb").read() == _v2_bytes(c)


# ---- 7. a pruned node --------------------------------------------------------------------------------
def _pruned_steps(k):
    """test_prune_compacts_the_store's run (n = 4, capacity 400): the steps up to and including prune k
    (counted from 1), and the rest, which holds a later prune. The second prune's frame has no Root.Others
    entry, the third one's has several: its file has pairs and its replay HGX_ROOT_OTHER events."""
    from test_gpu_bodies_rooted import SHAPES, chain_of, oracle_run
    c, run = chain_of(4), oracle_run(4)
    prunes = [i for i, x in enumerate(run["steps"]) if x["kind"] == "prune"]
    assert len(prunes) >= 4
    assert len(run["steps"][prunes[1]]["others"]) == 0 and len(run["steps"][prunes[2]]["others"]) >= 2
    at = prunes[k - 1]
    return c, SHAPES[4][4], run["steps"][:at + 1], run["steps"][at + 1:]


def _take_steps(h, c, steps):
    w = wireref.wire_cols(c)
    for x in steps:
        if x["kind"] == "prune":
            assert list(h.PruneToFrame()) == x["events"]
        else:
            h.insert_wire_bodies(w, int(x["sel"][0]), int(x["sel"][-1]) + 1)
        h.RunConsensus()


def _same_node(a, b, n):
    for p in range(n):
        assert a.GetRoot(p) == b.GetRoot(p), p
        assert a.GetRootIds(p) == b.GetRootIds(p), p
    assert a.GetRootOthers() == b.GetRootOthers()
    assert a.Blocks() == b.Blocks()
    for k in range(len(a.Blocks())):
        assert a.BlockHash(k) == b.BlockHash(k), k
    assert (a.LastConsensusRound(), a.LastCommitedRoundEvents(), a.ConsensusTransactions()) == \
        (b.LastConsensusRound(), b.LastCommitedRoundEvents(), b.ConsensusTransactions())
    assert list(a.Known()) == list(b.Known())
    assert a.BodiesState() == b.BodiesState() and a.num_events() == b.num_events()
    ea, eb = a.EventBodies(np.arange(a.num_events())), b.EventBodies(np.arange(b.num_events()))
    for k in ea:
        assert np.array_equal(ea[k], eb[k]), k
    ra, rb = a.results(), b.results()
    for k in KEYS:
        assert np.array_equal(np.asarray(ra[k]), np.asarray(rb[k])), k


@pytest.mark.parametrize("k", [2, 3])
def test_pruned_node(tmp_path, k):
    c, cap, head, rest = _pruned_steps(k)
    a = _hg(c, cap)
    _take_steps(a, c, head)
    assert len(a.GetRootOthers()) == len(head[-1]["others"]) and a.BodiesState()["state"] == 1
    p = str(tmp_path / "pruned.ckpt")
    a.save_bodies(p)
    r = checkpoint.read(p)
    assert r["version"] == 3 and r["flags"] == 1 | 2 | 4 | 16 and r["root_ids"][2] == a.GetRootOthers()
    assert sum(h is not None for h in r["kept_hashes"][0]) >= 1
    assert open(p, "rb").read() == _reencode(r)
    b = _hg(c, cap)
    b.Bootstrap(p)
    _same_node(a, b, c.n)
    # both go on: syncs from the wire, the later prune
    assert any(x["kind"] == "prune" for x in rest)
    _take_steps(a, c, rest)
    _take_steps(b, c, rest)
    _same_node(a, b, c.n)


# ---- 8. a tampered file ------------------------------------------------------------------------------
def test_tampered_file(tmp_path):
    c = _chain()
    E, C = 300, 4
    good = _write(tmp_path / "good.ckpt", _v3_bytes(c))
    k = next(k for k in range(100, 300) if c.txs[k] and any(len(b) for b in c.txs[k]))
    txs = list(c.txs)
    j = next(j for j, b in enumerate(txs[k]) if len(b))
    txs[k] = txs[k][:j] + [bytes([txs[k][j][0] ^ 1]) + txs[k][j][1:]] + txs[k][j + 1:]
    h = _hg(c)
    with pytest.raises(HgxError) as ei:
        h.Bootstrap(_write(tmp_path / "tx.ckpt", _v3_bytes(c, txs)))
    assert (ei.value.code, ei.value.msg) == (INVALID, f"hgx_bootstrap: event {k}: the file's id is not the event's hash")
    assert h.num_events() == k
    _ids_are(h, c.ids[:k])
    # structural faults: refused with the context untouched, which then takes the good file
    data = open(good, "rb").read()
    at_T = 32 + E * (4 + 8 * 4 + 32 + 1 + 4 + 1) + 32 * E + 65 * C + 32 * E
    T = int(np.frombuffer(data, "<i8", 1, at_T)[0])
    assert T == sum(len(x or []) for x in c.txs) and T >= 3
    off = np.frombuffer(data, "<i8", T + 1, at_T + 8)
    assert off[0] == 0 and off[-1] == len(data) - 8 - (at_T + 8 + 8 * (T + 1))
    h = _hg(c)
    _refused(h, _write(tmp_path / "t.ckpt", _patched(data, at_T, np.array([T + 1], "<i8").tobytes())),
             "T is not the sum of ntx")
    _refused(h, _write(tmp_path / "off.ckpt", _patched(data, at_T + 16, np.array([off[-1] + 1], "<i8").tobytes())),
             "tx_off decreases")
    _refused(h, _write(tmp_path / "flag.ckpt", _patched(data, 20, np.array([2 | 4 | 16 | 8], "<i4").tobytes())),
             "unsupported flags")
    body = data[:-8] + b"\0"
    _refused(h, _write(tmp_path / "long.ckpt", body + np.array([checkpoint.fnv1a(body)], "<u8").tobytes()), "size mismatch")
    h.Bootstrap(good)
    assert h.num_events() == E and h.BodiesState() == _counts(c, range(E))
    # pairs that are not the Root.Others keys: a rooted file
    cr, cap, head, _ = _pruned_steps(3)
    a = _hg(cr, cap)
    _take_steps(a, cr, head)
    pg = str(tmp_path / "rooted.ckpt")
    a.save_bodies(pg)
    r = checkpoint.read(pg)
    others = r["others"].copy()
    assert len(others) >= 1
    others[0, 5] ^= 1
    b = _hg(cr, cap)
    _refused(b, _write(tmp_path / "pairs.ckpt", _reencode(r, others=others)), "root pairs and Root.Others keys disagree")
    assert [b.GetRoot(p)["Index"] for p in range(cr.n)] == [-1] * cr.n   # (no root was installed)
    b.Bootstrap(pg)
    assert b.num_events() == a.num_events() and b.GetRootOthers() == a.GetRootOthers()


# ---- 9. hgx_save_bodies refusals ---------------------------------------------------------------------
def test_save_bodies_refusals(tmp_path):
    c = bodyref.chain(4, 200, 1)
    p = str(tmp_path / "no.ckpt")

    def refused(h, why):
        with pytest.raises(HgxError) as ei:
            h.save_bodies(p)
        assert (ei.value.code, ei.value.msg) == (INVALID, "hgx_save_bodies: " + why)
        assert not os.path.exists(p) and not os.path.exists(p + ".tmp")

    h = _hg(c, keep=None)   # never kept
    h.insert_bodies(c.cols, 0, 50)
    refused(h, "bodies not known")
    h = _hg(c)   # a lost store
    h.insert_bodies(c.cols, 0, 50)
    h.insert_trace(c.t, 50, 60)
    assert h.BodiesState()["state"] == 2
    refused(h, "bodies not known")
    h = _hg(c)   # the caller's own Reset: roots whose ids nobody supplied yet
    h.Reset([1, 1, 0, -1], [0, 0, 0, -1], [0, 0, 1, 0])
    assert h.BodiesState()["state"] == 1
    refused(h, "root ids not known")
    h.SetRootIds([None] * 4, [None, None, c.ids[0].tobytes(), None], [])
    h.save_bodies(p)   # (an empty rooted store is a file like any other)
    assert checkpoint.read(p)["E"] == 0
