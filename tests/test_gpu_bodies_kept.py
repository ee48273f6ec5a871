"""The resident body store (hgx_keep_bodies): R and the transaction bytes of every event
inserted through the body paths stay on the device and come back by gid (hgx_get_event_bodies), per
block (hgx_block_transactions) and with a sync response (hgx_diff_wire_bodies).

Expected values never come from the code under test: R and the transactions are the bodyref.Chain's,
order and block ranges come from the existing getters (hgx_consensus_events, hgx_block_info), block
contents of generated traces from hgref.Oracle.blocks()."""
import dataclasses
import functools
import hashlib

import numpy as np
import pytest

import bodyref
import hgref
import wireref
from babble_amd import trace as gtrace
from babble_amd._lib import HgxError
from babble_amd.hashgraph import Hashgraph, block_hash_batch, wire_body_columns

pytestmark = pytest.mark.gpu

INVALID, CAPACITY, NOT_FOUND, TOO_LATE = 102, 103, 1, 2
# every base64 tail, and every head / tail of the byte copy (16-byte vectors, dwords, single bytes)
LENS = (0, 1, 2, 3, 4, 15, 16, 17, 47, 48, 49, 255, 1000)
_OPEN = []


@pytest.fixture(autouse=True)
def _close_contexts():
    yield
    while _OPEN:
        _OPEN.pop().close()


def _hg(c, cap=None, keep=(1, 1), **kw):
    h = Hashgraph(c.n, capacity=max(cap or c.t.E, 16), **kw)
    _OPEN.append(h)
    h.set_participant_keys(c.keys)
    if keep is not None:
        h.KeepBodies(*keep)
    return h


def _own_lists(E, seed, sparse=False):
    """Per event nil, [], 1 or 3 transactions with lengths from LENS (sparse: about 85 % nil or [])."""
    rng = np.random.default_rng(seed)
    txs = []
    for _ in range(E):
        kind = rng.integers(0, 4) if not sparse else (rng.integers(0, 2) if rng.random() < 0.85 else rng.integers(2, 4))
        if kind == 0:
            txs.append(None)
        elif kind == 1:
            txs.append([])
        else:
            txs.append([rng.integers(0, 256, int(rng.choice(LENS)), dtype=np.uint8).tobytes()
                        for _ in range(1 if kind == 2 else 3)])
    return txs


@functools.lru_cache(maxsize=None)
def _chain_own(n, E, seed, sparse=False):
    """A gossip trace signed over the test's own transaction lists (the trace's ntx / txnil set to match)."""
    t = gtrace.gossip(n, E, seed, stale_prob=0.1, stale_depth=2)
    txs = _own_lists(E, seed + 1000, sparse)
    t = dataclasses.replace(t, ntx=np.asarray([len(x or []) for x in txs], np.int32),
                            txnil=np.asarray([x is None for x in txs], np.int32))
    return bodyref.build(t, txs)


def _expected(c, sel):
    """The chain's R, ntx (-1 = nil), offsets and bytes of chain events `sel`, in list order."""
    flat = [b for i in sel for b in (c.txs[int(i)] or [])]
    off = np.zeros(len(flat) + 1, np.int64)
    np.cumsum([len(b) for b in flat], out=off[1:])
    ntx = np.asarray([-1 if c.txs[int(i)] is None else len(c.txs[int(i)]) for i in sel], np.int32)
    return c.r[np.asarray(sel, np.int64)].reshape(-1, 32), ntx, off, b"".join(flat)


def _check(h, gids, c, src=None):
    """EventBodies(gids) equals the chain's (src: chain index of each resident gid, default identity)."""
    sel = [int(g) if src is None else src[int(g)] for g in gids]
    r, ntx, off, by = _expected(c, sel)
    got = h.EventBodies(gids)
    assert np.array_equal(got["sig_r"], r)
    assert np.array_equal(got["ntx"], ntx)
    assert np.array_equal(got["tx_off"], off)
    assert got["tx_bytes"].tobytes() == by


def _counts(c, sel):
    _, ntx, off, by = _expected(c, sel)
    return dict(state=1, events=len(sel), tx=int(np.maximum(ntx, 0).sum()), bytes=len(by))


def _raw_get(h, gids, tx_cap, bytes_cap, fill=0xA5):
    """hgx_get_event_bodies on sentinel-filled arrays: (rc, err message, n_tx, n_bytes, arrays)"""
    import ctypes as C
    from babble_amd._lib import hgx_error, ptr
    gids = np.ascontiguousarray(gids, np.int64)
    m = len(gids)
    r, ntx = np.full((max(m, 1), 32), fill, np.uint8), np.full(max(m, 1), 0x5A5A5A5A, np.int32)
    off, by = np.full(tx_cap + 1, -7, np.int64), np.full(max(bytes_cap, 1), fill, np.uint8)
    nt, nb, err = C.c_int64(-1), C.c_int64(-1), hgx_error()
    rc = h.L.hgx_get_event_bodies(h.ctx, ptr(gids), m, ptr(r), ptr(ntx), ptr(off), tx_cap, ptr(by), bytes_cap,
                                  C.byref(nt), C.byref(nb), C.byref(err))
    return rc, err.msg.decode(), nt.value, nb.value, (r, ntx, off, by)


def _untouched(arrays, fill=0xA5):
    r, ntx, off, by = arrays
    return (r == fill).all() and (ntx == 0x5A5A5A5A).all() and (off == -7).all() and (by == fill).all()


# ---- 1. round trip and growth ----------------------------------------------------------------------
def test_round_trip_and_growth():
    c = _chain_own(4, 300, 11)
    E = c.t.E
    kinds = {(-1 if x is None else len(x)) for x in c.txs}
    assert kinds == {-1, 0, 1, 3} and {len(b) for x in c.txs for b in (x or [])} == set(LENS)
    h = _hg(c, keep=(1, 1))   # the store grows several times from one transaction and one byte
    assert h.BodiesState() == dict(state=1, events=0, tx=0, bytes=0)
    assert np.array_equal(h.insert_bodies(c.cols, 0, 90), c.ids[:90])
    assert h.BodiesState() == _counts(c, range(90))
    _check(h, np.arange(90), c)
    assert np.array_equal(h.insert_bodies(c.cols, 90, 200), c.ids[90:200])
    ids, _, _ = h.insert_wire_bodies(wireref.wire_cols(c), 200, E)
    assert np.array_equal(ids, c.ids[200:])
    assert h.BodiesState() == _counts(c, range(E))
    rng = np.random.default_rng(3)
    for gids in (np.arange(E), np.arange(E)[::-1], rng.integers(0, E, 500), np.zeros(0, np.int64),
                 np.asarray([7, 7, 7]), np.asarray([E - 1])):
        _check(h, gids, c)
    # the sizing call, one short in either capacity, and gids outside the store
    _, ntx, off, by = _expected(c, range(E))
    T, B = len(off) - 1, len(by)
    all_g = np.arange(E)
    for tc, bc in ((0, 0), (T - 1, B), (T, B - 1)):
        rc, msg, nt, nb, arrays = _raw_get(h, all_g, tc, bc)
        assert (rc, nt, nb) == (CAPACITY, T, B) and msg.startswith("hgx_get_event_bodies:"), (tc, bc, msg)
        assert _untouched(arrays)
    rc, _, nt, nb, arrays = _raw_get(h, all_g, T, B)
    assert (rc, nt, nb) == (0, T, B) and arrays[3].tobytes() == by and np.array_equal(arrays[2], off)
    for bad in (E, -1):
        rc, msg, nt, nb, arrays = _raw_get(h, [0, bad, 1], T, B)
        assert (rc, msg) == (NOT_FOUND, f"{bad}, Not Found") and (nt, nb) == (-1, -1) and _untouched(arrays)


# ---- 2. the seam between two internal chunks -------------------------------------------------------
def test_chunk_seam():
    """test_large_transactions_split_into_chunks' batch: 40 first events of 768 KiB each and 10 small
    ones, two internal chunks; about 30 MiB go through the arena's growth."""
    big = bytes(range(256)) * (3 << 10)
    creator = list(range(40)) + list(range(10))
    sp = [-1] * 40 + list(range(10))
    op = [-1] * 40 + [(k + 7) % 40 for k in range(9)] + [48]
    txs = [[big[k:]] for k in range(40)] + [[b"a"], None, [], [b"bc", b""]] * 2 + [[b"d"], []]
    c = bodyref.manual(64, creator, sp, op, txs)
    assert sum(map(len, c.json[:32])) > 32 << 20 > sum(map(len, c.json[:31]))   # the seam: events 30 | 31
    h = _hg(c, keep=(0, 0))
    assert np.array_equal(h.insert_bodies(c.cols), c.ids)
    assert h.BodiesState() == _counts(c, range(50))
    _check(h, [29, 30, 31, 32, 39, 40, 41, 42, 43, 49, 0], c)
    _check(h, np.arange(50)[::-1], c)


# ---- 3. a rejected suffix leaves nothing behind ----------------------------------------------------
def test_rejected_suffix():
    c = _chain_own(4, 300, 11)
    h = _hg(c)
    h.insert_bodies(c.cols, 0, 100)
    m = 57
    s = c.t.s.copy()
    s[100 + m, 31] ^= 1
    with pytest.raises(HgxError) as ei:
        h.insert_bodies(c.columns(s=s), 100, 250)
    assert (ei.value.code, ei.value.msg, ei.value.inserted) == (104, "Invalid signature", m)
    assert h.BodiesState() == _counts(c, range(100 + m))
    h.insert_bodies(c.cols, 100 + m, 300)
    assert h.BodiesState() == _counts(c, range(300))
    _check(h, np.arange(300), c)


# ---- 4. the lost state -------------------------------------------------------------------------------
# Four consumers take a context (hgx_block_hash_batch has none, so no store to lose). The fifth reader of the
# store is hgx_find_order's eager hashing: on a lost store it still makes its blocks and hashes none of them.
def _consumers(h):
    return (("hgx_get_event_bodies", lambda: h.EventBodies([0])),
            ("hgx_block_transactions", lambda: h.BlockTransactions(0)),
            ("hgx_get_block_hash", lambda: h.BlockHash(0)),
            ("hgx_diff_wire_bodies", lambda: h.DiffWireBodies(np.full(h.n, -1, np.int32))))


def test_lost_state_and_contexts_that_never_kept():
    c = bodyref.chain(4, 200, 1)
    h = _hg(c)
    h.insert_bodies(c.cols, 0, 100)
    with pytest.raises(HgxError) as ei:   # only on a context without events
        h.KeepBodies(0, 0)
    assert ei.value.code == INVALID and ei.value.msg.startswith("hgx_keep_bodies: ")
    h.insert_trace(c.t, 100, 110)   # hgx_insert_events: ten events without their bodies
    assert h.BodiesState()["state"] == 2
    h.RunConsensus()   # hgx_find_order on the lost store: blocks as ever, block 0 exists for the two block consumers
    assert len(h.Blocks()) > 0
    for fn, call in _consumers(h):
        with pytest.raises(HgxError) as ei:
            call()
        assert (ei.value.code, ei.value.msg) == (INVALID, fn + ": bodies not known")
    h.insert_bodies(c.cols, 110, 120)   # nothing is appended while lost
    assert h.BodiesState() == dict(state=2, events=100, tx=_counts(c, range(100))["tx"],
                                   bytes=_counts(c, range(100))["bytes"])
    h.clear()
    assert h.BodiesState() == dict(state=1, events=0, tx=0, bytes=0)
    h.insert_bodies(c.cols)
    _check(h, np.arange(200), c)
    h.RunConsensus()
    assert len(h.Blocks()) > 0 and isinstance(h.BlockTransactions(0), list)
    rows, count, over = h.DiffWireBodies(np.full(4, -1, np.int32))
    assert count == 200 and not over
    # a context that never kept: the consumers refuse, and the body path gives what it gave before
    p = _hg(c, keep=None)
    assert np.array_equal(p.insert_bodies(c.cols), c.ids)
    assert p.BodiesState() == dict(state=0, events=0, tx=0, bytes=0)
    for fn, call in _consumers(p):
        with pytest.raises(HgxError) as ei:
            call()
        assert (ei.value.code, ei.value.msg) == (INVALID, fn + ": bodies not known")
    p.RunConsensus()
    a, b, o = p.results(), h.results(), hgref.oracle_run(c.t).results()
    for k in ("round", "witness", "famous", "rr", "cts", "order"):
        assert np.array_equal(np.asarray(a[k]), np.asarray(o[k])), k
        assert np.array_equal(np.asarray(b[k]), np.asarray(o[k])), k


def test_keep_bodies_refusals():
    c = bodyref.chain(4, 200, 1)
    h = _hg(c, keep=None)
    for hints in ((-1, 0), (0, -1)):
        with pytest.raises(HgxError) as ei:
            h.KeepBodies(*hints)
        assert (ei.value.code, ei.value.msg) == (INVALID, "hgx_keep_bodies: negative hint")
    assert h.BodiesState()["state"] == 0
    h.KeepBodies(0, 0)
    h.KeepBodies(10, 10)   # again on an empty context: allowed
    assert h.BodiesState()["state"] == 1


# ---- 5. the block encoder alone ----------------------------------------------------------------------
def _want_hash(rr, txs, nil):
    # (Block.Transactions is nil only while nothing was appended to a nil list: the oracle's encoder takes that flag)
    return hashlib.sha256(hgref.go_block_json(rr, txs, bool(nil) and not txs)).digest()


def test_block_encoder_alone():
    rng = np.random.default_rng(5)
    RR = (0, 9, 10, 999, 1000, 123456)
    blocks = [(rr, [rng.integers(0, 256, L, dtype=np.uint8).tobytes()], False) for L in range(201) for rr in RR]
    # every text length mod 64 occurs: both SHA padding cases and the 55 / 56 / 63 / 64 seams
    assert {len(hgref.go_block_json(*b)) % 64 for b in blocks} == set(range(64))
    blocks += [(3, [], True), (3, [], False), (4, [b""], True), (5, [b""] * 1000, False),
               (6, [rng.integers(0, 256, 200000, dtype=np.uint8).tobytes()], False),
               (7, [b"a", b"", b"bcd", b"\xff" * 50], True)]
    assert hgref.go_block_json(3, [], True).endswith(b'"Transactions":null}\n')
    assert hgref.go_block_json(3, [], False).endswith(b'"Transactions":[]}\n')
    got = block_hash_batch(blocks)
    bad = [k for k, b in enumerate(blocks) if got[k] != _want_hash(*b)]
    assert not bad, bad[:10]
    assert block_hash_batch([]) == []
    assert block_hash_batch(blocks[-1:]) == [_want_hash(*blocks[-1])]


# ---- 6. block transactions end to end ----------------------------------------------------------------
class _ListTrace:
    """A trace with explicit transaction lists, as hgref.Oracle.insert_trace takes one event at a time."""

    def __init__(self, c):
        t = c.t
        self.n, self.E = t.n, t.E
        self.creator, self.index, self.sp, self.op, self.ts = t.creator, t.index, t.sp, t.op, t.ts
        self.hash, self.s, self.txnil = t.hash, t.s, t.txnil
        self.txs = [x or [] for x in c.txs]


@functools.lru_cache(maxsize=None)
def _own_oracle(n, E, seed, sync):
    """Seeds chosen with the oracle: its blocks over the test's sparse lists, per consensus call."""
    c = _chain_own(n, E, seed, sparse=True)
    o = hgref.Oracle(n)
    lt = _ListTrace(c)
    per_call = []
    for lo in range(0, E, sync):
        o.insert_trace(lt, lo, min(E, lo + sync))
        rc, msg = o.run_consensus()
        assert not rc, msg
        per_call.append(len(o.blocks()))
    # blocks of two or more events whose first event is nil but which have transactions: a block is the
    # events of one round received, in the oracle's consensus order
    res = o.results()
    nil_first = 0
    for b in o.blocks():
        evs = [int(g) for g in res["order"] if res["rr"][int(g)] == b["rr"]]
        nil_first += len(evs) >= 2 and c.txs[evs[0]] is None and b["ntx"] > 0
    return c, o.blocks(), per_call, nil_first


_OWN_CASES = [(4, 400, 20), (16, 600, 37)]


def _own_conditions():
    """The issue's five conditions on the CPU oracle's result, before any context exists. At n = 16 a block of
    a 600-event trace holds some 150 events, so with 15 % of the events carrying transactions none can be
    null or [], and no call of 60 events makes two blocks: those three hold at n = 4 and are asserted over
    the two cases together; three committed blocks and a nil-first block with transactions hold in each."""
    runs = [_own_oracle(n, E, seed, 60) for n, E, seed in _OWN_CASES]
    blocks = [b for r in runs for b in r[1]]
    assert any(b["tx_nil"] and b["ntx"] == 0 for b in blocks)
    assert any(not b["tx_nil"] and b["ntx"] == 0 for b in blocks)
    assert any(y - x >= 2 for r in runs for x, y in zip([0] + r[2], r[2]))
    for r in runs:
        assert sum(b["committed"] for b in r[1]) >= 3
        assert r[3] >= 1


# The seeds were chosen with the oracle.
@pytest.mark.parametrize("n,E,seed", _OWN_CASES)
def test_block_transactions_own_lists(n, E, seed):
    _own_conditions()   # on the CPU oracle's result, before the GPU is used
    c, oblocks, per_call, _ = _own_oracle(n, E, seed, 60)
    h = _hg(c)
    seen = {}

    def on_commit(g, b, rr, first, nev, ntx):   # the block's transactions and hash from inside commitCh
        seen[b] = (h.BlockTransactions(b), h.BlockHash(b))
        assert len(seen[b][0]) == ntx

    h.set_commit_callback(on_commit)
    for lo in range(0, E, 60):
        h.insert_bodies(c.cols, lo, min(E, lo + 60))
        h.RunConsensus()
    order, blocks = h.ConsensusEvents(), h.Blocks()
    assert len(blocks) == len(oblocks)
    for b, (blk, ob) in enumerate(zip(blocks, oblocks)):
        evs = order[blk["first"]:blk["first"] + blk["n_events"]]
        want = [x for g in evs for x in (c.txs[int(g)] or [])]
        got = h.BlockTransactions(b)
        assert got == want == ob["txs"], b
        assert len(got) == blk["ntx"]
        assert h.BlockHash(b) == _want_hash(blk["rr"], want, blk["tx_nil"]) == ob["hash"], b
        if blk["committed"]:
            assert seen[b] == (want, ob["hash"])
    assert sorted(seen) == [b for b, blk in enumerate(blocks) if blk["committed"]]
    with pytest.raises(HgxError) as ei:
        h.BlockTransactions(len(blocks))
    assert (ei.value.code, ei.value.msg) == (NOT_FOUND, f"{len(blocks)}, Not Found")
    with pytest.raises(HgxError) as ei:
        h.BlockHash(len(blocks))
    assert (ei.value.code, ei.value.msg) == (NOT_FOUND, f"{len(blocks)}, Not Found")


def test_block_transactions_generated_trace():
    c = bodyref.chain(4, 400, 7)
    ob = hgref.oracle_run(c.t, chunk=80).blocks()
    h = _hg(c)
    for lo in range(0, 400, 80):
        h.insert_bodies(c.cols, lo, lo + 80)
        h.RunConsensus()
    assert len(h.Blocks()) == len(ob) >= 3
    for b, o in enumerate(ob):
        assert h.BlockTransactions(b) == o["txs"], b
        assert h.BlockHash(b) == o["hash"], b


# ---- 7. a batched context ----------------------------------------------------------------------------
def test_batched_context():
    a, b = bodyref.chain(4, 200, 1), bodyref.chain(4, 200, 5)
    t = dataclasses.replace(gtrace.concat_graphs([a.t, b.t]), n=8)   # (eight keys: graph g owns 4g .. 4g + 3)
    c = bodyref.build(t, a.txs + b.txs)
    h = Hashgraph(4, capacity=400, n_graphs=2)
    _OPEN.append(h)
    h.set_participant_keys(c.keys)
    h.KeepBodies(0, 0)
    assert np.array_equal(h.insert_bodies(c.cols), c.ids)
    h.RunConsensus()
    _check(h, np.arange(400)[::-1], c)
    for g in range(2):   # (the batched chain has its own signatures, so the order within a block is its own)
        order, blocks = h.ConsensusEvents(g), h.Blocks(g)
        assert len(blocks) >= 3 and sum(blk["ntx"] for blk in blocks) > 0
        for k, blk in enumerate(blocks):
            evs = order[blk["first"]:blk["first"] + blk["n_events"]]
            assert all(200 * g <= int(x) < 200 * (g + 1) for x in evs)
            want = [x for e in evs for x in (c.txs[int(e)] or [])]
            assert h.BlockTransactions(k, graph=g) == want and len(want) == blk["ntx"], (g, k)
            assert h.BlockHash(k, graph=g) == _want_hash(blk["rr"], want, blk["tx_nil"]), (g, k)


# ---- 8. prune ------------------------------------------------------------------------------------------
def test_prune_compacts_the_store():
    """test_gpu_bodies_rooted's long run (n = 4, capacity 400, syncs of 100, a prune before each sync that
    would not fit): the store follows the events through every prune."""
    from test_gpu_bodies_rooted import SHAPES, chain_of, oracle_run
    c, run = chain_of(4), oracle_run(4)
    assert run["n_prunes"] >= 3
    h = _hg(c, SHAPES[4][4])
    w = wireref.wire_cols(c)
    src, hashes = [], []

    def run_and_check_new_blocks():
        nb0 = len(h.Blocks())
        h.RunConsensus()
        order, blocks = h.ConsensusEvents(), h.Blocks()
        for b in range(nb0, len(blocks)):   # the blocks made by this call
            blk = blocks[b]
            evs = order[blk["first"]:blk["first"] + blk["n_events"]]
            want = [t for g in evs for t in (c.txs[src[int(g)]] or [])]
            assert h.BlockTransactions(b) == want, b
            hashes.append(_want_hash(blk["rr"], want, blk["tx_nil"]))
            assert h.BlockHash(b) == hashes[-1], b

    for x in run["steps"]:
        if x["kind"] == "prune":
            nb_before = len(h.Blocks())
            old = h.PruneToFrame()
            assert [h.BlockHash(b) for b in range(nb_before)] == hashes   # the hashes survive, as the blocks do
            assert list(old) == x["events"]
            src = [src[int(g)] for g in old]
            assert h.BodiesState() == _counts(c, src)   # the dropped events' bytes were released
            _check(h, np.arange(len(src)), c, src)
            if nb_before:
                with pytest.raises(HgxError) as ei:
                    h.BlockTransactions(0)
                assert (ei.value.code, ei.value.msg) == \
                    (TOO_LATE, "hgx_block_transactions: block 0: events no longer resident")
            run_and_check_new_blocks()
            continue
        sel = x["sel"]
        lo, hi = int(sel[0]), int(sel[-1]) + 1
        h.insert_wire_bodies(w, lo, hi)
        src += list(range(lo, hi))
        run_and_check_new_blocks()
    assert len(hashes) == len(h.Blocks()) >= 3
    assert h.BodiesState() == _counts(c, src)
    _check(h, np.arange(len(src))[::-1], c, src)


# ---- 9. the sync loop with no body store on the host -----------------------------------------------
def test_sync_loop_without_a_host_body_store():
    c = bodyref.chain(16, 600, 2)
    t, E = c.t, 600
    A, B = _hg(c), _hg(c, keep=None)
    A.insert_bodies(c.cols)
    B.insert_wire_bodies(wireref.wire_cols(c), 0, 100)
    rounds = 0
    while B.num_events() < E:
        known = B.Known()
        rows, count, over = A.DiffWireBodies(known, sync_limit=1000, cap=130)
        plain, count2, _ = A.DiffWire(known, sync_limit=1000, cap=130)
        assert not over and count == count2 == E - B.num_events() and len(rows["gid"]) == min(130, count)
        for k, v in plain.items():
            assert np.array_equal(rows[k], v), k
        g = rows["gid"]
        r, ntx, off, by = _expected(c, g)
        assert np.array_equal(rows["sig_r"], r) and np.array_equal(rows["tx_off"], off)
        assert rows["tx_bytes"].tobytes() == by
        assert np.array_equal(np.where(rows["tx_nil"] != 0, -1, rows["ntx"]), ntx)
        # B is fed only what A returned
        resp = dict(creator_id=rows["creator_id"], index=rows["index"], self_parent_index=rows["self_parent_index"],
                    other_parent_creator=rows["other_parent_creator"], other_parent_index=rows["other_parent_index"],
                    timestamp_ns=rows["timestamp_ns"], sig_r=rows["sig_r"], sig_s=rows["sig_s"],
                    ntx=np.where(rows["tx_nil"] != 0, -1, rows["ntx"]).astype(np.int32), tx_off=rows["tx_off"],
                    tx_bytes=np.concatenate([rows["tx_bytes"], np.zeros(1, np.uint8)]))
        ids, sp, op = B.insert_wire_bodies(resp)
        assert np.array_equal(ids, c.ids[g]) and np.array_equal(sp, t.sp[g]) and np.array_equal(op, t.op[g])
        B.RunConsensus()
        rounds += 1
    assert rounds == 4
    _, count, _ = A.DiffWireBodies(B.Known())
    assert count == 0
    A.RunConsensus()
    a, b, o = A.results(), B.results(), hgref.oracle_run(t, chunk=None).results()
    for k in ("round", "witness", "famous", "rr", "cts", "order"):
        assert np.array_equal(np.asarray(b[k]), np.asarray(o[k])), k
        assert np.array_equal(np.asarray(a[k]), np.asarray(o[k])), k


def test_diff_wire_bodies_sizing_capacity_and_limit():
    import ctypes as C
    from babble_amd import _lib
    from babble_amd._lib import hgx_error, ptr
    c = bodyref.chain(16, 600, 2)
    A = _hg(c)
    A.insert_bodies(c.cols)
    known = np.full(16, 3, np.int32)
    plain, total, _ = A.DiffWire(known)
    g_all = plain["gid"]
    spec = {nm: (dt, shp) for nm, dt, shp in _lib.WIRE_OUT_COLUMNS}

    def call(cap, tx_cap, bytes_cap, limit=-1, null_body=False):
        cols = {nm: np.full((max(cap, 1),) + shp, 0x5A, dt) for nm, (dt, shp) in spec.items()}
        r = np.full((max(cap, 1), 32), 0xA5, np.uint8)
        off, by = np.full(tx_cap + 1, -7, np.int64), np.full(max(bytes_cap, 1), 0xA5, np.uint8)
        out = _lib.hgx_wire_out(**{nm: ptr(a) for nm, a in cols.items()})
        body = _lib.hgx_wire_body_out(ptr(r), ptr(off), tx_cap, ptr(by), bytes_cap)
        cnt, nt, nb, over, err = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1), C.c_int32(-1), hgx_error()
        rc = A.L.hgx_diff_wire_bodies(A.ctx, 0, ptr(known), limit, C.byref(out), None if null_body else C.byref(body),
                                      cap, C.byref(cnt), C.byref(nt), C.byref(nb), C.byref(over), C.byref(err))
        clean = all((a == a.dtype.type(0x5A) if a.dtype != np.uint8 else a == 0x5A).all() for a in cols.values()) and \
            (r == 0xA5).all() and (off == -7).all() and (by == 0xA5).all()
        return rc, (cnt.value, nt.value, nb.value, over.value), clean, (cols, r, off, by)

    for cap in (total, 50):   # every row, and cap smaller than count
        g = g_all[:cap]
        r, ntx, off, by = _expected(c, g)
        T, B = len(off) - 1, len(by)
        assert T > 0 and B > 0
        for kw in (dict(tx_cap=0, bytes_cap=0), dict(tx_cap=0, bytes_cap=0, null_body=True),
                   dict(tx_cap=T - 1, bytes_cap=B), dict(tx_cap=T, bytes_cap=B - 1)):
            rc, counts, clean, _ = call(cap, **kw)
            assert rc == CAPACITY and counts == (total, T, B, 0) and clean, kw
        rc, counts, _, (cols, gr, goff, gby) = call(cap, T, B)
        assert rc == 0 and counts == (total, T, B, 0)
        assert np.array_equal(cols["gid"][:cap], g) and np.array_equal(gr[:cap], r)
        assert np.array_equal(goff, off) and gby[:B].tobytes() == by
    rc, counts, clean, _ = call(total, 0, 0, limit=10)   # over the sync limit: the sum, nothing else
    assert rc == 0 and counts[0] > 10 and counts[3] == 1 and clean
