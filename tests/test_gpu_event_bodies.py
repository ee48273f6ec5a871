"""Event bodies on the device: hgx_event_json_batch (the Go-JSON encoder, byte for byte against the
oracle's encoder) and hgx_insert_event_bodies (texts, ids in dependency order, body digests, verified
insert) against the chain tests/bodyref.py builds on the CPU with libcrypto signatures.
  * the encoder over every format edge (transaction lists and base64 tails, empty parents, timestamp
    fractions, pre-1970 and 2262, R / S magnitudes), the sizing call and the too-small capacity;
  * whole signed traces: every id equals the CPU chain's, consensus is bit-exact with the oracle;
  * two calls: the second call's parents' ids come from the store;
  * tampered events fail Event.Verify at the right position, the prefix stays, the good tail completes;
  * the refusals and the unknown-parent deviation (include/hgx.h)."""
import numpy as np
import pytest

import bodyref
import hgref
from babble_amd import trace as gtrace
from babble_amd._lib import HgxError
from babble_amd.hashgraph import Hashgraph, body_columns, compact_columns, event_json_batch

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------- the encoder
def _encoder_cases(m=210):
    rng = np.random.default_rng(3)
    rb = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()
    tx_lists = [None, [], [b""], [rb(1)], [rb(2)], [rb(3)], [rb(64)], [rb(1000)],
                [rb(k) for k in (0, 1, 2, 3, 64, 1000, 5)]]
    parents = [(-1, -1), (-1, 7), (7, -1), (7, 9)]
    stamps = [hgref.T0_NS, hgref.T0_NS + 500_000_000, hgref.T0_NS + 123_456_789, -1_500_000_000 - 250,
              2**63 - 1, 9_214_646_400_000_000_000 + 1000, 0]   # (…, pre-1970, 2262-04-11, 2262-01-01, the epoch)
    big = [bytes(32), bytes(31) + b"\x01", bytes(31) + b"\xc8", b"\xff" * 32, rb(32), bytes(12) + rb(20)]
    keys = np.frombuffer(rb(3 * 65), np.uint8).reshape(3, 65)
    ev = [dict(creator=i % 3, index=(0, 123456)[i % 2], sp=parents[i % 4][0], op=parents[i % 4][1],
               ts=stamps[i % 7], r=big[i % 6] if i % 11 else rb(32), s=big[(i // 6) % 6] if i % 13 else rb(32),
               txs=tx_lists[i % 9]) for i in range(m)]
    cols = body_columns(*[[e[k] for e in ev] for k in ("creator", "index", "sp", "op", "ts")],
                        np.frombuffer(b"".join(e["r"] for e in ev), np.uint8),
                        np.frombuffer(b"".join(e["s"] for e in ev), np.uint8), [e["txs"] for e in ev])
    spi = np.frombuffer(rb(32 * m), np.uint8).reshape(m, 32)
    opi = np.frombuffer(rb(32 * m), np.uint8).reshape(m, 32)
    want = [hgref.go_event_json(e["txs"], bodyref.hex_id(bytes(spi[i]) if e["sp"] != -1 else None),
                                bodyref.hex_id(bytes(opi[i]) if e["op"] != -1 else None), bytes(keys[e["creator"]]),
                                e["ts"], e["index"], e["r"], e["s"]) for i, e in enumerate(ev)]
    return cols, keys, spi, opi, want


def test_encoder_byte_for_byte():
    cols, keys, spi, opi, want = _encoder_cases()
    data, off = event_json_batch(cols, keys, spi, opi)
    assert off[0] == 0 and list(np.diff(off)) == [len(w) for w in want]
    raw = data.tobytes()
    for i, w in enumerate(want):
        assert raw[off[i]:off[i + 1]] == w, (i, raw[off[i]:off[i + 1]], w)
    assert any(b'"Transactions":null' in w for w in want) and any(b'"Parents":["",""]' in w for w in want)
    assert any(b"1969-12-31T23:59:58.49999975Z" in w for w in want) and any(b'"2262-04-11T' in w for w in want)
    assert any(b'"R":0,' in w for w in want) and any(w.endswith(b'"S":' + str(2**256 - 1).encode() + b"}\n") for w in want)


def test_encoder_sizing_call_and_small_capacity():
    cols, keys, spi, opi, want = _encoder_cases(60)
    total = sum(len(w) for w in want)
    data, off = event_json_batch(cols, keys, spi, opi, out_cap=0)      # out == NULL: sizes only
    assert len(data) == 0 and off[-1] == total and list(np.diff(off)) == [len(w) for w in want]
    with pytest.raises(HgxError) as ei:
        event_json_batch(cols, keys, spi, opi, out_cap=total - 1)
    assert ei.value.code == 102 and "out_cap" in ei.value.msg
    assert list(np.diff(ei.value.offsets)) == [len(w) for w in want]   # offsets are still filled
    data, _ = event_json_batch(cols, keys, spi, opi, out_cap=total)    # exactly enough
    assert data.tobytes() == b"".join(want)


# ----------------------------------------------------------------------------- the chain
def _hg(c, cap=None):
    h = Hashgraph(c.n, capacity=cap or c.t.E)
    h.set_participant_keys(c.keys)
    return h


def _same_consensus(h, t):
    a, b = h.results(), hgref.oracle_run(t).results()
    for k in ("round", "witness", "famous", "rr", "cts"):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    assert list(a["order"]) == list(b["order"])


@pytest.mark.parametrize("n,E,seed", [(4, 200, 1), (16, 600, 2), (2, 150, 3), (128, 1024, 4)])
def test_chain_ids_and_consensus(n, E, seed):
    c = bodyref.chain(n, E, seed)
    h = _hg(c)
    ids = h.insert_bodies(c.cols)
    assert h.num_events() == E
    bad = np.nonzero((ids != c.ids).any(axis=1))[0]
    assert len(bad) == 0, (bad[:8], c.level[bad[:8]])
    for g in (0, 1, E // 2, E - 1):
        assert h.event_id(g) == bytes(c.ids[g])
    h.RunConsensus()
    _same_consensus(h, c.t)


def test_two_calls_read_parent_ids_from_the_store():
    c = bodyref.chain(4, 200, 1)
    cut = 80   # 40 %
    h = _hg(c)
    a = h.insert_bodies(c.cols, 0, cut)
    b = h.insert_bodies(c.cols, cut, c.t.E)
    assert np.array_equal(np.concatenate([a, b]), c.ids)
    h.RunConsensus()
    h1 = _hg(c)
    h1.insert_bodies(c.cols)
    h1.RunConsensus()
    assert list(h.ConsensusEvents()) == list(h1.ConsensusEvents())
    _same_consensus(h, c.t)


def test_batched_context_one_workgroup_per_graph():
    """Two graphs in one batch, interleaved: the id pass runs a workgroup per graph."""
    a = gtrace.gossip(4, 120, 5)
    n, E = 4, 240
    creator = np.empty(E, np.int32)
    sp, op = np.empty(E, np.int64), np.empty(E, np.int64)
    for g in (0, 1):   # graph g's event i is batch position 2 i + g
        creator[g::2] = a.creator + g * n
        sp[g::2] = np.where(a.sp >= 0, 2 * a.sp + g, -1)
        op[g::2] = np.where(a.op >= 0, 2 * a.op + g, -1)
    c = bodyref.manual(2 * n, creator, sp, op, [[b"tx %d" % k] if k % 3 else [] for k in range(E)])
    h = Hashgraph(n, capacity=E, n_graphs=2)
    h.set_participant_keys(c.keys)
    assert np.array_equal(h.insert_bodies(c.cols), c.ids) and h.num_events() == E


def test_large_transactions_split_into_chunks():
    """40 first events of 1 MiB of text each: 31 fill one internal chunk (32 MiB), the rest of the
    batch goes through a second chunk whose parents' ids come from the first."""
    big = bytes(range(256)) * (3 << 10)   # 768 KiB, 1 MiB as base64
    creator = list(range(40)) + list(range(10))
    sp = [-1] * 40 + list(range(10))
    op = [-1] * 40 + [(k + 7) % 40 for k in range(9)] + [48]
    txs = [[big[k:]] for k in range(40)] + [[b"a"], None, [], [b"bc", b""]] * 2 + [[b"d"], []]
    c = bodyref.manual(64, creator, sp, op, txs)
    assert sum(map(len, c.json[:32])) > 32 << 20 > sum(map(len, c.json[:31]))
    h = _hg(c)
    assert np.array_equal(h.insert_bodies(c.cols), c.ids) and h.num_events() == 50


def test_forked_batch_wider_than_a_workgroup():
    """1 500 events without parents at n = 4: one level wider than the id pass's workgroup, which
    strides over it. The first four are the creators' first events; the fifth is a fork."""
    E = 1500
    none = np.full(E, -1, np.int64)
    c = bodyref.manual(4, np.arange(E) % 4, none, none, [[]] * E)
    assert c.level.max() == 0
    h = _hg(c)
    with pytest.raises(HgxError) as ei:
        h.insert_bodies(c.cols)
    assert ei.value.msg == "CheckSelfParent: Self-parent not last known event by creator"
    assert ei.value.inserted == 4 and np.array_equal(ei.value.ids, c.ids[:4])


def _tampered(c, what):
    t = c.t
    k0 = next(k for k in range(110, t.E) if t.ntx[k] > 0 and t.op[k] >= 0)
    if what == "tx":
        txs = list(c.txs)
        txs[k0] = [bytes([txs[k0][0][0] ^ 1]) + txs[k0][0][1:]]
        return k0, c.columns(txs=txs)
    if what == "ts":
        ts = t.ts.copy()
        ts[k0] += 1
        return k0, c.columns(ts=ts)
    op = t.op.copy()
    op[k0] = next(g for g in range(k0 - 1, -1, -1) if g != t.op[k0] and t.creator[g] != t.creator[k0])
    return k0, c.columns(op=op)


@pytest.mark.parametrize("what", ["tx", "ts", "op"])
def test_tampered_event_fails_verify(what):
    c = bodyref.chain(4, 200, 1)
    k0, cols = _tampered(c, what)
    h = _hg(c)
    with pytest.raises(HgxError) as ei:
        h.insert_bodies(cols)
    assert ei.value.msg == "Invalid signature" and ei.value.code == 104
    assert ei.value.inserted == k0 and h.num_events() == k0
    assert np.array_equal(ei.value.ids, c.ids[:k0])
    assert h.event_id(k0 - 1) == bytes(c.ids[k0 - 1])
    # the caller resends the good tail
    tail = h.insert_bodies(c.cols, k0, c.t.E)
    assert np.array_equal(tail, c.ids[k0:]) and h.num_events() == c.t.E
    h.RunConsensus()
    assert list(h.ConsensusEvents()) == list(hgref.oracle_run(c.t).results()["order"])


def test_good_signature_wrong_self_parent():
    """Event k0 names another creator's event as self-parent and is signed that way: Verify passes,
    CheckSelfParent rejects it."""
    c = bodyref.chain(4, 200, 1)
    t = c.t
    k0 = 120
    j = next(g for g in range(k0 - 1, -1, -1) if t.creator[g] != t.creator[k0])
    sp, r, s = t.sp.copy(), c.r.copy(), t.s.copy()
    sp[k0] = j
    r[k0], s[k0] = c.sign_event(k0, j, int(t.op[k0]))
    h = _hg(c)
    with pytest.raises(HgxError) as ei:
        h.insert_bodies(c.columns(sp=sp, r=r, s=s))
    assert ei.value.msg == "CheckSelfParent: Self-parent not last known event by creator" and ei.value.code == 100
    assert ei.value.inserted == k0 and np.array_equal(ei.value.ids, c.ids[:k0])


# ----------------------------------------------------------------------------- refusals
def test_refusals():
    c = bodyref.chain(4, 200, 1)
    h = Hashgraph(4, capacity=c.t.E)
    with pytest.raises(HgxError) as ei:
        h.insert_bodies(c.cols)
    assert ei.value.code == 102 and "participant keys not set" in ei.value.msg and h.num_events() == 0
    # a context filled through the compact columns holds no ids
    h.set_participant_keys(c.keys)
    assert h.insert_events32(compact_columns(c.t), 0, 50) == 50
    with pytest.raises(HgxError) as ei:
        h.insert_bodies(c.cols, 50, c.t.E)
    assert ei.value.code == 102 and "ids not known" in ei.value.msg and h.num_events() == 50
    # after a Reset the parents outside the store have no id column
    h2 = _hg(c)
    h2.Reset([3] * 4, [1] * 4, [0] * 4)
    with pytest.raises(HgxError) as ei:
        h2.insert_bodies(c.cols)
    assert ei.value.code == 102 and "hgx_reset" in ei.value.msg


def test_unknown_parent_cuts_the_batch():
    """An HGX_UNKNOWN_PARENT other-parent has no id string: the prefix is inserted, then the event
    fails its parent check (the documented deviation: no Verify for it)."""
    c = bodyref.chain(4, 200, 1)
    k0 = 130
    op = c.t.op.copy()
    op[k0] = -2
    h = _hg(c)
    with pytest.raises(HgxError) as ei:
        h.insert_bodies(c.columns(op=op))
    assert ei.value.msg == "CheckOtherParent: Other-parent not known" and ei.value.code == 101
    assert ei.value.inserted == k0 and h.num_events() == k0
    assert np.array_equal(ei.value.ids, c.ids[:k0])
    # a bad signature in the prefix comes first
    r = c.r.copy()
    r[40, 5] ^= 2
    h = _hg(c)
    with pytest.raises(HgxError) as ei:
        h.insert_bodies(c.columns(op=op, r=r))
    assert ei.value.msg == "Invalid signature" and ei.value.inserted == 40
