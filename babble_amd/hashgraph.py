"""Python mirror of the reference's hashgraph.Hashgraph API over libhgx's C ABI.

Reference: datatypevoid/babble v0.2.0 hashgraph/hashgraph.go. Method names follow
the Go API (InsertEvent, DivideRounds, DecideFame, FindOrder, Round, Witness,
StronglySee, ...) with the same argument meaning and the same error strings
(raised as babble_amd._lib.HgxError). Events are addressed by dense ids (gid, in
insertion order) -- the cgo shim described in INTEGRATION.md maps Go hex ids to
these. All computation happens in the HIP kernels of libhgx.so; this module only
marshals arrays.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import HgxError, hgx_error, hgx_events, ptr

UNKNOWN_PARENT = -2


def compact_columns(t) -> dict:
    """hgx_events32 columns of a trace (include/hgx.h): int32 Index and parents, the coin byte
    (middleBit: byte 16 of the event id is not 0, hashgraph.go:1039-1048) instead of the id, and
    len(Transactions) with -1 for nil. What a caller builds instead of the wide columns."""
    ntx = np.where(np.asarray(t.txnil) != 0, -1, np.asarray(t.ntx)).astype(np.int32)
    return dict(creator=np.ascontiguousarray(t.creator, np.int32), index=np.ascontiguousarray(t.index, np.int32),
                sp=np.ascontiguousarray(t.sp, np.int32), op=np.ascontiguousarray(t.op, np.int32),
                ts=np.ascontiguousarray(t.ts, np.int64),
                coin=np.ascontiguousarray(np.asarray(t.hash)[:, 16] != 0, np.uint8),
                s=np.ascontiguousarray(t.s, np.uint8), ntx=ntx)


class HostBuffer:
    """One page-locked host allocation (hgx_host_alloc), freed with the object. `.array` is a numpy
    view over it; the caller keeps the HostBuffer alive while the view is in use."""

    def __init__(self, shape, dtype):
        dt = np.dtype(dtype)
        nbytes = max(1, int(np.prod(shape)) * dt.itemsize)
        self._L = _lib.lib()
        self.p = self._L.hgx_host_alloc(nbytes)
        if not self.p:
            raise MemoryError(f"hgx_host_alloc({nbytes}) failed")
        raw = (C.c_uint8 * nbytes).from_address(self.p)
        self.array = np.frombuffer(raw, dtype=np.uint8)[:int(np.prod(shape)) * dt.itemsize].view(dt).reshape(shape)

    def __del__(self):
        p, self.p = getattr(self, "p", None), None
        if p:
            self.array = None
            self._L.hgx_host_free(p)


def pinned_columns(cols: dict) -> dict:
    """The same columns copied into page-locked host memory (hgx_host_alloc), as a caller that keeps
    its sync buffers there hands them over. The returned dict holds the buffers under "_buffers"."""
    out, bufs = {}, []
    for k, v in cols.items():
        if isinstance(v, np.ndarray):
            b = HostBuffer(v.shape, v.dtype)
            b.array[...] = v
            bufs.append(b)
            out[k] = b.array
        else:
            out[k] = v
    out["_buffers"] = bufs
    return out


def pack_columns(cols: dict, base: int) -> dict:
    """hgx_events_packed columns (include/hgx.h) of compact_columns() whose first event gets gid
    `base` (hgx_num_events of the context it goes into): creator as u16, each parent as its
    distance back (0 = "", 0xFFFF = the exception list), built by libhgx's hgx_pack_events32. The
    payload columns are shared with `cols`."""
    L = _lib.lib()
    m = len(cols["creator"])
    _, ev = _events32_of(cols, 0, m)
    out = dict(creator16=np.empty(m, np.uint16), sp_back=np.empty(m, np.uint16), op_back=np.empty(m, np.uint16))
    cap = max(16, m // 64)
    while True:
        x = dict(exc_pos=np.empty(cap, np.int64), exc_sp=np.empty(cap, np.int32), exc_op=np.empty(cap, np.int32))
        n_exc = C.c_int64(0)
        err = hgx_error()
        rc = L.hgx_pack_events32(C.byref(ev), m, base, ptr(out["creator16"]), ptr(out["sp_back"]),
                                 ptr(out["op_back"]), ptr(x["exc_pos"]), ptr(x["exc_sp"]), ptr(x["exc_op"]), cap,
                                 C.byref(n_exc), C.byref(err))
        if rc == 0:
            break
        if n_exc.value <= cap:
            _lib.check(rc, err)
        cap = n_exc.value
    k = n_exc.value
    out.update({nm: np.ascontiguousarray(v[:k]) for nm, v in x.items()})
    out.update(index=cols["index"], ts=cols["ts"], coin=cols["coin"], s=cols["s"], ntx=cols["ntx"])
    return out


def _events32_of(cols: dict, lo: int, hi: int):
    a = {k: v[lo:hi] for k, v in cols.items()}
    return a, _lib.hgx_events32(*[ptr(a[k]) for k in ("creator", "index", "sp", "op", "ts", "coin", "s", "ntx")])


def body_columns(creator, index, sp, op, ts, r, s, txs) -> dict:
    """hgx_event_bodies columns (include/hgx.h) of a batch: the DAG fields, the signatures' R and S
    (32 bytes big-endian each) and txs[k] = Body.Transactions of event k (None for nil, else a list of
    byte strings). r = s = None: events still to be signed (Hashgraph.sign_insert_event_bodies), both
    columns zero."""
    if r is None:
        r = np.zeros((len(txs), 32), np.uint8)
    if s is None:
        s = np.zeros((len(txs), 32), np.uint8)
    ntx = np.fromiter((-1 if t is None else len(t) for t in txs), np.int32, count=len(txs))
    flat = [b for t in txs if t for b in t]
    tx_off = np.zeros(len(flat) + 1, np.int64)
    np.cumsum(np.fromiter((len(b) for b in flat), np.int64, count=len(flat)), out=tx_off[1:])
    return dict(creator=np.ascontiguousarray(creator, np.int32), index=np.ascontiguousarray(index, np.int64),
                sp=np.ascontiguousarray(sp, np.int64), op=np.ascontiguousarray(op, np.int64),
                ts=np.ascontiguousarray(ts, np.int64), r=np.ascontiguousarray(r, np.uint8).reshape(-1, 32),
                s=np.ascontiguousarray(s, np.uint8).reshape(-1, 32), ntx=ntx, tx_off=tx_off,
                tx_bytes=np.frombuffer(b"".join(flat) + b"\0", np.uint8))


def _event_bodies_of(cols: dict, lo: int, hi: int):
    """The hgx_event_bodies of events [lo, hi) (tx_off starts at the slice's first transaction)."""
    a = {k: np.ascontiguousarray(cols[k][lo:hi]) for k in ("creator", "index", "sp", "op", "ts", "r", "s", "ntx")}
    first = int(np.maximum(cols["ntx"][:lo], 0).sum())
    a["tx_off"] = np.ascontiguousarray(cols["tx_off"][first:])
    a["tx_bytes"] = cols["tx_bytes"]
    return a, _lib.hgx_event_bodies(*[ptr(a[k]) for k in ("creator", "index", "sp", "op", "ts", "r", "s", "ntx",
                                                          "tx_off", "tx_bytes")])


_WIRE_BODY_FIELDS = ("creator_id", "index", "self_parent_index", "other_parent_creator", "other_parent_index",
                     "timestamp_ns", "sig_r", "sig_s", "ntx", "tx_off", "tx_bytes")


def wire_body_columns(rows: dict, r, txs) -> dict:
    """hgx_wire_bodies columns (include/hgx.h) from DiffWire rows (creator_id, index, self_parent_index,
    other_parent_creator, other_parent_index, timestamp_ns, sig_s: any mapping with these names), the
    signatures' R (32 bytes big-endian each) and txs[k] = Body.Transactions of row k (None for nil,
    else a list of byte strings): a SyncResponse as the peer decodes it."""
    b = body_columns(rows["creator_id"], rows["index"], rows["self_parent_index"], rows["other_parent_index"],
                     rows["timestamp_ns"], r, rows["sig_s"], txs)
    return dict(creator_id=b["creator"], index=b["index"], self_parent_index=b["sp"],
                other_parent_creator=np.ascontiguousarray(rows["other_parent_creator"], np.int32),
                other_parent_index=b["op"], timestamp_ns=b["ts"], sig_r=b["r"], sig_s=b["s"], ntx=b["ntx"],
                tx_off=b["tx_off"], tx_bytes=b["tx_bytes"])


def _wire_bodies_of(cols: dict, lo: int, hi: int):
    """The hgx_wire_bodies of events [lo, hi) (tx_off starts at the slice's first transaction)."""
    a = {k: np.ascontiguousarray(cols[k][lo:hi]) for k in _WIRE_BODY_FIELDS[:9]}
    first = int(np.maximum(cols["ntx"][:lo], 0).sum())
    a["tx_off"] = np.ascontiguousarray(cols["tx_off"][first:])
    a["tx_bytes"] = cols["tx_bytes"]
    return a, _lib.hgx_wire_bodies(*[ptr(a[k]) for k in _WIRE_BODY_FIELDS])


def event_json_batch(cols: dict, keys65, sp_id32, op_id32, device: int = 0, out_cap: Optional[int] = None):
    """Event.Marshal bytes of body_columns() events whose parents' ids the caller supplies
    (hgx_event_json_batch). Returns (data, offsets): event k's text is data[offsets[k]:offsets[k+1]].
    out_cap = 0 sizes only (data is empty); a smaller out_cap than the text needs raises HgxError with
    .offsets filled."""
    L = _lib.lib()
    m = len(cols["creator"])
    _, ev = _event_bodies_of(cols, 0, m)
    keys = np.ascontiguousarray(keys65, np.uint8).reshape(-1, 65)
    spi = np.ascontiguousarray(sp_id32, np.uint8).reshape(-1, 32)
    opi = np.ascontiguousarray(op_id32, np.uint8).reshape(-1, 32)
    offsets = np.zeros(m + 1, np.int64)

    def call(out, cap):
        err = hgx_error()
        rc = L.hgx_event_json_batch(device, C.byref(ev), m, ptr(keys), len(keys), ptr(spi), ptr(opi),
                                    ptr(out) if out is not None else None, cap, ptr(offsets), C.byref(err))
        if rc:
            e = HgxError(int(err.code or rc), err.msg.decode(errors="replace"))
            e.offsets = offsets
            raise e

    if out_cap is None:
        call(None, 0)
        out_cap = int(offsets[m])
    elif out_cap == 0:
        call(None, 0)
        return np.zeros(0, np.uint8), offsets
    out = np.zeros(max(out_cap, 1), np.uint8)
    call(out, out_cap)
    return out[:int(offsets[m])], offsets


def block_hash_batch(blocks, device: int = 0) -> List[bytes]:
    """Block.Hash of every (round_received, txs, tx_nil) of `blocks` on the device (hgx_block_hash_batch, the
    block encoder alone): txs a list of byte strings; null is printed for tx_nil and no transactions."""
    blocks = list(blocks)
    rr = np.asarray([b[0] for b in blocks], np.int64)
    ntx = np.asarray([len(b[1]) for b in blocks], np.int32)
    nil = np.asarray([1 if b[2] else 0 for b in blocks], np.int32)
    flat = [t for b in blocks for t in b[1]]
    off = np.zeros(len(flat) + 1, np.int64)
    np.cumsum([len(t) for t in flat], out=off[1:])
    by = np.frombuffer(b"".join(flat) + b"\0", np.uint8)
    out, err = np.zeros((max(len(blocks), 1), 32), np.uint8), hgx_error()
    rc = _lib.lib().hgx_block_hash_batch(device, ptr(rr) if len(blocks) else None, ptr(ntx) if len(blocks) else None,
                                         ptr(nil) if len(blocks) else None, ptr(off), ptr(by), len(blocks), ptr(out),
                                         C.byref(err))
    _lib.check(rc, err)
    return [out[k].tobytes() for k in range(len(blocks))]


def batch_levels(sp, op, base: int = 0):
    """Each event's depth inside a batch whose first event gets gid `base` (hgx_batch_levels, host
    only): returns (level [count] int32, number of levels)."""
    sp = np.ascontiguousarray(sp, np.int64)
    op = np.ascontiguousarray(op, np.int64)
    level = np.zeros(len(sp), np.int32)
    nl = C.c_int32(0)
    err = hgx_error()
    rc = _lib.lib().hgx_batch_levels(ptr(sp), ptr(op), len(sp), base, ptr(level), C.byref(nl), C.byref(err))
    _lib.check(rc, err)
    return level, nl.value


class Hashgraph:
    """One context = NewHashgraph(participants, NewInmemStore(participants, cap)) (hashgraph.go:39-66).

    n_graphs > 1 makes a batched context of independent hashgraphs (graph g owns
    participant ids g*n .. g*n+n-1); per-graph getters take `graph`.
    """

    def __init__(self, n_participants: int, capacity: int = 1 << 16, device: int = 0, n_graphs: int = 1,
                 shard_devices: Optional[Sequence[int]] = None):
        """shard_devices: one graph whose round recurrence is chain-sharded over these devices
        (hgx_create_sharded; shard 0 on shard_devices[0], ordinals may repeat)."""
        self.L = _lib.lib()
        self.n = n_participants
        self.G = n_graphs
        err = hgx_error()
        if shard_devices is not None:
            if n_graphs != 1:
                raise ValueError("a chain-sharded context holds one graph")
            devs = np.ascontiguousarray(list(shard_devices), np.int32)
            self.ctx = self.L.hgx_create_sharded(n_participants, capacity, len(devs), ptr(devs), C.byref(err))
        else:
            self.ctx = self.L.hgx_create_batch(n_graphs, n_participants, capacity, device, C.byref(err))
        if not self.ctx:
            raise HgxError(err.code, err.msg.decode(errors="replace"))
        self.capacity = capacity

    def close(self):
        if getattr(self, "ctx", None):
            self.L.hgx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ inserts
    def _insert_call(self, fn, *args) -> int:
        """fn(ctx, *args, &n_inserted, &err): returns n_inserted; raises HgxError with .inserted = the
        events inserted before the first rejected one, or the error a commit callback raised inside the
        call."""
        err = hgx_error()
        n_ins = C.c_int64(0)
        self._cb_error = None
        rc = fn(self.ctx, *args, C.byref(n_ins), C.byref(err))
        if rc:
            e = HgxError(int(err.code or rc), err.msg.decode(errors="replace"))
            e.inserted = n_ins.value
            raise e
        cb_err, self._cb_error = getattr(self, "_cb_error", None), None
        if cb_err is not None:
            raise cb_err
        return n_ins.value

    @staticmethod
    def _events_of(creator, index, sp, op, ts, hash32, s32, ntx, txnil):
        """The hgx_events struct over contiguous copies of the columns (returned first: they must outlive it)."""
        a = [np.ascontiguousarray(creator, np.int32), np.ascontiguousarray(index, np.int64),
             np.ascontiguousarray(sp, np.int64), np.ascontiguousarray(op, np.int64), np.ascontiguousarray(ts, np.int64),
             np.ascontiguousarray(hash32, np.uint8), np.ascontiguousarray(s32, np.uint8),
             np.ascontiguousarray(ntx, np.int32), np.ascontiguousarray(txnil, np.int32)]
        return a, hgx_events(*[ptr(x) for x in a])

    def _trace_events(self, t, lo: int, hi: int):
        sl = slice(lo, hi)
        return self._events_of(t.creator[sl], t.index[sl], t.sp[sl], t.op[sl], t.ts[sl], t.hash[sl], t.s[sl], t.ntx[sl],
                               t.txnil[sl])

    def insert_arrays(self, creator, index, sp, op, ts, hash32, s32, ntx, txnil) -> int:
        """Bulk InsertEvent(e, true) in order; raises HgxError on the first rejected event."""
        a, ev = self._events_of(creator, index, sp, op, ts, hash32, s32, ntx, txnil)
        return self._insert_call(self.L.hgx_insert_events, C.byref(ev), int(a[0].shape[0]))

    def set_participant_keys(self, keys65):
        """Participants' public keys (C x 65 bytes, participant id order) for Event.Verify."""
        k = np.ascontiguousarray(keys65, np.uint8).reshape(-1, 65)
        self._call(lambda ctx, e: self.L.hgx_set_participant_keys(ctx, ptr(k), e))

    def insert_verified(self, t, digest32, r32, lo: int = 0, hi: Optional[int] = None) -> int:
        """InsertEvent with Event.Verify (hgx_insert_events_verified): events [lo, hi) of a trace,
        their body digests and signature R (S = the trace's S column). Raises HgxError on the first
        rejected event, with .inserted = events inserted before it."""
        hi = t.E if hi is None else hi
        a, ev = self._trace_events(t, lo, hi)
        d = np.ascontiguousarray(np.asarray(digest32)[lo:hi], np.uint8)
        r = np.ascontiguousarray(np.asarray(r32)[lo:hi], np.uint8)
        return self._insert_call(self.L.hgx_insert_events_verified, C.byref(ev), ptr(d), ptr(r), hi - lo)

    def insert_bodies(self, cols: dict, lo: int = 0, hi: Optional[int] = None, other_parent_ids=None) -> np.ndarray:
        """InsertEvent with Event.Hash and Event.Verify computed on the device from the events' fields
        (hgx_insert_event_bodies): events [lo, hi) of body_columns(). Returns the events' ids
        [(hi - lo), 32]. Raises HgxError on the first rejected event, with .inserted = events inserted
        before it and .ids = their ids. other_parent_ids (hgx_insert_event_bodies_ext): [len(cols), 32]
        ids, read for the events whose other-parent is ROOT_OTHER on a context with root ids."""
        hi = len(cols["creator"]) if hi is None else hi
        a, ev = _event_bodies_of(cols, lo, hi)
        ids = np.zeros((hi - lo, 32), np.uint8)
        try:
            if other_parent_ids is None:
                self._insert_call(self.L.hgx_insert_event_bodies, C.byref(ev), hi - lo, ptr(ids))
            else:
                opi = np.ascontiguousarray(np.asarray(other_parent_ids, np.uint8).reshape(-1, 32)[lo:hi])
                assert opi.shape[0] == hi - lo
                self._insert_call(self.L.hgx_insert_event_bodies_ext, C.byref(ev), ptr(opi), hi - lo, ptr(ids))
        except HgxError as e:
            e.ids = ids[:e.inserted]
            raise
        return ids

    def insert_bodies_claimed(self, cols: dict, ids, other_parent_id32=None, lo: int = 0, hi: Optional[int] = None) -> int:
        """InsertEvent for events that come with their ids (hgx_insert_event_bodies_claimed): events
        [lo, hi) of body_columns() and ids [len(cols), 32], their claimed ids. One flat hash pass on the
        device proves every claimed id; Event.Verify and the insert follow as in insert_bodies. Returns
        the number inserted. Raises HgxError on the first rejected event or the first claimed id that is
        not its event's hash, with .inserted = events inserted before it."""
        hi = len(cols["creator"]) if hi is None else hi
        a, ev = _event_bodies_of(cols, lo, hi)
        cl = np.ascontiguousarray(np.asarray(ids, np.uint8).reshape(-1, 32)[lo:hi])
        assert cl.shape[0] == hi - lo
        opi = None
        if other_parent_id32 is not None:
            opi = np.ascontiguousarray(np.asarray(other_parent_id32, np.uint8).reshape(-1, 32)[lo:hi])
            assert opi.shape[0] == hi - lo
        return self._insert_call(self.L.hgx_insert_event_bodies_claimed, C.byref(ev), ptr(cl),
                                 None if opi is None else ptr(opi), hi - lo)

    # ------------------------------------------------------------------ the event-id index
    def KeepIdIndex(self):
        """hgx_keep_id_index: from here on the context keeps an index of its events' ids in device memory
        (16 to 32 bytes per event of capacity), built now from the events it already holds. Idempotent."""
        self._call(lambda ctx, e: self.L.hgx_keep_id_index(ctx, e))

    def IdIndexState(self) -> dict:
        """hgx_id_index_state: kept (0 off, 1 valid, 2 kept but invalid: ids not known), slots, entries,
        total_displacement (sum of (slot - home) mod slots) and wrapped (entries below their home slot)."""
        out = (C.c_int64 * 5)()
        self._call(lambda ctx, e: self.L.hgx_id_index_state(ctx, out, e))
        return dict(zip(("kept", "slots", "entries", "total_displacement", "wrapped"), (int(x) for x in out)))

    def FindEvents(self, ids) -> np.ndarray:
        """hgx_find_events: Store.GetEvent's lookup for a batch of 32-byte ids [m, 32]: each id's gid, or
        -1 where no resident event has it (the lowest gid where several do)."""
        q = np.ascontiguousarray(np.asarray(ids, np.uint8).reshape(-1, 32))
        out = np.full(q.shape[0], -1, np.int64)
        self._call(lambda ctx, e: self.L.hgx_find_events(ctx, ptr(q), q.shape[0], ptr(out), e))
        return out

    def insert_events_by_id(self, cols: dict, ids, sp_ids, op_ids, flags, lo: int = 0, hi: Optional[int] = None):
        """hgx_insert_events_by_id: insert_bodies_claimed for events whose parents are given as ids: events
        [lo, hi) of body_columns() (their sp / op columns are not read), ids / sp_ids / op_ids
        [len(cols), 32] and flags [len(cols)] (bit 0: a self-parent, bit 1: an other-parent; sp_ids / op_ids
        may be None where no flag names them). Returns (n_inserted, sp, op), the parents as the device
        resolved them. Raises HgxError as insert_bodies_claimed does, with .inserted, .sp and .op."""
        hi = len(cols["creator"]) if hi is None else hi
        m = hi - lo
        a, ev = _event_bodies_of(cols, lo, hi)

        def rows(x):
            if x is None:
                return None
            r = np.ascontiguousarray(np.asarray(x, np.uint8).reshape(-1, 32)[lo:hi])
            assert r.shape[0] == m
            return r
        cl, spi, opi = rows(ids), rows(sp_ids), rows(op_ids)
        fl = np.ascontiguousarray(np.asarray(flags, np.uint8)[lo:hi])
        assert fl.shape[0] == m
        sp, op = np.zeros(m, np.int64), np.zeros(m, np.int64)
        try:
            n = self._insert_call(self.L.hgx_insert_events_by_id, C.byref(ev), ptr(cl),
                                  None if spi is None else ptr(spi), None if opi is None else ptr(opi), ptr(fl), m,
                                  ptr(sp), ptr(op))
        except HgxError as e:
            e.sp, e.op = sp, op
            raise
        return n, sp, op

    def set_signing_keys(self, priv32):
        """The private keys Event.Sign uses here (hgx_set_signing_keys): C x 32 bytes (big-endian d),
        participant id order, 32 zero bytes = no key for that participant; None clears. Needs
        set_participant_keys first; every key must match its participant's public key."""
        k = None if priv32 is None else np.ascontiguousarray(priv32, np.uint8).reshape(-1, 32)
        if k is not None and k.shape[0] != self.G * self.n:
            raise ValueError("one private key per participant")
        self._call(lambda ctx, e: self.L.hgx_set_signing_keys(ctx, None if k is None else ptr(k), e))

    def sign_insert_event_bodies(self, cols: dict, other_parent_id32=None):
        """Core.SignAndInsertSelfEvent for a batch (hgx_sign_insert_event_bodies): the events of
        body_columns(..., r=None, s=None, ...) are signed on the device under their creators' signing
        keys, hashed, verified and inserted. Returns (r, s, ids, n_inserted). Raises like insert_bodies:
        HgxError with .inserted and the prefix's .r / .s / .ids."""
        m = len(cols["creator"])
        a = dict(cols, r=np.zeros((m, 32), np.uint8), s=np.zeros((m, 32), np.uint8))
        keep, ev = _event_bodies_of(a, 0, m)
        ev.sig_r = ev.sig_s = None   # (ignored by the call)
        r, s, ids = (np.zeros((m, 32), np.uint8) for _ in range(3))
        opi = None
        if other_parent_id32 is not None:
            opi = np.ascontiguousarray(np.asarray(other_parent_id32, np.uint8).reshape(-1, 32))
            assert opi.shape[0] == m
        try:
            k = self._insert_call(self.L.hgx_sign_insert_event_bodies, C.byref(ev), None if opi is None else ptr(opi), m,
                                  ptr(r), ptr(s), ptr(ids))
        except HgxError as e:
            e.r, e.s, e.ids = r[:e.inserted], s[:e.inserted], ids[:e.inserted]
            raise
        return r, s, ids, k

    def insert_verified_device(self, dt: "DeviceTrace", d_digest, d_r, lo: int = 0, hi: Optional[int] = None) -> int:
        """The same with every column resident in HBM (d_digest / d_r: device addresses of 32-byte rows)."""
        hi = dt.E if hi is None else hi
        ev = dt.events(lo, hi)
        return self._insert_call(self.L.hgx_insert_events_verified_device, C.byref(ev),
                                 C.c_void_p(int(d_digest) + 32 * lo), C.c_void_p(int(d_r) + 32 * lo), hi - lo)

    def insert_wire(self, creator_id, index, sp_index, op_creator, op_index, ts, hash32, s32, ntx, txnil) -> int:
        """Core.Sync's loop over WireEvents (hgx_insert_wire_events): ReadWireInfo + InsertEvent(e, false)
        per event; on the first error raises HgxError with .inserted = events inserted before it."""
        a = [np.ascontiguousarray(creator_id, np.int32), np.ascontiguousarray(index, np.int64),
             np.ascontiguousarray(sp_index, np.int64), np.ascontiguousarray(op_creator, np.int32),
             np.ascontiguousarray(op_index, np.int64), np.ascontiguousarray(ts, np.int64),
             np.ascontiguousarray(hash32, np.uint8), np.ascontiguousarray(s32, np.uint8),
             np.ascontiguousarray(ntx, np.int32), np.ascontiguousarray(txnil, np.int32)]
        ev = _lib.hgx_wire_events(*[ptr(x) for x in a])
        return self._insert_call(self.L.hgx_insert_wire_events, C.byref(ev), int(a[0].shape[0]))

    def insert_wire_bodies(self, cols: dict, lo: int = 0, hi: Optional[int] = None):
        """Core.Sync's loop over WireEvents from their wire fields alone (hgx_insert_wire_bodies): events
        [lo, hi) of wire_body_columns(); parents resolved, ids hashed and signatures verified on the device.
        Returns (ids [(hi - lo), 32], self_parent gids, other_parent gids; -1 for ""). On the first error
        raises HgxError with .inserted = events inserted before it and .ids / .self_parent / .other_parent
        = theirs."""
        hi = len(cols["creator_id"]) if hi is None else hi
        a, ev = _wire_bodies_of(cols, lo, hi)
        ids = np.zeros((hi - lo, 32), np.uint8)
        sp = np.full(hi - lo, -1, np.int64)
        op = np.full(hi - lo, -1, np.int64)
        try:
            self._insert_call(self.L.hgx_insert_wire_bodies, C.byref(ev), hi - lo, ptr(ids), ptr(sp), ptr(op))
        except HgxError as e:
            e.ids, e.self_parent, e.other_parent = ids[:e.inserted], sp[:e.inserted], op[:e.inserted]
            raise
        return ids, sp, op

    def insert_device(self, dt: "DeviceTrace", lo: int = 0, hi: Optional[int] = None) -> int:
        """Bulk InsertEvent of a trace already resident in HBM (hgx_insert_events_device)."""
        hi = dt.E if hi is None else hi
        ev = dt.events(lo, hi)
        return self._insert_call(self.L.hgx_insert_events_device, C.byref(ev), hi - lo)

    def clear(self):
        """Forget every event: a fresh NewHashgraph (device allocations kept)."""
        rc = self.L.hgx_clear(self.ctx)
        if rc:
            raise HgxError(rc, "hgx_clear failed")

    def insert_trace(self, t, lo: int = 0, hi: Optional[int] = None) -> int:
        hi = t.E if hi is None else hi
        sl = slice(lo, hi)
        return self.insert_arrays(t.creator[sl], t.index[sl], t.sp[sl], t.op[sl], t.ts[sl], t.hash[sl], t.s[sl],
                                  t.ntx[sl], t.txnil[sl])

    def insert_and_run(self, t, lo: int = 0, hi: Optional[int] = None) -> int:
        """Bootstrap / Core.Sync + RunConsensus in one call (hgx_insert_and_run): events [lo, hi) of a
        trace inserted, then DivideRounds / DecideFame / FindOrder, the payload columns copied to HBM
        while DivideRounds runs. Raises HgxError like insert_trace (.inserted = the accepted prefix)."""
        hi = t.E if hi is None else hi
        a, ev = self._trace_events(t, lo, hi)
        return self._insert_call(self.L.hgx_insert_and_run, C.byref(ev), hi - lo)

    def _events32(self, cols: dict, lo: int, hi: int):
        return _events32_of(cols, lo, hi)

    def insert_events32(self, cols: dict, lo: int = 0, hi: Optional[int] = None) -> int:
        """InsertEvent from the compact columns of compact_columns() (hgx_insert_events32)."""
        hi = len(cols["creator"]) if hi is None else hi
        a, ev = self._events32(cols, lo, hi)
        return self._insert_call(self.L.hgx_insert_events32, C.byref(ev), hi - lo)

    def insert_and_run32(self, cols: dict, lo: int = 0, hi: Optional[int] = None) -> int:
        """insert_and_run from the compact columns (hgx_insert_and_run32: 61 bytes per event)."""
        hi = len(cols["creator"]) if hi is None else hi
        a, ev = self._events32(cols, lo, hi)
        return self._insert_call(self.L.hgx_insert_and_run32, C.byref(ev), hi - lo)

    def _packed_call(self, fn, pk: dict) -> int:
        m = len(pk["creator16"])
        ev = _lib.hgx_events_packed(ptr(pk["creator16"]), ptr(pk["index"]), ptr(pk["sp_back"]), ptr(pk["op_back"]),
                                    len(pk["exc_pos"]), ptr(pk["exc_pos"]), ptr(pk["exc_sp"]), ptr(pk["exc_op"]),
                                    ptr(pk["ts"]), ptr(pk["coin"]), ptr(pk["s"]), ptr(pk["ntx"]))
        return self._insert_call(fn, C.byref(ev), m)

    def insert_events_packed(self, pk: dict) -> int:
        """InsertEvent from pack_columns() output (hgx_insert_events_packed); its base must be
        num_events() now."""
        return self._packed_call(self.L.hgx_insert_events_packed, pk)

    def insert_and_run_packed(self, pk: dict) -> int:
        """insert_and_run from pack_columns() output (hgx_insert_and_run_packed: 10-byte structure
        columns + the 45-byte compact payload)."""
        return self._packed_call(self.L.hgx_insert_and_run_packed, pk)

    def InsertEvent(self, creator: int, index: int, self_parent: int, other_parent: int, timestamp_ns: int,
                    hash32: bytes, s32: bytes, transactions: Optional[Sequence[bytes]]):
        """InsertEvent(event, true) (hashgraph.go:356-401): raises HgxError with the Go error string."""
        txs = [] if transactions is None else list(transactions)
        self.insert_arrays([creator], [index], [self_parent], [other_parent], [timestamp_ns],
                           np.frombuffer(hash32, np.uint8).reshape(1, 32), np.frombuffer(s32, np.uint8).reshape(1, 32),
                           [len(txs)], [1 if transactions is None else 0])

    # ------------------------------------------------------------------ the consensus calls
    def _call(self, fn):
        err = hgx_error()
        self._cb_error = None
        rc = fn(self.ctx, C.byref(err))
        _lib.check(rc, err)
        cb_err, self._cb_error = getattr(self, "_cb_error", None), None
        if cb_err is not None:   # a commit callback raised inside the call: re-raised here
            raise cb_err

    def DivideRounds(self):
        self._call(self.L.hgx_divide_rounds)

    def DecideFame(self):
        self._call(self.L.hgx_decide_fame)

    def FindOrder(self):
        self._call(self.L.hgx_find_order)

    def RunConsensus(self):
        """node/core.go:277-303"""
        self._call(self.L.hgx_run_consensus)

    def save(self, path: str):
        """Checkpoint of the resident events (hgx_save; the BadgerStore's topological event log,
        badger_store.go:309-343). Format: include/hgx.h, babble_amd/checkpoint.py."""
        self._call(lambda ctx, e: self.L.hgx_save(ctx, os.fsencode(path), e))

    def save_bodies(self, path: str):
        """Checkpoint of a context that keeps its event bodies (hgx_save_bodies): a version-3 file with
        every event's R and transactions, the roots' ids and the kept blocks' hashes. Bootstrap of such a
        file proves every id and signature in it and, on a keeping context, restores the body store."""
        self._call(lambda ctx, e: self.L.hgx_save_bodies(ctx, os.fsencode(path), e))

    def save_with_payloads(self, path: str, payloads: Sequence[bytes]):
        """Checkpoint with the caller's per-event bytes (hgx_save_ex), one entry per event
        (ValueError otherwise: hgx_save_ex reads E + 1 offsets and that many blob bytes)."""
        if len(payloads) != self.num_events():
            raise ValueError(f"save_with_payloads: {len(payloads)} payloads for {self.num_events()} events")
        off = np.zeros(len(payloads) + 1, np.int64)
        off[1:] = np.cumsum([len(b) for b in payloads]) if len(payloads) else []
        blob = np.frombuffer(b"".join(payloads) or b"\0", np.uint8).copy()
        self._call(lambda ctx, e: self.L.hgx_save_ex(ctx, os.fsencode(path), ptr(off), ptr(blob), e))

    def event_id(self, gid: int) -> bytes:
        """Event.Hash of an inserted event (hgx_get_event_id)."""
        out = np.zeros(32, np.uint8)
        self._call(lambda ctx, e: self.L.hgx_get_event_id(ctx, gid, ptr(out), e))
        return out.tobytes()

    def event_payload(self, gid: int) -> bytes:
        """The payload a bootstrapped checkpoint stored for the event (hgx_get_event_payload)."""
        ln = C.c_int64(0)
        self._call(lambda ctx, e: self.L.hgx_get_event_payload(ctx, gid, None, 0, C.byref(ln), e))
        out = np.zeros(max(1, ln.value), np.uint8)
        self._call(lambda ctx, e: self.L.hgx_get_event_payload(ctx, gid, ptr(out), ln.value, C.byref(ln), e))
        return out[:ln.value].tobytes()

    def Bootstrap(self, path: str):
        """Hashgraph.Bootstrap (hashgraph.go:1008-1037) from a checkpoint file: replay the events
        in topological order, then DivideRounds / DecideFame / FindOrder once (hgx_bootstrap)."""
        self._call(lambda ctx, e: self.L.hgx_bootstrap(ctx, os.fsencode(path), e))

    def set_commit_callback(self, fn):
        """commitCh (hashgraph.go:848-854): fn(graph, block, rr, first, n_events, n_tx) for every new
        block with transactions, at the end of FindOrder (after the counters are updated); None
        removes it. An exception raised by fn is kept (later blocks are still delivered) and
        re-raised when the FindOrder / RunConsensus call returns."""
        if fn is None:
            self._commit_cb = None
            rc = self.L.hgx_set_commit_callback(self.ctx, None, None)
        else:
            def tramp(_user, g, b, rr, first, nev, ntx):
                try:
                    fn(int(g), int(b), int(rr), int(first), int(nev), int(ntx))
                except BaseException as ex:   # ctypes would print and drop it
                    if getattr(self, "_cb_error", None) is None:
                        self._cb_error = ex
            self._commit_cb = _lib.COMMIT_FN(tramp)   # kept alive while registered
            rc = self.L.hgx_set_commit_callback(self.ctx, C.cast(self._commit_cb, C.c_void_p), None)
        if rc:
            raise HgxError(rc, "hgx_set_commit_callback failed")

    # ------------------------------------------------------------------ Reset / GetFrame
    ROOT_Y, ROOT_OTHER = -3, -4   # other-parent codes after a Reset (hgx.h)

    def Reset(self, root_index, root_round, root_y_is_event, others=None):
        """Hashgraph.Reset(roots) (hashgraph.go:877-895): per participant Root.Index, Root.Round and
        whether Root.Y names an event; `others` = the 32-byte ids of the events the roots' Others
        maps hold (hgx_set_root_others). Then insert with self-parent -1 = Root.X and other-parent
        ROOT_Y / ROOT_OTHER for parents outside the store."""
        a = [np.ascontiguousarray(x, np.int32) for x in (root_index, root_round, root_y_is_event)]
        err = hgx_error()
        rc = self.L.hgx_reset(self.ctx, *[ptr(x) for x in a], C.byref(err))
        _lib.check(rc, err)
        if others is not None and len(others):
            k = np.ascontiguousarray(others, np.uint8).reshape(-1, 32)
            self._call(lambda ctx, e: self.L.hgx_set_root_others(ctx, ptr(k), k.shape[0], e))

    def SetRootIds(self, x, y, others=()):
        """The ids of the roots installed by Reset (hgx_set_root_ids): x[p] / y[p] = the 32-byte id of
        participant p's Root.X / Root.Y (None for ""), others = (event id, other-parent id) pairs of
        the roots' Others maps. Afterwards GetRootIds / GetRootOthers answer and insert_bodies works."""
        C_ = self.n * self.G
        cols = []
        for v in (x, y):
            has = np.asarray([0 if b is None else 1 for b in v], np.int32)
            ids = np.zeros((C_, 32), np.uint8)
            for p, b in enumerate(v):
                if b is not None:
                    ids[p] = np.frombuffer(bytes(b), np.uint8)
            cols += [ids, has]
        others = list(others)
        ke = np.frombuffer(b"".join(bytes(k) for k, _ in others) + bytes(32), np.uint8)
        kv = np.frombuffer(b"".join(bytes(v) for _, v in others) + bytes(32), np.uint8)
        self._call(lambda ctx, e: self.L.hgx_set_root_ids(ctx, ptr(cols[0]), ptr(cols[1]), ptr(cols[2]), ptr(cols[3]),
                                                          ptr(ke), ptr(kv), len(others), e))

    def GetFrame(self):
        """Hashgraph.GetFrame (hashgraph.go:897-995): roots (x, y, index, round per participant),
        events (gids, topological order), others {event: other-parent}."""
        C_ = self.n * self.G
        ne, no = C.c_int64(), C.c_int64()
        rx, ry = np.zeros(C_, np.int64), np.zeros(C_, np.int64)
        ri, rr = np.zeros(C_, np.int32), np.zeros(C_, np.int32)
        err = hgx_error()
        cap = self.num_events() + 1
        ev = np.zeros(cap, np.int64)
        oe, op = np.zeros(cap, np.int64), np.zeros(cap, np.int64)
        rc = self.L.hgx_get_frame(self.ctx, ptr(ev), cap, C.byref(ne), ptr(rx), ptr(ry), ptr(ri), ptr(rr), ptr(oe),
                                  ptr(op), cap, C.byref(no), C.byref(err))
        _lib.check(rc, err)
        return dict(roots=[(int(rx[p]), int(ry[p]), int(ri[p]), int(rr[p])) for p in range(C_)],
                    events=[int(x) for x in ev[:ne.value]],
                    others={int(oe[k]): int(op[k]) for k in range(no.value)})

    def PruneToFrame(self) -> np.ndarray:
        """The resident hashgraph cut down to its last frame on the device (hgx_prune_to_frame):
        GetFrame, Reset(frame roots) and the re-insert of the frame's events in one call, with no
        event crossing PCIe. Returns old_gid: the old gid of each new gid. RunConsensus next."""
        nk = C.c_int64()
        old = np.zeros(max(1, self.num_events()), np.int64)
        self._call(lambda ctx, e: self.L.hgx_prune_to_frame(ctx, ptr(old), old.size, C.byref(nk), e))
        return old[:nk.value].copy()

    def get_frame_bodies_raw(self, arrays: dict, events_cap=0, others_cap=0, tx_cap=0, bytes_cap=0):
        """One bare hgx_get_frame_bodies call: arrays = {hgx_frame_out column: numpy array} (a column
        left out is NULL). Returns (rc, error, (n_events, n_others, n_tx, n_bytes)); nothing is raised."""
        out = _lib.hgx_frame_out()
        for nm, a in arrays.items():
            setattr(out, nm, ptr(a))
        out.events_cap, out.others_cap, out.tx_cap, out.bytes_cap = events_cap, others_cap, tx_cap, bytes_cap
        cnt = [C.c_int64() for _ in range(4)]
        err = hgx_error()
        rc = self.L.hgx_get_frame_bodies(self.ctx, C.byref(out), *[C.byref(x) for x in cnt], C.byref(err))
        return rc, err, tuple(int(x.value) for x in cnt)

    def GetFrameBodies(self, bodies: bool = True) -> dict:
        """Hashgraph.GetFrame complete, for serving a fast-forward (hgx_get_frame_bodies): the frame
        PruneToFrame would keep at this moment, and nothing changes. A sizing call, then the fill.
        Returns the event columns of hgx_frame_out as numpy arrays in frame order (with bodies: sig_r,
        tx_off and tx_bytes too), `roots` = dict(Index, Round, X, Y) per participant (None for "") and
        `others` = the roots' Others pairs (event id, other-parent id) sorted by event id."""
        C_ = self.n * self.G
        spec = dict(_lib.FRAME_OUT_FIELDS)
        want = [nm for nm in _lib.FRAME_EVENT_COLUMNS if bodies or nm != "sig_r"]
        sizing = {"sig_r": np.zeros((1, 32), np.uint8)} if bodies else {}   # (a body column makes the body totals count)
        rc, err, (ne, no, nt, nb) = self.get_frame_bodies_raw(sizing)
        if rc not in (0, 103):
            _lib.check(rc, err)
        arr = {nm: np.zeros((C_,) + spec[nm][1], spec[nm][0]) for nm in _lib.FRAME_ROOT_COLUMNS}
        arr.update({nm: np.zeros((max(1, no),) + spec[nm][1], spec[nm][0]) for nm in _lib.FRAME_OTHERS_COLUMNS})
        arr.update({nm: np.zeros((max(1, ne),) + spec[nm][1], spec[nm][0]) for nm in want})
        if bodies:
            arr["tx_off"] = np.zeros(nt + 1, np.int64)
            arr["tx_bytes"] = np.zeros(max(1, nb), np.uint8)
        rc, err, got = self.get_frame_bodies_raw(arr, ne, no, nt, nb)
        _lib.check(rc, err)
        assert got == (ne, no, nt, nb)
        res = {nm: arr[nm][:ne] for nm in want}
        if bodies:
            res["tx_off"], res["tx_bytes"] = arr["tx_off"], arr["tx_bytes"][:nb]
        res["roots"] = [dict(Index=int(arr["root_index"][p]), Round=int(arr["root_round"][p]),
                             X=arr["root_x_id32"][p].tobytes() if arr["root_has_x"][p] else None,
                             Y=arr["root_y_id32"][p].tobytes() if arr["root_has_y"][p] else None) for p in range(C_)]
        res["others"] = [(arr["others_event_id32"][j].tobytes(), arr["others_parent_id32"][j].tobytes())
                         for j in range(no)]
        return res

    def GetRootIds(self, participant: int) -> dict:
        """The 32-byte ids of the participant's Root.X and Root.Y (None for ""), known while every
        root traces back to genesis through PruneToFrame (hgx_get_root_ids)."""
        x, y = np.zeros(32, np.uint8), np.zeros(32, np.uint8)
        hx, hy = C.c_int32(), C.c_int32()
        self._call(lambda ctx, e: self.L.hgx_get_root_ids(ctx, participant, ptr(x), C.byref(hx), ptr(y), C.byref(hy), e))
        return dict(X=x.tobytes() if hx.value else None, Y=y.tobytes() if hy.value else None)

    def GetRootOthers(self) -> List[tuple]:
        """The roots' Others pairs (event id, other-parent id), sorted by event id (hgx_get_root_others)."""
        cnt = C.c_int64()
        self._call(lambda ctx, e: self.L.hgx_get_root_others(ctx, None, None, 0, C.byref(cnt), e))
        k, v = np.zeros((max(1, cnt.value), 32), np.uint8), np.zeros((max(1, cnt.value), 32), np.uint8)
        self._call(lambda ctx, e: self.L.hgx_get_root_others(ctx, ptr(k), ptr(v), cnt.value, C.byref(cnt), e))
        return [(k[j].tobytes(), v[j].tobytes()) for j in range(cnt.value)]

    # ------------------------------------------------------------------ row-sharded graph
    def set_shard(self, rank: int, world: int):
        """One graph row-sharded over `world` ranks (hgx_set_shard)."""
        if self.L.hgx_set_shard(self.ctx, rank, world) != 0:
            raise ValueError("invalid shard")
        self.shard = (rank, world)

    def FindOrderSharded(self, all_gather):
        """FindOrder of a row-sharded graph: begin, exchange of the shards' consensus timestamps,
        end. all_gather(local: np.ndarray[int64], counts: list[int]) -> list of every rank's
        array (torch.distributed over gloo, or over RCCL with device buffers)."""
        rank, world = self.shard
        self._call(self.L.hgx_find_order_begin)
        counts = [int(self.L.hgx_shard_values(self.ctx, r)) for r in range(world)]
        mine = np.zeros(counts[rank], np.int64)
        if counts[rank] and self.L.hgx_shard_export(self.ctx, ptr(mine), 0) != 0:
            raise HgxError(200, "hgx_shard_export failed")
        parts = all_gather(mine, counts)
        for r in range(world):
            if r != rank and counts[r]:
                a = np.ascontiguousarray(parts[r], np.int64)
                if self.L.hgx_shard_import(self.ctx, r, ptr(a), 0) != 0:
                    raise HgxError(200, "hgx_shard_import failed")
        self._call(self.L.hgx_find_order_end)

    def RunConsensusSharded(self, all_gather):
        self.DivideRounds()
        self.DecideFame()
        self.FindOrderSharded(all_gather)

    def reset_consensus(self):
        """Fresh consensus state over the same resident events (Bootstrap replay)."""
        rc = self.L.hgx_reset_consensus(self.ctx)
        if rc:
            raise HgxError(rc, "hgx_reset_consensus failed")

    # ------------------------------------------------------------------ state (hashgraph.go:15-37)
    def UndecidedRounds(self, graph: int = 0) -> List[int]:
        k = self.L.hgx_undecided_rounds(self.ctx, graph, None, 0)
        buf = np.zeros(max(k, 1), np.int32)
        self.L.hgx_undecided_rounds(self.ctx, graph, ptr(buf), k)
        return [int(v) for v in buf[:k]]

    def LastConsensusRound(self, graph: int = 0) -> Optional[int]:
        has = C.c_int32(0)
        v = self.L.hgx_last_consensus_round(self.ctx, graph, C.byref(has))
        return int(v) if has.value else None

    def LastCommitedRoundEvents(self, graph: int = 0) -> int:
        return int(self.L.hgx_last_commited_round_events(self.ctx, graph))

    def ConsensusTransactions(self, graph: int = 0) -> int:
        return int(self.L.hgx_consensus_transactions(self.ctx, graph))

    def PendingLoadedEvents(self, graph: int = 0) -> int:
        return int(self.L.hgx_pending_loaded_events(self.ctx, graph))

    def SuperMajority(self) -> int:
        return int(self.L.hgx_super_majority(self.ctx))

    # ------------------------------------------------------------------ Store views
    def LastRound(self, graph: int = 0) -> int:
        return int(self.L.hgx_last_round(self.ctx, graph))

    def RoundEvents(self, r: int, graph: int = 0) -> int:
        return int(self.L.hgx_round_event_count(self.ctx, graph, r))

    def RoundWitnesses(self, r: int, graph: int = 0) -> List[int]:
        buf = np.zeros(self.n, np.int64)
        k = self.L.hgx_round_witnesses(self.ctx, graph, r, ptr(buf), self.n)
        return [int(v) for v in buf[:k]]

    def Known(self, graph: int = 0) -> np.ndarray:
        out = np.zeros(self.n, np.int32)
        self.L.hgx_known(self.ctx, graph, ptr(out))
        return out

    def ConsensusEvents(self, graph: int = 0) -> np.ndarray:
        k = int(self.L.hgx_consensus_events_count(self.ctx, graph))
        out = np.zeros(max(k, 1), np.int64)
        if k:
            rc = self.L.hgx_consensus_events(self.ctx, graph, 0, k, ptr(out))
            if rc:
                raise HgxError(rc, "hgx_consensus_events failed")
        return out[:k]

    def GetBlock(self, rr: int, graph: int = 0) -> dict:
        """Store.GetBlock(rr): the block with that RoundReceived (HgxError "<rr>, Not Found")."""
        b, err = C.c_int64(), hgx_error()
        _lib.check(self.L.hgx_get_block(self.ctx, graph, rr, C.byref(b), C.byref(err)), err)
        return self.Blocks(graph)[b.value]

    def consensus_received(self, graph: int = 0, first: int = 0, count: Optional[int] = None):
        """(gids, round received, consensus timestamps) along the graph's consensus order."""
        k = int(self.L.hgx_consensus_events_count(self.ctx, graph))
        count = k - first if count is None else count
        g = np.zeros(max(count, 1), np.int64)
        rr = np.zeros(max(count, 1), np.int32)
        ts = np.zeros(max(count, 1), np.int64)
        if count:
            rc = self.L.hgx_consensus_received(self.ctx, graph, first, count, ptr(g), ptr(rr), ptr(ts))
            if rc:
                raise HgxError(rc, "hgx_consensus_received failed")
        return g[:count], rr[:count], ts[:count]

    # ------------------------------------------------------------------ Store: events by participant
    def LastFrom(self, participant: int):
        """(gid of the last event or -1, isRoot) (inmem_store.go:85-102)."""
        gid, root, err = C.c_int64(), C.c_int32(), hgx_error()
        _lib.check(self.L.hgx_last_from(self.ctx, participant, C.byref(gid), C.byref(root), C.byref(err)), err)
        return gid.value, bool(root.value)

    def ParticipantEvents(self, participant: int, skip: int) -> List[int]:
        cnt, err = C.c_int64(), hgx_error()
        _lib.check(self.L.hgx_participant_events(self.ctx, participant, skip, None, 0, C.byref(cnt), C.byref(err)),
                   err)
        out = np.zeros(max(cnt.value, 1), np.int64)
        _lib.check(self.L.hgx_participant_events(self.ctx, participant, skip, ptr(out), cnt.value, C.byref(cnt),
                                                 C.byref(err)), err)
        return [int(v) for v in out[:cnt.value]]

    def ParticipantEvent(self, participant: int, index: int) -> int:
        gid, err = C.c_int64(), hgx_error()
        _lib.check(self.L.hgx_participant_event(self.ctx, participant, index, C.byref(gid), C.byref(err)), err)
        return gid.value

    def GetRoot(self, participant: int) -> dict:
        x, y, idx, rnd, err = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int32(), hgx_error()
        _lib.check(self.L.hgx_get_root(self.ctx, participant, C.byref(x), C.byref(y), C.byref(idx), C.byref(rnd),
                                       C.byref(err)), err)
        return dict(X=x.value, Y=y.value, Index=idx.value, Round=rnd.value)

    def GetEvent(self, gid: int) -> dict:
        cr, ix, sp, op, ts, nt, nil, err = (C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64(),
                                            C.c_int32(), C.c_int32(), hgx_error())
        _lib.check(self.L.hgx_get_event(self.ctx, gid, C.byref(cr), C.byref(ix), C.byref(sp), C.byref(op),
                                        C.byref(ts), C.byref(nt), C.byref(nil), C.byref(err)), err)
        return dict(creator=cr.value, index=ix.value, self_parent=sp.value, other_parent=op.value,
                    timestamp=ts.value, ntx=nt.value, tx_nil=bool(nil.value))

    def wire_info(self, first: int = 0, count: Optional[int] = None):
        """SetWireInfo of events [first, first+count): (self-parent index, other-parent creator, other-parent index)."""
        count = self.num_events() - first if count is None else count
        a, b, c = (np.zeros(max(count, 1), np.int32) for _ in range(3))
        if count:
            rc = self.L.hgx_wire_info(self.ctx, first, count, ptr(a), ptr(b), ptr(c))
            if rc:
                raise HgxError(rc, "hgx_wire_info failed")
        return a[:count], b[:count], c[:count]

    def DiffWire(self, known, sync_limit: int = -1, graph: int = 0, cap: Optional[int] = None, columns=None):
        """node.processSyncRequest's OverSyncLimit + Diff + ToWire in one call on the device
        (hgx_diff_wire): the events the peer's `known` vector lacks, in topological order, as the wire
        columns insert_wire takes. Returns (cols, count, over_limit): cols maps hgx_wire_out's column
        names to arrays of min(cap, count) rows (empty when over the limit). cap=None sizes by the count
        (one sizing call with cap=0); columns = the names to request (default: all, without "hash"
        when the context's event ids are not known, which a sizing call with "hash" finds out)."""
        known = np.ascontiguousarray(known, np.int32)
        if known.shape != (self.n,):
            raise ValueError(f"known must have {self.n} entries")
        spec = {nm: (dt, shp) for nm, dt, shp in _lib.WIRE_OUT_COLUMNS}
        want = list(spec) if columns is None else list(columns)
        bad = [nm for nm in want if nm not in spec]
        if bad:
            raise ValueError(f"unknown columns {bad}")
        cnt, over = C.c_int64(0), C.c_int32(0)

        def call(cols, rows):
            out, err = _lib.hgx_wire_out(**{nm: ptr(a) for nm, a in cols.items()}), hgx_error()
            rc = self.L.hgx_diff_wire(self.ctx, graph, ptr(known), sync_limit, C.byref(out), rows, C.byref(cnt),
                                      C.byref(over), C.byref(err))
            return rc, err

        def alloc(rows):
            return {nm: np.zeros((max(rows, 1),) + spec[nm][1], spec[nm][0]) for nm in want}

        if cap is None or columns is None:   # the sizing call: the count, and whether "hash" can be had
            rc, err = call(alloc(0), 0)
            if rc == 102 and columns is None and b"ids are not known" in err.msg:
                want.remove("hash")
                rc, err = call(alloc(0), 0)
            _lib.check(rc, err)
        rows = cnt.value if cap is None else int(cap)
        cols = alloc(rows)
        if not (over.value and cap is None):
            rc, err = call(cols, rows)
            _lib.check(rc, err)
        m = 0 if over.value else min(rows, cnt.value)
        return {nm: a[:m] for nm, a in cols.items()}, cnt.value, bool(over.value)

    # ------------------------------------------------------------------ the resident body store
    def KeepBodies(self, tx_hint: int = 0, bytes_hint: int = 0):
        """hgx_keep_bodies: from here on the body paths keep every accepted event's R and transaction
        bytes on the device (a context with no events only). The hints are a first reservation."""
        err = hgx_error()
        _lib.check(self.L.hgx_keep_bodies(self.ctx, tx_hint, bytes_hint, C.byref(err)), err)

    def BodiesState(self) -> dict:
        """hgx_bodies_state: state 0 off / 1 complete / 2 lost, and the events, transactions and bytes held."""
        ne, nt, nb = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        st = self.L.hgx_bodies_state(self.ctx, C.byref(ne), C.byref(nt), C.byref(nb))
        return dict(state=int(st), events=ne.value, tx=nt.value, bytes=nb.value)

    @staticmethod
    def _sized(call):
        """call(tx_off, tx_cap, tx_bytes, bytes_cap, n_tx, n_bytes) -> (rc, err): the sizing call with
        NULL arrays, then the call with arrays of exactly that size. Returns (tx_off, tx_bytes)."""
        nt, nb = C.c_int64(0), C.c_int64(0)
        rc, err = call(None, 0, None, 0, nt, nb)
        if rc not in (0, 103):   # HGX_ERR_CAPACITY: the totals are set
            _lib.check(rc, err)
        off, by = np.zeros(nt.value + 1, np.int64), np.zeros(max(nb.value, 1), np.uint8)
        rc, err = call(off, nt.value, by, nb.value, nt, nb)
        _lib.check(rc, err)
        return off, by[:nb.value]

    def EventBodies(self, gids) -> dict:
        """hgx_get_event_bodies: R and the transactions of the events `gids` (any order, repeats allowed)
        from the body store, as hgx_event_bodies' columns in list order: sig_r [m, 32], ntx [m] (-1 =
        nil), tx_off [n_tx + 1] from 0, tx_bytes."""
        gids = np.ascontiguousarray(gids, np.int64)
        m = len(gids)
        r, ntx = np.zeros((max(m, 1), 32), np.uint8), np.zeros(max(m, 1), np.int32)

        def call(off, tcap, by, bcap, nt, nb):
            err = hgx_error()
            rc = self.L.hgx_get_event_bodies(self.ctx, ptr(gids) if m else None, m, ptr(r), ptr(ntx),
                                             ptr(off) if off is not None else None, tcap,
                                             ptr(by) if by is not None else None, bcap, C.byref(nt), C.byref(nb),
                                             C.byref(err))
            return rc, err

        off, by = self._sized(call)
        return dict(sig_r=r[:m], ntx=ntx[:m], tx_off=off, tx_bytes=by)

    def BlockTransactions(self, b: int, graph: int = 0) -> List[bytes]:
        """hgx_block_transactions: Block.Transactions of block b from the body store, in consensus order."""
        def call(off, tcap, by, bcap, nt, nb):
            err = hgx_error()
            rc = self.L.hgx_block_transactions(self.ctx, graph, b, ptr(off) if off is not None else None, tcap,
                                               ptr(by) if by is not None else None, bcap, C.byref(nt), C.byref(nb),
                                               C.byref(err))
            return rc, err

        off, by = self._sized(call)
        raw = by.tobytes()
        return [raw[int(off[j]):int(off[j + 1])] for j in range(len(off) - 1)]

    def BlockHash(self, b: int, graph: int = 0) -> bytes:
        """hgx_get_block_hash: Block.Hash of block b, computed on the device when the block was made."""
        out, err = np.zeros(32, np.uint8), hgx_error()
        _lib.check(self.L.hgx_get_block_hash(self.ctx, graph, b, ptr(out), C.byref(err)), err)
        return out.tobytes()

    def DiffWireBodies(self, known, sync_limit: int = -1, graph: int = 0, cap: Optional[int] = None):
        """A complete SyncResponse (hgx_diff_wire_bodies): DiffWire's columns plus sig_r, tx_off and
        tx_bytes of the same rows from the body store. Returns (cols, count, over_limit); with
        ntx = where(tx_nil, -1, ntx) the columns are insert_wire_bodies' on the peer. cap=None sizes by
        the count."""
        known = np.ascontiguousarray(known, np.int32)
        if known.shape != (self.n,):
            raise ValueError(f"known must have {self.n} entries")
        spec = {nm: (dt, shp) for nm, dt, shp in _lib.WIRE_OUT_COLUMNS}
        cnt, over, nt, nb = C.c_int64(0), C.c_int32(0), C.c_int64(0), C.c_int64(0)

        def call(cols, rows, body):
            out, err = _lib.hgx_wire_out(**{nm: ptr(a) for nm, a in cols.items()}), hgx_error()
            rc = self.L.hgx_diff_wire_bodies(self.ctx, graph, ptr(known), sync_limit, C.byref(out),
                                             C.byref(body) if body is not None else None, rows, C.byref(cnt),
                                             C.byref(nt), C.byref(nb), C.byref(over), C.byref(err))
            return rc, err

        def alloc(rows):
            return {nm: np.zeros((max(rows, 1),) + shp, dt) for nm, (dt, shp) in spec.items()}

        if cap is None:   # the row count first
            rc, err = call(alloc(0), 0, None)
            _lib.check(rc, err)
        rows = cnt.value if cap is None else int(cap)
        cols = alloc(rows)
        if over.value and cap is None:
            return {nm: a[:0] for nm, a in cols.items()}, cnt.value, True
        rc, err = call(cols, rows, None)   # the rows' totals (no array is written unless they are zero)
        if rc not in (0, 103):
            _lib.check(rc, err)
        r = np.zeros((max(rows, 1), 32), np.uint8)
        off, by = np.zeros(nt.value + 1, np.int64), np.zeros(max(nb.value, 1), np.uint8)
        body = _lib.hgx_wire_body_out(ptr(r), ptr(off), nt.value, ptr(by), nb.value)
        rc, err = call(cols, rows, body)
        _lib.check(rc, err)
        m = 0 if over.value else min(rows, cnt.value)
        res = {nm: a[:m] for nm, a in cols.items()}
        res.update(sig_r=r[:m], tx_off=off, tx_bytes=by[:nb.value])
        return res, cnt.value, bool(over.value)

    def ReadWireInfo(self, creator: int, sp_index: int, op_creator: int, op_index: int):
        sp, op, err = C.c_int64(), C.c_int64(), hgx_error()
        _lib.check(self.L.hgx_read_wire_info(self.ctx, creator, sp_index, op_creator, op_index, C.byref(sp),
                                             C.byref(op), C.byref(err)), err)
        return sp.value, op.value

    def Blocks(self, graph: int = 0) -> List[dict]:
        res = []
        for b in range(int(self.L.hgx_num_blocks(self.ctx, graph))):
            rr, nev, nil, com = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
            first, ntx = C.c_int64(), C.c_int64()
            self.L.hgx_block_info(self.ctx, graph, b, C.byref(rr), C.byref(first), C.byref(nev), C.byref(ntx),
                                  C.byref(nil), C.byref(com))
            res.append(dict(rr=rr.value, first=first.value, n_events=nev.value, ntx=ntx.value,
                            tx_nil=bool(nil.value), committed=bool(com.value)))
        return res

    # ------------------------------------------------------------------ primitives
    def Ancestor(self, x: int, y: int) -> bool:
        return bool(self.L.hgx_ancestor(self.ctx, x, y))

    def SelfAncestor(self, x: int, y: int) -> bool:
        return bool(self.L.hgx_self_ancestor(self.ctx, x, y))

    def See(self, x: int, y: int) -> bool:
        return bool(self.L.hgx_see(self.ctx, x, y))

    def StronglySee(self, x: int, y: int) -> bool:
        return bool(self.L.hgx_strongly_see(self.ctx, x, y))

    def OldestSelfAncestorToSee(self, x: int, y: int) -> int:
        return int(self.L.hgx_oldest_self_ancestor_to_see(self.ctx, x, y))

    def Round(self, x: int) -> int:
        return int(self.L.hgx_round(self.ctx, x))

    def Witness(self, x: int) -> bool:
        return bool(self.L.hgx_witness(self.ctx, x))

    def coords(self, x: int):
        la = np.zeros(self.n, np.int32)
        fd = np.zeros(self.n, np.int32)
        rc = self.L.hgx_get_coords(self.ctx, x, ptr(la), ptr(fd))
        if rc:
            raise HgxError(rc, "hgx_get_coords failed")
        return la, fd

    # ------------------------------------------------------------------ bulk results
    def num_events(self) -> int:
        return int(self.L.hgx_num_events(self.ctx))

    def rounds(self):
        E = self.num_events()
        rnd = np.zeros(max(E, 1), np.int32)
        wit = np.zeros(max(E, 1), np.int8)
        fam = np.zeros(max(E, 1), np.int8)
        if E:
            rc = self.L.hgx_get_rounds(self.ctx, 0, E, ptr(rnd), ptr(wit), ptr(fam))
            if rc:
                raise HgxError(rc, "hgx_get_rounds failed")
        return rnd[:E], wit[:E], fam[:E]

    def received(self):
        E = self.num_events()
        rr = np.zeros(max(E, 1), np.int32)
        cts = np.zeros(max(E, 1), np.int64)
        if E:
            rc = self.L.hgx_get_received(self.ctx, 0, E, ptr(rr), ptr(cts))
            if rc:
                raise HgxError(rc, "hgx_get_received failed")
        return rr[:E], cts[:E]

    def results(self, graph: int = 0) -> dict:
        """Same shape as tests' oracle results() for parity comparison (single-graph contexts)."""
        rnd, wit, fam = self.rounds()
        rr, cts = self.received()
        return dict(round=rnd, witness=wit, famous=fam, rr=rr, cts=np.where(rr >= 0, cts, 0),
                    order=self.ConsensusEvents(graph), last_round=self.LastRound(graph),
                    undecided=self.UndecidedRounds(graph), lcr=self.LastConsensusRound(graph),
                    lcre=self.LastCommitedRoundEvents(graph), consensus_tx=self.ConsensusTransactions(graph),
                    pending_loaded=self.PendingLoadedEvents(graph), blocks=self.Blocks(graph))

    def phase_times(self):
        out = np.zeros(28, np.float64)
        self.L.hgx_phase_times(self.ctx, ptr(out), 28)
        return dict(coords_ms=out[0], rounds_ms=out[1], fame_ms=out[2], order_ms=out[3],
                    la_sweeps=int(out[4]), rounds=int(out[5]), compact=int(out[6]),
                    la_rows=int(out[7]), rebuild=int(out[8]), r_lo=int(out[9]),
                    la_wave=int(out[10]), la_wave_fallbacks=int(out[11]), la_wave_segs=int(out[12]),
                    round_p_runs=int(out[13]), round_p_fallbacks=int(out[14]), round_p_ovf=int(out[15]),
                    round_p_fail_round=int(out[16]), round_p_fail_chain=int(out[17]),
                    round_g_runs=int(out[18]), la_small=int(out[19]), la_verify=int(out[20]),
                    sort_seg=int(out[21]), ingest_pieces=int(out[22]),
                    host_rounds_ms=out[23], host_fame_ms=out[24], host_order_ms=out[25],
                    payload_end_ms=out[26], cts_row=int(out[27]))

    def set_ingest_pipeline(self, pieces, min_events=4_000_000):
        """insert_and_run of compact columns on an empty context: the structure columns in `pieces`
        pieces, each inserted, laid out and its lastAncestors segments started while the next is
        copied (0: the serial order); batches below min_events stay serial. Same results."""
        if self.L.hgx_set_ingest_pipeline(self.ctx, int(pieces), int(min_events)) != 0:
            raise ValueError(f"invalid ingest pipeline {pieces}, {min_events}")

    def set_fame_tally(self, mode):
        """DecideFame tally: "popc" (default, one lane per voter), "vote" (per-round kernel), "mfma"
        (witness-tiled, int8 MFMA) or "tile" (witness-tiled popcount)."""
        m = {"popc": 0, "vote": 1, "mfma": 2, "tile": 3}[mode] if isinstance(mode, str) else int(mode)
        if self.L.hgx_set_fame_tally(self.ctx, m) != 0:
            raise ValueError(f"invalid fame tally {mode}")

    def set_la_kernel(self, mode):
        """DivideRounds lastAncestors: "wave" (default, one dataflow pass; a small graph's whole
        graph in LDS), "ring" (the dataflow pass without the small-graph form) or "sweep"
        (Gauss-Seidel); "wave+verify" runs the verify sweep after every time-segmented pass (by default
        only when the segments' exactness check fails)."""
        m = {"wave": 0, "sweep": 1, "ring": 1025, "wave+verify": 1026}[mode] if isinstance(mode, str) else int(mode)
        if self.L.hgx_set_la_kernel(self.ctx, m) != 0:
            raise ValueError(f"invalid lastAncestors kernel {mode}")

    def set_round_kernel(self, mode):
        """DivideRounds rounds: "auto" (default: the persistent recurrence on calls that lay the DAG
        out anew, where it applies, else per-round "candidate" launches; the whole-graph
        recurrence on every call for n <= 16), "persistent" (the persistent recurrence on every
        call where it applies), "graph" (one workgroup per graph of n <= 16 on every call),
        "block" (block binary search per round), "candidate" (one launch per round, one lane
        per candidate) or "auto-steps" ("auto" without the big-n persistent recurrence: n > 256
        runs the "candidate" steps)."""
        m = ({"auto": 0, "block": 1, "candidate": 2, "persistent": 3, "graph": 4, "auto-steps": 5}[mode]
             if isinstance(mode, str) else int(mode))
        if self.L.hgx_set_round_kernel(self.ctx, m) != 0:
            raise ValueError(f"invalid round kernel {mode}")

    def set_sort_kernel(self, mode):
        """FindOrder's sort: "auto" (default: buckets by (graph, roundReceived), each sorted in LDS,
        where every bucket holds <= 8 192 events) or "radix" (LSD radix passes over the whole list)."""
        m = {"auto": 0, "radix": 1}[mode] if isinstance(mode, str) else int(mode)
        if self.L.hgx_set_sort_kernel(self.ctx, m) != 0:
            raise ValueError(f"invalid sort kernel {mode}")

    def set_round_shards(self, shards: int):
        """hgx_create_sharded's chain-sharded recurrence with every shard on this context's device
        (hgx_set_round_shards): on an empty context; W shards on one device need
        GPU_MAX_HW_QUEUES >= W + 2."""
        if self.L.hgx_set_round_shards(self.ctx, int(shards)) != 0:
            raise ValueError(f"invalid shard count {shards} (an empty context, 1..8 shards, "
                             f"GPU_MAX_HW_QUEUES >= shards + 2 for shards sharing a device)")

    def set_shard_remote(self, on: bool = True):
        """Test switch (hgx_set_shard_remote): the shards' window stores take the cross-device
        (system-scope) path even where the shards share a device."""
        if self.L.hgx_set_shard_remote(self.ctx, 1 if on else 0) != 0:
            raise ValueError("hgx_set_shard_remote: not a chain-sharded context")

    def set_cts_kernel(self, mode):
        """FindOrder consensus timestamps: "auto" (default: "row" for 32 < n <= 256 on a call that
        receives at least 512 events per chain, else "tile"; "auto" no longer equals "tile"), "tile"
        (one tile of 8 positions per block), "pipe" (resident blocks with several tiles' loads in
        flight, hgx_cts.hip), "row" (blocks of 64 positions, lane = event, on every call where
        32 < n <= 256, else "tile") or "row1" ("row" with one staged WLAT row per block: the
        global-memory membership path, for tests and measurement)."""
        m = {"auto": 0, "tile": 1, "pipe": 2, "row": 3, "row1": 4}[mode] if isinstance(mode, str) else int(mode)
        if self.L.hgx_set_cts_kernel(self.ctx, m) != 0:
            raise ValueError(f"invalid timestamp kernel {mode}")

    def set_incremental(self, on: bool):
        """DivideRounds schedule: incremental (default) or full recompute on every call."""
        if self.L.hgx_set_incremental(self.ctx, 1 if on else 0) != 0:
            raise ValueError("invalid schedule")

    def reserve_rounds(self, rounds: int):
        """Size the per-round tables (before the first DivideRounds; small values exercise growth)."""
        if self.L.hgx_reserve_rounds(self.ctx, int(rounds)) != 0:
            raise ValueError("hgx_reserve_rounds failed")

    def set_coord_storage(self, mode):
        """0 = auto (uint16 coordinates when every Index fits), 1 = always int32."""
        if self.L.hgx_set_coord_storage(self.ctx, int(mode)) != 0:
            raise ValueError(f"invalid coordinate storage mode {mode}")

    def kernel_stats(self):
        res = {}
        for k in range(10):
            name = C.create_string_buffer(32)
            ms, launches, nbytes = C.c_double(), C.c_int64(), C.c_double()
            if self.L.hgx_kernel_stats(self.ctx, k, name, 32, C.byref(ms), C.byref(launches), C.byref(nbytes)):
                break
            res[name.value.decode()] = dict(ms=ms.value, launches=launches.value, bytes=nbytes.value)
        return res

    KERNELS = ("layout", "la_sweep", "fd_build", "round_gather", "round_search", "fame", "threshold",
               "round_received", "cts_median", "order_sort")

    def set_kernel_timing(self, which=True):
        """True = time every kernel launch with HIP events; a kernel name = only that one; False = off."""
        if which is True:
            mask = -1
        elif not which:
            mask = 0
        else:
            mask = 1 << self.KERNELS.index(which)
        self.L.hgx_set_kernel_timing(self.ctx, mask)

    def reset_stats(self):
        self.L.hgx_reset_stats(self.ctx)


class DeviceBuffer:
    """A host array copied to a buffer from hgx_device_alloc (libhgx's own HIP runtime)."""

    def __init__(self, a: np.ndarray, device: int = 0):
        self.L = _lib.lib()
        self.device = device
        a = np.ascontiguousarray(a)
        self.nbytes = a.nbytes
        self.p = C.c_void_p()
        if self.L.hgx_device_alloc(device, max(1, a.nbytes), C.byref(self.p)) != 0:
            raise HgxError(200, "hgx_device_alloc failed")
        if a.nbytes and self.L.hgx_device_copy(device, self.p, ptr(a), a.nbytes, 1) != 0:
            self.close()
            raise HgxError(200, "hgx_device_copy failed")

    @property
    def addr(self) -> int:
        return int(self.p.value or 0)

    def close(self):
        if getattr(self, "p", None) is not None and self.p.value:
            self.L.hgx_device_free(self.device, self.p)
            self.p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceTrace:
    """A trace's hgx_events columns resident in HBM (buffers from hgx_device_alloc on the
    context's device). Feeds Hashgraph.insert_device."""

    def __init__(self, t, device: int = 0):
        self.L = _lib.lib()
        self.device = device
        self.E = int(t.creator.shape[0])
        self.bufs = {}
        for name, src, dt in (("creator", t.creator, np.int32), ("index", t.index, np.int64),
                              ("sp", t.sp, np.int64), ("op", t.op, np.int64), ("ts", t.ts, np.int64),
                              ("hash", t.hash, np.uint8), ("s", t.s, np.uint8), ("ntx", t.ntx, np.int32),
                              ("nil", t.txnil, np.int32)):
            a = np.ascontiguousarray(src, dtype=dt)
            p = C.c_void_p()
            if self.L.hgx_device_alloc(device, a.nbytes, C.byref(p)) != 0:
                self.close()
                raise HgxError(200, "hgx_device_alloc failed")
            self.bufs[name] = (p, a.itemsize * (32 if name in ("hash", "s") else 1))
            if a.nbytes and self.L.hgx_device_copy(device, p, ptr(a), a.nbytes, 1) != 0:
                self.close()
                raise HgxError(200, "hgx_device_copy failed")

    def close(self):
        for p, _ in getattr(self, "bufs", {}).values():
            self.L.hgx_device_free(self.device, p)
        self.bufs = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def events(self, lo: int, hi: int) -> hgx_events:
        def p(name):
            base, per = self.bufs[name]
            return C.c_void_p((base.value or 0) + lo * per)

        return hgx_events(p("creator"), p("index"), p("sp"), p("op"), p("ts"), p("hash"), p("s"), p("ntx"), p("nil"))


def block_hash(rr: int, txs: List[bytes], tx_nil: bool) -> bytes:
    """SHA256(json.Encoder(Block)) (hashgraph/block.go:44-53), computed by libhgx."""
    L = _lib.lib()
    ntx = len(txs)
    bufs = [C.create_string_buffer(t, max(len(t), 1)) for t in txs]
    ptrs = (C.c_void_p * max(ntx, 1))(*[C.cast(b, C.c_void_p) for b in bufs])
    lens = (C.c_int64 * max(ntx, 1))(*[len(t) for t in txs])
    out = C.create_string_buffer(32)
    rc = L.hgx_block_hash(rr, ntx, ptrs, lens, 1 if tx_nil else 0, out)
    if rc:
        raise HgxError(rc, "hgx_block_hash failed")
    return out.raw


def sha256_batch(data: np.ndarray, offsets: np.ndarray, device: int = 0) -> np.ndarray:
    """crypto.SHA256 (crypto/utils.go:11-16) of every message data[offsets[i]:offsets[i+1]]
    in one device launch (hgx_sha256_batch). Returns a (count, 32) uint8 array.
    Raises HgxError (code HGX_ERR_DEVICE) without a gfx950 GPU: there is no CPU path."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    count = max(len(offsets) - 1, 0)
    out = np.zeros((count, 32), dtype=np.uint8)
    err = hgx_error()
    rc = _lib.lib().hgx_sha256_batch(device, ptr(data) if data.size else None, ptr(offsets) if count else None,
                                     count, ptr(out) if count else None, C.byref(err))
    _lib.check(rc, err)
    return out


def event_ids(bodies: Sequence[bytes], device: int = 0) -> List[bytes]:
    """Event.Hash for a batch of json.Encoder(Event) encodings (hashgraph/event.go:171-180),
    hashed on the GPU; Hex() is "0x%X" of each (event.go:183-188)."""
    lens = np.fromiter((len(b) for b in bodies), dtype=np.int64, count=len(bodies))
    offsets = np.zeros(len(bodies) + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    data = np.frombuffer(b"".join(bodies), dtype=np.uint8)
    return [bytes(r) for r in sha256_batch(data, offsets, device)]


def _splitmix64(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def sha256_bench_messages(n: int, min_len: int, max_len: int, seed: int) -> List[bytes]:
    """The first n synthetic messages hgx_sha256_bench hashes (include/hgx.h), rebuilt on the host."""
    i = np.arange(n, dtype=np.uint64)
    lens = min_len + (_splitmix64(~np.uint64(seed) + i) % np.uint64(max_len - min_len + 1)).astype(np.int64)
    total = int(lens.sum())
    words = _splitmix64(np.uint64(seed) + np.arange((total + 7) // 8, dtype=np.uint64))
    blob = words.astype("<u8").tobytes()
    out, o = [], 0
    for ln in lens:
        out.append(blob[o:o + int(ln)])
        o += int(ln)
    return out


def sha256_bench(count: int, min_len: int, max_len: int, seed: int = 5, warmup: int = 1, iters: int = 3,
                 n_sample: int = 64, device: int = 0) -> dict:
    """Device-resident SHA-256 throughput (hgx_sha256_bench) + digests of the first n_sample messages."""
    ms, tot, nb = C.c_double(), C.c_int64(), C.c_int64()
    sample = np.zeros((n_sample, 32), dtype=np.uint8)
    rc = _lib.lib().hgx_sha256_bench(device, count, min_len, max_len, seed, warmup, iters, C.byref(ms),
                                     C.byref(tot), C.byref(nb), n_sample, ptr(sample))
    if rc:
        raise HgxError(rc, "hgx_sha256_bench failed")
    return {"ms_per_launch": ms.value, "bytes": tot.value, "blocks": nb.value, "sample": sample}


def seg_sort_check(segoff, keys, vals, S, force_kv: bool = False, device: int = 0):
    """FindOrder's bucket sort on caller-given buckets (hgx_seg_sort_check): bucket b is elements
    [segoff[b], segoff[b + 1]) of (keys, vals), the last one ends at len(keys); vals are rows of S [m, 32].
    Returns (the values of every bucket ordered by (key, S row), whether the one-word path ran)."""
    so = np.ascontiguousarray(segoff, np.uint32)
    k = np.ascontiguousarray(keys, np.uint64)
    v = np.ascontiguousarray(vals, np.uint32)
    s = np.ascontiguousarray(S, np.uint8).reshape(-1, 32)
    m = k.shape[0]
    assert v.shape[0] == m and s.shape[0] == m
    out = np.zeros(m, np.uint32)
    packed = C.c_int32()
    rc = _lib.lib().hgx_seg_sort_check(device, so.shape[0], ptr(so), m, ptr(k), ptr(v), ptr(s), int(bool(force_kv)),
                                       ptr(out), C.byref(packed))
    if rc:
        raise HgxError(rc, "hgx_seg_sort_check failed")
    return out, bool(packed.value)


def _p256_cols(keys65, key_idx, digest, r, s):
    k = np.ascontiguousarray(keys65, np.uint8).reshape(-1, 65)
    cols = [np.ascontiguousarray(key_idx, np.int32)] + [np.ascontiguousarray(x, np.uint8).reshape(-1, 32)
                                                         for x in (digest, r, s)]
    m = cols[0].shape[0]
    assert all(c.shape[0] == m for c in cols[1:])
    return k, cols, m


def p256_verify(keys65, key_idx, digest, r, s, device: int = 0) -> np.ndarray:
    """Event.Verify for a batch (hgx_p256_verify_batch): 1 valid, 0 invalid, 2 key not a P-256 point."""
    k, cols, m = _p256_cols(keys65, key_idx, digest, r, s)
    out = np.zeros(m, np.uint8)
    err = hgx_error()
    rc = _lib.lib().hgx_p256_verify_batch(device, ptr(k), k.shape[0], *[ptr(c) for c in cols], m, ptr(out),
                                          C.byref(err))
    _lib.check(rc, err)
    return out


def p256_sign(priv32, key_idx, digest, device: int = 0):
    """crypto.Sign for a batch (hgx_p256_sign_batch): digest[i] under the private key priv32[key_idx[i]]
    (32 bytes big-endian each), RFC 6979 nonces. Returns (r [m, 32], s [m, 32])."""
    d = np.ascontiguousarray(priv32, np.uint8).reshape(-1, 32)
    idx = np.ascontiguousarray(key_idx, np.int32)
    dig = np.ascontiguousarray(digest, np.uint8).reshape(-1, 32)
    m = idx.shape[0]
    assert dig.shape[0] == m
    r, s = np.zeros((m, 32), np.uint8), np.zeros((m, 32), np.uint8)
    err = hgx_error()
    rc = _lib.lib().hgx_p256_sign_batch(device, ptr(d), d.shape[0], ptr(idx), ptr(dig), m, ptr(r), ptr(s), C.byref(err))
    _lib.check(rc, err)
    return r, s


def p256_public_keys(priv32, device: int = 0) -> np.ndarray:
    """0x04 | X | Y of d G for every private key (hgx_p256_public_keys): [n, 65]."""
    d = np.ascontiguousarray(priv32, np.uint8).reshape(-1, 32)
    out = np.zeros((d.shape[0], 65), np.uint8)
    err = hgx_error()
    rc = _lib.lib().hgx_p256_public_keys(device, ptr(d), d.shape[0], ptr(out), C.byref(err))
    _lib.check(rc, err)
    return out


def p256_verify_bench(keys65, key_idx, digest, r, s, warmup: int = 1, iters: int = 3, device: int = 0) -> dict:
    """Device-resident verify throughput (hgx_p256_verify_bench): ms per (tables + verify) launch."""
    k, cols, m = _p256_cols(keys65, key_idx, digest, r, s)
    out = np.zeros(m, np.uint8)
    ms = C.c_double()
    rc = _lib.lib().hgx_p256_verify_bench(device, ptr(k), k.shape[0], *[ptr(c) for c in cols], m, warmup, iters,
                                          ptr(out), C.byref(ms))
    if rc:
        raise HgxError(rc, "hgx_p256_verify_bench failed")
    return {"ms_per_launch": ms.value, "out": out}
