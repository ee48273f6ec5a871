"""Test infrastructure for hgx_insert_wire_bodies: the wire columns of a bodyref.Chain slice (what a peer
would send: no hash, parents as (creator id, Index)), a Python restatement of ReadWireInfo's resolution
rule (hashgraph.go:569-614 over RollingIndex.GetItem, common/rolling_index.go:40-50) with every
participant's item list spelled out, and the id of a chain event re-signed over other parents. Nothing
here is product code, and nothing here calls the code under test."""
from __future__ import annotations

import hashlib
from typing import List, Optional

import numpy as np

import bodyref
import hgref
from babble_amd.hashgraph import wire_body_columns

TOO_LATE, NOT_FOUND, PANIC = 2, 1, 300
PANIC_CREATOR = "runtime error: slice bounds out of range [2:0]"
PANIC_OTHER = "runtime error: invalid memory address or nil pointer dereference"


def rune(v: int) -> str:
    """Go's string(int)"""
    return "\ufffd" if v < 0 or v > 0x10FFFF or 0xD800 <= v <= 0xDFFF else chr(v)


def wire_rows(t, sel=None) -> dict:
    """The wire fields of trace events `sel` (default all): SetWireInfo without roots, from the trace's
    own parents (gids of the same trace)."""
    sel = np.arange(t.E) if sel is None else np.asarray(sel, np.int64)
    sp, op = t.sp[sel], t.op[sel]
    return dict(creator_id=t.creator[sel].astype(np.int32), index=t.index[sel].astype(np.int64),
                self_parent_index=np.where(sp >= 0, t.index[np.maximum(sp, 0)], -1).astype(np.int64),
                other_parent_creator=np.where(op >= 0, t.creator[np.maximum(op, 0)], -1).astype(np.int32),
                other_parent_index=np.where(op >= 0, t.index[np.maximum(op, 0)], -1).astype(np.int64),
                timestamp_ns=t.ts[sel].astype(np.int64), sig_s=t.s[sel])


def wire_cols(c: bodyref.Chain, sel=None, r=None, s=None, txs=None, **repl) -> dict:
    """hgx_wire_bodies columns of the chain's events `sel`; repl replaces wire fields (full-length arrays
    over sel), r / s / txs the signature columns and transactions (indexed like the chain)."""
    sel = np.arange(c.t.E) if sel is None else np.asarray(sel, np.int64)
    rows = wire_rows(c.t, sel)
    if s is not None:
        rows["sig_s"] = np.asarray(s)[sel]
    rows.update(repl)
    return wire_body_columns(rows, (c.r if r is None else np.asarray(r))[sel],
                             [(c.txs if txs is None else txs)[int(i)] for i in sel])


class Store:
    """participantEventsCache: per participant lastIndex and the cached items (gids)."""

    def __init__(self, n: int):
        self.n = n
        self.last = [-1] * n
        self.items: List[List[int]] = [[] for _ in range(n)]
        self.E = 0

    def add(self, creator: int, index: int):
        self.items[creator].append(self.E)
        self.last[creator] = index
        self.E += 1

    def get_item(self, p: int, index: int):
        """(gid, code, message)"""
        if p < 0 or p >= self.n:
            return None, PANIC, PANIC_OTHER
        n = len(self.items[p])
        oldest = self.last[p] - n + 1
        if index < oldest:
            return None, TOO_LATE, rune(index) + ", Too Late"
        if index - oldest >= n:
            return None, NOT_FOUND, rune(index) + ", Not Found"
        return self.items[p][index - oldest], 0, ""


def store_of(t, E: int) -> Store:
    st = Store(t.n)
    for g in range(E):
        st.add(int(t.creator[g]), int(t.index[g]))
    return st


def resolve(st: Store, w: dict, lo: int = 0, hi: Optional[int] = None):
    """ReadWireInfo per event of w[lo:hi] against st, each resolved event appended as InsertEvent would.
    Returns (sp gids, op gids, m, code, message): m = events before the first resolution error."""
    hi = len(w["creator_id"]) if hi is None else hi
    sp, op = [], []
    for k in range(lo, hi):
        c = int(w["creator_id"][k])
        if c < 0 or c >= st.n:
            return sp, op, k - lo, PANIC, PANIC_CREATOR
        s = o = -1
        if w["self_parent_index"][k] >= 0:
            s, code, msg = st.get_item(c, int(w["self_parent_index"][k]))
            if code:
                return sp, op, k - lo, code, msg
        if w["other_parent_index"][k] >= 0:
            o, code, msg = st.get_item(int(w["other_parent_creator"][k]), int(w["other_parent_index"][k]))
            if code:
                return sp, op, k - lo, code, msg
        sp.append(s)
        op.append(o)
        st.add(c, int(w["index"][k]))
    return sp, op, hi - lo, 0, ""


def resigned(c: bodyref.Chain, k: int, sp: int, op: int):
    """Chain event k with other parents (gids of the chain, -1 for ""), signed that way: (r, s, id)."""
    r, s = c.sign_event(k, sp, op)
    pid = lambda g: bytes(c.ids[g]) if g >= 0 else None
    js = hgref.go_event_json(c.txs[k], bodyref.hex_id(pid(sp)), bodyref.hex_id(pid(op)),
                             bytes(c.keys[c.t.creator[k]]), int(c.t.ts[k]), int(c.t.index[k]), bytes(r), bytes(s))
    return r, s, np.frombuffer(hashlib.sha256(js).digest(), np.uint8)
