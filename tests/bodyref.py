"""Test infrastructure: the expected event chain of a gossip trace, built on the CPU.

An event's Go-JSON holds its parents' hex ids, and an id is the SHA-256 of the parent's JSON with its
signature, so the chain is built level by level (a level = events whose parents all lie in earlier
levels): body JSON sliced out of hgref.go_event_json, body digest from hashlib, one hgref.sign_batch
per level (derived keys: identical across calls), then the event's JSON and its id. Nothing here is
product code.
"""
from __future__ import annotations

import functools
import hashlib
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

import hgref
from babble_amd import trace as gtrace
from babble_amd.hashgraph import body_columns

_TAIL0 = b',"R":0,"S":0}\n'
_ZERO = bytes(32)


def py_levels(sp, op, base: int = 0):
    """The reference for hgx_batch_levels: depth of every event inside the batch."""
    level = []
    for k, (s, o) in enumerate(zip(sp, op)):
        if s >= base + k or o >= base + k:
            raise ValueError(f"event {k} names a parent that is not an earlier event")
        level.append(max([level[p - base] + 1 for p in (int(s), int(o)) if p >= base], default=0))
    return np.asarray(level, np.int32), (max(level) + 1 if level else 0)


def hex_id(h: Optional[bytes]) -> str:
    return "" if h is None else "0x" + h.hex().upper()


def body_json(txs, sp_id, op_id, key: bytes, ts: int, index: int) -> bytes:
    """EventBody.Marshal: the body of the event's JSON plus Encode's newline."""
    js = hgref.go_event_json(txs, hex_id(sp_id), hex_id(op_id), key, ts, index, _ZERO, _ZERO)
    assert js.startswith(b'{"Body":') and js.endswith(_TAIL0)
    return js[8:-len(_TAIL0)] + b"\n"


@dataclass
class Chain:
    n: int
    t: gtrace.GossipTrace      # the trace with hash = the ids and s = the signatures' S
    txs: List[Optional[List[bytes]]]
    keys: np.ndarray           # [n, 65]
    r: np.ndarray              # [E, 32]
    dig: np.ndarray            # [E, 32] body digests
    ids: np.ndarray            # [E, 32]
    json: List[bytes]
    level: np.ndarray
    cols: dict                 # body_columns of the whole trace

    def columns(self, **repl) -> dict:
        """body_columns with some columns (or txs) replaced."""
        a = dict(creator=self.t.creator, index=self.t.index, sp=self.t.sp, op=self.t.op, ts=self.t.ts, r=self.r,
                 s=self.t.s, txs=self.txs)
        a.update(repl)
        return body_columns(**a)

    def sign_event(self, k: int, sp: int, op: int):
        """(r, s) of event k's body with other parents (ids of the chain), under its creator's key."""
        key = bytes(self.keys[self.t.creator[k]])
        bj = body_json(self.txs[k], bytes(self.ids[sp]) if sp >= 0 else None, bytes(self.ids[op]) if op >= 0 else None,
                       key, int(self.t.ts[k]), int(self.t.index[k]))
        d = np.frombuffer(hashlib.sha256(bj).digest(), np.uint8)
        _, r, s = hgref.sign_batch(self.n, [int(self.t.creator[k])], d[None, :])
        return r[0], s[0]


def manual(n: int, creator, sp, op, txs) -> Chain:
    """The signed chain of a hand-made DAG (n = participants over all graphs): Index counts each
    creator's events, timestamps are 1 µs apart."""
    creator = np.asarray(creator, np.int32)
    E = len(creator)
    index = np.zeros(E, np.int64)
    seen = {}
    for k, c in enumerate(creator):
        index[k] = seen.get(int(c), 0)
        seen[int(c)] = int(index[k]) + 1
    t = gtrace.GossipTrace(n=n, creator=creator, index=index, sp=np.asarray(sp, np.int64), op=np.asarray(op, np.int64),
                           ts=hgref.T0_NS + 1000 * np.arange(E, dtype=np.int64), hash=np.zeros((E, 32), np.uint8),
                           s=np.zeros((E, 32), np.uint8), ntx=np.asarray([len(x or []) for x in txs], np.int32),
                           txnil=np.asarray([x is None for x in txs], np.int32), tx_seq=np.full(E, -1, np.int64))
    return build(t, list(txs))


def build(t: gtrace.GossipTrace, txs: List[Optional[List[bytes]]]) -> Chain:
    E, n = t.E, t.n
    level, nl = py_levels(t.sp, t.op)
    keys, _, _ = hgref.sign_batch(n, [0], np.zeros((1, 32), np.uint8))
    ids = np.zeros((E, 32), np.uint8)
    dig = np.zeros((E, 32), np.uint8)
    r = np.zeros((E, 32), np.uint8)
    s = np.zeros((E, 32), np.uint8)
    js: List[bytes] = [b""] * E
    pid = lambda g: bytes(ids[g]) if g >= 0 else None
    for l in range(nl):
        ks = np.nonzero(level == l)[0]
        for k in ks:
            bj = body_json(txs[k], pid(t.sp[k]), pid(t.op[k]), bytes(keys[t.creator[k]]), int(t.ts[k]), int(t.index[k]))
            dig[k] = np.frombuffer(hashlib.sha256(bj).digest(), np.uint8)
        k2, r[ks], s[ks] = hgref.sign_batch(n, t.creator[ks], dig[ks])
        assert np.array_equal(k2, keys)
        for k in ks:
            js[k] = hgref.go_event_json(txs[k], hex_id(pid(t.sp[k])), hex_id(pid(t.op[k])), bytes(keys[t.creator[k]]),
                                        int(t.ts[k]), int(t.index[k]), bytes(r[k]), bytes(s[k]))
            ids[k] = np.frombuffer(hashlib.sha256(js[k]).digest(), np.uint8)
    t2 = gtrace.GossipTrace(**{**t.__dict__, "hash": ids.copy(), "s": s.copy()})
    c = Chain(n=n, t=t2, txs=txs, keys=keys, r=r, dig=dig, ids=ids, json=js, level=level, cols={})
    c.cols = c.columns()
    return c


@functools.lru_cache(maxsize=None)
def chain(n: int, E: int, seed: int) -> Chain:
    """The signed chain of gossip(n, E, seed); computed once and shared (treat it as read-only)."""
    t = gtrace.gossip(n, E, seed, stale_prob=0.1, stale_depth=2)
    return build(t, [t.txs(i) for i in range(t.E)])
