"""TEST INFRASTRUCTURE: the pure-Python reference of libhgx's signer.

ECDSA P-256 with Python integers (p256ref's affine points), nonces by RFC 6979 section 3.2 with
HMAC-SHA-256 (hmac / hashlib; qlen = hlen = 256, no additional data), s not normalised to the low half.
The test keys are oracle/p256_ref.c's derived ones: d_k = SHA-256("hgx test key \\0\\0\\0" | k as a
little-endian u32) mod N, with 0 -> 1, so p256_ref sign's public keys are the ones computed here. The
chain builder is bodyref.build with these signatures in place of libcrypto's random-nonce ones: level
by level, text from hgref.go_event_json. Nothing here is product code.
"""
from __future__ import annotations

import functools
import hashlib
import hmac
from typing import List, Optional

import numpy as np

import p256ref
from p256ref import G, N


def priv(k: int) -> int:
    d = int.from_bytes(hashlib.sha256(b"hgx test key \0\0\0" + int(k).to_bytes(4, "little")).digest(), "big") % N
    return d or 1


def priv_bytes(n: int) -> np.ndarray:
    """[n, 32] the derived private keys 0..n-1, big-endian."""
    return np.frombuffer(b"".join(priv(k).to_bytes(32, "big") for k in range(n)), np.uint8).reshape(n, 32).copy()


@functools.lru_cache(maxsize=None)
def pub65(d: int) -> bytes:
    return p256ref.pub65(p256ref.comb_mul(d, G))


def pub_bytes(n: int) -> np.ndarray:
    return np.frombuffer(b"".join(pub65(priv(k)) for k in range(n)), np.uint8).reshape(n, 65).copy()


def nonces(d: int, digest: bytes):
    """RFC 6979 3.2: the candidate nonces for the private key d and the 32-byte digest, in order
    (candidates outside [1, N-1] included: the caller skips them as step h.3 does)."""
    assert len(digest) == 32
    x = d.to_bytes(32, "big")                                        # int2octets
    h = (int.from_bytes(digest, "big") % N).to_bytes(32, "big")      # bits2octets
    mac = lambda key, msg: hmac.new(key, msg, hashlib.sha256).digest()
    V, K = b"\x01" * 32, b"\x00" * 32
    K = mac(K, V + b"\x00" + x + h)
    V = mac(K, V)
    K = mac(K, V + b"\x01" + x + h)
    V = mac(K, V)
    while True:
        V = mac(K, V)
        yield int.from_bytes(V, "big")
        K = mac(K, V + b"\x00")
        V = mac(K, V)


def sign(d: int, digest: bytes):
    """(r, s, k): the signature of the digest under d and the nonce that was used."""
    e = int.from_bytes(digest, "big") % N
    for k in nonces(d, digest):
        if not 1 <= k < N:
            continue
        r = p256ref.comb_mul(k, G)[0] % N
        s = pow(k, -1, N) * (e + r * d) % N
        if r and s:
            return r, s, k


def sign_batch(privs, key_idx, digests):
    """r [m, 32], s [m, 32] of digests[i] under the private key privs[key_idx[i]] (ints)."""
    digests = np.ascontiguousarray(digests, np.uint8).reshape(-1, 32)
    r = np.zeros((len(key_idx), 32), np.uint8)
    s = np.zeros((len(key_idx), 32), np.uint8)
    for i, k in enumerate(key_idx):
        ri, si, _ = sign(privs[int(k)], bytes(digests[i]))
        r[i] = np.frombuffer(ri.to_bytes(32, "big"), np.uint8)
        s[i] = np.frombuffer(si.to_bytes(32, "big"), np.uint8)
    return r, s


def event(txs, sp_id: Optional[bytes], op_id: Optional[bytes], d: int, ts: int, index: int):
    """One signed event from its parents' ids: (r, s, json, id, body digest), all bytes."""
    import bodyref
    import hgref
    key = pub65(d)
    dig = hashlib.sha256(bodyref.body_json(txs, sp_id, op_id, key, ts, index)).digest()
    r, s, _ = sign(d, dig)
    rb, sb = r.to_bytes(32, "big"), s.to_bytes(32, "big")
    js = hgref.go_event_json(txs, bodyref.hex_id(sp_id), bodyref.hex_id(op_id), key, ts, index, rb, sb)
    return rb, sb, js, hashlib.sha256(js).digest(), dig


def build(t, txs: List[Optional[List[bytes]]]):
    """bodyref.Chain of the trace signed with the derived keys and RFC 6979 nonces."""
    import bodyref
    from babble_amd import trace as gtrace
    E, n = t.E, t.n
    level, nl = bodyref.py_levels(t.sp, t.op)
    privs = [priv(k) for k in range(n)]
    keys = pub_bytes(n)
    ids, dig, r, s = (np.zeros((E, 32), np.uint8) for _ in range(4))
    js: List[bytes] = [b""] * E
    pid = lambda g: bytes(ids[g]) if g >= 0 else None
    for l in range(nl):
        for k in np.nonzero(level == l)[0]:
            rb, sb, js[k], idb, db = event(txs[k], pid(t.sp[k]), pid(t.op[k]), privs[int(t.creator[k])], int(t.ts[k]),
                                           int(t.index[k]))
            for col, b in ((r, rb), (s, sb), (ids, idb), (dig, db)):
                col[k] = np.frombuffer(b, np.uint8)
    t2 = gtrace.GossipTrace(**{**t.__dict__, "hash": ids.copy(), "s": s.copy()})
    c = bodyref.Chain(n=n, t=t2, txs=txs, keys=keys, r=r, dig=dig, ids=ids, json=js, level=level, cols={})
    c.cols = c.columns()
    return c


@functools.lru_cache(maxsize=None)
def chain(n: int, E: int, seed: int):
    """The chain of gossip(n, E, seed) (bodyref.chain's trace); computed once and shared (read-only)."""
    from babble_amd import trace as gtrace
    t = gtrace.gossip(n, E, seed, stale_prob=0.1, stale_depth=2)
    return build(t, [t.txs(i) for i in range(t.E)])


def manual(n: int, creator, sp, op, txs):
    """bodyref.manual's hand-made DAG, signed here."""
    import bodyref
    import hgref
    from babble_amd import trace as gtrace
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


def ref_lines(entries) -> str:
    """oracle/p256_ref check's input for (pub65, digest, r, s) byte tuples that must all verify."""
    return "".join(f"{p.hex()} {d.hex()} {r.hex()} {s.hex()} 1 1 sign\n" for p, d, r, s in entries)
