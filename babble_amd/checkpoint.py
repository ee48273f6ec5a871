"""Checkpoint files of the resident event DAG (include/hgx.h, "persistence").

The reference persists its DAG in the BadgerStore: events keyed by topological index with their
bodies and signatures, the participants, the roots and the blocks (badger_store.go:103-125,
309-343, 540); Hashgraph.Bootstrap replays the events through InsertEvent before running
consensus once (hashgraph.go:1008-1037, dbTopologicalEvents badger_store.go:345-386). Here the log
is one binary structure-of-arrays file; libhgx writes it (hgx_save / hgx_save_ex) and replays it
(hgx_bootstrap). This module reads and writes the same format on the host, so a synthetic trace
can be written as a checkpoint and bootstrapped, and a file written by the device can be
inspected. Little-endian layout (version 2; version 1 = no optional sections and flags <= 1;
version 3 below):

    "HGXCKPT1" | u32 version | i32 n | i32 graphs | i32 flags | i64 E
        flags: 1 rooted, 2 event ids, 4 participant keys, 8 payloads
    | rooted: i32 root_index[C] | i32 root_round[C] | u8 root_y_is_event[C] (zero pad to 4)
        | i64 n_others | u8 others[n_others][32]
        | per graph: i32 has_lcr, i32 lcr, i32 lcre, i32 0, i64 consensus_tx, i64 n_blocks,
          n_blocks x (i32 rr, i32 events, i64 transactions, i32 nil, i32 committed)
    | i32 creator[E] | i64 index[E] | i64 self_parent[E] | i64 other_parent[E]
    | i64 timestamp_ns[E] | u8 sig_s[E][32] | u8 coin[E] | i32 ntx[E] | u8 tx_nil[E]
    | ids u8[E][32] | keys u8[C][65] | payloads: i64 off[E+1], u8 bytes[off[E]]
    | u64 FNV-1a over every preceding byte

Version 3 (hgx_save_bodies: the checkpoint of a context that keeps its event bodies) has flags 2, 4 and
16 (bodies) set, 8 clear and 1 when rooted, and adds to the sections above, in place:

    behind the rooted section's per-graph kept state (rooted files only):
        u8 has_x[C] | u8 has_y[C] | zero pad to 4 | u8 x_id[C][32] | u8 y_id[C][32]
            (rows with has = 0 are zero; has_y equals root_y_is_event)
        | i64 n_pairs | u8 pair_event[n_pairs][32] | u8 pair_parent[n_pairs][32]
            (sorted by event id; pair_event equals the others section)
        | per graph, per kept block in order: u8 has_hash, 3 zero bytes, u8 hash[32]
    behind the keys:
        u8 sig_r[E][32] | i64 T | i64 tx_off[T+1] | u8 tx_bytes[tx_off[T]]
            (T = sum of ntx; tx_off starts at 0 and does not decrease)

read() refuses a version-3 file for the reasons hgx_bootstrap does, in the same words.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

MAGIC = b"HGXCKPT1"
VERSION = 2
VERSION_BODIES = 3
ROOTED, IDS, KEYS, PAYLOADS, BODIES = 1, 2, 4, 8, 16


def fnv1a(data: bytes) -> int:
    """64-bit FNV-1a of the bytes (the file's checksum), computed by libhgx (hgx_checksum; a
    host function, no device needed)."""
    from . import _lib
    L = _lib.lib()
    b = np.frombuffer(data, np.uint8)
    return int(L.hgx_checksum(_lib.ptr(b), b.size))


def encode(n: int, graphs: int, creator, index, sp, op, ts, sig_s, coin, ntx, tx_nil,
           roots: Optional[tuple] = None, others=None, kept: Optional[Sequence[dict]] = None,
           ids=None, keys=None, payloads: Optional[Sequence[bytes]] = None, bodies: Optional[tuple] = None,
           root_ids: Optional[tuple] = None, kept_hashes: Optional[Sequence[Sequence[Optional[bytes]]]] = None) -> bytes:
    """The file bytes for E events (gid order). roots = (root_index, root_round, root_y_is_event)
    of a context after a Reset (with its Root.Others keys and, per graph, what Reset kept:
    dict(has_lcr, lcr, lcre, consensus_tx, blocks=[(rr, events, transactions, nil, committed)]));
    ids = the events' 32-byte ids, keys = the participants' 65-byte keys, payloads = per-event bytes.
    bodies = (sig_r [E, 32], per event its list of transactions or None) makes a version-3 file, which
    needs ids and keys and takes no payloads; on a rooted one root_ids = (x ids [C], y ids [C], pairs
    [(event id, other-parent id)]) with None for a root without that id (others defaults to the pairs'
    event ids) and kept_hashes = per graph, per kept block its 32-byte hash or None."""
    E = len(creator)
    C = n * graphs
    if bodies is not None and (ids is None or keys is None or payloads is not None):
        raise ValueError("a version-3 file carries ids and keys and no payloads")
    if bodies is not None and roots is not None:
        xs, ys, pairs = root_ids if root_ids is not None else ([None] * C, [None] * C, [])
        pairs = sorted((bytes(a), bytes(b)) for a, b in pairs)
        if others is None:
            others = np.frombuffer(b"".join(a for a, _ in pairs), np.uint8).reshape(-1, 32)
    flags = (ROOTED if roots is not None else 0) | (IDS if ids is not None else 0) | \
        (KEYS if keys is not None else 0) | (PAYLOADS if payloads is not None else 0) | (BODIES if bodies is not None else 0)
    parts = [MAGIC, np.array([VERSION if bodies is None else VERSION_BODIES], "<u4").tobytes(),
             np.array([n, graphs, flags], "<i4").tobytes(), np.array([E], "<i8").tobytes()]
    if roots is not None:
        ri, rr, ry = roots
        y = np.zeros((C + 3) & ~3, np.uint8)
        y[:C] = np.asarray(ry, np.uint8)
        ok = np.zeros((0, 32), np.uint8) if others is None else np.asarray(others, np.uint8).reshape(-1, 32)
        parts += [np.asarray(ri, "<i4").tobytes(), np.asarray(rr, "<i4").tobytes(), y.tobytes(),
                  np.array([ok.shape[0]], "<i8").tobytes(), ok.tobytes()]
        for g in range(graphs):
            k = (kept or [{}] * graphs)[g]
            blocks = k.get("blocks", [])
            parts += [np.array([1 if k.get("has_lcr") else 0, k.get("lcr", 0), k.get("lcre", 0), 0], "<i4").tobytes(),
                      np.array([k.get("consensus_tx", 0), len(blocks)], "<i8").tobytes()]
            for rr_, nev, ntx_, nil_, com in blocks:
                parts += [np.array([rr_, nev], "<i4").tobytes(), np.array([ntx_], "<i8").tobytes(),
                          np.array([nil_, com], "<i4").tobytes()]
        if bodies is not None:
            has = np.zeros((2 * C + 3) & ~3, np.uint8)
            has[:C] = [x is not None for x in xs]
            has[C:2 * C] = [y is not None for y in ys]
            parts += [has.tobytes(), b"".join(bytes(32) if x is None else bytes(x) for x in xs),
                      b"".join(bytes(32) if y is None else bytes(y) for y in ys), np.array([len(pairs)], "<i8").tobytes(),
                      b"".join(a for a, _ in pairs), b"".join(b for _, b in pairs)]
            for g in range(graphs):
                nb = len((kept or [{}] * graphs)[g].get("blocks", []))
                hs = list((kept_hashes or [[]] * graphs)[g]) + [None] * nb
                for h in hs[:nb]:
                    parts.append(bytes(36) if h is None else b"\x01\0\0\0" + bytes(h))
    parts += [np.asarray(creator, "<i4").tobytes(), np.asarray(index, "<i8").tobytes(),
              np.asarray(sp, "<i8").tobytes(), np.asarray(op, "<i8").tobytes(), np.asarray(ts, "<i8").tobytes(),
              np.ascontiguousarray(np.asarray(sig_s, np.uint8).reshape(E, 32)).tobytes(),
              (np.asarray(coin) != 0).astype(np.uint8).tobytes(), np.asarray(ntx, "<i4").tobytes(),
              (np.asarray(tx_nil) != 0).astype(np.uint8).tobytes()]
    if ids is not None:
        parts.append(np.ascontiguousarray(np.asarray(ids, np.uint8).reshape(E, 32)).tobytes())
    if keys is not None:
        parts.append(np.ascontiguousarray(np.asarray(keys, np.uint8).reshape(C, 65)).tobytes())
    if payloads is not None:
        off = np.zeros(E + 1, "<i8")
        off[1:] = np.cumsum([len(b) for b in payloads]) if E else []
        parts += [off.tobytes(), b"".join(payloads)]
    if bodies is not None:
        sig_r, txs = bodies
        flat = [bytes(b) for x in txs for b in (x or [])]
        off = np.zeros(len(flat) + 1, "<i8")
        off[1:] = np.cumsum([len(b) for b in flat]) if flat else []
        parts += [np.ascontiguousarray(np.asarray(sig_r, np.uint8).reshape(E, 32)).tobytes(),
                  np.array([len(flat)], "<i8").tobytes(), off.tobytes(), b"".join(flat)]
    body = b"".join(parts)
    return body + np.array([fnv1a(body)], "<u8").tobytes()


def write_trace(path: str, t, graphs: int = 1, with_ids: bool = True) -> None:
    """A synthetic trace (babble_amd.trace.GossipTrace; n = participants per graph) as a checkpoint
    (with its event ids unless with_ids=False): the coin is the id's byte 16 (middleBit,
    hashgraph.go:1039-1048)."""
    data = encode(t.n, graphs, t.creator, t.index, t.sp, t.op, t.ts, t.s, t.hash[:, 16] != 0, t.ntx, t.txnil,
                  ids=t.hash if with_ids else None)
    with open(path, "wb") as f:
        f.write(data)


def read(path: str) -> dict:
    """Parse and verify a checkpoint file (ValueError on a bad magic, version, size or checksum)."""
    with open(path, "rb") as f:
        buf = f.read()
    if len(buf) < 40:
        raise ValueError("truncated file")
    if fnv1a(buf[:-8]) != int(np.frombuffer(buf[-8:], "<u8")[0]):
        raise ValueError("checksum mismatch")
    if buf[:8] != MAGIC:
        raise ValueError("not a checkpoint file")
    version = int(np.frombuffer(buf, "<u4", 1, 8)[0])
    if version not in (1, 2, 3):
        raise ValueError(f"unsupported version {version}")
    n, graphs, flags = (int(x) for x in np.frombuffer(buf, "<i4", 3, 12))
    if version == 1 and flags & ~ROOTED:
        raise ValueError("unsupported flags")
    v3 = version == 3
    if v3 and ((flags & (IDS | KEYS | BODIES)) != (IDS | KEYS | BODIES) or flags & ~(IDS | KEYS | BODIES | ROOTED)):
        raise ValueError("unsupported flags")
    if v3 and flags & ROOTED and graphs != 1:
        raise ValueError("roots need a single-graph context")
    E = int(np.frombuffer(buf, "<i8", 1, 24)[0])
    C = n * graphs
    pos = 32
    end = len(buf) - 8
    out = {"n": n, "graphs": graphs, "E": E, "version": version, "flags": flags, "roots": None, "others": None,
           "kept": None, "ids": None, "keys": None, "payloads": None, "root_ids": None, "kept_hashes": None,
           "sig_r": None, "tx_off": None, "tx_bytes": None}

    def take(dtype, count, shape=None):
        nonlocal pos
        a = np.frombuffer(buf, dtype, count, pos)
        pos += a.nbytes
        if pos > end:
            raise ValueError("truncated file")
        return a.reshape(shape) if shape else a

    try:
        if flags & ROOTED:
            ri, rr = take("<i4", C), take("<i4", C)
            y = take(np.uint8, (C + 3) & ~3)[:C]
            out["roots"] = (ri, rr, y)
            if version >= 2:
                no = int(take("<i8", 1)[0])
                out["others"] = take(np.uint8, 32 * no, (no, 32))
                kept = []
                for _ in range(graphs):
                    h4 = take("<i4", 4)
                    c2 = take("<i8", 2)
                    blocks = []
                    for _ in range(int(c2[1])):
                        a = take("<i4", 2)
                        t = take("<i8", 1)
                        b = take("<i4", 2)
                        blocks.append((int(a[0]), int(a[1]), int(t[0]), int(b[0]), int(b[1])))
                    kept.append(dict(has_lcr=bool(h4[0]), lcr=int(h4[1]), lcre=int(h4[2]),
                                     consensus_tx=int(c2[0]), blocks=blocks))
                out["kept"] = kept
            if v3:
                has = take(np.uint8, (2 * C + 3) & ~3)
                x_id, y_id = take(np.uint8, 32 * C, (C, 32)), take(np.uint8, 32 * C, (C, 32))
                if has[2 * C:].any():
                    raise ValueError("root id padding is not zero")
                hx, hy = has[:C], has[C:2 * C]
                if (has > 1).any():
                    raise ValueError("root id flags must be 0 or 1")
                for p in range(C):
                    if int(hy[p]) != (1 if y[p] else 0):
                        raise ValueError(f"has_y[{p}] disagrees with the root's root_y_is_event")
                    if (not hx[p] and x_id[p].any()) or (not hy[p] and y_id[p].any()):
                        raise ValueError("a root id without its flag is not zero")
                npairs = int(take("<i8", 1)[0])
                if npairs < 0:
                    raise ValueError("truncated file")
                pe, pp = take(np.uint8, 32 * npairs, (npairs, 32)), take(np.uint8, 32 * npairs, (npairs, 32))
                if pe.tobytes() != out["others"].tobytes():
                    raise ValueError("root pairs and Root.Others keys disagree")
                keys_ = [bytes(r) for r in pe]
                if any(a >= b for a, b in zip(keys_, keys_[1:])):
                    raise ValueError("root pairs are not sorted by event id")
                out["root_ids"] = ([bytes(x_id[p]) if hx[p] else None for p in range(C)],
                                   [bytes(y_id[p]) if hy[p] else None for p in range(C)],
                                   [(a, bytes(b)) for a, b in zip(keys_, pp)])
                hashes = []
                for g in range(graphs):
                    rec = take(np.uint8, 36 * len(kept[g]["blocks"]), (len(kept[g]["blocks"]), 36))
                    if (rec[:, 0] > 1).any() or rec[:, 1:4].any() or rec[rec[:, 0] == 0, 4:].any():
                        raise ValueError("bad block hash record")
                    hashes.append([bytes(r[4:]) if r[0] else None for r in rec])
                out["kept_hashes"] = hashes
        for name, dt, cnt, shp in (("creator", "<i4", E, None), ("index", "<i8", E, None),
                                   ("self_parent", "<i8", E, None), ("other_parent", "<i8", E, None),
                                   ("timestamp_ns", "<i8", E, None), ("sig_s", np.uint8, 32 * E, (E, 32)),
                                   ("coin", np.uint8, E, None), ("ntx", "<i4", E, None), ("tx_nil", np.uint8, E, None)):
            out[name] = take(dt, cnt, shp)
        if flags & IDS:
            out["ids"] = take(np.uint8, 32 * E, (E, 32))
        if flags & KEYS:
            out["keys"] = take(np.uint8, 65 * C, (C, 65))
        if v3:
            for i in range(E):
                if out["ntx"][i] < 0:
                    raise ValueError(f"negative ntx at event {i}")
                if out["tx_nil"][i] > 1 or (out["tx_nil"][i] and out["ntx"][i]):
                    raise ValueError(f"tx_nil and ntx disagree at event {i}")
                if (out["ids"][i, 16] != 0) != (out["coin"][i] != 0):
                    raise ValueError(f"event id and coin disagree at event {i}")
            out["sig_r"] = take(np.uint8, 32 * E, (E, 32))
            T = int(take("<i8", 1)[0])
            if T != int(out["ntx"].astype(np.int64).sum()):
                raise ValueError("T is not the sum of ntx")
            off = take("<i8", T + 1)
            if off[0] != 0:
                raise ValueError("tx_off must start at 0")
            if np.any(np.diff(off) < 0):
                raise ValueError("tx_off decreases")
            out["tx_off"] = off
            out["tx_bytes"] = take(np.uint8, int(off[-1])).tobytes()
        if flags & PAYLOADS:
            off = take("<i8", E + 1)
            if E >= 0 and (off[0] != 0 or np.any(np.diff(off) < 0)):
                raise ValueError("payload offsets decrease")   # (libhgx rejects the same file)
            blob = take(np.uint8, int(off[-1]) if E >= 0 else 0).tobytes()
            out["payloads"] = [blob[off[i]:off[i + 1]] for i in range(E)]
    except ValueError:
        raise
    except Exception as e:  # numpy out-of-range reads
        raise ValueError("truncated file") from e
    if pos != end:
        raise ValueError("size mismatch")
    return out
