"""Checkpoints with event bodies without a GPU: the new symbols are exported and declared,
the ABI is still 6, NULL contexts are refused before any device call, checkpoint.encode / read round-trip
version 3 and refuse what the library refuses, and the host side (hgx_ckpt_host.cpp: the version-3 parser,
validator and piece planner) passes its stand-alone check, tools/ckpt_host_check.cpp."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from babble_amd import _lib, checkpoint
from babble_amd._lib import hgx_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HGX_ERR_INVALID = 102
ARITY = dict(hgx_insert_event_bodies_claimed=7, hgx_save_bodies=3)


def test_symbols_exported_and_declared():
    L = _lib.lib()
    for name, arity in ARITY.items():
        f = getattr(L, name)   # AttributeError: not exported
        assert f.restype is C.c_int32 and len(f.argtypes) == arity, name
        assert f.argtypes[-1] == C.POINTER(hgx_error), name
    assert L.hgx_abi_version() == 6
    header = open(os.path.join(ROOT, "include", "hgx.h")).read()
    for name in ARITY:
        assert f"int32_t {name}(hgx_ctx* ctx," in header, name


def test_null_context_is_refused_before_any_device_call(tmp_path):
    L = _lib.lib()
    err = hgx_error()
    p = os.fsencode(str(tmp_path / "x.ckpt"))
    assert L.hgx_save_bodies(None, p, C.byref(err)) == HGX_ERR_INVALID
    assert err.code == HGX_ERR_INVALID and err.msg == b"hgx_save_bodies: bad arguments"
    assert L.hgx_save_bodies(None, p, None) == HGX_ERR_INVALID   # errors are optional
    assert not os.path.exists(p)
    assert L.hgx_bootstrap(None, p, C.byref(err)) == HGX_ERR_INVALID
    # the claimed insert: columns of one event, no context; then a NULL claimed column
    one32, one64 = (C.c_int32 * 1)(0), (C.c_int64 * 1)(-1)
    idx, ts, ntx, off = (C.c_int64 * 1)(0), (C.c_int64 * 1)(1), (C.c_int32 * 1)(-1), (C.c_int64 * 1)(0)
    sig, by = (C.c_uint8 * 32)(), (C.c_uint8 * 1)()
    v = lambda a: C.cast(a, C.c_void_p)
    ev = _lib.hgx_event_bodies(v(one32), v(idx), v(one64), v(one64), v(ts), v(sig), v(sig), v(ntx), v(off), v(by))
    claimed = (C.c_uint8 * 32)(*([0xA5] * 32))
    n_ins = C.c_int64(7)
    rc = L.hgx_insert_event_bodies_claimed(None, C.byref(ev), claimed, None, 1, C.byref(n_ins), C.byref(err))
    assert rc == HGX_ERR_INVALID and err.msg == b"hgx_insert_event_bodies_claimed: bad arguments" and n_ins.value == 0
    rc = L.hgx_insert_event_bodies_claimed(None, C.byref(ev), None, None, 1, C.byref(n_ins), C.byref(err))
    assert rc == HGX_ERR_INVALID and err.msg == b"hgx_insert_event_bodies_claimed: bad arguments"
    assert L.hgx_insert_event_bodies_claimed(None, None, claimed, None, 0, None, None) == HGX_ERR_INVALID
    assert list(claimed) == [0xA5] * 32


def test_python_wrappers_exist():
    from babble_amd.hashgraph import Hashgraph
    for name in ("insert_bodies_claimed", "save_bodies", "Bootstrap"):
        assert callable(getattr(Hashgraph, name)), name


# ---- checkpoint.py, version 3 --------------------------------------------------------------------------
def _events(E, C, seed):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, 256, (E, 32), dtype=np.uint8)
    txs = [None if k % 5 == 0 else [rng.integers(0, 256, int(L), dtype=np.uint8).tobytes() for L in rng.integers(0, 9, k % 4)]
           for k in range(E)]
    return dict(creator=rng.integers(0, C, E), index=np.arange(E), sp=np.arange(E) - 1, op=np.full(E, -1),
                ts=1_500_000_000_000_000_000 + np.arange(E), sig_s=rng.integers(0, 256, (E, 32), dtype=np.uint8),
                coin=ids[:, 16] != 0, ntx=[len(x or []) for x in txs], tx_nil=[x is None for x in txs]), ids, txs, \
        rng.integers(0, 256, (E, 32), dtype=np.uint8), rng.integers(0, 256, (C, 65), dtype=np.uint8)


def _file(tmp_path, rooted, **repl):
    n, E = 4, 23
    cols, ids, txs, sig_r, keys = _events(E, n, 9)
    a = dict(ids=ids, keys=keys, bodies=(sig_r, txs))
    want = dict(sig_r=sig_r, txs=txs, ids=ids)
    if rooted:
        x = [ids[1].tobytes(), None, None, ids[2].tobytes()]
        y = [None, ids[3].tobytes(), None, None]
        pairs = [(ids[7].tobytes(), ids[4].tobytes()), (ids[6].tobytes(), ids[5].tobytes())]
        kept = [dict(has_lcr=True, lcr=3, lcre=5, consensus_tx=11, blocks=[(1, 2, 3, 0, 1), (2, 3, 0, 1, 1), (3, 1, 1, 0, 0)])]
        a.update(roots=([1, 0, -1, 2], [0, 0, -1, 1], [0, 1, 0, 0]), kept=kept, root_ids=(x, y, pairs),
                 kept_hashes=[[ids[8].tobytes(), None, ids[9].tobytes()]])
        want.update(root_ids=(x, y, sorted(pairs)), kept_hashes=a["kept_hashes"], kept=kept)
    a.update(repl)
    data = checkpoint.encode(n, 1, cols["creator"], cols["index"], cols["sp"], cols["op"], cols["ts"], cols["sig_s"],
                             cols["coin"], cols["ntx"], cols["tx_nil"], **a)
    p = str(tmp_path / "f.ckpt")
    with open(p, "wb") as f:
        f.write(data)
    return p, data, want


@pytest.mark.parametrize("rooted", [False, True])
def test_encode_read_round_trip(tmp_path, rooted):
    p, data, want = _file(tmp_path, rooted)
    r = checkpoint.read(p)
    assert r["version"] == 3 and r["flags"] == 2 | 4 | 16 | (1 if rooted else 0) and r["payloads"] is None
    assert np.array_equal(r["sig_r"], want["sig_r"]) and np.array_equal(r["ids"], want["ids"])
    flat = [b for x in want["txs"] for b in (x or [])]
    assert r["tx_bytes"] == b"".join(flat) and list(np.diff(r["tx_off"])) == [len(b) for b in flat] and r["tx_off"][0] == 0
    if rooted:
        assert r["root_ids"] == want["root_ids"] and r["kept_hashes"] == want["kept_hashes"] and r["kept"] == want["kept"]
        assert r["others"].tobytes() == b"".join(a for a, _ in want["root_ids"][2])
    else:
        assert r["root_ids"] is None and r["kept_hashes"] is None
    # version 2 is what it was: no bodies, the old version number
    v2 = checkpoint.encode(4, 1, [0], [0], [-1], [-1], [1], np.zeros((1, 32), np.uint8), [0], [0], [0])
    assert int(np.frombuffer(v2, "<u4", 1, 8)[0]) == 2
    with pytest.raises(ValueError):
        checkpoint.encode(4, 1, [0], [0], [-1], [-1], [1], np.zeros((1, 32), np.uint8), [0], [0], [0],
                          bodies=(np.zeros((1, 32), np.uint8), [None]))   # (no ids, no keys)


def _closed(body):
    return body + np.array([checkpoint.fnv1a(body)], "<u8").tobytes()


def _read_refuses(tmp_path, data, why):
    p = str(tmp_path / "bad.ckpt")
    with open(p, "wb") as f:
        f.write(data)
    with pytest.raises(ValueError) as ei:
        checkpoint.read(p)
    assert str(ei.value) == why


def test_read_refuses_what_the_library_refuses(tmp_path):
    n, E = 4, 23
    p, data, want = _file(tmp_path, False)
    at_T = 32 + E * (4 + 8 * 4 + 32 + 1 + 4 + 1) + 32 * E + 65 * n + 32 * E
    T = int(np.frombuffer(data, "<i8", 1, at_T)[0])
    assert T == sum(len(x or []) for x in want["txs"]) >= 3
    last = int(np.frombuffer(data, "<i8", 1, at_T + 8 + 8 * T)[0])

    def patched(pos, new):
        return _closed(data[:pos] + new + data[pos + len(new):-8])

    _read_refuses(tmp_path, patched(at_T, np.array([T + 1], "<i8").tobytes()), "T is not the sum of ntx")
    _read_refuses(tmp_path, patched(at_T + 16, np.array([last + 1], "<i8").tobytes()), "tx_off decreases")
    _read_refuses(tmp_path, patched(at_T + 8, np.array([1], "<i8").tobytes()), "tx_off must start at 0")
    _read_refuses(tmp_path, patched(20, np.array([2 | 4 | 16 | 8], "<i4").tobytes()), "unsupported flags")
    _read_refuses(tmp_path, patched(20, np.array([2 | 16], "<i4").tobytes()), "unsupported flags")
    _read_refuses(tmp_path, _closed(data[:-8] + b"\0"), "size mismatch")
    _read_refuses(tmp_path, _closed(data[:-9]), "truncated file")
    _read_refuses(tmp_path, data[:-1] + bytes([data[-1] ^ 1]), "checksum mismatch")
    # a rooted file whose pairs are not its Root.Others keys
    _, _, want = _file(tmp_path, True)
    others = np.frombuffer(b"".join(a for a, _ in want["root_ids"][2]), np.uint8).reshape(-1, 32).copy()
    others[1, 0] ^= 1
    _, bad, _ = _file(tmp_path, True, others=others)
    _read_refuses(tmp_path, bad, "root pairs and Root.Others keys disagree")


# ---- the host side as a program of its own -------------------------------------------------------------
def test_host_side_stand_alone_check(tmp_path):
    """The parser, the validator and the piece planner are plain C++ with no HIP and no context, so a program
    with its own main checks them (built here without a sanitizer; the same program is meant for
    -fsanitize=address,undefined)."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        assert os.path.exists(hipcc), "no C++ compiler found"
        cxx = hipcc
    exe = str(tmp_path / "ckpt_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "babble_amd", "csrc"),
                           os.path.join(ROOT, "tools", "ckpt_host_check.cpp"),
                           os.path.join(ROOT, "babble_amd", "csrc", "hgx_ckpt_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "24 images ok" in r.stdout
