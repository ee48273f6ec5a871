"""The resident body store without a GPU: every new symbol is exported and declared in the ctypes
binding, hgx_wire_body_out has its five fields, the ABI is still 6, NULL contexts are refused before any
device call with the outputs untouched, the Python wrappers exist, and the host side
(hgx_bodystore_host.cpp: growth plan, capacity rule, argument check, the block-text sizing formula)
passes its stand-alone check, tools/bodystore_host_check.cpp."""
import ctypes as C
import os
import shutil
import subprocess

from babble_amd import _lib
from babble_amd._lib import hgx_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HGX_ERR_INVALID = 102
ARITY = dict(hgx_keep_bodies=4, hgx_bodies_state=4, hgx_get_event_bodies=12, hgx_block_transactions=10,
             hgx_diff_wire_bodies=12, hgx_get_block_hash=5, hgx_block_hash_batch=9)


def test_symbols_exported_and_declared():
    L = _lib.lib()
    for name, arity in ARITY.items():
        f = getattr(L, name)   # AttributeError: not exported
        assert f.restype is C.c_int32 and len(f.argtypes) == arity, name
        if name != "hgx_bodies_state":
            assert f.argtypes[-1] == C.POINTER(hgx_error), name
    assert L.hgx_abi_version() == 6
    assert [nm for nm, _ in _lib.hgx_wire_body_out._fields_] == ["sig_r", "tx_off", "tx_cap", "tx_bytes", "bytes_cap"]
    assert C.sizeof(_lib.hgx_wire_body_out) == 5 * 8


def test_null_context_is_refused_before_any_device_call():
    L = _lib.lib()
    err = hgx_error()
    assert L.hgx_keep_bodies(None, 0, 0, C.byref(err)) == HGX_ERR_INVALID
    assert err.code == HGX_ERR_INVALID and err.msg.startswith(b"hgx_keep_bodies: ")
    assert L.hgx_keep_bodies(None, 0, 0, None) == HGX_ERR_INVALID   # errors are optional
    ne, nt, nb = C.c_int64(7), C.c_int64(8), C.c_int64(9)
    assert L.hgx_bodies_state(None, C.byref(ne), C.byref(nt), C.byref(nb)) == 0
    assert (ne.value, nt.value, nb.value) == (7, 8, 9)
    gids = (C.c_int64 * 2)(0, 1)
    r, ntx = (C.c_uint8 * 64)(*([0xA5] * 64)), (C.c_int32 * 2)(77, 77)
    off, by = (C.c_int64 * 4)(-7, -7, -7, -7), (C.c_uint8 * 8)(*([0xA5] * 8))
    n_tx, n_bytes = C.c_int64(7), C.c_int64(9)
    rc = L.hgx_get_event_bodies(None, gids, 2, r, ntx, off, 3, by, 8, C.byref(n_tx), C.byref(n_bytes), C.byref(err))
    assert rc == HGX_ERR_INVALID and err.msg.startswith(b"hgx_get_event_bodies:")
    rc = L.hgx_block_transactions(None, 0, 0, off, 3, by, 8, C.byref(n_tx), C.byref(n_bytes), C.byref(err))
    assert rc == HGX_ERR_INVALID and err.msg.startswith(b"hgx_block_transactions:")
    h32 = (C.c_uint8 * 32)(*([0xA5] * 32))
    rc = L.hgx_get_block_hash(None, 0, 0, h32, C.byref(err))
    assert rc == HGX_ERR_INVALID and err.msg.startswith(b"hgx_get_block_hash:") and list(h32) == [0xA5] * 32
    # the encoder alone: bad arguments are refused before the device is looked for; the empty batch is fine
    rr, ntx1, nil1 = (C.c_int64 * 1)(1), (C.c_int32 * 1)(-1), (C.c_int32 * 1)(0)
    rc = L.hgx_block_hash_batch(0, rr, ntx1, nil1, None, None, 1, h32, C.byref(err))
    assert rc == HGX_ERR_INVALID and err.msg.startswith(b"hgx_block_hash_batch:") and list(h32) == [0xA5] * 32
    assert L.hgx_block_hash_batch(0, None, None, None, None, None, 1, h32, None) == HGX_ERR_INVALID
    assert L.hgx_block_hash_batch(0, None, None, None, None, None, 0, None, C.byref(err)) == 0
    known = (C.c_int32 * 4)(-1, -1, -1, -1)
    out = _lib.hgx_wire_out()
    body = _lib.hgx_wire_body_out(C.cast(r, C.c_void_p), C.cast(off, C.c_void_p), 3, C.cast(by, C.c_void_p), 8)
    cnt, over = C.c_int64(5), C.c_int32(6)
    rc = L.hgx_diff_wire_bodies(None, 0, known, -1, C.byref(out), C.byref(body), 2, C.byref(cnt), C.byref(n_tx),
                                C.byref(n_bytes), C.byref(over), C.byref(err))
    assert rc == HGX_ERR_INVALID and err.msg.startswith(b"hgx_diff_wire_bodies:")
    assert (n_tx.value, n_bytes.value, cnt.value, over.value) == (7, 9, 5, 6)   # nothing written
    assert list(r) == [0xA5] * 64 and list(ntx) == [77, 77] and list(off) == [-7] * 4 and list(by) == [0xA5] * 8
    assert L.hgx_diff_wire_bodies(None, 0, known, -1, C.byref(out), None, 0, C.byref(cnt), C.byref(n_tx),
                                  C.byref(n_bytes), None, None) == HGX_ERR_INVALID


def test_python_wrappers_exist():
    from babble_amd.hashgraph import Hashgraph
    from babble_amd import hashgraph
    for name in ("KeepBodies", "BodiesState", "EventBodies", "BlockHash", "BlockTransactions", "DiffWireBodies"):
        assert callable(getattr(Hashgraph, name)), name
    assert callable(hashgraph.block_hash_batch)


def test_host_side_stand_alone_check(tmp_path):
    """The host side is plain C++ with no HIP and no context, so a program with its own main checks it
    (built here without a sanitizer; the same program is meant for -fsanitize=address,undefined)."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        assert os.path.exists(hipcc), "no C++ compiler found"
        cxx = hipcc
    exe = str(tmp_path / "bodystore_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "babble_amd", "csrc"),
                           os.path.join(ROOT, "tools", "bodystore_host_check.cpp"),
                           os.path.join(ROOT, "babble_amd", "csrc", "hgx_bodystore_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "400 cases ok" in r.stdout
