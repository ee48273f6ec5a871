"""The event-id index without a GPU: the four symbols are exported and declared in the
ctypes binding, a NULL context and NULL columns are refused before any device call with the outputs
untouched, the Python wrappers exist, the table's contract (babble_amd/csrc/hgx_idindex.h) passes its
stand-alone check under the host sanitizers (tools/id_index_check.cpp: a sequential model over seeded
random key sets, statistics that do not depend on the insertion order, a cluster that wraps past the
last slot, the sizing rule), and tests/idindexref.py, the Python model the GPU tests compare with,
restates the same contract."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np

import idindexref
from babble_amd import _lib
from babble_amd._lib import hgx_error, ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HGX_ERR_INVALID = 102
BODY_FIELDS = ["creator", "index", "self_parent", "other_parent", "timestamp_ns", "sig_r", "sig_s", "ntx", "tx_off",
               "tx_bytes"]


def test_symbols_exported_and_declared():
    L = _lib.lib()
    E = C.POINTER(hgx_error)
    f = L.hgx_keep_id_index   # AttributeError: not exported
    assert f.restype is C.c_int32 and len(f.argtypes) == 2 and f.argtypes[-1] == E
    f = L.hgx_id_index_state
    assert f.restype is C.c_int32 and len(f.argtypes) == 3 and f.argtypes[-1] == E
    f = L.hgx_find_events
    assert f.restype is C.c_int32 and len(f.argtypes) == 5 and f.argtypes[2] is C.c_int64 and f.argtypes[-1] == E
    f = L.hgx_insert_events_by_id
    assert f.restype is C.c_int32 and len(f.argtypes) == 11 and f.argtypes[-1] == E
    assert f.argtypes[1] == C.POINTER(_lib.hgx_event_bodies) and f.argtypes[6] is C.c_int64
    assert L.hgx_abi_version() == 6
    assert [nm for nm, _ in _lib.hgx_event_bodies._fields_] == BODY_FIELDS


def _one_event():
    return dict(creator=np.zeros(1, np.int32), index=np.zeros(1, np.int64), self_parent=np.full(1, -1, np.int64),
                other_parent=np.full(1, -1, np.int64), timestamp_ns=np.zeros(1, np.int64),
                sig_r=np.zeros((1, 32), np.uint8), sig_s=np.zeros((1, 32), np.uint8), ntx=np.zeros(1, np.int32),
                tx_off=np.zeros(1, np.int64), tx_bytes=np.zeros(1, np.uint8))


def test_null_context_and_null_columns_are_invalid_before_any_device_call():
    L = _lib.lib()
    # hgx_keep_id_index / hgx_id_index_state
    err = hgx_error()
    assert L.hgx_keep_id_index(None, C.byref(err)) == HGX_ERR_INVALID == err.code
    assert err.msg == b"hgx_keep_id_index: bad arguments"
    assert L.hgx_keep_id_index(None, None) == HGX_ERR_INVALID
    st = (C.c_int64 * 5)(*([77] * 5))
    err = hgx_error()
    assert L.hgx_id_index_state(None, st, C.byref(err)) == HGX_ERR_INVALID == err.code
    assert err.msg == b"hgx_id_index_state: bad arguments" and list(st) == [77] * 5
    # hgx_find_events
    q = np.full((2, 32), 0x11, np.uint8)
    out = np.full(2, 55, np.int64)
    for count, qp, op in ((2, ptr(q), ptr(out)), (0, ptr(q), ptr(out)), (-1, ptr(q), ptr(out)), (2, None, None)):
        err = hgx_error()
        assert L.hgx_find_events(None, qp, count, op, C.byref(err)) == HGX_ERR_INVALID == err.code
        assert err.msg == b"hgx_find_events: bad arguments", err.msg
        assert (out == 55).all()
    assert L.hgx_find_events(None, ptr(q), 2, ptr(out), None) == HGX_ERR_INVALID
    # hgx_insert_events_by_id
    a = _one_event()
    ids, spi, opi = (np.full((1, 32), v, np.uint8) for v in (1, 2, 3))
    flags = np.full(1, 3, np.uint8)
    sp, op = np.full(1, 77, np.int64), np.full(1, 78, np.int64)

    def call(ctx, ev, cl=ptr(ids), fl=ptr(flags), count=1):
        err, n_ins = hgx_error(), C.c_int64(55)
        rc = L.hgx_insert_events_by_id(ctx, ev, cl, ptr(spi), ptr(opi), fl, count, ptr(sp), ptr(op), C.byref(n_ins),
                                       C.byref(err))
        assert rc == HGX_ERR_INVALID == err.code and err.msg.startswith(b"hgx_insert_events_by_id: "), err.msg
        assert n_ins.value == 0 and sp[0] == 77 and op[0] == 78
        return err.msg.decode()

    full = _lib.hgx_event_bodies(*[ptr(a[nm]) for nm in BODY_FIELDS])
    assert call(None, C.byref(full)) == "hgx_insert_events_by_id: bad arguments"
    assert call(None, None) == "hgx_insert_events_by_id: bad arguments"
    assert call(None, C.byref(full), count=-1) == "hgx_insert_events_by_id: bad arguments"
    assert call(None, C.byref(full), cl=None) == "hgx_insert_events_by_id: bad arguments"
    assert call(None, C.byref(full), fl=None) == "hgx_insert_events_by_id: bad arguments"
    assert L.hgx_insert_events_by_id(None, C.byref(full), ptr(ids), None, None, ptr(flags), 1, None, None, None,
                                     None) == HGX_ERR_INVALID


def test_python_wrappers_exist():
    from babble_amd import hashgraph
    for nm in ("KeepIdIndex", "IdIndexState", "FindEvents", "insert_events_by_id"):
        assert callable(getattr(hashgraph.Hashgraph, nm)), nm
    from babble_amd import build
    assert "hgx_idindex.hip" in build.SOURCES


def test_contract_stand_alone_check_under_the_host_sanitizers(tmp_path):
    """hgx_idindex.h's host side is plain C++ with no HIP and no context, so a program with its own main
    checks it, compiled with -fsanitize=address,undefined."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        assert os.path.exists(hipcc), "no C++ compiler found"
        cxx = hipcc
    exe = str(tmp_path / "id_index_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "babble_amd", "csrc"),
                           os.path.join(ROOT, "tools", "id_index_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"id index: (\d+) random key sets ok \((\d+) with a wrapped cluster\), sizing, wrap, full table ok",
                  r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) >= 300 and int(m.group(2)) > 20


def test_python_model_restates_the_contract():
    assert [idindexref.slots_for(c) for c in (1, 2, 3, 63, 64, 65)] == [2, 4, 8, 128, 128, 256]
    ident = np.arange(1, 33, dtype=np.uint8)
    assert idindexref.home(ident, 1 << 16) == 0x0201 and idindexref.tag(ident) == 0x0C0B0A09
    # the cluster of tools/id_index_check.cpp: five keys at home 6 of 8 slots, then one at home 0
    m = idindexref.Model(4)
    assert m.slots == 8
    keys = []
    for k in range(5):
        r = idindexref.forge_home(6, salt=k)
        keys.append(r)
        assert m.insert(r) == k
    keys.append(idindexref.forge_home(0, salt=9))
    m.insert(keys[5])
    assert [w != 0 for w in m.tab] == [True, True, True, True, False, False, True, True]
    assert m.state() == dict(kept=1, slots=8, entries=6, total_displacement=13, wrapped=3)
    assert [m.find(r) for r in keys] == list(range(6))
    assert m.find(idindexref.forge_home(7, salt=77)) == -1
    assert m.find(idindexref.forge_same_home_and_tag(keys[2])) == -1
    # a repeated key answers with its lowest gid; the statistics do not depend on the insertion order
    m.insert(keys[1])
    assert m.find(keys[1]) == 1
    rng = np.random.default_rng(5)
    ids = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    ids[:, :8] = 0
    ids[:, 0] = 120 + rng.integers(0, 8, 40)   # homes 120..127 of 128 slots: the cluster wraps
    a = idindexref.model_of(ids, 64).state()
    b = idindexref.model_of(ids[rng.permutation(40)], 64).state()
    assert a == b and a["wrapped"] >= 1 and a["entries"] == 40
