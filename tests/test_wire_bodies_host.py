"""hgx_insert_wire_bodies without a GPU: the symbol is exported and declared in the ctypes binding, a
NULL context and NULL columns are refused before any device call with the outputs untouched, the
Python wrapper exists, and the host plan (ReadWireInfo for a whole batch, hgx_wire_plan_host.cpp)
passes its stand-alone check: tools/wire_plan_check.cpp, 480 seeded random cases against a direct
restatement of hashgraph.go:569-614 over common/rolling_index.go:40-50 (empty chains, forward
references, both panics, Too Late on shortened chains, levels by hgx_batch_levels' rule)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np

from babble_amd import _lib
from babble_amd._lib import hgx_error, ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HGX_ERR_INVALID = 102
FIELDS = ["creator_id", "index", "self_parent_index", "other_parent_creator", "other_parent_index", "timestamp_ns",
          "sig_r", "sig_s", "ntx", "tx_off", "tx_bytes"]


def test_symbol_exported_and_declared():
    L = _lib.lib()
    f = L.hgx_insert_wire_bodies   # AttributeError: not exported
    assert f.restype is C.c_int32 and len(f.argtypes) == 8 and f.argtypes[-1] == C.POINTER(hgx_error)
    assert f.argtypes[1] == C.POINTER(_lib.hgx_wire_bodies)
    assert L.hgx_abi_version() == 6
    assert [nm for nm, _ in _lib.hgx_wire_bodies._fields_] == FIELDS
    assert C.sizeof(_lib.hgx_wire_bodies) == 11 * C.sizeof(C.c_void_p)
    # hgx_diff_wire's answer carries the first six fields and S under the same names
    out = [nm for nm, _ in _lib.hgx_wire_out._fields_]
    assert all(nm in out for nm in FIELDS[:6] + ["sig_s", "ntx"])


def _one_event():
    a = dict(creator_id=np.zeros(1, np.int32), index=np.zeros(1, np.int64), self_parent_index=np.full(1, -1, np.int64),
             other_parent_creator=np.zeros(1, np.int32), other_parent_index=np.full(1, -1, np.int64),
             timestamp_ns=np.zeros(1, np.int64), sig_r=np.zeros((1, 32), np.uint8), sig_s=np.zeros((1, 32), np.uint8),
             ntx=np.zeros(1, np.int32), tx_off=np.zeros(1, np.int64), tx_bytes=np.zeros(1, np.uint8))
    return a


def test_null_context_and_null_columns_are_invalid_before_any_device_call():
    L = _lib.lib()
    a = _one_event()
    ids = np.full((1, 32), 0x5A, np.uint8)
    sp, op = np.full(1, 77, np.int64), np.full(1, 78, np.int64)

    def call(ctx, ev, count=1):
        err, n_ins = hgx_error(), C.c_int64(55)
        rc = L.hgx_insert_wire_bodies(ctx, ev, count, ptr(ids), ptr(sp), ptr(op), C.byref(n_ins), C.byref(err))
        assert rc == HGX_ERR_INVALID == err.code and err.msg.startswith(b"hgx_insert_wire_bodies: "), err.msg
        assert n_ins.value == 0 and (ids == 0x5A).all() and sp[0] == 77 and op[0] == 78
        return err.msg.decode()

    full = _lib.hgx_wire_bodies(*[ptr(a[nm]) for nm in FIELDS])
    assert call(None, C.byref(full)) == "hgx_insert_wire_bodies: bad arguments"
    assert call(None, None) == "hgx_insert_wire_bodies: bad arguments"
    assert call(None, C.byref(full), count=-1) == "hgx_insert_wire_bodies: bad arguments"
    for nm in FIELDS[:-1]:   # (tx_bytes may be NULL while no transaction has bytes)
        ev = _lib.hgx_wire_bodies(*[None if x == nm else ptr(a[x]) for x in FIELDS])
        assert call(None, C.byref(ev)) == "hgx_insert_wire_bodies: null column", nm
    bad = dict(a, ntx=np.full(1, -2, np.int32))
    ev = _lib.hgx_wire_bodies(*[ptr(bad[nm]) for nm in FIELDS])
    assert call(None, C.byref(ev)) == "hgx_insert_wire_bodies: ntx below -1"   # the columns come before the context
    # errors and outputs are optional
    assert L.hgx_insert_wire_bodies(None, C.byref(full), 1, None, None, None, None, None) == HGX_ERR_INVALID


def test_python_wrapper_exists():
    from babble_amd import hashgraph
    assert callable(getattr(hashgraph.Hashgraph, "insert_wire_bodies"))
    rows = dict(creator_id=[1, 0], index=[0, 0], self_parent_index=[-1, -1], other_parent_creator=[-1, 1],
                other_parent_index=[-1, 0], timestamp_ns=[5, 6], sig_s=np.ones((2, 32), np.uint8))
    w = hashgraph.wire_body_columns(rows, np.zeros((2, 32), np.uint8), [None, [b"ab", b""]])
    assert sorted(w) == sorted(FIELDS)
    assert w["creator_id"].dtype == np.int32 and w["other_parent_creator"].dtype == np.int32
    assert w["other_parent_index"].dtype == np.int64 and list(w["ntx"]) == [-1, 2] and list(w["tx_off"]) == [0, 2, 2]
    a, ev = hashgraph._wire_bodies_of(w, 1, 2)
    assert list(a["tx_off"]) == [0, 2, 2] and list(a["creator_id"]) == [0] and isinstance(ev, _lib.hgx_wire_bodies)


def test_host_plan_stand_alone_check(tmp_path):
    """The plan is plain C++ with no HIP and no context, so a program with its own main checks it
    (built here without a sanitizer; the same program is meant for -fsanitize=address,undefined)."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        assert os.path.exists(hipcc), "no C++ compiler found"
        cxx = hipcc
    exe = str(tmp_path / "wire_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "babble_amd", "csrc"), os.path.join(ROOT, "tools", "wire_plan_check.cpp"),
                           os.path.join(ROOT, "babble_amd", "csrc", "hgx_wire_plan_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) cases ok \((\d+) clean, (\d+) too late \((\d+) on shortened chains\), (\d+) not found "
                  r"\((\d+) forward references\), (\d+) \+ (\d+) panics, (\d+) with empty chains", r.stdout)
    assert m, r.stdout
    cases, clean, late, late_short, nf, fwd, p1, p2, empty = map(int, m.groups())
    assert cases >= 400 and min(clean, late, late_short, nf, fwd, p1, p2, empty) > 0
