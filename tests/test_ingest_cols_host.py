"""The host column forms without a GPU. babble_amd/csrc/hgx_ingest_cols.h is the one table of the wide,
compact and packed forms; tools/ingest_cols_check.cpp, a program with its own main and
no HIP, prints it, and the figures and orders are compared here with the documented ones: bytes per
event, the order of the copies of a split insert, the order of a batch staged whole, the late payload
stage, and the one-copy layout of sync-sized batches. The six entry points that take those columns
refuse a NULL context, struct or column, a negative count and a bad exception list before any device
call, with their messages unchanged."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from babble_amd import _lib
from babble_amd._lib import hgx_error, ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HGX_ERR_INVALID = 102

# bytes per event: structure, payload, total; the packed form adds 16 per exception
BYTES = {"wide": (28, 80, 108), "compact": (16, 45, 61), "packed": (10, 45, 55)}
EXC_BYTES = {"wide": 0, "compact": 0, "packed": 16}
# a split insert: the structure's copies, then the payload's (S of the compact payload last)
SPLIT = {
    "wide": (["creator", "index", "sp", "op"], ["ts", "hash", "S", "ntx", "nil"]),
    "compact": (["creator", "index32", "sp32", "op32"], ["ts", "coin", "ntx", "S"]),
    "packed": (["creator16", "index32", "sp_back", "op_back", "exc_pos", "exc_sp", "exc_op"], ["ts", "coin", "ntx", "S"]),
}
# a batch staged whole (the one pinned copy of at most 65 536 events)
WHOLE = {
    "wide": ["creator", "index", "sp", "op", "ts", "hash", "S", "ntx", "nil"],
    "compact": ["creator", "index32", "sp32", "op32", "ts", "coin", "S", "ntx"],
    "packed": ["creator16", "index32", "sp_back", "op_back", "ts", "coin", "S", "ntx", "exc_pos", "exc_sp", "exc_op"],
}
LATE = {"wide": [], "compact": ["S"], "packed": ["S"]}   # (the packed form's payload is the compact one)
WIDTH = {"creator": 4, "index": 8, "sp": 8, "op": 8, "ts": 8, "hash": 32, "S": 32, "ntx": 4, "nil": 4, "index32": 4,
         "sp32": 4, "op32": 4, "coin": 1, "creator16": 2, "sp_back": 2, "op_back": 2, "exc_pos": 8, "exc_sp": 4,
         "exc_op": 4}


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        assert os.path.exists(hipcc), "no C++ compiler found"
        cxx = hipcc
    exe = str(tmp_path_factory.mktemp("ingest_cols") / "ingest_cols_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "babble_amd", "csrc"),
                           os.path.join(ROOT, "tools", "ingest_cols_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    out = {}
    for ln in r.stdout.splitlines()[:-1]:
        w = ln.split()
        out.setdefault(w[0], {}).setdefault(w[1], []).append(w[2:])
    return out


@pytest.mark.parametrize("form", ["wide", "compact", "packed"])
def test_bytes_per_event(table, form):
    (w,) = table["bytes"][form]
    got = dict(zip(w[0::2], map(int, w[1::2])))
    assert (got["structure"], got["payload"], got["structure"] + got["payload"]) == BYTES[form]
    assert got["exception"] == EXC_BYTES[form]


@pytest.mark.parametrize("form", ["wide", "compact", "packed"])
def test_column_order_and_late_stage(table, form):
    (w,) = table["split"][form]
    cols = [x.split(":") for x in w]
    structure = [nm for nm, _, kind in cols if kind in ("structure", "exception")]
    payload = [nm for nm, _, kind in cols if kind in ("payload", "late")]
    assert [nm for nm, _, _ in cols] == structure + payload   # the structure's copies come first
    assert (structure, payload) == SPLIT[form]
    assert all(int(b) == WIDTH[nm] for nm, b, _ in cols)
    assert [nm for nm, _, kind in cols if kind == "exception"] == [nm for nm in structure if nm.startswith("exc_")]
    (whole,) = table["whole"][form]
    assert whole == WHOLE[form]
    (late,) = table["late"][form]
    assert late == LATE[form] == [nm for nm, _, kind in cols if kind == "late"]


@pytest.mark.parametrize("form", ["wide", "compact", "packed"])
def test_one_copy_layout(table, form):
    """Offsets follow the whole-batch order, are 256-byte aligned, and the columns do not overlap."""
    seen = set()
    for w in table["layout"][form]:
        count, n_exc, total = int(w[0]), int(w[1]), int(w[2])
        seen.add((count, n_exc))
        cols = {nm: (int(off), int(b)) for nm, off, b in (x.split(":") for x in w[3:])}
        end = 0
        for nm in WHOLE[form]:
            off, b = cols[nm]
            assert b == WIDTH[nm] * (n_exc if nm.startswith("exc_") else count), (nm, count, n_exc)
            assert off % 256 == 0 and off >= end, (nm, count, n_exc)   # aligned, behind the column before it
            assert off == (end + 255) // 256 * 256   # ... and no further
            end = off + b
        assert total >= end and total % 256 == 0 and total - end < 256
    want = {(c, x) for c in (1, 1000, 65536) for x in ((0, 3) if form == "packed" else (0,))}
    assert seen == want


def _columns(count=4):
    a = dict(creator=np.zeros(count, np.int32), index=np.zeros(count, np.int64), sp=np.full(count, -1, np.int64),
             op=np.full(count, -1, np.int64), ts=np.zeros(count, np.int64), hash=np.zeros((count, 32), np.uint8),
             s=np.zeros((count, 32), np.uint8), ntx=np.zeros(count, np.int32), nil=np.zeros(count, np.int32),
             index32=np.zeros(count, np.int32), sp32=np.full(count, -1, np.int32), op32=np.full(count, -1, np.int32),
             coin=np.zeros(count, np.uint8), c16=np.zeros(count, np.uint16), spb=np.zeros(count, np.uint16),
             opb=np.zeros(count, np.uint16), exc_pos=np.zeros(count + 1, np.int64), exc_sp=np.zeros(count + 1, np.int32),
             exc_op=np.zeros(count + 1, np.int32))
    return a


FORMS = {
    "wide": (_lib.hgx_events, ["creator", "index", "sp", "op", "ts", "hash", "s", "ntx", "nil"],
             ["hgx_insert_events", "hgx_insert_and_run"]),
    "compact": (_lib.hgx_events32, ["creator", "index32", "sp32", "op32", "ts", "coin", "s", "ntx"],
                ["hgx_insert_events32", "hgx_insert_and_run32"]),
    "packed": (_lib.hgx_events_packed, ["c16", "index32", "spb", "opb", "n_exc", "exc_pos", "exc_sp", "exc_op", "ts", "coin",
                                        "s", "ntx"],
               ["hgx_insert_events_packed", "hgx_insert_and_run_packed"]),
}


@pytest.mark.parametrize("form", ["wide", "compact", "packed"])
def test_refusals_before_any_device_call(form):
    L = _lib.lib()
    struct, fields, names = FORMS[form]
    a = _columns()

    def build(null=None, n_exc=0):
        return struct(*[n_exc if nm == "n_exc" else None if nm == null else ptr(a[nm]) for nm in fields])

    for name in names:
        fn = getattr(L, name)

        def refused(ev, count=4):
            err, n_ins = hgx_error(), C.c_int64(55)
            rc = fn(None, None if ev is None else C.byref(ev), count, C.byref(n_ins), C.byref(err))
            assert rc == HGX_ERR_INVALID == err.code and n_ins.value == 0
            assert err.msg.decode() == name + ": bad arguments"

        refused(build())   # (the NULL context)
        refused(None)
        refused(build(), count=-1)
        for nm in fields:
            if nm != "n_exc" and not nm.startswith("exc_"):
                refused(build(null=nm))
        if form == "packed":
            refused(build(n_exc=5))   # more exceptions than events
            a["exc_pos"][:2] = 1
            refused(build(n_exc=2))   # a position twice
            for nm in ("exc_pos", "exc_sp", "exc_op"):
                refused(build(null=nm, n_exc=1))
        assert fn(None, None, 0, None, None) == HGX_ERR_INVALID   # errors and outputs are optional
