"""hgx_diff_wire without a GPU: the symbol is exported and declared in the ctypes binding, a NULL
context (and every other NULL argument) is refused before any device call, the Python wrapper
exists, and the host plan (Core.OverSyncLimit and the sizes of Core.Diff, hgx_diff_host.cpp) passes
its stand-alone check: tools/diff_host_check.cpp, 400 seeded random cases against a direct
restatement of node/core.go:147-188 over common/rolling_index.go:21-39."""
import ctypes as C
import os
import shutil
import subprocess

from babble_amd import _lib
from babble_amd._lib import hgx_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HGX_ERR_INVALID = 102


def test_symbol_exported_and_declared():
    L = _lib.lib()
    f = L.hgx_diff_wire   # AttributeError: not exported
    assert f.restype is C.c_int32 and len(f.argtypes) == 9 and f.argtypes[-1] == C.POINTER(hgx_error)
    assert L.hgx_abi_version() == 6
    names = [nm for nm, _ in _lib.hgx_wire_out._fields_]
    assert names == ["gid", "creator_id", "index", "self_parent_index", "other_parent_creator", "other_parent_index",
                     "timestamp_ns", "hash", "sig_s", "ntx", "tx_nil", "root_parent"]
    assert C.sizeof(_lib.hgx_wire_out) == 12 * C.sizeof(C.c_void_p)
    # the first ten columns after gid are hgx_wire_events' (the peer's insert takes them as they are)
    assert names[1:11] == [nm for nm, _ in _lib.hgx_wire_events._fields_]


def test_null_context_is_invalid_before_any_device_call():
    L = _lib.lib()
    err = hgx_error()
    known = (C.c_int32 * 4)(-1, -1, -1, -1)
    out = _lib.hgx_wire_out()
    cnt, over = C.c_int64(7), C.c_int32(9)
    rc = L.hgx_diff_wire(None, 0, known, -1, C.byref(out), 0, C.byref(cnt), C.byref(over), C.byref(err))
    assert rc == HGX_ERR_INVALID and err.code == HGX_ERR_INVALID and err.msg.startswith(b"hgx_diff_wire:")
    assert cnt.value == 7 and over.value == 9   # nothing written
    # errors are optional
    assert L.hgx_diff_wire(None, 0, known, -1, C.byref(out), 0, C.byref(cnt), None, None) == HGX_ERR_INVALID


def test_python_wrapper_exists():
    from babble_amd.hashgraph import Hashgraph
    assert callable(getattr(Hashgraph, "DiffWire"))
    assert len(_lib.WIRE_OUT_COLUMNS) == 12


def test_host_plan_stand_alone_check(tmp_path):
    """The plan is plain C++ with no HIP and no context, so a program with its own main checks it
    (built here without a sanitizer; the same program is meant for -fsanitize=address,undefined)."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        assert os.path.exists(hipcc), "no C++ compiler found"
        cxx = hipcc
    exe = str(tmp_path / "diff_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "babble_amd", "csrc"), os.path.join(ROOT, "tools", "diff_host_check.cpp"),
                           os.path.join(ROOT, "babble_amd", "csrc", "hgx_diff_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "400 cases ok" in r.stdout
