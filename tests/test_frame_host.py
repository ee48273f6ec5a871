"""hgx_get_frame_bodies without a GPU: the symbol is exported and declared in the ctypes binding with
its seven arguments, hgx_frame_out mirrors the header's field order, a NULL context (or a NULL out or
count pointer) is refused before any device work with the counts zeroed, and the Python wrapper exists."""
import ctypes as C
import os
import re

from babble_amd import _lib
from babble_amd._lib import hgx_error, hgx_frame_out

HGX_ERR_INVALID = 102
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_exported_and_declared():
    L = _lib.lib()
    f = L.hgx_get_frame_bodies   # AttributeError: not exported
    assert f.restype is C.c_int32 and f.argtypes is not None and len(f.argtypes) == 7
    assert f.argtypes[1] == C.POINTER(hgx_frame_out) and f.argtypes[-1] == C.POINTER(hgx_error)
    assert L.hgx_abi_version() == 6


def test_structure_follows_the_header():
    """Field names and order of the ctypes structure against the typedef in include/hgx.h; pointers
    and the four int64 capacities have the same size, so the order fixes the layout."""
    text = open(os.path.join(ROOT, "include", "hgx.h")).read()
    body = text[:text.index("} hgx_frame_out;")]
    body = body[body.rindex("typedef struct {"):]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = re.findall(r"(int32_t\*|int64_t\*|uint8_t\*|int64_t)\s+(\w+);", body)
    assert [nm for _, nm in decl] == [nm for nm, _ in hgx_frame_out._fields_]
    for (ty, nm), (_, ct) in zip(decl, hgx_frame_out._fields_):
        assert (ct is C.c_int64) == (ty == "int64_t"), nm
    assert C.sizeof(hgx_frame_out) == 8 * len(decl)
    assert [nm for ty, nm in decl if ty == "int64_t"] == ["others_cap", "events_cap", "tx_cap", "bytes_cap"]


def test_null_arguments_are_invalid():
    L = _lib.lib()
    err = hgx_error()
    out = hgx_frame_out()
    cnt = [C.c_int64(7) for _ in range(4)]
    refs = [C.byref(x) for x in cnt]
    assert L.hgx_get_frame_bodies(None, C.byref(out), *refs, C.byref(err)) == HGX_ERR_INVALID
    assert err.code == HGX_ERR_INVALID and err.msg.startswith(b"hgx_get_frame_bodies:")
    assert [x.value for x in cnt] == [0, 0, 0, 0]
    # a NULL out and NULL count pointers too, and errors are optional
    assert L.hgx_get_frame_bodies(None, None, *refs, C.byref(err)) == HGX_ERR_INVALID
    assert L.hgx_get_frame_bodies(None, C.byref(out), None, None, None, None, None) == HGX_ERR_INVALID


def test_python_wrapper_exists():
    from babble_amd.hashgraph import Hashgraph
    assert callable(Hashgraph.GetFrameBodies) and callable(Hashgraph.get_frame_bodies_raw)
