"""hgx_prune_to_frame, hgx_get_root_ids and hgx_get_root_others without a GPU: the symbols are
exported and declared in the ctypes binding, a NULL context is refused before any device work, and
the Python wrappers exist."""
import ctypes as C

from babble_amd import _lib
from babble_amd._lib import hgx_error

HGX_ERR_INVALID = 102
NAMES = ("hgx_prune_to_frame", "hgx_get_root_ids", "hgx_get_root_others")


def test_symbols_exported_and_declared():
    L = _lib.lib()
    for nm in NAMES:
        f = getattr(L, nm)   # AttributeError: not exported
        assert f.restype is C.c_int32 and f.argtypes is not None and f.argtypes[-1] == C.POINTER(hgx_error), nm
    assert len(L.hgx_prune_to_frame.argtypes) == 5
    assert len(L.hgx_get_root_ids.argtypes) == 7
    assert len(L.hgx_get_root_others.argtypes) == 6
    assert L.hgx_abi_version() == 6


def test_null_context_is_invalid():
    L = _lib.lib()
    err = hgx_error()
    nk = C.c_int64(7)
    assert L.hgx_prune_to_frame(None, None, 0, C.byref(nk), C.byref(err)) == HGX_ERR_INVALID
    assert err.code == HGX_ERR_INVALID and err.msg.startswith(b"hgx_prune_to_frame:") and nk.value == 0
    hx, hy = C.c_int32(1), C.c_int32(1)
    assert L.hgx_get_root_ids(None, 0, None, C.byref(hx), None, C.byref(hy), C.byref(err)) == HGX_ERR_INVALID
    assert err.code == HGX_ERR_INVALID and hx.value == 0 and hy.value == 0
    cnt = C.c_int64(3)
    assert L.hgx_get_root_others(None, None, None, 0, C.byref(cnt), C.byref(err)) == HGX_ERR_INVALID
    assert err.code == HGX_ERR_INVALID and cnt.value == 0
    # errors are optional
    assert L.hgx_prune_to_frame(None, None, 0, None, None) == HGX_ERR_INVALID


def test_python_wrappers_exist():
    from babble_amd.hashgraph import Hashgraph
    for nm in ("PruneToFrame", "GetRootIds", "GetRootOthers"):
        assert callable(getattr(Hashgraph, nm)), nm
