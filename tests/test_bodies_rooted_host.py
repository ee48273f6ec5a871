"""The host side of event bodies on rooted contexts (no GPU): the new entry points
exist and check their arguments before any device call, and hgx_batch_levels puts the root codes on
level 0, which the id pass relies on (their ids come from tables written before the launch)."""
import ctypes as C

import numpy as np

from babble_amd import _lib
from babble_amd.hashgraph import Hashgraph, batch_levels, body_columns, _event_bodies_of

ROOT_Y, ROOT_OTHER = -3, -4


def test_exported_symbols():
    L = _lib.lib()
    for name in ("hgx_set_root_ids", "hgx_insert_event_bodies_ext", "hgx_insert_event_bodies", "hgx_get_root_ids",
                 "hgx_get_root_others"):
        assert getattr(L, name, None) is not None, name
    assert L.hgx_abi_version() == 6
    assert (Hashgraph.ROOT_Y, Hashgraph.ROOT_OTHER) == (ROOT_Y, ROOT_OTHER)
    assert callable(Hashgraph.SetRootIds)


def test_root_codes_are_level_zero():
    # a frame as a batch at base 0: first events on Root.X with Root.Y / "", an Others event on a
    # resident self-parent, an event that depends on both
    sp = np.array([-1, -1, 0, -1, 2, 1], np.int64)
    op = np.array([ROOT_Y, -1, ROOT_OTHER, ROOT_OTHER, 3, ROOT_OTHER], np.int64)
    level, nl = batch_levels(sp, op)
    assert list(level) == [0, 0, 1, 0, 2, 1] and nl == 3
    # a sync on a resident set of 40: negative codes never count as in-batch parents
    sp = np.array([-1, 12, 40, -1], np.int64)
    op = np.array([ROOT_Y, ROOT_OTHER, ROOT_OTHER, ROOT_OTHER], np.int64)
    level, nl = batch_levels(sp, op, base=40)
    assert list(level) == [0, 0, 1, 0] and nl == 2


def test_null_context_is_refused_before_any_device_call():
    L = _lib.lib()
    err = _lib.hgx_error()
    has = np.zeros(4, np.int32)
    rc = L.hgx_set_root_ids(None, None, _lib.ptr(has), None, _lib.ptr(has), None, None, 0, C.byref(err))
    assert rc == 102 and err.msg.decode().startswith("hgx_set_root_ids: ")
    z = np.zeros(3, np.int64)
    cols = body_columns(np.zeros(3, np.int32), z, z - 1, z - 1, z, np.zeros((3, 32), np.uint8),
                        np.ones((3, 32), np.uint8), [[b"ab"]] * 3)
    _, ev = _event_bodies_of(cols, 0, 3)
    opi = np.zeros((3, 32), np.uint8)
    n_ins = C.c_int64(-1)
    rc = L.hgx_insert_event_bodies_ext(None, C.byref(ev), _lib.ptr(opi), 3, None, C.byref(n_ins), C.byref(err))
    assert rc == 102 and "bad arguments" in err.msg.decode() and n_ins.value == 0
    ev.sig_r = None   # the columns are checked first, as in hgx_insert_event_bodies
    rc = L.hgx_insert_event_bodies_ext(None, C.byref(ev), _lib.ptr(opi), 3, None, C.byref(n_ins), C.byref(err))
    assert rc == 102 and "null column" in err.msg.decode()
