"""The host side of the event-body front end (no GPU): hgx_batch_levels against a Python reference,
the argument checks of hgx_insert_event_bodies and hgx_event_json_batch (HGX_ERR_INVALID before any
device call), and no CPU fallback for the encoder."""
import ctypes as C

import numpy as np
import pytest

import bodyref
from babble_amd import _lib
from babble_amd import trace as gtrace
from babble_amd.hashgraph import batch_levels, body_columns, event_json_batch, _event_bodies_of


@pytest.mark.parametrize("n,E", [(4, 300), (64, 640), (2, 200)])
def test_batch_levels_matches_reference(n, E):
    t = gtrace.gossip(n, E, 11, stale_prob=0.1, stale_depth=2)
    want, nl = bodyref.py_levels(t.sp, t.op)
    got, got_nl = batch_levels(t.sp, t.op)
    assert np.array_equal(got, want) and got_nl == nl
    assert nl > 1 and (want[t.sp >= 0] > 0).all()


def test_batch_levels_with_base():
    """The second part of a split batch: parents below `base` are in the store, not in the batch."""
    t = gtrace.gossip(8, 500, 12)
    base = 200
    want, nl = bodyref.py_levels(t.sp[base:], t.op[base:], base)
    got, got_nl = batch_levels(t.sp[base:], t.op[base:], base)
    assert np.array_equal(got, want) and got_nl == nl
    assert got[0] == 0 and nl < bodyref.py_levels(t.sp, t.op)[1]


def test_batch_levels_all_genesis_and_empty():
    sp = np.full(16, -1, np.int64)
    got, nl = batch_levels(sp, sp)
    assert nl == 1 and not got.any()
    got, nl = batch_levels(sp[:0], sp[:0])
    assert nl == 0 and len(got) == 0


@pytest.mark.parametrize("which", ["sp", "op"])
@pytest.mark.parametrize("delta", [0, 1])
def test_batch_levels_rejects_parent_not_earlier(which, delta):
    t = gtrace.gossip(4, 50, 13)
    sp, op = t.sp.copy(), t.op.copy()
    base, k = 7, 20
    {"sp": sp, "op": op}[which][k] = base + k + delta   # its own gid, or a later one
    with pytest.raises(_lib.HgxError) as ei:
        batch_levels(sp, op, base)
    assert ei.value.code == 102 and "event 20" in ei.value.msg
    with pytest.raises(ValueError):
        bodyref.py_levels(sp, op, base)


def _cols(m=5):
    z = np.zeros(m, np.int64)
    return body_columns(np.zeros(m, np.int32), z, z - 1, z - 1, z, np.zeros((m, 32), np.uint8),
                        np.ones((m, 32), np.uint8), [[b"ab", b"c"]] * m)


def _insert_rc(cols, null=None):
    _, ev = _event_bodies_of(cols, 0, len(cols["creator"]))
    if null:
        setattr(ev, null, None)
    err = _lib.hgx_error()
    n_ins = C.c_int64(-1)
    rc = _lib.lib().hgx_insert_event_bodies(None, C.byref(ev), len(cols["creator"]), None, C.byref(n_ins), C.byref(err))
    return rc, err.msg.decode(), n_ins.value


@pytest.mark.parametrize("col", ["creator", "index", "self_parent", "other_parent", "timestamp_ns", "sig_r", "sig_s",
                                 "ntx", "tx_off"])
def test_insert_event_bodies_rejects_null_columns(col):
    rc, msg, n_ins = _insert_rc(_cols(), null=col)
    assert rc == 102 and "null column" in msg and n_ins == 0


def test_insert_event_bodies_rejects_bad_offsets_and_counts():
    cols = _cols()
    cols["tx_off"] = cols["tx_off"].copy()
    cols["tx_off"][3] = cols["tx_off"][2] - 1
    rc, msg, _ = _insert_rc(cols)
    assert rc == 102 and "non-decreasing" in msg
    cols = _cols()
    cols["ntx"] = cols["ntx"].copy()
    cols["ntx"][2] = -2
    rc, msg, _ = _insert_rc(cols)
    assert rc == 102 and "ntx below -1" in msg
    # good columns: the missing context is the next thing it names
    rc, msg, _ = _insert_rc(_cols())
    assert rc == 102 and "bad arguments" in msg


def test_event_json_batch_validates_then_fails_loudly_without_gpu():
    import torch
    keys = np.zeros((1, 65), np.uint8)
    ids = np.zeros((5, 32), np.uint8)
    cols = _cols()
    cols["tx_off"] = cols["tx_off"].copy()
    cols["tx_off"][1] = 99
    with pytest.raises(_lib.HgxError) as ei:
        event_json_batch(cols, keys, ids, ids)
    assert ei.value.code == 102 and "non-decreasing" in str(ei.value)
    cols = _cols()
    cols["creator"] = cols["creator"] + 1     # no key 1
    with pytest.raises(_lib.HgxError) as ei:
        event_json_batch(cols, keys, ids, ids)
    assert ei.value.code == 102 and "without a key" in str(ei.value)
    _, ev = _event_bodies_of(_cols(), 0, 5)
    ev.sig_r = None
    err = _lib.hgx_error()
    off = np.zeros(6, np.int64)
    rc = _lib.lib().hgx_event_json_batch(0, C.byref(ev), 5, _lib.ptr(keys), 1, _lib.ptr(ids), _lib.ptr(ids), None, 0,
                                         _lib.ptr(off), C.byref(err))
    assert rc == 102 and "null column" in err.msg.decode()
    if not torch.cuda.is_available():   # valid arguments: the device is what is missing
        with pytest.raises(_lib.HgxError) as ei:
            event_json_batch(_cols(), keys, ids, ids)
        assert ei.value.code == 200 and "no CPU fallback" in str(ei.value)
