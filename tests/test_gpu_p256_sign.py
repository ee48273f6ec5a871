"""hgx_p256_sign_batch / hgx_p256_public_keys on the device against tests/signref.py
(bit-exact: the nonces are RFC 6979's), the device's own verify, and libcrypto (oracle/p256_ref check)."""
import hashlib

import numpy as np
import pytest

import hgref
import signref
from babble_amd.hashgraph import p256_public_keys, p256_sign, p256_verify
from test_sign_ref import kat, ref_check

pytestmark = pytest.mark.gpu


def _b(hexes):
    return np.frombuffer(b"".join(bytes.fromhex(h) for h in hexes), np.uint8).reshape(len(hexes), -1).copy()


def test_fixture_lines_one_at_a_time():
    for c in kat()["cases"]:
        r, s = p256_sign(_b([c["d"]]), [0], _b([c["digest"]]))
        assert (r.tobytes().hex(), s.tobytes().hex()) == (c["r"], c["s"]), c["tag"]


def test_fixture_lines_cyclically_over_ragged_workgroups():
    """130 = two workgroups of 64 lanes and two lanes of a third."""
    cases = kat()["cases"]
    m = 130
    pick = [cases[i % len(cases)] for i in range(m)]
    r, s = p256_sign(_b([c["d"] for c in cases]), [i % len(cases) for i in range(m)], _b([c["digest"] for c in pick]))
    assert np.array_equal(r, _b([c["r"] for c in pick])) and np.array_equal(s, _b([c["s"] for c in pick]))


def test_300_digests_under_5_keys(tmp_path):
    m, nk = 300, 5
    dig = np.frombuffer(b"".join(hashlib.sha256(b"digest %d" % i).digest() for i in range(m)), np.uint8).reshape(m, 32)
    idx = np.arange(m, dtype=np.int32) * 7 % nk
    r, s = p256_sign(signref.priv_bytes(nk), idx, dig)
    wr, ws = signref.sign_batch([signref.priv(k) for k in range(nk)], idx, dig)
    assert np.array_equal(r, wr) and np.array_equal(s, ws)
    keys = signref.pub_bytes(nk)
    assert (p256_verify(keys, idx, dig, r, s) == 1).all()
    ref_check([(bytes(keys[idx[i]]), bytes(dig[i]), bytes(r[i]), bytes(s[i])) for i in range(m)], tmp_path)


def test_public_keys():
    keys, _, _ = hgref.sign_batch(5, [0], np.zeros((1, 32), np.uint8))
    assert np.array_equal(p256_public_keys(signref.priv_bytes(5)), keys)
    from p256ref import G, N, pub65
    one = np.frombuffer((1).to_bytes(32, "big"), np.uint8)
    assert p256_public_keys(one).tobytes() == pub65(G)
    # 70 keys: more than one workgroup; N - 1 gives -G
    d = [signref.priv(k) for k in range(69)] + [N - 1]
    got = p256_public_keys(_b(["%064x" % x for x in d]))
    assert got.tobytes() == b"".join(signref.pub65(x) for x in d)
