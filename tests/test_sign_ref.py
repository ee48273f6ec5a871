"""The signer's CPU side: the pure-Python reference against the committed known
answers and against libcrypto, and the argument checks of the stand-alone C entry points."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import hgref
import signref
from babble_amd import _lib
from babble_amd.hashgraph import p256_public_keys, p256_sign
from p256ref import N

HGX_ERR_INVALID = 102


def kat():
    with open(os.path.join(hgref.GOLDEN, "p256_sign_kat.json")) as f:
        return json.load(f)


def ref_check(entries, tmp_path):
    """oracle/p256_ref check (libcrypto's ECDSA_do_verify) accepts every (pub, digest, r, s)."""
    exe = os.path.join(hgref.ROOT, "oracle", "p256_ref")
    if not os.path.exists(exe):   # built as hgref.sign_batch builds it
        subprocess.check_call(["make", "-s", "-C", os.path.join(hgref.ROOT, "oracle")])
    path = os.path.join(str(tmp_path), "vectors.txt")
    with open(path, "w") as f:
        f.write(signref.ref_lines(entries))
    out = subprocess.run([exe, "check", path], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith(f"{len(entries)} vectors, 0 disagree"), out.stdout


def test_fixture_covers_what_it_should():
    k = kat()
    tags = [c["tag"] for c in k["cases"]]
    assert len(set(tags)) == len(tags)
    for want in ("rfc6979-a.2.5-sample", "rfc6979-a.2.5-test", "edge-key-1", "edge-key-N-1"):
        assert want in tags
    for ki in (0, 1):
        for e in ("0", "1", "N-1", "N", "N+1", "2^256-1"):
            assert f"edge-digest-{e}-key{ki}" in tags
    by = {t.rsplit("-try", 1)[0]: c for t, c in zip(tags, k["cases"])}
    assert int(by["short-r-248"]["r"], 16) < 2 ** 248
    assert int(by["short-s-248"]["s"], 16) < 2 ** 248
    if "short-r-240" in by:
        assert int(by["short-r-240"]["r"], 16) < 2 ** 240
    else:
        assert any("short-r-240" in n for n in k["notes"])
    # the RFC's printed answers (RFC 6979 A.2.5, SHA-256)
    s = by["rfc6979-a.2.5-sample"]
    assert s["k"].upper().startswith("A6E3C57D") and s["k"].upper().endswith("3D8AAD60")
    assert s["r"].upper() == "EFD48B2AACB6A8FD1140DD9CD45E81D69D2C877B56AAF991C34D0EA84EAF3716"
    assert s["s"].upper() == "F7CB1C942D657C41D436C7A1B6E29F65F3E900DBB9AFF4064DC4AB2F843ACDA8"
    t = by["rfc6979-a.2.5-test"]
    assert t["r"].upper() == "F1ABB023518351CD71D881567B1EA663ED3EFCF6C5132B354F28D3B0B7D38367"
    assert t["s"].upper() == "019F4113742A2B14BD25926B49C649155F267E60D3814B4C0CC84250E46F0083"


def test_signref_reproduces_every_fixture_line():
    for c in kat()["cases"]:
        d = int(c["d"], 16)
        r, s, k = signref.sign(d, bytes.fromhex(c["digest"]))
        assert ("%064x" % r, "%064x" % s, "%064x" % k) == (c["r"], c["s"], c["k"]), c["tag"]
        assert signref.pub65(d).hex() == c["pub"], c["tag"]


def test_fixture_passes_libcrypto(tmp_path):
    ref_check([tuple(bytes.fromhex(c[f]) for f in ("pub", "digest", "r", "s")) for c in kat()["cases"]], tmp_path)


def test_derived_keys_are_p256_refs():
    keys, _, _ = hgref.sign_batch(5, [0], np.zeros((1, 32), np.uint8))
    assert np.array_equal(keys, signref.pub_bytes(5))


def _rc(fn, *args):
    err = _lib.hgx_error()
    rc = fn(*args, C.byref(err))
    return rc, err.msg.decode(errors="replace")


def test_sign_batch_and_public_keys_validate_their_arguments():
    L = _lib.lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    d = signref.priv_bytes(2)
    idx = np.zeros(3, np.int32)
    dig = np.zeros((3, 32), np.uint8)
    r, s = np.zeros((3, 32), np.uint8), np.zeros((3, 32), np.uint8)
    pub = np.zeros((2, 65), np.uint8)
    good = [0, ptr(d), 2, ptr(idx), ptr(dig), 3, ptr(r), ptr(s)]
    for pos in (1, 3, 4, 6, 7):   # NULL pointers
        a = list(good)
        a[pos] = None
        rc, msg = _rc(L.hgx_p256_sign_batch, *a)
        assert rc == HGX_ERR_INVALID and msg.startswith("hgx_p256_sign_batch: "), (pos, rc, msg)
    for pos, v in ((2, 0), (2, -1), (5, -1)):   # n_keys <= 0, negative count
        a = list(good)
        a[pos] = v
        assert _rc(L.hgx_p256_sign_batch, *a)[0] == HGX_ERR_INVALID
    for bad in (-1, 2):   # a key index outside [0, n_keys)
        i2 = np.array([0, bad, 1], np.int32)
        a = list(good)
        a[3] = ptr(i2)
        rc, msg = _rc(L.hgx_p256_sign_batch, *a)
        assert rc == HGX_ERR_INVALID and "key index" in msg
    for bad in (0, N, N + 1, 2 ** 256 - 1):   # d = 0 or d >= N
        d2 = d.copy()
        d2[1] = np.frombuffer(bad.to_bytes(32, "big"), np.uint8)
        a = list(good)
        a[1] = ptr(d2)
        rc, msg = _rc(L.hgx_p256_sign_batch, *a)
        assert rc == HGX_ERR_INVALID and "not below N" in msg
        rc, msg = _rc(L.hgx_p256_public_keys, 0, ptr(d2), 2, ptr(pub))
        assert rc == HGX_ERR_INVALID and msg.startswith("hgx_p256_public_keys: ")
    for a in ([0, None, 2, ptr(pub)], [0, ptr(d), 2, None], [0, ptr(d), 0, ptr(pub)], [0, ptr(d), -3, ptr(pub)]):
        assert _rc(L.hgx_p256_public_keys, *a)[0] == HGX_ERR_INVALID
    # d = N - 1 is a key; an empty batch is no error and needs no device
    d2 = d.copy()
    d2[1] = np.frombuffer((N - 1).to_bytes(32, "big"), np.uint8)
    assert _rc(L.hgx_p256_sign_batch, 0, ptr(d2), 2, None, None, 0, None, None)[0] == 0


def test_sign_calls_fail_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        return   # (with a device the calls are tests/test_gpu_p256_sign.py's)
    d = signref.priv_bytes(2)
    with pytest.raises(_lib.HgxError) as ei:
        p256_sign(d, [0, 1], np.zeros((2, 32), np.uint8))
    assert "no CPU fallback" in str(ei.value)
    with pytest.raises(_lib.HgxError) as ei:
        p256_public_keys(d)
    assert "no CPU fallback" in str(ei.value)
