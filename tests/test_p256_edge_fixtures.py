"""The constructed P-256 edge vectors (tests/golden/p256_edge_vectors.txt, written by
tests/golden/make_p256_edge.py) and the plain reference that made them (tests/p256ref.py). CPU only.

  * the committed file is what the generator writes;
  * p256ref.verify / on_curve agree with `expected` / `key_ok` on every line of the edge file and
    of the libcrypto file p256_vectors.txt, and libcrypto (oracle/p256_ref check) with the edge file;
  * every vector tagged for a branch of k_p256_verify takes it in p256ref.comb_events, the exact
    model of the kernel's walk, and no vector of the other classes takes one by accident."""
import importlib.util
import os
import subprocess

import pytest

import p256ref as ref
from test_p256_fixtures import ROOT, VEC, load_vectors

EDGE = os.path.join(ROOT, "tests", "golden", "p256_edge_vectors.txt")

TAGS = ("dbl-G-Q", "dbl-cross", "opp-restart", "final-inf", "r-plus-N", "r-plus-N-twin", "r-plus-N-neg",
        "r-plus-N-wraps", "r-plus-N-wraps-match", "r-plus-N-carry", "r-plus-N-carry-neg", "key-x-zero", "key-x-small",
        "key-x-near-p", "key-x-limbs", "key-x-zero-bit", "key-x-small-bit", "key-x-near-p-bit", "key-x-limbs-bit",
        "key-x-p-plus", "pos-G", "pos-Q", "scalar-edge")


def _int(b):
    return int.from_bytes(b, "big")


def _agrees(rows):
    bad = []
    for i, (pub, dg, r, s, exp, kok, tag) in enumerate(rows):
        k = ref.on_curve(pub)
        ok = k and ref.verify(ref.parse_pub(pub), _int(dg), _int(r), _int(s))
        if (int(ok), int(k)) != (exp, kok):
            bad.append((i, tag, int(ok), int(k), exp, kok))
    return bad


def test_generator_reproduces_the_file():
    spec = importlib.util.spec_from_file_location("make_p256_edge", os.path.join(ROOT, "tests", "golden",
                                                                               "make_p256_edge.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    with open(EDGE) as f:
        assert f.read() == "\n".join(m.generate()) + "\n"


def test_file_has_every_class_and_stays_small():
    rows = load_vectors(EDGE)
    tags = {r[6] for r in rows}
    for t in TAGS:
        assert t in tags, t
    assert len({r[0] for r in rows}) <= 64                       # a key costs 512 KB of table
    assert os.path.getsize(EDGE) < os.path.getsize(VEC)
    n = {t: sum(r[6] == t for r in rows) for t in tags}
    assert n["pos-G"] == 96 and n["pos-Q"] == 96 and n["opp-restart"] >= 3 and n["final-inf"] >= 6
    # pos-G / pos-Q: u1 = e / s (u2 = r / s) is one byte, and every (position, digit) occurs
    for tag in ("pos-G", "pos-Q"):
        seen = set()
        for pub, dg, r, s, *_ in (x for x in rows if x[6] == tag):
            u = (_int(dg) if tag == "pos-G" else _int(r)) * pow(_int(s), -1, ref.N) % ref.N
            j = (u.bit_length() - 1) // 8
            assert u == (u >> (8 * j)) << (8 * j)
            seen.add((j, u >> (8 * j)))
        assert seen == {(j, b) for j in range(32) for b in (1, 128, 255)}


def test_reference_agrees_with_the_edge_file():
    assert _agrees(load_vectors(EDGE)) == []


def test_reference_agrees_with_the_libcrypto_vectors():
    assert _agrees(load_vectors()) == []


def test_libcrypto_agrees_with_the_edge_file():
    try:
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "p256_ref"])
    except (OSError, subprocess.CalledProcessError) as e:
        pytest.skip(f"cannot build oracle/p256_ref (gcc + libcrypto): {e}")
    out = subprocess.run([os.path.join(ROOT, "oracle", "p256_ref"), "check", EDGE], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


def test_tagged_vectors_take_their_branch():
    for i, (pub, dg, r, s, exp, kok, tag) in enumerate(load_vectors(EDGE)):
        if not kok:
            continue
        ev = ref.comb_events(ref.parse_pub(pub), _int(dg), _int(r), _int(s))
        what = (i, tag, ev)
        if tag.startswith("dbl-"):
            assert any(x.startswith("dbl@") for x in ev) and exp == 1, what
        elif tag == "opp-restart":
            k = [n for n, x in enumerate(ev) if x.startswith("opp@")]
            assert k and ev[k[0] + 1].startswith("from-inf@") and not ev[k[0] + 1].startswith("from-inf@0"), what
            assert "final-inf" not in ev and exp == 1, what
        elif tag == "final-inf":
            assert ev[-1] == "final-inf" and exp == 0, what
        elif tag == "r-plus-N":
            assert ev == ["x>=N"] and exp == 1, what
        else:
            assert not any(x.startswith(("dbl@", "opp@")) or x == "final-inf" for x in ev), what
            # x(R) >= N only where the class is about it
            assert "x>=N" not in ev, what
    # the model itself: the walks of three vectors written out
    N, G, nG = ref.N, ref.G, ref.neg(ref.G)
    assert ref.comb_events(G, *ref.forge(G, 0x0203, 0x0503)) == ["dbl@0Q"]
    assert ref.comb_events(nG, *ref.forge(nG, 0x0203, 0x050003)) == ["opp@0Q", "from-inf@1G"]
    assert ref.comb_events(nG, *ref.forge(nG, 7, 7, r=5)) == ["opp@0Q", "final-inf"]
    assert ref.comb_events(G, 1, 0, 1) == [] and ref.comb_events(G, 1, 1, N) == []


def test_reference_group_law():
    """p256ref against itself: the order of G, lift, and forge / forge_R round trips."""
    N, G = ref.N, ref.G
    assert ref.is_point(G) and ref.mul(N, G) is None and ref.mul(N - 1, G) == ref.neg(G)
    assert ref.lift(G[0], odd=True) == G and ref.lift(0) is not None and ref.lift(ref.N + 3) is not None
    assert all(ref.lift(x) is None for x in (ref.N, ref.N + 1, ref.N + 2, ref.P))
    Q = ref.mul(0xC0FFEE, G)
    assert ref.comb_mul(0xC0FFEE << 200 | 0x1234, G) == ref.mul(0xC0FFEE << 200 | 0x1234, G)
    e, r, s = ref.forge(Q, 12345, 67890)
    assert ref.verify(Q, e, r, s) and not ref.verify(Q, e + 1, r, s) and ref.verify(Q, e + N, r, s)
    R = ref.lift(N + 3)
    Q2, e, r, s = ref.forge_R(R, 11, 13)
    assert r == 3 and ref.add(ref.mul(11, G), ref.mul(13, Q2)) == R and ref.verify(Q2, e, r, s)
    assert ref.on_curve(ref.pub65(Q)) and not ref.on_curve(b"\x05" + ref.pub65(Q)[1:])
    x0 = next(x for x in range(1, 99) if ref.lift(x))
    assert not ref.on_curve(b"\x04" + (ref.P + x0).to_bytes(32, "big") + ref.lift(x0)[1].to_bytes(32, "big"))
