"""Generates tests/golden/p256_edge_vectors.txt: signatures that drive k_p256_verify (hgx_p256.hip)
through the branches a random signature reaches with probability about 2^-128: the doubling and
opposite branches of the mixed addition, the walk restarting from infinity, a final infinity, the
second compare X == (r + N) Z^2 and its two guards, public keys with degenerate coordinates, every
table position and the digits 1 / 128 / 255 one at a time, and the ends of the scalar ranges.

No private key and no libcrypto: tests/p256ref.py forges each signature from the u1, u2 (or the R)
it should make the verifier compute, and its verify / on_curve give `expected` / `key_ok`.
Deterministic (every random value is SHA-256 of a counter). The line format is p256_vectors.txt's:
"pub65 digest32 r32 s32 expected key_ok tag".  python tests/golden/make_p256_edge.py"""
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import p256ref as ref  # noqa: E402
from p256ref import G, N, P  # noqa: E402

OUT = os.path.join(HERE, "p256_edge_vectors.txt")


class Rng:
    def __init__(self, seed):
        self.seed, self.c = seed, 0

    def bits(self, n):
        out = b""
        while 8 * len(out) < n:
            out += hashlib.sha256(b"%s|%d" % (self.seed, self.c)).digest()
            self.c += 1
        return int.from_bytes(out, "big") >> (8 * len(out) - n)

    def scalar(self):
        """Uniform in [1, N-1] with a nonzero byte at every position (no comb digit skipped)."""
        while True:
            v = self.bits(256)
            if 0 < v < N and all((v >> (8 * j)) & 255 for j in range(32)):
                return v

    def digit(self):
        return 1 + self.bits(16) % 255


def above(v, j):
    """v with the bytes at positions < j cleared."""
    return v >> (8 * j) << (8 * j)


def first_liftable(start, step, count):
    out, x = [], start
    while len(out) < count:
        if ref.lift(x) is not None:
            out.append(x)
        x += step
    return out


def flip(v, bit):
    return v ^ (1 << bit)


def generate():
    """The file's lines, in order."""
    rng = Rng(b"hgx p256 edge 1")
    rows = []

    def emit(Q, e, r, s, tag):
        assert 0 <= e < 1 << 256 and 0 <= r < 1 << 256 and 0 <= s < 1 << 256
        pub = Q if isinstance(Q, bytes) else ref.pub65(Q)
        kok = ref.on_curve(pub)
        ok = kok and ref.verify(ref.parse_pub(pub), e, r, s)
        rows.append("%s %064x %064x %064x %d %d %s" % (pub.hex(), e, r, s, int(ok), int(kok), tag))
        return ok

    def valid(Q, u1, u2, tag):
        assert emit(Q, *ref.forge(Q, u1, u2), tag), tag

    nG = ref.neg(G)

    # dbl-G-Q: Q = G and the same lowest nonzero byte in u1 and u2: G's entry starts the walk, Q's is equal to it
    for j in (0, 1, 15, 31):
        for _ in range(2):
            b = rng.digit() << (8 * j)
            valid(G, above(rng.scalar(), j + 1) | b, above(rng.scalar(), j + 1) | b, "dbl-G-Q")
    # dbl-cross: Q = 256^j G, u2 = b (position 0 of Q's table) and u1 = b 256^j (position j of G's): the same point
    for j in (1, 5, 31):
        Qj = ref.mul(1 << (8 * j), G)
        for b in (1, 0x80, 0xFF, rng.digit()):
            valid(Qj, b << (8 * j), b, "dbl-cross")
        if j < 31:   # the same with digits above position j on both sides
            b = rng.digit()
            valid(Qj, above(rng.scalar(), j + 1) | b << (8 * j), above(rng.scalar(), j + 1) | b, "dbl-cross")
    # opp-restart: Q = -G, equal lowest bytes cancel to infinity, the walk goes on from a later digit
    h1, h2 = above(rng.scalar(), 1), above(rng.scalar(), 1)
    valid(nG, h1 | 0x5A, h2 | 0x5A, "opp-restart")                                 # restarts on G's digit at 1
    valid(nG, above(h1, 2) | 0x5A, h2 | 0x5A, "opp-restart")                       # on Q's digit at 1
    valid(nG, above(h1, 2) | 0x11C3, above(h2, 2) | 0x11C3, "opp-restart")         # two cancellations, restart at 2
    valid(nG, above(h1, 4) | 0xFF << 24, above(h2, 4) | 0xFF << 24, "opp-restart")  # cancels at 3, restarts at 4
    valid(nG, above(h1, 9) | 0x01 << 24, above(h2, 6) | 0x01 << 24, "opp-restart")  # cancels at 3, Q's digit at 6
    valid(nG, 0x0780 << 240, 0x0980 << 240, "opp-restart")                         # cancels at 30, restarts at 31
    # final-inf: u1 G + u2 Q = O whatever r is; Q = -G cancels position by position, Q = G only at the last addition
    for width in (1, 2, 4, 8, 16, 24, 31, 32):
        u = rng.scalar() >> (256 - 8 * width)
        r = {1: 1, 2: N - 1}.get(width, rng.scalar())
        assert not emit(nG, *ref.forge(nG, u, u, r), "final-inf")
    for _ in range(2):
        u2 = rng.scalar()
        assert not emit(G, *ref.forge(G, N - u2, u2, rng.scalar()), "final-inf")
    # r-plus-N: x(R) in [N, p), r = x(R) - N: only the second compare X == (r + N) Z^2 accepts
    for x in first_liftable(N, 1, 3):
        for odd in (False, True):
            u1, u2 = rng.scalar(), rng.scalar()
            Q, e, r, s = ref.forge_R(ref.lift(x, odd), u1, u2)
            assert r == x - N and emit(Q, e, r, s, "r-plus-N")
            assert not emit(Q, e, r + 1, s, "r-plus-N-neg")
            if r > 1:
                assert not emit(Q, e, r - 1, s, "r-plus-N-neg")
            if not odd and ref.lift(r) is not None:   # the same r reached by the first compare
                Q2, e2, r2, s2 = ref.forge_R(ref.lift(r), u1, u2)
                assert r2 == r and emit(Q2, e2, r2, s2, "r-plus-N-twin")
    # r-plus-N-wraps: x(R) small, r = x + p - N: r + N = x mod p but r + N >= p, so r is not x mod N
    for x in first_liftable(1, 1, 2):
        u1, u2 = rng.scalar(), rng.scalar()
        R = ref.lift(x, odd=bool(x & 1))
        Q, e, r, s = ref.forge_R(R, u1, u2, r=x + P - N)
        assert not emit(Q, e, r, s, "r-plus-N-wraps")
        Q, e, r, s = ref.forge_R(R, u1, u2)
        assert r == x and emit(Q, e, r, s, "r-plus-N-wraps-match")
    # r-plus-N-carry: r + N needs 256 bits (first compare), then 257: the sum's low 256 bits are below p
    top = (1 << 256) - N
    x = first_liftable(top - 1, -1, 1)[0]
    u1, u2 = rng.scalar(), rng.scalar()
    Q, e, r, s = ref.forge_R(ref.lift(x), u1, u2)
    assert r == x and emit(Q, e, r, s, "r-plus-N-carry")
    assert not emit(Q, e, r + 1, s, "r-plus-N-carry-neg")
    assert not emit(Q, e, top, s, "r-plus-N-carry-neg")        # r + N = 2^256 exactly
    for x in first_liftable(1, 1, 2):   # x(R) = r + N - 2^256: accepted if the carry out of r + N is ignored
        Q, e, r, s = ref.forge_R(ref.lift(x), rng.scalar(), rng.scalar(), r=top + x)
        assert not emit(Q, e, r, s, "r-plus-N-carry-neg")
    # keys with degenerate coordinates: valid signatures and one flipped bit of each field in turn
    pats = [1 << 224, 1 << 96, (1 << 96) - 1, (1 << 224) - 1, (1 << 32) - 1, 1 << 32, 1 << 192, (1 << 128) - 1,
            (1 << 256) - (1 << 224), ((1 << 32) - 1) << 96, ((1 << 64) - 1) << 128, P - (1 << 224), P - (1 << 96)]
    for tag, keys in (("key-x-zero", [ref.lift(0, False), ref.lift(0, True)]),
                      ("key-x-small", [ref.lift(x, bool(i & 1)) for i, x in enumerate(first_liftable(1, 1, 3))]),
                      ("key-x-near-p", [ref.lift(x, bool(i & 1)) for i, x in enumerate(first_liftable(P - 1, -1, 3))]),
                      ("key-x-limbs", [ref.lift(x, bool(i & 1)) for i, x in enumerate(pats) if ref.lift(x)])):
        for ki, Q in enumerate(keys):
            for i in range(3):
                e, r, s = ref.forge(Q, rng.scalar(), rng.scalar())
                assert emit(Q, e, r, s, tag)
            bit = rng.bits(8)
            bad = [(flip(e, bit), r, s), (e, flip(r, bit), s), (e, r, flip(s, bit))][ki % 3]
            assert not emit(Q, *bad, tag + "-bit")
    # x = p + x0 names the point (x0, y) mod p, but Go's Unmarshal rejects x >= p
    x0 = first_liftable(1, 1, 1)[0]
    Q = ref.lift(x0)
    e, r, s = ref.forge(Q, rng.scalar(), rng.scalar())
    assert not emit(b"\x04" + (P + x0).to_bytes(32, "big") + Q[1].to_bytes(32, "big"), e, r, s, "key-x-p-plus")
    # pos-G / pos-Q: one table entry of G (of the key) at a time, for every position and the digits 1, 128, 255
    d1, d2 = rng.scalar(), rng.scalar()
    K = [ref.mul(d1, G), ref.mul(d2, G)]
    for j in range(32):
        for bi, b in enumerate((1, 128, 255)):
            valid(K[(j + bi) & 1], b << (8 * j), rng.scalar(), "pos-G")
            valid(K[(j + bi + 1) & 1], rng.scalar(), b << (8 * j), "pos-Q")
    # scalar-edge: the ends of the ranges of s, u1, u2 and e, under the key d1 G (d1 is used for s = +-1 and for
    # the e that is u1 s + N: s = (e + r d) / k is ECDSA's own signing equation)
    Q = K[0]
    k = rng.scalar()
    r = ref.mul(k, G)[0] % N
    valid(Q, (k - r * d1) % N, r, "scalar-edge")            # s = 1
    assert rows[-1].split()[3] == "%064x" % 1
    valid(Q, (k + r * d1) % N, N - r, "scalar-edge")        # s = N - 1
    assert rows[-1].split()[3] == "%064x" % (N - 1)
    valid(Q, rng.scalar(), 1, "scalar-edge")                # u2 = 1: s = r
    valid(Q, rng.scalar(), N - 1, "scalar-edge")
    valid(Q, N - 1, rng.scalar(), "scalar-edge")
    valid(Q, N - 1, N - 1, "scalar-edge")
    valid(Q, (1 << 248) - 1, (1 << 248) - 1, "scalar-edge")  # every byte below N's top byte 0xFF
    valid(Q, (1 << 248) - 1, (1 << 128) - 1, "scalar-edge")
    for e0 in (0, 1, rng.bits(200), top - 1):               # digest = e0 + N < 2^256: reduced by one subtraction
        k = rng.scalar()
        r = ref.mul(k, G)[0] % N
        s = pow(k, -1, N) * (e0 + r * d1) % N
        assert emit(Q, e0 + N, r, s, "scalar-edge")
    return rows


if __name__ == "__main__":
    rows = generate()
    with open(OUT, "w") as f:
        f.write("\n".join(rows) + "\n")
    print("wrote", len(rows), "vectors,", len({x.split()[0] for x in rows}), "keys")
