"""TEST INFRASTRUCTURE: a plain ECDSA P-256 reference in Python integers (affine points, None is
the point at infinity), the second checker of libhgx's batched verify (hgx_p256.hip) beside
libcrypto (oracle/p256_ref.c), and the constructions that reach the kernel's rare branches on
purpose, without a private key:

    for any point Q and any u1, u2 (u2 != 0):  R = u1 G + u2 Q,  r = x(R) mod N,  s = r / u2,
    e = u1 s  is a signature that verifies, and the verifier's u1 = e / s, u2 = r / s are the
    chosen ones, so the kernel's comb digits are exactly the bytes of u1 and u2 (forge);
    conversely, for any R:  Q = (R - u1 G) / u2  makes the verifier arrive at R (forge_R).

comb_events models the walk of k_p256_verify (byte positions 0..31 ascending, G's digit before
Q's, zero digits skipped) in exact arithmetic and names the branches a signature takes."""

P = 0xFFFFFFFF00000001000000000000000000000000FFFFFFFFFFFFFFFFFFFFFFFF
N = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551
B = 0x5AC635D8AA3A93E7B3EBBD55769886BC651D06B0CC53B0F63BCE3C3E27D2604B
G = (0x6B17D1F2E12C4247F8BCE6E563A440F277037D812DEB33A0F4A13945D898C296,
     0x4FE342E2FE1A7F9B8EE7EB4A7C0F9E162BCE33576B315ECECBB6406837BF51F5)


def neg(a):
    return None if a is None else (a[0], (P - a[1]) % P)


def dbl(a):
    if a is None or a[1] == 0:
        return None
    x, y = a
    m = (3 * x * x - 3) * pow(2 * y, -1, P) % P
    x3 = (m * m - 2 * x) % P
    return (x3, (m * (x - x3) - y) % P)


def add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        return dbl(a) if a[1] == b[1] else None
    m = (b[1] - a[1]) * pow(b[0] - a[0], -1, P) % P
    x3 = (m * m - a[0] - b[0]) % P
    return (x3, (m * (a[0] - x3) - a[1]) % P)


def mul(k, a):
    """k a by double-and-add from the top bit (k >= 0, not reduced)."""
    acc = None
    for i in range(k.bit_length() - 1, -1, -1):
        acc = dbl(acc)
        if (k >> i) & 1:
            acc = add(acc, a)
    return acc


def is_point(a):
    return a is None or (0 <= a[0] < P and 0 <= a[1] < P and (a[1] * a[1] - (a[0] ** 3 - 3 * a[0] + B)) % P == 0)


def lift(x, odd=False):
    """The curve point with this x (0 <= x < p) and a y of the given parity, or None."""
    if not 0 <= x < P:
        return None
    rhs = (x * x * x - 3 * x + B) % P
    y = pow(rhs, (P + 1) // 4, P)   # p = 3 mod 4
    if y * y % P != rhs:
        return None
    if (y & 1) != int(bool(odd)):
        y = P - y
    return (x, y)


def verify(Q, e, r, s):
    """FIPS 186-4 section 6.4.2 on P-256; e is the digest as an integer (a 32-byte digest is used whole)."""
    if not (1 <= r < N and 1 <= s < N):
        return False
    w = pow(s, -1, N)
    R = add(mul(e % N * w % N, G), mul(r * w % N, Q))
    return R is not None and R[0] % N == r


def pub65(Q):
    return b"\x04" + Q[0].to_bytes(32, "big") + Q[1].to_bytes(32, "big")


def parse_pub(pub):
    return (int.from_bytes(pub[1:33], "big"), int.from_bytes(pub[33:65], "big"))


def on_curve(pub):
    """Go's elliptic.Unmarshal(P256(), pub) != nil for 65 bytes: prefix 0x04, x and y < p, on the curve."""
    if len(pub) != 65 or pub[0] != 0x04:
        return False
    x, y = parse_pub(pub)
    return x < P and y < P and (y * y - (x * x * x - 3 * x + B)) % P == 0


def _sig(R, u1, u2, r):
    if r is None:
        if R is None or R[0] % N == 0:
            raise ValueError("no r: R is the point at infinity or x(R) = 0 mod N")
        r = R[0] % N
    s = r * pow(u2, -1, N) % N
    return (u1 * s % N, r, s)


def forge(Q, u1, u2, r=None, mul=mul):
    """(e, r, s) under the key Q whose verification computes R = u1 G + u2 Q (u1, u2 in [0, N), u2 != 0).
    r defaults to x(R) mod N, which makes the signature valid; any other r in [1, N-1] keeps the walk
    (s = r / u2, e = u1 s still give back u1 and u2) and makes it invalid, and is the only choice when
    R is the point at infinity."""
    assert 0 <= u1 < N and 0 < u2 < N
    return _sig(add(mul(u1, G), mul(u2, Q)), u1, u2, r)


def forge_R(R, u1, u2, r=None, mul=mul):
    """(Q, e, r, s) with Q = (R - u1 G) / u2, so that u1 G + u2 Q = R."""
    assert 0 <= u1 < N and 0 < u2 < N and R is not None
    Q = mul(pow(u2, -1, N), add(R, neg(mul(u1, G))))
    if Q is None:
        raise ValueError("R = u1 G: no key")
    return (Q,) + _sig(R, u1, u2, r)


_tables = {}


def comb_table(Q):
    """T[j][b] = b 256^j Q for the 32 byte positions and the digits 1..255 (T[j][0] = None), cached per key."""
    t = _tables.get(Q)
    if t is None:
        t, Pj = [], Q
        for _ in range(32):
            row, acc = [None], None
            for _ in range(255):
                acc = add(acc, Pj)
                row.append(acc)
            t.append(row)
            Pj = add(acc, Pj)
        _tables[Q] = t
    return t


def comb_mul(k, a):
    """k a (0 <= k < 2^256) from a's comb table: at most 32 additions. Same signature as mul."""
    t, acc = comb_table(a), None
    for j in range(32):
        acc = add(acc, t[j][(k >> (8 * j)) & 255])
    return acc


def comb_events(Q, e, r, s):
    """The branches k_p256_verify's walk takes for this signature, in order: "dbl@<j><G|Q>" (the
    accumulator equals the entry added), "opp@<j><G|Q>" (it is its negative: infinity), "from-inf@<j><G|Q>"
    (an addition into an infinite accumulator other than the very first addition), then "final-inf" or
    "x>=N" (x(R) in [N, p): only the second compare accepts). [] when r or s is out of range."""
    if not (1 <= r < N and 1 <= s < N):
        return []
    w = pow(s, -1, N)
    u1, u2 = e % N * w % N, r * w % N
    tg, tq = comb_table(G), comb_table(Q)
    ev, acc, first = [], None, True
    for j in range(32):
        for name, tab, u in (("G", tg, u1), ("Q", tq, u2)):
            d = (u >> (8 * j)) & 255
            if d == 0:
                continue
            T = tab[j][d]
            if acc is None:
                if not first:
                    ev.append(f"from-inf@{j}{name}")
                acc = T
            elif acc == T:
                ev.append(f"dbl@{j}{name}")
                acc = dbl(acc)
            elif acc[0] == T[0]:
                ev.append(f"opp@{j}{name}")
                acc = None
            else:
                acc = add(acc, T)
            first = False
    if acc is None:
        ev.append("final-inf")
    elif acc[0] >= N:
        ev.append("x>=N")
    return ev
