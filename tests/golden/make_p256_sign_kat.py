"""Writes tests/golden/p256_sign_kat.json: known answers for libhgx's P-256 signer,
computed by tests/signref.py alone (Python integers, hmac, hashlib).

    python tests/golden/make_p256_sign_kat.py

Every case holds d, the 32-byte digest, the RFC 6979 nonce k, r and s as 64 hex digits each, and the
public key. The cases: both RFC 6979 A.2.5 SHA-256 vectors (checked against the RFC's printed k, r, s
here); the edge digests 0, 1, N-1, N, N+1, 2^256-1 under two derived keys; the edge keys d = 1 and
d = N-1; and short values found by a search over a counter in the digest's preimage (r < 2^248,
s < 2^248, r < 2^240 within 100 000 tries), where a byte or decimal printer loses leading zeros.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import signref  # noqa: E402
from p256ref import N  # noqa: E402

RFC_D = 0xC9AFA9D845BA75166B5C215767B1D6934E50C3DB36E89B127B8A622B120F6721
RFC = {
    b"sample": (0xA6E3C57DD01ABE90086538398355DD4C3B17AA873382B0F24D6129493D8AAD60,
                0xEFD48B2AACB6A8FD1140DD9CD45E81D69D2C877B56AAF991C34D0EA84EAF3716,
                0xF7CB1C942D657C41D436C7A1B6E29F65F3E900DBB9AFF4064DC4AB2F843ACDA8),
    b"test": (0xD16B6AE827F17175E040871A1C7EC3500192C4C92677336EC2537ACAEE0008E0,
              0xF1ABB023518351CD71D881567B1EA663ED3EFCF6C5132B354F28D3B0B7D38367,
              0x019F4113742A2B14BD25926B49C649155F267E60D3814B4C0CC84250E46F0083),
}
SEARCH_TRIES = 100_000


def case(tag, d, digest):
    r, s, k = signref.sign(d, digest)
    return dict(tag=tag, d="%064x" % d, digest=digest.hex(), k="%064x" % k, r="%064x" % r, s="%064x" % s,
                pub=signref.pub65(d).hex())


def main():
    cases, notes = [], []
    for msg, (k, r, s) in RFC.items():
        c = case("rfc6979-a.2.5-" + msg.decode(), RFC_D, hashlib.sha256(msg).digest())
        assert (int(c["k"], 16), int(c["r"], 16), int(c["s"], 16)) == (k, r, s), c
        cases.append(c)
    for ki in (0, 1):
        for name, e in (("0", 0), ("1", 1), ("N-1", N - 1), ("N", N), ("N+1", N + 1), ("2^256-1", 2 ** 256 - 1)):
            cases.append(case(f"edge-digest-{name}-key{ki}", signref.priv(ki), e.to_bytes(32, "big")))
    for name, d in (("1", 1), ("N-1", N - 1)):
        cases.append(case(f"edge-key-{name}", d, hashlib.sha256(b"edge key " + name.encode()).digest()))
    d = signref.priv(2)
    want = {"short-r-248": lambda r, s: r < 2 ** 248, "short-s-248": lambda r, s: s < 2 ** 248,
            "short-r-240": lambda r, s: r < 2 ** 240}
    for i in range(SEARCH_TRIES):
        if not want:
            break
        dg = hashlib.sha256(b"hgx short value search %d" % i).digest()
        r, s, _ = signref.sign(d, dg)
        for tag in [t for t, f in want.items() if f(r, s)]:
            cases.append(case(f"{tag}-try{i}", d, dg))
            del want[tag]
    for tag in want:
        notes.append(f"{tag}: not found within {SEARCH_TRIES} tries")
    out = dict(comment="ECDSA P-256 / RFC 6979 (HMAC-SHA-256) known answers; written by make_p256_sign_kat.py",
               notes=notes, cases=cases)
    with open(os.path.join(HERE, "p256_sign_kat.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(len(cases), "cases;", notes or "every search hit")


if __name__ == "__main__":
    main()
