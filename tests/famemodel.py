"""numpy model of k_fame_voter's mapping, and its inputs taken from the CPU oracle.

The model follows the kernel step by step, not DecideFame's text: a block per (round i, slice of
chains), a wave per 64 voter chains, vote words and decisions as ballots of a wave, the witness
mask of round j - 1 ANDed into the voters' S rows, one decision per (wave, x) merged lowest wave
first. It runs on the CPU, so the mapping is checked against the oracle without a GPU."""
import numpy as np

U64 = np.uint64


def ballot(pred) -> int:
    """bit l = pred[l] over the 64 lanes of a wave"""
    return int(np.packbits(np.asarray(pred, bool), bitorder="little").view("<u8")[0])


def popc_rows(a) -> np.ndarray:
    """popcount over the words of each row of a uint64 [rows, words] array"""
    a = np.ascontiguousarray(a, U64)
    return np.unpackbits(a.view(np.uint8), axis=-1).sum(axis=-1).astype(np.int64)


def ctz(m: int) -> int:
    return (m & -m).bit_length() - 1


def model_fame(n, LR, wstat, S, see, coin, sm, XS=64, r0=0):
    """wstat [R, n] bool: chain c has a witness of round r.
    S [R, n, NW] uint64: row of voter chain y in round j, bit w = y strongly sees the candidate of
        chain w in round j - 1 (unmasked: rows of non-witnesses and bits of non-witnesses are junk).
    see [R, n, n] bool: see[j][y][x] = the candidate y of round j sees the candidate x of j - 1.
    coin [R, n] bool. Returns (fame [R, n] int8: 1 / 2 / 0 at the witnesses, coin rounds walked)."""
    NW = (n + 63) // 64
    R = wstat.shape[0]
    pad = NW * 64
    fame = np.zeros((R, n), np.int8)
    coin_rounds = 0

    def lanes(row, fill=False):   # [n] -> [NW, 64]
        out = np.full(pad, fill, dtype=np.asarray(row).dtype)
        out[:n] = row
        return out.reshape(NW, 64)

    for i in range(r0, R):
        if i > LR:
            continue
        for xt in range((n + XS - 1) // XS):
            x0 = xt * XS
            nxs = min(XS, n - x0)
            isx = np.zeros(64, bool)
            isx[:nxs] = wstat[i, x0:x0 + nxs]
            xmask = ballot(isx)
            if xmask == 0:
                continue
            xl_of = np.nonzero(isx)[0]
            if i + 2 > LR:
                fame[i, x0 + xl_of] = 0
                continue
            V = np.zeros((2, 64, NW), U64)
            wm = np.zeros((2, NW), U64)
            # j = i + 1
            act = lanes(wstat[i + 1])
            for q in range(NW):
                am = ballot(act[q])
                wm[(i + 1) & 1][q] = am
                for xl in range(nxs):
                    sees = lanes(see[i + 1][:, x0 + xl])[q] & isx[xl]
                    V[0][xl][q] = ballot(sees) & am
            dec = np.zeros(64, np.int64)   # lane t: chain x0 + t, the same in every wave
            cur = 0
            for j in range(i + 2, LR + 1):
                normal = (j - i) % n != 0
                coin_rounds += 0 if normal else 1
                und = xmask & ballot(dec == 0)
                act = lanes(wstat[j])
                cj = lanes(coin[j])
                nv = np.zeros((NW, 64), U64)
                nd = np.zeros((NW, 64), np.int64)
                for q in range(NW):
                    am = ballot(act[q])
                    wm[j & 1][q] = am
                    rows = np.zeros((64, NW), U64)
                    ys = np.arange(64 * q, min(64 * q + 64, n))
                    rows[:len(ys)] = S[j, ys] & wm[(j - 1) & 1][None, :]
                    rows[~act[q]] = 0
                    tot = popc_rows(rows)
                    rem = und
                    while rem:
                        xl = ctz(rem)
                        rem &= rem - 1
                        yays = popc_rows(rows & V[cur][xl][None, :])
                        nays = tot - yays
                        v = yays >= nays
                        strong = np.where(v, yays, nays) >= sm
                        if normal:
                            vb = ballot(v)
                            d = ballot(strong) & am
                            nd[q][xl] = 0 if d == 0 else 2 - ((vb >> ctz(d)) & 1)
                            bits = vb & am
                        else:
                            bits = ballot(np.where(strong, v, cj[q])) & am
                        nv[q][xl] = bits
                for q in range(NW):
                    V[cur ^ 1][:, q] = nv[q]
                if normal:
                    for q in range(NW):   # the lowest deciding chain wins
                        dec = np.where(dec != 0, dec, nd[q])
                if xmask & ballot(dec == 0) == 0:
                    break
                cur ^= 1
            fame[i, x0 + xl_of] = dec[xl_of]
    return fame, coin_rounds


def plain_fame(n, LR, wstat, S, see, coin, sm):
    """DecideFame's text (hashgraph.go:649-730) over the same arrays, one x at a time with the voters in
    ascending chain order, so the first decider is the lowest chain. For inputs that no trace gives
    (random arrays, where deciders of a round may disagree and n = 3 reaches a coin round)."""
    R = wstat.shape[0]
    fame = np.zeros((R, n), np.int8)
    coin_rounds = 0
    bit = lambda j, y, w: (int(S[j, y, int(w) >> 6]) >> (int(w) & 63)) & 1
    for i in range(R):
        if i > LR or i + 2 > LR:
            continue
        for x in np.nonzero(wstat[i])[0]:
            votes = {}
            for j in range(i + 1, LR + 1):
                done = False
                coin_rounds += 1 if j > i + 1 and (j - i) % n == 0 else 0
                for y in np.nonzero(wstat[j])[0]:
                    if j == i + 1:
                        votes[(j, y)] = bool(see[j, y, x])
                        continue
                    yays = nays = 0
                    for w in np.nonzero(wstat[j - 1])[0]:
                        if bit(j, y, w):
                            if votes.get((j - 1, w), False):
                                yays += 1
                            else:
                                nays += 1
                    v = yays >= nays
                    t = yays if v else nays
                    if (j - i) % n != 0:
                        votes[(j, y)] = v
                        if t >= sm:
                            fame[i, x] = 1 if v else 2
                            done = True
                            break
                    else:
                        votes[(j, y)] = v if t >= sm else bool(coin[j, y])
                if done:
                    break
    return fame, coin_rounds


def random_inputs(n, R, seed, p_wit=0.85, p_s=0.7, p_see=0.5):
    """arrays of model_fame's shapes from a generator, not from a trace"""
    rng = np.random.default_rng(seed)
    NW = (n + 63) // 64
    wstat = rng.random((R, n)) < p_wit
    bits = rng.random((R, n, NW * 64)) < p_s
    S = np.packbits(bits, axis=-1, bitorder="little").view("<u8").reshape(R, n, NW).astype(U64)
    see = rng.random((R, n, n)) < p_see
    coin = rng.random((R, n)) < 0.5
    return wstat, S, see, coin


def inputs_from_oracle(o, t):
    """The kernel's inputs, from an oracle that has run consensus on trace t in one batch.
    Returns (LR, wit [R, n] gids or -1, wstat, S, see, coin). What the kernel must mask is junk here on
    purpose: rows of chains with no witness in the round are all ones, and an S row covers the
    candidates of the round before (the first event of a chain at or past that round), witness or not."""
    L, h, n = o.L, o.h, t.n
    E = o.E()
    NW = (n + 63) // 64
    rnd = np.array([L.hgo_round(h, x) for x in range(E)], np.int64)
    LR = int(L.hgo_last_round(h))
    R = LR + 1
    creator = np.asarray(t.creator[:E])
    wit = np.full((R, n), -1, np.int64)
    for r in range(R):
        for g in o.round_witnesses(r):
            wit[r, creator[g]] = g
    chains = [np.nonzero(creator == c)[0] for c in range(n)]
    cand = np.full((R, n), -1, np.int64)
    for c in range(n):
        rr = rnd[chains[c]]   # non-decreasing along a chain
        for r in range(R):
            k = int(np.searchsorted(rr, r, side="left"))
            if k < len(rr):
                cand[r, c] = chains[c][k]
    wstat = wit >= 0
    S = np.full((R, n, NW), ~U64(0), U64)
    see = np.ones((R, n, n), bool)
    coin = np.ones((R, n), bool)
    for j in range(1, R):
        for y in range(n):
            gy = int(wit[j, y])
            if gy < 0:
                continue
            coin[j, y] = t.hash[gy][16] != 0
            bits = np.zeros(NW * 64, bool)
            for w in range(n):
                gw = int(cand[j - 1, w])
                if gw >= 0:
                    bits[w] = L.hgo_strongly_see(h, gy, gw) != 0
                gx = int(wit[j - 1, w])
                see[j, y, w] = gx >= 0 and L.hgo_see(h, gy, gx) != 0
            S[j, y] = np.packbits(bits, bitorder="little").view("<u8")
    return LR, wit, wstat, S, see, coin


def oracle_fame(o, wit):
    """fame [R, n] of the oracle at the witnesses (0 elsewhere)"""
    out = np.zeros(wit.shape, np.int8)
    for r, c in zip(*np.nonzero(wit >= 0)):
        out[r, c] = o.L.hgo_famous(o.h, int(wit[r, c]))
    return out
