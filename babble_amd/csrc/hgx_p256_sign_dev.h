// Device-side ECDSA P-256 signing (Event.Sign, hashgraph/event.go:129-140 = crypto.Sign,
// crypto/utils.go:37-39), one lane per signature, shared by the batched signer (hgx_p256_sign.hip)
// and the signing id pass (hgx_goenc_dev.hip). DESIGN.md §3.16.
//
//   e = digest (32 bytes, big-endian) reduced once modulo N, as the verify kernel reduces it;
//   k = the RFC 6979 section 3.2 nonce for (d, digest) with HMAC-SHA-256 (qlen = hlen = 256: no
//       shifting, no additional data);
//   (X : Y : Z) = k G from G's fixed-base comb (at most 32 mixed additions, no doubling);
//   x = X / Z^2 (one Fermat inversion mod p), r = x mod N (x < p < 2N: one subtraction);
//   s = k^-1 (e + r d) mod N (one Fermat inversion mod N); s is not normalised to the low half.
//
// The nonce is deterministic where Go's is random: any verifier accepts either, and a signed chain
// is the same on every run. The comb lookups are indexed by the nonce's bytes and the DRBG's
// candidate test branches on k: NOT constant time (a memory-access side channel towards anything
// that shares the device).
//
// HMAC works on SHA-256 words throughout (a 32-byte string = 8 big-endian words, word j = limb 7 - j
// of the Fe): key and message blocks are assembled in registers with shifts of whole words, and one
// HMAC is a loop over its (at most) five compressions so that the 64 unrolled rounds appear once per
// call site. No array here is indexed by a runtime value.
#pragma once

#include "hgx_p256_dev.h"
#include "hgx_sha256_dev.h"

namespace hgx {
namespace p256 {

// HMAC-SHA-256 with the 32-byte key K over one of the DRBG's three messages:
//   mode 0: V                 (32 bytes)
//   mode 1: V || tag          (33 bytes)
//   mode 2: V || tag || x || h (97 bytes: int2octets(d), bits2octets(digest))
// out may be K or V.
__device__ __forceinline__ void hmac_drbg(uint32_t out[8], const uint32_t K[8], const uint32_t V[8], int mode,
                                          uint32_t tag, const uint32_t x[8], const uint32_t h[8]) {
    uint32_t st[8], inner[8];
#pragma unroll
    for (int j = 0; j < 8; j++) { st[j] = 0; inner[j] = 0; }
#pragma unroll 1
    for (int ph = 0; ph < 5; ph++) {
        if (ph == 2 && mode != 2) continue;
        uint32_t w[16];
        if (ph == 0 || ph == 3) {   // a fresh hash whose first block is K xor ipad / opad
            const uint32_t pad = ph == 0 ? 0x36363636u : 0x5c5c5c5cu;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                w[j] = K[j] ^ pad;
                w[8 + j] = pad;
                if (ph == 3) inner[j] = st[j];
            }
            st[0] = 0x6a09e667; st[1] = 0xbb67ae85; st[2] = 0x3c6ef372; st[3] = 0xa54ff53a;
            st[4] = 0x510e527f; st[5] = 0x9b05688c; st[6] = 0x1f83d9ab; st[7] = 0x5be0cd19;
        } else if (ph == 1) {       // message bytes 0..63
#pragma unroll
            for (int j = 0; j < 8; j++) w[j] = V[j];
            if (mode == 2) {
                w[8] = (tag << 24) | (x[0] >> 8);
#pragma unroll
                for (int j = 0; j < 7; j++) w[9 + j] = (x[j] << 24) | (x[j + 1] >> 8);
            } else {
                w[8] = mode == 1 ? (tag << 24) | 0x00800000u : 0x80000000u;
#pragma unroll
                for (int j = 9; j < 15; j++) w[j] = 0;
                w[15] = mode == 1 ? 8 * (64 + 33) : 8 * (64 + 32);
            }
        } else if (ph == 2) {       // mode 2: x's last byte, h, the padding
            w[0] = (x[7] << 24) | (h[0] >> 8);
#pragma unroll
            for (int j = 1; j < 8; j++) w[j] = (h[j - 1] << 24) | (h[j] >> 8);
            w[8] = (h[7] << 24) | 0x00800000u;
#pragma unroll
            for (int j = 9; j < 15; j++) w[j] = 0;
            w[15] = 8 * (64 + 97);
        } else {                    // the outer hash's second block: the inner digest
#pragma unroll
            for (int j = 0; j < 8; j++) w[j] = inner[j];
            w[8] = 0x80000000u;
#pragma unroll
            for (int j = 9; j < 15; j++) w[j] = 0;
            w[15] = 8 * (64 + 32);
        }
        sha256_compress(st, w);
    }
#pragma unroll
    for (int j = 0; j < 8; j++) out[j] = st[j];
}

// K = HMAC_K(V || tag [|| x || h]); V = HMAC_K(V)   (RFC 6979 3.2 steps d+e, f+g, and h.3's update)
__device__ __forceinline__ void drbg_update(uint32_t K[8], uint32_t V[8], uint32_t tag, bool with_data,
                                            const uint32_t x[8], const uint32_t h[8]) {
#pragma unroll 1
    for (int half = 0; half < 2; half++) {
        if (half == 0) hmac_drbg(K, K, V, with_data ? 2 : 1, tag, x, h);
        else hmac_drbg(V, K, V, 0, 0, x, h);
    }
}

// acc += (x2, y2): pmadd (madd-2007-bl with the infinity / doubling / opposite cases) with every case's
// result in whole values that are selected at the end. pmadd's early returns write only part of their
// output, which the compiler answers with a Pt in scratch (100 bytes per lane); here all 24 words are
// defined on every path and stay in registers.
__device__ __forceinline__ void pmadd_acc(Pt& acc, const Fe x2, const Fe y2) {
    Fe X3, Y3, Z3;
#pragma unroll
    for (int i = 0; i < 8; i++) { X3[i] = 0; Y3[i] = 0; Z3[i] = 0; }   // the point at infinity
    if (is_zero(acc.Z)) {
        cpy(X3, x2);
        cpy(Y3, y2);
        cpy(Z3, kOneP);
    } else {
        Fe z1z1, u2, s2, t, H, r;
        mmul<ModP>(z1z1, acc.Z, acc.Z);
        mmul<ModP>(u2, x2, z1z1);
        mmul<ModP>(t, acc.Z, z1z1);
        mmul<ModP>(s2, y2, t);
        msub<ModP>(H, u2, acc.X);
        msub<ModP>(r, s2, acc.Y);
        if (!is_zero(H)) {
            Fe HH, I, J, V;
            mmul<ModP>(HH, H, H);
            madd<ModP>(I, HH, HH);
            madd<ModP>(I, I, I);            // 4 HH
            mmul<ModP>(J, H, I);
            madd<ModP>(r, r, r);            // 2 (S2 - Y1)
            mmul<ModP>(V, acc.X, I);
            mmul<ModP>(X3, r, r);
            msub<ModP>(X3, X3, J);
            msub<ModP>(X3, X3, V);
            msub<ModP>(X3, X3, V);
            msub<ModP>(t, V, X3);
            mmul<ModP>(Y3, r, t);
            mmul<ModP>(t, acc.Y, J);
            madd<ModP>(t, t, t);
            msub<ModP>(Y3, Y3, t);
            madd<ModP>(t, acc.Z, H);
            mmul<ModP>(Z3, t, t);
            msub<ModP>(Z3, Z3, z1z1);
            msub<ModP>(Z3, Z3, HH);
        } else if (is_zero(r) && !is_zero(acc.Y)) {   // the same point: dbl-2001-b (a = -3), as pdbl
            Fe delta, gamma, beta, alpha, t1, t2, b4, b8, g2;
            mmul<ModP>(delta, acc.Z, acc.Z);
            mmul<ModP>(gamma, acc.Y, acc.Y);
            mmul<ModP>(beta, acc.X, gamma);
            msub<ModP>(t1, acc.X, delta);
            madd<ModP>(t2, acc.X, delta);
            mmul<ModP>(alpha, t1, t2);
            madd<ModP>(t1, alpha, alpha);
            madd<ModP>(alpha, t1, alpha);
            madd<ModP>(b4, beta, beta);
            madd<ModP>(b4, b4, b4);
            madd<ModP>(b8, b4, b4);
            mmul<ModP>(X3, alpha, alpha);
            msub<ModP>(X3, X3, b8);
            madd<ModP>(t1, acc.Y, acc.Z);
            mmul<ModP>(Z3, t1, t1);
            msub<ModP>(Z3, Z3, gamma);
            msub<ModP>(Z3, Z3, delta);
            mmul<ModP>(g2, gamma, gamma);
            madd<ModP>(g2, g2, g2);
            madd<ModP>(g2, g2, g2);
            madd<ModP>(g2, g2, g2);
            msub<ModP>(t1, b4, X3);
            mmul<ModP>(t2, alpha, t1);
            msub<ModP>(Y3, t2, g2);
        }   // else the opposite point: infinity
    }
    cpy(acc.X, X3);
    cpy(acc.Y, Y3);
    cpy(acc.Z, Z3);
}

// k G from G's comb table (k != 0 as an integer below 2^256): the next position's entry is loaded
// while the current one is added
__device__ __forceinline__ void comb_mul_g(Pt& acc, const Fe k, const uint32_t* __restrict__ tg) {
#pragma unroll
    for (int q = 0; q < 8; q++) { acc.X[q] = 0; acc.Y[q] = 0; acc.Z[q] = 0; }
    Fe gx, gy;
    uint32_t d1 = k[0] & 255u;
    ent_load(gx, gy, tg + (size_t)d1 * kEntWords);
    for (int j = 0; j < kCombPos; j++) {
        Fe ngx, ngy;
        uint32_t n1 = 0;
        if (j + 1 < kCombPos) {
            n1 = byte_at(k, j + 1);
            ent_load(ngx, ngy, tg + ((size_t)(j + 1) * kCombDig + n1) * kEntWords);
        }
        if (d1) pmadd_acc(acc, gx, gy);
        d1 = n1;
        cpy(gx, ngx); cpy(gy, ngy);
    }
}

// r, s (plain limbs) of the signature of the digest e_in (limbs of the 32 bytes read as a big-endian
// integer, not yet reduced) under the private key d (limbs, 1 <= d < N).
__device__ __forceinline__ void p256_sign_one(Fe r, Fe s, const Fe d, const Fe e_in, const uint32_t* __restrict__ tg) {
    Fe e;
    cpy(e, e_in);
    if (!lt(e, ModN::n)) {   // e < 2^256 < 2N: one subtraction (this is also bits2octets)
        Fe z = {0, 0, 0, 0, 0, 0, 0, 0};
        madd<ModN>(e, e, z);
    }
    uint32_t x[8], h[8], K[8], V[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        x[j] = d[7 - j];
        h[j] = e[7 - j];
        K[j] = 0;               // 3.2.c
        V[j] = 0x01010101u;     // 3.2.b
    }
    // 3.2.d-g
#pragma unroll 1
    for (uint32_t tag = 0; tag < 2; tag++) drbg_update(K, V, tag, true, x, h);
    // 3.2.h: candidates until one is in [1, N-1] and gives r != 0 and s != 0
    for (;;) {
        hmac_drbg(V, K, V, 0, 0, x, h);   // h.2 (tlen = qlen after one round)
        Fe k;
#pragma unroll
        for (int j = 0; j < 8; j++) k[j] = V[7 - j];   // h.3: bits2int(T)
        if (!is_zero(k) && lt(k, ModN::n)) {
            Pt acc;
            comb_mul_g(acc, k, tg);
            // x(k G) = X / Z^2, out of Montgomery form, then mod N
            Fe zi, zi2, xm;
            mpow_m2<ModP>(zi, acc.Z, kPm2, kOneP);
            mmul<ModP>(zi2, zi, zi);
            mmul<ModP>(xm, acc.X, zi2);
            Fe one = {1, 0, 0, 0, 0, 0, 0, 0};
            mmul<ModP>(r, xm, one);
            if (!lt(r, ModN::n)) {
                Fe z = {0, 0, 0, 0, 0, 0, 0, 0};
                madd<ModN>(r, r, z);
            }
            // s = k^-1 (e + r d)
            Fe km, ki, dm, t;
            mmul<ModN>(km, k, kR2N);
            mpow_m2<ModN>(ki, km, kNm2, kOneN);   // k^-1 R
            mmul<ModN>(dm, d, kR2N);              // d R
            mmul<ModN>(t, r, dm);                 // r d
            madd<ModN>(t, t, e);
            mmul<ModN>(s, t, ki);
            if (!is_zero(r) && !is_zero(s)) break;
        }
        drbg_update(K, V, 0, false, x, h);   // h.3: K = HMAC_K(V || 0x00), V = HMAC_K(V)
    }
}

// limbs -> 32 big-endian bytes at a 4-byte aligned address
__device__ __forceinline__ void store_be(uint8_t* out, const Fe a) {
    uint32_t* o = (uint32_t*)out;
#pragma unroll
    for (int j = 0; j < 8; j++) o[j] = __builtin_bswap32(a[7 - j]);
}

// 32 big-endian bytes at a 4-byte aligned address -> limbs
__device__ __forceinline__ void load_be_words(Fe r, const uint8_t* b) {
    const uint32_t* p = (const uint32_t*)b;
#pragma unroll
    for (int j = 0; j < 8; j++) r[7 - j] = __builtin_bswap32(p[j]);
}

}  // namespace p256
}  // namespace hgx
