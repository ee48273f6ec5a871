// Device-side P-256 arithmetic shared by the batched verify and the comb-table kernels
// (hgx_p256.hip), the signer (hgx_p256_sign.hip) and the signing id pass (hgx_goenc_dev.hip):
// 8 x 32-bit limbs, Montgomery multiplication (CIOS, v_mad_u64_u32) modulo p (field) and modulo N
// (scalars), Jacobian points with a = -3 doubling (dbl-2001-b), complete-case addition (add-2007-bl)
// and mixed addition (madd-2007-bl), Fermat inversion, and the fixed-base comb layout.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace hgx {
namespace p256 {

struct ModP {
    static constexpr uint32_t n[8] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x00000000u,
                                      0x00000000u, 0x00000000u, 0x00000001u, 0xFFFFFFFFu};
    static constexpr uint32_t n0 = 0x00000001u;   // -p^-1 mod 2^32
};
struct ModN {
    static constexpr uint32_t n[8] = {0xFC632551u, 0xF3B9CAC2u, 0xA7179E84u, 0xBCE6FAADu,
                                      0xFFFFFFFFu, 0xFFFFFFFFu, 0x00000000u, 0xFFFFFFFFu};
    static constexpr uint32_t n0 = 0xEE00BC4Fu;   // -N^-1 mod 2^32
};

// Montgomery constants (R = 2^256)
__device__ constexpr uint32_t kR2P[8] = {0x00000003u, 0x00000000u, 0xFFFFFFFFu, 0xFFFFFFFBu,
                                         0xFFFFFFFEu, 0xFFFFFFFFu, 0xFFFFFFFDu, 0x00000004u};
__device__ constexpr uint32_t kR2N[8] = {0xBE79EEA2u, 0x83244C95u, 0x49BD6FA6u, 0x4699799Cu,
                                         0x2B6BEC59u, 0x2845B239u, 0xF3D95620u, 0x66E12D94u};
__device__ constexpr uint32_t kOneP[8] = {0x00000001u, 0x00000000u, 0x00000000u, 0xFFFFFFFFu,
                                          0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFEu, 0x00000000u};
__device__ constexpr uint32_t kOneN[8] = {0x039CDAAFu, 0x0C46353Du, 0x58E8617Bu, 0x43190552u,
                                          0x00000000u, 0x00000000u, 0xFFFFFFFFu, 0x00000000u};
__device__ constexpr uint32_t kBm[8] = {0x29C4BDDFu, 0xD89CDF62u, 0x78843090u, 0xACF005CDu,
                                        0xF7212ED6u, 0xE5A220ABu, 0x04874834u, 0xDC30061Du};   // b R mod p
__device__ constexpr uint32_t kGx[8] = {0xD898C296u, 0xF4A13945u, 0x2DEB33A0u, 0x77037D81u,
                                        0x63A440F2u, 0xF8BCE6E5u, 0xE12C4247u, 0x6B17D1F2u};
__device__ constexpr uint32_t kGy[8] = {0x37BF51F5u, 0xCBB64068u, 0x6B315ECEu, 0x2BCE3357u,
                                        0x7C0F9E16u, 0x8EE7EB4Au, 0xFE1A7F9Bu, 0x4FE342E2u};
__device__ constexpr uint32_t kPm2[8] = {0xFFFFFFFDu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x00000000u,
                                         0x00000000u, 0x00000000u, 0x00000001u, 0xFFFFFFFFu};
__device__ constexpr uint32_t kNm2[8] = {0xFC63254Fu, 0xF3B9CAC2u, 0xA7179E84u, 0xBCE6FAADu,
                                         0xFFFFFFFFu, 0xFFFFFFFFu, 0x00000000u, 0xFFFFFFFFu};

typedef uint32_t Fe[8];

__device__ __forceinline__ void cpy(Fe r, const uint32_t* a) {
#pragma unroll
    for (int i = 0; i < 8; i++) r[i] = a[i];
}

__device__ __forceinline__ bool is_zero(const Fe a) {
    uint32_t x = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) x |= a[i];
    return x == 0;
}

__device__ __forceinline__ bool eq(const Fe a, const Fe b) {
    uint32_t x = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) x |= a[i] ^ b[i];
    return x == 0;
}

// a < b as 256-bit integers
__device__ __forceinline__ bool lt(const uint32_t* a, const uint32_t* b) {
    int64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int64_t x = (int64_t)a[i] - (int64_t)b[i] + br;
        br = x >> 32;
    }
    return br != 0;
}

// r = a b R^-1 mod M (inputs < M), CIOS
template <class M>
__device__ __forceinline__ void mmul(Fe r, const Fe a, const Fe b) {
    uint32_t t[10];
#pragma unroll
    for (int j = 0; j < 10; j++) t[j] = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint64_t c = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            c += (uint64_t)a[j] * b[i] + t[j];
            t[j] = (uint32_t)c;
            c >>= 32;
        }
        c += t[8];
        t[8] = (uint32_t)c;
        t[9] = (uint32_t)(c >> 32);
        const uint32_t m = t[0] * M::n0;
        c = ((uint64_t)m * M::n[0] + t[0]) >> 32;
#pragma unroll
        for (int j = 1; j < 8; j++) {
            c += (uint64_t)m * M::n[j] + t[j];
            t[j - 1] = (uint32_t)c;
            c >>= 32;
        }
        c += t[8];
        t[7] = (uint32_t)c;
        t[8] = t[9] + (uint32_t)(c >> 32);
    }
    uint32_t d[8];
    int64_t br = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int64_t x = (int64_t)t[j] - (int64_t)M::n[j] + br;
        d[j] = (uint32_t)x;
        br = x >> 32;
    }
    const bool ge = (t[8] != 0) || (br == 0);
#pragma unroll
    for (int j = 0; j < 8; j++) r[j] = ge ? d[j] : t[j];
}

template <class M>
__device__ __forceinline__ void madd(Fe r, const Fe a, const Fe b) {
    uint32_t s[8];
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        c += (uint64_t)a[j] + b[j];
        s[j] = (uint32_t)c;
        c >>= 32;
    }
    uint32_t d[8];
    int64_t br = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int64_t x = (int64_t)s[j] - (int64_t)M::n[j] + br;
        d[j] = (uint32_t)x;
        br = x >> 32;
    }
    const bool ge = (c != 0) || (br == 0);
#pragma unroll
    for (int j = 0; j < 8; j++) r[j] = ge ? d[j] : s[j];
}

template <class M>
__device__ __forceinline__ void msub(Fe r, const Fe a, const Fe b) {
    uint32_t s[8];
    int64_t br = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int64_t x = (int64_t)a[j] - (int64_t)b[j] + br;
        s[j] = (uint32_t)x;
        br = x >> 32;
    }
    if (br != 0) {   // a < b: add M back
        uint64_t c = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            c += (uint64_t)s[j] + M::n[j];
            s[j] = (uint32_t)c;
            c >>= 32;
        }
    }
    cpy(r, s);
}

// 32 big-endian bytes -> limbs
__device__ __forceinline__ void load_be(Fe r, const uint8_t* b) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint8_t* q = b + 28 - 4 * i;
        r[i] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | (uint32_t)q[3];
    }
}

struct Pt {
    Fe X, Y, Z;   // Montgomery form mod p; Z == 0 is the point at infinity
};

// dbl-2001-b (a = -3)
__device__ __forceinline__ void pdbl(Pt& o, const Pt& a) {
    if (is_zero(a.Z) || is_zero(a.Y)) {
#pragma unroll
        for (int i = 0; i < 8; i++) o.Z[i] = 0;
        return;
    }
    Fe delta, gamma, beta, alpha, t1, t2;
    mmul<ModP>(delta, a.Z, a.Z);
    mmul<ModP>(gamma, a.Y, a.Y);
    mmul<ModP>(beta, a.X, gamma);
    msub<ModP>(t1, a.X, delta);
    madd<ModP>(t2, a.X, delta);
    mmul<ModP>(alpha, t1, t2);
    madd<ModP>(t1, alpha, alpha);
    madd<ModP>(alpha, t1, alpha);   // 3 (X - delta)(X + delta)
    Fe b4, b8, X3;
    madd<ModP>(b4, beta, beta);
    madd<ModP>(b4, b4, b4);         // 4 beta
    madd<ModP>(b8, b4, b4);         // 8 beta
    mmul<ModP>(X3, alpha, alpha);
    msub<ModP>(X3, X3, b8);
    Fe Z3;
    madd<ModP>(t1, a.Y, a.Z);
    mmul<ModP>(Z3, t1, t1);
    msub<ModP>(Z3, Z3, gamma);
    msub<ModP>(Z3, Z3, delta);
    Fe g2;
    mmul<ModP>(g2, gamma, gamma);
    madd<ModP>(g2, g2, g2);
    madd<ModP>(g2, g2, g2);
    madd<ModP>(g2, g2, g2);         // 8 gamma^2
    msub<ModP>(t1, b4, X3);
    mmul<ModP>(t2, alpha, t1);
    msub<ModP>(o.Y, t2, g2);
    cpy(o.X, X3);
    cpy(o.Z, Z3);
}

// add-2007-bl with the equal / opposite / infinity cases
__device__ __forceinline__ void padd(Pt& o, const Pt& a, const Pt& b) {
    if (is_zero(a.Z)) { o = b; return; }
    if (is_zero(b.Z)) { o = a; return; }
    Fe z1z1, z2z2, u1, u2, s1, s2, t;
    mmul<ModP>(z1z1, a.Z, a.Z);
    mmul<ModP>(z2z2, b.Z, b.Z);
    mmul<ModP>(u1, a.X, z2z2);
    mmul<ModP>(u2, b.X, z1z1);
    mmul<ModP>(t, b.Z, z2z2);
    mmul<ModP>(s1, a.Y, t);
    mmul<ModP>(t, a.Z, z1z1);
    mmul<ModP>(s2, b.Y, t);
    Fe H, r;
    msub<ModP>(H, u2, u1);
    msub<ModP>(r, s2, s1);
    if (is_zero(H)) {
        if (is_zero(r)) {
            pdbl(o, a);
        } else {
#pragma unroll
            for (int i = 0; i < 8; i++) o.Z[i] = 0;
        }
        return;
    }
    Fe I, J, V, X3, Y3, Z3;
    madd<ModP>(t, H, H);
    mmul<ModP>(I, t, t);            // (2H)^2
    mmul<ModP>(J, H, I);
    madd<ModP>(r, r, r);            // 2 (S2 - S1)
    mmul<ModP>(V, u1, I);
    mmul<ModP>(X3, r, r);
    msub<ModP>(X3, X3, J);
    msub<ModP>(X3, X3, V);
    msub<ModP>(X3, X3, V);
    msub<ModP>(t, V, X3);
    mmul<ModP>(Y3, r, t);
    mmul<ModP>(t, s1, J);
    madd<ModP>(t, t, t);
    msub<ModP>(Y3, Y3, t);
    madd<ModP>(t, a.Z, b.Z);
    mmul<ModP>(Z3, t, t);
    msub<ModP>(Z3, Z3, z1z1);
    msub<ModP>(Z3, Z3, z2z2);
    mmul<ModP>(Z3, Z3, H);
    cpy(o.X, X3);
    cpy(o.Y, Y3);
    cpy(o.Z, Z3);
}

// madd-2007-bl: Jacobian a + affine (x2, y2) (Z2 = 1), with the infinity / doubling cases
__device__ __forceinline__ void pmadd(Pt& o, const Pt& a, const Fe x2, const Fe y2) {
    if (is_zero(a.Z)) {
        cpy(o.X, x2);
        cpy(o.Y, y2);
        cpy(o.Z, kOneP);
        return;
    }
    Fe z1z1, u2, s2, t, H, r;
    mmul<ModP>(z1z1, a.Z, a.Z);
    mmul<ModP>(u2, x2, z1z1);
    mmul<ModP>(t, a.Z, z1z1);
    mmul<ModP>(s2, y2, t);
    msub<ModP>(H, u2, a.X);
    msub<ModP>(r, s2, a.Y);
    if (is_zero(H)) {
        if (is_zero(r)) {
            pdbl(o, a);
        } else {
#pragma unroll
            for (int i = 0; i < 8; i++) o.Z[i] = 0;
        }
        return;
    }
    Fe HH, I, J, V, X3, Y3;
    mmul<ModP>(HH, H, H);
    madd<ModP>(I, HH, HH);
    madd<ModP>(I, I, I);            // 4 HH
    mmul<ModP>(J, H, I);
    madd<ModP>(r, r, r);            // 2 (S2 - Y1)
    mmul<ModP>(V, a.X, I);
    mmul<ModP>(X3, r, r);
    msub<ModP>(X3, X3, J);
    msub<ModP>(X3, X3, V);
    msub<ModP>(X3, X3, V);
    msub<ModP>(t, V, X3);
    mmul<ModP>(Y3, r, t);
    mmul<ModP>(t, a.Y, J);
    madd<ModP>(t, t, t);
    msub<ModP>(Y3, Y3, t);
    madd<ModP>(t, a.Z, H);
    mmul<ModP>(o.Z, t, t);
    msub<ModP>(o.Z, o.Z, z1z1);
    msub<ModP>(o.Z, o.Z, HH);
    cpy(o.X, X3);
    cpy(o.Y, Y3);
}

// a^(M - 2) (Montgomery form in and out), by square-and-multiply over a constant exponent
template <class M>
__device__ __forceinline__ void mpow_m2(Fe r, const Fe a, const uint32_t* e, const uint32_t* one) {
    cpy(r, one);
    for (int b = 255; b >= 0; b--) {
        mmul<M>(r, r, r);
        if ((e[b >> 5] >> (b & 31)) & 1u) mmul<M>(r, r, a);
    }
}

// comb table layout: [key][32 byte positions j][256 digits b][x | y] affine limbs (Montgomery form):
// entry (j, b) = b * 256^j * P; digit 0 unused. 512 KB per key; key nk is the base point G.
constexpr int kCombPos = 32, kCombDig = 256, kEntWords = 16;
constexpr size_t kTabWords = (size_t)kCombPos * kCombDig * kEntWords;

// byte j of a 256-bit scalar (j uniform: selects, not a dynamically indexed array in scratch)
__device__ __forceinline__ uint32_t byte_at(const Fe u, int j) {
    const int li = j >> 2;
    uint32_t w = u[0];
#pragma unroll
    for (int q = 1; q < 8; q++) w = li == q ? u[q] : w;
    return (w >> (8 * (j & 3))) & 255u;
}

__device__ __forceinline__ void ent_load(Fe x, Fe y, const uint32_t* __restrict__ t) {
    const uint4* t4 = (const uint4*)t;
    const uint4 a = t4[0], b = t4[1], c = t4[2], d = t4[3];
    x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
    y[0] = c.x; y[1] = c.y; y[2] = c.z; y[3] = c.w; y[4] = d.x; y[5] = d.y; y[6] = d.z; y[7] = d.w;
}

}  // namespace p256
}  // namespace hgx
