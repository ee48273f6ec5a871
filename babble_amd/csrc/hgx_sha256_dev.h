// Device-side SHA-256 shared by the batched hash (hgx_sha256.hip) and the event-body front end
// (hgx_goenc_dev.hip): the 64-round compression and the one-lane-per-message block reader.
//
// One lane hashes one message: the compression is fully unrolled in VGPRs (rotates are
// v_alignbit, Sigma/Ch/Maj v_bitop3). The work is VALU-bound (~1.5 k lane instructions per
// 64-byte block against ~68 bytes read), so there is no LDS staging: the lane streams its own
// message with 16-byte loads from the 16-byte-aligned address below each block (guarded: a
// 16-byte slice holding no message byte is not read), so a load may touch up to 15 bytes before
// the message's first byte and up to 15 bytes past its last byte, always inside the
// 16-byte-aligned span of the message. The Merkle-Damgard padding is built in registers.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace hgx {

__device__ __forceinline__ uint32_t rotr(uint32_t x, int n) { return __builtin_amdgcn_alignbit(x, x, n); }
// a ^ b ^ c in one v_bitop3_b32 (truth table 0x96)
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}

#define HGX_SHA_R(a, b, c, d, e, f, g, h, k, w)                                        \
    do {                                                                               \
        uint32_t t1 = h + xor3(rotr(e, 6), rotr(e, 11), rotr(e, 25)) + ((e & f) ^ (~e & g)) + (k) + (w); \
        uint32_t t2 = xor3(rotr(a, 2), rotr(a, 13), rotr(a, 22)) + ((a & b) ^ (c & (a ^ b)));          \
        d += t1;                                                                       \
        h = t1 + t2;                                                                   \
    } while (0)

__device__ __forceinline__ void sha256_compress(uint32_t st[8], uint32_t w[16]) {
    constexpr uint32_t K[64] = {
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
        0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
        0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
        0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
        0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
        0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
        0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
        0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
#pragma unroll
    for (int i = 0; i < 64; i += 8) {
        if (i >= 16) {
            // schedule the next 8 words in place (w is a rolling 16-word window)
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int t = (i + j) & 15;
                const uint32_t x15 = w[(t + 1) & 15], x2 = w[(t + 14) & 15];
                w[t] += xor3(rotr(x15, 7), rotr(x15, 18), x15 >> 3) + w[(t + 9) & 15] +
                        xor3(rotr(x2, 17), rotr(x2, 19), x2 >> 10);
            }
        }
        HGX_SHA_R(a, b, c, d, e, f, g, h, K[i + 0], w[(i + 0) & 15]);
        HGX_SHA_R(h, a, b, c, d, e, f, g, K[i + 1], w[(i + 1) & 15]);
        HGX_SHA_R(g, h, a, b, c, d, e, f, K[i + 2], w[(i + 2) & 15]);
        HGX_SHA_R(f, g, h, a, b, c, d, e, K[i + 3], w[(i + 3) & 15]);
        HGX_SHA_R(e, f, g, h, a, b, c, d, K[i + 4], w[(i + 4) & 15]);
        HGX_SHA_R(d, e, f, g, h, a, b, c, K[i + 5], w[(i + 5) & 15]);
        HGX_SHA_R(c, d, e, f, g, h, a, b, K[i + 6], w[(i + 6) & 15]);
        HGX_SHA_R(b, c, d, e, f, g, h, a, K[i + 7], w[(i + 7) & 15]);
    }
    st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}
#undef HGX_SHA_R

// SHA-256 of the message data[off, off + len) by one lane; the digest as 8 big-endian words to
// out (4-byte aligned). SUFFIX: the message is those bytes followed by the one byte `suffix`
// (EventBody.Marshal's trailing '\n' after a body that lies inside the event's text); the byte
// of data at off + len is then inside the loaded span (its value is ignored), so the caller keeps
// the 16-byte-aligned span of [off, off + len] mapped.
template <bool SUFFIX>
__device__ __forceinline__ void sha256_message(const uint8_t* data, int64_t off, int64_t mlen, uint32_t suffix,
                                               uint32_t* out) {
    const int64_t len = SUFFIX ? mlen + 1 : mlen;
    uint32_t st[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    const int64_t nb = (len + 72) >> 6;   // ceil((len + 1 + 8) / 64)
    const uintptr_t a0 = (uintptr_t)(data + off);
    // 16-byte loads from the aligned-down address: sh16 = q*4 + sh bytes of lead-in
    const int sh16 = (int)(a0 & 15), q = sh16 >> 2, sh = sh16 & 3;
    const uint4* vp = (const uint4*)(data + (off - sh16));   // derived from data: stays a global load
    const uint64_t bits = (uint64_t)len * 8;
    // one 16-byte slice per load that holds a message byte; 5 slices cover a 64-byte block
    auto load_block = [&](int64_t b, uint4 (&E)[5]) {
        const int64_t rem = len - 64 * b;
#pragma unroll
        for (int t = 0; t < 5; t++) E[t] = (16 * t - sh16 < rem) ? vp[4 * b + t] : make_uint4(0, 0, 0, 0);
    };
    uint4 E[5];
    load_block(0, E);
    for (int64_t b = 0; b < nb; b++) {
        const int64_t rem = len - 64 * b;   // message bytes from this block's first byte on
        uint32_t D[20];
#pragma unroll
        for (int t = 0; t < 5; t++) { D[4 * t] = E[t].x; D[4 * t + 1] = E[t].y; D[4 * t + 2] = E[t].z; D[4 * t + 3] = E[t].w; }
        if (b + 1 < nb) load_block(b + 1, E);   // next block in flight during this compression
        uint32_t d[17];
#pragma unroll
        for (int j = 0; j < 17; j++) d[j] = q == 0 ? D[j] : q == 1 ? D[j + 1] : q == 2 ? D[j + 2] : D[j + 3];
        uint32_t w[16];
        const int r = (int)(rem < 64 ? rem : 64);   // valid bytes in this block, 32-bit math below
        // SUFFIX: the message's last byte (index len - 1) is `suffix`, in this block when 1 <= rem <= 64
        const int ks = SUFFIX && rem >= 1 && rem <= 64 ? (r - 1) >> 2 : -1;
        const int ss = 24 - 8 * ((r - 1) & 3);
#pragma unroll
        for (int k = 0; k < 16; k++) {
            uint32_t x = __builtin_bswap32(__builtin_amdgcn_alignbyte(d[k + 1], d[k], sh));
            if (SUFFIX && k == ks) x = (x & ~(0xFFu << ss)) | (suffix << ss);
            const int v = r - 4 * k;   // valid bytes of word k
            uint32_t y;
            if (v >= 4) y = x;
            else if (v > 0) y = (x & (0xFFFFFFFFu << (32 - 8 * v))) | (0x80u << (24 - 8 * v));
            else y = (v == 0) ? 0x80000000u : 0u;
            w[k] = y;
        }
        if (b == nb - 1) {   // the last block (rem <= 55) carries the bit length
            w[14] = (uint32_t)(bits >> 32);
            w[15] = (uint32_t)bits;
        }
        sha256_compress(st, w);
    }
#pragma unroll
    for (int k = 0; k < 8; k++) out[k] = __builtin_bswap32(st[k]);
}

}  // namespace hgx
