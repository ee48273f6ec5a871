// Device helpers shared by the libhgx HIP translation units (gfx950, wave64).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>
#include <utility>

namespace hgx {

__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63); }

// exclusive scan of one value per thread over a block of 256 threads (sh: 4 words of LDS); *total =
// the block's sum. Every thread of the block must call it.
__device__ __forceinline__ uint32_t block_excl_scan256(uint32_t v, uint32_t* sh, uint32_t* total) {
    // 256 threads: wave-level inclusive scan by shuffles, then wave totals
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    uint32_t x = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    if (lane == 63) sh[wave] = x;
    __syncthreads();
    uint32_t wbase = 0;
    for (int w = 0; w < wave; w++) wbase += sh[w];
    *total = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
    return wbase + x - v;
}

// Strongly-see count of 8-bit rebased coordinates, 4 per dword: window bytes hold LA' in [0, 126], the
// candidate's bytes nf = 128 - FD' with FD' in [1, 127] (127 = none), so LA' + nf lies in [1, 253]: no
// carry leaves a byte, and bit 7 is set exactly when LA' >= FD'. With no carries the add may span 64
// bits (one v_lshl_add_u64 per 8 coordinates instead of a v_sub per 4).
template <int HD>
__device__ __forceinline__ uint32_t swar_ge_count(const uint32_t (&v)[HD], const uint32_t (&nf)[HD]) {
    uint32_t c = 0;
    if constexpr (HD % 2 == 0) {
        // one chain of v_bcnt_u32_b32 with its accumulate operand (the empty asm keeps the compiler from
        // re-associating the sum into bcnt(x, 0) + v_add3 trees: 2.5 instead of 3 VALU per dword)
#pragma unroll
        for (int i = 0; i < HD / 2; i++) {
            const uint64_t s = ((((uint64_t)v[2 * i + 1]) << 32) | v[2 * i]) + ((((uint64_t)nf[2 * i + 1]) << 32) | nf[2 * i]);
            c = __builtin_popcount((uint32_t)s & 0x80808080u) + c;
            asm volatile("" : "+v"(c));
            c = __builtin_popcount((uint32_t)(s >> 32) & 0x80808080u) + c;
            asm volatile("" : "+v"(c));
        }
    } else {
#pragma unroll
        for (int d = 0; d < HD; d++) c += __builtin_popcount((v[d] + nf[d]) & 0x80808080u);
    }
    return c;
}
// a candidate row dword (bytes FD' with the validity bit cleared) as its nf bytes (128 - FD'); 127 = none -> 1
__device__ __forceinline__ uint32_t swar_nf(uint32_t fd7) { return 0x80808080u - fd7; }

__device__ __forceinline__ uint64_t group_mask(int gs, int grp) {
    return (gs >= 64) ? ~0ull : (((1ull << gs) - 1ull) << (gs * grp));
}

// Storage of the coordinate arrays LA / FDT. int32_t: the raw values
// (lastAncestors -1 = none, firstDescendants MaxInt32 = none). uint16_t ("compact",
// every Index < 65534 and n even): LA stored as value + 1 (none = 0, so the encoding
// is order-preserving and max() works on it directly), FD stored as is with
// none = 0xFFFF. Kernels decode to int32 before comparing with raw values.
template <typename CT>
struct Coord;
template <>
struct Coord<int32_t> {
    static constexpr int32_t kLaNone = -1;
    __device__ __forceinline__ static int32_t la(int32_t v) { return v; }
    __device__ __forceinline__ static int32_t enc_la(int32_t v) { return v; }
    __device__ __forceinline__ static int32_t fd(int32_t v) { return v; }
    __device__ __forceinline__ static int32_t enc_fd(int32_t v) { return v; }
};
template <>
struct Coord<uint16_t> {
    static constexpr int32_t kLaNone = 0;
    __device__ __forceinline__ static int32_t la(uint32_t v) { return (int32_t)v - 1; }
    __device__ __forceinline__ static uint16_t enc_la(int32_t v) { return (uint16_t)(v + 1); }
    __device__ __forceinline__ static int32_t fd(uint32_t v) { return v == 0xFFFFu ? 2147483647 : (int32_t)v; }
    __device__ __forceinline__ static uint16_t enc_fd(int32_t v) { return v >= 0xFFFF ? (uint16_t)0xFFFF : (uint16_t)v; }
};

// order LDS accesses of one wave (lanes exchange data through LDS without a block barrier)
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// f(std::integral_constant<int, 0>) ... f(std::integral_constant<int, N - 1>): a loop whose index is a
// compile-time constant in the body (register arrays indexed by it never go to scratch)
template <int... I, class F>
__device__ __forceinline__ void static_for_seq(std::integer_sequence<int, I...>, F&& f) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    static_for_seq(std::make_integer_sequence<int, N>{}, f);
}

// the value lane (lane ^ D) of the wave holds, D a power of two, without LDS storage: DPP quad_perm for
// D = 1, 2 and row_ror:8 for D = 8 (inside a row of 16 a rotation by 8 is the xor), ds_swizzle in bit
// mode for D = 4, 16 (and 0x1F, xor D, inside each half of the wave), a bpermute across the halves.
// Every lane of the wave must be active.
template <int D>
__device__ __forceinline__ uint32_t lane_xor_u32(uint32_t v) {
    static_assert(D == 1 || D == 2 || D == 4 || D == 8 || D == 16 || D == 32, "lane distance");
    if constexpr (D == 1) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);   // [1,0,3,2]
    else if constexpr (D == 2) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true);   // [2,3,0,1]
    else if constexpr (D == 8) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xF, 0xF, true);
    else if constexpr (D == 32) return (uint32_t)__shfl_xor((int)v, 32);
    else return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x1F | (D << 10));
}
template <int D>
__device__ __forceinline__ uint64_t lane_xor_u64(uint64_t v) {
    return ((uint64_t)lane_xor_u32<D>((uint32_t)(v >> 32)) << 32) | lane_xor_u32<D>((uint32_t)v);
}

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t x) {
    for (int o = 32; o >= 1; o >>= 1) {
        const uint64_t y = __shfl_xor(x, o);
        x = y < x ? y : x;
    }
    return x;
}

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t x) {
    for (int o = 32; o >= 1; o >>= 1) {
        const uint64_t y = __shfl_xor(x, o);
        x = y > x ? y : x;
    }
    return x;
}

// Wave-cooperative exact selection: the K-th smallest (0-based) of the valid values
// held by the wave (CPL per lane). Radix select on (v - min) with 8-bit buckets from
// the top set bit of the range down: each pass histograms the still-active values in
// a 256-entry LDS scratch owned by this wave, finds the bucket holding rank K by a
// wave prefix scan and keeps only that bucket. ceil(bits(range)/8) passes (<= 8).
// Requires 0 <= K < #valid. Every lane returns the result.
template <int CPL>
__device__ uint64_t wave_select_kth(const uint64_t (&v)[CPL], const bool (&ok)[CPL], int K,
                                    uint32_t* __restrict__ hist) {
    const int lane = lane_id();
    uint64_t lo = ~0ull, hi = 0;
#pragma unroll
    for (int q = 0; q < CPL; q++)
        if (ok[q]) { lo = v[q] < lo ? v[q] : lo; hi = v[q] > hi ? v[q] : hi; }
    lo = wave_min_u64(lo);
    hi = wave_max_u64(hi);
    bool act[CPL];
#pragma unroll
    for (int q = 0; q < CPL; q++) act[q] = ok[q];
    uint64_t base = lo;
    uint64_t range = hi - lo;
    int k = K;
    while (range != 0) {
        int bits = 64 - __clzll((long long)range);
        const int shift = bits > 8 ? bits - 8 : 0;
#pragma unroll
        for (int t = 0; t < 4; t++) hist[lane * 4 + t] = 0;
        wave_lds_fence();
#pragma unroll
        for (int q = 0; q < CPL; q++)
            if (act[q]) atomicAdd(&hist[(uint32_t)((v[q] - base) >> shift)], 1u);
        wave_lds_fence();
        uint32_t h[4], s = 0;
#pragma unroll
        for (int t = 0; t < 4; t++) { h[t] = hist[lane * 4 + t]; s += h[t]; }
        uint32_t incl = s;   // inclusive prefix over lanes
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(incl, o);
            if (lane >= o) incl += y;
        }
        const uint32_t excl = incl - s;
        // the lane whose [excl, incl) holds k owns the bucket
        int bucket = -1;
        uint32_t below = 0;
        if ((uint32_t)k >= excl && (uint32_t)k < incl) {
            uint32_t acc = excl;
#pragma unroll
            for (int t = 0; t < 4; t++) {
                if (bucket < 0 && (uint32_t)k < acc + h[t]) { bucket = lane * 4 + t; below = acc; }
                acc += h[t];
            }
        }
        const uint64_t bm = __ballot(bucket >= 0);
        const int src = __ffsll((unsigned long long)bm) - 1;
        bucket = __shfl(bucket, src);
        below = __shfl(below, src);
        wave_lds_fence();
        k -= (int)below;
        const uint64_t nb = base + ((uint64_t)bucket << shift);
#pragma unroll
        for (int q = 0; q < CPL; q++) act[q] = act[q] && ((v[q] - base) >> shift) == (uint64_t)bucket;
        if (shift == 0) return nb;
        const uint64_t top = nb + ((1ull << shift) - 1);
        base = nb;
        range = (top < hi ? top : hi) - nb;
        // shrink to the actual active values for a tighter next pass
        uint64_t alo = ~0ull, ahi = 0;
#pragma unroll
        for (int q = 0; q < CPL; q++)
            if (act[q]) { alo = v[q] < alo ? v[q] : alo; ahi = v[q] > ahi ? v[q] : ahi; }
        alo = wave_min_u64(alo);
        ahi = wave_max_u64(ahi);
        base = alo;
        range = ahi - alo;
    }
    return base;
}

// Inclusive wave scans in lane order on DPP (GFX9 row_shr 1/2/4/8 within rows of 16,
// then row_bcast 15 / 31 across rows): a few VALU ops instead of ds_bpermute shuffles.
// Lanes without a DPP source keep the identity `id`.
#define HGX_DPP_SCAN(x, id, OP)                                                                  \
    do {                                                                                         \
        x = OP(x, (uint32_t)__builtin_amdgcn_update_dpp((int)(id), (int)(x), 0x111, 0xf, 0xf, false)); \
        x = OP(x, (uint32_t)__builtin_amdgcn_update_dpp((int)(id), (int)(x), 0x112, 0xf, 0xf, false)); \
        x = OP(x, (uint32_t)__builtin_amdgcn_update_dpp((int)(id), (int)(x), 0x114, 0xf, 0xf, false)); \
        x = OP(x, (uint32_t)__builtin_amdgcn_update_dpp((int)(id), (int)(x), 0x118, 0xf, 0xf, false)); \
        x = OP(x, (uint32_t)__builtin_amdgcn_update_dpp((int)(id), (int)(x), 0x142, 0xa, 0xf, false)); \
        x = OP(x, (uint32_t)__builtin_amdgcn_update_dpp((int)(id), (int)(x), 0x143, 0xc, 0xf, false)); \
    } while (0)
#define HGX_OP_ADD(a, b) ((a) + (b))
#define HGX_OP_MIN(a, b) min((a), (b))
#define HGX_OP_MAX(a, b) max((a), (b))

__device__ __forceinline__ uint32_t wave_scan_add_u32(uint32_t x) { HGX_DPP_SCAN(x, 0u, HGX_OP_ADD); return x; }
// wave-wide min / max of a u32, returned in an SGPR (lane 63 of the inclusive scan)
__device__ __forceinline__ uint32_t wave_reduce_min_u32(uint32_t x) {
    HGX_DPP_SCAN(x, 0xffffffffu, HGX_OP_MIN);
    return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}
__device__ __forceinline__ uint32_t wave_reduce_max_u32(uint32_t x) {
    HGX_DPP_SCAN(x, 0u, HGX_OP_MAX);
    return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}

// 32-bit k-th smallest for the common case (values already rebased): radix select with
// 8-bit digits from the top set bit of the range. Reductions and the bucket scan run on
// DPP, the chosen bucket is read from the owning lane with readlane, and the wave's
// 256-bin histogram (16-B aligned, lane l owns bins 4l..4l+3) is zeroed and read as one
// 16-B access per lane. Requires 0 <= K < #valid; every lane returns the result.
template <int CPL>
__device__ uint32_t wave_select_kth32(const uint32_t (&v)[CPL], const bool (&ok)[CPL], int K,
                                      uint32_t* __restrict__ hist) {
    const int lane = lane_id();
    uint32_t lo = 0xffffffffu, hi = 0;
#pragma unroll
    for (int q = 0; q < CPL; q++)
        if (ok[q]) { lo = min(lo, v[q]); hi = max(hi, v[q]); }
    lo = wave_reduce_min_u32(lo);
    hi = wave_reduce_max_u32(hi);
    const uint32_t range = hi - lo;
    if (range == 0) return lo;
    const int bits = 32 - __clz((int)range);
    uint32_t d[CPL];
    bool act[CPL];
#pragma unroll
    for (int q = 0; q < CPL; q++) { d[q] = v[q] - lo; act[q] = ok[q]; }
    uint4* __restrict__ h4 = (uint4*)hist;
    uint32_t prefix = 0;
    uint32_t k = (uint32_t)K;
    for (int shift = ((bits - 1) / 8) * 8; shift >= 0; shift -= 8) {
        h4[lane] = make_uint4(0u, 0u, 0u, 0u);
        wave_lds_fence();
#pragma unroll
        for (int q = 0; q < CPL; q++)
            if (act[q]) atomicAdd(&hist[(d[q] >> shift) & 255u], 1u);
        wave_lds_fence();
        const uint4 h = h4[lane];
        const uint32_t sum = h.x + h.y + h.z + h.w;
        const uint32_t incl = wave_scan_add_u32(sum);
        const uint32_t excl = incl - sum;
        // bucket of the k-th value inside this lane's 4 bins (meaningful in one lane)
        const uint32_t a1 = excl + h.x, a2 = a1 + h.y, a3 = a2 + h.z;
        const int bt = (k < a1) ? 0 : (k < a2) ? 1 : (k < a3) ? 2 : 3;
        const uint32_t below = (k < a1) ? excl : (k < a2) ? a1 : (k < a3) ? a2 : a3;
        const uint64_t bm = __ballot(k >= excl && k < incl);
        const int src = (int)__builtin_ctzll(bm);
        const uint32_t bucket = (uint32_t)__builtin_amdgcn_readlane(lane * 4 + bt, src);
        k -= (uint32_t)__builtin_amdgcn_readlane((int)below, src);
        wave_lds_fence();
        prefix |= bucket << shift;
#pragma unroll
        for (int q = 0; q < CPL; q++) act[q] = act[q] && ((d[q] >> shift) & 255u) == bucket;
    }
    return lo + prefix;
}

// wave_select_kth32 for a caller whose selects are bound by instruction issue (k_cts_row's phase 2:
// with two blocks per CU a histogram pass costs what the instructions of its dependent chain cost,
// about as much for 5 active values as for 256). The same result in fewer
// and shorter passes:
//  - 6-bit digits, one bin per lane: the chosen bin is the lane whose [excl, incl) of the wave scan
//    holds rank k, found by one ballot; its count and the values below it are two readlanes, and
//    there is no walk over a lane's bins;
//  - digits aligned to the top of the range (shift = bits - 6 first, the last digit takes what is
//    left), so the first pass spreads the values over all 64 bins whatever the range is;
//  - the select ends as soon as the chosen bin holds one value (the histogram gives its count; the
//    value is read from the one lane that still counts), or at shift 0. The consensus timestamps'
//    offsets span 21 - 23 bits: wave_select_kth32 takes 3 passes on every event, this 2 on 98 % and
//    3 on the rest (profiles/r11_cts_select/select_passes.txt);
//  - a value that has left still adds to its bin, but 0: no EXEC masking around the atomics.
// hist: 64 words owned by this wave. Requires 0 <= K < #valid; every lane returns the result. The
// pass loop is bounded: six digits cover 32 bits.
template <int CPL>
__device__ __forceinline__ uint32_t wave_select_kth32_top(const uint32_t (&v)[CPL], const bool (&ok)[CPL], int K,
                                                          uint32_t* __restrict__ hist) {
    constexpr int DB = 6;   // 1 << DB bins = lanes of a wave
    const int lane = lane_id();
    uint32_t lo = 0xffffffffu, hi = 0;
#pragma unroll
    for (int q = 0; q < CPL; q++)
        if (ok[q]) { lo = min(lo, v[q]); hi = max(hi, v[q]); }
    lo = wave_reduce_min_u32(lo);
    hi = wave_reduce_max_u32(hi);
    if (hi <= lo) return lo;   // (all equal; no valid value: lo = 0xffffffff)
    int top = 32 - __clz((int)(hi - lo));   // bits of v - lo not yet resolved
    uint32_t d[CPL], inc[CPL];
#pragma unroll
    for (int q = 0; q < CPL; q++) { d[q] = v[q] - lo; inc[q] = ok[q] ? 1u : 0u; }
    uint32_t prefix = 0, k = (uint32_t)K;
#pragma unroll 1
    for (int pass = 0; pass < (32 + DB - 1) / DB; pass++) {
        const int shift = top > DB ? top - DB : 0;
        uint32_t dig[CPL];
#pragma unroll
        for (int q = 0; q < CPL; q++) dig[q] = __builtin_amdgcn_ubfe(d[q], (uint32_t)shift, (uint32_t)(top - shift));
        hist[lane] = 0;
        wave_lds_fence();
#pragma unroll
        for (int q = 0; q < CPL; q++) atomicAdd(&hist[dig[q]], inc[q]);
        wave_lds_fence();
        const uint32_t h = hist[lane];
        wave_lds_fence();
        const uint32_t incl = wave_scan_add_u32(h);
        const uint32_t excl = incl - h;
        const uint64_t bm = __builtin_amdgcn_ballot_w64(k >= excl) & __builtin_amdgcn_ballot_w64(k < incl);
        const int bucket = bm ? (int)__builtin_ctzll(bm) : 0;   // (k < #counted: bm has one bit)
        k -= (uint32_t)__builtin_amdgcn_readlane((int)excl, bucket);
        const uint32_t cnt = (uint32_t)__builtin_amdgcn_readlane((int)h, bucket);
        prefix |= (uint32_t)bucket << shift;
        if (shift == 0) break;
#pragma unroll
        for (int q = 0; q < CPL; q++) inc[q] = dig[q] == (uint32_t)bucket ? inc[q] : 0u;
        if (cnt == 1u) {   // the value alone in its bin
            uint32_t r = lo + prefix;
#pragma unroll
            for (int q = 0; q < CPL; q++) {
                const uint64_t b = __builtin_amdgcn_ballot_w64(inc[q] != 0u);
                if (b) r = (uint32_t)__builtin_amdgcn_readlane((int)v[q], (int)__builtin_ctzll(b));
            }
            return r;
        }
        top = shift;
    }
    return lo + prefix;
}

// Reductions and the inclusive scan over groups of 8 consecutive lanes, on DPP: quad_perm [1,0,3,2],
// quad_perm [2,3,0,1], row_half_mirror (lane i <-> 7 - i of its half row). Every lane of a group gets
// the group's result. All 64 lanes must be active.
template <int CTRL, int BANK = 0xf>
__device__ __forceinline__ uint32_t dpp_mov0(uint32_t x) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xf, BANK, false);
}
#define HGX_DPP_GROUP8(x, OP)                    \
    do {                                         \
        x = OP(x, dpp_mov0<0xB1>(x));            \
        x = OP(x, dpp_mov0<0x4E>(x));            \
        x = OP(x, dpp_mov0<0x141>(x));           \
    } while (0)
#define HGX_OP_OR(a, b) ((a) | (b))
__device__ __forceinline__ uint32_t group8_add_u32(uint32_t x) { HGX_DPP_GROUP8(x, HGX_OP_ADD); return x; }
__device__ __forceinline__ uint32_t group8_or_u32(uint32_t x) { HGX_DPP_GROUP8(x, HGX_OP_OR); return x; }
__device__ __forceinline__ uint32_t group8_min_u32(uint32_t x) { HGX_DPP_GROUP8(x, HGX_OP_MIN); return x; }
__device__ __forceinline__ uint32_t group8_max_u32(uint32_t x) { HGX_DPP_GROUP8(x, HGX_OP_MAX); return x; }
// l = lane & 7. row_shr 1 and 2 cross the groups of a row of 16 (masked by l), row_shr 4 is enabled in the
// upper quad of each group only (bank mask 0xA); a lane without a source reads 0.
__device__ __forceinline__ uint32_t group8_scan_add_u32(uint32_t x, int l) {
    const uint32_t y1 = dpp_mov0<0x111>(x);   // (read by every lane: a DPP source must be an active lane)
    x += l >= 1 ? y1 : 0u;
    const uint32_t y2 = dpp_mov0<0x112>(x);
    x += l >= 2 ? y2 : 0u;
    x += dpp_mov0<0x114, 0xA>(x);
    return x;
}


// wave_select_kth32_top for eight events side by side: 8 consecutive lanes per event (l = lane & 7),
// VPL values per lane, one instruction serves eight selects. Same arithmetic per event (values rebased
// to the event's minimum, 6-bit digits from the top of the event's range, exit on a bin of one or at
// shift 0, at most six passes), with the event's minimum, top, shift, rank and prefix in VGPRs.
struct Group8Sel {
    uint32_t lo, res, prefix, k;   // minimum, result so far, digits chosen, rank among what still counts
    int top;                       // bits of v - lo not yet resolved
    bool live;                     // still selecting (the same in the 8 lanes of an event)
};

// One histogram pass over d[q] = v - lo; bit q of act: the value still counts (act = 0: the lanes run
// along and add 0, there is no EXEC masking around the atomics). Returns the count of the chosen bin and
// leaves in act the values inside it.
//  - hcol: the event's 64 bins, hcol[b * LD], LDS words that only this event's lanes touch. Lane l owns
//    bins l + 8t, t = 0..7: with LD = 65 and the events of a wave 8 columns apart, the 64 lanes of a
//    clear or a read hit 64 banks (bins 8l..8l+7 would put 8 lanes on each bank). The chosen bin is found
//    by walking the 8 row totals (three DPP steps each), then by a scan over the 8 lanes of that row;
//    the owner hands bin, rank below and count to its group in one packed word.
//  - the winner of a bin of one is the minimum over the values that still count.
template <int NV, int LD>
__device__ __forceinline__ uint32_t group8_select_pass(const uint32_t (&d)[NV], uint32_t& act, Group8Sel& s,
                                                       uint32_t* hcol, int l) {
    constexpr int DB = 6;
    const int shift = s.top > DB ? s.top - DB : 0;
    const uint32_t width = (uint32_t)(s.top - shift);   // <= DB: every digit is a bin of hcol
    // bin b of the event, as a byte offset from hcol: one v_mad_u32_u24
    auto bin = [&](uint32_t b) -> uint32_t* { return (uint32_t*)((char*)hcol + __umul24(b, (uint32_t)(LD * 4))); };
#pragma unroll
    for (int t = 0; t < 8; t++) hcol[(l + 8 * t) * LD] = 0;
    wave_lds_fence();
#pragma unroll
    for (int q = 0; q < NV; q++) atomicAdd(bin(__builtin_amdgcn_ubfe(d[q], (uint32_t)shift, width)), (act >> q) & 1u);
    wave_lds_fence();
    uint32_t h[8];
#pragma unroll
    for (int t = 0; t < 8; t++) h[t] = hcol[(l + 8 * t) * LD];
    wave_lds_fence();
    // the row of 8 bins that holds rank k: the last whose exclusive prefix is <= k
    uint32_t acc = 0, below = 0, hsel = 0, tsel = 0;
#pragma unroll
    for (int t = 0; t < 8; t++) {
        const bool c = s.k >= acc;
        below = c ? acc : below;
        hsel = c ? h[t] : hsel;
        tsel = c ? (uint32_t)t : tsel;
        acc += group8_add_u32(h[t]);
    }
    const uint32_t k1 = s.k - below;
    const uint32_t incl = group8_scan_add_u32(hsel, l), excl = incl - hsel;
    const bool own = k1 >= excl && k1 < incl;   // one lane of a selecting event
    const uint32_t pk = group8_or_u32(own ? (tsel * 8 + (uint32_t)l) | excl << 6 | hsel << 16 : 0u);
    const uint32_t bucket = pk & 63u, cnt = pk >> 16;
    s.k = k1 - ((pk >> 6) & 1023u);
    s.prefix |= bucket << shift;
    const bool last = shift == 0, one = cnt == 1u;
    if (__builtin_amdgcn_ballot_w64(s.live && !last)) {
        uint32_t keep = 0;
#pragma unroll
        for (int q = 0; q < NV; q++) keep |= __builtin_amdgcn_ubfe(d[q], (uint32_t)shift, width) == bucket ? 1u << q : 0u;
        act &= keep;
    }
    if (__builtin_amdgcn_ballot_w64(s.live && !last && one)) {   // the value alone in its bin
        uint32_t w = 0xffffffffu;
#pragma unroll
        for (int q = 0; q < NV; q++) w = min(w, d[q] | ~(uint32_t)__builtin_amdgcn_sbfe((int)act, q, 1));
        w = group8_min_u32(w);
        s.res = s.live && !last && one ? s.lo + w : s.res;
    }
    s.res = s.live && last ? s.lo + s.prefix : s.res;
    s.live = s.live && !last && !one;
    act = s.live ? act : 0u;
    s.top = shift;
    return cnt;
}

// The select of eight events. v[q], bit q of `member`: the lane's values and which of them count.
// member = 0 in all 8 lanes: the event takes no part (its lanes run along and return 0xffffffff).
// Requires #members >= 1 otherwise; the rank is #members / 2. v is overwritten. hcol: see above. list: CAP
// = 32 words of LDS per event, the event's lanes only (any values of the event's own may be left in it).
// With two blocks per CU a pass costs what its LDS atomics cost, about as much for a lane that adds 0 as
// for one that adds 1. After the first pass few values are left (17 of 256 at the
// median of a gossip trace), so when every event of the wave that still selects has at most CAP of them,
// they are written to `list` in lane order, each lane takes CAP / 8 back, and the later passes issue CAP /
// 8 atomics instead of VPL. Otherwise (two-valued offsets, say) all passes run over the VPL values. The pass
// loops end when a ballot shows no event of the wave still selecting. Every lane of an event returns its
// result.
template <int VPL, int LD>
__device__ __forceinline__ uint32_t group8_select_kth32_top(uint32_t (&v)[VPL], uint32_t member, uint32_t* hcol,
                                                            uint32_t* list, int l) {
    constexpr int DB = 6, PASSES = (32 + DB - 1) / DB, CAP = 32, LV = CAP / 8;
    uint32_t lo = 0xffffffffu, hi = 0;
#pragma unroll
    for (int q = 0; q < VPL; q++) {
        const uint32_t in = (uint32_t)__builtin_amdgcn_sbfe((int)member, q, 1);   // all ones: counts
        lo = min(lo, v[q] | ~in);
        hi = max(hi, v[q] & in);
    }
    lo = group8_min_u32(lo);
    hi = group8_max_u32(hi);
    const uint32_t m = group8_add_u32((uint32_t)__popc(member));
    Group8Sel s;
    s.lo = lo;
    s.res = lo;            // (all equal, or no member)
    s.prefix = 0;
    s.k = m >> 1;
    s.live = hi > lo;
    s.top = s.live ? 32 - __clz((int)(hi - lo)) : 0;
#pragma unroll
    for (int q = 0; q < VPL; q++) v[q] -= lo;
    uint32_t act = s.live ? member : 0u;
    if (!__builtin_amdgcn_ballot_w64(s.live)) return s.res;
    const uint32_t cnt = group8_select_pass<VPL, LD>(v, act, s, hcol, l);
    if (!__builtin_amdgcn_ballot_w64(s.live)) return s.res;
    if (VPL > LV && !__builtin_amdgcn_ballot_w64(s.live && cnt > (uint32_t)CAP)) {
        const uint32_t mine = (uint32_t)__popc(act);
        uint32_t pos = group8_scan_add_u32(mine, l) - mine;
        // VPL stores under EXEC, once, for VPL - LV fewer atomics in every later pass: a store is not the
        // 20 cycles of an atomic, and at c3 FindOrder went 7.3 -> 6.85 ms with the list (sweep.txt job 3)
#pragma unroll
        for (int q = 0; q < VPL; q++)
            if ((act >> q) & 1u) list[pos++ & (CAP - 1)] = v[q];   // (pos < cnt <= CAP)
        wave_lds_fence();
        uint32_t w[LV], wact = 0;
#pragma unroll
        for (int j = 0; j < LV; j++) {
            w[j] = list[l + 8 * j];
            wact |= (uint32_t)(l + 8 * j) < cnt ? 1u << j : 0u;
        }
        wact = s.live ? wact : 0u;
        wave_lds_fence();
#pragma unroll 1
        for (int pass = 1; pass < PASSES; pass++) {
            group8_select_pass<LV, LD>(w, wact, s, hcol, l);
            if (!__builtin_amdgcn_ballot_w64(s.live)) break;
        }
    } else {
#pragma unroll 1
        for (int pass = 1; pass < PASSES; pass++) {
            group8_select_pass<VPL, LD>(v, act, s, hcol, l);
            if (!__builtin_amdgcn_ballot_w64(s.live)) break;
        }
    }
    return s.res;
}

// The same k-th smallest by bisection on the value: each step counts the valid values <= mid with
// CPL compares whose ballots are popcounted in SGPRs (no LDS, no atomics). For rows whose values
// crowd into a few buckets (the witnesses' lastAncestors of one chain in k_threshold span a few
// dozen indices), the radix select's LDS atomics hit the same bins from most lanes and serialise;
// here a step costs CPL VALU compares and a handful of scalar ops, log2(range) steps.
template <int CPL>
__device__ uint32_t wave_select_kth32_bisect(const uint32_t (&v)[CPL], const bool (&ok)[CPL], int K) {
    uint32_t lo = 0xffffffffu, hi = 0;
#pragma unroll
    for (int q = 0; q < CPL; q++)
        if (ok[q]) { lo = min(lo, v[q]); hi = max(hi, v[q]); }
    lo = wave_reduce_min_u32(lo);
    hi = wave_reduce_max_u32(hi);
    uint32_t a = 0, b = hi - lo;   // answer in [a, b]: the smallest t with #(v - lo <= t) > K
    uint32_t d[CPL];
#pragma unroll
    for (int q = 0; q < CPL; q++) d[q] = ok[q] ? v[q] - lo : 0xffffffffu;   // (invalid: above every t < 2^32 - 1)
    while (a < b) {
        const uint32_t mid = a + ((b - a) >> 1);
        int cnt = 0;
#pragma unroll
        for (int q = 0; q < CPL; q++) cnt += __popcll(__ballot(d[q] <= mid));
        if (cnt > K) b = mid;
        else a = mid + 1;
    }
    return lo + a;
}

}  // namespace hgx
