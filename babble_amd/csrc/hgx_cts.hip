// Consensus timestamps, software-pipelined (DecideRoundReceived's median, hashgraph.go:780-787,
// MedianTimestamp :860-868, OldestSelfAncestorToSee :141-167). DESIGN.md §3.5.
//
// Same math as k_cts_tile (hgx_kernels.hip): for a newly received event x at position p of
// chain tc, round received i = rr(x), and every witness chain c of its graph, c contributes
// ts(c, FD[x][c]) when the round-i witness of c is famous and sees x (WLAT[i][tc][c] >= j);
// the consensus timestamp is element floor(m/2) of the m contributions (upper median).
//
// What changes is the schedule. k_cts_tile handles one tile of 8 positions per block and walks
// three dependent global levels per tile (the tile's rr/ts -> the famous flag, WLAT and FD
// of every witness chain -> the FD event's timestamp) with only one tile's loads in flight.
// Here a block is resident (grid = what fits the device) and loops over its tiles with the
// three levels of three consecutive tiles in flight at once, behind the selects of a fourth:
//    gathers of tile k+1 | WLAT/FD loads of tile k+2 | rr/ts of tile k+3 | selects of tile k
// so one tile costs about one global latency or one tile's selects, whichever is longer.
// The per-chain terms that k_cts_tile loaded per lane (c_off - c_base of every chain, the
// tile geometry fu / rcnt / c_off of the launched chains) are read once per block into LDS.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>

#include "hgx_device.h"
#include "hgx_kernels.h"

namespace hgx {

constexpr int kCpT = 8;        // positions per tile (one chain, consecutive)
constexpr int kCpRing = 4;     // tile-info ring slots (a slot is rewritten 4 tiles later)
constexpr int kCpMaxC = 4096;  // chains whose per-chain terms fit the LDS tables
constexpr int64_t kCtsRedo = (int64_t)0x8000000000000000ull;   // p_cts marker: select again in 64 bits

struct CtsTileInfo {
    int32_t row[kCpT];   // round received of the event, -1 = no event at this position
    int64_t ts[kCpT];    // the event's own timestamp (base of the 32-bit offsets)
    int32_t tc, p0;      // chain (global id) and first position of the tile
};

__device__ __forceinline__ void cp_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
__device__ __forceinline__ void cp_order() { asm volatile("" ::: "memory"); }

template <int NPAD, typename CT>
__global__ void __launch_bounds__(256) k_cts_pipe(const int32_t* __restrict__ fu, const int32_t* __restrict__ rcnt,
                                                  const int32_t* __restrict__ p_rr, const int32_t* __restrict__ c_off,
                                                  const int32_t* __restrict__ c_base, const int32_t* __restrict__ WLAT, const CT* __restrict__ FDT,
                                                  const int64_t* __restrict__ p_ts, int64_t* __restrict__ p_cts, int C,
                                                  int n, int64_t Pcap, int c_lo, int c_cnt, int ntt) {
    constexpr int T = kCpT, LD = T + 1, NG = 256 / T, U = NPAD / NG, CPL = NPAD / 64;
    extern __shared__ __attribute__((aligned(16))) uint8_t dyn[];
    // dynamic LDS: kd[C] | tp0[c_cnt] | trc[c_cnt] | vals[2][NPAD * LD] | memb[2][NPAD * LD]
    int32_t* kd = (int32_t*)dyn;
    int32_t* tp0 = kd + C;
    int32_t* trc = tp0 + c_cnt;
    uint32_t* vals = (uint32_t*)(dyn + ((4 * (C + 2 * c_cnt) + 15) & ~15));   // (offsets from dyn keep LDS addressing)
    uint8_t* memb = (uint8_t*)(vals + 2 * NPAD * LD);
    __shared__ CtsTileInfo ring[kCpRing];
    __shared__ __attribute__((aligned(16))) uint32_t whist[4][256];

    const int t = threadIdx.x;
    for (int c = t; c < C; c += 256) kd[c] = c_off[c] - c_base[c];
    for (int c = t; c < c_cnt; c += 256) {
        tp0[c] = c_off[c_lo + c] + fu[c_lo + c];
        trc[c] = rcnt[c_lo + c];
    }
    __syncthreads();
    const int total = c_cnt * ntt;
    const int gstep = (int)gridDim.x;
    // the block's tiles: u = blockIdx.x + k * gridDim.x, time-major (u = tt * c_cnt + chain), so
    // the blocks in flight cover every chain at about the same time (their timestamp gathers
    // share L2 lines); empty tiles (past a chain's received events) are skipped
    auto next_tile = [&](int u) -> int {
        for (; u < total; u += gstep) {
            const int ci = u % c_cnt, tt = u / c_cnt;
            if (tt * T < trc[ci]) break;
        }
        return __builtin_amdgcn_readfirstlane(min(u, total));
    };
    // Every global load below is issued unconditionally (a missing event or tile reads a valid
    // dummy address and is masked afterwards): loads under a branch make the compiler's
    // vmcnt accounting at the join conservative, and it would then wait for the gathers of the
    // tile before the loads of the next tiles are even issued.
    // level 1 of tile u: rr and own timestamp of its positions (lane t: position t % T); a tile
    // u >= total gets a dummy entry (no events) so that its level 2 reads valid addresses
    const int e = t & (T - 1), cg = t / T;
    int32_t l1_rr = -1;
    int64_t l1_ts = 0;
    bool l1_in = false;
    auto l1_issue = [&](int u) {
        const bool vu = u < total;
        const int ci = vu ? u % c_cnt : 0, tt = vu ? u / c_cnt : 0;
        l1_in = vu && tt * T + e < trc[ci];
        const int p = l1_in ? tp0[ci] + tt * T + e : 0;
        l1_rr = p_rr[p];
        l1_ts = p_ts[p];
    };
    auto l1_store = [&](int u, int slot) {
        const bool vu = u < total;
        const int ci = vu ? u % c_cnt : 0, tt = vu ? u / c_cnt : 0;
        int32_t rr_v = l1_in ? l1_rr : -1;
        int64_t ts_v = l1_ts;
        asm volatile("" : "+v"(rr_v), "+v"(ts_v));   // the loads are consumed here, outside the branch
        if (t < T) {
            ring[slot].row[t] = rr_v;
            ring[slot].ts[t] = ts_v;
            if (t == 0) {
                ring[slot].tc = c_lo + ci;
                ring[slot].p0 = tp0[ci] + tt * T;
            }
        }
    };
    // level 2 of the tile in `slot`: lane (e, cg) loads WLAT (famous flag folded in) and FD of
    // chains cg + NG*u; idx = position of the FD event's timestamp, -1 = not a member
    int32_t l2_w[U];
    CT l2_fd[U];
    auto l2_issue = [&](int slot) {
        const int i = ring[slot].row[e];
        const int tc = ring[slot].tc, g = tc / n;
        const int p = ring[slot].p0 + e;
        const size_t fb = (size_t)max(i, 0) * C + (size_t)g * n;
        const size_t wrow = (fb + (tc - g * n)) * n;
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int c = cg + NG * u;
            const bool in = i >= 0 && c < n;
            const int cc = in ? c : 0;
            l2_w[u] = WLAT[wrow + cc];
            l2_fd[u] = FDT[(size_t)cc * Pcap + (in ? p : 0)];
        }
    };
    int32_t idx[U];
    auto l2_finish = [&](int slot) {
        const int i = ring[slot].row[e];
        const int tc = ring[slot].tc, g = tc / n;
        const int j = ring[slot].p0 + e - kd[tc];   // Index of the event
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int c = cg + NG * u;
            const bool in = i >= 0 && c < n;
            const int cc = in ? c : 0;
            const int32_t k = kd[g * n + cc] + Coord<CT>::fd(l2_fd[u]);
            idx[u] = (in & (l2_w[u] >= j)) ? k : -1;
        }
    };

    // prologue: tiles 0 and 1's level 1, tile 0's level 2, then tile 0's gathers, tile 1's level
    // 2 and tile 2's level 1 go out
    int u0 = next_tile(blockIdx.x);
    if (u0 >= total) return;
    int u1 = next_tile(u0 + gstep);
    int u2 = next_tile(u1 + gstep);
    l1_issue(u0);
    l1_store(u0, 0);
    l1_issue(u1);
    l1_store(u1, 1);
    __syncthreads();
    l2_issue(0);
    l2_finish(0);
    const int lane = lane_id(), wave = t >> 6;
    int64_t x[U];
#pragma unroll
    for (int u = 0; u < U; u++) x[u] = p_ts[max(idx[u], 0)];
    cp_order();
    l2_issue(1);
    cp_order();
    l1_issue(u2);
    cp_order();

    // iteration k: (A) tile k's gathers land -> offsets and membership into LDS buffer k & 1;
    // (B) tile k+1's gather indices, tile k+2's level 1 into the ring; barrier; (C) tile k+1's
    // gathers, tile k+2's level 2 and tile k+3's level 1 go out; (D) tile k's selects run while
    // they are in flight
    for (int k = 0; u0 < total; k++) {
        const int s0 = k & (kCpRing - 1), s1 = (k + 1) & (kCpRing - 1), s2 = (k + 2) & (kCpRing - 1);
        {   // (A)
            uint32_t* v = vals + (k & 1) * NPAD * LD;
            uint8_t* mb = memb + (k & 1) * NPAD * LD;
            const int64_t base = ring[s0].ts[e];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int c = cg + NG * u;
                const bool ok = idx[u] >= 0;
                const int64_t dlt = x[u] - base;
                const bool ov = ok && (dlt < INT32_MIN || dlt > INT32_MAX);
                v[c * LD + e] = (uint32_t)(int32_t)dlt ^ 0x80000000u;   // (c >= n: not a member)
                mb[c * LD + e] = (uint8_t)((ok ? 1 : 0) | (ov ? 2 : 0));
            }
        }
        // (B)
        l2_finish(s1);
        l1_store(u2, s2);
        cp_lds_barrier();
        // (C)
        const int u3 = next_tile(u2 + gstep);
#pragma unroll
        for (int u = 0; u < U; u++) x[u] = p_ts[max(idx[u], 0)];
        cp_order();
        l2_issue(s2);
        cp_order();
        l1_issue(u3);
        cp_order();
        // (D) one wave per event: radix select of element floor(m/2)
        {
            const uint32_t* v = vals + (k & 1) * NPAD * LD;
            const uint8_t* mb = memb + (k & 1) * NPAD * LD;
            for (int ev = wave; ev < T; ev += 4) {
                if (ring[s0].row[ev] < 0) continue;   // wave-uniform
                bool ok[CPL];
                uint32_t vv[CPL];
                int m = 0;
                bool any_ov = false;
#pragma unroll
                for (int q = 0; q < CPL; q++) {
                    const int c = lane + 64 * q;
                    const uint8_t b = mb[c * LD + ev];
                    ok[q] = (b & 1) != 0;
                    vv[q] = v[c * LD + ev];
                    m += __popcll(__ballot(ok[q]));
                    any_ov |= __ballot((b & 2) != 0) != 0;
                }
                // rare: an offset beyond 32 bits -> kCtsRedo, k_cts_redo selects in 64 bits
                int64_t res = kCtsRedo;
                if (!any_ov) {
                    const uint32_t sel = wave_select_kth32<CPL>(vv, ok, m / 2, whist[wave]);
                    res = ring[s0].ts[ev] + (int64_t)(int32_t)(sel ^ 0x80000000u);
                }
                if (lane == 0) p_cts[ring[s0].p0 + ev] = res;
            }
        }
        u0 = u1;
        u1 = u2;
        u2 = u3;
    }
}

// the events k_cts_pipe left at kCtsRedo (a timestamp offset beyond 32 bits): one wave per
// event regathers the contributions and selects in 64 bits. A true median equal to kCtsRedo
// is recomputed to the same value, so the marker needs no separate flag.
template <int NPAD, typename CT>
__global__ void __launch_bounds__(256) k_cts_redo(const int32_t* __restrict__ fu, const int32_t* __restrict__ rcnt,
                                                  const int32_t* __restrict__ p_rr, const int32_t* __restrict__ c_off,
                                                  const int32_t* __restrict__ c_base, const int32_t* __restrict__ WLAT,
                                                  const CT* __restrict__ FDT, const int64_t* __restrict__ p_ts,
                                                  int64_t* __restrict__ p_cts, int C, int n, int64_t Pcap, int c_lo) {
    constexpr int CPL = NPAD / 64;
    __shared__ int32_t list[256];
    __shared__ int32_t cnt;
    __shared__ __attribute__((aligned(16))) uint32_t whist[4][256];
    const int gc = c_lo + blockIdx.y, g = gc / n;
    const int k = (int)blockIdx.x * 256 + threadIdx.x;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    const int64_t p0 = (int64_t)c_off[gc] + fu[gc];
    if (k < rcnt[gc] && p_cts[p0 + k] == kCtsRedo) list[atomicAdd(&cnt, 1)] = k;
    __syncthreads();
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    for (int q0 = wave; q0 < cnt; q0 += 4) {
        const int64_t p = p0 + list[q0];
        const int i = p_rr[p];
        const int j = c_base[gc] + (int)(p - c_off[gc]);
        const size_t row = ((size_t)i * C + gc) * n;
        uint64_t v[CPL];
        bool ok[CPL];
        int m = 0;
#pragma unroll
        for (int q = 0; q < CPL; q++) {
            const int c = lane + 64 * q;
            ok[q] = c < n && WLAT[row + c] >= j;
            int64_t x = 0;
            if (ok[q]) {
                const int ch = g * n + c;
                x = p_ts[c_off[ch] - c_base[ch] + Coord<CT>::fd(FDT[(size_t)c * Pcap + p])];
            }
            v[q] = (uint64_t)x ^ 0x8000000000000000ull;
            m += __popcll(__ballot(ok[q]));
        }
        const int64_t res = (int64_t)(wave_select_kth<CPL>(v, ok, m / 2, whist[wave]) ^ 0x8000000000000000ull);
        if (lane == 0) p_cts[p] = res;
    }
}

template <int NPAD, typename CT>
static bool cts_pipe_launch(hipStream_t s, const DevArrays& a, int c_lo, int c_cnt, int C, int n, int64_t P,
                            int max_cnt) {
    constexpr int LD = kCpT + 1;
    const size_t lds = (((size_t)4 * C + (size_t)8 * c_cnt + 15) & ~(size_t)15) + (size_t)2 * NPAD * LD * 5;
    const void* f = (const void*)k_cts_pipe<NPAD, CT>;
    static int dev_cus[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
    if (ensure_lds_limit(f, lds) != hipSuccess) return false;
    if (dev_cus[dev] == 0) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
            return false;
        dev_cus[dev] = cus;
    }
    int per_cu = 0;
    if (blocks_per_cu(f, 256, lds, &per_cu) != hipSuccess || per_cu < 1) return false;
    const int ntt = (max_cnt + kCpT - 1) / kCpT;
    const int64_t tiles = (int64_t)c_cnt * ntt;
    if (tiles <= 0) return true;
    if (tiles > 0x7FFFFFFF - (int64_t)dev_cus[dev] * per_cu) return false;
    const unsigned grid = (unsigned)std::min<int64_t>(tiles, (int64_t)dev_cus[dev] * per_cu);
    hipLaunchKernelGGL((k_cts_pipe<NPAD, CT>), dim3(grid), dim3(256), lds, s, a.fu, a.rcnt, a.p_rr, a.c_off, a.c_base,
                       a.WLAT, (const CT*)a.FDT, a.p_ts, a.p_cts, C, n, P, c_lo, c_cnt, ntt);
    hipLaunchKernelGGL((k_cts_redo<NPAD, CT>), dim3((max_cnt + 255) / 256, c_cnt), dim3(256), 0, s, a.fu, a.rcnt, a.p_rr,
                       a.c_off, a.c_base, a.WLAT, (const CT*)a.FDT, a.p_ts, a.p_cts, C, n, P, c_lo);
    return true;
}

template <typename CT>
static bool launch_cts_pipe_t(hipStream_t s, const DevArrays& a, int c_lo, int c_cnt, int C, int n, int64_t P,
                              int max_cnt) {
    if (n <= 64) return cts_pipe_launch<64, CT>(s, a, c_lo, c_cnt, C, n, P, max_cnt);
    if (n <= 128) return cts_pipe_launch<128, CT>(s, a, c_lo, c_cnt, C, n, P, max_cnt);
    if (n <= 256) return cts_pipe_launch<256, CT>(s, a, c_lo, c_cnt, C, n, P, max_cnt);
    return cts_pipe_launch<512, CT>(s, a, c_lo, c_cnt, C, n, P, max_cnt);
}

bool cts_pipe_ok(int n, int C) { return n > 32 && n <= 512 && C <= kCpMaxC; }

bool launch_cts_pipe(hipStream_t s, const DevArrays& a, int c_lo, int c_cnt, int C, int n, int64_t P, int max_cnt) {
    if (max_cnt <= 0 || c_cnt <= 0) return true;
    if (!cts_pipe_ok(n, C)) return false;
    return a.compact ? launch_cts_pipe_t<uint16_t>(s, a, c_lo, c_cnt, C, n, P, max_cnt)
                     : launch_cts_pipe_t<int32_t>(s, a, c_lo, c_cnt, C, n, P, max_cnt);
}

// ---------------------------------------------------------------------------------
// Round 9: lane = event, instruction = witness chain (k_cts_small's mapping for 32 < n <= 256).
// A block owns TP = 64 consecutive positions of one chain. In phase 1 a wave's 64 lanes are the
// tile's events and every wave walks NPAD / NW witness chains: FDT[c][p0 .. p0 + TP) is one
// coalesced load whose lines are used whole (k_cts_tile's instruction touches 8 columns for
// 16 bytes each), and since firstDescendants are monotone along a chain the TP timestamp
// gathers of a chain fall into a few lines. The per-chain terms are wave-uniform (read from a
// lane). The gathered values go to LDS as k_cts_tile's 32-bit offsets, vals[c][e]; phase 2 is the
// radix select of element floor(m/2), eight events per wave: 8 lanes per event, NPAD / 8 values per
// lane (group8_select_kth32_top, hgx_device.h: wave_select_kth32_top's arithmetic per event, 6-bit
// digits from the top of the event's range, exit on a bin of one). Wave w takes the events it took one
// at a time before, e = w + 8s (four waves: two groups, w and w + 4); the bins of an event are its own
// column of vals once the values are in registers, and membership is one word per lane (memw). An event
// whose offsets need 64 bits takes no part and is done afterwards by one wave, as before.
// Round 12 (profiles/r12_cts_group): with two blocks per CU phase 2 costs what its LDS
// atomics cost, a wave instruction about the same whether its lanes add 1, add 0 or are masked off. Kept:
// the group select with an active mask per lane, and the passes after the first over a list of the
// values still left (4 atomics per pass instead of 32). Rejected: marking a value that has left by
// overwriting it, all of them adding to one bin (same-address atomics: slower than one wave per event);
// EXEC masks around the atomics (0.1 ms, not kept). Not measured: 16-bit bins in the waves' 256 words.
// Membership (WLAT[(rr, tc)][c] >= Index) needs the row of the event's round received; rr is
// non-decreasing along a chain and TP positions span a few rounds, so the block stages the K
// rows from its smallest rr in LDS (loads issued beside the gathers) and an event beyond them
// reads its row from global memory.
// Measured at c3: round 9 6.46 ms against k_cts_tile's 7.0, 3.3 ms without the selects;
// round 11 5.25 ms against 6.50 in the same job, 2.85 without the selects; round 12 FindOrder's device time (this
// kernel and 2.5 ms of sorting) 6.85 ms against 7.75 in the same job, the kernel itself 4.35 - 4.41 ms against
// 5.28 - 5.37 warm and 4.84 against 5.41 as a process's first dispatch (SQ_LDS_IDX_ACTIVE 1.13 -> 0.88 G,
// SQ_INSTS_VALU 2.26 -> 2.21 G). The c3 step gained 0.75 - 1.07 ms in five jobs; that was three times the
// parent's range in one of them (profiles/r12_cts_group/README.md).
constexpr int kRowKMax = 8;   // staged WLAT rows at most
constexpr int kRowTP = 64;    // positions per block = lanes of a wave (32 with two chains per instruction: c3 7.13 - 7.24 ms, removed)
constexpr int kRowD = 16;     // chain instructions in flight per wave (4: 6.55, 8: 6.63 - 6.66, 32: 6.57 ms)
// waves per block: vals lets two blocks share a CU whatever their size, and the selects of phase 2
// need waves to hide behind (c3: 4 waves 10.3 - 10.5 ms, 8: 6.9, 16: 9.0, before the per-chain
// terms moved from scalar loads to a lane: 8 waves 6.9 -> 6.46)
constexpr int row_waves(int npad) { return npad >= 128 ? 8 : 4; }

template <int NPAD, typename CT, int TP, int DREQ, int NW>
__global__ void __launch_bounds__(64 * NW) k_cts_row(const int32_t* __restrict__ fu, const int32_t* __restrict__ rcnt,
                                                 const int32_t* __restrict__ p_rr, const int32_t* __restrict__ c_off,
                                                 const int32_t* __restrict__ c_base, const int32_t* __restrict__ WLAT,
                                                 const CT* __restrict__ FDT, const int64_t* __restrict__ p_ts,
                                                 int64_t* __restrict__ p_cts, int C, int n, int64_t Pcap, int c_lo,
                                                 int c_cnt, int R, int K) {
    static_assert(TP == 64, "k_cts_row: a wave's lanes are the block's events");
    constexpr int LD = TP + 1;            // row stride of vals: conflict-free for both phases
    constexpr int CPL = NPAD / 64;
    constexpr int CW = NPAD / NW;         // chains per wave
    constexpr int NI = CW;                // chain instructions per wave: instruction k takes chain wc0 + k
    constexpr int D = DREQ < NI ? DREQ : NI;
    constexpr int NB = NI / D;
    constexpr int VPL = NPAD / 8;         // phase 2: values per lane, 8 lanes per event
    static_assert(NI % D == 0 && NI % 8 == 0 && NI <= 32 && 8 % NW == 0, "k_cts_row: batches, membership words, groups");
    constexpr int RG = 64 * NW / NPAD;    // staged rows loaded at once (thread t: word t % NPAD of row t / NPAD)
    constexpr int KL = kRowKMax / RG;     // staging loads per thread
    static_assert(RG >= 1 && kRowKMax % RG == 0, "k_cts_row: staging loads");
    // [NPAD][LD] offsets + 2^31 | wl[K][n + 1], reused by phase 2 as the waves' histograms [NW][256]
    extern __shared__ __attribute__((aligned(16))) uint32_t vals[];
    int32_t* wl = (int32_t*)(vals + NPAD * LD);
    // memw[l * LD + e]: bit q = chain l + 8q is a member of event e (phase 2's lane (e, l) holds those
    // chains; with the stride LD the 64 lanes of either phase hit 64 banks)
    __shared__ uint32_t memw[8 * LD];
    __shared__ int32_t e_row[TP];
    __shared__ int64_t e_ts[TP];
    __shared__ int32_t e_ovf[TP];
    __shared__ uint32_t s_min[NW];
    // time-major blocks (b = tile * c_cnt + chain): the blocks in flight gather timestamps of the
    // same period on every chain and share those lines in L2. Tiles are cut at multiples of TP
    // from the 32-position boundary below the chain's first new event (chain slots and the
    // column stride are multiples of 32 positions, so an FD load starts 64-byte aligned); a
    // chain's first tile may be short.
    const int cl = (int)(blockIdx.x % (unsigned)c_cnt), tt = (int)(blockIdx.x / (unsigned)c_cnt);
    const int tc = c_lo + cl;
    const int f0 = fu[tc], co = c_off[tc];
    const int64_t q0 = (int64_t)co + f0, pend = q0 + rcnt[tc];
    const int64_t ps = (int64_t)co + (f0 & ~31) + (int64_t)tt * TP;
    // (block-uniform) no event in this tile. A chain that receives nothing has ps <= q0 = pend when its
    // fu is off a 32-position boundary: q0 may then be past the chain's last event, where
    // firstDescendants are not defined, so nothing may be loaded from it.
    if ((ps > q0 ? ps : q0) >= pend) return;
    const int lane = lane_id(), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int e = lane;
    const int64_t p = ps + e;
    const bool ev = p >= q0 && p < pend;
    const int64_t pl = ev ? p : (ps > q0 ? ps : q0);   // a valid position for the loads of a missing event
    const int i = p_rr[pl];
    const int64_t base = p_ts[pl];
    const int g = tc / n, gb = g * n;
    const int j = c_base[tc] + (int)(pl - co);
    const bool evi = ev && i >= 0;
    const int wc0 = wave * CW;
    uint32_t* whist = vals + NPAD * LD + 256 * wave;
    // chain of instruction k in this lane, clamped to a chain of the graph (a chain >= n loads
    // valid addresses and is never a member)
    auto chain = [&](int k) { const int c = wc0 + k; return c < n ? c : 0; };
    auto load_fd = [&](int b, CT (&fd)[D]) {
#pragma unroll
        for (int u = 0; u < D; u++) fd[u] = FDT[(size_t)chain(b * D + u) * Pcap + pl];
    };
    CT fd[2][D];
    load_fd(0, fd[0]);
    // c_off - c_base of the wave's chains, one per lane: an instruction's term is read from its
    // lane into an SGPR (a scalar load per chain put its latency in front of every gather)
    const int kc = wc0 + lane < n && lane < CW ? wc0 + lane : 0;
    const int32_t kdv = c_off[gb + kc] - c_base[gb + kc];
    // the block's smallest round received (level 1 only: the FD loads above stay in flight)
    const uint32_t wmin = wave_reduce_min_u32(evi ? (uint32_t)i : 0x7fffffffu);
    if (lane == 0) s_min[wave] = wmin;
    if (threadIdx.x < TP) {
        e_row[e] = evi ? i : -1;
        e_ts[e] = base;
        e_ovf[e] = 0;
    }
    for (int w = (int)threadIdx.x; w < 8 * LD; w += 64 * NW) memw[w] = 0;
    cp_lds_barrier();
    uint32_t bmin = s_min[0];
#pragma unroll
    for (int w = 1; w < NW; w++) bmin = min(bmin, s_min[w]);
    const int imin = bmin == 0x7fffffffu ? 0 : (int)bmin;
    // rows imin .. imin + K - 1 of (round, tc), clamped to the rounds that exist: level 2, beside
    // the gathers. Every load is issued (a row past K or a word past n repeats a valid one and
    // is dropped).
    int32_t st[KL];
    const int sw = (int)threadIdx.x % NPAD, srow = (int)threadIdx.x / NPAD;
#pragma unroll
    for (int q = 0; q < KL; q++)
        st[q] = WLAT[((size_t)min(imin + min(q * RG + srow, K - 1), R - 1) * C + tc) * n + min(sw, n - 1)];
    // The chains' pipeline, in program order (the memory counter retires in order, so a wait
    // for a batch leaves the batches issued after it in flight):
    //    F0 F1 G0 | F2 G1 use0 | F3 G2 use1 | ...
    // F = a batch's D FD loads, G = its timestamp gathers, use = offsets to LDS. The compiler
    // barriers keep that order: without them the address arithmetic of a later batch's FD values
    // was scheduled right behind each load and every load waited for on its own.
    int64_t x[2][D];
    auto gather = [&](int b, const CT (&f)[D], int64_t (&xo)[D]) {
#pragma unroll
        for (int u = 0; u < D; u++) {
            const int k = b * D + u;
            const int32_t kd = __builtin_amdgcn_readlane(kdv, k);   // the instruction's chain: wave-uniform
            const int32_t fv = Coord<CT>::fd(f[u]);
            xo[u] = p_ts[fv != kMaxI32 ? kd + fv : 0];
        }
    };
    uint64_t ovm = 0;   // bit k: the offset of instruction k's chain does not fit 32 bits
    if (NB > 1) load_fd(1, fd[1]);
    cp_order();
    gather(0, fd[0], x[0]);
    cp_order();
#pragma unroll
    for (int b = 0; b < NB; b++) {
        if (b + 2 < NB) load_fd(b + 2, fd[b & 1]);
        cp_order();
        if (b + 1 < NB) gather(b + 1, fd[(b + 1) & 1], x[(b + 1) & 1]);
        cp_order();
#pragma unroll
        for (int u = 0; u < D; u++) {
            const int k = b * D + u;
            const int64_t dlt = x[b & 1][u] - base;
            ovm |= (uint64_t)(dlt < INT32_MIN || dlt > INT32_MAX) << k;
            vals[(wc0 + k) * LD + e] = (uint32_t)(int32_t)dlt ^ 0x80000000u;
        }
        cp_order();
    }
    const int WS = n + 1;   // row stride of the staged rows (lanes of different rounds: different banks)
#pragma unroll
    for (int q = 0; q < KL; q++)
        if (q * RG + srow < K && sw < n) wl[(q * RG + srow) * WS + sw] = st[q];
    __syncthreads();
    {
        uint64_t okm = 0;   // bit k: the chain of instruction k is a member
        if (!evi || i - imin < K) {
            const int32_t* row = wl + (evi ? i - imin : 0) * WS;
#pragma unroll
            for (int k = 0; k < NI; k++) okm |= (uint64_t)(row[chain(k)] >= j) << k;
        } else {   // a tile spanning more than K rounds
            const int32_t* __restrict__ row = WLAT + ((size_t)i * C + tc) * n;
#pragma unroll
            for (int k = 0; k < NI; k++) okm |= (uint64_t)(row[chain(k)] >= j) << k;
        }
        // (chains >= n: the last chains of the last wave in use, k >= n - wc0)
        const int live = n - wc0;
        if (live < NI) okm &= live > 0 ? ((uint64_t)1 << live) - 1 : 0;
        if (!evi) okm = 0;
        // the wave's chains wc0 + l + 8j are bits wc0 / 8 + j of word l: bits l, l + 8, l + 16, l + 24 of okm,
        // gathered by a multiply (the partial products land on distinct bits, none carries into 28..31)
        const uint32_t ok32 = (uint32_t)okm;
#pragma unroll
        for (int l = 0; l < 8; l++)
            atomicOr(&memw[l * LD + e], ((((ok32 >> l) & 0x01010101u) * 0x10204080u) >> 28) << (wc0 / 8));
        if (ovm & okm) e_ovf[e] = 1;
    }
    __syncthreads();
    // phase 2: eight events per wave, 8 lanes each. Lane (gs, gl) of group vw = wave + NW * grp belongs to
    // event vw + 8 * gs and holds chains gl + 8q: a load of vals[c][e] hits 64 banks. The bins of an event
    // are its own column of vals (rows 0..63), which no other lane reads once the values are in registers.
    const int gs = lane >> 3, gl = lane & 7;
    for (int grp = 0; grp < 8 / NW; grp++) {
        const int vw = wave + NW * grp, e2 = vw + 8 * gs;
        const bool has = e_row[e2] >= 0, wide = e_ovf[e2] != 0;
        if (!__builtin_amdgcn_ballot_w64(has)) continue;   // no event in the group
        const bool part = has && !wide;   // absent and 64-bit events take no part: no member
        if (__builtin_amdgcn_ballot_w64(part)) {
            uint32_t* hcol = vals + e2;
            const uint32_t member = part ? memw[gl * LD + e2] : 0u;
            uint32_t v[VPL];
#pragma unroll
            for (int q = 0; q < VPL; q++) v[q] = hcol[(gl + 8 * q) * LD];
            const uint32_t u = group8_select_kth32_top<VPL, LD>(v, member, hcol, whist + 32 * gs, gl);
            if (part && gl == 0) p_cts[ps + e2] = e_ts[e2] + (int64_t)(int32_t)(u ^ 0x80000000u);
        }
        // rare: offsets beyond 32 bits -> one wave per event, regather and select in 64 bits
        for (uint64_t todo = __builtin_amdgcn_ballot_w64(has && wide) & 0x0101010101010101ull; todo; todo &= todo - 1) {
            const int e3 = vw + (int)__builtin_ctzll(todo);   // (bit 8 * gs: event vw + 8 * gs)
            const uint32_t mw = memw[gl * LD + e3];
            bool ok[CPL];
            uint64_t v[CPL];
            int m = 0;
#pragma unroll
            for (int q = 0; q < CPL; q++) {
                const int c = lane + 64 * q;   // = gl + 8 * (gs + 8q)
                ok[q] = (mw >> (gs + 8 * q)) & 1u;
                m += __popcll(__builtin_amdgcn_ballot_w64(ok[q]));
                int64_t x = 0;
                if (ok[q]) x = p_ts[c_off[gb + c] - c_base[gb + c] + Coord<CT>::fd(FDT[(size_t)c * Pcap + ps + e3])];
                v[q] = (uint64_t)x ^ 0x8000000000000000ull;
            }
            const int64_t res = (int64_t)(wave_select_kth<CPL>(v, ok, m / 2, whist) ^ 0x8000000000000000ull);
            if (lane == 0) p_cts[ps + e3] = res;
        }
    }
}

template <int NPAD, typename CT>
static bool cts_row_launch(hipStream_t s, const DevArrays& a, int c_lo, int c_cnt, int C, int n, int64_t P,
                           int max_cnt, int R, int k_rows) {
    constexpr int TP = kRowTP, NW = row_waves(NPAD);
    // two blocks per CU at NPAD = 256: the block's static LDS, vals and the staged rows within 79 KB
    constexpr size_t kStatic = (size_t)8 * (TP + 1) * 4 + (size_t)TP * 16 + 4 * NW;
    const size_t fixed = (size_t)NPAD * (TP + 1) * 4, row = (size_t)(n + 1) * 4;
    const int room = (int)(((size_t)79 * 1024 - kStatic - fixed) / row);
    const int K = k_rows > 0 ? std::min(k_rows, kRowKMax) : std::max(1, std::min(room, kRowKMax));
    const size_t lds = fixed + std::max((size_t)K * row, (size_t)NW * 1024);   // (the rows' space is the histograms' in phase 2)
    const void* f = (const void*)k_cts_row<NPAD, CT, TP, kRowD, NW>;
    if (ensure_lds_limit(f, lds) != hipSuccess) return false;
    const int64_t blocks = (int64_t)c_cnt * ((max_cnt + 31 + TP - 1) / TP);   // (a first tile starts up to 31 positions early)
    if (blocks > 0x7FFFFFFF) return false;
    hipLaunchKernelGGL((k_cts_row<NPAD, CT, TP, kRowD, NW>), dim3((unsigned)blocks), dim3(64 * NW), lds, s, a.fu, a.rcnt, a.p_rr,
                       a.c_off, a.c_base, a.WLAT, (const CT*)a.FDT, a.p_ts, a.p_cts, C, n, P, c_lo, c_cnt, R, K);
    return true;
}

template <typename CT>
static bool launch_cts_row_t(hipStream_t s, const DevArrays& a, int c_lo, int c_cnt, int C, int n, int64_t P,
                             int max_cnt, int R, int k_rows) {
    if (n <= 64) return cts_row_launch<64, CT>(s, a, c_lo, c_cnt, C, n, P, max_cnt, R, k_rows);
    if (n <= 128) return cts_row_launch<128, CT>(s, a, c_lo, c_cnt, C, n, P, max_cnt, R, k_rows);
    return cts_row_launch<256, CT>(s, a, c_lo, c_cnt, C, n, P, max_cnt, R, k_rows);
}

bool cts_row_ok(int n) { return n > 32 && n <= 256; }
int cts_row_tile() { return kRowTP; }

bool launch_cts_row(hipStream_t s, const DevArrays& a, int c_lo, int c_cnt, int C, int n, int64_t P, int max_cnt,
                    int R, int k_rows) {
    if (max_cnt <= 0 || c_cnt <= 0) return true;
    if (!cts_row_ok(n) || R <= 0) return false;
    return a.compact ? launch_cts_row_t<uint16_t>(s, a, c_lo, c_cnt, C, n, P, max_cnt, R, k_rows)
                     : launch_cts_row_t<int32_t>(s, a, c_lo, c_cnt, C, n, P, max_cnt, R, k_rows);
}

}  // namespace hgx
