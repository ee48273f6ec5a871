// hgx_insert_wire_bodies on the device: ReadWireInfo's parent lookup
// (hashgraph.go:569-614, Store.ParticipantEvent) for a whole SyncResponse.
//
// The host plan (hgx_wire_plan.h) decided every error and every in-batch parent from the per-chain
// tables; what it cannot know without the O(E) host mirror is the gid of a resident (creator, Index).
// k_wire_window finds those: per creator the batch names a window [lo[c], last_index[c]] of Indexes, and
// every resident event inside its creator's window writes its own gid to its slot. A chain holds each
// Index once, so no two events share a slot: no atomic, no workgroup waits for another, the result is
// deterministic. 8 bytes are read per resident event (creator and Index). k_wire_resolve then turns the
// chunk's window descriptors into gids, in the columns the encoder and the verified insert read.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hgx_device.h"
#include "hgx_kernels.h"

namespace hgx {

constexpr int kWireThreads = 256;
constexpr int kWirePer = kWireChunk / kWireThreads;   // 8 consecutive gids per thread
constexpr int kWireMaxN = 1024;                       // participants (lo[] and woff[] in LDS: 8 KB)

__global__ void __launch_bounds__(kWireThreads) k_wire_window(WireWinArgs a) {
    __shared__ int32_t sh_lo[kWireMaxN];
    __shared__ int32_t sh_woff[kWireMaxN];
    for (int i = threadIdx.x; i < a.n; i += kWireThreads) {
        sh_lo[i] = a.tab[i];
        sh_woff[i] = a.tab[a.n + i];
    }
    __syncthreads();
    const int64_t e0 = (int64_t)blockIdx.x * kWireChunk + (int64_t)threadIdx.x * kWirePer;
    if (e0 >= a.E) return;
    int32_t cr[kWirePer], ix[kWirePer];
    if (e0 + kWirePer <= a.E) {   // two 16-byte loads per column for the whole group of 8
        const int4 c0 = *(const int4*)(a.g_creator + e0), c1 = *(const int4*)(a.g_creator + e0 + 4);
        const int4 i0 = *(const int4*)(a.g_index + e0), i1 = *(const int4*)(a.g_index + e0 + 4);
        cr[0] = c0.x; cr[1] = c0.y; cr[2] = c0.z; cr[3] = c0.w; cr[4] = c1.x; cr[5] = c1.y; cr[6] = c1.z; cr[7] = c1.w;
        ix[0] = i0.x; ix[1] = i0.y; ix[2] = i0.z; ix[3] = i0.w; ix[4] = i1.x; ix[5] = i1.y; ix[6] = i1.z; ix[7] = i1.w;
    } else {
#pragma unroll
        for (int k = 0; k < kWirePer; k++) {
            const bool in = e0 + k < a.E;
            cr[k] = in ? a.g_creator[e0 + k] : -1;
            ix[k] = in ? a.g_index[e0 + k] : 0;
        }
    }
#pragma unroll
    for (int k = 0; k < kWirePer; k++) {
        const uint32_t c = (uint32_t)cr[k];
        if (c >= (uint32_t)a.n) continue;
        const int32_t lo = sh_lo[c];
        if (ix[k] < lo) continue;   // (a creator nobody names: lo = INT32_MAX)
        const int64_t slot = (int64_t)sh_woff[c] + ((int64_t)ix[k] - lo);
        if (slot < a.slots) a.win[slot] = (int32_t)(e0 + k);
    }
}

__device__ __forceinline__ int64_t wire_gid(int64_t d, int64_t k, const int32_t* __restrict__ win, int64_t slots,
                                            unsigned long long* fail) {
    if (d >= -1) return d;
    const int64_t slot = -2 - d;
    const int32_t g = slot < slots ? win[slot] : -1;
    if (g >= 0) return g;
    atomicMin(fail, ((unsigned long long)k << 8) | (unsigned long long)INS_WIRE_HOLE);
    return kWireHoleParent;
}

__global__ void __launch_bounds__(256) k_wire_resolve(int64_t m, int64_t* __restrict__ sp, int64_t* __restrict__ op,
                                                      const int32_t* __restrict__ win, int64_t slots,
                                                      unsigned long long* fail) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    const int64_t s = sp[k], o = op[k];
    if (s < -1) sp[k] = wire_gid(s, k, win, slots, fail);
    if (o < -1) op[k] = wire_gid(o, k, win, slots, fail);
}

void launch_wire_window(hipStream_t s, const WireWinArgs& a) {
    if (a.E <= 0 || a.slots <= 0) return;
    const unsigned nb = (unsigned)((a.E + kWireChunk - 1) / kWireChunk);
    hipLaunchKernelGGL(k_wire_window, dim3(nb), dim3(kWireThreads), 0, s, a);
}

void launch_wire_resolve(hipStream_t s, int64_t m, int64_t* sp, int64_t* op, const int32_t* win, int64_t slots,
                         unsigned long long* fail) {
    if (m <= 0) return;
    hipLaunchKernelGGL(k_wire_resolve, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, m, sp, op, win, slots, fail);
}

}  // namespace hgx
