// hgx_diff_wire on the device: Core.Diff and ToWire (node/core.go:166-188,
// hashgraph.go:532-567) as a filter over two columns plus a gather.
//
// The resident events lie in gid order, which is the reference's topological order, so the response is
// the events with Index > known[creator] in ascending gid. Whether an event is selected is a function
// of (g_creator[e], g_index[e]) and the small known[] table: it is recomputed, never stored. Three
// launches: k_diff_count (selected events per 2 048 gids), k_scan_top over those partials
// (hgx_kernels.hip), k_diff_gather (every selected event's row = its workgroup's scanned partial plus
// its rank inside the workgroup). No workgroup waits for another, and there is no atomic: the result
// is deterministic. 16 bytes are read per resident event (creator and Index, twice).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hgx_device.h"
#include "hgx_kernels.h"

namespace hgx {

constexpr int kDiffThreads = 256;
constexpr int kDiffPer = kDiffChunk / kDiffThreads;   // 8 consecutive gids per thread
constexpr int kDiffMaxN = 1024;                       // participants of one graph (known[] in LDS)

// bit k of the result: gid e0 + k is selected. Two 16-byte loads per column for a whole group of 8.
__device__ __forceinline__ uint32_t diff_flags(const DiffArgs& a, int64_t e0, const int32_t* sh_known) {
    int32_t cr[kDiffPer], ix[kDiffPer];
    if (e0 + kDiffPer <= a.E) {
        const int4 c0 = *(const int4*)(a.g_creator + e0), c1 = *(const int4*)(a.g_creator + e0 + 4);
        const int4 i0 = *(const int4*)(a.g_index + e0), i1 = *(const int4*)(a.g_index + e0 + 4);
        cr[0] = c0.x; cr[1] = c0.y; cr[2] = c0.z; cr[3] = c0.w; cr[4] = c1.x; cr[5] = c1.y; cr[6] = c1.z; cr[7] = c1.w;
        ix[0] = i0.x; ix[1] = i0.y; ix[2] = i0.z; ix[3] = i0.w; ix[4] = i1.x; ix[5] = i1.y; ix[6] = i1.z; ix[7] = i1.w;
    } else {
#pragma unroll
        for (int k = 0; k < kDiffPer; k++) {
            const bool in = e0 + k < a.E;
            cr[k] = in ? a.g_creator[e0 + k] : -1;
            ix[k] = in ? a.g_index[e0 + k] : 0;
        }
    }
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < kDiffPer; k++) {
        const uint32_t l = (uint32_t)(cr[k] - a.c0);   // the graph's creator range: [0, n)
        if (l < (uint32_t)a.n && ix[k] > sh_known[l]) m |= 1u << k;
    }
    return m;
}

__global__ void __launch_bounds__(kDiffThreads) k_diff_count(DiffArgs a) {
    __shared__ int32_t sh_known[kDiffMaxN];
    __shared__ uint32_t sh[4];
    for (int i = threadIdx.x; i < a.n; i += kDiffThreads) sh_known[i] = a.tab[i];
    __syncthreads();
    const int64_t e0 = (int64_t)blockIdx.x * kDiffChunk + (int64_t)threadIdx.x * kDiffPer;
    uint32_t s = e0 < a.E ? (uint32_t)__popc(diff_flags(a, e0, sh_known)) : 0u;
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    if (lane_id() == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) a.part[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// Phase 1 (a thread per selected event, consecutive threads on consecutive rows): the 4- and 8-byte
// columns with the parents' wire indices. Phase 2: the 32-byte id and S rows as 16-byte vectors,
// consecutive lanes on consecutive 16 bytes of the output.
__global__ void __launch_bounds__(kDiffThreads) k_diff_gather(DiffArgs a) {
    __shared__ int32_t sh_known[kDiffMaxN];
    __shared__ int32_t sh_root[kDiffMaxN];
    __shared__ uint16_t sh_src[kDiffChunk];   // the selected events' offsets in the chunk, in gid order
    __shared__ uint32_t sh[4];
    for (int i = threadIdx.x; i < a.n; i += kDiffThreads) {
        sh_known[i] = a.tab[i];
        sh_root[i] = a.tab[a.n + i];
    }
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kDiffChunk;
    const int64_t e0 = base + (int64_t)threadIdx.x * kDiffPer;
    const uint32_t m = e0 < a.E ? diff_flags(a, e0, sh_known) : 0u;
    uint32_t tot;
    uint32_t pos = block_excl_scan256((uint32_t)__popc(m), sh, &tot);
    const uint32_t row0 = a.part[blockIdx.x];
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *a.total = row0 + tot;
    if (tot == 0 || (int64_t)row0 >= a.rows) return;   // (uniform over the workgroup)
#pragma unroll
    for (int k = 0; k < kDiffPer; k++)
        if (m & (1u << k)) sh_src[pos++] = (uint16_t)(threadIdx.x * kDiffPer + k);
    __syncthreads();
    // rows of this workgroup that the caller's arrays hold
    const uint32_t cnt = (uint32_t)(a.rows - row0 < (int64_t)tot ? a.rows - row0 : (int64_t)tot);
    for (uint32_t k = threadIdx.x; k < cnt; k += kDiffThreads) {
        const int64_t e = base + sh_src[k], row = (int64_t)row0 + k;
        const int l = a.g_creator[e] - a.c0;
        if (a.o_gid) a.o_gid[row] = e;
        if (a.o_creator) a.o_creator[row] = l;
        if (a.o_index) a.o_index[row] = a.g_index[e];
        if (a.o_spi) {   // SetWireInfo: Root.Index for a chain's first event (hashgraph.go:537-545)
            const int32_t sp = a.g_sp[e];
            a.o_spi[row] = (sp >= 0 && sp < a.E) ? a.g_index[sp] : sh_root[l];
        }
        if (a.o_opc || a.o_opi || a.o_root) {
            const int32_t op = a.g_op[e];
            const bool ev = op >= 0 && op < a.E;
            if (a.o_opc) a.o_opc[row] = ev ? a.g_creator[op] - a.c0 : -1;
            if (a.o_opi) a.o_opi[row] = ev ? a.g_index[op] : -1;
            if (a.o_root) a.o_root[row] = op == (int32_t)kRootY ? 1 : op == (int32_t)kRootOther ? 2 : 0;
        }
        if (a.o_ts) a.o_ts[row] = a.g_ts[e];
        if (a.o_ntx) a.o_ntx[row] = a.g_ntx[e];
        if (a.o_nil) a.o_nil[row] = a.g_txnil[e];
    }
    if (!a.o_hash && !a.o_S) return;
    for (uint32_t u = threadIdx.x; u < 2 * cnt; u += kDiffThreads) {
        const int64_t src = (base + sh_src[u >> 1]) * 2 + (u & 1), dst = ((int64_t)row0 + (u >> 1)) * 2 + (u & 1);
        if (a.o_hash) ((uint4*)a.o_hash)[dst] = ((const uint4*)a.g_id)[src];
        if (a.o_S) ((uint4*)a.o_S)[dst] = ((const uint4*)a.g_S)[src];
    }
}

void launch_diff(hipStream_t s, const DiffArgs& a) {
    if (a.E <= 0) return;
    const unsigned nb = (unsigned)((a.E + kDiffChunk - 1) / kDiffChunk);
    hipLaunchKernelGGL(k_diff_count, dim3(nb), dim3(kDiffThreads), 0, s, a);
    launch_scan_top(s, a.part, (int)nb);
    hipLaunchKernelGGL(k_diff_gather, dim3(nb), dim3(kDiffThreads), 0, s, a);
}

}  // namespace hgx
