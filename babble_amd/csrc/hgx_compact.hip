// hgx_prune_to_frame on the device: the resident events cut down to the frame
// GetFrame would return (hashgraph.go:897-995), renumbered, as the columns of one insert batch.
//
// The frame is a suffix of every chain, so an event is kept iff its Index is at least its chain's
// cut (cut[c], from the host's round tables; INT32_MAX for a chain that keeps nothing). gids are
// topological, so the new gid of a kept event is the number of kept events before it: an exclusive
// scan of the keep flags (k_scan_reduce / k_scan_top / k_scan_down, hgx_kernels.hip). One gather
// kernel then writes every kept event's columns at its new gid with the parents resolved as
// InsertEvent resolves them after a Reset (hashgraph.go:404-445):
//   a kept parent -> its new gid; the self-parent of a chain's first kept event -> -1 (Root.X);
//   an other-parent outside the frame -> HGX_ROOT_Y for the chain's first kept event, else
//   HGX_ROOT_OTHER (the event is a key of Root.Others).
// No workgroup waits for another: the keep flag of any event is recomputed from (creator, Index)
// and the scan is complete before the gather starts.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hgx_device.h"
#include "hgx_kernels.h"

namespace hgx {

constexpr int kPruneThreads = 256;

__device__ __forceinline__ bool prune_kept(const PruneArgs& a, int64_t x) {
    return a.g_index[x] >= a.cut[a.g_creator[x]];
}

// keep flags (the scan's input) and, per chain, the gid of its first kept event
__global__ void __launch_bounds__(kPruneThreads) k_prune_mark(PruneArgs a) {
    const int64_t e = (int64_t)blockIdx.x * kPruneThreads + threadIdx.x;
    if (e >= a.E) return;
    const int cr = a.g_creator[e];
    const int32_t idx = a.g_index[e], c = a.cut[cr];
    a.scan[e] = idx >= c ? 1u : 0u;
    if (idx == c) a.first_gid[cr] = (int32_t)e;
}

__device__ __forceinline__ void copy_row32(uint8_t* dst, const uint8_t* src) {
    const uint4* s = (const uint4*)src;
    uint4* d = (uint4*)dst;
    d[0] = s[0];
    d[1] = s[1];
}

__device__ __forceinline__ void zero_row32(uint8_t* dst) {
    uint4* d = (uint4*)dst;
    d[0] = make_uint4(0, 0, 0, 0);
    d[1] = make_uint4(0, 0, 0, 0);
}

// 256 events per workgroup. Phase 1 (a thread per event, coalesced along gid): the 4- and 8-byte
// columns, the remapped parents, old_gid and the Root.Others entries. Phase 2: the 32-byte id and S
// rows of the kept events as 16-byte vectors, consecutive lanes on consecutive 16 bytes.
__global__ void __launch_bounds__(kPruneThreads) k_prune_gather(PruneArgs a) {
    __shared__ int32_t sh_new[kPruneThreads];
    const int64_t base = (int64_t)blockIdx.x * kPruneThreads;
    const int64_t e = base + threadIdx.x;
    int32_t nw = -1;
    bool oth = false;
    int32_t op = -1;
    if (e < a.E) {
        const int cr = a.g_creator[e];
        const int32_t idx = a.g_index[e], c = a.cut[cr];
        const uint32_t pos = a.scan[e];
        if (idx >= c && (int64_t)pos < a.n_kept) {
            nw = (int32_t)pos;
            const bool first = idx == c;
            const int32_t sp = a.g_sp[e];
            op = a.g_op[e];
            int32_t sp_new = -1, op_new = -1;
            if (!first && sp >= 0 && sp < a.E) sp_new = (int32_t)a.scan[sp];
            if (op != -1) {
                if (op >= 0 && op < a.E && prune_kept(a, op)) op_new = (int32_t)a.scan[op];
                else if (first) op_new = (int32_t)kRootY;
                else { op_new = (int32_t)kRootOther; oth = true; }
            }
            a.st_creator[nw] = cr;
            a.st_index[nw] = idx;
            a.st_sp[nw] = sp_new;
            a.st_op[nw] = op_new;
            a.st_ts[nw] = a.g_ts[e];
            a.st_ntx[nw] = a.g_txnil[e] ? -1 : a.g_ntx[e];   // hgx_events32's ntx: -1 = nil Transactions
            a.old_gid[nw] = (int32_t)e;
        }
        if (e == a.E - 1) *a.kept_total = pos + (idx >= c ? 1u : 0u);
    }
    sh_new[threadIdx.x] = nw;
    // Root.Others entries: one counter increment per wave
    const uint64_t m = __ballot(oth);
    if (m) {
        const int lane = lane_id();
        const int leader = __ffsll((long long)m) - 1;
        uint32_t slot0 = 0;
        if (lane == leader) slot0 = atomicAdd(a.oth_count, (uint32_t)__popcll(m));
        slot0 = __shfl(slot0, leader);
        const int64_t slot = (int64_t)slot0 + __popcll(m & ((1ull << lane) - 1ull));
        if (oth && slot < a.n_kept) {
            a.oth_new[slot] = nw;
            a.oth_op[slot] = op;
            copy_row32(a.oth_key + 32 * slot, a.g_id + 32 * e);
            if (op >= 0 && op < a.E) copy_row32(a.oth_pid + 32 * slot, a.g_id + 32 * (int64_t)op);
            else zero_row32(a.oth_pid + 32 * slot);
        }
    }
    if (!__syncthreads_or(nw >= 0)) return;
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int u = threadIdx.x + j * kPruneThreads;
        const int32_t d = sh_new[u >> 1];
        if (d < 0) continue;
        const int64_t src = (base + (u >> 1)) * 2 + (u & 1), dst = (int64_t)d * 2 + (u & 1);
        ((uint4*)a.st_hash)[dst] = ((const uint4*)a.g_id)[src];
        ((uint4*)a.st_S)[dst] = ((const uint4*)a.g_S)[src];
    }
}

// per participant: the first kept event's parents and the ids of the event and of both parents
// (the new Root's X and Y; zero rows where a parent is not a stored event)
__global__ void __launch_bounds__(kPruneThreads) k_prune_roots(PruneArgs a) {
    const int p = blockIdx.x * kPruneThreads + threadIdx.x;
    if (p >= a.C) return;
    const int32_t e = a.first_gid[p];
    uint8_t* ids = a.root_ids + 96 * (int64_t)p;
    if (e < 0 || e >= a.E) {
        a.root_sp[p] = -1;
        a.root_op[p] = -1;
        zero_row32(ids);
        zero_row32(ids + 32);
        zero_row32(ids + 64);
        return;
    }
    const int32_t sp = a.g_sp[e], op = a.g_op[e];
    a.root_sp[p] = sp;
    a.root_op[p] = op;
    copy_row32(ids, a.g_id + 32 * (int64_t)e);
    if (sp >= 0 && sp < a.E) copy_row32(ids + 32, a.g_id + 32 * (int64_t)sp); else zero_row32(ids + 32);
    if (op >= 0 && op < a.E) copy_row32(ids + 64, a.g_id + 32 * (int64_t)op); else zero_row32(ids + 64);
}

void launch_prune(hipStream_t s, const PruneArgs& a, uint32_t* scan_part) {
    if (a.E <= 0) return;
    const unsigned nb = (unsigned)((a.E + kPruneThreads - 1) / kPruneThreads);
    hipLaunchKernelGGL(k_prune_mark, dim3(nb), dim3(kPruneThreads), 0, s, a);
    hipLaunchKernelGGL(k_prune_roots, dim3((unsigned)((a.C + kPruneThreads - 1) / kPruneThreads)), dim3(kPruneThreads), 0, s, a);
    launch_scan_u32(s, a.scan, a.E, scan_part);
    hipLaunchKernelGGL(k_prune_gather, dim3(nb), dim3(kPruneThreads), 0, s, a);
}

}  // namespace hgx
