// hgx_get_frame_bodies on the device: Go's Body.Parents of every frame event as ids.
//
// The frame's selection, its remapped columns and the old gid of every frame event are launch_prune's
// (hgx_compact.hip), unchanged. What a peer needs beside them is the text of both parents, whether
// or not the parent is in the frame. A stored parent names its source:
//   a gid >= 0                 that event's row of g_id;
//   self-parent -1             the creator's Root.X row of root_tab when the root has an X, else "";
//   other-parent HGX_ROOT_Y    the creator's Root.Y row of root_tab;
//   other-parent HGX_ROOT_OTHER the value of the Root.Others pair whose key is the event's own id
//                              (a binary search of root_pairs, keys as 4 big-endian words);
//   other-parent -1            "".
// A root id or a pair that must exist and does not sets a fail word (the host reports a panic); the
// row is never left as a silent zero. No atomics, no workgroup waits for another, every loop bounded.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hgx_device.h"
#include "hgx_kernels.h"

namespace hgx {

constexpr int kFrameThreads = 256;

__device__ __forceinline__ uint64_t frame_be64(const uint8_t* p) { return __builtin_bswap64(*(const uint64_t*)p); }

// the value row of the pair whose key is id32 (null: no such pair); at most 64 halvings
__device__ __forceinline__ const uint8_t* frame_find_pair(const FrameArgs& a, const uint8_t* id32) {
    const uint64_t k0 = frame_be64(id32), k1 = frame_be64(id32 + 8), k2 = frame_be64(id32 + 16), k3 = frame_be64(id32 + 24);
    int64_t lo = 0, hi = a.n_pairs;
    for (int it = 0; it < 64 && lo < hi; it++) {
        const int64_t mid = lo + (hi - lo) / 2;
        const uint64_t* q = a.root_pairs + 8 * mid;
        int c = q[0] < k0 ? -1 : q[0] > k0 ? 1 : 0;   // the pair's key against the event's
        if (!c) c = q[1] < k1 ? -1 : q[1] > k1 ? 1 : 0;
        if (!c) c = q[2] < k2 ? -1 : q[2] > k2 ? 1 : 0;
        if (!c) c = q[3] < k3 ? -1 : q[3] > k3 ? 1 : 0;
        if (!c) return (const uint8_t*)(q + 4);
        if (c < 0) lo = mid + 1; else hi = mid;
    }
    return nullptr;
}

// 256 frame events per workgroup. Phase 1 (a lane per event): the source row of each parent id and
// the flag byte. Phase 2: the 32-byte rows as 16-byte vectors, consecutive lanes on consecutive
// 16 bytes of the output (first the self-parent column's 512 pieces, then the other-parent's).
__global__ void __launch_bounds__(kFrameThreads) k_frame_parent_ids(FrameArgs a) {
    __shared__ const uint8_t* sh_src[2 * kFrameThreads];
    const int64_t base = (int64_t)blockIdx.x * kFrameThreads;
    const int64_t k = base + threadIdx.x;
    const uint8_t *s_sp = nullptr, *s_op = nullptr;
    if (k < a.n_kept) {
        const int64_t e = a.old_gid[k];
        bool bad = e < 0 || e >= a.E;
        if (!bad) {
            const int cr = a.g_creator[e];
            const int32_t sp = a.g_sp[e], op = a.g_op[e];
            bad = cr < 0 || cr >= a.C;
            if (!bad) {
                const size_t Cz = (size_t)a.C;
                if (sp >= 0 && sp < a.E) s_sp = a.g_id + 32 * (int64_t)sp;
                else if (sp == -1) s_sp = a.root_tab && a.root_tab[64 * Cz + cr] ? a.root_tab + 32 * (size_t)cr : nullptr;
                else bad = true;
                if (op >= 0 && op < a.E) {
                    s_op = a.g_id + 32 * (int64_t)op;
                } else if (op == (int32_t)kRootY) {
                    s_op = a.root_tab && a.root_tab[65 * Cz + cr] ? a.root_tab + 32 * (Cz + (size_t)cr) : nullptr;
                    bad = bad || !s_op;
                } else if (op == (int32_t)kRootOther) {
                    s_op = a.root_pairs ? frame_find_pair(a, a.g_id + 32 * e) : nullptr;
                    bad = bad || !s_op;
                } else if (op != -1) {
                    bad = true;
                }
            }
        }
        if (bad) {
            *a.fail = 1u;   // (every writer stores the same word)
            s_sp = s_op = nullptr;
        }
        a.o_flags[k] = (uint8_t)((s_sp ? 1 : 0) | (s_op ? 2 : 0));
    }
    sh_src[threadIdx.x] = s_sp;
    sh_src[kFrameThreads + threadIdx.x] = s_op;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int u = threadIdx.x + j * kFrameThreads;   // 0 .. 1023: column, event, half
        const int col = u >> 9, v = u & 511;
        const int64_t row = base + (v >> 1);
        if (row >= a.n_kept) continue;
        const uint8_t* src = sh_src[col * kFrameThreads + (v >> 1)];
        const uint4 x = src ? ((const uint4*)src)[v & 1] : make_uint4(0, 0, 0, 0);
        ((uint4*)(col ? a.o_opid : a.o_spid))[row * 2 + (v & 1)] = x;
    }
}

void launch_frame_parent_ids(hipStream_t s, const FrameArgs& a) {
    if (a.n_kept <= 0) return;
    const unsigned nb = (unsigned)((a.n_kept + kFrameThreads - 1) / kFrameThreads);
    hipLaunchKernelGGL(k_frame_parent_ids, dim3(nb), dim3(kFrameThreads), 0, s, a);
}

}  // namespace hgx
