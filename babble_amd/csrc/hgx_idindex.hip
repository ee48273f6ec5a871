// The event-id index on the device (hgx_keep_id_index; the contract is hgx_idindex.h).
//
//   k_idx_insert   a lane per event: rows [first, first + count) of an id column claim their slots with
//                  a 64-bit atomicCAS on an empty word. A lane that loses a slot moves on by +1: it never
//                  waits for another lane.
//   k_idx_find     a lane per query: idx_probe from the home slot to the first empty one.
//   k_idx_stats    a lane per slot: entries, summed displacement, entries below their home slot.
//   k_idx_resolve  a lane per event of an hgx_insert_events_by_id batch: both parents' ids -> gids and
//                  the root codes, against the resident table and then the batch's scratch table.
//
// A table is written by one launch and read by later launches on the context's stream only: no kernel
// inserts into and reads from the same table, so the kernel boundary is all the ordering there is.
// Every probe loop is bounded by `slots`; one that reaches the bound raises the sticky word st[0],
// which the host turns into "id index corrupt".
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "hgx.h"
#include "hgx_device.h"
#include "hgx_engine.h"
#include "hgx_idindex.h"

#define HGX_TRY(x)                              \
    do {                                        \
        hipError_t _e = (x);                    \
        if (_e != hipSuccess) return _e;        \
    } while (0)

namespace hgx {

namespace {

constexpr int kIdxThreads = 256;
constexpr int64_t kIdxFindChunk = 1 << 20;   // queries per launch of hgx_find_events (40 MiB of scratch)
// the status block: [0] the corrupt flag (sticky), [1] entries, [2] displacement, [3] wrapped
constexpr int kIdxStWords = 4;

__global__ void __launch_bounds__(kIdxThreads) k_idx_insert(unsigned long long* __restrict__ tab, uint64_t slots,
                                                            const uint8_t* __restrict__ rows, int64_t first,
                                                            int64_t count, unsigned long long* __restrict__ st) {
    const int64_t k = (int64_t)blockIdx.x * kIdxThreads + threadIdx.x;
    if (k >= count) return;
    const int64_t v = first + k;
    const uint8_t* id = rows + 32 * v;
    const unsigned long long w = idx_word(idx_tag(id), v);
    uint64_t s = idx_home(id, slots);
    for (uint64_t i = 0; i < slots; i++, s = (s + 1) & (slots - 1))
        if (atomicCAS(&tab[s], 0ull, w) == 0ull) return;
    st[0] = 1;   // no empty slot: the table holds more than its capacity
}

__global__ void __launch_bounds__(kIdxThreads) k_idx_find(const uint64_t* __restrict__ tab, uint64_t slots,
                                                          const uint8_t* __restrict__ rows, int64_t E,
                                                          const uint8_t* __restrict__ q, int64_t m,
                                                          int64_t* __restrict__ out, unsigned long long* __restrict__ st) {
    const int64_t k = (int64_t)blockIdx.x * kIdxThreads + threadIdx.x;
    if (k >= m) return;
    int64_t r = idx_probe(tab, slots, rows, E, q + 32 * k, E);
    if (r == kIdxCorrupt) {
        st[0] = 1;
        r = kIdxNone;
    }
    out[k] = r;
}

__global__ void __launch_bounds__(kIdxThreads) k_idx_stats(const uint64_t* __restrict__ tab, uint64_t slots,
                                                           const uint8_t* __restrict__ rows, int64_t E,
                                                           unsigned long long* __restrict__ st) {
    const uint64_t s = (uint64_t)blockIdx.x * kIdxThreads + threadIdx.x;
    unsigned long long ent = 0, disp = 0, wr = 0;
    if (s < slots && tab[s] != 0) {
        uint64_t d1 = 0, w1 = 0;
        if (idx_slot_stats(tab, slots, rows, E, s, &d1, &w1)) ent = 1;
        else st[0] = 1;
        disp = d1;
        wr = w1;
    }
    // the wave's sums, one atomic each from its first lane
    for (int d = 32; d > 0; d >>= 1) {
        ent += __shfl_down(ent, d);
        disp += __shfl_down(disp, d);
        wr += __shfl_down(wr, d);
    }
    if (lane_id() == 0 && ent) {
        atomicAdd(&st[1], ent);
        atomicAdd(&st[2], disp);
        atomicAdd(&st[3], wr);
    }
}

// an id as a parent of batch position k: a resident gid first, then the lowest earlier batch position
__device__ __forceinline__ int64_t idx_parent(const IdxResolveArgs& a, const uint8_t* id, int64_t k) {
    int64_t r = idx_probe(a.tab, a.slots, a.g_id, a.E, id, a.E);
    if (r >= 0) return r;
    if (r == kIdxCorrupt) a.st[0] = 1;
    r = idx_probe(a.btab, a.bslots, a.claimed, a.count, id, k);
    if (r >= 0) return a.E + r;
    if (r == kIdxCorrupt) a.st[0] = 1;
    return kIdxNone;
}

__global__ void __launch_bounds__(kIdxThreads) k_idx_resolve(IdxResolveArgs a) {
    const int64_t k = (int64_t)blockIdx.x * kIdxThreads + threadIdx.x;
    if (k >= a.count) return;
    const int fl = a.flags[k];
    const bool has_sp = fl & 1, has_op = fl & 2;
    const uint32_t cr = (uint32_t)a.creator[k];
    const bool rooted = a.root_tab != nullptr && cr < (uint32_t)a.C;   // (an unknown creator has no root)
    const size_t Cz = (size_t)a.C;
    const bool has_x = rooted && a.root_tab[64 * Cz + cr], has_y = rooted && a.root_tab[65 * Cz + cr];
    const uint8_t *x_id = a.root_tab + 32 * (size_t)cr, *y_id = a.root_tab + 32 * Cz + 32 * (size_t)cr;
    const uint8_t *sid = a.sp_id + 32 * k, *oid = a.op_id + 32 * k;
    int64_t sp, op;
    if (!has_sp) {
        // "" is Root.X only where the root has none; else the text would print Root.X for it
        sp = has_x ? HGX_UNKNOWN_PARENT : -1;
    } else {
        sp = idx_parent(a, sid, k);
        if (sp < 0) sp = (has_x && idx_row_eq(sid, x_id)) ? -1 : HGX_UNKNOWN_PARENT;
    }
    if (!has_op) {
        op = -1;
    } else {
        op = idx_parent(a, oid, k);
        if (op < 0) {
            if (a.root_tab == nullptr) {
                op = HGX_UNKNOWN_PARENT;
            } else {
                // hashgraph.go:434: other-parent = Root.Y and self-parent = Root.X (both "" counts)
                const bool sp_is_x = has_sp == has_x && (!has_sp || idx_row_eq(sid, x_id));
                op = (has_y && idx_row_eq(oid, y_id) && sp_is_x) ? HGX_ROOT_Y : HGX_ROOT_OTHER;
            }
        }
    }
    a.out_sp[k] = sp;
    a.out_op[k] = op;
}

inline unsigned idx_blocks(uint64_t items) { return (unsigned)((items + kIdxThreads - 1) / kIdxThreads); }
inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

void launch_idx_insert(hipStream_t s, uint64_t* tab, uint64_t slots, const uint8_t* rows, int64_t first, int64_t count,
                       uint64_t* st) {
    if (count <= 0) return;
    hipLaunchKernelGGL(k_idx_insert, dim3(idx_blocks((uint64_t)count)), dim3(kIdxThreads), 0, s, (unsigned long long*)tab,
                       slots, rows, first, count, (unsigned long long*)st);
}

void launch_idx_find(hipStream_t s, const uint64_t* tab, uint64_t slots, const uint8_t* rows, int64_t E, const uint8_t* q,
                     int64_t m, int64_t* out, uint64_t* st) {
    if (m <= 0) return;
    hipLaunchKernelGGL(k_idx_find, dim3(idx_blocks((uint64_t)m)), dim3(kIdxThreads), 0, s, tab, slots, rows, E, q, m, out,
                       (unsigned long long*)st);
}

void launch_idx_stats(hipStream_t s, const uint64_t* tab, uint64_t slots, const uint8_t* rows, int64_t E, uint64_t* st) {
    hipLaunchKernelGGL(k_idx_stats, dim3(idx_blocks(slots)), dim3(kIdxThreads), 0, s, tab, slots, rows, E,
                       (unsigned long long*)st);
}

void launch_idx_resolve(hipStream_t s, const IdxResolveArgs& a) {
    if (a.count <= 0) return;
    hipLaunchKernelGGL(k_idx_resolve, dim3(idx_blocks((uint64_t)a.count)), dim3(kIdxThreads), 0, s, a);
}

// hgx_keep_id_index: the table for this context's capacity, built from the resident ids when they are
// known. hipErrorOutOfMemory: nothing is kept.
hipError_t Engine::idx_keep() {
    if (idx_kept) return hipSuccess;
    const uint64_t slots = idx_slots_for(std::max<int64_t>(cap, 1));
    if (idx_tab.alloc((size_t)slots) != hipSuccess || idx_st.alloc(kIdxStWords) != hipSuccess) {
        (void)hipGetLastError();
        idx_tab.release();
        idx_st.release();
        return hipErrorOutOfMemory;
    }
    idx_slots = slots;
    idx_kept = true;
    HGX_TRY(hipMemsetAsync(idx_st.p, 0, kIdxStWords * 8, stream));
    HGX_TRY(idx_zero());
    HGX_TRY(idx_append());
    return hipStreamSynchronize(stream);
}

// the table emptied (hgx_clear, hgx_reset, and ahead of a prune's or a bootstrap's re-insert)
hipError_t Engine::idx_zero() {
    if (!idx_kept) return hipSuccess;
    idx_done = 0;
    return hipMemsetAsync(idx_tab.p, 0, (size_t)idx_slots * 8, stream);
}

// the events not yet indexed, [idx_done, E), in one launch behind whatever committed their ids; nothing
// while the ids are not known (the index is invalid until a clear makes them known again)
hipError_t Engine::idx_append() {
    if (!idx_kept || !ids_known || idx_done >= E) return hipSuccess;
    const int64_t count = E - idx_done;
    launch_idx_insert(stream, idx_tab.p, idx_slots, g_id.p, idx_done, count, idx_st.p);
    idx_done = E;
    return hipGetLastError();
}

// the sticky corrupt flag (after a synchronize)
hipError_t Engine::idx_read_flag(bool* corrupt) {
    unsigned long long f = 0;
    HGX_TRY(hipMemcpyAsync(&f, idx_st.p, 8, hipMemcpyDeviceToHost, stream));
    HGX_TRY(hipStreamSynchronize(stream));
    *corrupt = f != 0;
    return hipSuccess;
}

hipError_t Engine::idx_state(int64_t out[5], bool* corrupt) {
    *corrupt = false;
    out[0] = !idx_kept ? 0 : ids_known ? 1 : 2;
    out[1] = idx_kept ? (int64_t)idx_slots : 0;
    out[2] = out[3] = out[4] = 0;
    if (out[0] != 1) return hipSuccess;
    HGX_TRY(idx_append());
    HGX_TRY(hipMemsetAsync(idx_st.p + 1, 0, 3 * 8, stream));
    launch_idx_stats(stream, idx_tab.p, idx_slots, g_id.p, E, idx_st.p);
    HGX_TRY(hipGetLastError());
    unsigned long long st[kIdxStWords] = {};
    HGX_TRY(hipMemcpyAsync(st, idx_st.p, sizeof(st), hipMemcpyDeviceToHost, stream));
    HGX_TRY(hipStreamSynchronize(stream));
    *corrupt = st[0] != 0;
    out[2] = (int64_t)st[1];
    out[3] = (int64_t)st[2];
    out[4] = (int64_t)st[3];
    return hipSuccess;
}

// hgx_find_events: m queries of 32 bytes (host) -> gids or -1 (host), in chunks of kIdxFindChunk
hipError_t Engine::idx_find(const uint8_t* id32, int64_t m, int64_t* out_gid, bool* corrupt) {
    *corrupt = false;
    if (!idx_kept || !ids_known) return hipErrorInvalidValue;
    HGX_TRY(idx_append());
    const size_t chunk = (size_t)std::min(m, kIdxFindChunk), o_out = up256(chunk * 32);
    if (idx_buf.n < o_out + chunk * 8) HGX_TRY(idx_buf.alloc(o_out + chunk * 8));
    for (int64_t k0 = 0; k0 < m; k0 += kIdxFindChunk) {
        const int64_t c = std::min(kIdxFindChunk, m - k0);
        HGX_TRY(hipMemcpyAsync(idx_buf.p, id32 + 32 * k0, (size_t)c * 32, hipMemcpyHostToDevice, stream));
        launch_idx_find(stream, idx_tab.p, idx_slots, g_id.p, E, idx_buf.p, c, (int64_t*)(idx_buf.p + o_out), idx_st.p);
        HGX_TRY(hipGetLastError());
        HGX_TRY(hipMemcpyAsync(out_gid + k0, idx_buf.p + o_out, (size_t)c * 8, hipMemcpyDeviceToHost, stream));
        HGX_TRY(hipStreamSynchronize(stream));   // (pageable host memory on both sides of the chunk)
    }
    return idx_read_flag(corrupt);
}

// hgx_insert_events_by_id's resolution: two launches. The first builds the scratch table of the batch's
// claimed ids (value = position), the second probes the resident table and then the scratch table for
// every present parent. Host columns in, the two resolved columns (16 bytes per event) out.
hipError_t Engine::idx_resolve(const uint8_t* claimed, const uint8_t* sp_id, const uint8_t* op_id, const uint8_t* flags,
                               const int32_t* creator, int64_t count, int64_t* out_sp, int64_t* out_op, bool* corrupt) {
    *corrupt = false;
    if (!idx_kept || !ids_known || count <= 0) return hipErrorInvalidValue;
    HGX_TRY(idx_append());
    const size_t c = (size_t)count;
    const uint64_t bslots = idx_slots_for(count);
    size_t total = 0;
    auto take = [&](size_t bytes) {
        const size_t off = total;
        total += up256(bytes);
        return off;
    };
    const size_t o_btab = take((size_t)bslots * 8), o_cl = take(c * 32), o_sp = take(c * 32), o_op = take(c * 32),
                 o_fl = take(c), o_cr = take(c * 4), o_osp = take(c * 8), o_oop = take(c * 8);
    if (idx_buf.n < total) HGX_TRY(idx_buf.alloc(total));
    uint8_t* b = idx_buf.p;
    HGX_TRY(hipMemsetAsync(b + o_btab, 0, (size_t)bslots * 8, stream));
    HGX_TRY(hipMemcpyAsync(b + o_cl, claimed, c * 32, hipMemcpyHostToDevice, stream));
    if (sp_id) HGX_TRY(hipMemcpyAsync(b + o_sp, sp_id, c * 32, hipMemcpyHostToDevice, stream));
    if (op_id) HGX_TRY(hipMemcpyAsync(b + o_op, op_id, c * 32, hipMemcpyHostToDevice, stream));
    HGX_TRY(hipMemcpyAsync(b + o_fl, flags, c, hipMemcpyHostToDevice, stream));
    HGX_TRY(hipMemcpyAsync(b + o_cr, creator, c * 4, hipMemcpyHostToDevice, stream));
    launch_idx_insert(stream, (uint64_t*)(b + o_btab), bslots, b + o_cl, 0, count, idx_st.p);
    IdxResolveArgs a{};
    a.tab = idx_tab.p; a.slots = idx_slots; a.g_id = g_id.p; a.E = E;
    a.btab = (const uint64_t*)(b + o_btab); a.bslots = bslots; a.claimed = b + o_cl; a.count = count;
    a.sp_id = b + o_sp; a.op_id = b + o_op; a.flags = b + o_fl; a.creator = (const int32_t*)(b + o_cr); a.C = C;
    a.root_tab = root_ids_set ? root_tab_d.p : nullptr;
    a.out_sp = (int64_t*)(b + o_osp); a.out_op = (int64_t*)(b + o_oop);
    a.st = idx_st.p;
    launch_idx_resolve(stream, a);
    HGX_TRY(hipGetLastError());
    HGX_TRY(hipMemcpyAsync(out_sp, b + o_osp, c * 8, hipMemcpyDeviceToHost, stream));
    HGX_TRY(hipMemcpyAsync(out_op, b + o_oop, c * 8, hipMemcpyDeviceToHost, stream));
    return idx_read_flag(corrupt);
}

}  // namespace hgx
