// The resident body store (hgx_keep_bodies): R and the transaction bytes of every
// event, kept where the body paths already put them, and read back by gid.
//
// Layout, per gid: g_R (32 B) beside g_S / g_id / g_ntx / g_txnil, and g_txi [cap + 1], the event's
// first slot of the transaction table tx_off [T + 1] (offsets into one byte arena). An event's
// transactions are consecutive slots, so its bytes are ONE run of the arena:
// [tx_off[g_txi[gid]], tx_off[g_txi[gid + 1]]). g_txi[E] = T and tx_off[T] = the arena's end always.
//
// Append (Engine::bodies_append, one launch behind a chunk's insert_verified): the accepted prefix's
// R rows, slots, rebased offsets and bytes (a prefix of the chunk's byte buffer).
// Gather (Engine::bodies_gather): a list of gids, any order, repeats allowed ->
//   k_body_size   a thread per entry: transaction and byte counts, their 64-bit totals
//   the three-pass scan (launch_scan_u32) over both counts
//   k_body_copy   a wave per entry (lanes of `stripes` waves strided over a long run): the offsets
//                 rebased, the run of bytes moved, R rows as 16-byte vectors on a lane pair
// The host reads the totals between the scan and the copy pass, so every bound of the copy pass is
// known before it launches. No workgroup waits for another.
// hgx_prune_to_frame compacts the store with the same gather (gids = old_gid) into a new arena.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>

#include "hgx_bodystore.h"
#include "hgx_device.h"
#include "hgx_engine.h"

#define HGX_TRY(x)                              \
    do {                                        \
        hipError_t _e = (x);                    \
        if (_e != hipSuccess) return _e;        \
    } while (0)

namespace hgx {

namespace {

struct BodyView {   // the store as the kernels read it
    int64_t E;
    const int32_t* g_ntx;
    const uint8_t* g_txnil;
    const int64_t* g_txi;
    const int64_t* tx_off;
    const uint8_t* arena;
    const uint8_t* g_R;
};

struct BodyGatherArgs {
    int64_t m;
    const int64_t* gids64;   // the list: one of the two
    const int32_t* gids32;
    BodyView st;
    uint32_t *cnt_tx, *cnt_by;     // [m] counts, then their exclusive scans
    unsigned long long* totals;    // [2] transactions, bytes (zeroed before the size pass)
    uint8_t* o_R;                  // [m][32] (null: not wanted)
    int32_t* o_ntx;                // [m] -1 = nil (null: not wanted)
    int64_t* o_txi;                // [m + 1] first slot of each entry (null: not wanted)
    int64_t* o_off;                // [total transactions + 1]
    uint8_t* o_bytes;
};

struct BodyAppendArgs {
    int64_t a, nt, nbytes;   // accepted events, their transactions and bytes
    int64_t E0, T0, B0;      // the store's ends before the append
    const uint8_t* r;        // the chunk: R rows, slots, offsets (chunk-relative), bytes
    const int64_t* txi;
    const int64_t* off;
    const uint8_t* bytes;
    uint8_t* g_R;
    int64_t* g_txi;
    int64_t* tx_off;
    uint8_t* arena;
};

constexpr int kBodyThreads = 256;

// len bytes from src to dst by threads tid of nth (all of them call it with the same arguments): the
// bytes before dst's first 16-byte boundary and the tail one at a time; between them 16-byte vectors
// where src is aligned like dst, else dwords stored aligned and read as two aligned dwords shifted
// together (the second read may pass the run's end by up to 7 bytes: every source buffer has 16 spare,
// the arena by kArenaSpare, the gather scratch by its B + 16, the chunk's staged tx_bytes by the 16
// bytes EvScratch::stage puts behind every column)
__device__ __forceinline__ void copy_bytes(uint8_t* dst, const uint8_t* src, int64_t len, int64_t tid, int64_t nth) {
    if (len <= 0) return;
    int64_t head = (int64_t)((0 - (uintptr_t)dst) & 15);
    if (head > len) head = len;
    for (int64_t k = tid; k < head; k += nth) dst[k] = src[k];
    const uint8_t* s = src + head;
    uint8_t* d = dst + head;
    const int64_t rest = len - head;
    int64_t body;
    if ((((uintptr_t)s) & 15) == 0) {
        const int64_t nv = rest >> 4;
        body = nv << 4;
        const uint4* sv = (const uint4*)s;
        uint4* dv = (uint4*)d;
        for (int64_t k = tid; k < nv; k += nth) dv[k] = sv[k];
    } else {
        const int64_t nw = rest >> 2;
        body = nw << 2;
        const unsigned sh = (unsigned)((uintptr_t)s & 3) * 8;
        const uint32_t* sa = (const uint32_t*)((uintptr_t)s & ~(uintptr_t)3);
        uint32_t* dw = (uint32_t*)d;
        for (int64_t k = tid; k < nw; k += nth) {
            uint32_t v = sa[k];
            if (sh) v = (v >> sh) | (sa[k + 1] << (32 - sh));
            dw[k] = v;
        }
    }
    for (int64_t k = body + tid; k < rest; k += nth) d[k] = s[k];
}

__device__ __forceinline__ int64_t body_gid(const BodyGatherArgs& a, int64_t i) {
    const int64_t g = a.gids64 ? a.gids64[i] : (int64_t)a.gids32[i];
    return (g >= 0 && g < a.st.E) ? g : -1;   // (the host checked its lists; a device list names resident events)
}

__global__ void __launch_bounds__(kBodyThreads) k_body_size(BodyGatherArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kBodyThreads + threadIdx.x;
    unsigned long long nt = 0, nb = 0;
    if (i < a.m) {
        const int64_t g = body_gid(a, i);
        if (g >= 0) {
            const int64_t t0 = a.st.g_txi[g], t1 = a.st.g_txi[g + 1];
            nt = (unsigned long long)(t1 - t0);
            nb = (unsigned long long)(a.st.tx_off[t1] - a.st.tx_off[t0]);
        }
        a.cnt_tx[i] = (uint32_t)nt;
        a.cnt_by[i] = (uint32_t)nb;
    }
    for (int o = 32; o >= 1; o >>= 1) {
        nt += __shfl_xor(nt, o);
        nb += __shfl_xor(nb, o);
    }
    if (lane_id() == 0 && (nt | nb)) {
        atomicAdd(a.totals, nt);
        atomicAdd(a.totals + 1, nb);
    }
}

// grid (ceil(m / 4), stripes): wave w of workgroup x and its stripes-1 siblings in y move entry 4x + w
__global__ void __launch_bounds__(kBodyThreads) k_body_copy(BodyGatherArgs a) {
    const int lane = lane_id();
    const int64_t i = (int64_t)blockIdx.x * (kBodyThreads / 64) + (threadIdx.x >> 6);
    if (i >= a.m) return;
    const int64_t g = body_gid(a, i);
    const int64_t dt = a.cnt_tx[i], db = a.cnt_by[i];
    int64_t t0 = 0, nt = 0, b0 = 0, len = 0;
    if (g >= 0) {
        t0 = a.st.g_txi[g];
        nt = a.st.g_txi[g + 1] - t0;
        b0 = a.st.tx_off[t0];
        len = a.st.tx_off[t0 + nt] - b0;
    }
    const int64_t tid = (int64_t)blockIdx.y * 64 + lane, nth = (int64_t)gridDim.y * 64;
    if (blockIdx.y == 0) {
        if (a.o_R && lane < 2) {
            uint4 v = make_uint4(0, 0, 0, 0);
            if (g >= 0) v = ((const uint4*)a.st.g_R)[2 * g + lane];
            ((uint4*)a.o_R)[2 * i + lane] = v;
        }
        if (lane == 2) {
            if (a.o_ntx) a.o_ntx[i] = (g >= 0 && a.st.g_txnil[g]) ? -1 : (int32_t)nt;
            if (a.o_txi) a.o_txi[i] = dt;
            if (i == a.m - 1) {   // the tables' ends
                if (a.o_txi) a.o_txi[a.m] = dt + nt;
                a.o_off[dt + nt] = db + len;
            }
        }
    }
    for (int64_t j = tid; j < nt; j += nth) a.o_off[dt + j] = db + (a.st.tx_off[t0 + j] - b0);
    copy_bytes(a.o_bytes + db, a.st.arena + b0, len, tid, nth);
}

__global__ void __launch_bounds__(kBodyThreads) k_body_append(BodyAppendArgs a) {
    const int64_t tid = (int64_t)blockIdx.x * kBodyThreads + threadIdx.x, nth = (int64_t)gridDim.x * kBodyThreads;
    const uint4* rs = (const uint4*)a.r;
    uint4* rd = (uint4*)(a.g_R + 32 * a.E0);
    for (int64_t k = tid; k < 2 * a.a; k += nth) rd[k] = rs[k];
    for (int64_t k = tid; k <= a.a; k += nth) a.g_txi[a.E0 + k] = a.T0 + (k < a.a ? a.txi[k] : a.nt);
    for (int64_t j = tid; j <= a.nt; j += nth) a.tx_off[a.T0 + j] = a.B0 + a.off[j];
    copy_bytes(a.arena + a.B0, a.bytes, a.nbytes, tid, nth);
}

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
constexpr int64_t kArenaSpare = 16;   // copy_bytes' shifted reads

}  // namespace

hipError_t Engine::bodies_keep(int64_t tx_hint, int64_t bytes_hint) {
    if (b_R.n < (size_t)std::max<int64_t>(cap, 1) * 32) HGX_TRY(b_R.alloc((size_t)std::max<int64_t>(cap, 1) * 32));
    if (b_txi.n < (size_t)cap + 1) HGX_TRY(b_txi.alloc((size_t)cap + 1));
    if (b_off.n < (size_t)tx_hint + 1) HGX_TRY(b_off.alloc((size_t)tx_hint + 1));
    if (b_arena.n < (size_t)(bytes_hint + kArenaSpare)) HGX_TRY(b_arena.alloc((size_t)(bytes_hint + kArenaSpare)));
    bodies_state = kBodiesComplete;
    return bodies_reset();
}

// the store emptied (hgx_clear, hgx_reset); allocations are kept
hipError_t Engine::bodies_reset() {
    if (bodies_state == kBodiesOff) return hipSuccess;
    bodies_state = kBodiesComplete;
    bodies_events = bodies_tx = bodies_bytes = 0;
    HGX_TRY(hipMemsetAsync(b_txi.p, 0, 8, stream));
    return hipMemsetAsync(b_off.p, 0, 8, stream);
}

// room for add_tx more transactions and add_bytes more bytes: by doubling, a new allocation plus a
// device-to-device copy (hipErrorOutOfMemory: nothing changed)
hipError_t Engine::bodies_reserve(int64_t add_tx, int64_t add_bytes) {
    const int64_t need_t = bodies_tx + add_tx + 1, need_b = bodies_bytes + add_bytes + kArenaSpare;
    const int64_t cap_t = body_grow_plan((int64_t)b_off.n, need_t), cap_b = body_grow_plan((int64_t)b_arena.n, need_b);
    if (cap_t < 0 || cap_b < 0) return hipErrorOutOfMemory;
    if ((size_t)cap_t > b_off.n && b_off.grow_copy((size_t)cap_t, (size_t)bodies_tx + 1, stream) != hipSuccess) {
        (void)hipGetLastError();
        return hipErrorOutOfMemory;
    }
    if ((size_t)cap_b > b_arena.n && b_arena.grow_copy((size_t)cap_b, (size_t)bodies_bytes, stream) != hipSuccess) {
        (void)hipGetLastError();
        return hipErrorOutOfMemory;
    }
    return hipSuccess;
}

// events [0, a) of a chunk behind the store's end: gids [E - a, E) (the chunk's insert has run)
hipError_t Engine::bodies_append(const uint8_t* r, const int64_t* txi, const int64_t* off, const uint8_t* bytes,
                                 int64_t a, int64_t nt, int64_t nbytes) {
    if (a <= 0) return hipSuccess;
    if (bodies_events + a != E || bodies_events + a > cap || (size_t)(bodies_tx + nt + 1) > b_off.n ||
        (size_t)(bodies_bytes + nbytes + kArenaSpare) > b_arena.n)
        return hipErrorInvalidValue;   // (bodies_reserve ran for the whole chunk)
    BodyAppendArgs p{a, nt, nbytes, bodies_events, bodies_tx, bodies_bytes, r, txi, off, bytes,
                     b_R.p, b_txi.p, b_off.p, b_arena.p};
    const int64_t work = std::max<int64_t>(std::max<int64_t>(2 * a, nt + 1), nbytes / 16);
    const unsigned nb = (unsigned)std::min<int64_t>(1024, (work + kBodyThreads - 1) / kBodyThreads);
    hipLaunchKernelGGL(k_body_append, dim3(nb), dim3(kBodyThreads), 0, stream, p);
    HGX_TRY(hipGetLastError());
    bodies_events += a;
    bodies_tx += nt;
    bodies_bytes += nbytes;
    return hipSuccess;
}

hipError_t Engine::bodies_read(BodyTable which, int64_t lo, int64_t count, void* dst) {
    if (bodies_state != kBodiesComplete || lo < 0 || count < 0 || !dst) return hipErrorInvalidValue;
    if (count == 0) return hipSuccess;
    const int64_t have = which == kBodyRows ? bodies_events : which == kBodySlots ? bodies_events + 1
                         : which == kBodyOffsets ? bodies_tx + 1 : bodies_bytes;
    if (lo + count > have) return hipErrorInvalidValue;
    const size_t w = which == kBodyRows ? 32 : which == kBodyArena ? 1 : 8;
    const uint8_t* src = which == kBodyRows ? b_R.p : which == kBodySlots ? (const uint8_t*)b_txi.p
                         : which == kBodyOffsets ? (const uint8_t*)b_off.p : b_arena.p;
    HGX_TRY(hipMemcpyAsync(dst, src + (size_t)lo * w, (size_t)count * w, hipMemcpyDeviceToHost, stream));
    return hipStreamSynchronize(stream);
}

// The sizing half of a gather: the list (host gids, or a device list of either width) measured and
// scanned, its totals read back. plan keeps what the copy half needs.
hipError_t Engine::bodies_measure(const int64_t* gids_host, const int64_t* gids_dev64, const int32_t* gids_dev32,
                                  int64_t m, BodyPlan& plan) {
    plan = BodyPlan();
    plan.m = m;
    if (bodies_state != kBodiesComplete || m < 0) return hipErrorInvalidValue;
    if (m == 0) return hipSuccess;
    const size_t M = (size_t)m, nparts = (M + 2047) / 2048 + 1;
    size_t total = 0;
    auto take = [&](size_t bytes) {
        const size_t off = total;
        total += up256(bytes);
        return off;
    };
    const size_t o_tot = take(16), o_ct = take(4 * M), o_cb = take(4 * M), o_pt = take(4 * nparts), o_pb = take(4 * nparts),
                 o_g = take(gids_host ? 8 * M : 0);
    if (b_work.n < total) HGX_TRY(b_work.alloc(std::max(total, 2 * b_work.n)));
    uint8_t* w = b_work.p;
    if (gids_host) {
        HGX_TRY(hipMemcpyAsync(w + o_g, gids_host, 8 * M, hipMemcpyHostToDevice, stream));
        gids_dev64 = (const int64_t*)(w + o_g);
        gids_dev32 = nullptr;
    }
    plan.gids64 = gids_dev64;
    plan.gids32 = gids_dev64 ? nullptr : gids_dev32;
    plan.cnt_tx = (uint32_t*)(w + o_ct);
    plan.cnt_by = (uint32_t*)(w + o_cb);
    HGX_TRY(hipMemsetAsync(w + o_tot, 0, 16, stream));
    BodyGatherArgs a{};
    a.m = m; a.gids64 = plan.gids64; a.gids32 = plan.gids32;
    a.st = BodyView{bodies_events, g_ntx.p, g_txnil.p, b_txi.p, b_off.p, b_arena.p, b_R.p};
    a.cnt_tx = plan.cnt_tx; a.cnt_by = plan.cnt_by; a.totals = (unsigned long long*)(w + o_tot);
    hipLaunchKernelGGL(k_body_size, dim3((unsigned)((M + kBodyThreads - 1) / kBodyThreads)), dim3(kBodyThreads), 0, stream, a);
    launch_scan_u32(stream, a.cnt_tx, m, (uint32_t*)(w + o_pt));
    launch_scan_u32(stream, a.cnt_by, m, (uint32_t*)(w + o_pb));
    HGX_TRY(hipGetLastError());
    unsigned long long tot[2] = {0, 0};
    HGX_TRY(hipMemcpyAsync(tot, w + o_tot, 16, hipMemcpyDeviceToHost, stream));
    HGX_TRY(hipStreamSynchronize(stream));
    plan.n_tx = (int64_t)tot[0];
    plan.n_bytes = (int64_t)tot[1];
    // the scans are 32-bit: one gather moves less than 4 Gi transactions and less than 4 GiB
    plan.too_large = (tot[0] >> 32) != 0 || (tot[1] >> 32) != 0;
    return hipSuccess;
}

// The copy half into device memory: o_R [m][32] (may be null), o_ntx [m] (may be null), o_txi [m + 1] (may be null),
// o_off [n_tx + 1], o_bytes [n_bytes (+ nothing read past it)]
hipError_t Engine::bodies_copy(const BodyPlan& plan, uint8_t* o_R, int32_t* o_ntx, int64_t* o_txi, int64_t* o_off,
                               uint8_t* o_bytes) {
    if (plan.m <= 0 || plan.too_large) return plan.too_large ? hipErrorInvalidValue : hipSuccess;
    BodyGatherArgs a{};
    a.m = plan.m; a.gids64 = plan.gids64; a.gids32 = plan.gids32;
    a.st = BodyView{bodies_events, g_ntx.p, g_txnil.p, b_txi.p, b_off.p, b_arena.p, b_R.p};
    a.cnt_tx = plan.cnt_tx; a.cnt_by = plan.cnt_by;
    a.o_R = o_R; a.o_ntx = o_ntx; a.o_txi = o_txi; a.o_off = o_off; a.o_bytes = o_bytes;
    // waves per entry from the mean run: a wave moves 1 KiB per pass over its run. (One very long run
    // among many short ones is still moved by the few waves the mean gives it: slower, never wrong.)
    const int64_t mean = plan.n_bytes / plan.m;
    const unsigned stripes = (unsigned)std::min<int64_t>(32, std::max<int64_t>(1, mean / 4096));
    hipLaunchKernelGGL(k_body_copy, dim3((unsigned)((plan.m + 3) / 4), stripes), dim3(kBodyThreads), 0, stream, a);
    return hipGetLastError();
}

// hgx_get_event_bodies and the consumers that stand on it: measure, check the caller's capacities,
// copy into scratch, ONE device-to-host copy into page-locked memory, then the caller's arrays.
// *fit: BodyFit (anything but kBodyFits: the totals alone were reported, HGX_ERR_CAPACITY).
hipError_t Engine::bodies_gather(const int64_t* gids_host, const int64_t* gids_dev64, const int32_t* gids_dev32,
                                 int64_t m, const BodyOut& out, int64_t* n_tx, int64_t* n_bytes, BodyFit* fit) {
    BodyPlan plan;
    *fit = kBodyShort;
    HGX_TRY(bodies_measure(gids_host, gids_dev64, gids_dev32, m, plan));
    *n_tx = plan.n_tx;
    *n_bytes = plan.n_bytes;
    if (plan.too_large) {
        *fit = kBodyTooLarge;
        return hipSuccess;
    }
    if (body_out_fits(plan.n_tx, plan.n_bytes, out.tx_off, out.tx_cap, out.tx_bytes, out.bytes_cap)) return hipSuccess;
    *fit = kBodyFits;
    return bodies_fetch(plan, out);
}

hipError_t Engine::bodies_fetch(const BodyPlan& plan, const BodyOut& out) {
    const int64_t m = plan.m;
    if (m == 0) {
        if (out.tx_off) out.tx_off[0] = 0;
        return hipSuccess;
    }
    const size_t M = (size_t)m, T = (size_t)plan.n_tx, B = (size_t)plan.n_bytes;
    const size_t o_R = 0, o_off = up256(32 * M), o_ntx = o_off + up256(8 * (T + 1)), o_by = o_ntx + up256(4 * M),
                 total = o_by + up256(B + 16);
    if (b_out.n < total) HGX_TRY(b_out.alloc(std::max(total, 2 * b_out.n)));
    if (b_host_cap < total) {
        if (b_host) (void)hipHostFree(b_host);
        b_host = nullptr;
        b_host_cap = 0;
        const size_t want = std::max(total, (size_t)1 << 16);
        HGX_TRY(hipHostMalloc((void**)&b_host, want, hipHostMallocDefault));
        b_host_cap = want;
    }
    uint8_t* d = b_out.p;
    // (a per-event column nobody asked for is not gathered: hgx_block_transactions wants neither)
    HGX_TRY(bodies_copy(plan, out.sig_r ? d + o_R : nullptr, out.ntx ? (int32_t*)(d + o_ntx) : nullptr, nullptr,
                        (int64_t*)(d + o_off), d + o_by));
    HGX_TRY(hipMemcpyAsync(b_host, d, o_by + B, hipMemcpyDeviceToHost, stream));
    HGX_TRY(hipStreamSynchronize(stream));
    if (out.sig_r) std::memcpy(out.sig_r, b_host + o_R, 32 * M);
    if (out.ntx) std::memcpy(out.ntx, b_host + o_ntx, 4 * M);
    if (out.tx_off) std::memcpy(out.tx_off, b_host + o_off, 8 * (T + 1));
    if (out.tx_bytes && B) std::memcpy(out.tx_bytes, b_host + o_by, B);
    return hipSuccess;
}

// hgx_prune_to_frame, before the events are dropped: the kept events' bodies gathered through
// old_gid (device, kept entries) into new tables, which bodies_install puts in place once the
// context has been cleared. A failure here leaves the store as it was and no new table allocated.
hipError_t Engine::bodies_compact(const int32_t* old_gid_dev, int64_t kept, bool* too_large) {
    b_new_ready = false;
    *too_large = false;
    if (bodies_state != kBodiesComplete) return hipSuccess;
    BodyPlan plan;
    HGX_TRY(bodies_measure(nullptr, nullptr, old_gid_dev, kept, plan));
    if (plan.too_large) {
        *too_large = true;
        return hipSuccess;
    }
    const size_t K = (size_t)kept;
    const int64_t cap_t = body_grow_plan(0, plan.n_tx + 1), cap_b = body_grow_plan(0, plan.n_bytes + kArenaSpare);
    const size_t o_txi = up256(32 * std::max<size_t>(K, 1));
    if (b_new_off.alloc((size_t)cap_t) != hipSuccess || b_new_arena.alloc((size_t)cap_b) != hipSuccess ||
        b_new_rows.alloc(o_txi + 8 * (K + 1)) != hipSuccess) {
        (void)hipGetLastError();
        b_new_off.release();
        b_new_arena.release();
        b_new_rows.release();
        return hipErrorOutOfMemory;
    }
    if (kept > 0) {
        HGX_TRY(bodies_copy(plan, b_new_rows.p, nullptr, (int64_t*)(b_new_rows.p + o_txi), b_new_off.p, b_new_arena.p));
    } else {
        HGX_TRY(hipMemsetAsync(b_new_rows.p + o_txi, 0, 8, stream));
        HGX_TRY(hipMemsetAsync(b_new_off.p, 0, 8, stream));
    }
    HGX_TRY(hipStreamSynchronize(stream));
    b_new_events = kept;
    b_new_tx = plan.n_tx;
    b_new_bytes = plan.n_bytes;
    b_new_ready = true;
    return hipSuccess;
}

hipError_t Engine::bodies_install() {
    if (!b_new_ready) return hipSuccess;
    b_new_ready = false;
    const size_t K = (size_t)b_new_events, o_txi = up256(32 * std::max<size_t>(K, 1));
    if (K) HGX_TRY(hipMemcpyAsync(b_R.p, b_new_rows.p, 32 * K, hipMemcpyDeviceToDevice, stream));
    HGX_TRY(hipMemcpyAsync(b_txi.p, b_new_rows.p + o_txi, 8 * (K + 1), hipMemcpyDeviceToDevice, stream));
    HGX_TRY(hipStreamSynchronize(stream));
    b_new_rows.release();
    std::swap(b_off.p, b_new_off.p);
    std::swap(b_off.n, b_new_off.n);
    std::swap(b_arena.p, b_new_arena.p);
    std::swap(b_arena.n, b_new_arena.n);
    b_new_off.release();     // the old tables: the dropped events' bytes go back to the device
    b_new_arena.release();
    bodies_events = b_new_events;
    bodies_tx = b_new_tx;
    bodies_bytes = b_new_bytes;
    return hipSuccess;
}

}  // namespace hgx
