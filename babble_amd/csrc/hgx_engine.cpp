// Engine host code: device allocation, per-call orchestration of the kernels,
// D2H of the small per-round tables the Go-semantics bookkeeping needs.
#include "hgx_engine.h"
#include "hgx_bodystore.h"

#include <algorithm>
#include <array>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>

namespace hgx {

template <typename T>
hipError_t DBuf<T>::alloc(size_t count) {
    release();
    if (count == 0) count = 1;
    hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
    if (e == hipSuccess) n = count; else p = nullptr;
    return e;
}

template <typename T>
hipError_t DBuf<T>::grow_copy(size_t count, size_t keep, hipStream_t s) {
    if (count <= n) return hipSuccess;
    T* q = nullptr;
    HGX_TRY(hipMalloc((void**)&q, count * sizeof(T)));
    if (p && keep) {
        HGX_TRY(hipMemcpyAsync(q, p, std::min(keep, n) * sizeof(T), hipMemcpyDeviceToDevice, s));
        HGX_TRY(hipStreamSynchronize(s));
    }
    if (p) (void)hipFree(p);
    p = q;
    n = count;
    return hipSuccess;
}

template <typename T>
void DBuf<T>::release() {
    if (p && own) (void)hipFree(p);
    p = nullptr;
    n = 0;
    own = true;
}

template struct DBuf<int32_t>;
template struct DBuf<int64_t>;
template struct DBuf<uint8_t>;
template struct DBuf<int8_t>;
template struct DBuf<uint32_t>;
template struct DBuf<uint64_t>;
template struct DBuf<unsigned long long>;

static int bitlen(uint64_t v) {
    int b = 0;
    while (v) { b++; v >>= 1; }
    return b;
}

// ---- chain-sharded group -------------------------------------------------
bool ShardGroup::wait() {
    std::unique_lock<std::mutex> lk(m);
    if (broken) return false;
    const uint64_t g = gen;
    if (++count == W) {
        count = 0;
        gen++;
        cv.notify_all();
        return true;
    }
    // (a shard that failed breaks the barrier; the time limit only guards against a lost thread)
    if (!cv.wait_for(lk, std::chrono::seconds(120), [&] { return gen != g || broken; })) broken = true;
    if (broken) cv.notify_all();
    return !broken;
}

void ShardGroup::fail() {
    std::lock_guard<std::mutex> lk(m);
    broken = true;
    cv.notify_all();
}

void ShardGroup::rearm() {
    std::lock_guard<std::mutex> lk(m);
    broken = false;
    count = 0;
}

hipError_t Engine::share_round_rows(int32_t r_a, int32_t r_b) {
    if (!grp || grp->W < 2) return hipSuccess;
    const int lo = grp->c_split[shard], hi = grp->c_split[shard + 1];
    if (hi <= lo || r_b < r_a) return hipSuccess;
    const int32_t r_s = std::min(r_b, r_cap - 1);   // rows of the [r_cap x C] tables
    const size_t Cz = (size_t)C, w = (size_t)(hi - lo);
    for (int k = 0; k < grp->W; k++) {
        if (k == shard) continue;
        Engine* q = grp->eng[k];
        // the peer's tables have the same shapes (identical calls, identical growth)
        if (q->r_cap != r_cap) return hipErrorInvalidValue;
        HGX_TRY(hipMemcpy2DAsync(q->Bm.p + (size_t)r_a * Cz + lo, Cz * 4, Bm.p + (size_t)r_a * Cz + lo, Cz * 4, w * 4,
                                 (size_t)(r_b - r_a + 1), hipMemcpyDefault, stream));
        if (r_s >= r_a) {
            const size_t rows = (size_t)(r_s - r_a + 1);
            HGX_TRY(hipMemcpy2DAsync(q->Smat.p + ((size_t)r_a * Cz + lo) * nw, Cz * nw * 8, Smat.p + ((size_t)r_a * Cz + lo) * nw,
                                     Cz * nw * 8, w * nw * 8, rows, hipMemcpyDefault, stream));
            HGX_TRY(hipMemcpy2DAsync(q->wstat.p + (size_t)r_a * Cz + lo, Cz, wstat.p + (size_t)r_a * Cz + lo, Cz, w, rows,
                                     hipMemcpyDefault, stream));
            HGX_TRY(hipMemcpy2DAsync(q->wflag.p + (size_t)r_a * Cz + lo, Cz, wflag.p + (size_t)r_a * Cz + lo, Cz, w, rows,
                                     hipMemcpyDefault, stream));
        }
    }
    return hipStreamSynchronize(stream);
}

Engine::~Engine() {
    if (stream) (void)wipe_signing_keys();   // the private keys' HBM copy is zeroed before it is freed
    free_ev_scratch(ev_scratch);
    if (pay_thread.joinable()) pay_thread.join();
    if (stream2) (void)hipStreamSynchronize(stream2);
    if (ev_pay) (void)hipEventDestroy(ev_pay);
    if (stream2) (void)hipStreamDestroy(stream2);
    if (stream) (void)hipStreamSynchronize(stream);
    for (auto e : kev) (void)hipEventDestroy(e);
    if (ph0) (void)hipEventDestroy(ph0);
    if (ph1) (void)hipEventDestroy(ph1);
    if (ph2) (void)hipEventDestroy(ph2);
    if (h_small) (void)hipHostFree(h_small);
    if (h_pack) (void)hipHostFree(h_pack);
    if (h_stage) (void)hipHostFree(h_stage);
    if (h_ins) (void)hipHostFree(h_ins);
    if (h_cpar) (void)hipHostFree(h_cpar);
    if (h_flag) (void)hipHostFree(h_flag);
    if (h_segc) (void)hipHostFree(h_segc);
    if (df_host) (void)hipHostFree(df_host);
    if (b_host) (void)hipHostFree(b_host);
    if (pipe_thread.joinable()) pipe_thread.join();
    if (stream_p) {
        (void)hipStreamSynchronize(stream_p);
        (void)hipStreamDestroy(stream_p);
    }
    for (hipEvent_t e : ev_pc) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : ev_lay) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : ev_side) if (e) (void)hipEventDestroy(e);
    if (stream_o) (void)hipStreamSynchronize(stream_o);
    for (auto e : ev_o)
        if (e) (void)hipEventDestroy(e);
    if (stream_o) (void)hipStreamDestroy(stream_o);
    for (auto e : flag_ev)
        if (e) (void)hipEventDestroy(e);
    for (auto e : la_ev)
        if (e) (void)hipEventDestroy(e);
    drop_step_graph();
    if (stream) (void)hipStreamDestroy(stream);
}

hipError_t Engine::init(int device, int n_graphs, int n_part, int64_t cap_events, std::string& why) {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        why = "no HIP device available (libhgx has no CPU fallback)";
        return e != hipSuccess ? e : hipErrorNoDevice;
    }
    if (device < 0 || device >= count) {
        why = "invalid HIP device ordinal";
        return hipErrorInvalidDevice;
    }
    hipDeviceProp_t prop;
    HGX_TRY(hipGetDeviceProperties(&prop, device));
    num_cus = std::max(1, prop.multiProcessorCount);
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        why = std::string("device is ") + prop.gcnArchName + ", libhgx is built for gfx950 (MI355X) only";
        return hipErrorInvalidDeviceFunction;
    }
    dev = device;
    HGX_TRY(hipSetDevice(dev));
    HGX_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    HGX_TRY(hipEventCreate(&ph0));
    HGX_TRY(hipEventCreate(&ph1));
    HGX_TRY(hipEventCreate(&ph2));
    G = n_graphs;
    n = n_part;
    C = G * n;
    sm = 2 * n / 3 + 1;   // hashgraph.go:63
    shard_lo = 0;
    shard_hi = C;
    nw = (n + 63) / 64;
    cap = std::max<int64_t>(cap_events, 1);
    const size_t P = (size_t)cap;
    // positions: the events plus slack for chains to grow in place between DivideRounds
    Ppos = cap + std::max<int64_t>(cap / 2, (int64_t)256 * C);
    const size_t PP = (size_t)Ppos;
    HGX_TRY(g_creator.alloc(P)); HGX_TRY(g_index.alloc(P)); HGX_TRY(g_sp.alloc(P)); HGX_TRY(g_op.alloc(P));
    HGX_TRY(g_ntx.alloc(P)); HGX_TRY(g_rr.alloc(P)); HGX_TRY(g_pos.alloc(P)); HGX_TRY(g_ts.alloc(P));
    HGX_TRY(g_cts.alloc(P)); HGX_TRY(g_ck.alloc(P)); HGX_TRY(g_S.alloc(P * 32)); HGX_TRY(g_coin.alloc(P)); HGX_TRY(g_loaded.alloc(P));
    HGX_TRY(g_txnil.alloc(P)); HGX_TRY(g_id.alloc(P * 32));
    // insert state: no claims, no events per creator
    HGX_TRY(succ.alloc(P)); HGX_TRY(first_none.alloc(C));
    ins_gl_off = ((size_t)3 * C + 1) & ~(size_t)1;
    HGX_TRY(ins_blk.alloc(ins_gl_off + (size_t)2 * G));
    last_gid_d.view(ins_blk.p, C);
    last_index_d.view(ins_blk.p + C, C);
    chain_base_d.view(ins_blk.p + 2 * C, C);
    graph_loaded_d.view((unsigned long long*)(ins_blk.p + ins_gl_off), G);
    HGX_TRY(ins_fail.alloc(1));
    HGX_TRY(hipMemsetAsync(ins_fail.p, 0xFF, 8, stream));   // re-armed after every read
    HGX_TRY(hipHostMalloc((void**)&h_ins, ins_blk.n * sizeof(int32_t), hipHostMallocDefault));
    HGX_TRY(cpar_blk.alloc((size_t)3 * C));
    HGX_TRY(hipHostMalloc((void**)&h_cpar, (size_t)3 * C * sizeof(int32_t), hipHostMallocDefault));
    HGX_TRY(hipMemsetAsync(succ.p, 0xFF, P * 4, stream));
    HGX_TRY(hipMemsetAsync(first_none.p, 0xFF, (size_t)C * 4, stream));
    HGX_TRY(hipMemsetAsync(last_gid_d.p, 0xFF, (size_t)C * 8, stream));   // last_gid, last_index
    HGX_TRY(hipMemsetAsync(chain_base_d.p, 0, (ins_blk.n - (size_t)2 * C) * 4, stream));   // chain_base, graph_loaded
    HGX_TRY(c_off.alloc(C + 1));
    c_len.view(cpar_blk.p, C);
    c_base.view(cpar_blk.p + C, C);
    c_old.view(cpar_blk.p + 2 * C, C);
    HGX_TRY(fu.alloc(C)); HGX_TRY(rcnt.alloc(C));
    HGX_TRY(root_round_d.alloc(C)); HGX_TRY(root_y_ext_d.alloc(C));
    HGX_TRY(hipMemsetAsync(root_round_d.p, 0xFF, (size_t)C * 4, stream));   // genesis: Round -1, Y ""
    HGX_TRY(hipMemsetAsync(root_y_ext_d.p, 0, (size_t)C, stream));
    HGX_TRY(p_gid.alloc(PP)); HGX_TRY(p_chain.alloc(PP)); HGX_TRY(p_op.alloc(PP)); HGX_TRY(p_opu.alloc(PP));
    HGX_TRY(p_opk.alloc(PP));
    HGX_TRY(p_round.alloc(PP)); HGX_TRY(p_rr.alloc(PP)); HGX_TRY(p_ts.alloc(PP)); HGX_TRY(p_cts.alloc(PP));
    fd_ld = (Ppos + 31) & ~(int64_t)31;   // firstDescendants columns: 64-byte aligned 32-position segments
    HGX_TRY(LA.alloc(PP * n));
    HGX_TRY(FDT.alloc((size_t)fd_ld * n + 128));   // slack: compact window staging reads past a column
    HGX_TRY(recv_list.alloc(P)); HGX_TRY(counters.alloc(kCtWords));
    HGX_TRY(hipMemsetAsync(counters.p, 0, kCtWords * 4, stream)); HGX_TRY(order_gid.alloc(P));
    HGX_TRY(scan_part.alloc((size_t)256 * ((P + 2047) / 2048 + 1) / 2048 + 64));
    HGX_TRY(key_a.alloc(P)); HGX_TRY(key_b.alloc(P)); HGX_TRY(val_a.alloc(P)); HGX_TRY(val_b.alloc(P));
    HGX_TRY(hist.alloc((size_t)256 * ((P + 2047) / 2048 + 1)));
    HGX_TRY(minmax.alloc(3));
    HGX_TRY(lr.alloc(G));
    for (auto& e : la_ev) HGX_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HGX_TRY(hipEventCreateWithFlags(&flag_ev[0], hipEventDisableTiming));
    HGX_TRY(hipEventCreateWithFlags(&flag_ev[1], hipEventDisableTiming));
    HGX_TRY(hipHostMalloc((void**)&h_small, kHsWords * sizeof(int32_t), hipHostMallocDefault));
    HGX_TRY(hipHostMalloc((void**)&h_flag, 16 * sizeof(int32_t), hipHostMallocMapped | hipHostMallocCoherent));
    HGX_TRY(hipHostGetDevicePointer((void**)&d_flag, h_flag, 0));
    // rounds: initial guess, grown on demand
    const int lg = std::max(1, bitlen((uint64_t)n));
    // rounds of the largest graph: ~events per graph / (n log n) (SURVEY §8 estimate), x2
    const int64_t per_graph = (cap + G - 1) / G;
    int32_t guess = (int32_t)std::min<int64_t>(1 << 20, std::max<int64_t>(64, 2 * per_graph / std::max(1, n * lg) + 16));
    HGX_TRY(ensure_round_cap(guess));
    return hipStreamSynchronize(stream);
}

hipError_t Engine::ensure_round_cap(int32_t need) {
    if (need <= r_cap) return hipSuccess;
    const int32_t old = r_cap;
    int32_t nc = std::max<int32_t>(need, old * 2);
    const size_t Cz = (size_t)C;
    HGX_TRY(Bm.grow_copy((size_t)(nc + 1) * Cz, (size_t)(old + 1) * Cz, stream));
    HGX_TRY(WLA.grow_copy((size_t)nc * Cz * n, (size_t)old * Cz * n, stream));
    HGX_TRY(WFD.grow_copy((size_t)nc * Cz * n, (size_t)old * Cz * n, stream));
    HGX_TRY(wflag.grow_copy((size_t)nc * Cz, (size_t)old * Cz, stream));
    HGX_TRY(wstat.grow_copy((size_t)nc * Cz, (size_t)old * Cz, stream));
    drop_step_graph();
    HGX_TRY(wcoin.grow_copy((size_t)nc * Cz, (size_t)old * Cz, stream));
    HGX_TRY(active.grow_copy((size_t)nc + 1, (size_t)old + 1, stream));
    HGX_TRY(ovf.grow_copy((size_t)nc + 2, (size_t)old + 2, stream));
    HGX_TRY(Tthr.grow_copy((size_t)nc * Cz, 0, stream));
    HGX_TRY(fw.grow_copy((size_t)nc * Cz, 0, stream));
    HGX_TRY(elig.grow_copy((size_t)nc * G, 0, stream));
    HGX_TRY(ur_empty.grow_copy((size_t)G, 0, stream));
    // S rows of earlier rounds were written by the round steps of this DivideRounds (the
    // growth happens between step batches) and are read by DecideFame: keep them
    HGX_TRY(Smat.grow_copy((size_t)nc * Cz * nw, (size_t)old * Cz * nw, stream));
    HGX_TRY(Vbuf.grow_copy((size_t)nc * 2 * Cz * nw, 0, stream));
    HGX_TRY(fame.grow_copy((size_t)nc * Cz, 0, stream));
    HGX_TRY(blk_cnt.grow_copy((size_t)nc * G, 0, stream));
    HGX_TRY(blk_loaded.grow_copy((size_t)nc * G, 0, stream));
    HGX_TRY(blk_ntx.grow_copy((size_t)nc * G, 0, stream));
    HGX_TRY(blk_nil.grow_copy((size_t)nc * G, 0, stream));
    if (old < nc) {
        HGX_TRY(hipMemsetAsync(active.p + old + 1, 0, (size_t)(nc - old) * sizeof(int32_t), stream));
        HGX_TRY(hipMemsetAsync(ovf.p + old + 2, 0, (size_t)(nc - old) * sizeof(int32_t), stream));
    }
    r_cap = nc;
    return hipSuccess;
}

DevArrays Engine::arrays() {
    DevArrays a;
    a.g_creator = g_creator.p; a.g_index = g_index.p; a.g_op = g_op.p; a.g_ntx = g_ntx.p;
    a.g_ts = g_ts.p; a.g_S = g_S.p; a.g_coin = g_coin.p; a.g_loaded = g_loaded.p; a.g_txnil = g_txnil.p;
    a.g_rr = g_rr.p; a.g_pos = g_pos.p; a.g_cts = g_cts.p; a.g_ck = g_ck.p;
    a.c_off = c_off.p; a.c_len = c_len.p; a.c_base = c_base.p;
    a.p_gid = p_gid.p; a.p_chain = p_chain.p; a.p_op = p_op.p; a.p_opu = p_opu.p; a.p_opk = p_opk.p; a.p_round = p_round.p; a.p_rr = p_rr.p;
    a.p_ts = p_ts.p; a.p_cts = p_cts.p;
    a.LA = LA.p; a.FDT = FDT.p; a.compact = compact;
    a.Bm = Bm.p; a.wflag = wflag.p; a.wstat = wstat.p; a.wcoin = wcoin.p; a.WLA = WLA.p; a.WFD = WFD.p; a.WLAT = WLAT.p;
    a.active = active.p; a.lr = lr.p;
    a.Smat = Smat.p; a.Vbuf = Vbuf.p; a.fame = fame.p;
    a.elig = elig.p; a.fw = fw.p; a.ur_empty = ur_empty.p; a.T = Tthr.p;
    a.recv_list = recv_list.p; a.counters = counters.p; a.fu = fu.p; a.rcnt = rcnt.p; a.scan_part = scan_part.p;
    a.key_a = key_a.p; a.key_b = key_b.p; a.val_a = val_a.p; a.val_b = val_b.p; a.hist = hist.p;
    a.minmax = minmax.p; a.order_gid = order_gid.p;
    a.blk_cnt = blk_cnt.p; a.blk_loaded = blk_loaded.p; a.blk_ntx = blk_ntx.p; a.blk_nil = blk_nil.p;
    return a;
}

// ---- per-kernel timing (only when time_kernels) ---------------------------------
// count = launches the window covers (a hipGraph replay of round steps); sample = false
// counts them without timing (a per-launch average from the timed sample: KernelStat.timed)
// HGX_HOST_TIME_KERNELS=1 (diagnostic): every timed window also drained and timed by the host clock,
// one stderr line per window (a cross-check of the HIP-event and profiler kernel times)
static const bool g_host_time = getenv("HGX_HOST_TIME_KERNELS") != nullptr;
static std::chrono::steady_clock::time_point g_host_t0;

void Engine::kbeg(int k, bool sample, int64_t count) {
    kstat[k].launches += count;
    if (!((time_mask >> k) & 1u) || !sample) return;
    if (g_host_time) {
        (void)hipStreamSynchronize(stream);
        g_host_t0 = std::chrono::steady_clock::now();
    }
    while (kev.size() < kev_used + 2) {
        hipEvent_t e;
        // timing only (nothing on the host waits on them): no system-scope fences, so that the
        // events bracketing every round-step replay cost the timed region as little as possible
        if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) return;
        kev.push_back(e);
    }
    (void)hipEventRecord(kev[kev_used], stream);
    kopen.push_back({k, kev_used, 0, count});
    kev_used += 2;
}

void Engine::kend(int k, double bytes) {
    kstat[k].bytes += bytes;
    if (!((time_mask >> k) & 1u) || kopen.empty() || kopen.back().k != k) return;
    Open& o = kopen.back();
    o.bytes = bytes;
    (void)hipEventRecord(kev[o.e0 + 1], stream);
    if (g_host_time) {
        (void)hipStreamSynchronize(stream);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - g_host_t0).count();
        float ev = 0.f;
        (void)hipEventElapsedTime(&ev, kev[o.e0], kev[o.e0 + 1]);
        fprintf(stderr, "[hgx host-timed] kernel %d host %.4f ms events %.4f ms\n", k, ms, (double)ev);
    }
}

// bytes known only after the launch completed (attributed to the last open launch of k)
void Engine::kadd_bytes(int k, double bytes) {
    kstat[k].bytes += bytes;
    for (auto it = kopen.rbegin(); it != kopen.rend(); ++it)
        if (it->k == k) { it->bytes += bytes; break; }
}

hipError_t Engine::stage_reserve(size_t bytes) {
    const size_t need = stage_used + ((bytes + 63) & ~(size_t)63);
    if (need <= stage_cap) return hipSuccess;
    // grow: nothing staged may still be in flight, and staged D2H data is copied out first
    HGX_TRY(hipStreamSynchronize(stream));
    size_t cap = std::max(need, std::max((size_t)1 << 20, 2 * stage_cap));
    uint8_t* q = nullptr;
    HGX_TRY(hipHostMalloc((void**)&q, cap, hipHostMallocDefault));
    if (h_stage) {
        std::memcpy(q, h_stage, stage_used);
        (void)hipHostFree(h_stage);
    }
    h_stage = q;
    stage_cap = cap;
    return hipHostGetDevicePointer((void**)&d_stage, h_stage, 0);
}

hipError_t Engine::stage_h2d(void* dev, const void* host, size_t bytes) {
    if (bytes == 0) return hipSuccess;
    HGX_TRY(stage_reserve(bytes));
    std::memcpy(h_stage + stage_used, host, bytes);
    pend.push_back({0, stage_used, dev, nullptr, nullptr, bytes});
    stage_used += (bytes + 63) & ~(size_t)63;
    return hipSuccess;
}

hipError_t Engine::stage_d2h(void* host, const void* dev, size_t bytes) {
    if (bytes == 0) return hipSuccess;
    HGX_TRY(stage_reserve(bytes));
    stage_out.push_back({host, stage_used, bytes});
    pend.push_back({1, stage_used, dev, nullptr, nullptr, bytes});
    stage_used += (bytes + 63) & ~(size_t)63;
    return hipSuccess;
}

hipError_t Engine::copy_to_pinned(void* pinned_dst, const void* dev, size_t bytes, int reset) {
    if (bytes == 0) return hipSuccess;
    void* d = nullptr;
    HGX_TRY(hipHostGetDevicePointer(&d, pinned_dst, 0));
    PendCopy p{2, 0, dev, pinned_dst, d, bytes};
    p.reset = reset;
    pend.push_back(p);
    return hipSuccess;
}

hipError_t Engine::copy_from_pinned(void* dev, const void* pinned_src, size_t bytes) {
    if (bytes == 0) return hipSuccess;
    void* d = nullptr;
    HGX_TRY(hipHostGetDevicePointer(&d, const_cast<void*>(pinned_src), 0));
    PendCopy p{3, 0, dev, nullptr, nullptr, bytes};
    p.host_src = pinned_src;
    p.dev_src = d;
    pend.push_back(p);
    return hipSuccess;
}

hipError_t Engine::stage_issue() {
    if (pend.empty()) return hipSuccess;
    size_t total = 0;
    for (const PendCopy& p : pend) total += p.bytes;
    if (pend.size() <= (size_t)kCopyMax && total <= kCopyKernelMax) {
        CopyRange r[kCopyMax];
        int k = 0;
        for (const PendCopy& p : pend) {
            if (p.kind == 0) r[k++] = {d_stage + p.off, const_cast<void*>(p.dev), (uint32_t)p.bytes};
            else if (p.kind == 1) r[k++] = {p.dev, d_stage + p.off, (uint32_t)p.bytes};
            else if (p.kind == 2) r[k++] = {p.dev, p.dev_dst, (uint32_t)p.bytes, p.reset};
            else r[k++] = {p.dev_src, const_cast<void*>(p.dev), (uint32_t)p.bytes};
        }
        launch_copy_many(stream, r, k);
        pend.clear();
        return hipGetLastError();
    }
    for (const PendCopy& p : pend) {
        if (p.kind == 0) HGX_TRY(hipMemcpyAsync(const_cast<void*>(p.dev), h_stage + p.off, p.bytes, hipMemcpyHostToDevice, stream));
        else if (p.kind == 1) HGX_TRY(hipMemcpyAsync(h_stage + p.off, p.dev, p.bytes, hipMemcpyDeviceToHost, stream));
        else if (p.kind == 2) {
            HGX_TRY(hipMemcpyAsync(p.host_dst, p.dev, p.bytes, hipMemcpyDeviceToHost, stream));
            if (p.reset >= 0) HGX_TRY(hipMemsetAsync(const_cast<void*>(p.dev), p.reset, p.bytes, stream));
        }
        else HGX_TRY(hipMemcpyAsync(const_cast<void*>(p.dev), p.host_src, p.bytes, hipMemcpyHostToDevice, stream));
    }
    pend.clear();
    return hipSuccess;
}

void Engine::stage_flush() {
    for (const StagedD2H& d : stage_out) std::memcpy(d.dst, h_stage + d.off, d.bytes);
    stage_out.clear();
    stage_used = 0;
}

hipError_t Engine::collect_kernel_times() {
    if (kopen.empty()) return hipSuccess;
    HGX_TRY(hipStreamSynchronize(stream));
    for (const Open& o : kopen) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, kev[o.e0], kev[o.e0 + 1]) == hipSuccess) {
            kstat[o.k].ms += ms;
            kstat[o.k].timed += o.count;
        }
    }
    kopen.clear();
    kev_used = 0;
    return hipSuccess;
}

// ---- inputs: InsertEvent batches (hgx_insert.hip) ----------------------------------
InsertState Engine::insert_state() {
    InsertState st;
    st.g_creator = g_creator.p; st.g_index = g_index.p; st.g_sp = g_sp.p; st.g_op = g_op.p; st.g_ntx = g_ntx.p;
    st.g_rr = g_rr.p; st.g_ts = g_ts.p; st.g_cts = g_cts.p; st.g_S = g_S.p; st.g_coin = g_coin.p;
    st.g_loaded = g_loaded.p; st.g_txnil = g_txnil.p; st.g_id = g_id.p;
    st.succ = succ.p; st.first_none = first_none.p;
    st.last_gid = last_gid_d.p; st.last_index = last_index_d.p; st.chain_base = chain_base_d.p;
    st.fail = ins_fail.p; st.graph_loaded = graph_loaded_d.p;
    st.root_y_ext = root_y_ext_d.p; st.rooted = rooted ? 1 : 0;
    st.others = others_d.p; st.n_others = n_others; st.others_trust = others_trust ? 1 : 0;
    return st;
}

template <typename T>
static hipError_t reserve_bytes(DBuf<T>& b, size_t bytes, void*& p) {
    if (b.n < bytes / sizeof(T)) HGX_TRY(b.alloc(bytes / sizeof(T)));
    p = b.p;
    return hipSuccess;
}

hipError_t Engine::stage_buf(ColId id, size_t bytes, void*& p) {
    switch (id) {
        case kColCreator: return reserve_bytes(st_creator, bytes, p);
        case kColIndex: return reserve_bytes(st_index, bytes, p);
        case kColSp: return reserve_bytes(st_sp, bytes, p);
        case kColOp: return reserve_bytes(st_op, bytes, p);
        case kColTs: return reserve_bytes(st_ts, bytes, p);
        case kColHash: return reserve_bytes(st_hash, bytes, p);
        case kColS: return reserve_bytes(st_S, bytes, p);
        case kColNtx: return reserve_bytes(st_ntx, bytes, p);
        case kColNil: return reserve_bytes(st_nil, bytes, p);
        case kColIndex32: return reserve_bytes(st_index32, bytes, p);
        case kColSp32: return reserve_bytes(st_sp32, bytes, p);
        case kColOp32: return reserve_bytes(st_op32, bytes, p);
        case kColCoin: return reserve_bytes(st_coin, bytes, p);
        case kColCreator16: return reserve_bytes(st_c16, bytes, p);
        case kColSpBack: return reserve_bytes(st_spb, bytes, p);
        case kColOpBack: return reserve_bytes(st_opb, bytes, p);
        case kColExcPos: return reserve_bytes(st_exc_pos, bytes, p);
        case kColExcSp: return reserve_bytes(st_exc_sp, bytes, p);
        case kColExcOp: return reserve_bytes(st_exc_op, bytes, p);
        default: return hipErrorInvalidValue;
    }
}

// the InsertIn field of a column staged at p (the packed structure has none: it is decoded first)
static void set_col(InsertIn& in, ColId id, const void* p) {
    switch (id) {
        case kColCreator: in.creator = (const int32_t*)p; break;
        case kColIndex: in.index = (const int64_t*)p; break;
        case kColSp: in.sp = (const int64_t*)p; break;
        case kColOp: in.op = (const int64_t*)p; break;
        case kColTs: in.ts = (const int64_t*)p; break;
        case kColHash: in.hash = (const uint8_t*)p; break;
        case kColS: in.S = (const uint8_t*)p; break;
        case kColNtx: in.ntx = (const int32_t*)p; break;
        case kColNil: in.nil = (const int32_t*)p; break;
        case kColIndex32: in.index32 = (const int32_t*)p; break;
        case kColSp32: in.sp32 = (const int32_t*)p; break;
        case kColOp32: in.op32 = (const int32_t*)p; break;
        case kColCoin: in.coin = (const uint8_t*)p; break;
        default: break;
    }
}

// a sync-sized batch (at most kPackEvents): the host columns packed into pinned memory and sent as
// one copy into st_pack (a pageable copy per column costs a staged, blocking transfer each); off[i] =
// byte offset in st_pack of the form's column i
hipError_t Engine::stage_pinned(const HostCols& hc, int64_t count, size_t* off) {
    const FormSpec& fs = form_spec(hc.form);
    const size_t total = one_copy_layout(fs, count, hc.n_exc, off);
    if (st_pack.n < total) HGX_TRY(st_pack.alloc(std::max(total, (size_t)2 * st_pack.n)));
    if (h_pack_cap < total) {   // (every insert synchronized before returning: the buffer is free)
        if (h_pack) (void)hipHostFree(h_pack);
        h_pack = nullptr;
        h_pack_cap = 0;
        HGX_TRY(hipHostMalloc((void**)&h_pack, std::max(total, (size_t)2 * st_pack.n), hipHostMallocDefault));
        h_pack_cap = std::max(total, (size_t)2 * st_pack.n);
    }
    for (int i = 0; i < fs.n; i++)
        if (const size_t bytes = col_bytes(fs.col[i], count, hc.n_exc))
            std::memcpy(h_pack + off[i], hc.col[fs.col[i].id], bytes);
    return hipMemcpyAsync(st_pack.p, h_pack, total, hipMemcpyHostToDevice, stream);
}

hipError_t Engine::stage(const HostCols& hc, int64_t count, StagePart part, InsertIn& in) {
    const FormSpec& fs = form_spec(hc.form);
    const bool packed = hc.form == Form::packed, one_copy = part == kStageAll && count <= kPackEvents;
    const void* at[kNumCols] = {};   // where each column landed
    void* p = nullptr;
    in = InsertIn{};
    if (packed) {   // the decoded columns
        HGX_TRY(stage_buf(kColCreator, (size_t)count * 4, p));
        HGX_TRY(stage_buf(kColSp32, (size_t)count * 4, p));
        HGX_TRY(stage_buf(kColOp32, (size_t)count * 4, p));
    }
    // a copy per column: the structure in the table's order, the payload (behind the decode) in the
    // order of a batch staged whole, S into the staging with the rest
    auto copy_cols = [&](bool payload) {
        for (int k = 0; k < fs.n; k++) {
            const ColSpec& cs = fs.col[payload ? fs.whole[k] : k];
            if (is_payload(cs) != payload) continue;
            const size_t bytes = col_bytes(cs, count, hc.n_exc);
            HGX_TRY(stage_buf(cs.id, bytes, p));
            at[cs.id] = p;
            if (bytes || cs.kind != kColException)
                HGX_TRY(hipMemcpyAsync(p, hc.col[cs.id], bytes, hipMemcpyHostToDevice, stream));
        }
        return hipSuccess;
    };
    if (one_copy) {
        size_t off[kMaxFormCols];
        HGX_TRY(stage_pinned(hc, count, off));
        for (int i = 0; i < fs.n; i++) at[fs.col[i].id] = st_pack.p + off[i];
    } else {
        HGX_TRY(copy_cols(false));
    }
    if (packed) {
        launch_unpack_packed(stream, count, E, (const uint16_t*)at[kColCreator16], (const uint16_t*)at[kColSpBack],
                             (const uint16_t*)at[kColOpBack], hc.n_exc, (const int64_t*)at[kColExcPos],
                             (const int32_t*)at[kColExcSp], (const int32_t*)at[kColExcOp], st_creator.p, st_sp32.p,
                             st_op32.p);
        HGX_TRY(hipGetLastError());
        at[kColCreator] = st_creator.p; at[kColSp32] = st_sp32.p; at[kColOp32] = st_op32.p;
    }
    if (part == kStageAll && !one_copy) HGX_TRY(copy_cols(true));
    for (int id = 0; id < kNumCols; id++)
        if (at[id]) set_col(in, (ColId)id, at[id]);
    // (an insert of compact columns brings the coin byte, not the event's id)
    if (part == kStageAll && hc.form != Form::wide && count > 0) ids_known = false;
    return hipSuccess;
}

hipError_t Engine::set_keys(const uint8_t* keys65) {
    HGX_TRY(pk_keys.alloc((size_t)C * 65 + 1));
    HGX_TRY(pk_valid.alloc((size_t)C + 1));
    HGX_TRY(pk_tab.alloc(p256_table_bytes(C) / 4 + 1));
    HGX_TRY(hipMemcpyAsync(pk_keys.p, keys65, (size_t)C * 65, hipMemcpyHostToDevice, stream));
    launch_p256_tables(stream, C, pk_keys.p, pk_tab.p, pk_valid.p);
    HGX_TRY(hipGetLastError());
    HGX_TRY(hipStreamSynchronize(stream));
    keys_set = true;
    return wipe_signing_keys();   // (signing keys were checked against the keys this call replaced)
}

hipError_t Engine::wipe_signing_keys() {
    sign_keys_set = false;
    sign_has.clear();
    if (sk_keys.p) {
        HGX_TRY(hipMemsetAsync(sk_keys.p, 0, sk_keys.n, stream));
        HGX_TRY(hipStreamSynchronize(stream));
        sk_keys.release();
    }
    return hipSuccess;
}

hipError_t Engine::set_signing_keys(const uint8_t* priv32, int32_t* mismatch) {
    *mismatch = -1;
    if (!priv32) return wipe_signing_keys();
    if (!keys_set) return hipErrorNotReady;
    const size_t nc = (size_t)C;
    DBuf<uint8_t> fresh, pub;
    struct Wipe {   // the candidate copy never outlives this call unzeroed
        DBuf<uint8_t>& b;
        hipStream_t s;
        ~Wipe() {
            if (!b.p) return;
            (void)hipMemsetAsync(b.p, 0, b.n, s);
            (void)hipStreamSynchronize(s);
        }
    } wipe{fresh, stream};
    HGX_TRY(fresh.alloc(32 * nc));
    HGX_TRY(pub.alloc(65 * nc));
    std::vector<uint8_t> want(65 * nc), got(65 * nc);
    HGX_TRY(hipMemcpyAsync(fresh.p, priv32, 32 * nc, hipMemcpyHostToDevice, stream));
    // d G beside the participant's key (a participant without a signing key keeps its own row)
    HGX_TRY(hipMemcpyAsync(pub.p, pk_keys.p, 65 * nc, hipMemcpyDeviceToDevice, stream));
    launch_p256_pub(stream, C, fresh.p, pk_tab.p + nc * kP256TabWords, pub.p);
    HGX_TRY(hipGetLastError());
    HGX_TRY(hipMemcpyAsync(got.data(), pub.p, 65 * nc, hipMemcpyDeviceToHost, stream));
    HGX_TRY(hipMemcpyAsync(want.data(), pk_keys.p, 65 * nc, hipMemcpyDeviceToHost, stream));
    HGX_TRY(hipStreamSynchronize(stream));
    for (size_t c = 0; c < nc; c++)
        if (std::memcmp(&got[65 * c], &want[65 * c], 65) != 0) {
            *mismatch = (int32_t)c;
            return hipSuccess;
        }
    HGX_TRY(wipe_signing_keys());
    sk_keys.p = fresh.p;
    sk_keys.n = fresh.n;
    fresh.p = nullptr;
    fresh.n = 0;
    sign_has.assign(nc, 0);
    for (size_t c = 0; c < nc; c++)
        for (int j = 0; j < 32; j++) sign_has[c] |= priv32[32 * c + j] != 0;
    sign_keys_set = true;
    return hipSuccess;
}

hipError_t Engine::stage_sig(const uint8_t* digest, const uint8_t* r, int64_t count, const uint8_t** d_digest,
                             const uint8_t** d_r) {
    const size_t c = (size_t)count * 32;
    if (st_dig.n < c) HGX_TRY(st_dig.alloc(c));
    if (st_r.n < c) HGX_TRY(st_r.alloc(c));
    if (c) {
        HGX_TRY(hipMemcpyAsync(st_dig.p, digest, c, hipMemcpyHostToDevice, stream));
        HGX_TRY(hipMemcpyAsync(st_r.p, r, c, hipMemcpyHostToDevice, stream));
    }
    *d_digest = st_dig.p;
    *d_r = st_r.p;
    return hipSuccess;
}

hipError_t Engine::insert_verified(const InsertIn& in, const uint8_t* digest, const uint8_t* r, int64_t count,
                                   InsertOut& out, bool fail_armed) {
    if (!keys_set) return hipErrorNotReady;
    if (count > 0) {
        if (pk_out.n < (size_t)count) HGX_TRY(pk_out.alloc((size_t)count));
        if (!fail_armed) {
            if (ins_fail_sig.n < 1) HGX_TRY(ins_fail_sig.alloc(1));
            HGX_TRY(hipMemsetAsync(ins_fail_sig.p, 0xFF, 8, stream));
        }
        // Event.Verify of the whole batch (hgx_p256.hip; key = the creator's), then its first failure
        launch_p256_verify(stream, count, C, in.creator, digest, r, in.S, pk_tab.p, pk_valid.p, pk_out.p);
        launch_insert_sig_first(stream, count, C, in.creator, pk_out.p, ins_fail_sig.p);
        HGX_TRY(hipGetLastError());
    }
    HGX_TRY(insert_impl(in, count, out, count > 0 ? ins_fail_sig.p : nullptr));
    return idx_kept ? idx_append() : hipSuccess;   // (the body paths' chunks: the id index follows each)
}

hipError_t Engine::insert(const InsertIn& in, int64_t count, InsertOut& out) {
    HGX_TRY(insert_impl(in, count, out, nullptr));
    // the id index follows the commit in a launch of its own (nothing on a context that keeps none, or
    // whose ids are not known). A split insert (hgx_insert_and_run) does not pass here: its events are
    // indexed by the next call that goes through here or that reads the index.
    return idx_kept ? idx_append() : hipSuccess;
}

hipError_t Engine::insert_split_begin(const HostCols& hc, int64_t count, InsertOut& out) {
    InsertIn in;
    HGX_TRY(stage(hc, count, kStageStructure, in));   // (no payload yet)
    flight = hc.form == Form::wide ? kFlightWide : kFlightCompact;
    return insert_impl(in, count, out, nullptr, kCommitStructure);
}

hipError_t Engine::payload_streams() {
    if (!stream2) {
        HGX_TRY(hipStreamCreateWithFlags(&stream2, hipStreamNonBlocking));
        HGX_TRY(hipEventCreateWithFlags(&ev_pay, hipEventDisableTiming));
    }
    if (!ev_pay_S) HGX_TRY(hipEventCreateWithFlags(&ev_pay_S, hipEventDisableTiming));
    return hipSuccess;
}

// The payload columns of events [E0, E0 + c) on stream2: the first stage into the staging columns and
// ev_pay (pay_stage = 1 releases payload_commit), then the late stage (S of the compact payload)
// straight into the event store and ev_pay_S.
hipError_t Engine::copy_payload(const HostCols& hc, size_t c, size_t E0, hipError_t e, const std::atomic<int>* stop) {
    const FormSpec& fs = form_spec(hc.form);
    auto go = [&]() { return c && e == hipSuccess && !(stop && stop->load(std::memory_order_acquire)); };
    bool late = false;
    void* p = nullptr;
    for (int i = 0; i < fs.n; i++) {
        const ColSpec& cs = fs.col[i];
        late |= cs.kind == kColPayloadLate;
        if (cs.kind != kColPayload || !go()) continue;
        e = stage_buf(cs.id, 0, p);   // (sized by the caller)
        if (e == hipSuccess) e = hipMemcpyAsync(p, hc.col[cs.id], c * cs.bytes, hipMemcpyHostToDevice, stream2);
    }
    if (e == hipSuccess) e = hipEventRecord(ev_pay, stream2);
    pay_err_a = e;
    pay_stage.store(1, std::memory_order_release);
    if (late) {
        if (go()) e = hipMemcpyAsync(g_S.p + 32 * E0, hc.col[kColS], c * 32, hipMemcpyHostToDevice, stream2);
        if (e == hipSuccess) e = hipEventRecord(ev_pay_S, stream2);
    }
    const hipError_t es = hipStreamSynchronize(stream2);   // the caller's buffers are read completely
    return e != hipSuccess ? e : es;
}

hipError_t Engine::payload_begin(const HostCols& hc, int64_t m_ok) {
    HGX_TRY(payload_streams());
    const FormSpec& fs = form_spec(hc.form);
    const size_t c = (size_t)m_ok;   // the accepted prefix only (just appended): gids E - m_ok ..
    bool late = false;
    void* p = nullptr;
    for (int i = 0; i < fs.n; i++) {
        late |= fs.col[i].kind == kColPayloadLate;
        if (fs.col[i].kind == kColPayload) HGX_TRY(stage_buf(fs.col[i].id, c * fs.col[i].bytes, p));
    }
    if (pay_thread.joinable()) pay_thread.join();
    pay_err = hipSuccess;
    pay_stage = 0;
    pay_S_pending = late;
    pay_commit_pending = true;
    pay_E0 = E - m_ok;
    pay_m = m_ok;
    pay_host_ms = 0;
    if (hc.form != Form::wide && m_ok > 0) ids_known = false;
    // pageable host memory: each copy returns once its source has been consumed, so the copies
    // run on their own host thread (and stream) beside the DivideRounds launches
    pay_thread = std::thread([this, hc, c, E0 = (size_t)pay_E0]() { pay_err = copy_payload(hc, c, E0, hipSetDevice(dev), nullptr); });
    return hipSuccess;
}

namespace {
struct HostTimer {   // adds the scope's host wall clock to a counter
    double& acc;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    explicit HostTimer(double& a) : acc(a) {}
    ~HostTimer() { acc += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};
}  // namespace

hipError_t Engine::payload_commit(bool positions, hipStream_t on) {
    if (!on) on = stream;
    if (!pay_commit_pending) return hipSuccess;
    HostTimer tm(pay_host_ms);
    pay_commit_pending = false;
    if (pay_S_pending) {   // the compact payload: its first stage only (S lands in g_S later)
        while (pay_stage.load(std::memory_order_acquire) == 0) std::this_thread::yield();
        HGX_TRY(pay_err_a);
    } else {
        if (pay_thread.joinable()) pay_thread.join();
        HGX_TRY(pay_err);
    }
    HGX_TRY(hipStreamWaitEvent(on, ev_pay, 0));
    // the staging columns of the batch in flight (without the late S: it lands in the store itself)
    InsertIn in{};
    const FormSpec& fs = form_spec(flight == kFlightWide ? Form::wide : Form::compact);
    void* p = nullptr;
    for (int i = 0; i < fs.n; i++)
        if (fs.col[i].kind != kColPayloadLate) {
            HGX_TRY(stage_buf(fs.col[i].id, 0, p));
            set_col(in, fs.col[i].id, p);
        }
    flight = kFlightNone;
    launch_insert_commit(on, pay_m, nullptr, nullptr, pay_E0, n, in, insert_state(), kCommitPayload);
    // (the layout ran before the timestamps were committed)
    if (positions) launch_ts_to_pos(on, pay_E0, pay_m, g_pos.p, g_ts.p, p_ts.p);
    return hipGetLastError();
}

hipError_t Engine::payload_finish(bool laid_out_new, int32_t wcoin_r0) {
    if (pay_commit_pending) {
        HGX_TRY(payload_commit(laid_out_new));
        HostTimer tm(pay_host_ms);
        // the rounds' coin pass read the coins before they were committed
        if (laid_out_new && R > wcoin_r0) launch_wcoin(stream, arrays(), wcoin_r0, R, C);
        HGX_TRY(hipGetLastError());
    }
    HostTimer tm(pay_host_ms);
    return hipMemcpyAsync(h_ins, ins_blk.p, ins_blk.n * sizeof(int32_t), hipMemcpyDeviceToHost, stream);
}

void Engine::payload_loaded(std::vector<uint64_t>& loaded) const {
    loaded.resize(G);
    std::memcpy(loaded.data(), h_ins + ins_gl_off, (size_t)G * 8);
}

hipError_t Engine::payload_wait_S() {
    if (!pay_S_pending) return hipSuccess;
    pay_S_pending = false;
    if (pay_thread.joinable()) pay_thread.join();
    HGX_TRY(pay_err);
    return hipStreamWaitEvent(stream, ev_pay_S, 0);
}

hipError_t Engine::insert_impl(const InsertIn& in, int64_t count, InsertOut& out, const unsigned long long* fail_sig,
                               int commit_mode) {
    out = InsertOut();
    const int64_t E0 = E;
    pipe_ready = false;
    InsertState st = insert_state();
    if (count > 0) {
        // checks, then the commit of the accepted prefix and the withdrawal of the rest's claims:
        // the kernels take the prefix from the first-failure words, so the batch costs one host
        // round trip (the chunked schedule inserts 1 000 events per call)
        // (ins_fail is ~0 here: set at creation, re-armed by the read-back below)
        if (!launch_insert_fused(stream, count, fail_sig, E0, cap, C, n, in, st, commit_mode)) {
            launch_insert_claim(stream, count, E0, cap, C, in, st);
            launch_insert_check(stream, count, E0, cap, C, n, in, st);
            launch_insert_commit(stream, count, ins_fail.p, fail_sig, E0, n, in, st, commit_mode);
            launch_insert_unclaim(stream, count, ins_fail.p, fail_sig, E0, cap, C, in, st);
        }
        HGX_TRY(copy_to_pinned(h_small + kHsInsFail, ins_fail.p, 8, 0xFF));
        if (fail_sig) HGX_TRY(copy_to_pinned(h_small + kHsInsFailSig, fail_sig, 8));
    }
    // the first-failure words and the whole state block into pinned memory (one launch), then
    // the host mirrors
    HGX_TRY(copy_to_pinned(h_ins, ins_blk.p, ins_blk.n * sizeof(int32_t)));
    HGX_TRY(stage_issue());
    HGX_TRY(hipStreamSynchronize(stream));
    if (count > 0) {
        unsigned long long fail = 0, fsig = ~0ull;
        std::memcpy(&fail, h_small + kHsInsFail, 8);
        if (fail_sig) std::memcpy(&fsig, h_small + kHsInsFailSig, 8);
        // Verify comes first in InsertEvent: at the same event the signature's failure wins
        // (the kernels' accepted_prefix)
        if ((fsig >> 8) <= (fail >> 8) && fsig != ~0ull) fail = fsig;
        const int64_t m_ok = (fail == ~0ull) ? count : (int64_t)(fail >> 8);
        out.accepted = m_ok;
        out.code = (fail == ~0ull) ? 0 : (int)(fail & 0xFF);
        if (out.code) {   // the failing event's creator and Index for the error string
            HGX_TRY(hipMemcpyAsync(&out.fail_creator, in.creator + m_ok, 4, hipMemcpyDeviceToHost, stream));
            if (in.index32) {
                int32_t fi = 0;
                HGX_TRY(hipMemcpyAsync(&fi, in.index32 + m_ok, 4, hipMemcpyDeviceToHost, stream));
                HGX_TRY(hipStreamSynchronize(stream));
                out.fail_index = fi;
            } else {
                HGX_TRY(hipMemcpyAsync(&out.fail_index, in.index + m_ok, 8, hipMemcpyDeviceToHost, stream));
            }
            HGX_TRY(hipStreamSynchronize(stream));
        }
        E = E0 + m_ok;
    }
    read_insert_state(out);
    return hipSuccess;
}

void Engine::read_insert_state(InsertOut& out) const {
    out.last_gid.assign(h_ins, h_ins + C);
    out.last_index.assign(h_ins + C, h_ins + 2 * C);
    out.chain_base.assign(h_ins + 2 * C, h_ins + 3 * C);
    out.graph_loaded.resize(G);
    std::memcpy(out.graph_loaded.data(), h_ins + ins_gl_off, (size_t)G * 8);
}

hipError_t Engine::clear() {
    HGX_TRY(payload_wait_S());
    if (E > 0) HGX_TRY(hipMemsetAsync(succ.p, 0xFF, (size_t)E * 4, stream));
    HGX_TRY(hipMemsetAsync(first_none.p, 0xFF, (size_t)C * 4, stream));
    HGX_TRY(hipMemsetAsync(last_gid_d.p, 0xFF, (size_t)C * 8, stream));   // last_gid, last_index
    HGX_TRY(hipMemsetAsync(chain_base_d.p, 0, (ins_blk.n - (size_t)2 * C) * 4, stream));   // chain_base, graph_loaded
    E = 0;
    E_div = 0;
    R = 0;
    laid_out = false;
    ids_known = true;
    pipe_ready = false;
    HGX_TRY(bodies_reset());   // (nothing queued on a context that keeps no bodies)
    HGX_TRY(idx_zero());       // (nor on one that keeps no id index)
    return hipStreamSynchronize(stream);
}

// ---- the pipelined ingest --------------------------------------------------
hipError_t Engine::insert_pipe32(const HostCols& hc, int64_t count, InsertOut& out, bool& taken) {
    taken = false;
    pipe_used = 0;
    if (pipe_pieces <= 0 || count < pipe_min || count < 2 || count > cap || E != 0 || rooted || G != 1 || grp ||
        time_mask != 0 || la_kernel != 0 || n > 896)
        return hipSuccess;
    // the plan's guesses, checked against the histogram: compact coordinates when they are allowed
    // and the mean chain fits, and the time segments that follow from them
    const int guess = (!force_coord32 && (n % 2) == 0 && count / C <= 65533) ? 1 : 0;
    // The segments: a segment's pass is bound by its own DAG depth (c3: 3.3 ms for 1 220 rows per
    // chain, alone on the device or beside 31 others), and a serial rebuild takes as many as the CUs
    // hold at once. Here the early pieces' passes run while the later columns are still on the way,
    // so shorter segments shorten the tail behind the last piece: kPipeSegMult times the serial
    // choice, still of at least 2 x kLaHeadRows rows per chain
    const int base = rebuild_segments(count, guess);
    if (base < 2) return hipSuccess;
    const int nts = la_segs_override > 0
                        ? base
                        : std::max(base, (int)std::min<int64_t>((int64_t)kPipeSegMult * base, count / C / (2 * kLaHeadRows)));
    const int pieces = std::min(std::min(pipe_pieces, (int)kPipeMaxPieces), nts);
    int seg_cut[kPipeMaxPieces + 1];
    int64_t cut[kPipeMaxPieces + 1];
    for (int k = 0; k <= pieces; k++) {
        seg_cut[k] = (int)((int64_t)nts * k / pieces);
        cut[k] = count * seg_cut[k] / nts;   // (k_la_wave's segment bounds)
    }
    const size_t c = (size_t)count, Cz = (size_t)C;
    const FormSpec& fs = form_spec(Form::compact);
    void* p = nullptr;
    for (int i = 0; i < fs.n; i++)   // (S goes straight into g_S)
        if (fs.col[i].kind != kColPayloadLate) HGX_TRY(stage_buf(fs.col[i].id, c * fs.col[i].bytes, p));
    const size_t o_hist = 64, o_lim = o_hist + kPipeMaxPieces * Cz;
    if (pipe_buf.n < o_lim + kPipeMaxPieces * Cz) HGX_TRY(pipe_buf.alloc(o_lim + kPipeMaxPieces * Cz));
    HGX_TRY(payload_streams());
    if (!stream_o) {
        HGX_TRY(hipStreamCreateWithFlags(&stream_o, hipStreamNonBlocking));
        for (int k = 0; k <= kOrderParts; k++) HGX_TRY(hipEventCreateWithFlags(&ev_o[k], hipEventDisableTiming));
    }
    if (!stream_p) {
        HGX_TRY(hipStreamCreateWithFlags(&stream_p, hipStreamNonBlocking));
        for (hipEvent_t& e : ev_pc) HGX_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        for (hipEvent_t& e : ev_lay) HGX_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        for (hipEvent_t& e : ev_side) HGX_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    HGX_TRY(payload_wait_S());
    if (pay_thread.joinable()) pay_thread.join();   // (stream2 is free)
    if (pipe_thread.joinable()) pipe_thread.join();
    pipe_err = hipSuccess;
    pipe_stage = 0;
    pipe_stop = 0;
    pay_err = pay_err_a = hipSuccess;
    pay_stage = 0;
    // one copier: the creator column, then index / sp / op piece by piece, an event behind each
    // (a host thread: a copy from pageable memory returns only once its source has been consumed),
    // then the payload as payload_begin's copier (copy_payload; the context is empty: S at gid 0).
    // pipe_stop (a way out of the pipeline) ends it at the next column; what it wrote by then the
    // serial path's own payload copy overwrites.
    std::vector<int64_t> cuts(cut, cut + pieces + 1);
    const int32_t *creator = (const int32_t*)hc.col[kColCreator], *index = (const int32_t*)hc.col[kColIndex32],
                  *sp = (const int32_t*)hc.col[kColSp32], *op = (const int32_t*)hc.col[kColOp32];
    pipe_thread = std::thread([=]() {
        hipError_t e = hipSetDevice(dev);
        if (e == hipSuccess) e = hipMemcpyAsync(st_creator.p, creator, c * 4, hipMemcpyHostToDevice, stream2);
        if (e == hipSuccess) e = hipEventRecord(ev_pc[0], stream2);
        if (e != hipSuccess) pipe_err = e;
        pipe_stage.store(1, std::memory_order_release);
        for (int k = 0; k < pieces; k++) {
            if (pipe_stop.load(std::memory_order_acquire)) break;
            const size_t g0 = (size_t)cuts[k], m = (size_t)(cuts[k + 1] - cuts[k]);
            if (e == hipSuccess) e = hipMemcpyAsync(st_index32.p + g0, index + g0, m * 4, hipMemcpyHostToDevice, stream2);
            if (e == hipSuccess) e = hipMemcpyAsync(st_sp32.p + g0, sp + g0, m * 4, hipMemcpyHostToDevice, stream2);
            if (e == hipSuccess) e = hipMemcpyAsync(st_op32.p + g0, op + g0, m * 4, hipMemcpyHostToDevice, stream2);
            if (e == hipSuccess) e = hipEventRecord(ev_pc[k + 1], stream2);
            if (e != hipSuccess) pipe_err = e;
            pipe_stage.store(k + 2, std::memory_order_release);
        }
        // (pay_err_a / pay_err are read once the pipeline was taken)
        pay_err = copy_payload(hc, c, 0, e, &pipe_stop);
        if (e == hipSuccess && pay_err != hipSuccess) pipe_err = pay_err;
    });
    // every way out joins the copier; `fail` leaves the context empty for the serial path
    auto stop = [&](hipError_t e) {
        pipe_stop.store(1, std::memory_order_release);
        if (pipe_thread.joinable()) pipe_thread.join();
        return e != hipSuccess ? e : pipe_err;
    };
    auto wait_stage = [&](int want) {
        // the event must have been recorded before a stream is made to wait for it
        while (pipe_stage.load(std::memory_order_acquire) < want) std::this_thread::yield();
        return pipe_err;
    };
#define PIPE_TRY(x)                                  \
    do {                                             \
        const hipError_t e_ = (x);                   \
        if (e_ != hipSuccess) return stop(e_);       \
    } while (0)
    int32_t* gate = pipe_buf.p;
    PIPE_TRY(hipMemsetAsync(pipe_buf.p, 0, (o_hist + (size_t)pieces * Cz) * 4, stream));
    PIPE_TRY(wait_stage(1));
    PIPE_TRY(hipStreamWaitEvent(stream, ev_pc[0], 0));
    launch_pipe_hist(stream, pieces, cut, C, st_creator.p, pipe_buf.p + o_hist);
    PIPE_TRY(hipGetLastError());
    pipe_hist.resize((size_t)pieces * Cz);
    PIPE_TRY(hipMemcpyAsync(pipe_hist.data(), pipe_buf.p + o_hist, pipe_hist.size() * 4, hipMemcpyDeviceToHost, stream));
    PIPE_TRY(hipStreamSynchronize(stream));
    // the plan: every chain's rows at the end of each piece, the totals, and what divide_rounds
    // will derive from them (first Index 0 on every chain: k_pipe_check holds the batch to it)
    pipe_lim.assign((size_t)pieces * Cz, 0);
    std::vector<int32_t> len(Cz, 0);
    int64_t known = 0;
    int mlen = 0;
    for (int k = 0; k < pieces; k++)
        for (size_t ch = 0; ch < Cz; ch++) {
            len[ch] += pipe_hist[(size_t)k * Cz + ch];
            pipe_lim[(size_t)k * Cz + ch] = len[ch];
        }
    for (size_t ch = 0; ch < Cz; ch++) {
        known += len[ch];
        mlen = std::max(mlen, len[ch]);
    }
    const int plan_compact = (!force_coord32 && (n % 2) == 0 && mlen - 1 <= 65533) ? 1 : 0;
    if (known != count || plan_compact != guess || !la_wave_ok(n, mlen, n)) {
        PIPE_TRY(stop(hipSuccess));
        return hipSuccess;   // (an unknown creator, or very uneven chains: the serial path)
    }
    compact = plan_compact;
    layout_slots(C, Ppos, count, len.data(), pipe_off);
    std::memcpy(h_cpar, len.data(), Cz * 4);
    std::memset(h_cpar + C, 0, 2 * Cz * 4);   // c_base, c_old
    PIPE_TRY(hipMemcpyAsync(c_off.p, pipe_off.data(), (Cz + 1) * 4, hipMemcpyHostToDevice, stream));
    PIPE_TRY(hipMemcpyAsync(cpar_blk.p, h_cpar, 3 * Cz * 4, hipMemcpyHostToDevice, stream));
    PIPE_TRY(hipMemcpyAsync(pipe_buf.p + o_lim, pipe_lim.data(), pipe_lim.size() * 4, hipMemcpyHostToDevice, stream));
    const DevArrays a = arrays();
    const InsertState st = insert_state();
    for (int k = 0; k < pieces; k++) {
        const int64_t g0 = cut[k], g1 = cut[k + 1];
        PIPE_TRY(wait_stage(k + 2));
        PIPE_TRY(hipStreamWaitEvent(stream, ev_pc[k + 1], 0));
        InsertIn in{};
        in.creator = st_creator.p + g0; in.index32 = st_index32.p + g0; in.sp32 = st_sp32.p + g0; in.op32 = st_op32.p + g0;
        launch_pipe_insert(stream, g1 - g0, g0, cap, C, n, in, st, gate);
        launch_layout(stream, g0, g1, a, C, n, kLaSeg, gate);
        PIPE_TRY(hipGetLastError());
        PIPE_TRY(hipEventRecord(ev_lay[k], stream));
        // the piece's segments, beside the next piece's copy, insert and layout
        hipStream_t side = (k & 1) ? stream_p : stream_o;
        PIPE_TRY(hipStreamWaitEvent(side, ev_lay[k], 0));
        LaSubset sub;
        sub.first = seg_cut[k]; sub.count = seg_cut[k + 1] - seg_cut[k];
        sub.c_lim = pipe_buf.p + o_lim + (size_t)k * Cz; sub.gate = gate;
        PIPE_TRY(launch_la_wave(side, a, 1, n, nullptr, count, nts, 0, counters.p + kCtWaveErr, nullptr, n, false, sub));
    }
    PIPE_TRY(hipEventRecord(ev_side[0], stream_o));
    PIPE_TRY(hipStreamWaitEvent(stream, ev_side[0], 0));
    if (pieces > 1) {
        PIPE_TRY(hipEventRecord(ev_side[1], stream_p));
        PIPE_TRY(hipStreamWaitEvent(stream, ev_side[1], 0));
    }
    // one read-back, as insert_impl: the first-failure word (re-armed) and the state block
    PIPE_TRY(copy_to_pinned(h_small + kHsInsFail, ins_fail.p, 8, 0xFF));
    PIPE_TRY(copy_to_pinned(h_ins, ins_blk.p, ins_blk.n * sizeof(int32_t)));
    PIPE_TRY(stage_issue());
    PIPE_TRY(hipStreamSynchronize(stream));   // (behind every piece's event: the structure columns are read completely)
#undef PIPE_TRY
    unsigned long long fail = 0;
    std::memcpy(&fail, h_small + kHsInsFail, 8);
    if (fail != ~0ull) {
        // a check failed in some piece: stop the copier, empty the context again (the claims of every
        // piece issued so far included) and let the serial path produce the error and the accepted
        // prefix, and copy the payload itself
        HGX_TRY(stop(hipSuccess));
        E = count;
        return clear();
    }
    // the copier runs on as the payload's: payload_commit and payload_wait_S find it as payload_begin's
    pay_thread = std::move(pipe_thread);
    flight = kFlightCompact;
    pay_S_pending = true;
    pay_commit_pending = true;
    pay_E0 = 0;
    pay_m = count;
    pay_host_ms = 0;
    ids_known = false;
    E = count;
    out = InsertOut();
    out.accepted = count;
    read_insert_state(out);
    pipe_ready = true;
    pipe_En = count;
    pipe_nts = nts;
    pipe_compact = plan_compact;
    pipe_used = pieces;
    taken = true;
    return hipSuccess;
}

// ---- hgx_prune_to_frame (hgx_compact.hip) ---------------------------------
// Stage: nothing resident is changed. The kept events' columns are gathered into pr_buf as one
// insert batch (pr_in), and what the host needs comes back: O(kept) gids and Root.Others entries,
// O(C) root parents and ids.
hipError_t Engine::prune_stage(const std::vector<int32_t>& cut, int64_t n_kept, PruneOut& out) {
    out = PruneOut();
    pr_count = -1;
    if ((int)cut.size() != C || n_kept < 0 || n_kept > E || !ids_known) return hipErrorInvalidValue;
    HGX_TRY(payload_wait_S());
    const size_t Ez = (size_t)E, K = (size_t)std::max<int64_t>(n_kept, 1), Cz = (size_t)C;
    const size_t nparts = (Ez + 2047) / 2048 + 1;
    // one block, every part 256-byte aligned
    size_t total = 0;
    auto take = [&](size_t bytes) {
        const size_t off = total;
        total += (bytes + 255) & ~(size_t)255;
        return off;
    };
    const size_t o_scan = take(Ez * 4), o_part = take(nparts * 4), o_cut = take(Cz * 4), o_first = take(Cz * 4),
                 o_cnt = take(8), o_cr = take(K * 4), o_idx = take(K * 4), o_sp = take(K * 4), o_op = take(K * 4),
                 o_ntx = take(K * 4), o_old = take(K * 4), o_ts = take(K * 8), o_hash = take(K * 32),
                 o_S = take(K * 32), o_fsp = take(K * 32), o_fop = take(K * 32), o_fl = take(K), o_fail = take(4),
                 o_on = take(K * 4), o_oo = take(K * 4), o_ok = take(K * 32),
                 o_opid = take(K * 32), o_rsp = take(Cz * 4), o_rop = take(Cz * 4), o_rid = take(Cz * 96);
    if (pr_buf.n < total) HGX_TRY(pr_buf.alloc(total));
    uint8_t* b = pr_buf.p;
    PruneArgs a{};
    a.E = E; a.n_kept = n_kept; a.C = C;
    a.g_creator = g_creator.p; a.g_index = g_index.p; a.g_sp = g_sp.p; a.g_op = g_op.p; a.g_ntx = g_ntx.p;
    a.g_ts = g_ts.p; a.g_S = g_S.p; a.g_id = g_id.p; a.g_txnil = g_txnil.p;
    a.cut = (const int32_t*)(b + o_cut); a.scan = (uint32_t*)(b + o_scan); a.first_gid = (int32_t*)(b + o_first);
    a.kept_total = (uint32_t*)(b + o_cnt); a.oth_count = (uint32_t*)(b + o_cnt) + 1;
    a.st_creator = (int32_t*)(b + o_cr); a.st_index = (int32_t*)(b + o_idx); a.st_sp = (int32_t*)(b + o_sp);
    a.st_op = (int32_t*)(b + o_op); a.st_ntx = (int32_t*)(b + o_ntx); a.old_gid = (int32_t*)(b + o_old);
    a.st_ts = (int64_t*)(b + o_ts); a.st_hash = b + o_hash; a.st_S = b + o_S;
    a.oth_new = (int32_t*)(b + o_on); a.oth_op = (int32_t*)(b + o_oo); a.oth_key = b + o_ok; a.oth_pid = b + o_opid;
    a.root_sp = (int32_t*)(b + o_rsp); a.root_op = (int32_t*)(b + o_rop); a.root_ids = b + o_rid;
    out.old_gid.resize((size_t)n_kept);
    out.root_sp.resize(Cz);
    out.root_op.resize(Cz);
    out.root_ids.resize(Cz * 96);
    HGX_TRY(hipMemcpyAsync(b + o_cut, cut.data(), Cz * 4, hipMemcpyHostToDevice, stream));
    HGX_TRY(hipMemsetAsync(b + o_first, 0xFF, Cz * 4, stream));
    HGX_TRY(hipMemsetAsync(b + o_cnt, 0, 8, stream));
    launch_prune(stream, a, (uint32_t*)(b + o_part));
    HGX_TRY(hipGetLastError());
    uint32_t cnt[2] = {0, 0};
    HGX_TRY(hipMemcpyAsync(cnt, b + o_cnt, 8, hipMemcpyDeviceToHost, stream));
    if (n_kept) HGX_TRY(hipMemcpyAsync(out.old_gid.data(), a.old_gid, (size_t)n_kept * 4, hipMemcpyDeviceToHost, stream));
    HGX_TRY(hipMemcpyAsync(out.root_sp.data(), a.root_sp, Cz * 4, hipMemcpyDeviceToHost, stream));
    HGX_TRY(hipMemcpyAsync(out.root_op.data(), a.root_op, Cz * 4, hipMemcpyDeviceToHost, stream));
    HGX_TRY(hipMemcpyAsync(out.root_ids.data(), a.root_ids, Cz * 96, hipMemcpyDeviceToHost, stream));
    HGX_TRY(hipStreamSynchronize(stream));
    if ((int64_t)cnt[0] != n_kept || (int64_t)cnt[1] > n_kept) return hipErrorInvalidValue;   // host and device disagree on the cut
    const size_t no = cnt[1];
    out.n_others = (int64_t)no;
    out.oth_new.resize(no);
    out.oth_op.resize(no);
    out.oth_key.resize(no * 32);
    out.oth_pid.resize(no * 32);
    if (no) {
        HGX_TRY(hipMemcpyAsync(out.oth_new.data(), a.oth_new, no * 4, hipMemcpyDeviceToHost, stream));
        HGX_TRY(hipMemcpyAsync(out.oth_op.data(), a.oth_op, no * 4, hipMemcpyDeviceToHost, stream));
        HGX_TRY(hipMemcpyAsync(out.oth_key.data(), a.oth_key, no * 32, hipMemcpyDeviceToHost, stream));
        HGX_TRY(hipMemcpyAsync(out.oth_pid.data(), a.oth_pid, no * 32, hipMemcpyDeviceToHost, stream));
        HGX_TRY(hipStreamSynchronize(stream));
    }
    pr_in = InsertIn{};
    pr_in.creator = a.st_creator; pr_in.index32 = a.st_index; pr_in.sp32 = a.st_sp; pr_in.op32 = a.st_op;
    pr_in.ts = a.st_ts; pr_in.hash = a.st_hash; pr_in.S = a.st_S; pr_in.ntx = a.st_ntx;
    pr_count = n_kept;
    pr_old_gid = a.old_gid;
    pr_lay = PruneLayout{o_cr, o_idx, o_sp, o_op, o_ntx, o_old, o_ts, o_hash, o_S, o_fsp, o_fop, o_fl, o_fail, o_fail + 256};
    return hipSuccess;
}

// ---- hgx_get_frame_bodies (hgx_frame.hip) ----------------------------------
// Behind prune_stage: one launch writes the parents' ids and flags behind the staged columns, and
// the whole range (161 bytes per frame event and the fail word) comes back in ONE copy into
// page-locked memory, then one synchronise.
hipError_t Engine::frame_fetch(bool* missing) {
    *missing = false;
    if (pr_count < 0 || !ids_known) return hipErrorInvalidValue;
    const size_t back = pr_lay.end - pr_lay.creator;
    if (df_host_cap < back) {
        if (df_host) (void)hipHostFree(df_host);
        df_host = nullptr;
        df_host_cap = 0;
        const size_t want = std::max(back, (size_t)1 << 16);
        HGX_TRY(hipHostMalloc((void**)&df_host, want, hipHostMallocDefault));
        df_host_cap = want;
    }
    uint8_t* b = pr_buf.p;
    FrameArgs a{};
    a.E = E; a.n_kept = pr_count; a.C = C;
    a.g_creator = g_creator.p; a.g_sp = g_sp.p; a.g_op = g_op.p; a.g_id = g_id.p;
    a.old_gid = pr_old_gid;
    a.root_tab = root_ids_set ? root_tab_d.p : nullptr;
    a.root_pairs = root_ids_set && n_root_pairs > 0 ? root_pairs_d.p : nullptr;
    a.n_pairs = a.root_pairs ? n_root_pairs : 0;
    a.o_spid = b + pr_lay.spid; a.o_opid = b + pr_lay.opid; a.o_flags = b + pr_lay.flags;
    a.fail = (uint32_t*)(b + pr_lay.fail);
    HGX_TRY(hipMemsetAsync(b + pr_lay.fail, 0, 4, stream));
    launch_frame_parent_ids(stream, a);
    HGX_TRY(hipGetLastError());
    HGX_TRY(hipMemcpyAsync(df_host, b + pr_lay.creator, back, hipMemcpyDeviceToHost, stream));
    HGX_TRY(hipStreamSynchronize(stream));
    uint32_t f = 0;
    std::memcpy(&f, df_host + (pr_lay.fail - pr_lay.creator), 4);
    *missing = f != 0;
    return hipSuccess;
}

// the rows frame_fetch brought back, widened to the C ABI's columns
void Engine::frame_give(const FrameCols& out) const {
    const size_t K = (size_t)std::max<int64_t>(pr_count, 0);
    auto at = [&](size_t off) { return df_host + (off - pr_lay.creator); };
    auto widen = [&](int64_t* dst, size_t off) {
        if (!dst) return;
        const int32_t* s = (const int32_t*)at(off);
        for (size_t k = 0; k < K; k++) dst[k] = s[k];
    };
    widen(out.gid, pr_lay.old); widen(out.index, pr_lay.index); widen(out.sp, pr_lay.sp); widen(out.op, pr_lay.op);
    auto give = [&](void* dst, size_t off, size_t width) {
        if (dst && K) std::memcpy(dst, at(off), width * K);
    };
    give(out.ts, pr_lay.ts, 8); give(out.creator, pr_lay.creator, 4); give(out.ntx, pr_lay.ntx, 4);
    give(out.id, pr_lay.hash, 32); give(out.S, pr_lay.S, 32); give(out.spid, pr_lay.spid, 32);
    give(out.opid, pr_lay.opid, 32); give(out.flags, pr_lay.flags, 1);
}

// A keeping context, between prune_stage and the commit: the kept events' bodies into new tables.
// Nothing the context holds is changed, so a failure here leaves it whole.
hipError_t Engine::prune_bodies(bool* too_large) {
    *too_large = false;
    if (pr_count < 0) return hipErrorInvalidValue;
    return bodies_compact(pr_old_gid, pr_count, too_large);
}

// Commit: Reset with the new roots and Root.Others keys, then InsertEvent for the staged batch (the
// validation kernels re-check the frame; out.code != 0 is a bug the caller reports)
hipError_t Engine::prune_to_frame(const std::vector<int32_t>& root_round, const std::vector<uint8_t>& y_ext,
                                  const PruneOut& st, InsertOut& out) {
    if (pr_count < 0) return hipErrorInvalidValue;
    const int64_t count = pr_count;
    pr_count = -1;
    const bool lost = bodies_state == kBodiesLost;   // a prune is no hgx_clear: a lost store stays lost
    HGX_TRY(clear());
    if (lost) bodies_state = kBodiesLost;
    HGX_TRY(bodies_install());
    HGX_TRY(set_roots(root_round, y_ext));
    HGX_TRY(set_root_others(st.oth_key.data(), st.n_others));
    return insert(pr_in, count, out);
}

// ---- hgx_diff_wire (hgx_diff.hip) -----------------------------------------
// The host plan gave the exact row count, so the staging and the read-back are sized before any
// launch: known | root_index go up through the staged-copy path, three launches, and the header
// (the device's total) with every requested column comes back in ONE copy, then one synchronise.
hipError_t Engine::diff_wire(int graph, const int32_t* known, const int32_t* root_index, int64_t rows, int64_t expect,
                             const DiffCols& out, int64_t* dev_total, DiffBodies* body) {
    *dev_total = expect;
    if (graph < 0 || graph >= G || rows < 0 || rows > expect || expect > E || (out.hash && !ids_known))
        return hipErrorInvalidValue;
    if (rows == 0) return hipSuccess;   // a sizing call: the plan's total is the answer, nothing to launch
    // a payload copy of a split insert still in flight: the gather reads g_S (g_ts / g_id were joined
    // by payload_end, which every split insert runs before it returns)
    HGX_TRY(payload_wait_S());
    const size_t R = (size_t)rows, nb = (size_t)((E + kDiffChunk - 1) / kDiffChunk), nz = (size_t)n;
    size_t total = 0;
    auto take = [&](size_t bytes) {
        const size_t off = total;
        total += (bytes + 255) & ~(size_t)255;
        return off;
    };
    const size_t o_tab = take(2 * nz * 4), o_part = take(nb * 4), o_hdr = take(256);
    // the columns, widest first so that each stays aligned to its element (the 32-byte rows to 16)
    size_t col = o_hdr + 256;
    auto column = [&](bool want, size_t width) {
        if (!want) return (size_t)0;
        const size_t off = col;
        col += width * R;
        return off;
    };
    const size_t c_hash = column(out.hash, 32), c_S = column(out.S, 32),
                 c_gid = column(out.gid || body, 8),   // (the body gather's list is the gid column)
                 c_index = column(out.index, 8), c_spi = column(out.spi, 8), c_opi = column(out.opi, 8),
                 c_ts = column(out.ts, 8), c_creator = column(out.creator, 4), c_opc = column(out.opc, 4),
                 c_ntx = column(out.ntx, 4), c_nil = column(out.nil, 4), c_root = column(out.root, 1);
    total = col;
    if (df_buf.n < total) HGX_TRY(df_buf.alloc(std::max(total, 2 * df_buf.n)));
    const size_t back = col - o_hdr;   // header + columns
    if (df_host_cap < back) {
        if (df_host) (void)hipHostFree(df_host);
        df_host = nullptr;
        df_host_cap = 0;
        const size_t want = std::max(back, (size_t)1 << 16);
        HGX_TRY(hipHostMalloc((void**)&df_host, want, hipHostMallocDefault));
        df_host_cap = want;
    }
    uint8_t* b = df_buf.p;
    DiffArgs a{};
    a.E = E; a.rows = rows; a.c0 = graph * n; a.n = n;
    a.g_creator = g_creator.p; a.g_index = g_index.p; a.g_sp = g_sp.p; a.g_op = g_op.p; a.g_ntx = g_ntx.p;
    a.g_ts = g_ts.p; a.g_S = g_S.p; a.g_id = g_id.p; a.g_txnil = g_txnil.p;
    a.tab = (const int32_t*)(b + o_tab); a.part = (uint32_t*)(b + o_part); a.total = (uint32_t*)(b + o_hdr);
    auto at = [&](size_t off) { return off ? b + off : nullptr; };
    a.o_hash = at(c_hash); a.o_S = at(c_S);
    a.o_gid = (int64_t*)at(c_gid); a.o_index = (int64_t*)at(c_index); a.o_spi = (int64_t*)at(c_spi);
    a.o_opi = (int64_t*)at(c_opi); a.o_ts = (int64_t*)at(c_ts);
    a.o_creator = (int32_t*)at(c_creator); a.o_opc = (int32_t*)at(c_opc); a.o_ntx = (int32_t*)at(c_ntx);
    a.o_nil = (int32_t*)at(c_nil); a.o_root = at(c_root);
    std::vector<int32_t> tab(2 * nz);
    std::memcpy(tab.data(), known, nz * 4);
    std::memcpy(tab.data() + nz, root_index, nz * 4);
    HGX_TRY(stage_h2d(b + o_tab, tab.data(), 2 * nz * 4));
    HGX_TRY(stage_issue());
    launch_diff(stream, a);
    HGX_TRY(hipGetLastError());
    HGX_TRY(hipMemcpyAsync(df_host, b + o_hdr, back, hipMemcpyDeviceToHost, stream));
    HGX_TRY(hipStreamSynchronize(stream));
    stage_flush();
    uint32_t dt = 0;
    std::memcpy(&dt, df_host, 4);
    *dev_total = dt;
    bool hand_out = (int64_t)dt == expect;   // (a mismatch is a bug the caller reports: nothing is handed out)
    if (hand_out && body) {
        // hgx_diff_wire_bodies: the selected gids are in the staging; their R and transactions follow, and
        // the plain columns go out only when those fit
        body->ran = true;
        HGX_TRY(bodies_gather(nullptr, a.o_gid, nullptr, rows, body->out, &body->n_tx, &body->n_bytes, &body->fit));
        hand_out = body->fit == kBodyFits;
    }
    if (hand_out) {
        auto give = [&](void* dst, size_t off, size_t width) {
            if (dst && off) std::memcpy(dst, df_host + (off - o_hdr), width * R);
        };
        give(out.hash, c_hash, 32); give(out.S, c_S, 32); give(out.gid, c_gid, 8); give(out.index, c_index, 8);
        give(out.spi, c_spi, 8); give(out.opi, c_opi, 8); give(out.ts, c_ts, 8); give(out.creator, c_creator, 4);
        give(out.opc, c_opc, 4); give(out.ntx, c_ntx, 4); give(out.nil, c_nil, 4); give(out.root, c_root, 1);
    }
    return hipSuccess;
}

hipError_t Engine::get_ids(int64_t first, int64_t count, uint8_t* out32) {
    if (!ids_known || first < 0 || first + count > E) return hipErrorInvalidValue;
    if (count <= 0) return hipSuccess;
    HGX_TRY(hipMemcpyAsync(out32, g_id.p + 32 * first, (size_t)count * 32, hipMemcpyDeviceToHost, stream));
    return hipStreamSynchronize(stream);
}

hipError_t Engine::get_keys(uint8_t* out65) {
    if (!keys_set) return hipErrorNotReady;
    HGX_TRY(hipMemcpyAsync(out65, pk_keys.p, (size_t)C * 65, hipMemcpyDeviceToHost, stream));
    return hipStreamSynchronize(stream);
}

hipError_t Engine::set_roots(const std::vector<int32_t>& round, const std::vector<uint8_t>& y_ext) {
    rooted = false;
    root_gmax = -1;
    for (int c = 0; c < C; c++) {
        if (round[c] >= 0 || y_ext[c]) rooted = true;
        root_gmax = std::max(root_gmax, round[c] + 1);
    }
    if (!rooted) root_gmax = -1;
    HGX_TRY(hipMemcpyAsync(root_round_d.p, round.data(), (size_t)C * 4, hipMemcpyHostToDevice, stream));
    HGX_TRY(hipMemcpyAsync(root_y_ext_d.p, y_ext.data(), (size_t)C, hipMemcpyHostToDevice, stream));
    return hipStreamSynchronize(stream);
}

// Root.Others keys (event ids, 32 bytes each): sorted as 4 big-endian words for k_insert_check
hipError_t Engine::set_root_others(const uint8_t* keys32, int64_t count) {
    std::vector<std::array<uint64_t, 4>> k((size_t)count);
    for (int64_t i = 0; i < count; i++)
        for (int w = 0; w < 4; w++) {
            uint64_t x = 0;
            for (int b = 0; b < 8; b++) x = (x << 8) | keys32[32 * i + 8 * w + b];
            k[(size_t)i][w] = x;
        }
    std::sort(k.begin(), k.end());
    k.erase(std::unique(k.begin(), k.end()), k.end());
    n_others = (int64_t)k.size();
    if (others_d.n < (size_t)std::max<int64_t>(1, 4 * n_others)) HGX_TRY(others_d.alloc((size_t)std::max<int64_t>(1, 4 * n_others)));
    if (n_others) HGX_TRY(hipMemcpyAsync(others_d.p, k.data(), (size_t)n_others * 32, hipMemcpyHostToDevice, stream));
    return hipStreamSynchronize(stream);
}

// The roots' ids for the event-body encoder: one block of per-chain rows and the sorted Others pairs
// (the keys as set_root_others stores them, so the two binary searches order alike)
hipError_t Engine::set_root_ids(const uint8_t* x_id32, const uint8_t* has_x, const uint8_t* y_id32, const uint8_t* has_y,
                                const uint8_t* pairs64, int64_t n_pairs) {
    const size_t Cz = (size_t)C;
    std::vector<uint8_t> tab(66 * Cz, 0);
    bool any = n_pairs > 0;
    for (size_t p = 0; p < Cz; p++) {
        if (has_x && has_x[p]) {
            std::memcpy(tab.data() + 32 * p, x_id32 + 32 * p, 32);
            tab[64 * Cz + p] = 1;
            any = true;
        }
        if (has_y && has_y[p]) {
            std::memcpy(tab.data() + 32 * Cz + 32 * p, y_id32 + 32 * p, 32);
            tab[65 * Cz + p] = 1;
            any = true;
        }
    }
    std::vector<uint64_t> pr((size_t)n_pairs * 8);
    for (int64_t i = 0; i < n_pairs; i++) {
        for (int w = 0; w < 4; w++) {
            uint64_t x = 0;
            for (int b = 0; b < 8; b++) x = (x << 8) | pairs64[64 * i + 8 * w + b];
            pr[(size_t)i * 8 + w] = x;
        }
        std::memcpy(&pr[(size_t)i * 8 + 4], pairs64 + 64 * i + 32, 32);
    }
    if (root_tab_d.n < tab.size()) HGX_TRY(root_tab_d.alloc(tab.size()));
    if (root_pairs_d.n < std::max<size_t>(8, pr.size())) HGX_TRY(root_pairs_d.alloc(std::max<size_t>(8, pr.size())));
    HGX_TRY(hipMemcpyAsync(root_tab_d.p, tab.data(), tab.size(), hipMemcpyHostToDevice, stream));
    if (n_pairs) HGX_TRY(hipMemcpyAsync(root_pairs_d.p, pr.data(), pr.size() * 8, hipMemcpyHostToDevice, stream));
    HGX_TRY(hipStreamSynchronize(stream));
    n_root_pairs = n_pairs;
    root_ids_set = any;
    return hipSuccess;
}

hipError_t Engine::round_first_gids(int32_t r0, std::vector<int32_t>& out) {
    out.assign((size_t)std::max(0, R - r0), 0x7FFFFFFF);
    if (R <= r0) return hipSuccess;
    if (rfirst.n < (size_t)(R - r0)) HGX_TRY(rfirst.alloc((size_t)std::max(R - r0, 2 * (int)rfirst.n)));
    HGX_TRY(hipMemsetAsync(rfirst.p, 0x7F, (size_t)(R - r0) * 4, stream));
    launch_round_first_gid(stream, arrays(), r0, R, C, rfirst.p);
    HGX_TRY(hipMemcpyAsync(out.data(), rfirst.p, (size_t)(R - r0) * 4, hipMemcpyDeviceToHost, stream));
    return hipStreamSynchronize(stream);
}

hipError_t Engine::get_events(std::vector<int32_t>& creator, std::vector<int32_t>& index, std::vector<int32_t>& sp,
                              std::vector<int32_t>& op) {
    creator.resize((size_t)E);
    index.resize((size_t)E);
    sp.resize((size_t)E);
    op.resize((size_t)E);
    if (E == 0) return hipSuccess;
    HGX_TRY(hipMemcpyAsync(creator.data(), g_creator.p, (size_t)E * 4, hipMemcpyDeviceToHost, stream));
    HGX_TRY(hipMemcpyAsync(index.data(), g_index.p, (size_t)E * 4, hipMemcpyDeviceToHost, stream));
    HGX_TRY(hipMemcpyAsync(sp.data(), g_sp.p, (size_t)E * 4, hipMemcpyDeviceToHost, stream));
    HGX_TRY(hipMemcpyAsync(op.data(), g_op.p, (size_t)E * 4, hipMemcpyDeviceToHost, stream));
    return hipStreamSynchronize(stream);
}

hipError_t Engine::get_columns(std::vector<int32_t>& creator, std::vector<int32_t>& index, std::vector<int32_t>& sp,
                               std::vector<int32_t>& op, std::vector<int64_t>& ts, std::vector<uint8_t>& S,
                               std::vector<uint8_t>& coin, std::vector<int32_t>& ntx, std::vector<uint8_t>& txnil) {
    HGX_TRY(payload_wait_S());
    HGX_TRY(get_events(creator, index, sp, op));
    const size_t e = (size_t)E;
    ts.resize(e);
    S.resize(e * 32);
    coin.resize(e);
    ntx.resize(e);
    txnil.resize(e);
    if (e == 0) return hipSuccess;
    HGX_TRY(hipMemcpyAsync(ts.data(), g_ts.p, e * 8, hipMemcpyDeviceToHost, stream));
    HGX_TRY(hipMemcpyAsync(S.data(), g_S.p, e * 32, hipMemcpyDeviceToHost, stream));
    HGX_TRY(hipMemcpyAsync(coin.data(), g_coin.p, e, hipMemcpyDeviceToHost, stream));
    HGX_TRY(hipMemcpyAsync(ntx.data(), g_ntx.p, e * 4, hipMemcpyDeviceToHost, stream));
    HGX_TRY(hipMemcpyAsync(txnil.data(), g_txnil.p, e, hipMemcpyDeviceToHost, stream));
    return hipStreamSynchronize(stream);
}

hipError_t Engine::get_event_fields(int64_t gid, int64_t* ts, int32_t* ntx, int32_t* tx_nil) {
    uint8_t nil = 0;
    HGX_TRY(hipMemcpyAsync(ts, g_ts.p + gid, 8, hipMemcpyDeviceToHost, stream));
    HGX_TRY(hipMemcpyAsync(ntx, g_ntx.p + gid, 4, hipMemcpyDeviceToHost, stream));
    HGX_TRY(hipMemcpyAsync(&nil, g_txnil.p + gid, 1, hipMemcpyDeviceToHost, stream));
    HGX_TRY(hipStreamSynchronize(stream));
    *tx_nil = nil;
    return hipSuccess;
}

hipError_t Engine::reserve_rounds(int32_t rounds) {
    rounds = std::max<int32_t>(rounds, 1);
    drop_step_graph();
    Bm.release(); WLA.release(); WFD.release(); wflag.release(); wstat.release(); wcoin.release();
    active.release(); Tthr.release(); fw.release(); elig.release(); ur_empty.release(); Smat.release();
    Vbuf.release(); fame.release(); blk_cnt.release(); blk_loaded.release(); blk_ntx.release(); blk_nil.release();
    ovf.release();
    WLAT.release();
    r_cap = 0;
    R = 0;
    E_div = 0;
    HGX_TRY(ensure_round_cap(rounds));
    return hipStreamSynchronize(stream);
}

int Engine::rebuild_segments(int64_t En, int coord_compact) const {
    if (G != 1 || En < (int64_t)kLaSegMinRows * C) return 1;
    // as many segments as the CUs hold, of at least 2 x kLaHeadRows rows per chain: c2 (64 chains
    // of 16 384 rows, 4 column blocks) took 2.04 ms at 16 segments, 0.69 at 128, and at 192 its
    // exactness check failed (the verify sweep ran); c3 keeps its LDS-bound 16 (profiles/r05/b28_*, b29_*)
    // (the round-4 cap of kLaMaxSegs alone: c2 2.04 ms)
    const int cap_segs = (int)std::max<int64_t>(kLaMaxSegs, En / C / (2 * kLaHeadRows));
    return la_segs_override > 0 ? la_segs_override : la_wave_segments(n, coord_compact, num_cus, cap_segs);
}

// the rows divide_rounds left in the staging (defer_rows): copied into the host tables, which get
// their final sizes. The staging keeps them until the next stage_flush; what decide_fame_launch
// stages meanwhile goes behind them.
void Engine::divide_rounds_rows(RoundsHost& out) {
    if (!rows_pending) return;
    rows_pending = false;
    for (size_t k = 0; k < rows_n && k < stage_out.size(); k++) {   // (not what was staged behind them)
        StagedD2H& d = stage_out[k];
        std::memcpy(d.dst, h_stage + d.off, d.bytes);
        d.bytes = 0;
    }
    out.bm.resize((size_t)(R + 1) * C);
    out.wflag.resize((size_t)R * C);
}

// 1 + the lowest round of an event not yet received (rounds below it cannot be a
// roundReceived any more), R when every event is received; max_unrecv = most unreceived
// events of one chain
int32_t Engine::recv_round_lo(const RoundsHost& rh, int& max_unrecv) const {
    int32_t lo = R;
    max_unrecv = 0;
    if (E_div == 0 || rh.R == 0) return lo;
    for (int c = 0; c < C; c++) {
        const int32_t k = h_fu[c], len = h_len_div[c];
        if (k >= len) continue;
        max_unrecv = std::max(max_unrecv, len - k);
        int32_t a = 0, b = rh.R;   // round of offset k: largest r with bm[r][c] <= k
        while (a < b) {
            const int32_t mid = (a + b + 1) / 2;
            if (rh.bm[(size_t)mid * C + c] <= k) a = mid; else b = mid - 1;
        }
        lo = std::min(lo, a + 1);
    }
    return lo;
}

// ---- DecideFame -----------------------------------------------------------------
hipError_t Engine::decide_fame(int32_t r0, std::vector<int8_t>& fame_out) {
    HGX_TRY(decide_fame_launch(r0, fame_out));
    return fame_pending ? decide_fame_wait() : hipSuccess;
}

hipError_t Engine::decide_fame_launch(int32_t r0, std::vector<int8_t>& fame_out) {
    fame_pending = false;
    if (!rows_pending) {   // every earlier call synchronized: the staging is free
        stage_out.clear();
        stage_used = 0;
    }   // (else divide_rounds' rows are still in it: this call's go behind them)
    pend.clear();
    // rows [r0, R) are copied back below; the caller reads no row below r0, so the buffer only
    // grows (no O(R C) clear per call: the chunked schedule calls this thousands of times)
    if (fame_out.size() < (size_t)R * C) fame_out.resize((size_t)R * C, 0);
    r0 = std::max(r0, 0);
    if (R <= r0) return hipSuccess;
    DevArrays a = arrays();
    HGX_TRY(hipEventRecord(ph0, stream));
    HGX_TRY(hipGetLastError());   // (an error left by DivideRounds' launches surfaces there, not here)
    kbeg(K_FAME);
    launch_fame(stream, a, r0, R, C, n, nw, sm, G, fame_tally, num_cus);
    kend(K_FAME, 0);
    HGX_TRY(hipGetLastError());
    const size_t o = (size_t)r0 * C;
    HGX_TRY(stage_d2h(fame_out.data() + o, fame.p + o, fame_out.size() - o));
    HGX_TRY(stage_issue());
    HGX_TRY(hipEventRecord(ph1, stream));
    fame_pending = true;
    return hipSuccess;
}

hipError_t Engine::decide_fame_wait() {
    if (!fame_pending) {   // (no round from r0: nothing was launched; the stream's earlier work is awaited all the same)
        return hipStreamSynchronize(stream);
    }
    fame_pending = false;
    HGX_TRY(hipEventSynchronize(ph1));
    stage_flush();
    float ms = 0;
    HGX_TRY(hipEventElapsedTime(&ms, ph0, ph1));
    phase_ms[2] = ms;
    return collect_kernel_times();
}

// ---- FindOrder ------------------------------------------------------------------
hipError_t Engine::find_order(const std::vector<uint8_t>& el, const std::vector<uint8_t>& famous,
                              const std::vector<uint8_t>& ure, int32_t r0, int max_unrecv, OrderHost& out) {
    HGX_TRY(find_order_begin(el, famous, ure, r0, max_unrecv, out));
    return find_order_end(out, nullptr);
}

// threshold and roundReceived (every chain), consensus timestamps of the shard's chains
hipError_t Engine::find_order_begin(const std::vector<uint8_t>& el, const std::vector<uint8_t>& famous,
                                    const std::vector<uint8_t>& ure, int32_t r0, int max_unrecv, OrderHost& out) {
    stage_out.clear();   // every earlier call synchronized: the staging is free
    pend.clear();
    stage_used = 0;
    out = OrderHost();
    fo_m = 0;
    fo_cnt.assign(C, 0);
    if (R == 0 || E_div == 0 || max_unrecv == 0 || r0 >= R) return hipSuccess;
    DevArrays a = arrays();
    HGX_TRY(hipEventRecord(ph0, stream));
    const size_t o = (size_t)r0 * C;
    HGX_TRY(stage_h2d(elig.p, el.data(), (size_t)G * R));
    HGX_TRY(stage_h2d(fw.p + o, famous.data() + o, (size_t)R * C - o));
    HGX_TRY(stage_h2d(ur_empty.p, ure.data(), (size_t)G));
    HGX_TRY(stage_issue());
    if (WLAT.n < (size_t)R * C * n) {   // grown geometrically: R grows by a round or two per call
        // the first allocation covers the round tables' capacity (at most 256 M entries): each
        // later doubling was a synchronous free + allocation inside one FindOrder of the chunked
        // schedule (0.6-0.9 ms outliers)
        const size_t want = (size_t)R * C * n + (size_t)C * n;
        const size_t first = WLAT.n ? 0 : std::min((size_t)r_cap * C * n, (size_t)1 << 28);
        HGX_TRY(WLAT.alloc(std::max(want, std::max(2 * WLAT.n, first))));
        a = arrays();
    }
    kbeg(K_THRESHOLD);
    launch_wla_transpose(stream, a, r0, R, G, C, n);
    launch_threshold(stream, a, r0, R, C, n);
    kend(K_THRESHOLD, 0);
    {
        FillRange fr[2] = {{counters.p + kCtRecv, 8, 0}, {rcnt.p, (uint32_t)((size_t)C * 4), 0}};
        launch_fill_many(stream, fr, 2);
        HGX_TRY(hipGetLastError());
    }
    kbeg(K_ROUND_RECEIVED);
    launch_round_received(stream, a, R, C, n, max_unrecv);
    kend(K_ROUND_RECEIVED, 0);
    HGX_TRY(copy_to_pinned(h_small + kHsRecv, counters.p + kCtRecv, 8));
    HGX_TRY(stage_d2h(fo_cnt.data(), rcnt.p, (size_t)C * 4));
    HGX_TRY(stage_issue());
    HGX_TRY(hipStreamSynchronize(stream));
    stage_flush();
    fo_m = h_small[kHsRecv];
    out.panic = h_small[kHsRecv + 1] != 0;
    out.m = fo_m;
    int max_cnt = 0, unrecv = 0;
    for (int c = 0; c < C; c++) unrecv += h_len_div[c] - h_fu[c];
    for (int c = shard_lo; c < shard_hi; c++) max_cnt = std::max(max_cnt, fo_cnt[c]);
    kadd_bytes(K_ROUND_RECEIVED, (double)unrecv * 16);
    if (out.panic || fo_m == 0) {
        fo_m = 0;
        return collect_kernel_times();
    }
    int64_t own = 0;
    for (int c = shard_lo; c < shard_hi; c++) own += fo_cnt[c];
    const int c_cnt = shard_hi - shard_lo;
    // auto: the lane = event kernel where a launched chain receives at least 8 tiles (512 events) on
    // average. Measured at n = 256: from 16 to 256 events per chain its few large
    // blocks do not fill the device and k_cts_tile is 1-6 us ahead, from about 1 000 the two tie,
    // from 2 000 it is ahead (3.5 %, 8 % at 39 000); a SyncLimit-sized call receives a handful per
    // chain. Modes 3 / 4 force it wherever it has an instantiation
    constexpr int kCtsRowMinTiles = 8;
    const bool row = cts_row_ok(n) &&
        (cts_kernel >= 3 || (cts_kernel == 0 && own >= (int64_t)kCtsRowMinTiles * cts_row_tile() * c_cnt));
    kbeg(K_CTS);
    if (row && launch_cts_row(stream, a, shard_lo, c_cnt, C, n, fd_ld, max_cnt, R, cts_kernel == 4 ? 1 : 0))
        cts_row_runs++;
    else if (cts_kernel != 2 || !launch_cts_pipe(stream, a, shard_lo, c_cnt, C, n, fd_ld, max_cnt))
        launch_cts(stream, a, shard_lo, c_cnt, C, n, fd_ld, max_cnt);
    kend(K_CTS, (double)own * (4.0 * n + 8.0 * n));
    return hipSuccess;
}

// the consensus timestamps of the events newly received on chains [lo, hi), chain-major
// ([fu, fu + rcnt) of each chain): the values a shard exchanges
int64_t Engine::shard_values(int lo, int hi) const {
    int64_t k = 0;
    for (int c = lo; c < hi && c < (int)fo_cnt.size(); c++) k += fo_cnt[c];
    return k;
}

hipError_t Engine::shard_copy(int lo, int hi, void* buf, bool on_device, bool to_buf) {
    const int64_t cnt = shard_values(lo, hi);
    if (cnt == 0) return hipSuccess;
    std::vector<int32_t> offs(C + 1, 0);   // exclusive scan of the counts over [lo, hi)
    for (int c = lo; c < hi; c++) offs[c + 1] = offs[c] + fo_cnt[c];
    if (sh_off.n < (size_t)C + 1) HGX_TRY(sh_off.alloc((size_t)C + 1));
    HGX_TRY(hipMemcpyAsync(sh_off.p, offs.data(), (size_t)(C + 1) * 4, hipMemcpyHostToDevice, stream));
    int64_t* dev = (int64_t*)buf;
    if (!on_device) {
        if (sh_buf.n < (size_t)cnt) HGX_TRY(sh_buf.alloc((size_t)cnt));
        dev = sh_buf.p;
        if (!to_buf) HGX_TRY(hipMemcpyAsync(dev, buf, (size_t)cnt * 8, hipMemcpyHostToDevice, stream));
    }
    launch_cts_shard_copy(stream, arrays(), lo, hi, sh_off.p, dev, to_buf ? 1 : 0);
    if (!on_device && to_buf) HGX_TRY(hipMemcpyAsync(buf, dev, (size_t)cnt * 8, hipMemcpyDeviceToHost, stream));
    return hipStreamSynchronize(stream);
}

// sort by (graph, rr, cts, S), blocks
// order_dst (pinned, room for the m received events): the order is copied there with the block
// tables, in the same host round trip
hipError_t Engine::find_order_end(OrderHost& out, int32_t* order_dst) {
    HGX_TRY(payload_wait_S());   // (the sort's tie-break reads S)
    out.blk_cnt.assign((size_t)G * std::max(R, 1), 0);
    out.blk_ntx.assign((size_t)G * std::max(R, 1), 0);
    out.blk_loaded.assign((size_t)G * std::max(R, 1), 0);
    out.blk_nil.assign((size_t)G * std::max(R, 1), 0);
    const int32_t m = fo_m;
    if (m == 0) return hipSuccess;
    fo_m = 0;
    DevArrays a = arrays();
    uint32_t* vals = nullptr;
    const bool small = sort_small_ok(m);
    {   // one launch for the per-(graph, rr) block tables (and the small sort's ranks)
        FillRange fr[5] = {{blk_cnt.p, (uint32_t)((size_t)G * R * 4), 0},
                           {blk_loaded.p, (uint32_t)((size_t)G * R * 4), 0},
                           {blk_ntx.p, (uint32_t)((size_t)G * R * 8), 0},
                           {blk_nil.p, (uint32_t)((size_t)G * R), 0},
                           {val_b.p, (uint32_t)((size_t)m * 4), 0}};
        launch_fill_many(stream, fr, small ? 5 : 4);
        HGX_TRY(hipGetLastError());
    }
    // a large order (a full pass: 40 MB at c3) is written straight into the pinned host arena
    // (coalesced writes over the host link while the kernel runs) instead of a D2H copy after it --
    // by the bucket sort itself, which finishes every bucket it places (k_seg_sort, SortFinish: its
    // host-link writes overlap the other buckets' sorting), or by k_finish_order after the other
    // sorts; a small one comes back with the block tables in the copy launch
    // A large order into a pinned order_dst: the bucket sort runs in kOrderParts parts of about equal
    // event counts, each part's order copied to the host (DMA on stream_o) while the next part sorts
    // (round 6: the sort writing the gids over the host link itself took as long as sorting and copying
    // one after the other, c3 1.0 + 0.85 ms); the other sorts write the order straight into the arena.
    void* dst_dev = nullptr;
    const bool big_dst = order_dst && (size_t)m * 4 > kCopyKernelMax &&
                         hipHostGetDevicePointer(&dst_dev, order_dst, 0) == hipSuccess && dst_dev;
    if (order_dst && !big_dst) (void)hipGetLastError();   // (a pageable order_dst: the query's error is not sticky)
    bool direct = false, finished = false, piped = false;
    auto go_direct = [&]() {
        if (big_dst) {
            a.order_gid = (int32_t*)dst_dev;
            direct = true;
        }
    };
    if (small) {
        go_direct();
        kbeg(K_SORT);
        launch_sort_small(stream, a, m, n, &vals);
        kend(K_SORT, (double)m * 24.0);
    } else {
        // sort keys: cts range, then (graph, rr); and the (graph, rr) buckets' sizes (the segmented
        // sort's condition), read back in the same round trip
        const unsigned long long init[3] = {~0ull, 0ull, 0ull};
        HGX_TRY(hipMemcpyAsync(minmax.p, init, 24, hipMemcpyHostToDevice, stream));
        const int64_t nseg64 = (int64_t)G * R;
        const bool seg_try = sort_seg_enabled && nseg64 >= 1 && nseg64 <= (int64_t)1 << 24;
        const int nseg = (int)nseg64;
        if (seg_try) {   // (the bucket counts with the timestamp range, one pass)
            // sized for the round tables' capacity (then doubled): an exact-size reallocation whenever R
            // had grown since the last bucket sort was a hipFree + hipMalloc inside a chunked-schedule
            // FindOrder (1-2 ms calls)
            if (seg_off.n < (size_t)nseg + 1) {
                const size_t cap = std::max({(size_t)nseg + 1, (size_t)G * std::max(r_cap, 1) + 1, 2 * seg_off.n});
                HGX_TRY(seg_off.alloc(cap));
                HGX_TRY(seg_cur.alloc(cap));
            }
            HGX_TRY(hipMemsetAsync(seg_off.p, 0, (size_t)nseg * 4, stream));
            launch_seg_count(stream, a, m, R, n, nseg, seg_off.p, (unsigned long long*)minmax.p + 2);
        } else {
            launch_minmax(stream, a, m);
        }
        // (the bucket counts come back in the same round trip; below kOrderPipeMin the parts' launch tails
        // cost more than the copy they hide -- c2, 4 MB: order sort 0.23 -> 0.43 ms -- and the sort writes
        // the order straight into the arena)
        const bool want_cuts = seg_try && big_dst && (size_t)m * 4 >= kOrderPipeMin;
        if (want_cuts && h_segc_n < (size_t)nseg) {
            if (h_segc) HGX_TRY(hipHostFree(h_segc));
            h_segc = nullptr;
            h_segc_n = 0;
            const size_t cap = std::max((size_t)nseg, (size_t)G * std::max(r_cap, 1));
            HGX_TRY(hipHostMalloc((void**)&h_segc, cap * 4, hipHostMallocDefault));
            h_segc_n = cap;
        }
        if (want_cuts) HGX_TRY(hipMemcpyAsync(h_segc, seg_off.p, (size_t)nseg * 4, hipMemcpyDeviceToHost, stream));
        unsigned long long mm[3];
        HGX_TRY(hipMemcpyAsync(mm, minmax.p, 24, hipMemcpyDeviceToHost, stream));
        HGX_TRY(hipStreamSynchronize(stream));
        const int64_t cmin = (int64_t)(mm[0] ^ 0x8000000000000000ull);
        const int64_t cmax = (int64_t)(mm[1] ^ 0x8000000000000000ull);
        const int cts_bits = bitlen((uint64_t)(cmax - cmin));
        const int seg_bits = bitlen((uint64_t)G * (uint64_t)R - 1);
        uint64_t* keys = nullptr;
        kbeg(K_SORT);
        // (a refused LDS limit for the 1 024-thread bucket sort is reported before anything is
        // launched, and the radix passes run instead)
        const bool seg_ok = seg_try && cts_bits + seg_bits <= 64 && mm[2] >= 1 &&
                            mm[2] <= (unsigned long long)seg_sort_cap();
        // parts: cuts[k] = the first bucket of part k, off[k] = its first element of the order
        std::vector<int> cuts;
        std::vector<int64_t> off;
        if (seg_ok && want_cuts) {
            cuts.push_back(0);
            off.push_back(0);
            int64_t cum = 0;
            for (int sg = 0; sg < nseg && (int)cuts.size() < kOrderParts; sg++) {
                cum += h_segc[sg];
                if (cum * kOrderParts >= (int64_t)m * (int64_t)cuts.size() && sg + 1 < nseg) {
                    cuts.push_back(sg + 1);
                    off.push_back(cum);
                }
            }
            cuts.push_back(nseg);
            off.push_back(m);
            piped = cuts.size() > 2;
            if (piped && !stream_o) {
                HGX_TRY(hipStreamCreateWithFlags(&stream_o, hipStreamNonBlocking));
                for (auto& e : ev_o) HGX_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            }
        }
        // (a failure here is fatal, not a fallback to the radix passes: earlier parts' copies are queued)
        hipError_t part_err = hipSuccess;
        const std::function<hipError_t(int)> copy_part = [&](int k) -> hipError_t {
            const int64_t o0 = off[k], cnt = off[k + 1] - off[k];
            if (cnt <= 0) return hipSuccess;
            part_err = hipEventRecord(ev_o[k], stream);
            if (part_err == hipSuccess) part_err = hipStreamWaitEvent(stream_o, ev_o[k], 0);
            if (part_err == hipSuccess)
                part_err = hipMemcpyAsync(order_dst + o0, order_gid.p + o0, (size_t)cnt * 4, hipMemcpyDeviceToHost,
                                          stream_o);
            return part_err;
        };
        if (seg_ok && !piped) go_direct();
        const bool seg = seg_ok && launch_sort_seg(stream, a, m, cmin, cts_bits, R, n, nseg, seg_off.p, seg_cur.p,
                                                   (int)mm[2], &vals, &keys, piped ? &cuts : nullptr,
                                                   piped ? copy_part : nullptr) == hipSuccess;
        HGX_TRY(part_err);
        if (seg) {
            sort_seg_runs++;
            finished = true;
            if (piped) {   // the stream waits for the last part's copy
                HGX_TRY(hipEventRecord(ev_o[kOrderParts], stream_o));
                HGX_TRY(hipStreamWaitEvent(stream, ev_o[kOrderParts], 0));
            }
            kend(K_SORT, (double)m * 24.0 * 2);   // (bucket scatter + in-LDS sort: two passes' bytes)
        } else {
            (void)hipGetLastError();
            piped = false;
            direct = false;
            a.order_gid = order_gid.p;
            go_direct();
            launch_sort(stream, a, m, cmin, cts_bits, R, n, seg_bits, &vals, &keys);
            kend(K_SORT, (double)m * 24.0 *
                             (cts_bits + seg_bits <= 64 ? (cts_bits + seg_bits + 7) / 8
                                                        : (cts_bits + 7) / 8 + (seg_bits + 7) / 8));
        }
    }
    if (!finished) launch_finish_order(stream, a, m, vals, R, n);
    launch_fu_advance(stream, a, C);
    for (int c = 0; c < C; c++) h_fu[c] += fo_cnt[c];
    stage_out.clear();
    pend.clear();
    stage_used = 0;
    HGX_TRY(stage_d2h(out.blk_cnt.data(), blk_cnt.p, (size_t)G * R * 4));
    HGX_TRY(stage_d2h(out.blk_ntx.data(), blk_ntx.p, (size_t)G * R * 8));
    HGX_TRY(stage_d2h(out.blk_loaded.data(), blk_loaded.p, (size_t)G * R * 4));
    HGX_TRY(stage_d2h(out.blk_nil.data(), blk_nil.p, (size_t)G * R));
    if (order_dst && !direct && !piped) HGX_TRY(copy_to_pinned(order_dst, order_gid.p, (size_t)m * 4));
    HGX_TRY(stage_issue());
    HGX_TRY(hipEventRecord(ph1, stream));
    HGX_TRY(hipEventSynchronize(ph1));
    stage_flush();
    float ms = 0;
    HGX_TRY(hipEventElapsedTime(&ms, ph0, ph1));
    phase_ms[3] = ms;
    return collect_kernel_times();
}

hipError_t Engine::copy_order(int32_t* dst, int64_t first, int64_t count) {
    if (count <= 0) return hipSuccess;
    return hipMemcpyAsync(dst, order_gid.p + first, (size_t)count * 4, hipMemcpyDeviceToHost, stream);
}

hipError_t Engine::reset_received() {
    if (E > 0) {
        HGX_TRY(hipMemsetAsync(g_rr.p, 0xFF, (size_t)E * 4, stream));
        HGX_TRY(hipMemsetAsync(g_cts.p, 0, (size_t)E * 8, stream));
    }
    E_div = 0;
    R = 0;
    laid_out = false;
    return hipStreamSynchronize(stream);
}

// ---- getters --------------------------------------------------------------------
hipError_t Engine::get_rounds(std::vector<int32_t>& round_by_gid) {
    round_by_gid.assign((size_t)E_div, -1);
    if (E_div == 0) return hipSuccess;
    launch_gather_i32(stream, E_div, p_round.p, g_pos.p, recv_list.p);
    HGX_TRY(hipMemcpyAsync(round_by_gid.data(), recv_list.p, (size_t)E_div * 4, hipMemcpyDeviceToHost, stream));
    return hipStreamSynchronize(stream);
}

hipError_t Engine::get_received(std::vector<int32_t>& rr, std::vector<int64_t>& cts) {
    rr.assign((size_t)E, -1);
    cts.assign((size_t)E, 0);
    if (E == 0) return hipSuccess;
    HGX_TRY(hipMemcpyAsync(rr.data(), g_rr.p, (size_t)E * 4, hipMemcpyDeviceToHost, stream));
    HGX_TRY(hipMemcpyAsync(cts.data(), g_cts.p, (size_t)E * 8, hipMemcpyDeviceToHost, stream));
    return hipStreamSynchronize(stream);
}

hipError_t Engine::get_coords(int64_t gid, int32_t* la, int32_t* fd) {
    int32_t pos = 0;
    HGX_TRY(hipMemcpyAsync(&pos, g_pos.p + gid, 4, hipMemcpyDeviceToHost, stream));
    HGX_TRY(hipStreamSynchronize(stream));
    if (!compact) {
        HGX_TRY(hipMemcpyAsync(la, LA.p + (size_t)pos * n, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
        HGX_TRY(hipMemcpy2DAsync(fd, 4, FDT.p + pos, (size_t)fd_ld * 4, 4, (size_t)n, hipMemcpyDeviceToHost, stream));
        return hipStreamSynchronize(stream);
    }
    std::vector<uint16_t> l16(n), f16(n);
    const uint16_t* la16 = (const uint16_t*)LA.p;
    const uint16_t* fd16 = (const uint16_t*)FDT.p;
    HGX_TRY(hipMemcpyAsync(l16.data(), la16 + (size_t)pos * n, (size_t)n * 2, hipMemcpyDeviceToHost, stream));
    HGX_TRY(hipMemcpy2DAsync(f16.data(), 2, fd16 + pos, (size_t)fd_ld * 2, 2, (size_t)n, hipMemcpyDeviceToHost, stream));
    HGX_TRY(hipStreamSynchronize(stream));
    for (int i = 0; i < n; i++) {   // Coord<uint16_t> decode
        la[i] = (int32_t)l16[i] - 1;
        fd[i] = f16[i] == 0xFFFF ? 2147483647 : (int32_t)f16[i];
    }
    return hipSuccess;
}

}  // namespace hgx


namespace hgx {
void StepGraph::drop() {
    if (exec) (void)hipGraphExecDestroy(exec);
    if (graph) (void)hipGraphDestroy(graph);
    exec = nullptr;
    graph = nullptr;
}

void Engine::drop_step_graph() {
    for (auto& g : step_g) g.drop();
}
}  // namespace hgx
