// Engine::divide_rounds: the phases of one DivideRounds call ("call structure").
// What the call decides before its first launch is hgx_divide_plan.h's; the phases below launch it.
#include "hgx_engine.h"

#include <algorithm>
#include <cstring>

namespace hgx {

// nb round-step nodes captured as one hipGraph (their round arguments are rewritten per replay)
hipError_t Engine::capture_steps(StepGraph& sgr, const RoundArgs& args, int kern, int nb) {
    sgr.drop();
    sgr.args = args;
    sgr.kernel = kern;
    sgr.compact = compact;
    sgr.nb = nb;
    HGX_TRY(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
    hipError_t le = hipSuccess;   // a failed launch ends the capture, then is reported
    for (int k = 0; k < nb && le == hipSuccess; k++) le = launch_round_step(stream, sgr.args, k, kern);
    const hipError_t ce = hipStreamEndCapture(stream, &sgr.graph);
    if (le != hipSuccess) {
        if (ce == hipSuccess && sgr.graph) (void)hipGraphDestroy(sgr.graph);
        sgr.graph = nullptr;
        return le;
    }
    HGX_TRY(ce);
    HGX_TRY(hipGraphInstantiate(&sgr.exec, sgr.graph, nullptr, nullptr, 0));
    // the step nodes in launch order (a linear chain)
    size_t nn = 0;
    HGX_TRY(hipGraphGetNodes(sgr.graph, nullptr, &nn));
    std::vector<hipGraphNode_t> nodes(nn);
    HGX_TRY(hipGraphGetNodes(sgr.graph, nodes.data(), &nn));
    sgr.nodes.clear();
    sgr.params.clear();
    hipGraphNode_t nd_cur = nullptr;
    for (auto nd : nodes) {
        size_t nd_deps = 0;
        HGX_TRY(hipGraphNodeGetDependencies(nd, nullptr, &nd_deps));
        if (nd_deps == 0) nd_cur = nd;
    }
    while (nd_cur) {
        hipKernelNodeParams kp;
        HGX_TRY(hipGraphKernelNodeGetParams(nd_cur, &kp));
        sgr.nodes.push_back(nd_cur);
        sgr.params.push_back(kp);
        size_t nd_out = 0;
        HGX_TRY(hipGraphNodeGetDependentNodes(nd_cur, nullptr, &nd_out));
        if (nd_out == 0) break;
        std::vector<hipGraphNode_t> outs(nd_out);
        HGX_TRY(hipGraphNodeGetDependentNodes(nd_cur, outs.data(), &nd_out));
        nd_cur = outs[0];
    }
    if ((int)sgr.nodes.size() != nb) return hipErrorUnknown;
    return hipSuccess;
}

// ---- DivideRounds ---------------------------------------------------------------
// Chains are laid out with slack (positions [c_off[c], c_off[c] + slot)), so that a call
// after more InsertEvents only appends rows: the events of earlier calls keep their
// positions, lastAncestors rows and rounds, and the call works on the new events (DESIGN.md
// §3.7). The layout is rebuilt (and everything recomputed) when a chain outgrows its slot,
// the coordinate storage changes, or after reset_received / reserve_rounds / clear.
hipError_t Engine::divide_rounds(int64_t En, const std::vector<int32_t>& chain_len,
                                 const std::vector<int32_t>& chain_base, RoundsHost& out) {
    DivideIn in{};
    in.n = n; in.G = G; in.C = C; in.Ppos = Ppos; in.En = En;
    in.chain_len = chain_len.data(); in.chain_base = chain_base.data();
    in.len_div = h_len_div.data(); in.bm = out.bm.data(); in.R = out.R;
    in.laid_out = laid_out; in.E_div = E_div; in.compact = compact;
    in.incremental = incremental; in.force_coord32 = force_coord32;
    in.force_rebuild = false; in.seg = kLaSeg;
    divide_plan(in, h_off, div_plan);
    DivCall first{En, chain_len, chain_base, out, div_plan, false};
    HGX_TRY(divide_attempt(first));
    // a resumed call reads the wavefront's error word with its tail: a lane that gave up waiting
    // (bounded spins; never seen in practice) left rows unbuilt, and the call is made once more as a
    // rebuild with the sweeps for lastAncestors (which cannot give up: no third attempt)
    if (!(first.one_trip() && la_wave_used && h_small[kHsWaveErr] != 0)) return div_finish(first);
    la_wave_fallbacks++;
    in.force_rebuild = true;
    in.compact = compact;
    divide_plan(in, h_off, div_plan);
    DivCall second{En, chain_len, chain_base, out, div_plan, true};
    HGX_TRY(divide_attempt(second));
    return div_finish(second);
}

// one pass over the phases up to the tail's arrival on the host
hipError_t Engine::divide_attempt(DivCall& d) {
    stage_out.clear();   // every earlier call synchronized: the staging is free
    pend.clear();
    stage_used = 0;
    HGX_TRY(div_coordinates(d));
    HGX_TRY(div_rebuild_wait(d));
    HGX_TRY(div_round_tables(d));
    HGX_TRY(div_recurrence(d));
    if (d.r_done < 0) HGX_TRY(div_steps(d));
    if (!d.tail_ready) {
        HGX_TRY(enqueue_tail(d, d.r_done >= 0 ? d.r_done : d.plan.r_lo + d.launched * d.rc.nb));
        HGX_TRY(hipEventSynchronize(ph1));
    }
    return hipSuccess;
}

// ---- coordinates ------------------------------------------------------------------
// the layout's uploads, the positions of the new events and the lastAncestors rows' initial state
hipError_t Engine::div_layout(DivCall& d) {
    const DividePlan& p = d.plan;
    const int64_t En = d.En, E0 = p.E0;
    E = En;
    compact = p.compact;
    max_len = p.max_len;
    const size_t csz = compact ? 2 : 4;
    if (p.rebuild) {
        HGX_TRY(hipMemcpyAsync(c_off.p, h_off.data(), (C + 1) * 4, hipMemcpyHostToDevice, stream));
        h_len_div.assign(C, 0);
    }
    last_rebuild = p.rebuild;
    // c_len | c_base | c_old in one copy from pinned staging (the previous call's copy has
    // completed: every call synchronizes before returning)
    std::memcpy(h_cpar, d.chain_len.data(), (size_t)C * 4);
    std::memcpy(h_cpar + C, d.chain_base.data(), (size_t)C * 4);
    std::memcpy(h_cpar + 2 * C, h_len_div.data(), (size_t)C * 4);
    HGX_TRY(copy_from_pinned(cpar_blk.p, h_cpar, (size_t)3 * C * 4));
    HGX_TRY(stage_issue());
    d.a = arrays();
    HGX_TRY(hipEventRecord(ph0, stream));
    // lastAncestors: fixed point from all -1 (new rows), dirty-tracked sweeps (k_la_sweep)
    const size_t nunits = (size_t)((max_len + kLaSeg - 1) / kLaSeg) * C;
    // above kLaLanes chains a workgroup cannot give every chain a lane: the plan's lane map
    if (p.lanes_fit) {
        if (la_lmap.n < (size_t)std::max(1, p.la_na)) HGX_TRY(la_lmap.alloc((size_t)n));
        HGX_TRY(hipMemcpyAsync(la_lmap.p, p.lmap.data(), (size_t)p.la_na * 4, hipMemcpyHostToDevice, stream));
        d.la_map = la_lmap.p;
    }
    la_wave_used = la_kernel == 0 && !d.sweeps_only && la_wave_ok(n, max_len, p.la_na) && (n <= kLaLanes || d.la_map);
    // a rebuild of one large graph runs the wavefront on time segments in parallel (their
    // rows are lower bounds), then a verify sweep and the dirty sweeps complete them
    // the pipelined ingest laid these events out and ran the main pass of its segments already
    d.piped = pipe_ready && p.rebuild && la_wave_used && !d.la_map && pipe_nts > 1 && En == pipe_En &&
              compact == pipe_compact && h_off == pipe_off;
    pipe_ready = false;
    la_wave_segs = d.piped ? pipe_nts : (la_wave_used && p.rebuild) ? rebuild_segments(En, compact) : 1;
    kbeg(K_LAYOUT);
    if (!d.piped) launch_layout(stream, E0, En, d.a, C, n, kLaSeg);
    kend(K_LAYOUT, (double)(En - E0) * 64);
    if (p.rebuild) {   // (the wavefront writes every row it builds before anything reads it)
        if (!la_wave_used) HGX_TRY(hipMemsetAsync(LA.p, compact ? 0x00 : 0xFF, (size_t)h_off[C] * n * csz, stream));
    } else {
        launch_init_new(stream, d.a, E0, En - E0, n, fd_ld);
    }
    if (la_chg.n < nunits) {   // change stamps: new units start at 0, a stamp no sweep uses
        const size_t old = la_chg.n;
        HGX_TRY(la_chg.grow_copy(std::max(nunits, 2 * la_chg.n), old, stream));
        HGX_TRY(hipMemsetAsync(la_chg.p + old, 0, (la_chg.n - old) * 4, stream));
    }
    if (la_usum.n < nunits) HGX_TRY(la_usum.grow_copy(std::max(nunits, 2 * la_usum.n), la_usum.n, stream));
    d.cold = p.rebuild ? nullptr : c_old.p;
    la_sweeps = 0;
    la_rows = 0;
    return hipSuccess;
}

// dirty-tracked lastAncestors sweeps until one changes nothing (first_mode: the first sweep's,
// launch_la_sweep's `first`)
hipError_t Engine::run_sweeps(DivCall& d, int first_mode) {
    // sweep k's counters in ring slot k % kLaRing; up to kLaAhead sweeps are queued
    // before the host reads the oldest one's "units changed" (a sweep after the one that
    // changed nothing finds no dirty unit and does nothing)
    // dirty flags are sweep stamps (monotone over calls: stale ones never match), so a
    // sweep is one kernel, one 8-byte read-back and one event
    const size_t csz = compact ? 2 : 4;
    int launched_s = 0;
    HGX_TRY(hipMemsetAsync(counters.p + kCtSweep, 0, 16, stream));
    for (;;) {
        // a verify sweep usually finds nothing to redo: wait for it before queueing more
        const int ahead = (first_mode == 2 && la_sweeps == 0) ? 1 : kLaAhead;
        for (; launched_s < la_sweeps + ahead; launched_s++) {
            const int slot = launched_s % kLaRing;
            int32_t* cnt = counters.p + kCtSweep + 4 * slot;
            int32_t* cnt_next = counters.p + kCtSweep + 4 * ((launched_s + 1) % kLaRing);
            kbeg(K_LA_SWEEP);
            launch_la_sweep(stream, d.a, C, n, max_len, kLaSeg, launched_s == 0 ? first_mode : 0, la_chg.p, ++la_stamp,
                            la_usum.p, cnt, cnt_next, d.cold, d.plan.u0);
            kend(K_LA_SWEEP, 0);
            HGX_TRY(hipMemcpyAsync(h_small + kHsSweep + 4 * slot, cnt, 8, hipMemcpyDeviceToHost, stream));
            HGX_TRY(hipEventRecord(la_ev[slot], stream));
        }
        const int slot = la_sweeps % kLaRing;
        HGX_TRY(hipEventSynchronize(la_ev[slot]));
        const int32_t rows = h_small[kHsSweep + 4 * slot], changed = h_small[kHsSweep + 4 * slot + 1];
        // algorithmic bytes of the rows this sweep recomputed (read the two
        // parent rows, write the row, 12n + 16; the self-parent row is the register carry)
        la_rows += rows;
        kadd_bytes(K_LA_SWEEP, (double)rows * (3.0 * csz * n + 16));
        la_sweeps++;
        if (changed == 0) break;
        if (la_sweeps > 100000) return hipErrorUnknown;
    }
    return hipSuccess;
}

// lastAncestors of the new rows: the wavefront (whole, small-graph or on time segments) or the sweeps
hipError_t Engine::div_last_ancestors(DivCall& d) {
    const DividePlan& p = d.plan;
    const int64_t En = d.En, E0 = p.E0;
    const size_t csz = compact ? 2 : 4;
    if (!la_wave_used) return run_sweeps(d, 1);
    // one dataflow pass (k_la_wave); its error flag is read with the phase clock below
    // the error flag is 0 here: zeroed at creation, re-armed by every read
    int32_t* err = counters.p + kCtWaveErr;
    kbeg(K_LA_SWEEP);
    // a small graph (c1) entirely in one workgroup's LDS
    const size_t small_lds =
        (la_wave_segs == 1 && !d.la_map && la_small_override != 0) ? la_small_bytes(n, compact, p.graph_events) : 0;
    la_small_used = small_lds > 0;
    if (la_small_used) HGX_TRY(launch_la_small(stream, d.a, G, n, d.cold, small_lds, err));
    else if (!d.piped)
        HGX_TRY(launch_la_wave(stream, d.a, G, n, d.cold, En, la_wave_segs, 0, err, d.la_map, p.la_na,
                               !p.rebuild && (En - E0) <= 8 * (int64_t)C));
    if (la_wave_segs > 1)
        HGX_TRY(launch_la_wave(stream, d.a, G, n, nullptr, En, la_wave_segs, kLaHeadRows, err, d.la_map, p.la_na));
    const double rows = (double)(En - E0);
    kend(K_LA_SWEEP, rows * (3.0 * csz * n + 16));
    if (p.rebuild) {
        HGX_TRY(hipMemcpyAsync(h_small + kHsWaveErr, err, 4, hipMemcpyDeviceToHost, stream));
        HGX_TRY(hipMemsetAsync(err, 0, 4, stream));
    }
    if (la_wave_segs > 1) {
        // the verify sweep (+ dirty sweeps, counted there) only when the segments' exactness check
        // fails (k_la_seg_check): c3 1.6 ms per pass otherwise
        const size_t nt = (size_t)(la_wave_segs + 1) * n;
        if (la_chk.n < nt + 1) HGX_TRY(la_chk.alloc(nt + 1));
        HGX_TRY(hipMemsetAsync(la_chk.p, 0, 4, stream));
        HGX_TRY(launch_la_seg_check(stream, d.a, n, En, la_wave_segs, kLaHeadRows, la_chk.p + 1, la_chk.p));
        HGX_TRY(hipMemcpyAsync(h_small + kHsSegCheck, la_chk.p, 4, hipMemcpyDeviceToHost, stream));
        HGX_TRY(hipStreamSynchronize(stream));
        la_verified = h_small[kHsSegCheck] != 0 || la_verify_always;
        if (la_verified) HGX_TRY(run_sweeps(d, 2));
    }
    la_sweeps++;
    la_rows += (int64_t)rows;
    return hipSuccess;
}

// firstDescendants of the events of chains [d_lo, d_hi) (0, -1: every chain), then the root floors of
// every position on a rooted context (after a Reset). timed: the call's first build,
// which counts as K_FD_BUILD and takes the payload's side commit up again before the floors.
hipError_t Engine::fd_then_floors(DivCall& d, const int32_t* cold, int max_new, int d_lo, int d_hi, bool floors,
                                  bool timed) {
    if (timed) kbeg(K_FD_BUILD);
    launch_fd_build(stream, d.a, C, n, max_len, fd_ld, cold, max_new, d_lo, d_hi);
    if (timed) kend(K_FD_BUILD, (double)(d.En - d.plan.E0) * 2.0 * (compact ? 2 : 4) * n);
    if (timed && d.side_commit) HGX_TRY(hipStreamWaitEvent(stream, ev_side[1], 0));
    if (!floors || !rooted) return hipSuccess;
    if (gfl.n < (size_t)Ppos) HGX_TRY(gfl.alloc((size_t)Ppos));
    const size_t need = (size_t)(root_gmax + 1) * C;
    if (gB.n < need) {
        HGX_TRY(gB.alloc(need));
        drop_step_graph();
    }
    launch_root_floor(stream, d.a, root_round_d.p, gfl.p, gB.p, root_gmax, C, n, max_len);
    return hipSuccess;
}

hipError_t Engine::div_coordinates(DivCall& d) {
    HGX_TRY(div_layout(d));
    HGX_TRY(div_last_ancestors(d));
    // the compact payload of hgx_insert_and_run32 / _packed: its first columns started with this call
    // (or right behind the pipelined ingest's last piece) and have crossed PCIe under lastAncestors,
    // so they are committed here, ahead of the rounds and their coin pass, and nothing of the payload
    // is left between the recurrence and DecideFame. (Not earlier: issuing a copy from pageable memory
    // returns only once its source is consumed, and the wait for that would hold up the launches above.)
    // After a pipelined ingest its second side stream is idle (its segments were joined before the
    // ingest returned, and so was the layout): the commit runs there beside k_fd_build, which neither
    // reads nor writes what it touches, and the context stream takes it up again before the rounds.
    if (pay_commit_pending && pay_S_pending && !grp) {
        d.side_commit = d.piped && stream_p != nullptr && time_mask == 0;
        HGX_TRY(payload_commit(true, d.side_commit ? stream_p : stream));
        if (d.side_commit) HGX_TRY(hipEventRecord(ev_side[1], stream_p));
    }
    // (a chain-sharded group, one graph: the firstDescendants of this shard's chains' events)
    HGX_TRY(fd_then_floors(d, d.cold, d.plan.max_new, grp ? grp->c_split[shard] : 0, grp ? grp->c_split[shard + 1] : -1,
                           true, true));
    if (d.plan.rebuild) {   // events received before the rebuild (a prefix of every chain)
        HGX_TRY(hipMemsetAsync(fu.p, 0, (size_t)C * 4, stream));
        launch_fu_count(stream, d.a, d.En);
        h_fu.assign(C, 0);
        HGX_TRY(hipMemcpyAsync(h_fu.data(), fu.p, (size_t)C * 4, hipMemcpyDeviceToHost, stream));
    }
    return hipSuccess;
}

// A rebuild waits here for its coordinates (phase time 0) and reads the wavefront's error word.
// A call resuming the state makes one host round trip: its word is read with the rounds' results
// (enqueue_tail), and divide_rounds makes the second attempt.
hipError_t Engine::div_rebuild_wait(DivCall& d) {
    if (d.one_trip()) {
        HGX_TRY(hipEventRecord(ph2, stream));
    } else {
        HGX_TRY(hipEventRecord(ph1, stream));
        HGX_TRY(hipEventSynchronize(ph1));
        if (la_wave_used && h_small[kHsWaveErr] != 0) {
            // a wavefront lane gave up waiting (bounded spins): redo lastAncestors and the
            // firstDescendants built from them with the sweeps
            la_wave_used = false;
            la_wave_fallbacks++;
            HGX_TRY(hipMemsetAsync(LA.p, compact ? 0x00 : 0xFF, (size_t)h_off[C] * n * (compact ? 2 : 4), stream));
            HGX_TRY(run_sweeps(d, 1));
            HGX_TRY(fd_then_floors(d, d.cold, d.plan.max_new, 0, -1, true, false));
            HGX_TRY(hipEventRecord(ph1, stream));
            HGX_TRY(hipEventSynchronize(ph1));
        }
        float ms = 0;
        HGX_TRY(hipEventElapsedTime(&ms, ph0, ph1));
        phase_ms[0] = ms;
    }
    h_len_div = d.chain_len;
    E_div = d.En;
    laid_out = true;
    return hipSuccess;
}

// ---- rounds, from r_lo ---------------------------------------------
hipError_t Engine::div_round_tables(DivCall& d) {
    const int32_t r_lo = d.plan.r_lo;
    if (!d.one_trip()) HGX_TRY(hipEventRecord(ph0, stream));
    HGX_TRY(ensure_round_cap(r_lo + 2 * kStepBatch + 2));
    d.a = arrays();
    {   // one launch for the round tables' resets
        FillRange fr[4] = {{lr.p, (uint32_t)((size_t)G * 4), 0xFF},
                           {active.p + r_lo, (uint32_t)((size_t)(r_cap + 1 - r_lo) * 4), 0},
                           {ovf.p + r_lo, (uint32_t)((size_t)(r_cap + 2 - r_lo) * 4), 0},
                           {Bm.p, (uint32_t)((size_t)C * 4), 0}};
        launch_fill_many(stream, fr, r_lo == 0 ? 4 : 3);
        HGX_TRY(hipGetLastError());
    }
    const size_t need = (size_t)2 * C * round_k_ndw(n);
    if (FD8.n < need) {
        HGX_TRY(FD8.alloc(need));
        drop_step_graph();
    }
    kbeg(K_ROUND_GATHER);
    launch_round_gather(stream, d.a, r_lo, C, n, fd_ld);   // W'_{r_lo}: round 0 = first event of every chain
    kend(K_ROUND_GATHER, (double)C * n * 16);
    RoundPathIn in{};
    in.round_kernel = round_kernel; in.rooted = rooted; in.sharded = grp != nullptr; in.rebuild = d.plan.rebuild;
    in.round_pb_enabled = round_pb_enabled;
    in.g_ok = round_g_ok(n, nw); in.p_ok = round_p_ok(n, C, num_cus); in.pb_ok = round_pb_ok(n, G);
    in.new_events = d.En - d.plan.E0; in.C = C;
    d.rc = round_path(in);
    return hipSuccess;
}

RoundArgs Engine::round_args() const {
    RoundArgs A{};
    A.n = n; A.C = C; A.sm = sm; A.nw = nw; A.Pcap = fd_ld;
    A.c_len = c_len.p; A.c_off = c_off.p; A.c_base = c_base.p; A.LA = LA.p; A.FDT = FDT.p; A.compact = compact;
    A.p_gid = p_gid.p; A.g_coin = g_coin.p; A.FD8 = FD8.p; A.ovf = ovf.p;
    A.Bm = Bm.p; A.WLA = WLA.p; A.WFD = WFD.p; A.p_round = p_round.p; A.active = active.p;
    A.lr = lr.p; A.wflag = wflag.p; A.wstat = wstat.p; A.wcoin = wcoin.p; A.Smat = Smat.p;
    A.gB = rooted ? gB.p : c_len.p;   // (any int array without roots: read, never used)
    A.gmax = rooted ? root_gmax : -1;
    return A;
}

// What only the persistent kernels (hgx_round_p.hip, hgx_round_pb.hip) set up around the driver
struct Engine::PersistentSetup {
    bool sh = false;    // a chain-sharded group of more than one shard
    bool big = false;   // n > 256 (one graph): k_round_pb, a workgroup per chain with events
    int c_lo = 0, c_hi = 0, na = 0;
    RoundPWindows win;
    const RoundPWindows* win_d = nullptr;
};

static hipError_t group_wait(ShardGroup* grp) { return grp->wait() ? hipSuccess : hipErrorUnknown; }

hipError_t Engine::persistent_setup(DivCall& d, PersistentSetup& ps) {
    ps.sh = grp && grp->W > 1;
    ps.big = d.rc.path == RoundPath::PersistentBig;
    ps.c_hi = C;
    // a chain-sharded group: this shard's chain block, its candidate rows and granules written into
    // every shard's window; the host threads of the W shards meet at the barriers
    if (ps.sh) {
        RoundPWindows& win = ps.win;
        ps.c_lo = grp->c_split[shard];
        ps.c_hi = grp->c_split[shard + 1];
        HGX_TRY(hipStreamSynchronize(stream));
        HGX_TRY(group_wait(grp));   // every window is cleared and registered (its engine's FD8p / gran / st)
        win.nwin = grp->W;
        for (int k = 0; k <= grp->W; k++) win.c_split[k] = grp->c_split[k];
        for (int k = 0; k < grp->W; k++) {
            Engine* q = grp->eng[k];
            win.FD8p[k] = q->FD8p.p;
            win.gran[k] = q->rp_gran.p;
            win.st[k] = q->rp_st.p;
            win.FDT[k] = q->FDT.p;
            if (grp->dev[k] != dev || (grp->force_remote && k != shard)) win.remote |= 1u << k;
        }
        if (rp_win.n < sizeof(RoundPWindows)) HGX_TRY(rp_win.alloc(sizeof(RoundPWindows)));
        HGX_TRY(hipMemcpyAsync(rp_win.p, &win, sizeof(RoundPWindows), hipMemcpyHostToDevice, stream));
        HGX_TRY(hipStreamSynchronize(stream));
        ps.win_d = (const RoundPWindows*)rp_win.p;
    }
    if (ps.big) {
        h_amap.clear();
        for (int c = 0; c < C; c++)
            if (d.chain_len[c] > 0) h_amap.push_back(c);
        ps.na = (int)h_amap.size();
        if (ps.na == 0) return hipErrorCooperativeLaunchTooLarge;   // (nothing to step: the steps' path)
        if (rp_amap.n < (size_t)C) HGX_TRY(rp_amap.alloc((size_t)C));
        HGX_TRY(hipMemcpyAsync(rp_amap.p, h_amap.data(), (size_t)ps.na * 4, hipMemcpyHostToDevice, stream));
    }
    return hipSuccess;
}

// rounds [s, capacity) in one persistent launch
hipError_t Engine::persistent_launch(const PersistentSetup& ps, int32_t* fin, int32_t s, int init) {
    if (ps.big) {
        kbeg(K_ROUND_SEARCH);
        HGX_TRY(launch_round_pb(stream, round_args(), FD8p.p, rp_gran.p, rp_st.p, fin, rp_amap.p, ps.na, s, r_cap - 1,
                                num_cus, init != 0));
        kend(K_ROUND_SEARCH, 0);
        return hipSuccess;
    }
    if (ps.sh && init) {
        // W'_{r_lo} of this shard's chains into every window; every shard's launch starts once
        // every window holds the whole W'_{r_lo}
        HGX_TRY(launch_round_p(stream, round_args(), FD8p.p, rp_gran.p, rp_st.p, fin, s, r_cap - 1, 2, num_cus,
                               ps.c_lo, ps.c_hi, ps.win_d, ps.win.nwin));
        HGX_TRY(hipStreamSynchronize(stream));
        HGX_TRY(group_wait(grp));
    }
    kbeg(K_ROUND_SEARCH);
    HGX_TRY(launch_round_p(stream, round_args(), FD8p.p, rp_gran.p, rp_st.p, fin, s, r_cap - 1, ps.sh ? 0 : init,
                           num_cus, ps.c_lo, ps.c_hi, ps.win_d, ps.sh ? ps.win.nwin : 1));
    kend(K_ROUND_SEARCH, 0);
    return hipSuccess;
}

// every shard's outcome merged into st; then this shard's round rows into every shard's tables
hipError_t Engine::persistent_share(int32_t s, int32_t st[4]) {
    for (int k = 0; k < 4; k++) grp->st[shard][k] = st[k];
    HGX_TRY(group_wait(grp));
    for (int k = 0; k < grp->W; k++) {
        if (grp->st[k][0] != 0 && st[0] == 0) {
            st[0] = grp->st[k][0];
            st[3] = grp->st[k][3];
        }
        st[1] = std::max(st[1], grp->st[k][1]);
        st[2] = std::max(st[2], grp->st[k][2]);
    }
    if (st[0] == 0) HGX_TRY(share_round_rows(s, std::min(st[1] + 1, r_cap)));
    return group_wait(grp);
}

// The driver of the recurrences that run every round in one launch: the persistent one
// (hgx_round_p.hip; n > 256: hgx_round_pb.hip) and the whole-graph one (hgx_round_g.hip, n <= 16: one
// workgroup per graph, nothing shared between workgroups). A launch that reaches the round tables'
// capacity is continued from there by another (the whole-graph kernel's prologue rebuilds a round's
// state from Bm alone). Sets r_done = rounds [r_lo, r_done) written (the last one empty).
hipError_t Engine::run_recurrence(DivCall& d, RecurKind kind) {
    const int32_t r_lo = d.plan.r_lo;
    const bool pers = kind == kRecurPersistent;
    PersistentSetup ps;
    if (pers) {
        const int ndw = round_k_ndw(n);
        if (FD8p.n < (size_t)kRoundPBufs * C * ndw) HGX_TRY(FD8p.alloc((size_t)kRoundPBufs * C * ndw));
        if (rp_gran.n < (size_t)4 * C) HGX_TRY(rp_gran.alloc((size_t)4 * C));
    }
    if (rp_st.n < (size_t)4 + G) HGX_TRY(rp_st.alloc((size_t)4 + G));
    int32_t* fin = rp_st.p + 4;
    if (pers) HGX_TRY(hipMemsetAsync(rp_gran.p, 0, (size_t)4 * C * 8, stream));   // no tag survives a call
    HGX_TRY(hipMemsetAsync(fin, 0xFF, (size_t)G * 4, stream));                    // no graph finished yet
    if (pers) HGX_TRY(persistent_setup(d, ps));
    int32_t s = r_lo, last = -1;
    int finished = 0;
    for (int init = 1;; init = 0) {
        if (r_cap - 1 <= s + 1) {
            HGX_TRY(ensure_round_cap(s + 64));
            d.a = arrays();
        }
        HGX_TRY(hipMemsetAsync(rp_st.p, 0, 16, stream));
        if (pers) {
            HGX_TRY(persistent_launch(ps, fin, s, init));
        } else {
            kbeg(K_ROUND_SEARCH);
            HGX_TRY(launch_round_g(stream, round_args(), rp_st.p, fin, s, r_cap - 1));
            kend(K_ROUND_SEARCH, 0);
        }
        HGX_TRY(hipMemcpyAsync(h_small + kHsRoundSt, rp_st.p, 16, hipMemcpyDeviceToHost, stream));
        HGX_TRY(hipStreamSynchronize(stream));
        (pers ? round_p_runs : round_g_runs)++;
        // st[0] = 1 + the chain of a workgroup that gave up waiting (persistent only), st[1] the last
        // round written, st[2] graphs finished by this launch, st[3] rows counted exactly / that round
        int32_t st[4] = {h_small[kHsRoundSt], h_small[kHsRoundSt + 1], h_small[kHsRoundSt + 2], h_small[kHsRoundSt + 3]};
        round_p_ovf += st[3];
        if (ps.sh) HGX_TRY(persistent_share(s, st));
        if (pers && st[0] != 0) {
            round_p_fail_chain = st[0] - 1;
            round_p_fail_round = st[3];
            return hipErrorLaunchTimeOut;
        }
        last = std::max(last, st[1]);
        finished += st[2];
        if (finished >= G) break;
        s = st[1];   // the round tables' capacity: continue from there
    }
    d.r_done = last + 1;
    // graphs that finished earlier: empty rows up to the last round (k_last_round,
    // fame and the host copies read every graph's rows of every round)
    launch_round_p_tail(stream, round_args(), fin, last);
    if (ps.big) launch_round_pb_silent(stream, round_args(), r_lo, last);
    kbeg(K_ROUND_GATHER);
    launch_round_p_post(stream, round_args(), r_lo, last);
    kend(K_ROUND_GATHER, (double)(last - r_lo + 1) * C * n * (sizeof(int32_t) + (compact ? 2 : 4)));
    return hipGetLastError();
}

// the recurrence the plan chose; a persistent launch that cannot run or gave up re-enters at the steps
hipError_t Engine::div_recurrence(DivCall& d) {
    if (d.rc.path == RoundPath::WholeGraph) return run_recurrence(d, kRecurGraph);
    if (d.rc.path == RoundPath::Steps) return hipSuccess;
    const hipError_t pe = run_recurrence(d, kRecurPersistent);
    if (pe != hipSuccess) {
        // redo the rounds with the per-launch steps (a timed-out launch left partial rows)
        (void)hipGetLastError();
        if (pe != hipErrorLaunchTimeOut && pe != hipErrorCooperativeLaunchTooLarge) return pe;
        round_p_fallbacks++;
        d.r_done = -1;
        if (grp) {
            // the steps read every candidate's firstDescendants: this shard built its own chains'
            // only, so the whole table is rebuilt here, and W'_{r_lo} gathered again from it
            HGX_TRY(fd_then_floors(d, nullptr, 0, 0, -1, false, false));
            launch_round_gather(stream, d.a, d.plan.r_lo, C, n, fd_ld);
        }
    } else if (d.rc.precapture) {
        // the resumed calls that follow use the per-launch steps: their hipGraphs are captured and
        // instantiated now, inside this (long) rebuild call, not in the first short resumed one
        // (c2: a 7 ms first resumed call)
        for (int i = 1; i <= 2; i++)
            if (!step_g[i].exec) HGX_TRY(capture_steps(step_g[i], round_args(), 0, i == 1 ? kStepBatchSmall : 2 * kStepBatchSmall));
    }
    return hipSuccess;
}

// ---- the per-launch steps (n <= 1024, hgx_create's limit) --------------------------------
// nb step nodes replayed as one hipGraph; before each replay the nodes' round arguments are
// rewritten (hipGraphExecKernelNodeSetParams), so a step knows its round without a dependent
// device load.
hipError_t Engine::launch_batch(DivCall& d) {
    StepGraph& sgr = step_g[d.rc.step_graph];
    const int nb = d.rc.nb, kern = d.rc.step_kernel;
    const int32_t r_lo = d.plan.r_lo;
    const int need = r_lo + (d.launched + 2) * nb + 2;
    if (need > r_cap) {
        HGX_TRY(ensure_round_cap(need));
        d.a = arrays();
    }
    const RoundArgs cur = round_args();
    if (!sgr.exec || sgr.kernel != kern || sgr.compact != compact || sgr.nb != nb || sgr.args.gB != cur.gB ||
        sgr.args.gmax != cur.gmax)
        HGX_TRY(capture_steps(sgr, cur, kern, nb));
    const int slot = d.launched & 1;
    // the batch's last step writes round + 1 into this slot's host-mapped flag when a
    // chain still has events beyond its boundary (no D2H copy between the replays)
    sgr.args_last[slot] = sgr.args;
    sgr.args_last[slot].hflag = d_flag + slot;
    h_flag[slot] = 0;
    for (int k = 0; k < nb; k++) {
        sgr.round[k] = r_lo + d.launched * nb + k;
        void* args[2] = {(void*)(k == nb - 1 ? &sgr.args_last[slot] : &sgr.args), (void*)&sgr.round[k]};
        hipKernelNodeParams kp = sgr.params[k];
        kp.kernelParams = args;
        kp.extra = nullptr;
        HGX_TRY(hipGraphExecKernelNodeSetParams(sgr.exec, sgr.nodes[k], &kp));
    }
    // nb step kernels per replay, every replay bracketed by timing events when the round
    // search is timed (a sample of replays misjudged the pass: the first replays' rounds hold
    // most of the events, the last ones' steps find little left -- c5: 19.4 ms sampled
    // against 12.8 ms in the rocprofv3 trace)
    kbeg(K_ROUND_SEARCH, true, nb);
    HGX_TRY(hipGraphLaunch(sgr.exec, stream));
    kend(K_ROUND_SEARCH, 0);
    HGX_TRY(hipEventRecord(flag_ev[slot], stream));
    d.launched++;
    return hipSuccess;
}

// Batch i+1 is queued before the host looks at batch i's "any candidate left" flag (pipelined check).
hipError_t Engine::div_steps(DivCall& d) {
    launch_round_k_gather(stream, round_args(), d.plan.r_lo);   // W'_{r_lo} rebased for k_round_k
    // a rebuild keeps two batches in flight; a resumed call usually ends within its first
    // batch, so it waits for that batch's flag before queueing another
    HGX_TRY(launch_batch(d));
    if (d.plan.rebuild) HGX_TRY(launch_batch(d));
    if (d.one_trip()) {
        // the tail queued right behind the first batch: when that batch ends the rounds (the
        // usual resumed call), the call has made its only host round trip here
        HGX_TRY(enqueue_tail(d, d.plan.r_lo + d.launched * d.rc.nb));
        HGX_TRY(hipEventSynchronize(ph1));
        const int more = __atomic_load_n(&h_flag[0], __ATOMIC_ACQUIRE);
        d.checked = 1;
        if (!more) d.tail_ready = true;
        else {
            if (d.launched == d.checked) HGX_TRY(launch_batch(d));
            HGX_TRY(launch_batch(d));
        }
    }
    while (!d.tail_ready) {
        HGX_TRY(hipEventSynchronize(flag_ev[d.checked & 1]));
        const int more = __atomic_load_n(&h_flag[d.checked & 1], __ATOMIC_ACQUIRE);
        d.checked++;
        if (!more) break;
        if (d.launched == d.checked) HGX_TRY(launch_batch(d));   // no batch in flight
        HGX_TRY(launch_batch(d));
    }
    return hipSuccess;
}

// ---- the tail and the finish ----------------------------------------------------------
// the tail of the call: every graph's last round over the rounds stepped so far, and the rows
// [r_lo, r_hi] of the boundaries / [r_lo, r_hi) of the witness flags for the host copies
// (rows beyond the last round are copied and dropped), then ph1
hipError_t Engine::enqueue_tail(DivCall& d, int32_t r_hi) {
    RoundsHost& out = d.out;
    const int32_t r_lo = d.plan.r_lo;
    stage_out.clear();   // (a tail queued before more steps were needed is superseded)
    pend.clear();
    stage_used = 0;
    launch_last_round(stream, d.r_scan(), r_hi, G, C, n, wstat.p, lr.p);
    h_lr.assign(G, -1);
    HGX_TRY(stage_d2h(h_lr.data(), lr.p, (size_t)G * 4));
    const size_t b0 = (size_t)r_lo * C;
    if (out.bm.size() < (size_t)(r_hi + 1) * C) out.bm.resize((size_t)(r_hi + 1) * C);
    if (out.wflag.size() < (size_t)r_hi * C) out.wflag.resize((size_t)r_hi * C);
    HGX_TRY(stage_d2h(out.bm.data() + b0, Bm.p + b0, ((size_t)(r_hi + 1) * C - b0) * 4));
    if (r_hi > r_lo) HGX_TRY(stage_d2h(out.wflag.data() + b0, wstat.p + b0, (size_t)r_hi * C - b0));
    if (d.one_trip() && la_wave_used && !d.la_flag_read) {   // (read and re-armed once)
        HGX_TRY(copy_to_pinned(h_small + kHsWaveErr, counters.p + kCtWaveErr, 4, 0));
        d.la_flag_read = true;
    }
    HGX_TRY(stage_issue());
    return hipEventRecord(ph1, stream);
}

hipError_t Engine::div_finish(DivCall& d) {
    RoundsHost& out = d.out;
    // the staged rows: the graphs' last rounds (the first entry) are needed now; the boundary and
    // witness-flag rows (megabytes at c3) can wait for divide_rounds_rows when the caller asked so
    const bool defer = defer_rows && !stage_out.empty();
    defer_rows = false;
    if (defer) {
        StagedD2H& s0 = stage_out[0];
        std::memcpy(s0.dst, h_stage + s0.off, s0.bytes);
        s0.bytes = 0;
    } else {
        stage_flush();
    }
    // rounds below r_lo are unchanged and every round up to a graph's last one has witnesses,
    // so only [r_lo, R) is scanned: last = max(that, min(previous last, r_lo - 1))
    const int32_t r_scan = d.r_scan();
    if (r_scan > 0)
        for (int g = 0; g < G; g++) {
            const int32_t pl = g < (int)out.last_round.size() ? out.last_round[g] : -1;
            h_lr[g] = std::max(h_lr[g], std::min(pl, r_scan - 1));
        }
    out.last_round.assign(h_lr.begin(), h_lr.end());
    int32_t mx = -1;
    for (int g = 0; g < G; g++) mx = std::max(mx, out.last_round[g]);
    R = mx + 1;
    out.R = R;
    out.r_lo = std::min(d.plan.r_lo, R);
    // the host copies keep the rows below r_lo (rows the tail copied beyond R are dropped)
    rows_pending = defer;
    rows_n = stage_out.size();
    if (!defer) {
        out.bm.resize((size_t)(R + 1) * C);
        out.wflag.resize((size_t)R * C);
    }
    launch_wcoin(stream, d.a, out.r_lo, R, C);   // (DecideFame reads the coins on this stream)
    HGX_TRY(hipGetLastError());
    float ms = 0;
    if (d.one_trip()) {
        HGX_TRY(hipEventElapsedTime(&ms, ph0, ph2));
        phase_ms[0] = ms;
        HGX_TRY(hipEventElapsedTime(&ms, ph2, ph1));
    } else {
        HGX_TRY(hipEventElapsedTime(&ms, ph0, ph1));
    }
    phase_ms[1] = ms;
    step_prof_dump();   // -DHGX_STEP_PROF builds only
    return collect_kernel_times();
}

}  // namespace hgx
