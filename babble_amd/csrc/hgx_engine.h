// Device engine of libhgx: HBM-resident event DAG + the consensus kernels
// (hgx_kernels.hip). One Engine per context, one HIP stream. See DESIGN.md.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

#include "hgx_divide_plan.h"
#include "hgx_ingest_cols.h"
#include "hgx_kernels.h"

#ifndef HGX_TRY
#define HGX_TRY(x)                              \
    do {                                        \
        hipError_t _e = (x);                    \
        if (_e != hipSuccess) return _e;        \
    } while (0)
#endif

namespace hgx {


// kStepBatch round steps captured as one hipGraph, replayed with rewritten round arguments
struct StepGraph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    std::vector<hipGraphNode_t> nodes;   // the step nodes, in order
    std::vector<hipKernelNodeParams> params;
    RoundArgs args{};
    RoundArgs args_last[2]{};   // the last step node's arguments: args + the host flag of a batch slot
    int kernel = -1, compact = -1, nb = 0;   // what the graph was captured for
    int32_t round[64] = {};
    void drop();
};

enum KernelId {
    K_LAYOUT = 0, K_LA_SWEEP, K_FD_BUILD, K_ROUND_GATHER, K_ROUND_SEARCH, K_FAME, K_THRESHOLD,
    K_ROUND_RECEIVED, K_CTS, K_SORT, K_NUM
};

struct KernelStat {
    double ms = 0;        // summed device time (HIP events around the timed launches)
    int64_t launches = 0;
    int64_t timed = 0;    // launches inside HIP-event windows (the round steps time a sample of replays)
    double bytes = 0;     // algorithmic bytes summed over launches
};

template <typename T>
struct DBuf {
    T* p = nullptr;
    size_t n = 0;
    bool own = true;   // false: a view into another buffer (never freed here)
    hipError_t alloc(size_t count);
    hipError_t grow_copy(size_t count, size_t keep, hipStream_t s);
    void release();
    void view(T* q, size_t count) {   // point into a block owned elsewhere
        release();
        p = q;
        n = count;
        own = false;
    }
    ~DBuf() { release(); }
};

// What the host bookkeeping needs after DivideRounds
struct RoundsHost {
    int32_t R = 0;                    // rounds materialised: max over graphs of LastRound + 1
    int32_t r_lo = 0;                 // rows below r_lo are unchanged by the last DivideRounds
    std::vector<int32_t> last_round;  // [G], -1 = no events
    std::vector<int32_t> bm;          // [(R+1) x C] first chain offset with round >= r
    std::vector<uint8_t> wflag;       // [R x C] 0 none, 1 candidate with higher round, 2 witness
};

struct OrderHost {
    int32_t m = 0;                    // newly received events
    std::vector<int32_t> order_gid;   // [m] graph-major (rr, cts, S) order
    std::vector<int32_t> blk_cnt;     // [G x R]
    std::vector<int64_t> blk_ntx;     // [G x R]
    std::vector<int32_t> blk_loaded;  // [G x R]
    std::vector<uint8_t> blk_nil;     // [G x R] the block's first event has nil Transactions
    bool panic = false;
};

// Outcome of one insert batch (Engine::insert)
struct InsertOut {
    int64_t accepted = 0;          // events appended (the prefix before the first failure)
    int code = 0;                  // InsertCode of the first failing event (0: none)
    int32_t fail_creator = 0;      // its creator and Index (error messages)
    int64_t fail_index = 0;
    // per-creator state after the batch ([C]) and loaded events per graph ([G], cumulative)
    std::vector<int32_t> last_gid, last_index, chain_base;
    std::vector<unsigned long long> graph_loaded;
};

class Engine;
struct BodiesIn;     // hgx_bodies.h
struct EvScratch;    // hgx_goenc_dev.hip: the event-body front end's chunk buffers
void free_ev_scratch(EvScratch* p);

// A chain-sharded group (hgx_create_sharded / hgx_set_round_shards): W engines in one
// process, shard k's on device dev[k] (devices may repeat), each holding the whole DAG. Shard k
// builds the firstDescendants of its chains' events [c_split[k], c_split[k+1]), runs the persistent
// recurrence for those chains and their consensus timestamps, and hands its candidate rows and
// granules to every shard through that shard's window (peer-mapped device memory, write-through);
// the round outputs of its chains are copied to every shard after each launch. The W engines' host
// threads meet at the group's barriers.
struct ShardGroup {
    int W = 1;
    int dev[kMaxShards] = {};
    int32_t c_split[kMaxShards + 1] = {};
    Engine* eng[kMaxShards] = {};
    int32_t st[kMaxShards][4] = {};   // every shard's status words after its last persistent launch
    // hgx_set_shard_remote (test switch): every other shard's window is written as if it were on
    // another device (system-scope stores), so one GPU runs the instructions an 8-GPU node runs
    bool force_remote = false;
    bool wait();                      // false: a shard failed (or 120 s passed): leave with an error
    void fail();
    void rearm();                     // before a group call (no thread inside the group)
   private:
    std::mutex m;
    std::condition_variable cv;
    int count = 0;
    uint64_t gen = 0;
    bool broken = false;
};

class Engine {
   public:
    ~Engine();
    hipError_t init(int device, int n_graphs, int n_part, int64_t cap_events, std::string& why);

    // InsertEvent for `count` events whose columns are device pointers (hgx_insert_events_device)
    // or host pointers staged to HBM first (hgx_insert_events); validation and append on the GPU.
    hipError_t insert(const InsertIn& in, int64_t count, InsertOut& out);
    // the same with Event.Verify first (hashgraph.go:356-363): digest (EventBody.Hash) and R per
    // event, S = in.S, key = the creator's (set_keys); device pointers
    // fail_armed: the caller armed ins_fail_sig and a check of its own has filed into it (the flat id pass)
    hipError_t insert_verified(const InsertIn& in, const uint8_t* digest, const uint8_t* r, int64_t count,
                               InsertOut& out, bool fail_armed = false);
    hipError_t stage_sig(const uint8_t* digest, const uint8_t* r, int64_t count, const uint8_t** d_digest,
                         const uint8_t** d_r);
    // the same with Event.Hash and Event.Verify's digest computed here from the events' fields (host
    // columns): Go-JSON texts, ids in dependency order, body digests, then insert_verified, in internal
    // chunks (hgx_goenc_dev.hip). txi: bodies_check's. out_id32 (host, may be null)
    // gets the accepted prefix's ids. op_id32 (host, may be null): the ids of the HGX_ROOT_OTHER
    // other-parents, 32 bytes per event (read on a context with root ids only).
    hipError_t insert_bodies(const BodiesIn& ev, const std::vector<int64_t>& txi, int64_t count, const uint8_t* op_id32,
                             uint8_t* out_id32, InsertOut& out);
    // The same with every event's claimed id supplied (host, [count][32]): the ids are
    // proven in one flat pass instead of computed level after level. out.code = INS_ID_MISMATCH at the
    // first event whose claimed id is not its hash, behind the proven and accepted prefix.
    hipError_t insert_bodies_claimed(const BodiesIn& ev, const std::vector<int64_t>& txi, int64_t count,
                                     const uint8_t* op_id32, const uint8_t* claimed_id32, InsertOut& out);
    // The same for a SyncResponse's wire events (hgx_wire.hip): ev.sp / ev.op hold the
    // host plan's parent descriptors (hgx_wire_plan.h), lo / woff / slots its windows. The window is
    // filled once against the resident events (not launched when n_resident == 0), every chunk's
    // descriptors become gids on the device before the encoder reads them, then insert_bodies' chunks
    // unchanged. out_sp / out_op (host, may be null) get the accepted prefix's parent gids.
    struct WireWindows {
        const int32_t *lo, *woff;   // [n]
        int64_t slots, n_resident;
    };
    hipError_t insert_wire_bodies(const BodiesIn& ev, const std::vector<int64_t>& txi, int64_t count,
                                  const WireWindows& w, uint8_t* out_id32, int64_t* out_sp, int64_t* out_op,
                                  InsertOut& out);
    // Event.Sign on the device. set_signing_keys: C private keys of 32 big-endian bytes
    // (each 0 = none, or in [1, N-1]: the caller checked), null clears; d G of every key is compared with
    // the participant's key: *mismatch = the first participant whose key differs (nothing is changed
    // then), else -1. The device copy is zeroed before it is freed. sign_insert_bodies = insert_bodies
    // with R and S computed by the device (ev.r / ev.s are not read); out_r32 / out_s32 / out_id32 (host,
    // may be null) get the accepted prefix.
    hipError_t set_signing_keys(const uint8_t* priv32, int32_t* mismatch);
    hipError_t sign_insert_bodies(const BodiesIn& ev, const std::vector<int64_t>& txi, int64_t count,
                                  const uint8_t* op_id32, uint8_t* out_r32, uint8_t* out_s32, uint8_t* out_id32,
                                  InsertOut& out);
    bool sign_keys_set = false;
    std::vector<uint8_t> sign_has;   // [C] the participant has a signing key
    EvScratch* ev_scratch = nullptr;
    // The resident body store (hgx_keep_bodies, hgx_bodystore.hip): R and the
    // transaction bytes of every event, appended by insert_bodies_run behind each chunk's insert and
    // read back by gid. bodies_state: hgx_bodystore.h's (off / complete / lost); the caller (finish_insert)
    // marks the store lost when events arrived without their bodies (bodies_events != E).
    struct BodyOut {   // host arrays, any may be null (capacities in transactions / bytes)
        uint8_t* sig_r;
        int32_t* ntx;
        int64_t* tx_off;
        int64_t tx_cap;
        uint8_t* tx_bytes;
        int64_t bytes_cap;
    };
    // a gather's outcome: the caller's capacities are short (the totals alone are reported), the arrays
    // are written, or the list names 4 GiB or more (nothing was copied)
    enum BodyFit { kBodyShort = 0, kBodyFits = 1, kBodyTooLarge = 2 };
    struct BodyPlan {   // a measured gather: the list, its scanned counts (device scratch) and totals
        int64_t m = 0, n_tx = 0, n_bytes = 0;
        const int64_t* gids64 = nullptr;
        const int32_t* gids32 = nullptr;
        uint32_t *cnt_tx = nullptr, *cnt_by = nullptr;
        bool too_large = false;
    };
    hipError_t bodies_keep(int64_t tx_hint, int64_t bytes_hint);
    hipError_t bodies_reset();
    hipError_t bodies_reserve(int64_t add_tx, int64_t add_bytes);
    hipError_t bodies_append(const uint8_t* r, const int64_t* txi, const int64_t* off, const uint8_t* bytes, int64_t a,
                             int64_t nt, int64_t nbytes);
    hipError_t bodies_measure(const int64_t* gids_host, const int64_t* gids_dev64, const int32_t* gids_dev32, int64_t m,
                              BodyPlan& plan);
    hipError_t bodies_copy(const BodyPlan& plan, uint8_t* o_R, int32_t* o_ntx, int64_t* o_txi, int64_t* o_off,
                           uint8_t* o_bytes);
    // hgx_save_bodies: the store is in gid order, so a gid range is a slice of each table. `count` entries
    // from `lo` of the R rows (32 bytes each), the events' first slots (b_txi, E + 1 entries), the
    // transaction offsets (b_off, T + 1 entries) or the arena's bytes, into host memory; returns when copied.
    enum BodyTable { kBodyRows = 0, kBodySlots = 1, kBodyOffsets = 2, kBodyArena = 3 };
    hipError_t bodies_read(BodyTable which, int64_t lo, int64_t count, void* dst);
    hipError_t bodies_gather(const int64_t* gids_host, const int64_t* gids_dev64, const int32_t* gids_dev32, int64_t m,
                             const BodyOut& out, int64_t* n_tx, int64_t* n_bytes, BodyFit* fit);
    // the second half of bodies_gather for a measured list that fits `out`: copy, one read-back, the arrays
    hipError_t bodies_fetch(const BodyPlan& plan, const BodyOut& out);
    // hgx_prune_to_frame on a keeping context, behind prune_stage and before anything is dropped: the
    // kept events' bodies gathered into new tables, which prune_to_frame puts in place. On a failure
    // (hipErrorOutOfMemory; *too_large: the kept bodies reach 4 GiB) the context is as it was.
    hipError_t prune_bodies(bool* too_large);
    hipError_t bodies_compact(const int32_t* old_gid_dev, int64_t kept, bool* too_large);
    // Block.Hash of the last find_order's new blocks (hgx_goenc_dev.hip): `count` blocks over the n_events
    // newly ordered events, in the order's own sequence; rr / ntx / nil host arrays, out32 32 bytes per block.
    // *too_large: the blocks' bytes or text reach 4 GiB, nothing was hashed. Changes nothing but scratch.
    hipError_t order_block_hashes(int64_t n_events, const int64_t* rr, const int32_t* ntx, const int32_t* nil,
                                  int64_t count, uint8_t* out32, bool* too_large);
    hipError_t bodies_install();
    int bodies_state = 0;
    int64_t bodies_events = 0, bodies_tx = 0, bodies_bytes = 0;
    DBuf<uint8_t> b_R, b_arena, b_work, b_out, b_new_arena, b_new_rows;
    DBuf<int64_t> b_txi, b_off, b_new_off;
    bool b_new_ready = false;
    int64_t b_new_events = 0, b_new_tx = 0, b_new_bytes = 0;
    uint8_t* b_host = nullptr;   // page-locked: a gather's result comes back in one copy
    size_t b_host_cap = 0;
    // The roots' ids on the device: Root.X / Root.Y per chain and the Root.Others
    // pairs sorted by event id, the text of the parents that are in no id column. has_x / has_y: [C];
    // pairs: (event id, other-parent id) sorted by event id. root_ids_set = some id is installed (a
    // context without one encodes exactly as an unrooted one).
    hipError_t set_root_ids(const uint8_t* x_id32, const uint8_t* has_x, const uint8_t* y_id32, const uint8_t* has_y,
                            const uint8_t* pairs64, int64_t n_pairs);
    bool root_ids_set = false;
    DBuf<uint8_t> root_tab_d;      // x_id [C][32] | y_id [C][32] | has_x [C] | has_y [C]
    DBuf<uint64_t> root_pairs_d;   // [n_root_pairs][8]: the key as 4 big-endian words, the value's 32 bytes
    int64_t n_root_pairs = 0;
    // participants' public keys (65 bytes each, C of them): device window tables built once
    hipError_t set_keys(const uint8_t* keys65);
    bool keys_set = false;
    // A batch's host columns (hgx_ingest_cols.h, any form) staged to HBM and `in` pointed at them:
    // kStageAll every column (a batch of at most kPackEvents in one pinned copy, else a copy per
    // column), kStageStructure the structure columns alone. The packed form's structure is decoded
    // into the compact staging columns (launch_unpack_packed); its exceptions are already checked.
    enum StagePart { kStageStructure, kStageAll };
    hipError_t stage(const HostCols& hc, int64_t count, StagePart part, InsertIn& in);
    // hgx_insert_and_run's split insert of host columns: the structure columns (creator, index,
    // parents) are staged, validated and committed now (out.graph_loaded is not final); a worker
    // thread copies the payload columns (timestamps, hash or coin, S, transactions) of the accepted
    // prefix on a second stream while the caller runs DivideRounds; payload_commit / payload_finish
    // (below) join it, commit the payload, rewrite the layout's timestamps and the candidates' coins,
    // and payload_loaded returns the graphs' loaded counts. Not for rooted contexts (Root.Others needs
    // the hash at validation).
    hipError_t insert_split_begin(const HostCols& hc, int64_t count, InsertOut& out);
    hipError_t payload_begin(const HostCols& hc, int64_t m_ok);
    // payload_end in three parts, so that no host wait stands between the rounds and DecideFame:
    // payload_commit waits for the first columns, commits them and (positions) rewrites the layout's
    // timestamps -- divide_rounds queues it for the compact payload ahead of k_fd_build, where the
    // copy has landed and the coins are in place for the witnesses' coin pass; payload_finish commits
    // what is still pending (the wide payload; a DivideRounds that did not run or failed), redoes the
    // coins then, and queues the read-back of the graphs' loaded counts without waiting for it;
    // payload_loaded reads them once the stream has been synchronized (DecideFame's round trip).
    hipError_t payload_commit(bool positions, hipStream_t on = nullptr);   // (on: another stream than the context's)
    hipError_t payload_finish(bool laid_out_new, int32_t wcoin_r0);
    void payload_loaded(std::vector<uint64_t>& loaded) const;
    double pay_host_ms = 0;   // host time of the three for the last payload (hgx_phase_times)
    // the compact payload's S column (copied last, straight into g_S): wait for it (the sort's
    // tie-break, a read-back, a clear) and for the caller's buffer to be read completely
    hipError_t payload_wait_S();
    // forget every event (a fresh NewHashgraph); allocations are kept
    hipError_t clear();
    // hgx_prune_to_frame (hgx_compact.hip) in two steps. prune_stage changes nothing
    // resident: the events with Index >= cut[creator] (n_kept of them, counted by the caller) are
    // gathered into a staging block as one insert batch with renumbered parents, and their old gids,
    // the Root.Others entries and the new roots' parents and ids are read back (O(kept + C) bytes).
    // prune_to_frame then clears the store, installs the roots and the Others keys and re-inserts
    // the staged batch through the validation kernels.
    struct PruneOut {
        std::vector<int32_t> old_gid;            // [n_kept] old gid of each new gid
        std::vector<int32_t> root_sp, root_op;   // [C] parents of each chain's first kept event (-1 without one)
        std::vector<uint8_t> root_ids;           // [C][3][32] ids of that event, its self- and other-parent (zero: none)
        int64_t n_others = 0;                    // Root.Others entries, in no particular order:
        std::vector<int32_t> oth_new, oth_op;    // the event's new gid, its old other-parent (gid or HGX_ROOT_OTHER)
        std::vector<uint8_t> oth_key, oth_pid;   // the event's id and its other-parent's (zero for a code)
    };
    hipError_t prune_stage(const std::vector<int32_t>& cut, int64_t n_kept, PruneOut& out);
    hipError_t prune_to_frame(const std::vector<int32_t>& root_round, const std::vector<uint8_t>& y_ext,
                              const PruneOut& st, InsertOut& out);
    // hgx_get_frame_bodies (hgx_frame.hip), behind prune_stage: frame_fetch adds the
    // parents' ids and flags (k_frame_parent_ids) to the staged columns and brings the whole range back
    // in one copy into df_host; *missing: a root id or Others pair that must exist was not found (nothing
    // may be handed out). frame_give then converts the rows into the caller's arrays (null = not
    // wanted), frame_measure_bodies and bodies_fetch size and gather R and the transactions through the
    // staging's old gids, and
    // prune_unstage disarms the staging. None of them changes anything resident.
    struct FrameCols {
        int64_t *gid, *index, *ts, *sp, *op;
        int32_t *creator, *ntx;
        uint8_t *id, *S, *spid, *opid, *flags;
    };
    hipError_t frame_fetch(bool* missing);
    void frame_give(const FrameCols& out) const;
    hipError_t frame_measure_bodies(BodyPlan& plan) { return bodies_measure(nullptr, nullptr, pr_old_gid, pr_count, plan); }
    void prune_unstage() { pr_count = -1; }
    // hgx_diff_wire (hgx_diff.hip): graph `graph`'s events with Index > known[creator]
    // in gid order, as wire columns (host pointers, null = not wanted; `rows` entries each are
    // filled, rows <= expect = the host plan's total; rows = 0 launches nothing). known / root_index:
    // n entries. *dev_total = the device's own count: unless it equals expect (a bug the caller
    // reports) no column is written. Changes nothing but scratch.
    struct DiffCols {
        int64_t *gid, *index, *spi, *opi, *ts;
        int32_t *creator, *opc, *ntx, *nil;
        uint8_t *hash, *S, *root;
    };
    // body (hgx_diff_wire_bodies, may be null): R and the transactions of the same rows from the body
    // store, gathered behind the selection; then no column is written unless they fit body->out.
    struct DiffBodies {
        BodyOut out{};
        int64_t n_tx = 0, n_bytes = 0;
        BodyFit fit = kBodyShort;
        bool ran = false;
    };
    hipError_t diff_wire(int graph, const int32_t* known, const int32_t* root_index, int64_t rows, int64_t expect,
                         const DiffCols& out, int64_t* dev_total, DiffBodies* body = nullptr);
    // chain lengths at the last DivideRounds (events past them have no round yet)
    int32_t len_div(int chain) const { return laid_out && chain < (int)h_len_div.size() ? h_len_div[(size_t)chain] : 0; }
    // per-event columns (gid order) for the host-side getters
    hipError_t get_events(std::vector<int32_t>& creator, std::vector<int32_t>& index, std::vector<int32_t>& sp,
                          std::vector<int32_t>& op);
    hipError_t get_event_fields(int64_t gid, int64_t* ts, int32_t* ntx, int32_t* tx_nil);
    // event ids (Event.Hash) of events [first, first + count): only when every inserted event
    // brought its id (hgx_events; an hgx_events32 insert brings the coin byte alone)
    bool ids_known = true;
    hipError_t get_ids(int64_t first, int64_t count, uint8_t* out32);
    hipError_t get_keys(uint8_t* out65);   // the participants' keys (hgx_set_participant_keys)
    // every column of the inserted events (gid order) for a checkpoint (hgx_save)
    hipError_t get_columns(std::vector<int32_t>& creator, std::vector<int32_t>& index, std::vector<int32_t>& sp,
                           std::vector<int32_t>& op, std::vector<int64_t>& ts, std::vector<uint8_t>& S,
                           std::vector<uint8_t>& coin, std::vector<int32_t>& ntx, std::vector<uint8_t>& txnil);
    hipError_t divide_rounds(int64_t E, const std::vector<int32_t>& chain_len,
                             const std::vector<int32_t>& chain_base, RoundsHost& out);
    // The pipelined ingest of a large first batch (compact columns in host memory):
    // the creator column is copied first and gives the layout plan; the other structure columns
    // follow in pieces cut at time-segment boundaries, and each piece is inserted, laid out and its
    // segments' lastAncestors main pass launched while the later pieces still cross PCIe. taken =
    // false: nothing was inserted (the path does not apply, or a check failed and the context was
    // cleared) and the caller runs insert_split_begin on the same columns.
    // The copier goes on with the payload columns right behind the last piece (copy_payload: ts, coin,
    // ntx into the staging columns, S straight into g_S at gid 0), so PCIe does not idle while the call
    // finishes; taken = true leaves the payload in flight as payload_begin would. taken = false: the
    // copier has been joined, and whatever it wrote early is overwritten by the caller's payload_begin.
    hipError_t insert_pipe32(const HostCols& hc, int64_t count, InsertOut& out, bool& taken);
    static constexpr int kPipeSegMult = 2;   // time segments of a pipelined ingest over a serial rebuild's
    int pipe_pieces = 4;                // hgx_set_ingest_pipeline: 0 = always the serial path
    int64_t pipe_min = 4000000;         // ... batches of at least this many events
    int pipe_used = 0;                  // pieces of the last insert_and_run32 (0: serial)
    // fame of the witnesses of rounds >= r0 (the first undecided round); rows below stay 0
    hipError_t decide_fame(int32_t r0, std::vector<int8_t>& fame_out);
    // the same in two halves: the kernel and the staged read-back queued (no wait), then the wait
    // and the rows' copy into fame_out (the same vector, untouched in between); the caller's
    // bookkeeping runs between the two
    // defer_rows (set before a divide_rounds, cleared by it): the call returns with the round tables'
    // rows still in the staging (last_round, R and r_lo are final); divide_rounds_rows copies them out,
    // after decide_fame_launch and before anything reads RoundsHost::bm / wflag
    bool defer_rows = false;
    void divide_rounds_rows(RoundsHost& out);
    hipError_t decide_fame_launch(int32_t r0, std::vector<int8_t>& fame_out);
    hipError_t decide_fame_wait();
    // round received etc. for the events not yet received; r0 / max_unrecv from recv_round_lo
    hipError_t find_order(const std::vector<uint8_t>& elig, const std::vector<uint8_t>& famous,
                          const std::vector<uint8_t>& ur_empty, int32_t r0, int max_unrecv, OrderHost& out);
    int32_t recv_round_lo(const RoundsHost& rh, int& max_unrecv) const;
    // the same in two halves around the shard exchange of a row-sharded graph:
    // begin = threshold, roundReceived, consensus timestamps of chains [shard_lo, shard_hi);
    // end = sort and blocks
    hipError_t find_order_begin(const std::vector<uint8_t>& elig, const std::vector<uint8_t>& famous,
                                const std::vector<uint8_t>& ur_empty, int32_t r0, int max_unrecv, OrderHost& out);
    hipError_t find_order_end(OrderHost& out, int32_t* order_dst = nullptr);
    int64_t shard_values(int lo, int hi) const;   // newly received events of chains [lo, hi)
    // their consensus timestamps to (to_buf) or from buf, a device or host pointer
    hipError_t shard_copy(int lo, int hi, void* buf, bool on_device, bool to_buf);
    int shard_lo = 0, shard_hi = 0;               // chains whose consensus timestamps this context computes
    // Roots (hgx_reset): per chain Root.Round and whether Root.Y is an event outside the store;
    // genesis roots (Round -1, Y "") when not rooted
    hipError_t set_roots(const std::vector<int32_t>& round, const std::vector<uint8_t>& y_ext);
    hipError_t set_root_others(const uint8_t* keys32, int64_t count);   // Root.Others keys (event ids)
    bool others_trust = false;   // checkpoint replay: Root.Others codes accepted without a key
    bool rooted = false;
    int root_gmax = -1;   // max Root.Round + 1 (rounds that root floors can force), -1 unrooted
    // smallest gid of a witness of each round in [r0, R) (UndecidedRounds order after a Reset)
    hipError_t round_first_gids(int32_t r0, std::vector<int32_t>& out);
    // D2H of order[first, first+count) of the last find_order (async; then sync())
    hipError_t copy_order(int32_t* dst, int64_t first, int64_t count);
    hipError_t sync() { return hipStreamSynchronize(stream); }

    hipError_t reset_received();
    // per-round tables reserved for `rounds` rounds (testing: a small value forces the growth path)
    hipError_t reserve_rounds(int32_t rounds);
    hipError_t get_rounds(std::vector<int32_t>& round_by_gid);
    hipError_t get_received(std::vector<int32_t>& rr, std::vector<int64_t>& cts);
    hipError_t get_coords(int64_t gid, int32_t* la, int32_t* fd);

    int n = 0, G = 0, C = 0, sm = 0, nw = 1;
    int64_t cap = 0, E = 0, E_div = 0;   // E_div: events laid out by the last divide_rounds
    int64_t Ppos = 0;                    // chain-major positions (events + per-chain slack)
    bool incremental = true;             // hgx_set_incremental(0): every DivideRounds rebuilds
    bool last_rebuild = false;           // the last divide_rounds rebuilt the layout
    int32_t R = 0;
    int la_sweeps = 0;
    int la_kernel = 0;            // 0 dataflow wavefront (k_la_wave) where it applies, 1 sweeps (hgx_set_la_kernel)
    bool la_wave_used = false;    // the last DivideRounds built lastAncestors with k_la_wave
    int la_wave_segs = 1;         // ... on this many time segments
    int la_segs_override = 0;     // > 0: time segments of a rebuild (hgx_set_la_kernel mode >= 2, measurement)
    int num_cus = 256;            // compute units of the device
    static constexpr int kLaMaxSegs = 16;
    static constexpr int kLaHeadRows = 64;   // rows per chain rebuilt at the start of each time segment
    static constexpr int kLaSegMinRows = 512;   // time segments only when the graph has >= this many rows per chain
    int64_t la_wave_fallbacks = 0;   // k_la_wave gave up and the sweeps redid the pass
    bool la_verified = false;        // the last time-segmented pass ran the verify sweep (its exactness check failed)
    bool la_verify_always = false;   // hgx_set_la_kernel(1026): the verify sweep after every segmented pass (tests)
    int compact = 0;             // coordinates of the last DivideRounds stored as uint16
    bool force_coord32 = false;  // hgx_set_coord_storage(1)
    int64_t la_rows = 0;   // rows recomputed over all sweeps of the last divide_rounds
    static constexpr int kLaSeg = 16;   // rows per lastAncestors unit
    hipStream_t stream = nullptr;
    double phase_ms[4] = {0, 0, 0, 0};   // coordinates, rounds, fame, order (last calls)
    KernelStat kstat[K_NUM];
    uint32_t time_mask = 0;   // kernels (bit = KernelId) timed with HIP events
    int fame_tally = 0;       // launch_fame tally (hgx_set_fame_tally)
    int round_kernel = 0;     // hgx_set_round_kernel: 0 persistent recurrence on rebuilds where it applies (3: every call),
                              // else per-launch per-candidate steps; 1 block-search steps; 2 per-candidate steps
    int cts_kernel = 0;       // hgx_set_cts_kernel: 0 auto (lane = event blocks on calls that receive >= 8 tiles per
                              // chain, else 1), 1 per-tile blocks, 2 pipelined, 3 lane = event, 4 the same with one staged row
    int64_t cts_row_runs = 0; // FindOrders whose timestamps ran on k_cts_row
    int64_t round_g_runs = 0;   // whole-graph recurrence launches (n <= 16)
    // shard `shard` of a chain-sharded group (nullptr: not sharded)
    ShardGroup* grp = nullptr;
    int shard = 0;
    // the round outputs of this shard's chains (Bm rows [r_a, r_b], S rows / witness flags [r_a,
    // min(r_b, capacity - 1)]) copied into every other shard's tables (after its launches)
    hipError_t share_round_rows(int32_t r_a, int32_t r_b);
    hipError_t capture_steps(StepGraph& sgr, const RoundArgs& args, int kern, int nb);
    bool la_small_used = false;   // the last DivideRounds built lastAncestors with k_la_small
    int la_small_override = -1;   // 0: never k_la_small (hgx_set_la_kernel 2), else where it applies
    bool sort_seg_enabled = true;      // FindOrder's bucketed sort (hgx_set_sort_kernel)
    int64_t sort_seg_runs = 0;         // FindOrders sorted by buckets
    bool round_pb_enabled = true;   // n > 256: k_round_pb (hgx_set_round_kernel 5 turns it off)
    int64_t round_p_runs = 0, round_p_fallbacks = 0;   // persistent launches / calls redone per launch
    int64_t round_p_ovf = 0;
    int32_t round_p_fail_round = -1, round_p_fail_chain = -1;   // the last give-up: round and chain   // candidate rows the persistent launches counted exactly (over 8 bits)
    int dev = 0;

   private:
    hipError_t ensure_round_cap(int32_t need);
    hipError_t insert_impl(const InsertIn& in, int64_t count, InsertOut& out, const unsigned long long* fail_sig,
                           int commit_mode = kCommitAll);
    // insert_bodies' chunk loop; wire: the parent columns carry window descriptors (insert_wire_bodies);
    // claimed: the flat id pass against these claimed ids in place of the level plan and k_ev_ids
    struct WireRun {
        const int32_t* win;   // the filled window (device)
        int64_t slots;
        int64_t *out_sp, *out_op;
    };
    struct SignOut {   // the signing path: where the accepted prefix's R and S go (host, may be null)
        uint8_t *out_r, *out_s;
    };
    hipError_t insert_bodies_run(const BodiesIn& ev, const std::vector<int64_t>& txi, int64_t count,
                                 const uint8_t* op_id32, uint8_t* out_id32, InsertOut& out, const WireRun* wire,
                                 const SignOut* sign = nullptr, const uint8_t* claimed = nullptr);
    hipError_t wipe_signing_keys();
    DBuf<uint8_t> sk_keys;   // [C][32] the private keys (HBM only: never saved, exported or stored with bodies)
    hipStream_t stream2 = nullptr;   // payload copies of insert_split (created on first use)
    // the pipelined ingest: stream_p and stream_o take the pieces' k_la_wave launches in turn
    int rebuild_segments(int64_t En, int coord_compact) const;
    hipStream_t stream_p = nullptr;
    hipEvent_t ev_pc[kPipeMaxPieces + 1] = {}, ev_lay[kPipeMaxPieces] = {}, ev_side[2] = {};
    std::atomic<int> pipe_stage{0};   // 1: the creator column issued and ev_pc[0] recorded, k + 2: piece k
    std::atomic<int> pipe_stop{0};
    std::thread pipe_thread;
    hipError_t pipe_err = hipSuccess;
    DBuf<int32_t> pipe_buf;           // [0] the gate word, [64 ..) the histogram, then the pieces' chain lengths
    std::vector<int32_t> pipe_hist, pipe_lim, pipe_off;
    bool pipe_ready = false;          // layout and main pass done for pipe_En / pipe_nts / pipe_off / pipe_compact
    int64_t pipe_En = 0;
    int pipe_nts = 0, pipe_compact = 0;
    // the form of the split batch in flight, set with its structure (a packed batch is compact once
    // decoded); payload_commit reads the staging columns it names
    enum Flight { kFlightNone, kFlightWide, kFlightCompact } flight = kFlightNone;
    hipError_t payload_streams();    // stream2, ev_pay and ev_pay_S, created on first use
    // the payload copier's body, on the copier's thread behind its hipSetDevice (e: that thread's
    // error so far; stop: a flag that ends it at the next column, or null)
    hipError_t copy_payload(const HostCols& hc, size_t c, size_t E0, hipError_t e, const std::atomic<int>* stop);
    hipError_t stage_buf(ColId id, size_t bytes, void*& p);   // the column's staging buffer, of at least `bytes`
    void read_insert_state(InsertOut& out) const;             // h_ins, once the stream has been synchronized
    hipEvent_t ev_pay = nullptr;
    // the S column is copied last, straight into g_S: only FindOrder's sort reads it, so DecideFame
    // and the first FindOrder kernels run while it crosses PCIe (payload_wait_S before the sort)
    hipEvent_t ev_pay_S = nullptr;
    std::atomic<int> pay_stage{0};   // 1: ts / coin / ntx (/ hash / nil) issued and ev_pay recorded
    bool pay_S_pending = false;
    bool pay_commit_pending = false;   // the payload in flight is not committed yet (payload_commit)
    int64_t pay_E0 = 0, pay_m = 0;     // ... its events: gids [pay_E0, pay_E0 + pay_m)
    bool fame_pending = false;         // decide_fame_launch without its decide_fame_wait
    bool rows_pending = false;         // divide_rounds left its rows in the staging (defer_rows)
    size_t rows_n = 0;                 // ... the first rows_n entries of stage_out
    std::thread pay_thread;
    hipError_t pay_err = hipSuccess;
    hipError_t pay_err_a = hipSuccess;   // the compact payload's first stage (before pay_stage = 1)
    InsertState insert_state();
    void kbeg(int k, bool sample = true, int64_t count = 1);
    void kend(int k, double bytes);
    void kadd_bytes(int k, double bytes);
    hipError_t collect_kernel_times();
    DevArrays arrays();

    int max_len = 0;
    bool laid_out = false;
    std::vector<int32_t> h_off;        // [C+1] chain slots (positions), fixed until a rebuild
    std::vector<int32_t> h_len_div;    // [C] chain lengths at the last divide_rounds
    std::vector<int32_t> h_fu;         // [C] events of each chain received so far (a prefix)
    int32_t fo_m = 0;                  // events received by the FindOrder in progress
    std::vector<int32_t> fo_cnt;       // [C] ... per chain
    DBuf<int32_t> root_round_d, gfl, gB, rfirst;   // roots: [C], per position floor, [(gmax+1) x C], [R]
    DBuf<uint8_t> root_y_ext_d;
    DBuf<uint64_t> others_d;   // [n_others][4] sorted Root.Others keys
    int64_t n_others = 0;
    DBuf<int32_t> sh_off;              // shard exchange: chain offsets
    DBuf<int64_t> sh_buf;              // ... and staging of host buffers
    // gid order
    DBuf<int32_t> g_creator, g_index, g_sp, g_op, g_ntx, g_rr, g_pos;
    DBuf<int64_t> g_ts, g_cts, g_ck;   // g_ck: (creator << 32) | chain offset (k_ck_pack, the layout's op lookups)
    DBuf<uint8_t> g_S, g_coin, g_loaded, g_txnil, g_id;
    // insert state (hgx_insert.hip)
    DBuf<uint32_t> succ, first_none;
    // small per-call tables in one block each, so that one copy moves them (views below):
    // [last_gid | last_index | chain_base | graph_loaded (8-byte)] read back after every insert
    // batch, [c_len | c_base | c_old] written before every DivideRounds
    DBuf<int32_t> ins_blk, cpar_blk;
    int32_t* h_ins = nullptr;    // pinned staging of ins_blk
    int32_t* h_cpar = nullptr;   // pinned staging of cpar_blk
    size_t ins_gl_off = 0;       // graph_loaded's offset in ins_blk (int32 units, even)
    DBuf<int32_t> last_gid_d, last_index_d, chain_base_d;
    DBuf<unsigned long long> ins_fail, graph_loaded_d;
    // host-batch staging (hgx_insert_events)
    DBuf<int32_t> st_creator, st_ntx, st_nil;
    DBuf<int64_t> st_index, st_sp, st_op, st_ts;
    DBuf<uint8_t> st_hash, st_S, st_dig, st_r;
    DBuf<int32_t> st_index32, st_sp32, st_op32;   // hgx_events32 columns
    DBuf<uint16_t> st_c16, st_spb, st_opb;        // hgx_events_packed columns
    DBuf<int64_t> st_exc_pos;
    DBuf<int32_t> st_exc_sp, st_exc_op;
    DBuf<uint8_t> st_coin;
    // hgx_prune_to_frame: the scan, the staged batch and the read-back tables (one block)
    DBuf<uint8_t> pr_buf;
    InsertIn pr_in{};
    int64_t pr_count = -1;   // events staged by prune_stage (-1: none)
    const int32_t* pr_old_gid = nullptr;   // ... their old gids (in pr_buf)
    // the staged frame's columns as one range of pr_buf (byte offsets, [creator, end)), with room behind them for hgx_get_frame_bodies' parent ids, flags and fail word
    struct PruneLayout {
        size_t creator = 0, index = 0, sp = 0, op = 0, ntx = 0, old = 0, ts = 0, hash = 0, S = 0, spid = 0, opid = 0,
               flags = 0, fail = 0, end = 0;
    } pr_lay;
    // hgx_diff_wire: known | root_index, the per-2 048-gid partials, then a 256-byte header (the
    // device's total) and the output columns, 121 bytes per returned row; the header and the
    // columns come back in one copy into df_host (page-locked). Both grown on demand.
    DBuf<uint8_t> df_buf;
    uint8_t* df_host = nullptr;
    size_t df_host_cap = 0;
    // batches of at most kPackEvents from host memory: the columns packed in one pinned buffer,
    // one H2D copy into st_pack
    static constexpr int64_t kPackEvents = 65536;
    hipError_t stage_pinned(const HostCols& hc, int64_t count, size_t* off);
    DBuf<uint8_t> st_pack;
    uint8_t* h_pack = nullptr;
    size_t h_pack_cap = 0;
    // signatures (Event.Verify): keys, window tables, per-event results, first failure
    DBuf<uint8_t> pk_keys, pk_valid, pk_out;
    DBuf<uint32_t> pk_tab;
    DBuf<unsigned long long> ins_fail_sig;
    // chains
    DBuf<int32_t> c_off, c_len, c_base, c_old, fu, rcnt;
    // positions
    DBuf<int32_t> p_gid, p_chain, p_op, p_opu, p_opk, p_round, p_rr;
    DBuf<int32_t> la_chg;   // [units] change stamps of the lastAncestors sweeps (sweep number)
    int32_t la_stamp = 1;   // stamp of the last sweep launched (monotone over calls)
    DBuf<int64_t> la_usum;  // [units] sum of each unit's values (change detection)
    DBuf<int64_t> p_ts, p_cts;
    // coordinates
    DBuf<int32_t> LA, FDT;   // int32 storage; uint16 views when `compact`
    int64_t fd_ld = 0;       // FDT row stride (coordinates): cap rounded up to even
    // per round
    int32_t r_cap = 0;
    DBuf<int32_t> Bm, WLA, WFD, WLAT, Tthr, active, lr;
    hipEvent_t flag_ev[2] = {nullptr, nullptr};
    static constexpr int kLaRing = 8, kLaAhead = 3;   // lastAncestors sweeps queued ahead of the check
    hipEvent_t la_ev[kLaRing] = {};
    StepGraph step_g[3];   // [0] full DivideRounds, [1] / [2] resumed (incremental) calls of 2 / 4 steps
    void drop_step_graph();
    // The words of `counters` (device) and of h_small (pinned, where the host reads results), in ints.
    // A sweep's ring slot holds 4 ints: rows recomputed, units changed, two spare.
    static constexpr int kCtRecv = 0;       // FindOrder: events received, [+1] the panic flag
    static constexpr int kCtWaveErr = 6;    // a k_la_wave / k_la_small lane gave up
    static constexpr int kCtSweep = 8;      // the sweeps' ring [kLaRing][4]
    static constexpr int kCtWords = kCtSweep + 4 * kLaRing;
    static constexpr int kHsInsFail = 0;    // insert: the first-failure word (8 bytes)
    static constexpr int kHsInsFailSig = 2; // ... and the signatures' (8 bytes)
    static constexpr int kHsRecv = 0;       // FindOrder's received / panic pair, in the insert's words: every
                                            // call reads its own before it returns, and calls do not overlap
    static constexpr int kHsSweep = 16;     // the sweeps' ring [kLaRing][4] (rows and changed are copied)
    static constexpr int kHsWaveErr = kHsSweep + 4 * kLaRing;
    static constexpr int kHsSegCheck = 50;  // the time segments' exactness check
    static constexpr int kHsRoundSt = 56;   // the four status words of a recurrence launch
    static constexpr int kHsWords = 64;
    static_assert(kCtRecv + 2 <= kCtWaveErr && kCtWaveErr < kCtSweep, "counters: ranges overlap");
    static_assert(kHsInsFail + 2 <= kHsInsFailSig && kHsInsFailSig + 2 <= kHsSweep && kHsRecv + 2 <= kHsSweep,
                  "h_small: the insert's / FindOrder's words reach the sweep ring");
    static_assert(kHsWaveErr < kHsSegCheck && kHsSegCheck < kHsRoundSt && kHsRoundSt + 4 <= kHsWords,
                  "h_small: ranges overlap or leave the block");

    // ---- DivideRounds (hgx_engine_divide.cpp): divide_rounds runs these phases in order; they share the
    // call's state through one DivCall on its stack
    struct DivCall {
        int64_t En;
        const std::vector<int32_t>&chain_len, &chain_base;
        RoundsHost& out;
        const DividePlan& plan;
        bool sweeps_only;              // the second attempt: lastAncestors by the sweeps
        DevArrays a{};                 // re-taken by whoever grows a table
        const int32_t* cold = nullptr; // the chains' old lengths (device) on a resumed call
        const int32_t* la_map = nullptr;
        bool piped = false;            // the pipelined ingest laid out and ran the segments' main pass
        bool side_commit = false;      // the payload's commit is in flight on the side stream
        RoundChoice rc{};
        int32_t r_done = -1;           // a recurrence wrote rounds [r_lo, r_done) (the last one empty)
        int launched = 0, checked = 0; // step batches queued / whose flag the host has read
        bool tail_ready = false;       // the tail queued behind the first batch stands
        bool la_flag_read = false;     // the wavefront's error word is queued with the tail (once)
        bool one_trip() const { return !plan.rebuild; }
        int32_t r_scan() const { return plan.rebuild ? 0 : plan.r_lo; }
    };
    DividePlan div_plan;   // (its lane map keeps its capacity over the calls)
    hipError_t divide_attempt(DivCall& d);
    hipError_t div_layout(DivCall& d);
    hipError_t div_last_ancestors(DivCall& d);
    hipError_t div_coordinates(DivCall& d);
    hipError_t run_sweeps(DivCall& d, int first_mode);
    hipError_t fd_then_floors(DivCall& d, const int32_t* cold, int max_new, int d_lo, int d_hi, bool floors, bool timed);
    hipError_t div_rebuild_wait(DivCall& d);
    hipError_t div_round_tables(DivCall& d);
    RoundArgs round_args() const;
    enum RecurKind { kRecurGraph, kRecurPersistent };
    struct PersistentSetup;
    hipError_t persistent_setup(DivCall& d, PersistentSetup& ps);
    hipError_t persistent_launch(const PersistentSetup& ps, int32_t* fin, int32_t s, int init);
    hipError_t persistent_share(int32_t s, int32_t st[4]);
    hipError_t run_recurrence(DivCall& d, RecurKind kind);
    hipError_t div_recurrence(DivCall& d);
    hipError_t launch_batch(DivCall& d);
    hipError_t div_steps(DivCall& d);
    hipError_t enqueue_tail(DivCall& d, int32_t r_hi);
    hipError_t div_finish(DivCall& d);
    DBuf<uint8_t> wflag, wstat, wcoin, elig, fw, ur_empty;
    DBuf<uint64_t> Smat, Vbuf;
    DBuf<uint32_t> FD8;   // [2][C][ndw] rebased candidate rows (k_round_k)
    DBuf<uint32_t> FD8p;  // [kRoundPBufs][C][ndw] the same, row-major, self-validating (k_round_p)
    DBuf<uint64_t> rp_gran;   // [4][C] k_round_p hand-off granules
    DBuf<int32_t> rp_st;      // k_round_p status: abort, rounds done, finished
    DBuf<uint32_t> seg_off, seg_cur;   // the segmented order sort's bucket starts / cursors
    DBuf<int32_t> rp_amap;    // k_round_pb: the chains with events
    std::vector<int32_t> h_amap;
    DBuf<uint8_t> rp_win;     // a chain-sharded group's RoundPWindows (device copy read by k_round_p)
    DBuf<int32_t> la_lmap;          // k_la_wave lanes -> chains with events (one graph, n > 896)
    DBuf<int32_t> la_chk;           // k_la_seg_check: [0] flag, then the segments' first rows [(nts + 1) x n]
    DBuf<int32_t> ovf;    // [r_cap + 2]
    DBuf<int8_t> fame;
    // order
    DBuf<int32_t> recv_list, counters, order_gid, blk_cnt, blk_loaded;
    DBuf<uint8_t> blk_nil;
    DBuf<uint32_t> scan_part;
    DBuf<uint64_t> key_a, key_b;
    DBuf<uint32_t> val_a, val_b, hist;
    DBuf<int64_t> minmax, blk_ntx;
    int32_t* h_small = nullptr;   // pinned scratch (flags)
    // pinned staging of the per-call host tables (instead of pageable copies): a cursor per
    // phase; D2H copies land here and are handed out by stage_flush() after the phase's sync.
    // The copies are queued and stage_issue() sends them: up to kCopyMax small ones (together
    // at most kCopyKernelMax bytes) as ONE k_copy_many launch, otherwise one DMA copy each
    uint8_t* h_stage = nullptr;
    uint8_t* d_stage = nullptr;   // its device address
    size_t stage_cap = 0, stage_used = 0;
    struct StagedD2H { void* dst; size_t off, bytes; };
    std::vector<StagedD2H> stage_out;
    // kind 0: stage -> dev (H2D), 1: dev -> stage (D2H), 2: dev -> pinned host (host_dst, its
    // device address dev_dst), 3: pinned host (host_src, its device address dev_src) -> dev
    struct PendCopy {
        int kind;
        size_t off;
        const void* dev;
        void* host_dst;
        void* dev_dst;
        size_t bytes;
        const void* host_src = nullptr;
        const void* dev_src = nullptr;
        int reset = -1;   // kind 2: the device bytes are set to this value once copied
    };
    std::vector<PendCopy> pend;
    static constexpr size_t kCopyKernelMax = 256 << 10;
    hipError_t stage_reserve(size_t bytes);
    hipError_t stage_h2d(void* dev, const void* host, size_t bytes);
    hipError_t stage_d2h(void* host, const void* dev, size_t bytes);
    hipError_t copy_to_pinned(void* pinned_dst, const void* dev, size_t bytes, int reset = -1);   // queued like the stagings
    hipError_t copy_from_pinned(void* dev, const void* pinned_src, size_t bytes);
    hipError_t stage_issue();
    void stage_flush();   // after the stream synchronized: copy the D2H tables out, reset the cursor
    // the bucket sort's parts (find_order_end): bucket counts read back with the timestamp range, the
    // order's D2H copies on their own stream behind each part
    static constexpr int kOrderParts = 4;
    static constexpr size_t kOrderPipeMin = 16u << 20;   // order bytes from which the parts pay
    uint32_t* h_segc = nullptr;
    size_t h_segc_n = 0;
    hipStream_t stream_o = nullptr;
    hipEvent_t ev_o[kOrderParts + 1] = {};
    int32_t* h_flag = nullptr;    // host-mapped, coherent: the round-step batches' "candidates left" flags
    int32_t* d_flag = nullptr;    // its device address
    // timing
    hipEvent_t ph0 = nullptr, ph1 = nullptr, ph2 = nullptr;
    std::vector<int32_t> h_lr;   // DivideRounds: every graph's last round (staged copy)
    std::vector<hipEvent_t> kev;
    struct Open { int k; size_t e0; double bytes; int64_t count; };
    std::vector<Open> kopen;
    size_t kev_used = 0;

   public:
    // The event-id index (hgx_keep_id_index, hgx_idindex.hip / hgx_idindex.h): an
    // open-addressing table over g_id, kept behind every insert() / insert_verified() that leaves ids_known
    // true (idx_append: one launch over the events not yet indexed, [idx_done, E); the lookups run it
    // first, which covers a split insert), emptied by clear() and so rebuilt by a prune's or a
    // bootstrap's re-insert. It is valid exactly while ids_known. Nothing below is
    // allocated or launched on a context that never called idx_keep.
    hipError_t idx_keep();
    hipError_t idx_zero();
    hipError_t idx_append();
    // out: hgx_id_index_state's five fields; *corrupt: a probe met no empty slot (a bug, or a table
    // overwritten from outside)
    hipError_t idx_state(int64_t out[5], bool* corrupt);
    hipError_t idx_find(const uint8_t* id32, int64_t m, int64_t* out_gid, bool* corrupt);
    // hgx_insert_events_by_id: the batch's parents' ids (host columns; sp_id32 / op_id32 may be null when
    // no flag names them) resolved to gids and root codes in out_sp / out_op (host, count entries each)
    hipError_t idx_resolve(const uint8_t* claimed_id32, const uint8_t* sp_id32, const uint8_t* op_id32,
                           const uint8_t* flags, const int32_t* creator, int64_t count, int64_t* out_sp, int64_t* out_op,
                           bool* corrupt);
    bool idx_kept = false;
    uint64_t idx_slots = 0;
    int64_t idx_done = 0;      // events [0, idx_done) are in the table
    DBuf<uint64_t> idx_tab;    // [idx_slots]
    DBuf<uint64_t> idx_st;     // the status block: the sticky corrupt flag and the statistics
    DBuf<uint8_t> idx_buf;     // scratch of a find or a resolve (queries, the batch's table and columns)
    hipError_t idx_read_flag(bool* corrupt);
};

}  // namespace hgx
