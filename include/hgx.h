/*
 * hgx.h -- C ABI of the MI355X-native Hashgraph consensus engine (libhgx.so).
 *
 * Drop-in boundary for the reference's consensus hot path (datatypevoid/babble
 * v0.2.0, package hashgraph). A thin cgo shim keeps the Go API
 *   (*Hashgraph).InsertEvent(Event, bool) error   hashgraph/hashgraph.go:356
 *   (*Hashgraph).DivideRounds() error             hashgraph/hashgraph.go:616
 *   (*Hashgraph).DecideFame() error               hashgraph/hashgraph.go:649
 *   (*Hashgraph).FindOrder() error                hashgraph/hashgraph.go:801
 * and the exported state Core reads (UndeterminedEvents, PendingLoadedEvents,
 * LastConsensusRound, LastCommitedRoundEvents, ConsensusTransactions;
 * hashgraph.go:15-37, node/core.go:335-369), mapping event hex ids to dense ids.
 *
 * Conventions
 *  - Events get dense ids ("gid") in insertion order (the reference's
 *    topologicalIndex, hashgraph.go:373). A parent that is "" is -1; a parent
 *    hash the shim cannot resolve is HGX_UNKNOWN_PARENT.
 *  - Participants are ids 0..n-1 (Hashgraph.Participants, hashgraph.go:16).
 *    A batched context holds n_graphs independent hashgraphs; graph g owns
 *    participant ids [g*n, (g+1)*n).
 *  - All input arrays are copied before the call returns; no caller pointer is
 *    retained (cgo pointer rules). Output arrays are caller-allocated.
 *  - Every entry point returns HGX_OK (0) or an error code; the message of the
 *    last error is written to hgx_error.msg verbatim as the Go error string.
 *  - A context is single-caller (the reference serialises calls under
 *    node.coreLock, node/node.go:226-237); it owns one HIP stream.
 *  - The library fails loudly (HGX_ERR_DEVICE) when no gfx950 device is usable:
 *    there is no CPU fallback.
 */
#ifndef HGX_H
#define HGX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HGX_ABI_VERSION 6   /* (still 6 with hgx_insert_event_bodies(_ext), hgx_set_root_ids, hgx_event_json_batch and hgx_batch_levels,
                                 with hgx_prune_to_frame, hgx_get_root_ids and hgx_get_root_others, with hgx_diff_wire, and
                                 with hgx_insert_wire_bodies, and with hgx_keep_bodies and its consumers
                                 (hgx_get_event_bodies, hgx_block_transactions, hgx_get_block_hash,
                                 hgx_block_hash_batch, hgx_diff_wire_bodies), and with the signer
                                 (hgx_p256_sign_batch, hgx_p256_public_keys, hgx_set_signing_keys,
                                 hgx_sign_insert_event_bodies), and with the event-id index
                                 (hgx_keep_id_index, hgx_id_index_state, hgx_find_events,
                                 hgx_insert_events_by_id), and with hgx_get_frame_bodies (hgx_frame_out):
                                 purely additive, no existing entry or structure changed)
                              6: hgx_host_alloc / hgx_host_free (page-locked caller buffers);
                              5: hgx_events_packed (hgx_insert_events_packed, hgx_insert_and_run_packed,
                                 hgx_pack_events32);
                              4: hgx_create_sharded (chain-sharded recurrence over devices);
                              3: HGX_ROOT_OTHER needs its key registered (hgx_set_root_others) */

/* Error codes. 1..5 mirror common.StoreErrType + 1 (common/errors.go:7-13). */
enum {
    HGX_OK = 0,
    HGX_ERR_KEY_NOT_FOUND = 1,  /* "%s, Not Found"        errors.go:27 */
    HGX_ERR_TOO_LATE = 2,       /* "%s, Too Late"         errors.go:29 */
    HGX_ERR_PASSED_INDEX = 3,   /* "%s, Passed Index"     errors.go:31 */
    HGX_ERR_SKIPPED_INDEX = 4,  /* "%s, Skipped Index"    errors.go:33 */
    HGX_ERR_NO_ROOT = 5,        /* "%s, No Root"          errors.go:35 */
    HGX_ERR_SELF_PARENT = 100,  /* "CheckSelfParent: Self-parent not last known event by creator" hashgraph.go:366,416 */
    HGX_ERR_OTHER_PARENT = 101, /* "CheckOtherParent: Other-parent not known" hashgraph.go:370,441 */
    HGX_ERR_INVALID = 102,      /* bad argument to the C ABI itself */
    HGX_ERR_CAPACITY = 103,     /* context capacity exceeded */
    HGX_ERR_SIGNATURE = 104,    /* "Invalid signature" hashgraph.go:358-363 (Event.Verify false) */
    HGX_ERR_DEVICE = 200,       /* HIP error / no gfx950 device */
    HGX_ERR_PANIC = 300         /* the reference would panic here (e.g. UndecidedRounds[0] on empty) */
};

#define HGX_UNKNOWN_PARENT (-2)
/* After hgx_reset, other-parents outside the store that CheckOtherParent accepts through the
 * creator's Root (hashgraph.go:430-440): */
#define HGX_ROOT_Y (-3)       /* Root.Y (the creator's first event, self-parent = Root.X = -1) */
#define HGX_ROOT_OTHER (-4)   /* Root.Others[event]: the event's hash must be a key registered with
                                 hgx_set_root_others (the caller checked the entry's value; on the
                                 body path, hgx_insert_event_bodies_ext, the device checks it) */

typedef struct {
    int32_t code;
    char msg[252];
} hgx_error;

typedef struct hgx_ctx hgx_ctx;

/* Event batch, structure of arrays, `count` entries each (hashgraph/event.go:14-76). */
typedef struct {
    const int32_t* creator;       /* participant id (global id in a batched ctx) */
    const int64_t* index;         /* Body.Index */
    const int64_t* self_parent;   /* gid, -1 for "" */
    const int64_t* other_parent;  /* gid, -1 for "", HGX_UNKNOWN_PARENT if not known */
    const int64_t* timestamp_ns;  /* Body.Timestamp as Unix ns (UTC) */
    const uint8_t* hash;          /* 32 bytes per event: SHA-256 event id (Event.Hash) */
    const uint8_t* sig_s;         /* 32 bytes per event: signature S, big-endian, zero-padded */
    const int32_t* ntx;           /* len(Body.Transactions) */
    const int32_t* tx_nil;        /* 1 if Body.Transactions == nil */
} hgx_events;

/* ---- lifecycle ------------------------------------------------------------ */
int32_t hgx_abi_version(void);
/* NewHashgraph(participants, store, ...) (hashgraph.go:39-66) with an InmemStore of
 * cacheSize >= capacity_events (no eviction). device = HIP device ordinal. The context pins
 * 4 bytes of host memory per event of capacity (at most 64 MB up front, grown on demand) for
 * the consensus order, which FindOrder writes there directly. */
hgx_ctx* hgx_create(int32_t n_participants, int64_t capacity_events, int32_t device, hgx_error* err);
/* n_graphs independent hashgraphs of n_participants each (seed-sharded simulations) */
hgx_ctx* hgx_create_batch(int32_t n_graphs, int32_t n_participants, int64_t capacity_events,
                          int32_t device, hgx_error* err);
/* One graph whose round recurrence is chain-sharded over n_shards devices (the north star's
 * single-graph mode; no reference counterpart: the Go Hashgraph is one object on one
 * core). devices[k] = shard k's HIP device (ordinals may repeat: shards that share a device need
 * GPU_MAX_HW_QUEUES >= shards on it + 2, set before the HIP runtime starts); shard 0 is the returned
 * context. Every shard holds the whole DAG (inserts, lastAncestors, fame, round received, sort:
 * replicated); shard k owns chains [C k / W, C (k + 1) / W): it builds their events'
 * firstDescendants, runs their workgroups of the persistent recurrence (writing each candidate row and
 * granule write-through into every shard's window, over the peer mapping when the shard lies on
 * another device) and their events' consensus timestamps, which FindOrder exchanges device to device.
 * The drop-in calls and getters work as on one context, with the same results; n <= 256, one graph;
 * hgx_reset, hgx_bootstrap, verified and wire inserts, hgx_set_shard and the public FindOrder halves
 * return HGX_ERR_INVALID on it. */
hgx_ctx* hgx_create_sharded(int32_t n_participants, int64_t capacity_events, int32_t n_shards,
                            const int32_t* devices, hgx_error* err);
void hgx_destroy(hgx_ctx* ctx);

/* ---- the four drop-in calls ------------------------------------------------ */
/* InsertEvent(e, true) for each event in order (hashgraph.go:356-401); stops at the first
 * failure like Core.Sync (node/core.go:199-211): *n_inserted = events accepted, err = the
 * Go error of the first rejected event. The batch is copied to HBM and validated there
 * (CheckSelfParent :404-420, CheckOtherParent :423-445, RollingIndex.Add
 * common/rolling_index.go:54-68) by data-parallel kernels; a whole Core.Sync batch is one call.
 * Event.Verify (the signature) stays with the caller. */
int32_t hgx_insert_events(hgx_ctx* ctx, const hgx_events* ev, int64_t count, int64_t* n_inserted,
                          hgx_error* err);
/* The compact form of the same batch (61 instead of 108 bytes per event cross PCIe): Index and
 * parents as int32 (gids are < 2^31 by hgx_create's capacity), the one byte of the event id that
 * consensus reads instead of the 32-byte id, and len(Body.Transactions) with -1 for nil. */
typedef struct {
    const int32_t* creator;       /* participant id (global id in a batched ctx) */
    const int32_t* index;         /* Body.Index */
    const int32_t* self_parent;   /* gid, -1 for "" */
    const int32_t* other_parent;  /* gid, -1 for "", HGX_UNKNOWN_PARENT / HGX_ROOT_Y as in hgx_events */
    const int64_t* timestamp_ns;  /* Body.Timestamp as Unix ns (UTC) */
    const uint8_t* coin;          /* 1 byte per event: middleBit (hashgraph.go:1039-1048), i.e. byte 16 of
                                     Event.Hash() is not 0 -- the coin of DecideFame's coin rounds */
    const uint8_t* sig_s;         /* 32 bytes per event: signature S, big-endian, zero-padded */
    const int32_t* ntx;           /* len(Body.Transactions); -1 if Body.Transactions == nil */
} hgx_events32;
/* hgx_insert_events / hgx_insert_and_run with hgx_events32 host columns. Same results, errors and
 * counters. Not after hgx_reset (the Root.Others check reads the 32-byte id): HGX_ERR_INVALID. */
int32_t hgx_insert_events32(hgx_ctx* ctx, const hgx_events32* ev, int64_t count, int64_t* n_inserted, hgx_error* err);
int32_t hgx_insert_and_run32(hgx_ctx* ctx, const hgx_events32* ev, int64_t count, int64_t* n_inserted,
                             hgx_error* err);
/* The same batch with its structure columns in 10 instead of 16 bytes per event (what
 * validation and DivideRounds wait for; the payload columns are those of hgx_events32). Event k
 * of the batch gets gid base + k, base = hgx_num_events(ctx) at the call. A parent is stored as
 * its distance back from that gid: 0 = "" (-1), 1..65534 = gid base + k - d, HGX_PARENT_ESCAPE =
 * the event's entry in the exception list (exc_pos: batch positions, distinct, any order;
 * exc_self_parent / exc_other_parent: both parents as hgx_events32 holds them, HGX_UNKNOWN_PARENT
 * included). An escaped parent without an entry reads as HGX_UNKNOWN_PARENT. The columns are
 * decoded on the device into the hgx_events32 form, so results, errors and counters are those of
 * hgx_insert_events32 / hgx_insert_and_run32 on the decoded batch. hgx_pack_events32 builds them. */
#define HGX_PARENT_ESCAPE 0xFFFF
typedef struct {
    const uint16_t* creator;            /* participant id (global id in a batched ctx), < 65536 */
    const int32_t* index;               /* Body.Index */
    const uint16_t* self_parent_back;   /* distance back, 0 = "", HGX_PARENT_ESCAPE */
    const uint16_t* other_parent_back;
    int64_t n_exc;                      /* exception list (host memory) */
    const int64_t* exc_pos;
    const int32_t* exc_self_parent;
    const int32_t* exc_other_parent;
    const int64_t* timestamp_ns;        /* the payload columns, as in hgx_events32 */
    const uint8_t* coin;
    const uint8_t* sig_s;
    const int32_t* ntx;
} hgx_events_packed;
int32_t hgx_insert_events_packed(hgx_ctx* ctx, const hgx_events_packed* ev, int64_t count, int64_t* n_inserted,
                                 hgx_error* err);
int32_t hgx_insert_and_run_packed(hgx_ctx* ctx, const hgx_events_packed* ev, int64_t count, int64_t* n_inserted,
                                  hgx_error* err);
/* Host helper (no device): the packed structure columns of an hgx_events32 batch whose first
 * event will get gid `base`. Writes creator16 / sp_back / op_back (count each) and up to exc_cap
 * exceptions; *n_exc = the number needed (HGX_ERR_INVALID "exception list full" if > exc_cap,
 * HGX_ERR_INVALID "creator outside 0..65535" for a creator the form cannot hold). */
int32_t hgx_pack_events32(const hgx_events32* ev, int64_t count, int64_t base, uint16_t* creator16, uint16_t* sp_back,
                          uint16_t* op_back, int64_t* exc_pos, int32_t* exc_self_parent, int32_t* exc_other_parent,
                          int64_t exc_cap, int64_t* n_exc, hgx_error* err);
/* Page-locked host memory for the caller's event columns (Core's sync buffers, allocated once and
 * reused: C memory, so cgo may hand Go slices over it with unsafe.Slice). Every insert call accepts
 * pageable memory as well; from page-locked memory the column copies are DMA transfers at the host
 * link's rate instead of staged copies. NULL on failure or bytes <= 0; hgx_host_free(NULL) is a no-op.
 * Usable with a context on any device. */
void* hgx_host_alloc(int64_t bytes);
void hgx_host_free(void* p);
/* The same with every hgx_events column a DEVICE pointer on the context's device (events
 * decoded / hashed on the GPU, or a trace resident in HBM). hash and sig_s must be
 * 16-byte aligned. Synchronous: the columns may be reused when the call returns. */
int32_t hgx_insert_events_device(hgx_ctx* ctx, const hgx_events* ev, int64_t count, int64_t* n_inserted,
                                 hgx_error* err);
/* Participants' public keys for Event.Verify: C = graphs * n_participants entries of 65 bytes
 * (Body.Creator: the uncompressed P-256 point 0x04|X|Y, participant id order). The device
 * window tables are built once here. A key that is not a P-256 point is accepted; an event it
 * signs then fails as in the reference, where elliptic.Unmarshal returns nil and
 * ecdsa.Verify dereferences it: HGX_ERR_PANIC "runtime error: invalid memory address or nil
 * pointer dereference". */
int32_t hgx_set_participant_keys(hgx_ctx* ctx, const uint8_t* keys65, hgx_error* err);
/* InsertEvent including Event.Verify (hashgraph.go:356-363, event.go:142-152): every event's
 * signature (R = sig_r32, S = ev->sig_s, 32 bytes big-endian each) is checked on the device
 * against its creator's key (hgx_set_participant_keys) and its body digest digest32
 * (EventBody.Hash: SHA-256 of the body JSON, event.go:48-54; hgx_sha256_batch computes it),
 * in the same data-parallel pass as the parent checks. The batch stops at the first failing
 * event; at one event the signature's failure ("Invalid signature", HGX_ERR_SIGNATURE) comes
 * before its parent checks, as in the reference. Host pointers (copied to HBM), or device
 * pointers (_device). HGX_ERR_INVALID "participant keys not set" without keys. */
int32_t hgx_insert_events_verified(hgx_ctx* ctx, const hgx_events* ev, const uint8_t* digest32, const uint8_t* sig_r32,
                                   int64_t count, int64_t* n_inserted, hgx_error* err);
int32_t hgx_insert_events_verified_device(hgx_ctx* ctx, const hgx_events* ev, const uint8_t* digest32,
                                          const uint8_t* sig_r32, int64_t count, int64_t* n_inserted, hgx_error* err);
/* Event fields instead of event hashes (hashgraph/event.go:14-37): what a node holds after decoding
 * a sync batch, before any hashing. */
typedef struct {
    const int32_t* creator;       /* participant id; Body.Creator = that participant's 65-byte key */
    const int64_t* index;         /* Body.Index */
    const int64_t* self_parent;   /* gid, -1 for "" */
    const int64_t* other_parent;  /* gid, -1 for "" */
    const int64_t* timestamp_ns;  /* Body.Timestamp as Unix ns (UTC) */
    const uint8_t* sig_r;         /* 32 B big-endian each */
    const uint8_t* sig_s;
    const int32_t* ntx;           /* len(Body.Transactions), -1 for nil */
    const int64_t* tx_off;        /* T+1 byte offsets into tx_bytes, T = sum(max(ntx,0)); an event's
                                     transactions are consecutive entries, events in batch order */
    const uint8_t* tx_bytes;
} hgx_event_bodies;
/* InsertEvent including Event.Hash and Event.Verify (hashgraph.go:356-363, event.go:142-188), host
 * pointers: the device builds every event's Go-JSON (Event.Marshal), computes the event ids (SHA-256
 * of that text) level by level -- an event's text holds its parents' hex ids, so a batch is hashed in
 * dependency order (hgx_batch_levels) --, the body digests (EventBody.Hash), and hands both to the
 * verified insert. A parent's id comes from the store's id column for a gid below hgx_num_events and
 * from this batch for a later gid. Results, error strings, stop-at-first-failure and *n_inserted are
 * those of hgx_insert_events_verified on the same events with host-computed hash and digest32;
 * out_id32 (may be NULL) receives the ids of the accepted prefix, 32 bytes each, and
 * hgx_get_event_id works afterwards. Needs hgx_set_participant_keys. HGX_ERR_INVALID "<reason>":
 * bad columns (a NULL column, ntx < -1, decreasing tx_off: checked before anything else), keys not
 * set, the context's ids are not known (events came through hgx_events32 / packed inserts or an
 * id-less bootstrap), the context has roots whose ids are not known (after hgx_reset with roots or a
 * rooted hgx_bootstrap, until hgx_set_root_ids), or it is chain-sharded or row-sharded.
 * Deviation from the reference: an event whose creator has no key, or with a parent that is neither
 * -1 nor an earlier gid (HGX_UNKNOWN_PARENT included), has no id string, so no text. The batch is
 * cut before it, the prefix is inserted first (its first failure wins), then the event fails with
 * its parent check's Go error (CheckSelfParent / CheckOtherParent / "<creator>, Not Found") and
 * *n_inserted = its position; the reference would report "Invalid signature" first when its
 * signature is bad as well.
 * Scratch: the batch is processed in internal chunks of at most 65 536 events and 32 MiB of JSON
 * (8 bytes counted per transaction on top of its base64), so the scratch the context keeps is bounded
 * whatever the batch size: on the device 32 MiB of text, at most 24 MiB of transaction bytes and 32 MiB
 * of their offsets, and 220 bytes per event of a chunk for columns, level plan, ids and digests (under
 * 104 MiB in all); the same without the text in page-locked host memory. Only a single event whose
 * own text exceeds 32 MiB raises it, to that event's size. With other_parent_id32 (_ext) 32 bytes more
 * per event of a chunk on both sides: 252 bytes per event, under 106 MiB in all.
 * hgx_insert_event_bodies is hgx_insert_event_bodies_ext with other_parent_id32 = NULL. */
int32_t hgx_insert_event_bodies(hgx_ctx* ctx, const hgx_event_bodies* ev, int64_t count, uint8_t* out_id32,
                                int64_t* n_inserted, hgx_error* err);
/* The same on a context with roots (after hgx_prune_to_frame, or hgx_reset + hgx_set_root_ids;
 * DESIGN.md §3.12), where an event's Body.Parents may name events outside the store (hashgraph.go:404-445).
 * The parent codes print as
 *   self-parent -1   the creator's Root.X id, or "" where the root has none (has_x = 0);
 *   HGX_ROOT_Y       the creator's Root.Y id;
 *   HGX_ROOT_OTHER   that event's row of other_parent_id32 (32 bytes per event, host memory, read only
 *                    for this code; may be NULL);
 *   a gid            as above.
 * An HGX_ROOT_Y event whose creator's root has no Y, an HGX_ROOT_OTHER event without other_parent_id32
 * and any other negative code have no text: the batch is cut before them by the deviation rule above.
 * The device checks the Root.Others entry of every HGX_ROOT_OTHER event after its id is known: the id
 * must be a key of the roots' pairs (hgx_get_root_others) and the entry must equal the supplied id,
 * else the event fails with "CheckOtherParent: Other-parent not known" at its position (after "Invalid
 * signature" at the same event). On a context without roots the call equals hgx_insert_event_bodies
 * byte for byte. */
int32_t hgx_insert_event_bodies_ext(hgx_ctx* ctx, const hgx_event_bodies* ev, const uint8_t* other_parent_id32,
                                    int64_t count, uint8_t* out_id32, int64_t* n_inserted, hgx_error* err);
/* hgx_insert_event_bodies_ext for events that arrive with their ids: a checkpoint,
 * a Frame, or a Go Event out of a store, whose Body.Parents are hex strings. claimed_id32 (32 bytes per
 * event, host memory) is every event's CLAIMED id. The texts are built with the parents' claimed ids
 * (a parent below hgx_num_events from the store's id column, the root codes as in _ext), all of them are
 * hashed in ONE flat pass, one lane per event, with no dependency order, and every hash is compared with
 * the event's claimed id. If all agree every claimed id is the event's hash (induction in gid order: the
 * first event with a wrong claimed id has parents whose claimed ids are right, so its text is its true
 * text and its hash differs from the claim); hence the smallest mismatching position k is exact, events
 * [0, k) are proven and go through Event.Verify and the insert, and everything computed behind k is
 * dropped. Preconditions, refusals ("hgx_insert_event_bodies_claimed: <reason>"), the cut rule for
 * events without a text, the internal chunks, the scratch bound (32 bytes more per event of a chunk on
 * both sides; no level plan is built) and the resulting context state, body store included, are those of
 * hgx_insert_event_bodies_ext on the same events. One more outcome: HGX_ERR_INVALID
 * "hgx_insert_event_bodies_claimed: event <k>: the claimed id is not the event's hash", *n_inserted = k,
 * events [0, k) resident with their proven ids. First failure inside a call: a failure of the proven
 * prefix (its Go error: "Invalid signature", the parent and index checks) at a position j < k comes
 * first; at the same position the mismatch wins. claimed_id32 == NULL is HGX_ERR_INVALID. */
int32_t hgx_insert_event_bodies_claimed(hgx_ctx* ctx, const hgx_event_bodies* ev, const uint8_t* claimed_id32,
                                        const uint8_t* other_parent_id32, int64_t count, int64_t* n_inserted,
                                        hgx_error* err);
/* Event.Sign on the device. hgx_set_signing_keys: C = graphs * n_participants
 * private keys of 32 bytes (big-endian d), participant id order; 32 zero bytes = this participant does
 * not sign here (a real node holds one key); NULL clears. Needs hgx_set_participant_keys first (a later
 * hgx_set_participant_keys clears the signing keys). HGX_ERR_INVALID for a d >= N, and for a key whose
 * d G is not the participant's public key ("hgx_set_signing_keys: key <c> does not match participant
 * <c>'s public key"); nothing is changed then. The keys live in device memory only: they are zeroed
 * there when cleared, replaced or the context is destroyed, and never enter hgx_save / hgx_save_ex,
 * hgx_shard_export or the body store. Signing is NOT constant time (table lookups indexed by nonce
 * bytes): for a node that owns its GPU, or test nets.
 *
 * hgx_sign_insert_event_bodies: Core.SignAndInsertSelfEvent (node/core.go:122-130, 232-255) for a batch
 * = hgx_insert_event_bodies_ext whose R and S the device computes: per event, in dependency order, the
 * body digest, an ECDSA P-256 signature under the creator's signing key with the RFC 6979 nonce
 * (HMAC-SHA-256; deterministic, where Go's is random: any verifier accepts either), the text with that R
 * and S, and the id. ev->sig_r / ev->sig_s are ignored and may be NULL. out_r32 / out_s32 / out_id32
 * (32 bytes per event, each may be NULL) receive the accepted prefix. The fresh signatures go through
 * the same device Event.Verify as anyone's. Results, error strings, first-failure order, *n_inserted and
 * the context's state are those of hgx_insert_event_bodies_ext on the same events carrying the same R
 * and S. Additional refusals (HGX_ERR_INVALID "hgx_sign_insert_event_bodies: <reason>", checked on the
 * host before anything is staged): signing keys not set; an event whose creator has no signing key. */
int32_t hgx_set_signing_keys(hgx_ctx* ctx, const uint8_t* priv32, hgx_error* err);
int32_t hgx_sign_insert_event_bodies(hgx_ctx* ctx, const hgx_event_bodies* ev, const uint8_t* other_parent_id32,
                                     int64_t count, uint8_t* out_r32, uint8_t* out_s32, uint8_t* out_id32,
                                     int64_t* n_inserted, hgx_error* err);
/* The encoder alone: Event.Marshal bytes (json.Encoder output of {Body, R, S}, event.go:155-162) of
 * a batch whose parents' ids the caller supplies (sp_id32 / op_id32: 32 bytes per event, ignored
 * where the parent gid is -1; a parent is printed when its gid is not -1). keys65: n_keys keys of 65
 * bytes, creator[k] in [0, n_keys). Event k's text is out[offsets[k], offsets[k+1]); offsets gets
 * count + 1 entries. out == NULL sizes only; with out_cap smaller than offsets[count] the call
 * returns HGX_ERR_INVALID and still fills offsets. EventBody.Marshal is the text from byte 8 up to
 * and including the '}' before ,"R": followed by '\n'. Host pointers. */
int32_t hgx_event_json_batch(int32_t device, const hgx_event_bodies* ev, int64_t count, const uint8_t* keys65,
                             int32_t n_keys, const uint8_t* sp_id32, const uint8_t* op_id32, uint8_t* out,
                             int64_t out_cap, int64_t* offsets, hgx_error* err);
/* Host helper (no device): each event's depth inside a batch whose first event gets gid `base`:
 * level[k] = 0 when no parent has gid >= base, else 1 + the maximum over its in-batch parents;
 * *n_levels = the largest level + 1 (0 for an empty batch). Events of one level do not depend on
 * each other. HGX_ERR_INVALID for a parent gid >= the event's own gid (base + k). */
int32_t hgx_batch_levels(const int64_t* self_parent, const int64_t* other_parent, int64_t count, int64_t base,
                         int32_t* level, int32_t* n_levels, hgx_error* err);
/* WireEvents (event.go:252-267) as a SyncResponse carries them (net/commands.go:10-15), the
 * caller having decoded the JSON: the participants' ids instead of hashes. */
typedef struct {
    const int32_t* creator_id;            /* WireBody.CreatorID */
    const int64_t* index;                 /* WireBody.Index */
    const int64_t* self_parent_index;     /* WireBody.SelfParentIndex (-1: no self-parent) */
    const int32_t* other_parent_creator;  /* WireBody.OtherParentCreatorID */
    const int64_t* other_parent_index;    /* WireBody.OtherParentIndex (-1: "") */
    const int64_t* timestamp_ns;
    const uint8_t* hash;                  /* 32 bytes per event: the event id (Event.Hash) */
    const uint8_t* sig_s;                 /* 32 bytes per event: S, big-endian */
    const int32_t* ntx;
    const int32_t* tx_nil;
} hgx_wire_events;
/* Core.Sync's insert loop (node/core.go:199-211) in one call: per event ReadWireInfo
 * (hashgraph.go:569-614: parents through Store.ParticipantEvent, which sees the batch's earlier
 * events) then InsertEvent(ev, false); stops at the first error with Go's string (the
 * ReadWireInfo errors "<index>, Too Late" / "<index>, Not Found" included). */
int32_t hgx_insert_wire_events(hgx_ctx* ctx, const hgx_wire_events* ev, int64_t count, int64_t* n_inserted,
                               hgx_error* err);
/* WireEvents exactly as a peer sends them (event.go:252-267): no hash, parents as (creator id, Index).
 * These are hgx_diff_wire's columns plus R and the transactions. */
typedef struct {
    const int32_t* creator_id;            /* WireBody.CreatorID, 0..n-1 */
    const int64_t* index;                 /* WireBody.Index */
    const int64_t* self_parent_index;     /* < 0: no self-parent */
    const int32_t* other_parent_creator;  /* read only where other_parent_index >= 0 */
    const int64_t* other_parent_index;    /* < 0: "" */
    const int64_t* timestamp_ns;
    const uint8_t* sig_r;                 /* 32 B big-endian each */
    const uint8_t* sig_s;
    const int32_t* ntx;                   /* -1 for nil, as hgx_event_bodies */
    const int64_t* tx_off;                /* as hgx_event_bodies */
    const uint8_t* tx_bytes;
} hgx_wire_bodies;
/* Core.Sync's insert loop (node/core.go:199-211) from the wire fields alone: per
 * event ReadWireInfo (hashgraph.go:569-614), then InsertEvent(ev, false) with Event.Hash and
 * Event.Verify on the device as hgx_insert_event_bodies does them; stops at the first error with Go's
 * string. A parent (creator, Index) resolves as Store.ParticipantEvent does over the participant's
 * resident events plus the batch's earlier events, positionally (RollingIndex.GetItem): "<rune>, Too
 * Late" (HGX_ERR_TOO_LATE) below the chain's oldest Index, "<rune>, Not Found" (HGX_ERR_KEY_NOT_FOUND)
 * above the last event inserted so far -- a parent at a later batch position included --, and
 * HGX_ERR_PANIC "runtime error: slice bounds out of range [2:0]" / "runtime error: invalid memory
 * address or nil pointer dereference" for a creator id / an other-parent creator id outside 0..n-1.
 * A resolution error at position m cuts the batch: events [0, m) take the body path, whose failure, if
 * any, is the call's; otherwise the call returns the resolution error with *n_inserted = m. For the
 * prefix everything equals hgx_insert_event_bodies_ext on the same events with the parents as gids:
 * ids, error strings and their order, hgx_get_event_id, the context's state.
 * out_id32 (32 bytes per event), out_self_parent and out_other_parent (the resolved parent gids, -1 for
 * "") receive the accepted prefix; each may be NULL.
 * On a context with known root ids a self-parent index < 0 prints the creator's Root.X id (§3.12); an
 * index >= 0 resolves like any other. A wire event cannot name HGX_ROOT_Y / HGX_ROOT_OTHER.
 * Nothing proportional to the resident events crosses to the host, and the host mirror of the event
 * columns is neither built nor read: the plan uses the per-chain tables every insert keeps, the gids
 * of the resident parents are looked up on the device.
 * HGX_ERR_INVALID "hgx_insert_wire_bodies: <reason>", nothing changed: bad columns (as
 * hgx_insert_event_bodies, checked first), ctx NULL, a batch (G > 1), chain-sharded or row-sharded
 * context, roots whose ids are not known, keys not set, ids not known.
 * Scratch, on top of hgx_insert_event_bodies': the window of resident parents, 4 bytes per slot, one
 * slot per Index from the smallest one the batch names of a chain to that chain's head -- a few KB for a
 * sync between peers that gossip regularly, at worst 4 bytes per resident event (a batch naming every
 * chain's oldest event) --, plus 8 bytes per participant. The plan's parent descriptors travel in the
 * chunk's two parent columns (16 bytes per event), which the body path stages anyway. */
int32_t hgx_insert_wire_bodies(hgx_ctx* ctx, const hgx_wire_bodies* ev, int64_t count, uint8_t* out_id32,
                               int64_t* out_self_parent, int64_t* out_other_parent, int64_t* n_inserted,
                               hgx_error* err);
int32_t hgx_divide_rounds(hgx_ctx* ctx, hgx_error* err);
int32_t hgx_decide_fame(hgx_ctx* ctx, hgx_error* err);
int32_t hgx_find_order(hgx_ctx* ctx, hgx_error* err);
/* FindOrder in two halves (hgx_find_order = begin + end): begin = DecideRoundReceived and the
 * consensus timestamps of the context's shard of chains; end = the ConsensusSorter order and
 * the blocks. A row-sharded graph exchanges the shards' timestamps in between. */
int32_t hgx_find_order_begin(hgx_ctx* ctx, hgx_error* err);
int32_t hgx_find_order_end(hgx_ctx* ctx, hgx_error* err);
/* One graph row-sharded over `world` ranks: every rank holds
 * the whole DAG and runs the replicated phases (lastAncestors, firstDescendants, the round
 * steps, fame, roundReceived); the consensus-timestamp medians of the events newly received
 * are computed by the rank owning their creator (chains [C*rank/world, C*(rank+1)/world)) and
 * all-gathered between hgx_find_order_begin and _end: hgx_shard_values(ctx, r) = how many int64
 * values rank r contributes, hgx_shard_export writes this rank's, hgx_shard_import reads rank
 * r's (device pointers on the context's device, e.g. RCCL buffers, or host pointers, e.g.
 * gloo). hgx_find_order refuses a sharded context. */
int32_t hgx_set_shard(hgx_ctx* ctx, int32_t rank, int32_t world);
int64_t hgx_shard_values(hgx_ctx* ctx, int32_t rank);
int32_t hgx_shard_export(hgx_ctx* ctx, void* dst, int32_t dst_on_device);
int32_t hgx_shard_import(hgx_ctx* ctx, int32_t src_rank, const void* src, int32_t src_on_device);
/* Bootstrap from host columns / Core.Sync followed by Core.RunConsensus (hashgraph.go:1008-1037,
 * node/core.go:190-303): hgx_insert_events for the batch, then hgx_run_consensus, in one call.
 * For batches of 65 536 events and more (single-graph or batched contexts without roots, not
 * row-sharded) the timestamps, hashes, S and transaction columns are copied to HBM while
 * DivideRounds runs (they are read from FindOrder on); the result, the errors and the
 * counters equal the two calls'. On an insert error the accepted prefix stays inserted and
 * consensus does not run (the error is returned). The host buffers are read before it returns. */
int32_t hgx_insert_and_run(hgx_ctx* ctx, const hgx_events* ev, int64_t count, int64_t* n_inserted, hgx_error* err);
/* Core.RunConsensus (node/core.go:277-303): the three calls in sequence */
int32_t hgx_run_consensus(hgx_ctx* ctx, hgx_error* err);
/* Forget every consensus result but keep the inserted events resident in HBM:
 * the state of a fresh NewHashgraph after InsertEvent of the same events
 * (Bootstrap replay, hashgraph.go:1008-1022). Used to repeat timed passes. */
int32_t hgx_reset_consensus(hgx_ctx* ctx);
/* Forget every event as well: the state of a fresh NewHashgraph (hashgraph.go:39-66) with
 * the device allocations kept. */
int32_t hgx_clear(hgx_ctx* ctx);

/* ---- persistence: checkpoint file + Bootstrap (hashgraph.go:1008-1037) ----- */
/* The reference persists the DAG in its BadgerStore (events under topological-index keys with
 * their bodies and signatures, the participants, the roots and the blocks; badger_store.go:103-125,
 * 309-343, 540) and Hashgraph.Bootstrap replays the events in topological order through
 * InsertEvent, then runs DivideRounds / DecideFame / FindOrder once (dbTopologicalEvents,
 * badger_store.go:345-386). The equivalent here is a binary SoA file of the resident events in
 * gid (= topological) order, little-endian (version 2; version-1 files are still read):
 *   "HGXCKPT1" | u32 version 2 | i32 n | i32 graphs | i32 flags | i64 E
 *     flags: 1 rooted, 2 event ids, 4 participant keys, 8 payloads
 *   | rooted: i32 root_index[C], i32 root_round[C], u8 root_y_is_event[C], zero pad to 4
 *     | i64 n_others | u8 others[n_others][32] (the Root.Others keys, hgx_set_root_others)
 *     | per graph, what Reset kept (hashgraph.go:877-895): i32 has_lcr, i32 LastConsensusRound,
 *       i32 LastCommitedRoundEvents, i32 0, i64 ConsensusTransactions, i64 n_blocks, then per block
 *       i32 RoundReceived, i32 events, i64 transactions, i32 nil, i32 committed
 *   | i32 creator[E] | i64 index[E] | i64 self_parent[E] | i64 other_parent[E]
 *   | i64 timestamp_ns[E] | u8 sig_s[E][32] | u8 coin[E] (Event.Hash byte 16 != 0)
 *   | i32 ntx[E] | u8 tx_nil[E]
 *   | ids: u8 id[E][32] (Event.Hash), when every event was inserted with its id (hgx_events)
 *   | keys: u8 key[C][65] (hgx_set_participant_keys)
 *   | payloads: i64 off[E+1] | u8 bytes[off[E]] (the caller's per-event bytes, e.g. the body's
 *     transactions as the shim serialises them; opaque to libhgx)
 *   | u64 FNV-1a of every preceding byte
 * (C = graphs * n). hgx_save writes it atomically (a temporary file renamed over `path`);
 * hgx_save_ex also stores the caller's payloads (payload_off: E + 1 non-decreasing offsets from
 * 0 into payload, or NULL). hgx_bootstrap = Bootstrap on a fresh context (no events inserted):
 * checks the file (magic, version, n, graphs, sizes, checksum: HGX_ERR_INVALID "<reason>"),
 * installs the roots, the Root.Others keys and the kept state of a rooted file, the participant
 * keys, inserts every event in order (hgx_insert_events with the ids when the file has them:
 * their Go error if one is rejected), keeps the payloads (hgx_get_event_payload) and runs the
 * three consensus calls once (hgx_run_consensus). */
int32_t hgx_save(hgx_ctx* ctx, const char* path, hgx_error* err);
int32_t hgx_save_ex(hgx_ctx* ctx, const char* path, const int64_t* payload_off, const uint8_t* payload,
                    hgx_error* err);
/* hgx_save_bodies: the checkpoint of a context that keeps its event bodies (hgx_keep_bodies; DESIGN.md
 * section 3.17), a VERSION 3 file, written atomically like hgx_save. The header is version 2's with
 * version = 3; the flags hold 2, 4 and 16 (bodies), never 8, and 1 when rooted. The sections are
 * version 2's in the same order, with these additions:
 *   behind the rooted section's per-graph kept state (rooted files only):
 *     u8 has_x[C] | u8 has_y[C] | zero pad to 4 | u8 x_id[C][32] | u8 y_id[C][32]   (hgx_get_root_ids;
 *       rows with has = 0 are zero; has_y equals root_y_is_event)
 *     | i64 n_pairs | u8 pair_event[n_pairs][32] | u8 pair_parent[n_pairs][32]   (hgx_get_root_others,
 *       sorted by event id; pair_event equals the Root.Others keys section)
 *     | per graph, per kept block in order: u8 has_hash, 3 zero bytes, u8 hash[32]   (Block.Hash of the
 *       blocks that outlived a prune)
 *   behind the keys:
 *     u8 sig_r[E][32] | i64 T | i64 tx_off[T+1] | u8 tx_bytes[tx_off[T]]   (T = sum of ntx; tx_off starts
 *       at 0 and does not decrease; an event's transactions are consecutive entries, gid order)
 *   | u64 FNV-1a of every preceding byte.
 * The store is read in slices of bounded size (it is in gid order), so host memory beyond the per-event
 * columns stays bounded. Refused with HGX_ERR_INVALID "hgx_save_bodies: <reason>": "bodies not known"
 * (hgx_bodies_state != 1), "ids not known", "root ids not known" (rooted, before hgx_set_root_ids),
 * "participant keys not set", chain- or row-sharded. hgx_save / hgx_save_ex keep writing version 2.
 *
 * hgx_bootstrap of a version-3 file trusts nothing in it. Pass 1 checks the checksum and every section
 * with the context untouched (the refusals above, "unsupported flags", "root pairs and Root.Others keys
 * disagree", "T is not the sum of ntx", "tx_off decreases", "size mismatch", ...). Pass 2 installs the
 * roots, the kept state with its block hashes, the keys and the root ids (hgx_set_root_ids), then feeds the
 * events in pieces to hgx_insert_event_bodies_claimed with the file's ids as the claimed ids (an
 * HGX_ROOT_OTHER event's other-parent id is its pair's; without a pair the device's check fails it with
 * "CheckOtherParent: Other-parent not known"), then hgx_run_consensus. So every id is proven to be its
 * event's hash and every signature is verified, as the reference's Bootstrap does through InsertEvent. A
 * replay failure returns its Go error, or HGX_ERR_INVALID "hgx_bootstrap: event <gid>: the file's id is
 * not the event's hash", with the accepted prefix resident. On a context that called hgx_keep_bodies
 * while empty the store grows once to the file's totals and ends complete with the file's bodies; on
 * any other context the file is verified all the same and hgx_bodies_state stays 0. Afterwards the ids
 * and the root ids are known. */
int32_t hgx_save_bodies(hgx_ctx* ctx, const char* path, hgx_error* err);
/* the file's checksum: 64-bit FNV-1a of `bytes` bytes (host function, no device) */
uint64_t hgx_checksum(const void* data, int64_t bytes);
int32_t hgx_bootstrap(hgx_ctx* ctx, const char* path, hgx_error* err);
/* The id (Event.Hash, 32 bytes) of an inserted event: known when every event was inserted with
 * hgx_events (or bootstrapped from a file with ids); else HGX_ERR_INVALID. */
int32_t hgx_get_event_id(hgx_ctx* ctx, int64_t gid, uint8_t* out32, hgx_error* err);
/* The payload bytes of a bootstrapped event (hgx_save_ex): *len = its size, the first min(cap,
 * len) bytes to out; HGX_ERR_KEY_NOT_FOUND "<gid>, Not Found" without one. */
int32_t hgx_get_event_payload(hgx_ctx* ctx, int64_t gid, uint8_t* out, int64_t cap, int64_t* len, hgx_error* err);

/* ---- persistence: Reset / GetFrame (hashgraph.go:877-995, root.go) -------- */
/* Hashgraph.Reset(roots): forget the events and rounds (keeping LastConsensusRound,
 * LastCommitedRoundEvents, ConsensusTransactions and the blocks, like the reference) and
 * install one Root per participant: Index, Round and whether Root.Y names an event (1) or is
 * "" (0). Inserted events then name Root.X as self-parent -1 and Root.Y / Root.Others as
 * HGX_ROOT_Y / HGX_ROOT_OTHER. Single-graph contexts. */
int32_t hgx_reset(hgx_ctx* ctx, const int32_t* root_index, const int32_t* root_round, const int32_t* root_y_is_event,
                  hgx_error* err);
/* The keys of the roots' Others maps (root.go: Others[event hex] = other-parent hex,
 * hashgraph.go:437-440): the 32-byte ids of the events allowed to name HGX_ROOT_OTHER. After
 * hgx_reset the set is empty; an event inserted with HGX_ROOT_OTHER whose hash (hgx_events.hash)
 * is not a key fails with "CheckOtherParent: Other-parent not known", as in the reference. The
 * value (which other-parent the entry names) stays the shim's check, since the other-parent is
 * outside the store. hgx_bootstrap re-checks the HGX_ROOT_OTHER events of a rooted version-2
 * checkpoint against its keys and ids (a version-1 file, without ids, is trusted). */
int32_t hgx_set_root_others(hgx_ctx* ctx, const uint8_t* event_hash32, int64_t count, hgx_error* err);
/* Hashgraph.GetFrame: per participant root_x / root_y (gid; -1 = the current Root.X / ""; 
 * HGX_ROOT_Y / HGX_ROOT_OTHER as inserted), root_index, root_round; the frame's events (gids,
 * topological order) and Root.Others pairs (event, other-parent). Counts are returned in full;
 * arrays get the first `cap`. "<r>, Not Found" when LastConsensusRound's round is not stored. */
int32_t hgx_get_frame(hgx_ctx* ctx, int64_t* events, int64_t events_cap, int64_t* n_events, int64_t* root_x,
                      int64_t* root_y, int32_t* root_index, int32_t* root_round, int64_t* others_event,
                      int64_t* others_parent, int64_t others_cap, int64_t* n_others, hgx_error* err);
/* The resident hashgraph cut down to its last frame where it lives: the context
 * ends in the state that hgx_get_frame, hgx_reset(frame roots), hgx_set_root_others(ids of the
 * frame's Others events) and hgx_insert_events of the frame's events (in frame order, which is
 * ascending old gid) leave, without the caller holding any event and with nothing proportional to
 * the resident events crossing PCIe. The kept events keep their ids, timestamps, S, coin,
 * ntx / tx_nil and payloads (hgx_get_event_payload); new gid k is the position in the frame. Parents
 * as InsertEvent resolves them after a Reset (hashgraph.go:404-445): a kept parent -> its new gid;
 * the self-parent of a creator's first kept event -> -1 (the new Root.X); an other-parent outside
 * the frame -> HGX_ROOT_Y for that first event, else HGX_ROOT_OTHER (the event is a Root.Others key);
 * the codes of an already rooted context by the same rules. old_gid[0 .. min(cap, *n_kept)) gets the
 * old gid of each new gid, *n_kept the full count. Consensus is not run (hgx_run_consensus next, as
 * after a Reset). Kept and forgotten as by hgx_reset; the participant keys and the commit callback
 * stay. Refusals leave the context untouched: HGX_ERR_KEY_NOT_FOUND "<r>, Not Found" where
 * hgx_get_frame gives it; HGX_ERR_INVALID "<reason>" for a batch (G > 1), chain-sharded or
 * row-sharded context, a context whose event ids are not known (hgx_events32 / packed inserts, a
 * checkpoint without ids: the Others keys are event ids), and for a NULL ctx or n_kept. A frame
 * event the validation kernels reject is reported as HGX_ERR_PANIC (a bug; the events up to it are
 * resident). */
int32_t hgx_prune_to_frame(hgx_ctx* ctx, int64_t* old_gid, int64_t cap, int64_t* n_kept, hgx_error* err);
/* The 32-byte ids of the current roots' X and Y (has_x / has_y = 0 for "": a genesis root) and the
 * roots' Others pairs (event id, other-parent id), sorted by event id; *count in full, the arrays
 * get the first `cap`. hgx_prune_to_frame gathers them before the dropped events go, and carries
 * them over a further prune (a participant without events keeps its whole root). Known only while
 * every root traces back to genesis through prunes, or the caller installed them: after the caller's
 * own hgx_reset with roots, or a rooted hgx_bootstrap, both return HGX_ERR_INVALID "root ids not
 * known" until hgx_set_root_ids. */
int32_t hgx_get_root_ids(hgx_ctx* ctx, int32_t participant, uint8_t* x_id32, int32_t* has_x, uint8_t* y_id32,
                         int32_t* has_y, hgx_error* err);
int32_t hgx_get_root_others(hgx_ctx* ctx, uint8_t* event_id32, uint8_t* other_parent_id32, int64_t cap,
                            int64_t* count, hgx_error* err);
/* The ids of roots the caller installed with hgx_reset (a fast-forward join: Reset(frame.Roots),
 * hashgraph.go:877-895): per participant Root.X (x_id32, has_x: 0 for "") and Root.Y (y_id32, has_y),
 * 32 bytes per participant (rows with has = 0 are not read; a column may be NULL when every flag is 0),
 * and the Others pairs (event id, other-parent id), n_others of them in any order. The library sorts
 * the pairs by event id; their keys replace those of hgx_set_root_others. Afterwards the root ids are
 * known: hgx_get_root_ids / hgx_get_root_others answer, hgx_insert_event_bodies_ext works, and a later
 * hgx_prune_to_frame carries the ids on. A copy of the tables lives on the device (66 bytes per
 * participant and 64 per pair). HGX_ERR_INVALID "<reason>", with nothing changed: ctx NULL, a batch
 * (G > 1), chain-sharded or row-sharded context, has_y[p] different from the root's root_y_is_event,
 * an event id twice in the pairs, pairs on a context without roots, or events already resident (call
 * it between hgx_reset and the first insert). */
int32_t hgx_set_root_ids(hgx_ctx* ctx, const uint8_t* x_id32, const int32_t* has_x, const uint8_t* y_id32,
                         const int32_t* has_y, const uint8_t* others_event_id32, const uint8_t* others_parent_id32,
                         int64_t n_others, hgx_error* err);
/* Hashgraph.GetFrame complete, for a peer's fast-forward (hashgraph.go:900-1006): the
 * frame hgx_prune_to_frame would keep and the roots it would install at this moment, with ids and,
 * on a context that keeps them, bodies. Nothing the caller can observe changes. Every array is
 * host memory the caller owns; a NULL array is not written. */
typedef struct {
    /* the frame's Roots, n rows each (root.go:62-67) */
    int32_t* root_index;  int32_t* root_round;
    uint8_t* root_x_id32; int32_t* root_has_x;     /* 32 bytes per row; has = 0: "" (the row is zero) */
    uint8_t* root_y_id32; int32_t* root_has_y;
    /* Root.Others pairs sorted by event id, others_cap rows of 32 bytes each */
    uint8_t* others_event_id32; uint8_t* others_parent_id32; int64_t others_cap;
    /* the frame's Events in frame order (ascending gid), events_cap rows */
    int64_t* gid;                                   /* the resident gid: old_gid of a prune run next */
    int32_t* creator; int64_t* index; int64_t* timestamp_ns;
    int32_t* ntx;                                   /* -1 = nil, as hgx_event_bodies */
    int64_t* self_parent; int64_t* other_parent;    /* frame position, or -1 / HGX_ROOT_Y / HGX_ROOT_OTHER:
                                                       the columns hgx_prune_to_frame would re-insert */
    uint8_t* id32; uint8_t* sig_s;
    /* Body.Parents as ids, whether or not the parent is in the frame; parent_flags bit 0 / bit 1 =
     * the self- / other-parent is present, as hgx_insert_events_by_id reads them; the row of a clear
     * flag is zero. A parent stored as a code reads the current roots: self-parent -1 -> the creator's
     * Root.X id if it has one, HGX_ROOT_Y -> its Root.Y id, HGX_ROOT_OTHER -> the value of the
     * Root.Others pair whose key is the event's id. */
    uint8_t* self_parent_id32; uint8_t* other_parent_id32; uint8_t* parent_flags;
    int64_t events_cap;
    /* bodies (only on a context that keeps them): R, and the transactions as hgx_event_bodies has
     * them (tx_off holds *n_tx + 1 offsets from 0, tx_cap counts transactions) */
    uint8_t* sig_r; int64_t* tx_off; int64_t tx_cap; uint8_t* tx_bytes; int64_t bytes_cap;
} hgx_frame_out;
/* *n_events, *n_others, *n_tx, *n_bytes: the totals, always in full (the body totals are 0 unless one
 * of sig_r, tx_off, tx_bytes is requested). All or nothing: a group of columns (events, Others,
 * tx_off, tx_bytes) whose arrays are all NULL has capacity 0, and if events_cap < *n_events,
 * others_cap < *n_others, tx_cap < *n_tx or bytes_cap < *n_bytes the call returns HGX_ERR_CAPACITY with
 * the four totals set and no array written, the roots' included: an `out` of NULL arrays and zero
 * capacities is the sizing call. The roots are what hgx_get_root_ids / hgx_get_root_others answer after
 * the prune; a participant without events reports its whole current root. HGX_ERR_KEY_NOT_FOUND "<r>,
 * Not Found" where hgx_get_frame gives it. HGX_ERR_INVALID "hgx_get_frame_bodies: <reason>", nothing
 * written: NULL ctx, out or count pointer; a batch (G > 1), chain-sharded or row-sharded context; a
 * FindOrder in progress; "ids not known"; "root ids not known" (a rooted context before
 * hgx_set_root_ids); "bodies not known" when a body column is requested and hgx_bodies_state is not 1.
 * HGX_ERR_PANIC when a root id or an Others pair that a stored code names is missing (a bug). */
int32_t hgx_get_frame_bodies(hgx_ctx* ctx, hgx_frame_out* out, int64_t* n_events, int64_t* n_others,
                             int64_t* n_tx, int64_t* n_bytes, hgx_error* err);

/* ---- Hashgraph state (hashgraph.go:15-37) --------------------------------- */
int64_t hgx_num_events(hgx_ctx* ctx);
int32_t hgx_super_majority(hgx_ctx* ctx);
int64_t hgx_num_undetermined(hgx_ctx* ctx, int32_t graph);
int32_t hgx_undecided_rounds(hgx_ctx* ctx, int32_t graph, int32_t* out, int32_t cap); /* returns length */
int32_t hgx_last_consensus_round(hgx_ctx* ctx, int32_t graph, int32_t* has_value);
int32_t hgx_last_commited_round_events(hgx_ctx* ctx, int32_t graph);
int64_t hgx_consensus_transactions(hgx_ctx* ctx, int32_t graph);
int64_t hgx_pending_loaded_events(hgx_ctx* ctx, int32_t graph);

/* ---- Store views (hashgraph/store.go:3-25) -------------------------------- */
int32_t hgx_last_round(hgx_ctx* ctx, int32_t graph);                       /* Store.LastRound */
int32_t hgx_round_event_count(hgx_ctx* ctx, int32_t graph, int32_t r);     /* Store.RoundEvents */
int32_t hgx_round_witnesses(hgx_ctx* ctx, int32_t graph, int32_t r, int64_t* out, int32_t cap);
int32_t hgx_known(hgx_ctx* ctx, int32_t graph, int32_t* last_index);     /* Store.Known */
int64_t hgx_consensus_events_count(hgx_ctx* ctx, int32_t graph);         /* Store.ConsensusEventsCount */
/* full consensus order (AddConsensusEvent sequence) of one graph: gids */
int32_t hgx_consensus_events(hgx_ctx* ctx, int32_t graph, int64_t first, int64_t count, int64_t* gids);
/* Blocks in SetBlock order (hashgraph.go:826-854): rr, first position in the
 * graph's consensus order, number of events, number of transactions, nil flag,
 * committed (sent on commitCh: len(Transactions) > 0). */
int64_t hgx_num_blocks(hgx_ctx* ctx, int32_t graph);
int32_t hgx_block_info(hgx_ctx* ctx, int32_t graph, int64_t b, int32_t* round_received, int64_t* first,
                       int32_t* n_events, int64_t* n_tx, int32_t* tx_nil, int32_t* committed);
/* commitCh (hashgraph.go:848-854, node/node.go:150-154 -> AppProxy.CommitBlock): fn is called
 * from hgx_find_order for every new block with transactions, in SetBlock order, after the
 * block's state is recorded (graph, block index b, RoundReceived, first position and number of
 * its events in the graph's consensus order, transactions). NULL removes it. */
typedef void (*hgx_commit_fn)(void* user, int32_t graph, int64_t b, int32_t round_received, int64_t first,
                              int32_t n_events, int64_t n_tx);
int32_t hgx_set_commit_callback(hgx_ctx* ctx, hgx_commit_fn fn, void* user);
/* Store.GetBlock(rr) (inmem_store.go:163-169): index b of the block with RoundReceived rr,
 * else HGX_ERR_KEY_NOT_FOUND "<rr>, Not Found" */
int32_t hgx_get_block(hgx_ctx* ctx, int32_t graph, int32_t round_received, int64_t* b, hgx_error* err);
/* positions [first, first+count) of a graph's consensus order: gid, RoundReceived and
 * consensusTimestamp (ns) of each, in one call (any output may be NULL) */
int32_t hgx_consensus_received(hgx_ctx* ctx, int32_t graph, int64_t first, int64_t count, int64_t* gids,
                               int32_t* round_received, int64_t* consensus_ts);

/* ---- Store: events by participant (store.go:3-25, inmem_store.go:48-161) ---
 * Participant ids are the context's creator ids (global ids in a batched context). The
 * RollingIndex never evicts (cacheSize >= events). Errors carry Go's strings. */
/* LastFrom: gid of the participant's last event; none: gid -1 and is_root 1 (Root.X = "") */
int32_t hgx_last_from(hgx_ctx* ctx, int32_t participant, int64_t* gid, int32_t* is_root, hgx_error* err);
/* ParticipantEvents(p, skip) (caches.go:54-72): the events with Index > skip, in Index
 * order; *count = how many (gids gets the first min(count, cap)) */
int32_t hgx_participant_events(hgx_ctx* ctx, int32_t participant, int64_t skip, int64_t* gids, int64_t cap,
                               int64_t* count, hgx_error* err);
/* ParticipantEvent(p, index) (caches.go:74-80): "<index>, Too Late" / "<index>, Not Found" */
int32_t hgx_participant_event(hgx_ctx* ctx, int32_t participant, int64_t index, int64_t* gid, hgx_error* err);
/* GetRoot (inmem_store.go:163-169): X = -1 (Root.X), Y = -1 ("") or HGX_ROOT_Y, Index, Round
 * (the genesis Root: Index = Round = -1, or the one hgx_reset installed) */
int32_t hgx_get_root(hgx_ctx* ctx, int32_t participant, int64_t* x, int64_t* y, int32_t* index, int32_t* round,
                     hgx_error* err);
/* GetEvent (inmem_store.go:48-55): the DAG fields of an inserted event (bodies stay with the caller, or with
 * the context after hgx_keep_bodies: hgx_get_event_bodies) */
int32_t hgx_get_event(hgx_ctx* ctx, int64_t gid, int32_t* creator, int64_t* index, int64_t* self_parent,
                      int64_t* other_parent, int64_t* timestamp_ns, int32_t* ntx, int32_t* tx_nil, hgx_error* err);
/* SetWireInfo (hashgraph.go:532-567) of events [first, first+count): self-parent Index
 * (Root.Index -1 for a first event), other-parent creator id and Index (-1 for "") */
int32_t hgx_wire_info(hgx_ctx* ctx, int64_t first, int64_t count, int32_t* self_parent_index,
                      int32_t* other_parent_creator, int32_t* other_parent_index);
/* ReadWireInfo (hashgraph.go:569-614): parents of a wire event as gids (-1 for an index < 0),
 * through ParticipantEvent (its errors) */
int32_t hgx_read_wire_info(hgx_ctx* ctx, int32_t creator, int64_t self_parent_index, int32_t other_parent_creator,
                           int64_t other_parent_index, int64_t* self_parent, int64_t* other_parent, hgx_error* err);

/* ---- answering a SyncRequest (node/node.go:214-270) ------------------------
 * SyncResponse.Events as columns: the writable twin of hgx_wire_events plus the sender's gid.
 * Caller-allocated, `cap` entries each; a NULL column is skipped. */
typedef struct {
    int64_t* gid;                   /* the sender's gid (its body store's key) */
    int32_t* creator_id;            /* WireBody.CreatorID */
    int64_t* index;                 /* WireBody.Index */
    int64_t* self_parent_index;     /* WireBody.SelfParentIndex (Root.Index for a chain's first event) */
    int32_t* other_parent_creator;  /* WireBody.OtherParentCreatorID (-1: "") */
    int64_t* other_parent_index;    /* WireBody.OtherParentIndex (-1: "") */
    int64_t* timestamp_ns;
    uint8_t* hash;                  /* 32 B per event: Event.Hash; needs the context's ids */
    uint8_t* sig_s;                 /* 32 B per event */
    int32_t* ntx;
    int32_t* tx_nil;
    uint8_t* root_parent;           /* 0, or 1 / 2: the other-parent was inserted as HGX_ROOT_Y / HGX_ROOT_OTHER */
} hgx_wire_out;
/* node.processSyncRequest's three steps in one call, where the events live. known:
 * the peer's Hashgraph.Known(), one entry per participant of `graph` (the last Index it has, -1 none).
 *  1. Core.OverSyncLimit (node/core.go:147-159), on the host: sum over i of max(0, last_index[i] -
 *     known[i]). If sync_limit >= 0 and the sum exceeds it: *over_limit = 1, *count = the sum, nothing
 *     else written, HGX_OK. sync_limit < 0: no limit.
 *  2. Core.Diff (node/core.go:166-188): Store.ParticipantEvents(pk, known[id]) per participant, with
 *     the window rule and errors of hgx_participant_events: nothing when known > last, HGX_ERR_TOO_LATE
 *     "\x03, Too Late" when known + 1 < the oldest Index (common/rolling_index.go:21-39). The
 *     participants are checked in ascending id and the first failing one is reported; Go ranges over
 *     a map, so with two failing participants the reference's choice is random. An error leaves every
 *     output untouched.
 *  3. The selected events in ascending gid (ByTopologicalOrder), each as ToWire gives it
 *     (hashgraph.go:532-567): self_parent_index = the self-parent's Index, or the creator's Root.Index
 *     where the stored self-parent is -1; other_parent_creator / other_parent_index from the stored
 *     other-parent gid, -1 / -1 when there is none. An other-parent stored as a root code (after
 *     hgx_reset or hgx_prune_to_frame) has no wire index in libhgx: the row reports the code in
 *     root_parent and -1 / -1 in the two columns, as hgx_wire_info does, and the caller fills them from
 *     its own store.
 * *count = the full number of events; the arrays get the first min(cap, *count) rows and rows beyond
 * that are not written; *over_limit = 0 (over_limit may be NULL). creator_id and other_parent_creator
 * are ids within the graph, 0..n-1, as a WireBody carries them, so the columns are directly the
 * hgx_wire_events of hgx_insert_wire_events on the peer. R and the transaction bytes stay with the
 * caller's body store, keyed by gid; on a context that keeps them (hgx_keep_bodies) hgx_diff_wire_bodies
 * returns them with the rows. Works on batched (G > 1) and row-sharded contexts. The call
 * changes no context state apart from scratch buffers (121 bytes per returned row, and one word per
 * 2 048 resident events), and neither builds nor drops the host mirror behind the other store views.
 * HGX_ERR_INVALID "<reason>", nothing written: NULL ctx, known, out or count; graph outside the
 * context; cap < 0; a chain-sharded context; out->hash on a context whose event ids are not known
 * (hgx_events32 / packed inserts: the other columns still work there). */
int32_t hgx_diff_wire(hgx_ctx* ctx, int32_t graph, const int32_t* known, int64_t sync_limit,
                      hgx_wire_out* out, int64_t cap, int64_t* count, int32_t* over_limit, hgx_error* err);

/* ---- the event-id index --------------------------------- */
/* Opt in: from here on the context keeps an index of its events' ids in device memory, so that a caller
 * who addresses events by hash (Store.GetEvent, Body.Parents) needs no table of its own. Idempotent; on a
 * context that already holds events with known ids the index is built from them in one launch.
 * The table: open addressing over the id column, slots = the smallest power of two >= 2 x the context's
 * capacity (load <= 0.5), one 8-byte word per slot, 0 = empty, else (tag << 32) | (gid + 1); home slot =
 * id bytes 0..7 as a little-endian u64 masked with slots - 1, tag = id bytes 8..11 as a little-endian
 * u32, linear probing by +1 with wrap-around; a match needs the tag and all 32 bytes of the event's id.
 * Memory: 8 bytes per slot, so 16 bytes per event of capacity (up to 32 at the worst rounding): 256 MiB
 * at a capacity of 10 M events. Upkeep: every insert that brings ids (hgx_insert_events* with a hash
 * column, the body paths chunk by chunk, the wire paths, hgx_bootstrap with ids) adds its accepted events
 * in one more launch behind its commit (the split insert of a large hgx_insert_and_run batch: with the next insert
 * or lookup); hgx_clear and hgx_reset empty the table; hgx_prune_to_frame and
 * hgx_bootstrap empty it and rebuild it under the new gids. An insert without ids (hgx_events32 / packed,
 * an id-less bootstrap) leaves the index kept but invalid: the lookups refuse with "ids not known" until
 * hgx_clear, hgx_reset or a bootstrap with ids. The index is never written to a checkpoint (it can be
 * derived); the keep flag survives all of the above. HGX_ERR_INVALID "hgx_keep_id_index: <reason>": NULL
 * ctx, a batched (G > 1), chain-sharded or row-sharded context. HGX_ERR_DEVICE when the table cannot be
 * allocated: the index stays off. A context that never called hgx_keep_id_index allocates nothing for it
 * and launches no kernel of it. */
int32_t hgx_keep_id_index(hgx_ctx* ctx, hgx_error* err);
/* out = {kept (0 off, 1 valid, 2 kept but invalid), slots, entries, total_displacement, wrapped}:
 * total_displacement = the sum over entries of (slot - home) mod slots, wrapped = the entries stored at a
 * slot below their home slot. Both depend on the set of ids alone, not on the order the device inserted
 * them in. Computed by a reduction on request (entries and the two sums are 0 unless kept = 1). */
int32_t hgx_id_index_state(hgx_ctx* ctx, int64_t out[5], hgx_error* err);
/* Store.GetEvent's lookup for `count` ids (host memory, 32 bytes each): out_gid[k] = the gid of the
 * resident event with id k, or -1. Where several resident events have one id (the wide insert takes
 * hashes on trust) the lowest gid. count = 0 is HGX_OK. HGX_ERR_INVALID "hgx_find_events: <reason>": bad
 * arguments, "id index not kept", "ids not known ..."; out_gid is written on HGX_OK only.
 * HGX_ERR_DEVICE "hgx_find_events: id index corrupt" when a probe met no empty slot (a bug). */
int32_t hgx_find_events(hgx_ctx* ctx, const uint8_t* id32, int64_t count, int64_t* out_gid, hgx_error* err);
/* InsertEvent for Go Events as they are: hgx_insert_event_bodies_claimed whose parents come as ids.
 * ev->self_parent / ev->other_parent are ignored and may be NULL. parent_flags[k] bit 0 / bit 1: event k
 * has a self-parent / an other-parent; a clear bit is Go's "" and that id row is not read. The device
 * resolves every parent in two launches (a scratch table of the batch's claimed ids, 2 x count rounded up
 * to a power of two slots; then a probe of the resident index and of that table), the resolved columns
 * come back (16 bytes per event of the batch), and the call continues exactly as
 * hgx_insert_event_bodies_claimed on them with other_parent_id32 as its id column.
 *   self-parent   absent: -1; on a context with root ids whose creator's root has an X:
 *                 HGX_UNKNOWN_PARENT (the text would print Root.X; Go fails CheckSelfParent there).
 *                 present: the resident gid; else the LOWEST EARLIER batch position j < k whose claimed
 *                 id equals it, as gid hgx_num_events + j; else -1 if it is the creator's Root.X id; else
 *                 HGX_UNKNOWN_PARENT.
 *   other-parent  absent: -1. present: resident, or an earlier batch position, as above; else with root
 *                 ids HGX_ROOT_Y when it is the creator's Root.Y id and the event's self-parent string
 *                 equals the root's X (both "" counts; hashgraph.go:434), otherwise HGX_ROOT_OTHER (the
 *                 device's Root.Others check then decides); without root ids HGX_UNKNOWN_PARENT.
 * A resident match wins over a batch match; a parent at the same or a later batch position is unknown.
 * out_self_parent / out_other_parent (count entries, each may be NULL) receive the resolved codes of the
 * whole batch. Results, Go error strings, first-failure order, *n_inserted, the body store and the
 * context's state equal hgx_insert_event_bodies_claimed's on the same events with those codes; the error
 * prefix is "hgx_insert_events_by_id: ". Further refusals, nothing changed: "id index not kept", "ids not
 * known ...", NULL claimed_id32 or parent_flags, a NULL parent id column that some flag needs. Raw
 * 32-byte ids only. Device scratch: 117 bytes per event of the batch plus its table (16 to 32). */
int32_t hgx_insert_events_by_id(hgx_ctx* ctx, const hgx_event_bodies* ev, const uint8_t* claimed_id32,
                                const uint8_t* self_parent_id32, const uint8_t* other_parent_id32,
                                const uint8_t* parent_flags, int64_t count, int64_t* out_self_parent,
                                int64_t* out_other_parent, int64_t* n_inserted, hgx_error* err);

/* ---- the resident body store ---------------------------- */
/* Opt in: from here on the body paths (hgx_insert_event_bodies, _ext, hgx_insert_wire_bodies) keep every
 * accepted event's R and transaction bytes in device memory, keyed by gid, and the consumers below
 * serve them from there. Allowed on a context with no events (a fresh one, or after hgx_clear).
 * tx_hint / bytes_hint: a first reservation in transactions and bytes (0 is allowed); the store grows
 * by doubling when a chunk would not fit, a new allocation plus a device-to-device copy. If that
 * allocation fails the insert returns HGX_ERR_CAPACITY before that chunk is inserted (earlier chunks of
 * the call stay inserted). HGX_ERR_INVALID "hgx_keep_bodies: <reason>": NULL ctx, resident events,
 * negative hints, a chain-sharded or row-sharded context.
 * State rules: an insert that brings events without bodies (hgx_insert_events and its 32 / packed /
 * _device / _verified forms, hgx_insert_wire_events, hgx_insert_and_run*, hgx_bootstrap) leaves the
 * store lost: every consumer returns HGX_ERR_INVALID "<fn>: bodies not known" and nothing more is
 * kept until hgx_clear (or hgx_reset), which empties the store and makes it complete again.
 * hgx_prune_to_frame compacts the store with the events: kept events keep R and transactions under
 * their new gids, the dropped events' bytes are released. That compaction runs before anything is
 * dropped: if its allocation fails, or the kept bodies reach 4 GiB, hgx_prune_to_frame returns
 * HGX_ERR_CAPACITY and the context, its events and the store are as they were. A context that never called hgx_keep_bodies
 * takes exactly the paths, allocations and launches it took before. hgx_save does not store bodies. */
int32_t hgx_keep_bodies(hgx_ctx* ctx, int64_t tx_hint, int64_t bytes_hint, hgx_error* err);
/* 0 off, 1 complete, 2 lost; the events, transactions and bytes held (each pointer may be NULL) */
int32_t hgx_bodies_state(hgx_ctx* ctx, int64_t* n_events, int64_t* n_tx, int64_t* n_bytes);
/* R and the transactions of the events `gids` (any order, repeats allowed), as the sig_r / ntx / tx_off /
 * tx_bytes columns of hgx_event_bodies in list order: ntx -1 = nil; tx_off holds *n_tx + 1 offsets from
 * 0 (an array of tx_cap + 1 entries), tx_bytes *n_bytes bytes. A NULL array is not written.
 * HGX_ERR_KEY_NOT_FOUND "<gid>, Not Found" for a gid outside [0, hgx_num_events), nothing written.
 * HGX_ERR_CAPACITY when tx_cap < *n_tx or bytes_cap < *n_bytes (a NULL array has capacity 0): *n_tx
 * and *n_bytes are set and no array is touched, so NULL arrays with capacities 0 make a sizing call.
 * One call moves less than 4 GiB (HGX_ERR_CAPACITY beyond). HGX_ERR_INVALID "hgx_get_event_bodies:
 * bodies not known" unless hgx_bodies_state is 1. */
int32_t hgx_get_event_bodies(hgx_ctx* ctx, const int64_t* gids, int64_t count, uint8_t* sig_r, int32_t* ntx,
                             int64_t* tx_off, int64_t tx_cap, uint8_t* tx_bytes, int64_t bytes_cap, int64_t* n_tx,
                             int64_t* n_bytes, hgx_error* err);
/* Block.Transactions of block b of `graph` (hashgraph.go:826-854): the transactions of the block's
 * events in consensus order, from the body store; sizing and capacity rules of hgx_get_event_bodies.
 * *n_tx equals hgx_block_info's n_tx (HGX_ERR_PANIC otherwise). HGX_ERR_TOO_LATE
 * "hgx_block_transactions: block <b>: events no longer resident" after hgx_reset / hgx_prune_to_frame
 * dropped them; HGX_ERR_KEY_NOT_FOUND "<b>, Not Found" for b outside the blocks. Callable from
 * inside hgx_commit_fn. */
int32_t hgx_block_transactions(hgx_ctx* ctx, int32_t graph, int64_t b, int64_t* tx_off, int64_t tx_cap,
                               uint8_t* tx_bytes, int64_t bytes_cap, int64_t* n_tx, int64_t* n_bytes, hgx_error* err);
/* Block.Hash (block.go:44-53) of block b of `graph`: on a keeping context in state 1 every hgx_find_order
 * gathers its new blocks' transactions from the body store (the gid list is the device-resident order),
 * encodes {"RoundReceived":N,"Transactions":T}\n and hashes it on the device, and stores 32 bytes with
 * the block before the commit callbacks fire, so this is callable from inside hgx_commit_fn. The hashes
 * survive hgx_reset / hgx_prune_to_frame as the blocks do. The hashes are computed before the call's
 * blocks are recorded: if that fails (HGX_ERR_CAPACITY when one call's new blocks reach 4 GiB of
 * transactions or text) hgx_find_order returns the error and has made no block. HGX_ERR_KEY_NOT_FOUND "<b>, Not Found" for b
 * outside the blocks or a block made while the state was not 1; HGX_ERR_INVALID "hgx_get_block_hash:
 * bodies not known" in states 0 and 2. */
int32_t hgx_get_block_hash(hgx_ctx* ctx, int32_t graph, int64_t b, uint8_t* out32, hgx_error* err);
/* The encoder alone (host pointers, no context): Block.Hash of `count` blocks on `device`. Block k has
 * ntx[k] transactions, consecutive in tx_off (the sum of ntx, plus one, offsets into tx_bytes); its text
 * prints null for tx_nil[k] && ntx[k] == 0, else the list ("" for an empty transaction). The texts are
 * built in groups of at most 32 MiB (a single larger block raises the bound to its size); the whole
 * batch's text stays below 4 GiB (HGX_ERR_CAPACITY beyond, decided on the host before any launch). out32: 32 bytes per block. The host twin is hgx_block_hash. */
int32_t hgx_block_hash_batch(int32_t device, const int64_t* round_received, const int32_t* ntx,
                             const int32_t* tx_nil, const int64_t* tx_off, const uint8_t* tx_bytes, int64_t count,
                             uint8_t* out32, hgx_error* err);
/* R and the transactions of hgx_diff_wire_bodies' rows: caller-allocated, sig_r `cap` rows of 32 bytes,
 * tx_off tx_cap + 1 entries, tx_bytes bytes_cap bytes; a NULL array is skipped (capacity 0). */
typedef struct {
    uint8_t* sig_r;
    int64_t* tx_off;
    int64_t tx_cap;
    uint8_t* tx_bytes;
    int64_t bytes_cap;
} hgx_wire_body_out;
/* A complete SyncResponse: hgx_diff_wire (plan, launches, errors, the cap rule and the untouched outputs
 * on error, all unchanged) plus R and the transactions of the first min(cap, *count) rows from the body
 * store. *n_tx / *n_bytes are those rows' totals. If they do not fit body's capacities: HGX_ERR_CAPACITY
 * with *count, *n_tx and *n_bytes set and no array written, so a NULL body (or capacities 0) with cap =
 * the row count makes a sizing call. With ntx = tx_nil ? -1 : ntx the returned columns are directly the
 * hgx_wire_bodies of hgx_insert_wire_bodies on the peer. HGX_ERR_INVALID "hgx_diff_wire_bodies: bodies
 * not known" unless hgx_bodies_state is 1. */
int32_t hgx_diff_wire_bodies(hgx_ctx* ctx, int32_t graph, const int32_t* known, int64_t sync_limit,
                             hgx_wire_out* out, hgx_wire_body_out* body, int64_t cap, int64_t* count, int64_t* n_tx,
                             int64_t* n_bytes, int32_t* over_limit, hgx_error* err);

/* ---- per-event results (bulk) --------------------------------------------- */
/* round (Round), witness (Witness), famous (RoundEvent.Famous: 0 Undefined,1 True,2 False) */
int32_t hgx_get_rounds(hgx_ctx* ctx, int64_t first, int64_t count, int32_t* round, int8_t* witness,
                       int8_t* famous);
/* RoundReceived (-1 = nil) and consensusTimestamp (Unix ns) */
int32_t hgx_get_received(hgx_ctx* ctx, int64_t first, int64_t count, int32_t* round_received,
                         int64_t* consensus_ts);
/* lastAncestors / firstDescendants indexes of one event (n values each) */
int32_t hgx_get_coords(hgx_ctx* ctx, int64_t gid, int32_t* last_ancestors, int32_t* first_descendants);

/* ---- primitives (hashgraph.go:73-339), valid after hgx_divide_rounds ------ */
int32_t hgx_ancestor(hgx_ctx* ctx, int64_t x, int64_t y);
int32_t hgx_self_ancestor(hgx_ctx* ctx, int64_t x, int64_t y);
int32_t hgx_see(hgx_ctx* ctx, int64_t x, int64_t y);
int32_t hgx_strongly_see(hgx_ctx* ctx, int64_t x, int64_t y);
int64_t hgx_oldest_self_ancestor_to_see(hgx_ctx* ctx, int64_t x, int64_t y);
int32_t hgx_round(hgx_ctx* ctx, int64_t x);
int32_t hgx_witness(hgx_ctx* ctx, int64_t x);

/* ---- Go encodings (parity unpinned) -------------------- */
/* SHA256(json.Encoder(Block)) with Block{RoundReceived, Transactions} (block.go:26-53) */
int32_t hgx_block_hash(int64_t round_received, int32_t ntx, const uint8_t* const* tx, const int64_t* tx_len,
                       int32_t tx_nil, uint8_t* out32);

/* ---- ingest front end: batched SHA-256 ----------------- */
/* crypto.SHA256 (crypto/utils.go:11-16) of `count` messages in one launch, message i =
 * data[offsets[i], offsets[i+1]) (offsets has count+1 non-decreasing entries). Replaces the
 * per-event calls Event.Hash (hashgraph/event.go:171-180; the event id of Hex() :183-188),
 * EventBody.Hash (:48-54, the bytes Verify checks :142-152) and Block.Hash (block.go:44-53)
 * over a whole sync batch (node/core.go:199-211). Host buffers, copied to HBM; out32 gets
 * 32 bytes per message. HGX_ERR_DEVICE without a gfx950 device (no CPU fallback). */
int32_t hgx_sha256_batch(int32_t device, const uint8_t* data, const int64_t* offsets, int64_t count,
                         uint8_t* out32, hgx_error* err);
/* The same on device-resident buffers, enqueued on `stream` (a hipStream_t; NULL = null
 * stream) without synchronising. d_out32 must be 4-byte aligned. Message bytes are read
 * with 16-byte loads from the 16-byte-aligned span of each message: up to 15 bytes before
 * d_data + offsets[i] and past d_data + offsets[i+1] may be read (harmless inside one
 * allocation; the caller keeps that span mapped). */
int32_t hgx_sha256_batch_device(const uint8_t* d_data, const int64_t* d_offsets, int64_t count,
                                uint8_t* d_out32, void* stream);
/* Measurement: `count` synthetic messages resident in HBM (message i has length
 * min_len + splitmix64(~seed + i) % (max_len - min_len + 1); packed 8-byte word j of the
 * data is splitmix64(seed + j)), hashed warmup + iters times; *ms_per_launch from HIP
 * events on the launch stream; digests of the first n_sample messages to sample32. */
int32_t hgx_sha256_bench(int32_t device, int64_t count, int32_t min_len, int32_t max_len, uint64_t seed,
                         int32_t warmup, int32_t iters, double* ms_per_launch, int64_t* total_bytes,
                         int64_t* n_blocks, int64_t n_sample, uint8_t* sample32);

/* Measurement (bench.py roofline.latency): the exchange floor of one round of the persistent
 * recurrence -- `chains` resident workgroups of k_round_p's geometry at n coordinates (16 < n <= 256,
 * chains <= the device's CUs) that per round only publish their n-byte candidate row and granule
 * (write-through) and poll every other one's (sc1), no search. *us_per_round from HIP events over one
 * launch of `rounds` rounds after a warm-up launch; chains = 2 is one 1-to-1 hand-off each way. */
int32_t hgx_exchange_floor_bench(int32_t device, int32_t chains, int32_t n, int32_t rounds, double* us_per_round);

/* Test entry: FindOrder's bucket sort (k_seg_sort, the kernels launch_sort_seg runs) on caller-given
 * buckets. Bucket b holds elements [segoff[b], segoff[b + 1]) of the m (key, value) pairs (segoff[0] = 0,
 * the last bucket ends at m; no bucket over 8 192 elements); a value is a row of the m 32-byte rows S32,
 * values < m. out_vals[m]: every bucket's values ordered by (key, S row as a big-endian number). The
 * kernel instantiation follows the largest bucket as in FindOrder; the one-word path (key and index in
 * 64 bits) is taken when the highest set bit of any key leaves room for the index, unless force_kv is
 * nonzero; *packed_out (optional) = 1 when it was taken. */
int32_t hgx_seg_sort_check(int32_t device, int32_t nseg, const uint32_t* segoff, int32_t m, const uint64_t* keys,
                           const uint32_t* vals, const uint8_t* S32, int32_t force_kv, uint32_t* out_vals,
                           int32_t* packed_out);

/* ---- ingest front end: batched ECDSA P-256 verify ------ */
/* Event.Verify (hashgraph/event.go:142-152) for a whole sync batch: crypto.ToECDSAPub of
 * Body.Creator (crypto/utils.go:22-28) and crypto.Verify (crypto/utils.go:41-43) = Go's
 * ecdsa.Verify on P-256. keys65: n_keys public keys, 65 bytes each (0x04 || X || Y, the
 * bytes of Body.Creator); key_idx[i]: the key of signature i; digest32: EventBody.Hash
 * (SHA-256 of the body, hgx_sha256_batch); r32, s32: R and S big-endian, zero-padded.
 * out[i] = 1 valid, 0 invalid, 2 the key is not a P-256 point (Go's elliptic.Unmarshal
 * returns nil there). Pinned by libcrypto answers (oracle/p256_ref.c). */
int32_t hgx_p256_verify_batch(int32_t device, const uint8_t* keys65, int32_t n_keys, const int32_t* key_idx,
                              const uint8_t* digest32, const uint8_t* r32, const uint8_t* s32, int64_t count,
                              uint8_t* out, hgx_error* err);
/* bench.py: the same batch resident in HBM; the key tables built once (as a context does when its
 * keys are set), then the verify launch warmup + iters times, device time per verify launch from
 * HIP events; out = the results of the last launch */
int32_t hgx_p256_verify_bench(int32_t device, const uint8_t* keys65, int32_t n_keys, const int32_t* key_idx,
                              const uint8_t* digest32, const uint8_t* r32, const uint8_t* s32, int64_t count,
                              int32_t warmup, int32_t iters, uint8_t* out, double* ms_per_launch);
/* crypto.Sign (crypto/utils.go:37-39) for a batch, stand-alone like hgx_p256_verify_batch (host
 * pointers; the base point's table is built per call): priv32 = n_keys private keys of 32 bytes
 * (big-endian d, 1 <= d < N), key_idx[i] the key of digest i, out_r32 / out_s32 = R and S, 32 bytes
 * big-endian each. Nonces by RFC 6979 (HMAC-SHA-256), so the output is a function of (d, digest); s
 * is not normalised to the low half (Go's is not). hgx_p256_public_keys: 0x04 | X | Y of d G per key.
 * HGX_ERR_INVALID for NULL pointers, n_keys <= 0, a negative count, a key index outside [0, n_keys)
 * and a d that is 0 or not below N. Not constant time. */
int32_t hgx_p256_sign_batch(int32_t device, const uint8_t* priv32, int32_t n_keys, const int32_t* key_idx,
                            const uint8_t* digest32, int64_t count, uint8_t* out_r32, uint8_t* out_s32, hgx_error* err);
int32_t hgx_p256_public_keys(int32_t device, const uint8_t* priv32, int32_t n_keys, uint8_t* out_keys65, hgx_error* err);

/* ---- timing / instrumentation --------------------------------------------- */
/* per-phase device times (ms) of the last calls: coords, rounds, fame, order; then
 * LA sweeps, rounds, 1 if the coordinates were stored compact (uint16); then of the last
 * DivideRounds: lastAncestors rows recomputed, 1 if it rebuilt the layout (0: incremental),
 * the first round step it ran, 1 if the lastAncestors pass was the dataflow kernel; then
 * the number of dataflow passes that gave up and were redone by the sweeps, and the time
 * segments of the last dataflow pass; then the persistent round launches so far and the
 * DivideRounds calls whose persistent launch gave up and were redone per round, and the
 * candidate rows it counted with exact compares (over 8 bits), the round and chain of the last
 * persistent launch that gave up, then the whole-graph round launches so far (up to 19 values) */
/* ... 1 if the last DivideRounds ran the whole graph in one workgroup, 1 if its verify sweep ran, the
 * FindOrders sorted by buckets, and the pieces of the last hgx_insert_and_run32's pipelined ingest
 * (0: the serial path) (up to 23 values) */
/* ... then host wall clock (ms) of the last calls' host-only sections: the bookkeeping after
 * DivideRounds' device work, after DecideFame's, before and after FindOrder's, and the time the
 * payload commit of the last hgx_insert_and_run* took (up to 27 values) */
/* ... then the FindOrders so far whose consensus timestamps ran on the lane = event kernel (k_cts_row)
 * (up to 28 values) */
int32_t hgx_phase_times(hgx_ctx* ctx, double* out, int32_t cap);
/* dominant-kernel accounting for the roofline line of bench.py:
 * name of the kernel, summed device ms (the round steps time one hipGraph replay in four and
 * scale the sample to every launch), launches, algorithmic bytes moved */
int32_t hgx_kernel_stats(hgx_ctx* ctx, int32_t k, char* name, int32_t name_cap, double* ms, int64_t* launches,
                         double* bytes);
int32_t hgx_reset_stats(hgx_ctx* ctx);
/* time the kernels in bitmask `mask` (bit k = kernel id of hgx_kernel_stats; -1 = all) with HIP events on the context stream (bench.py roofline) */
int32_t hgx_set_kernel_timing(hgx_ctx* ctx, int32_t mask);

/* coordinate storage of later DivideRounds calls: 0 = auto (uint16 when every Index
 * <= 65533 and n is even, else int32), 1 = always int32. Same results either way. */
int32_t hgx_set_coord_storage(hgx_ctx* ctx, int32_t mode);
/* DecideFame vote tally: 0 = popcount with one lane per voter (default), 1 = per-round popcount
 * kernel, 2 = witness-tiled int8 MFMA, 3 = witness-tiled popcount (the default before the
 * lane-per-voter kernel). Same results; for measurement. */
int32_t hgx_set_fame_tally(hgx_ctx* ctx, int32_t mode);
/* hgx_insert_and_run32 on an empty, unrooted, unsharded one-graph context of n <= 896 with at least
 * min_events events (default 4 000 000) and a time-segmented lastAncestors pass: the structure columns
 * cross PCIe in `pieces` pieces (default 4, at most 8) and each piece is inserted, laid out and its
 * segments' lastAncestors started while the later ones are still being copied (on twice the time
 * segments of a serial rebuild unless hgx_set_la_kernel fixes their number). pieces = 0: always the
 * serial order. Same results and errors (a failed check redoes the batch serially); for measurement
 * (DESIGN.md §3.0). */
int32_t hgx_set_ingest_pipeline(hgx_ctx* ctx, int32_t pieces, int64_t min_events);
/* DivideRounds lastAncestors: 0 = one dataflow pass per (graph, column block) where it
 * applies (default: n <= 896, chains < 2^21 rows; hgx_la_wave.hip), and for a small graph
 * (n <= 32 compact / 16 int32, its rows within 150 KB) the pass with the whole graph in one
 * workgroup's LDS; 1 = Gauss-Seidel sweeps to the fixed point (hgx_kernels.hip), 2 <= m <= 1024 =
 * the dataflow pass with m time segments on a rebuild (measurement), 1025 = the dataflow pass
 * without the small-graph form, 1026 = the default with the verify sweep after every time-segmented
 * pass (by default it runs only when the segments' exactness check fails). Same results
 * (DESIGN.md §3.1). */
int32_t hgx_set_la_kernel(hgx_ctx* ctx, int32_t mode);
/* DivideRounds rounds: 0 = default: the persistent recurrence (hgx_round_p.hip, one resident
 * workgroup per chain runs every round in one launch) where it applies (n <= 256, at most one
 * chain per compute unit, no roots; for 256 < n <= 1024 and one graph hgx_round_pb.hip, one
 * resident workgroup per chain with events) on a call that lays the DAG out anew (a call resuming after
 * a few inserts runs a few rounds: one launch per round of mode 2 there, and wherever the
 * persistent launch does not apply); 3 = the persistent recurrence on every call where it
 * applies;
 * 1 = block binary search per round (hgx_rounds.hip; per-candidate search over streamed rows
 * above n = 256); 2 = one launch per round, one lane per candidate, 8-bit rebased compares
 * (hgx_round_k.hip; candidates in chunks of 128 above n = 256); 4 = the whole-graph recurrence
 * (hgx_round_g.hip: one workgroup per graph runs every round in one launch, n <= 16), which mode 0
 * also uses on every call where it applies; 5 = mode 0 without hgx_round_pb.hip (n > 256: the
 * steps of mode 2). Same results. */
int32_t hgx_set_round_kernel(hgx_ctx* ctx, int32_t mode);
/* FindOrder's sort of the received events by (graph, roundReceived, consensus timestamp, S): 0 =
 * default: bucketed by (graph, roundReceived) and every bucket sorted in one workgroup's LDS where
 * every bucket holds at most 8 192 events (else as 1); 1 = LSD radix passes over the whole list.
 * Same results. */
int32_t hgx_set_sort_kernel(hgx_ctx* ctx, int32_t mode);
/* hgx_create_sharded's shards on this context's own device: shards = W in [1, 8] (1 = back to one
 * context), on an empty context only (before the first insert). W shards on one device need
 * GPU_MAX_HW_QUEUES >= W + 2 (HGX_ERR_INVALID otherwise). Same results. */
int32_t hgx_set_round_shards(hgx_ctx* ctx, int32_t shards);
/* Test switch of a chain-sharded context (hgx_create_sharded / hgx_set_round_shards): on = 1 writes
 * every other shard's window as a window on another device (system-scope write-through stores, the
 * peer path), also where the shards share a device, so a one-GPU box runs the instructions the
 * shards of an 8-GPU node run. HGX_ERR_INVALID on a context without shards. Same results. */
int32_t hgx_set_shard_remote(hgx_ctx* ctx, int32_t on);
/* FindOrder consensus timestamps: 0 = default: for 32 < n <= 256, blocks of 64 positions of one chain
 * with lane = event and whole firstDescendants lines per load (k_cts_row, hgx_cts.hip) on a call
 * that receives at least 512 events per launched chain, otherwise as 1; 1 = one tile of 8
 * positions per block (k_cts_small / k_cts_tile, hgx_kernels.hip); 2 = resident blocks with three
 * tiles' loads in flight behind the selects of a fourth (hgx_cts.hip) where it applies (32 < n <= 512,
 * at most 4096 chains), otherwise mode 1 (measured slower at c3: 12.6 against 8.9 ms); 3 = k_cts_row
 * on every call where it applies (32 < n <= 256), otherwise mode 1; 4 = mode 3 with one staged
 * WLAT row per block, so most blocks read their membership rows from global memory (tests and
 * measurement). Same results. */
int32_t hgx_set_cts_kernel(hgx_ctx* ctx, int32_t mode);
/* DivideRounds schedule: 1 = incremental (default: a call after more InsertEvents extends
 * lastAncestors/firstDescendants for the new events only and resumes the round steps at the
 * lowest round that can change; FindOrder works on the events not yet received), 0 = every
 * call recomputes from the whole DAG. Same results. */
int32_t hgx_set_incremental(hgx_ctx* ctx, int32_t on);
/* Size the per-round device tables for `rounds` rounds (they grow on demand during
 * DivideRounds); before the first DivideRounds only. A small value exercises the growth path. */
int32_t hgx_reserve_rounds(hgx_ctx* ctx, int32_t rounds);

/* ---- device buffers (for callers without a device allocator: bench, tests) ---- */
int32_t hgx_device_alloc(int32_t device, int64_t bytes, void** ptr);
int32_t hgx_device_free(int32_t device, void* ptr);
/* synchronous copy; to_device 1: host src -> device dst, 0: device src -> host dst */
int32_t hgx_device_copy(int32_t device, void* dst, const void* src, int64_t bytes, int32_t to_device);

/* ---- synthetic gossip traces (BASELINE.md / SURVEY 8d generator) ---------- */
/* Seeded random gossip modelled on node/core_test.go:514-537: every active peer
 * emits a genesis event, then each step a uniformly chosen `to` emits
 * (sp = head[to], op = head[from]); ts = t0 + step*1000 ns; w.p. 1/2 one
 * 16-byte-class payload "p%03d tx %08d", else an empty non-nil payload; S and
 * the event id are PRNG bytes (synthetic ids). Silent peers are the last
 * `n_silent` ids (never to/from, no genesis). With probability stale_prob the
 * `from` head is replaced by one of from's last stale_depth events. Fills
 * caller arrays of length n_events (index/parents as in hgx_events; tx_seq =
 * per-creator payload counter or -1). Returns HGX_OK. */
int32_t hgx_trace_gossip(int32_t n_participants, int32_t n_silent, int64_t n_events, uint64_t seed,
                         double stale_prob, int32_t stale_depth,
                         int32_t* creator, int64_t* index, int64_t* self_parent, int64_t* other_parent,
                         int64_t* timestamp_ns, uint8_t* hash, uint8_t* sig_s, int32_t* ntx, int32_t* tx_nil,
                         int64_t* tx_seq);
/* payload bytes of generated transaction (creator, seq); returns length */
int32_t hgx_trace_tx_payload(int32_t creator, int64_t seq, uint8_t* out, int32_t cap);

#ifdef __cplusplus
}
#endif
#endif /* HGX_H */
