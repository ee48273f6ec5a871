// Event bodies on the device: the Go-JSON of every event of a batch
// (Event.Marshal, hashgraph/event.go:155-162: json.Encoder output of {Body, R, S}), the event ids
// (Event.Hash :171-180 = SHA-256 of that text) in dependency order, the body digests
// (EventBody.Hash :48-54 = SHA-256 of EventBody.Marshal, the bytes Event.Verify checks :142-152),
// and the hand-over to the verified insert. The text of one event is
//   {"Body":{"Transactions":T,"Parents":["SP","OP"],"Creator":"B64","Timestamp":"TS","Index":N},"R":DEC,"S":DEC}\n
// (SURVEY Appendix B): T = null | [] | ["b64",...] (std base64 with padding), a parent = 0x + 64
// upper-case hex digits or empty, Creator = base64 of the 65 key bytes, TS = RFC3339Nano in UTC,
// N a signed decimal, R and S bare decimals. EventBody.Marshal is the {...} after "Body": plus '\n',
// so the body digest is hashed out of the event's text with a one-byte suffix.
//
// One lane per event: a sizing pass (the same encoder into a counting sink), an exclusive scan, a
// write pass that leaves the two parent slots open; then the id pass, one workgroup per graph looping
// over the batch's dependency levels (a level's events patch their parents' hex into their text and
// hash it; __syncthreads() and an agent-scope fence order the levels; no workgroup waits for
// another); then the body digests, one lane per event.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "hgx.h"
#include "hgx_bodies.h"
#include "hgx_bodystore.h"
#include "hgx_engine.h"
#include "hgx_kernels.h"
#include "hgx_p256_sign_dev.h"
#include "hgx_sha256_dev.h"

#define HGX_TRY(x)                              \
    do {                                        \
        hipError_t _e = (x);                    \
        if (_e != hipSuccess) return _e;        \
    } while (0)

namespace hgx {

// ---- sinks: the encoder writes through one of these (host-callable as well: the text is plain
// integer code, so a host harness can compare it with the oracle's encoder byte for byte) --------
struct CountSink {
    int64_t n = 0;
    __host__ __device__ __forceinline__ void put(uint32_t) { n++; }
    __host__ __device__ __forceinline__ void skip(int k) { n += k; }
    __host__ __device__ __forceinline__ void finish() {}
};

// bytes gathered into aligned 4-byte stores; the first and last word of a run are stored bytewise
struct ByteSink {
    uint8_t* w;     // the aligned word being filled
    uint32_t acc = 0;
    int lo, nb;     // its bytes [lo, nb) are gathered in acc
    int64_t n = 0;
    __host__ __device__ __forceinline__ explicit ByteSink(uint8_t* p) {
        lo = nb = (int)((uintptr_t)p & 3);
        w = p - lo;
    }
    __host__ __device__ __forceinline__ void flush() {
        if (lo == 0 && nb == 4) *(uint32_t*)w = acc;
        else for (int j = lo; j < nb; j++) w[j] = (uint8_t)(acc >> (8 * j));
        w += 4;
        acc = 0;
        lo = nb = 0;
    }
    __host__ __device__ __forceinline__ void put(uint32_t c) {
        acc |= c << (8 * nb);
        n++;
        if (++nb == 4) flush();
    }
    __host__ __device__ __forceinline__ void skip(int k) {   // leave k bytes unwritten
        uint8_t* p = w + nb + k;
        if (nb > lo) flush();
        lo = nb = (int)((uintptr_t)p & 3);
        w = p - lo;
        acc = 0;
        n += k;
    }
    __host__ __device__ __forceinline__ void finish() {
        if (nb > lo) flush();
    }
};

template <typename S>
__host__ __device__ __forceinline__ void put_str(S& s, const char* lit) {
    for (; *lit; lit++) s.put((uint32_t)(uint8_t)*lit);
}

__host__ __device__ __forceinline__ uint32_t b64_char(uint32_t v) {
    return v < 26 ? 'A' + v : v < 52 ? 'a' + (v - 26) : v < 62 ? '0' + (v - 52) : v == 62 ? '+' : '/';
}

template <typename S>
__host__ __device__ __forceinline__ void put_base64(S& s, const uint8_t* in, int64_t len) {
    int64_t i = 0;
    for (; i + 3 <= len; i += 3) {
        const uint32_t v = ((uint32_t)in[i] << 16) | ((uint32_t)in[i + 1] << 8) | in[i + 2];
        s.put(b64_char(v >> 18)); s.put(b64_char((v >> 12) & 63)); s.put(b64_char((v >> 6) & 63)); s.put(b64_char(v & 63));
    }
    if (len - i == 1) {
        const uint32_t v = (uint32_t)in[i] << 16;
        s.put(b64_char(v >> 18)); s.put(b64_char((v >> 12) & 63)); s.put('='); s.put('=');
    } else if (len - i == 2) {
        const uint32_t v = ((uint32_t)in[i] << 16) | ((uint32_t)in[i + 1] << 8);
        s.put(b64_char(v >> 18)); s.put(b64_char((v >> 12) & 63)); s.put(b64_char((v >> 6) & 63)); s.put('=');
    }
}

__host__ __device__ __forceinline__ uint32_t hex_char(uint32_t v) { return v < 10 ? '0' + v : 'A' + (v - 10); }

// "0x%X" of a 32-byte id (Event.Hex, event.go:183-188), read as 8 words (ids are 4-byte aligned);
// FRESH: the id may have been written by another wave of this launch, so the words are read past L1
template <bool FRESH, typename S>
__host__ __device__ __forceinline__ void put_hex_id(S& s, const uint8_t* id) {
    s.put('0');
    s.put('x');
    uint32_t* p = (uint32_t*)id;
    for (int j = 0; j < 8; j++) {
        const uint32_t x = FRESH ? __hip_atomic_load(p + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : p[j];
        for (int b = 0; b < 4; b++) {
            const uint32_t v = (x >> (8 * b)) & 0xFF;
            s.put(hex_char(v >> 4));
            s.put(hex_char(v & 15));
        }
    }
}

// v < 10^9 as decimal digits: all nine when `started`, else from its first non-zero digit (nothing
// for 0); `keep` digits at most (the timestamp's fraction drops its trailing zeros)
template <typename S>
__host__ __device__ __forceinline__ void put_chunk9(S& s, uint32_t v, bool& started, int keep = 9) {
    uint32_t d = 100000000u;
#pragma unroll
    for (int j = 0; j < 9; j++) {
        const uint32_t q = v / d;
        v -= q * d;
        if (q) started = true;
        if (started && j < keep) s.put('0' + q);
        d /= 10;
    }
}

template <typename S>
__host__ __device__ __forceinline__ void put_u64(S& s, uint64_t v) {
    const uint32_t c0 = (uint32_t)(v % 1000000000ull);
    const uint64_t t = v / 1000000000ull;
    const uint32_t c1 = (uint32_t)(t % 1000000000ull), c2 = (uint32_t)(t / 1000000000ull);
    bool started = false;
    put_chunk9(s, c2, started);
    put_chunk9(s, c1, started);
    put_chunk9(s, c0, started);
    if (!started) s.put('0');
}

template <typename S>
__host__ __device__ __forceinline__ void put_i64(S& s, int64_t v) {
    if (v < 0) s.put('-');
    put_u64(s, v < 0 ? 0 - (uint64_t)v : (uint64_t)v);
}

// big.Int.String of a 256-bit magnitude: eight 32-bit limbs (most significant first) divided by 10^9
// nine times
template <typename S>
__host__ __device__ __forceinline__ void put_dec256_limbs(S& s, uint32_t limb[8]) {
    uint32_t chunk[9];
#pragma unroll
    for (int c = 0; c < 9; c++) {
        uint64_t rem = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint64_t cur = (rem << 32) | limb[j];
            limb[j] = (uint32_t)(cur / 1000000000ull);
            rem = cur % 1000000000ull;
        }
        chunk[c] = (uint32_t)rem;
    }
    bool started = false;
#pragma unroll
    for (int c = 8; c >= 0; c--) put_chunk9(s, chunk[c], started);
    if (!started) s.put('0');
}

// the same of 32 big-endian bytes
template <typename S>
__host__ __device__ __forceinline__ void put_dec256(S& s, const uint8_t* be) {
    uint32_t limb[8];
#pragma unroll
    for (int j = 0; j < 8; j++)
        limb[j] = ((uint32_t)be[4 * j] << 24) | ((uint32_t)be[4 * j + 1] << 16) | ((uint32_t)be[4 * j + 2] << 8) | be[4 * j + 3];
    put_dec256_limbs(s, limb);
}

template <typename S>
__host__ __device__ __forceinline__ void put_2d(S& s, uint32_t v) {
    s.put('0' + v / 10);
    s.put('0' + v % 10);
}

// time.Time.MarshalJSON of a UTC instant (RFC3339Nano): floor division below 1970, the fraction
// without its trailing zeros and absent when it is 0
template <typename S>
__host__ __device__ __forceinline__ void put_rfc3339nano(S& s, int64_t unix_ns) {
    int64_t secs = unix_ns / 1000000000ll, nsec = unix_ns % 1000000000ll;
    if (nsec < 0) { nsec += 1000000000ll; secs -= 1; }
    int64_t days = secs / 86400, sod = secs % 86400;
    if (sod < 0) { sod += 86400; days -= 1; }
    // civil date of a day count (proleptic Gregorian)
    const int64_t z = days + 719468;
    const int64_t era = (z >= 0 ? z : z - 146096) / 146097;
    const uint32_t doe = (uint32_t)(z - era * 146097);
    const uint32_t yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
    const uint32_t doy = doe - (365 * yoe + yoe / 4 - yoe / 100);
    const uint32_t mp = (5 * doy + 2) / 153;
    const uint32_t d = doy - (153 * mp + 2) / 5 + 1, m = mp < 10 ? mp + 3 : mp - 9;
    const uint32_t y = (uint32_t)((int64_t)yoe + era * 400 + (m <= 2));   // 1677..2262 for an int64 of ns
    put_2d(s, y / 100); put_2d(s, y % 100); s.put('-'); put_2d(s, m); s.put('-'); put_2d(s, d); s.put('T');
    const uint32_t so = (uint32_t)sod;
    put_2d(s, so / 3600); s.put(':'); put_2d(s, (so / 60) % 60); s.put(':'); put_2d(s, so % 60);
    if (nsec) {
        uint32_t f = (uint32_t)nsec;
        int keep = 9;
        while (f % 10 == 0) { f /= 10; keep--; }
        s.put('.');
        bool started = true;
        put_chunk9(s, (uint32_t)nsec, started, keep);
    }
    s.put('Z');
}

// The event columns of one chunk on the device (one lane reads row k)
struct EvCols {
    const int32_t* creator;
    const int64_t *index, *sp, *op, *ts;
    const uint8_t *r, *s;
    const int32_t* ntx;
    const int64_t* txi;      // [m] the event's first entry of tx_off
    const int64_t* tx_off;   // offsets into tx_bytes
    const uint8_t* tx_bytes;
    const uint8_t* keys65;   // [n_keys][65]
    const uint8_t *sp_id, *op_id;   // [m][32] the parents' ids, or null: the slots stay open
    const uint8_t* root_has_x;      // [n_keys] the creator's Root.X has an id (§3.12), or null: no root ids
    int32_t open_sig;               // the signing path (§3.16): r / s are not read, the tail behind the body stays open
};

// The tail of an event's text behind its body, at its longest: ,"R": and ,"S": with 78 digits each, }\n
constexpr int kSigTailMax = 5 + 78 + 5 + 78 + 2;

// The roots' ids (Engine::set_root_ids, §3.12): the text of parents that are in no id column. All null
// on a context without root ids.
struct RootIds {
    const uint8_t *x_id, *y_id;      // [C][32]
    const uint8_t *has_x, *has_y;    // [C]
    const uint64_t* pairs;           // [n_pairs][8] Root.Others: key (4 big-endian words), value (32 bytes)
    int64_t n_pairs;
};

// Event k's text into the sink; slot = where the self-parent string starts, body_end = one past the
// body's closing brace (the body starts at byte 8)
template <typename S>
__host__ __device__ __forceinline__ void encode_event(S& s, const EvCols& c, int64_t k, int64_t& slot, int64_t& body_end) {
    put_str(s, "{\"Body\":{\"Transactions\":");
    const int ntx = c.ntx[k];
    if (ntx < 0) {
        put_str(s, "null");
    } else {
        s.put('[');
        const int64_t t0 = c.txi[k];
        for (int i = 0; i < ntx; i++) {
            if (i) s.put(',');
            s.put('"');
            const int64_t a = c.tx_off[t0 + i];
            put_base64(s, c.tx_bytes + a, c.tx_off[t0 + i + 1] - a);
            s.put('"');
        }
        s.put(']');
    }
    put_str(s, ",\"Parents\":[\"");
    slot = s.n;
    // ("" for -1, except on a context with root ids where the creator's Root.X has one)
    if (c.sp[k] != -1 || (c.root_has_x && c.root_has_x[c.creator[k]])) {
        if (c.sp_id) put_hex_id<false>(s, c.sp_id + 32 * k);
        else s.skip(66);
    }
    put_str(s, "\",\"");
    if (c.op[k] != -1) {
        if (c.op_id) put_hex_id<false>(s, c.op_id + 32 * k);
        else s.skip(66);
    }
    put_str(s, "\"],\"Creator\":\"");
    put_base64(s, c.keys65 + 65 * (int64_t)c.creator[k], 65);
    put_str(s, "\",\"Timestamp\":\"");
    put_rfc3339nano(s, c.ts[k]);
    put_str(s, "\",\"Index\":");
    put_i64(s, c.index[k]);
    s.put('}');
    body_end = s.n;
    if (c.open_sig) {   // sized for the longest R and S; k_ev_sign_ids writes the tail and the true length
        s.skip(kSigTailMax);
    } else {
        put_str(s, ",\"R\":");
        put_dec256(s, c.r + 32 * k);
        put_str(s, ",\"S\":");
        put_dec256(s, c.s + 32 * k);
        put_str(s, "}\n");
    }
    s.finish();
}

// ---- kernels ------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_ev_size(int64_t m, EvCols c, int64_t* __restrict__ len) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    CountSink s;
    int64_t slot, body_end;
    encode_event(s, c, k, slot, body_end);
    len[k] = s.n;
}

// off[0] = 0, off[k + 1] = off[k] + len[k] rounded up to `align` (a power of two): one workgroup,
// every lane sums a contiguous run, the runs' sums are scanned in LDS
__global__ void __launch_bounds__(1024) k_ev_scan(int64_t m, const int64_t* __restrict__ len, int64_t align,
                                                  int64_t* __restrict__ off) {
    __shared__ int64_t part[1024];
    const int t = threadIdx.x;
    const int64_t per = (m + 1023) / 1024, a = std::min(m, t * per), b = std::min(m, a + per);
    int64_t sum = 0;
    for (int64_t k = a; k < b; k++) sum += (len[k] + align - 1) & ~(align - 1);
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int64_t v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int64_t run = part[t] - sum;
    if (t == 0) off[0] = 0;
    for (int64_t k = a; k < b; k++) {
        run += (len[k] + align - 1) & ~(align - 1);
        off[k + 1] = run;
    }
}

__global__ void __launch_bounds__(256) k_ev_write(int64_t m, EvCols c, const int64_t* __restrict__ off,
                                                  uint8_t* __restrict__ text, int64_t* __restrict__ slot,
                                                  int64_t* __restrict__ body_len) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    ByteSink s(text + off[k]);
    int64_t sl, body_end;
    encode_event(s, c, k, sl, body_end);
    if (slot) slot[k] = sl;
    if (body_len) body_len[k] = body_end - 8;
}

// Event k's parents' hex ids into the open slots of its text, which start at text + at (s0 / o0 = its
// parent columns; every parent source: see k_ev_ids)
__device__ __forceinline__ void patch_parents(int64_t k, int64_t s0, int64_t o0, int64_t at, int64_t base,
                                              const uint8_t* store_id, uint8_t* text, const uint8_t* ids,
                                              const int32_t* __restrict__ creator, const RootIds& rt,
                                              const uint8_t* op_rid) {
    const uint8_t* src = nullptr;
    if (s0 >= 0) src = s0 < base ? store_id + 32 * s0 : ids + 32 * (s0 - base);
    else if (rt.has_x && rt.has_x[creator[k]]) src = rt.x_id + 32 * (int64_t)creator[k];
    if (src) {
        ByteSink w(text + at);
        put_hex_id<true>(w, src);
        w.finish();
        at += 66;
    }
    src = nullptr;
    if (o0 >= 0) src = o0 < base ? store_id + 32 * o0 : ids + 32 * (o0 - base);
    else if (o0 == kRootY && rt.y_id) src = rt.y_id + 32 * (int64_t)creator[k];
    else if (o0 == kRootOther) src = op_rid ? op_rid + 32 * k : nullptr;
    if (src) {
        ByteSink w(text + at + 3);
        put_hex_id<true>(w, src);
        w.finish();
    }
}

// The id pass. Workgroup j owns one graph's events of the chunk, grouped by dependency level
// (LevelPlan); level after level its lanes stride over the level's events: patch the parents' hex ids
// into the open slots (a parent below `base` from the store's id column, a later one from this
// chunk's ids; on a context with root ids self-parent -1 from the creator's Root.X row, HGX_ROOT_Y
// from its Root.Y row and HGX_ROOT_OTHER from the staged op_rid row: level 0, tables written before
// the launch), hash the text, store the id. A level's ids are complete before the next level reads
// them: agent-scope fence, barrier, fence; the ids are read past L1. Every lane of the workgroup runs
// the same wg_nl[j] rounds, and no workgroup waits for another.
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(4)))
k_ev_ids(const int32_t* __restrict__ wg_lo, const int32_t* __restrict__ wg_nl, const int32_t* __restrict__ loff,
         const int32_t* __restrict__ pos, const int64_t* __restrict__ sp, const int64_t* __restrict__ op,
         const int64_t* __restrict__ off, const int64_t* __restrict__ len, const int64_t* __restrict__ slot,
         int64_t base, const uint8_t* store_id, uint8_t* text, uint8_t* ids, const int32_t* __restrict__ creator,
         RootIds rt, const uint8_t* op_rid) {
    const int32_t lo = wg_lo[blockIdx.x], nl = wg_nl[blockIdx.x];
    for (int32_t l = 0; l < nl; l++) {
        const int32_t a = loff[lo + l], b = loff[lo + l + 1];
        for (int32_t i = a + (int32_t)threadIdx.x; i < b; i += (int32_t)blockDim.x) {
            const int64_t k = pos[i];
            const int64_t o = off[k];
            patch_parents(k, sp[k], op[k], o + slot[k], base, store_id, text, ids, creator, rt, op_rid);
            sha256_message<false>(text, o, len[k], 0, (uint32_t*)(ids + 32 * k));
        }
        __threadfence();
        __syncthreads();
        __threadfence();
    }
}

// The flat id pass (hgx_insert_event_bodies_claimed): the caller supplies every event's
// claimed id, so no event waits for its parents' hashes. One lane per chunk event, no level plan, no
// fence, no barrier: patch the parents' hex ids with the chunk's CLAIMED column as the in-chunk source
// (resident parents from the store's id column, root codes from the root tables and op_rid, as in
// k_ev_ids), hash the text into the separate computed column (other lanes read the claimed column, which
// is never written), compare the 32 bytes. A difference files the chunk position in *first, the verified
// insert's signature word (kInsIdWordCode in its low byte: at one position it sorts before Verify's
// codes). By induction in gid order the smallest filed position m is exact and every event before it is
// proven; ids computed behind m may rest on a wrong parent id and are dropped with the rejected tail.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4)))
k_ev_ids_claimed(int64_t m, const int64_t* __restrict__ sp, const int64_t* __restrict__ op,
                 const int64_t* __restrict__ off, const int64_t* __restrict__ len, const int64_t* __restrict__ slot,
                 int64_t base, const uint8_t* store_id, uint8_t* text, const uint8_t* claimed, uint8_t* __restrict__ ids,
                 const int32_t* __restrict__ creator, RootIds rt, const uint8_t* op_rid, unsigned long long* first) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    const int64_t o = off[k];
    patch_parents(k, sp[k], op[k], o + slot[k], base, store_id, text, claimed, creator, rt, op_rid);
    uint32_t h[8];
    sha256_message<false>(text, o, len[k], 0, h);
    const uint32_t* want = (const uint32_t*)(claimed + 32 * k);
    uint32_t diff = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        ((uint32_t*)(ids + 32 * k))[j] = h[j];
        diff |= h[j] ^ want[j];
    }
    if (diff) atomicMin(first, ((unsigned long long)k << 8) | (unsigned long long)kInsIdWordCode);
}

// What the signing id pass reads of a staged chunk (k_ev_ids' parameters)
struct IdPass {
    const int32_t *wg_lo, *wg_nl, *loff, *pos;
    const int64_t *sp, *op, *off, *slot;
    int64_t base;
    const uint8_t* store_id;
    uint8_t *text, *ids;
    const int32_t* creator;
    RootIds rt;
    const uint8_t* op_rid;
};

// The signing twin of k_ev_ids (hgx_sign_insert_event_bodies): the same level plan and
// the same fence / barrier / fence between levels; an event of a level gets its parents' ids patched in,
// its body digest (EventBody.Hash: the body plus '\n'), R and S from p256_sign_one under its creator's
// private key (priv32 [C][32]; tg = the base point's comb table), both into the chunk's own R / S columns
// and, with the digest, to where the verified insert reads them; then the tail ,"R":<dec>,"S":<dec>}\n
// behind the body (the write pass left kSigTailMax bytes open), the text's true length into len[k], and
// the id = SHA-256 of the text. kSignBlock lanes per workgroup at one wave per SIMD: no scratch.
__global__ void __launch_bounds__(kSignBlock)
k_ev_sign_ids(IdPass p, int64_t* __restrict__ len, const int64_t* __restrict__ body_len,
              const uint8_t* __restrict__ priv32, const uint32_t* __restrict__ tg, uint8_t* __restrict__ col_r,
              uint8_t* __restrict__ col_s, uint8_t* __restrict__ dig) {
    const int32_t lo = p.wg_lo[blockIdx.x], nl = p.wg_nl[blockIdx.x];
    for (int32_t l = 0; l < nl; l++) {
        const int32_t a = p.loff[lo + l], b = p.loff[lo + l + 1];
        for (int32_t i = a + (int32_t)threadIdx.x; i < b; i += (int32_t)blockDim.x) {
            const int64_t k = p.pos[i];
            const int64_t o = p.off[k], bl = body_len[k];
            patch_parents(k, p.sp[k], p.op[k], o + p.slot[k], p.base, p.store_id, p.text, p.ids, p.creator, p.rt, p.op_rid);
            uint32_t dg[8];   // the digest's bytes in memory order
            sha256_message<true>(p.text, o + 8, bl, '\n', dg);
            p256::Fe d, e, r, s;
            p256::load_be_words(d, priv32 + 32 * (int64_t)p.creator[k]);
#pragma unroll
            for (int j = 0; j < 8; j++) {
                e[7 - j] = __builtin_bswap32(dg[j]);
                ((uint32_t*)(dig + 32 * k))[j] = dg[j];
            }
            p256::p256_sign_one(r, s, d, e, tg);
            p256::store_be(col_r + 32 * k, r);
            p256::store_be(col_s + 32 * k, s);
            ByteSink w(p.text + o + 8 + bl);
            uint32_t limb[8];
            put_str(w, ",\"R\":");
#pragma unroll
            for (int j = 0; j < 8; j++) limb[j] = r[7 - j];
            put_dec256_limbs(w, limb);
            put_str(w, ",\"S\":");
#pragma unroll
            for (int j = 0; j < 8; j++) limb[j] = s[7 - j];
            put_dec256_limbs(w, limb);
            put_str(w, "}\n");
            w.finish();
            const int64_t tl = 8 + bl + w.n;
            len[k] = tl;
            sha256_message<false>(p.text, o, tl, 0, (uint32_t*)(p.ids + 32 * k));
        }
        __threadfence();
        __syncthreads();
        __threadfence();
    }
}

// The value check of Root.Others (hashgraph.go:437-440: Root.Others[event.Hex()] == OtherParent), one
// lane per chunk event, after the ids are known and before the insert: an HGX_ROOT_OTHER event whose
// id is no key of the pairs, or whose entry names another other-parent than the supplied one, gets
// HGX_UNKNOWN_PARENT in the staged column; k_insert_check then rejects it with CheckOtherParent's error
// at its place in the first-failure order.
__global__ void __launch_bounds__(256) k_ev_others(int64_t m, int64_t* __restrict__ op, const uint8_t* __restrict__ ids,
                                                   const uint8_t* __restrict__ op_rid, const uint64_t* __restrict__ pairs,
                                                   int64_t n_pairs) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m || op[k] != kRootOther) return;
    const uint8_t* h = ids + 32 * k;
    uint64_t q[4];
#pragma unroll
    for (int w = 0; w < 4; w++) {
        uint64_t x = 0;
        for (int b = 0; b < 8; b++) x = (x << 8) | h[8 * w + b];
        q[w] = x;
    }
    int64_t lo = 0, hi = n_pairs;
    while (lo < hi) {   // first key >= q
        const int64_t mid = (lo + hi) >> 1;
        const uint64_t* kk = pairs + 8 * mid;
        int cmp = 0;
        for (int w = 0; w < 4 && cmp == 0; w++) cmp = kk[w] < q[w] ? -1 : kk[w] > q[w] ? 1 : 0;
        if (cmp < 0) lo = mid + 1; else hi = mid;
    }
    bool ok = op_rid != nullptr && lo < n_pairs;
    if (ok) {
        const uint64_t* kk = pairs + 8 * lo;
        ok = kk[0] == q[0] && kk[1] == q[1] && kk[2] == q[2] && kk[3] == q[3];
        const uint8_t* v = (const uint8_t*)(kk + 4);
        for (int b = 0; b < 32 && ok; b++) ok = v[b] == op_rid[32 * k + b];
    }
    if (!ok) op[k] = HGX_UNKNOWN_PARENT;
}

// EventBody.Hash of every event: the body inside the event's text plus '\n'
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4)))
k_ev_digest(int64_t m, const uint8_t* __restrict__ text, const int64_t* __restrict__ off,
            const int64_t* __restrict__ body_len, uint8_t* __restrict__ dig) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    sha256_message<true>(text, off[k] + 8, body_len[k], '\n', (uint32_t*)(dig + 32 * k));
}

// ---- one chunk's buffers ------------------------------------------------------------------------
namespace {

struct DevMem {
    uint8_t* p = nullptr;
    size_t cap = 0;
    hipError_t need(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        const hipError_t e = hipMalloc((void**)&p, bytes);
        if (e == hipSuccess) cap = bytes;
        return e;
    }
    ~DevMem() { if (p) (void)hipFree(p); }
};

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

// The inputs of a chunk cross in one copy from a pinned blob; texts, lengths, ids and digests live in
// buffers that grow to the largest chunk seen (bounded by the chunk limits of hgx_bodies.h).
struct EvScratch {
    DevMem in, text, meta, ids;
    uint8_t* h = nullptr;
    size_t h_cap = 0;
    LevelPlan plan;
    std::vector<int32_t> level;
    // hgx_insert_wire_bodies: lo[n] | woff[n], then the window (4 bytes per slot); the
    // table goes up from a page-locked copy
    DevMem wire;
    DevMem blk_meta, blk_sz, blk_text, blk_out, blk_in;   // the block encoder (block_hashes_run)
    int32_t* h_wtab = nullptr;
    size_t h_wtab_cap = 0;
    ~EvScratch() {
        if (h) (void)hipHostFree(h);
        if (h_wtab) (void)hipHostFree(h_wtab);
    }

    // device views of the staged chunk
    EvCols cols{};
    const int32_t *d_wg_lo = nullptr, *d_wg_nl = nullptr, *d_loff = nullptr, *d_pos = nullptr;
    int64_t *d_len = nullptr, *d_off = nullptr, *d_slot = nullptr, *d_blen = nullptr;
    uint8_t *d_ids = nullptr, *d_dig = nullptr;
    const uint8_t* d_op_rid = nullptr;   // the staged ids of HGX_ROOT_OTHER other-parents, or null
    const uint8_t* d_claimed = nullptr;  // the staged claimed ids (the flat id pass), or null
    int64_t n_root_other = 0;            // the chunk's events with that code (counted when the column is staged)

    // Stage events [lo, hi) (m of them): columns, transactions, the parents' ids (json mode) or the
    // level plan (insert mode, base = gid of event lo), and on a context with root ids the Root.X flags
    // and the ids of the HGX_ROOT_OTHER other-parents (op_rid, may be null), and the claimed ids of the flat
    // id pass (claimed, may be null), in ONE host-to-device copy.
    hipError_t stage(const BodiesIn& ev, const std::vector<int64_t>& txi, int64_t lo, int64_t hi, const uint8_t* keys_dev,
                     const uint8_t* keys_host, int32_t n_keys, const uint8_t* sp_id, const uint8_t* op_id, bool with_plan,
                     int64_t base, int32_t n_per_graph, hipStream_t s, const uint8_t* root_has_x = nullptr,
                     const uint8_t* op_rid = nullptr, const uint8_t* claimed = nullptr) {
        const size_t m = (size_t)(hi - lo);
        const int64_t t0 = txi[(size_t)lo], t1 = txi[(size_t)hi];
        const size_t nt = (size_t)(t1 - t0);
        const int64_t b0 = ev.tx_off[t0];
        const size_t nbytes = (size_t)(ev.tx_off[t1] - b0);
        if (with_plan) {
            level.resize(m);
            int32_t nl = 0;
            (void)batch_levels(ev.sp + lo, ev.op + lo, (int64_t)m, base, level.data(), &nl);
            plan_levels(ev.creator + lo, level.data(), (int64_t)m, n_per_graph, plan);
        }
        const size_t nwg = with_plan ? plan.wg_lo.size() : 0, nloff = with_plan ? plan.loff.size() : 0;
        const void* src[16] = {ev.creator + lo, ev.index + lo, ev.sp + lo, ev.op + lo, ev.ts + lo,
                               ev.r ? ev.r + 32 * lo : nullptr,   // (null on the signing path: the device writes both)
                               ev.s ? ev.s + 32 * lo : nullptr, ev.ntx + lo, nullptr, nullptr, nbytes ? ev.tx_bytes + b0 : nullptr,
                               keys_host, sp_id ? sp_id + 32 * lo : nullptr, op_id ? op_id + 32 * lo : nullptr, nullptr,
                               nullptr};
        size_t bytes[20] = {4 * m, 8 * m, 8 * m, 8 * m, 8 * m, 32 * m, 32 * m, 4 * m, 8 * m, 8 * (nt + 1), nbytes,
                            keys_host ? (size_t)65 * (size_t)n_keys : 0, sp_id ? 32 * m : 0, op_id ? 32 * m : 0,
                            4 * nwg, 4 * nwg, 4 * nloff, with_plan ? 4 * m : 0, op_rid ? 32 * m : 0, claimed ? 32 * m : 0};
        size_t o[20], total = 0;
        for (int i = 0; i < 20; i++) {
            o[i] = total;
            // 16 spare bytes behind every column: the hash reader's aligned loads, and for tx_bytes
            // (o[10]) the shifted dword reads of k_body_append's copy_bytes, up to 7 bytes past the end
            total += up256(bytes[i] + 16);
        }
        if (h_cap < total) {
            if (h) (void)hipHostFree(h);
            h = nullptr;
            h_cap = 0;
            HGX_TRY(hipHostMalloc((void**)&h, total, hipHostMallocDefault));
            h_cap = total;
        }
        HGX_TRY(in.need(total));
        for (int i = 0; i < 14; i++)
            if (src[i] && bytes[i]) std::memcpy(h + o[i], src[i], bytes[i]);
        int64_t* h_txi = (int64_t*)(h + o[8]);
        for (size_t k = 0; k < m; k++) h_txi[k] = txi[(size_t)lo + k] - t0;
        int64_t* h_off = (int64_t*)(h + o[9]);
        for (size_t j = 0; j <= nt; j++) h_off[j] = ev.tx_off[t0 + (int64_t)j] - b0;
        if (with_plan) {
            if (nwg) std::memcpy(h + o[14], plan.wg_lo.data(), 4 * nwg);
            if (nwg) std::memcpy(h + o[15], plan.wg_nl.data(), 4 * nwg);
            if (nloff) std::memcpy(h + o[16], plan.loff.data(), 4 * nloff);
            std::memcpy(h + o[17], plan.pos.data(), 4 * m);
        }
        n_root_other = 0;
        if (op_rid) {
            std::memcpy(h + o[18], op_rid + 32 * lo, 32 * m);
            for (int64_t k = lo; k < hi; k++) n_root_other += ev.op[k] == HGX_ROOT_OTHER;
        }
        if (claimed) std::memcpy(h + o[19], claimed + 32 * lo, 32 * m);
        HGX_TRY(hipMemcpyAsync(in.p, h, total, hipMemcpyHostToDevice, s));
        uint8_t* d = in.p;
        cols.creator = (const int32_t*)(d + o[0]); cols.index = (const int64_t*)(d + o[1]);
        cols.sp = (const int64_t*)(d + o[2]); cols.op = (const int64_t*)(d + o[3]); cols.ts = (const int64_t*)(d + o[4]);
        cols.r = d + o[5]; cols.s = d + o[6]; cols.ntx = (const int32_t*)(d + o[7]);
        cols.txi = (const int64_t*)(d + o[8]); cols.tx_off = (const int64_t*)(d + o[9]); cols.tx_bytes = d + o[10];
        cols.keys65 = keys_host ? d + o[11] : keys_dev;
        cols.sp_id = sp_id ? d + o[12] : nullptr; cols.op_id = op_id ? d + o[13] : nullptr;
        cols.root_has_x = root_has_x;
        d_op_rid = op_rid ? d + o[18] : nullptr;
        d_claimed = claimed ? d + o[19] : nullptr;
        d_wg_lo = (const int32_t*)(d + o[14]); d_wg_nl = (const int32_t*)(d + o[15]);
        d_loff = (const int32_t*)(d + o[16]); d_pos = (const int32_t*)(d + o[17]);
        // lengths, offsets (m + 1), slots, body lengths; ids and digests (16-byte aligned)
        HGX_TRY(meta.need(up256(8 * m) * 3 + up256(8 * (m + 1))));
        d_len = (int64_t*)meta.p; d_off = (int64_t*)(meta.p + up256(8 * m));
        d_slot = (int64_t*)((uint8_t*)d_off + up256(8 * (m + 1))); d_blen = (int64_t*)((uint8_t*)d_slot + up256(8 * m));
        HGX_TRY(ids.need(2 * up256(32 * m)));
        d_ids = ids.p; d_dig = ids.p + up256(32 * m);
        return hipSuccess;
    }

    hipError_t size_and_scan(int64_t m, int64_t align, hipStream_t s) {
        const unsigned blocks = (unsigned)((m + 255) / 256);
        hipLaunchKernelGGL(k_ev_size, dim3(blocks), dim3(256), 0, s, m, cols, d_len);
        hipLaunchKernelGGL(k_ev_scan, dim3(1), dim3(1024), 0, s, m, (const int64_t*)d_len, align, d_off);
        return hipGetLastError();
    }

    hipError_t write(int64_t m, size_t text_bytes, bool with_meta, hipStream_t s) {
        HGX_TRY(text.need(text_bytes + 64));
        const unsigned blocks = (unsigned)((m + 255) / 256);
        hipLaunchKernelGGL(k_ev_write, dim3(blocks), dim3(256), 0, s, m, cols, (const int64_t*)d_off, text.p,
                           with_meta ? d_slot : nullptr, with_meta ? d_blen : nullptr);
        return hipGetLastError();
    }
};

void free_ev_scratch(EvScratch* p) { delete p; }

// InsertEvent with Event.Hash and Event.Verify computed here (hgx_insert_event_bodies): chunk after
// chunk, texts -> ids in level order -> body digests -> insert_verified with the chunk's id buffer
// as the hash column. Stops at the first chunk with a rejected event; out is the last insert's with
// accepted = the whole call's. Every event of [0, count) has a text (the caller cut the batch).
// On a context with root ids (§3.12) the encoder and the id pass read the root tables, op_id32 is staged
// with each chunk and the Others value check runs before the insert.
hipError_t Engine::insert_bodies(const BodiesIn& ev, const std::vector<int64_t>& txi, int64_t count, const uint8_t* op_id32,
                                 uint8_t* out_id32, InsertOut& out) {
    return insert_bodies_run(ev, txi, count, op_id32, out_id32, out, nullptr);
}

// Core.SignAndInsertSelfEvent for a batch (hgx_sign_insert_event_bodies): the same chunks
// with the texts' tails open, k_ev_sign_ids in place of k_ev_ids and k_ev_digest, and the verified insert
// reading the R / S columns and the digests the device wrote. ev.r / ev.s are not read.
hipError_t Engine::sign_insert_bodies(const BodiesIn& ev, const std::vector<int64_t>& txi, int64_t count,
                                      const uint8_t* op_id32, uint8_t* out_r32, uint8_t* out_s32, uint8_t* out_id32,
                                      InsertOut& out) {
    const SignOut so{out_r32, out_s32};
    return insert_bodies_run(ev, txi, count, op_id32, out_id32, out, nullptr, &so);
}

// The flat route (hgx_insert_event_bodies_claimed): claimed_id32 (host, [count][32]) stands
// for the ids of in-call parents, k_ev_ids_claimed proves it; the first wrong claimed id ends the call
// with INS_ID_MISMATCH behind the proven prefix, unless that prefix has a failure of its own.
hipError_t Engine::insert_bodies_claimed(const BodiesIn& ev, const std::vector<int64_t>& txi, int64_t count,
                                         const uint8_t* op_id32, const uint8_t* claimed_id32, InsertOut& out) {
    if (!claimed_id32) return hipErrorInvalidValue;
    return insert_bodies_run(ev, txi, count, op_id32, nullptr, out, nullptr, nullptr, claimed_id32);
}

// The wire route (hgx_insert_wire_bodies): the window of the resident parents is filled once, against
// the events resident before the call; a later chunk's parents in an earlier chunk are final gids.
hipError_t Engine::insert_wire_bodies(const BodiesIn& ev, const std::vector<int64_t>& txi, int64_t count,
                                      const WireWindows& w, uint8_t* out_id32, int64_t* out_sp, int64_t* out_op,
                                      InsertOut& out) {
    if (G != 1 || n > 1024 || w.slots < 0 || w.slots > E) return hipErrorInvalidValue;
    if (!ev_scratch) ev_scratch = new EvScratch();
    EvScratch& sc = *ev_scratch;
    WireRun run{nullptr, 0, out_sp, out_op};
    if (count > 0 && w.n_resident > 0) {
        const size_t tab = up256(8 * (size_t)n);
        HGX_TRY(sc.wire.need(tab + 4 * (size_t)w.slots));
        if (sc.h_wtab_cap < tab) {
            if (sc.h_wtab) (void)hipHostFree(sc.h_wtab);
            sc.h_wtab = nullptr;
            sc.h_wtab_cap = 0;
            HGX_TRY(hipHostMalloc((void**)&sc.h_wtab, tab, hipHostMallocDefault));
            sc.h_wtab_cap = tab;
        }
        std::memcpy(sc.h_wtab, w.lo, 4 * (size_t)n);
        std::memcpy(sc.h_wtab + n, w.woff, 4 * (size_t)n);
        int32_t* win = (int32_t*)(sc.wire.p + tab);
        HGX_TRY(hipMemcpyAsync(sc.wire.p, sc.h_wtab, 8 * (size_t)n, hipMemcpyHostToDevice, stream));
        HGX_TRY(hipMemsetAsync(win, 0xFF, 4 * (size_t)w.slots, stream));   // -1: a slot nobody filled
        launch_wire_window(stream, WireWinArgs{E, n, g_creator.p, g_index.p, (const int32_t*)sc.wire.p, win, w.slots});
        HGX_TRY(hipGetLastError());
        run.win = win;
        run.slots = w.slots;
    }
    return insert_bodies_run(ev, txi, count, nullptr, out_id32, out, &run);
}

hipError_t Engine::insert_bodies_run(const BodiesIn& ev, const std::vector<int64_t>& txi, int64_t count,
                                     const uint8_t* op_id32, uint8_t* out_id32, InsertOut& out, const WireRun* wire,
                                     const SignOut* sign, const uint8_t* claimed) {
    if (sign && !sign_keys_set) return hipErrorNotReady;
    if (claimed && (sign || wire)) return hipErrorInvalidValue;
    if (!ev_scratch) ev_scratch = new EvScratch();
    EvScratch& sc = *ev_scratch;
    int64_t done = 0;
    out = InsertOut();
    RootIds rt{};
    if (root_ids_set) {
        const uint8_t* t = root_tab_d.p;
        rt = RootIds{t, t + 32 * (size_t)C, t + 64 * (size_t)C, t + 65 * (size_t)C, root_pairs_d.p, n_root_pairs};
    } else {
        op_id32 = nullptr;
    }
    if (count <= 0) return insert_verified(InsertIn{}, nullptr, nullptr, 0, out);
    while (done < count) {
        int64_t bound = 0;
        const int64_t hi = bodies_chunk_end(ev, txi, done, count, &bound);
        const int64_t m = hi - done;
        // a keeping context: room for the whole chunk before any of it is inserted
        const bool keep = bodies_state == kBodiesComplete && bodies_events == E;
        const int64_t t_lo = txi[(size_t)done];
        if (keep && bodies_reserve(txi[(size_t)hi] - t_lo, ev.tx_off[txi[(size_t)hi]] - ev.tx_off[t_lo]) != hipSuccess) {
            InsertOut co;   // the earlier chunks stay inserted: their state, and the store's own failure code
            HGX_TRY(insert_verified(InsertIn{}, nullptr, nullptr, 0, co));
            out = std::move(co);
            out.accepted = done;
            out.code = INS_BODY_CAPACITY;
            break;
        }
        // (the flat pass needs no level plan: neither hgx_batch_levels nor the (graph, level) sort runs)
        HGX_TRY(sc.stage(ev, txi, done, hi, pk_keys.p, nullptr, C, nullptr, nullptr, claimed == nullptr, E, n, stream,
                         rt.has_x, op_id32, claimed));
        sc.cols.open_sig = sign ? 1 : 0;
        if (wire && wire->win)   // window descriptors -> gids, before the encoder reads the parent columns
            launch_wire_resolve(stream, m, const_cast<int64_t*>(sc.cols.sp), const_cast<int64_t*>(sc.cols.op), wire->win,
                                wire->slots, ins_fail.p);
        HGX_TRY(sc.size_and_scan(m, 16, stream));
        HGX_TRY(sc.write(m, (size_t)bound, true, stream));
        const IdPass idp{sc.d_wg_lo, sc.d_wg_nl, sc.d_loff, sc.d_pos, sc.cols.sp, sc.cols.op, sc.d_off, sc.d_slot, E,
                         g_id.p, sc.text.p, sc.d_ids, sc.cols.creator, rt, sc.d_op_rid};
        if (claimed) {
            // the verified insert's signature word, armed here: the mismatches and Verify's failures share it
            if (ins_fail_sig.n < 1) HGX_TRY(ins_fail_sig.alloc(1));
            HGX_TRY(hipMemsetAsync(ins_fail_sig.p, 0xFF, 8, stream));
            hipLaunchKernelGGL(k_ev_ids_claimed, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, stream, m, sc.cols.sp,
                               sc.cols.op, (const int64_t*)sc.d_off, (const int64_t*)sc.d_len, (const int64_t*)sc.d_slot, E,
                               (const uint8_t*)g_id.p, sc.text.p, sc.d_claimed, sc.d_ids, sc.cols.creator, rt, sc.d_op_rid,
                               ins_fail_sig.p);
        } else if (sign) {
            // a level's lanes stride over its events: the signer's workgroup is one wave whatever the width
            hipLaunchKernelGGL(k_ev_sign_ids, dim3((unsigned)sc.plan.wg_lo.size()), dim3(kSignBlock), 0, stream, idp, sc.d_len,
                               (const int64_t*)sc.d_blen, (const uint8_t*)sk_keys.p,
                               (const uint32_t*)(pk_tab.p + (size_t)C * kP256TabWords), const_cast<uint8_t*>(sc.cols.r),
                               const_cast<uint8_t*>(sc.cols.s), sc.d_dig);
        } else {
            const int bs = std::min(1024, std::max(64, (sc.plan.max_width + 63) & ~63));
            hipLaunchKernelGGL(k_ev_ids, dim3((unsigned)sc.plan.wg_lo.size()), dim3(bs), 0, stream, sc.d_wg_lo, sc.d_wg_nl,
                               sc.d_loff, sc.d_pos, sc.cols.sp, sc.cols.op, (const int64_t*)sc.d_off,
                               (const int64_t*)sc.d_len, (const int64_t*)sc.d_slot, E, (const uint8_t*)g_id.p, sc.text.p,
                               sc.d_ids, sc.cols.creator, rt, sc.d_op_rid);
        }
        if (sc.n_root_other)
            hipLaunchKernelGGL(k_ev_others, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, stream, m,
                               const_cast<int64_t*>(sc.cols.op), (const uint8_t*)sc.d_ids, sc.d_op_rid, rt.pairs, rt.n_pairs);
        if (!sign)   // (the signing id pass stored the digests it signed)
            hipLaunchKernelGGL(k_ev_digest, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, stream, m,
                               (const uint8_t*)sc.text.p, (const int64_t*)sc.d_off, (const int64_t*)sc.d_blen, sc.d_dig);
        HGX_TRY(hipGetLastError());
        InsertIn in{};
        in.creator = sc.cols.creator; in.index = sc.cols.index; in.sp = sc.cols.sp; in.op = sc.cols.op;
        in.ts = sc.cols.ts; in.hash = sc.d_ids; in.S = sc.cols.s; in.ntx = sc.cols.ntx; in.nil = nullptr;
        InsertOut co;
        HGX_TRY(insert_verified(in, sc.d_dig, sc.cols.r, m, co, claimed != nullptr));
        // (a prefix cut by a word without a code: the flat pass's, which no check of the prefix came before)
        if (claimed && co.code == INS_OK && co.accepted < m) co.code = INS_ID_MISMATCH;
        if (keep && co.accepted > 0) {   // the accepted prefix's R rows, slots, offsets and bytes (one launch)
            const int64_t t_hi = txi[(size_t)(done + co.accepted)];
            HGX_TRY(bodies_append(sc.cols.r, sc.cols.txi, sc.cols.tx_off, sc.cols.tx_bytes, co.accepted, t_hi - t_lo,
                                  ev.tx_off[t_hi] - ev.tx_off[t_lo]));
        }
        if (wire && wire->win && co.code) {
            // a window slot nobody filled made this event fail its checks: that bug is the finding
            int64_t par[2] = {0, 0};
            HGX_TRY(hipMemcpyAsync(&par[0], sc.cols.sp + co.accepted, 8, hipMemcpyDeviceToHost, stream));
            HGX_TRY(hipMemcpyAsync(&par[1], sc.cols.op + co.accepted, 8, hipMemcpyDeviceToHost, stream));
            HGX_TRY(hipStreamSynchronize(stream));
            if (par[0] == kWireHoleParent || par[1] == kWireHoleParent) co.code = INS_WIRE_HOLE;
        }
        const bool want_par = wire && (wire->out_sp || wire->out_op);
        const bool want_sig = sign && (sign->out_r || sign->out_s);
        if ((out_id32 || want_par || want_sig) && co.accepted > 0) {
            const size_t acc = (size_t)co.accepted;
            if (sign && sign->out_r)
                HGX_TRY(hipMemcpyAsync(sign->out_r + 32 * done, sc.cols.r, 32 * acc, hipMemcpyDeviceToHost, stream));
            if (sign && sign->out_s)
                HGX_TRY(hipMemcpyAsync(sign->out_s + 32 * done, sc.cols.s, 32 * acc, hipMemcpyDeviceToHost, stream));
            if (out_id32) HGX_TRY(hipMemcpyAsync(out_id32 + 32 * done, sc.d_ids, 32 * acc, hipMemcpyDeviceToHost, stream));
            if (wire && wire->out_sp)
                HGX_TRY(hipMemcpyAsync(wire->out_sp + done, sc.cols.sp, 8 * acc, hipMemcpyDeviceToHost, stream));
            if (wire && wire->out_op)
                HGX_TRY(hipMemcpyAsync(wire->out_op + done, sc.cols.op, 8 * acc, hipMemcpyDeviceToHost, stream));
            HGX_TRY(hipStreamSynchronize(stream));
        }
        done += co.accepted;
        const int64_t total = done;
        out = std::move(co);
        out.accepted = total;
        if (out.code) break;
    }
    return hipSuccess;
}


// ---- Block.Hash (block.go:44-53) for a batch of blocks -----------------------
// The block text is hgx_block_hash's: {"RoundReceived":N,"Transactions":T}\n with T = null for a nil
// list without transactions, else [ "<std base64, padded>", ... ]. The texts are laid out as elements,
// block b's head at element tx0[b] + b and its transactions behind it: the head carries everything up
// to and including '[' (or the whole rest of a block without transactions), a transaction its quoted
// base64 and the comma, or "]}\n" behind the block's last one. One more element of size 0 ends the
// array, so the scan's value at a block's head is where its text starts.
struct BlkArgs {
    int64_t count, T;
    const int64_t* rr;       // [count]
    const int64_t* tx0;      // [count + 1] first transaction of each block
    const int32_t* nil;      // [count]
    const int32_t* tx_blk;   // [T] the block of each transaction
    const int64_t* off;      // [T + 1] offsets into bytes
    const uint8_t* bytes;
    uint32_t* sz;            // [T + count + 1] element sizes, then their exclusive scan
    int64_t* starts;         // [count + 1] text start of each block
};

__device__ __forceinline__ int blk_decimal(int64_t v, char* buf) {   // digits (and '-') of v, returns the length
    char tmp[20];
    int n = 0;
    const bool neg = v < 0;
    do {
        const int d = (int)(v % 10);
        tmp[n++] = (char)('0' + (d < 0 ? -d : d));
        v /= 10;
    } while (v != 0);
    int len = 0;
    if (neg) buf[len++] = '-';
    while (n > 0) buf[len++] = tmp[--n];
    return len;
}

__device__ __forceinline__ int blk_decimal_len(int64_t v) {
    int len = v < 0 ? 1 : 0;
    do {
        len++;
        v /= 10;
    } while (v != 0);
    return len;
}

__global__ void __launch_bounds__(256) k_blk_size(BlkArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.count) {
        const int64_t nt = a.tx0[i + 1] - a.tx0[i];
        uint32_t s = 17 + (uint32_t)blk_decimal_len(a.rr[i]) + 16;
        s += nt > 0 ? 1u : (a.nil[i] ? 6u : 4u);   // "["  |  "null}\n"  |  "[]}\n"
        a.sz[a.tx0[i] + i] = s;
    }
    if (i < a.T) {
        const int32_t b = a.tx_blk[i];
        const int64_t l = a.off[i + 1] - a.off[i];
        a.sz[i + b + 1] = (uint32_t)(4 * ((l + 2) / 3) + 2 + (i + 1 == a.tx0[b + 1] ? 3 : 1));
    }
    if (i == 0) a.sz[a.T + a.count] = 0;
}

__global__ void __launch_bounds__(256) k_blk_starts(BlkArgs a) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b <= a.count) a.starts[b] = (int64_t)a.sz[a.tx0[b] + b];
}

// one thread per block of [b_lo, b_hi): the head (and the tail of a block without transactions)
__global__ void __launch_bounds__(256) k_blk_heads(BlkArgs a, int64_t b_lo, int64_t b_hi, int64_t base,
                                                   uint8_t* __restrict__ text) {
    const int64_t b = b_lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= b_hi) return;
    uint8_t* p = text + ((int64_t)a.sz[a.tx0[b] + b] - base);
    const char h1[] = "{\"RoundReceived\":", h2[] = ",\"Transactions\":";
    for (int k = 0; k < 17; k++) *p++ = (uint8_t)h1[k];
    char dec[20];
    const int nd = blk_decimal(a.rr[b], dec);
    for (int k = 0; k < nd; k++) *p++ = (uint8_t)dec[k];
    for (int k = 0; k < 16; k++) *p++ = (uint8_t)h2[k];
    if (a.tx0[b + 1] > a.tx0[b]) {
        *p = '[';
    } else if (a.nil[b]) {
        const char t[] = "null}\n";
        for (int k = 0; k < 6; k++) p[k] = (uint8_t)t[k];
    } else {
        const char t[] = "[]}\n";
        for (int k = 0; k < 4; k++) p[k] = (uint8_t)t[k];
    }
}

// a wave per transaction of [t_lo, t_hi), its lanes strided over the 3-byte groups
__global__ void __launch_bounds__(256) k_blk_txs(BlkArgs a, int64_t t_lo, int64_t t_hi, int64_t base,
                                                 uint8_t* __restrict__ text) {
    const int64_t j = t_lo + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= t_hi) return;
    const int lane = (int)(threadIdx.x & 63);
    const int32_t b = a.tx_blk[j];
    const int64_t l = a.off[j + 1] - a.off[j], ng = (l + 2) / 3;
    const uint8_t* src = a.bytes + a.off[j];
    uint8_t* p = text + ((int64_t)a.sz[j + b + 1] - base);
    for (int64_t g = lane; g < ng; g += 64) {
        const int64_t at = 3 * g;
        const int have = (int)(l - at < 3 ? l - at : 3);
        const uint32_t v = (uint32_t)src[at] << 16 | (have > 1 ? (uint32_t)src[at + 1] << 8 : 0u) |
                           (have > 2 ? (uint32_t)src[at + 2] : 0u);
        uint8_t* q = p + 1 + 4 * g;
        q[0] = (uint8_t)b64_char(v >> 18);
        q[1] = (uint8_t)b64_char((v >> 12) & 63);
        q[2] = have > 1 ? (uint8_t)b64_char((v >> 6) & 63) : (uint8_t)'=';
        q[3] = have > 2 ? (uint8_t)b64_char(v & 63) : (uint8_t)'=';
    }
    if (lane == 0) {
        p[0] = '"';
        uint8_t* q = p + 1 + 4 * ng;
        q[0] = '"';
        if (j + 1 == a.tx0[b + 1]) {
            q[1] = ']'; q[2] = '}'; q[3] = '\n';
        } else {
            q[1] = ',';
        }
    }
}

// Block.Hash of blocks [b_lo, b_hi): one lane per text
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4)))
k_blk_digest(BlkArgs a, int64_t b_lo, int64_t b_hi, int64_t base, const uint8_t* __restrict__ text,
             uint8_t* __restrict__ out) {
    const int64_t b = b_lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= b_hi) return;
    sha256_message<false>(text, a.starts[b] - base, a.starts[b + 1] - a.starts[b], 0, (uint32_t*)(out + 32 * b));
}

constexpr int64_t kBlkTextGroup = (int64_t)32 << 20;   // text scratch per group of blocks (§3.10's bound)

// The hashes of `count` blocks whose transactions are on the device (d_off [T + 1] offsets from any
// base into d_bytes, T = the sum of ntx): sizing pass, scan, then per group of at most kBlkTextGroup of
// text (a single larger block raises the bound to its size) write pass and SHA-256; the hashes come
// back in one copy. rr / ntx / nil are host arrays.
static hipError_t block_hashes_run(hipStream_t s, EvScratch& sc, const int64_t* rr, const int32_t* ntx, const int32_t* nil,
                                   int64_t count, const int64_t* d_off, const uint8_t* d_bytes, uint8_t* out32_host) {
    if (count <= 0) return hipSuccess;
    const size_t B = (size_t)count;
    std::vector<int64_t> tx0(B + 1, 0);
    for (size_t b = 0; b < B; b++) tx0[b + 1] = tx0[b] + (ntx[b] > 0 ? ntx[b] : 0);
    const size_t T = (size_t)tx0[B];
    if (T + B + 1 >= ((size_t)1 << 31)) return hipErrorInvalidValue;
    std::vector<int32_t> tx_blk(T);
    for (size_t b = 0; b < B; b++)
        for (int64_t j = tx0[b]; j < tx0[b + 1]; j++) tx_blk[(size_t)j] = (int32_t)b;
    const size_t o_rr = 0, o_tx0 = up256(8 * B), o_nil = o_tx0 + up256(8 * (B + 1)), o_blk = o_nil + up256(4 * B),
                 o_st = o_blk + up256(4 * T), meta = o_st + up256(8 * (B + 1));
    HGX_TRY(sc.blk_meta.need(meta));
    const size_t ne = T + B + 1, nparts = (ne + 2047) / 2048 + 1;
    HGX_TRY(sc.blk_sz.need(up256(4 * ne) + 4 * nparts));
    HGX_TRY(sc.blk_out.need(32 * B));
    uint8_t* m = sc.blk_meta.p;
    HGX_TRY(hipMemcpyAsync(m + o_rr, rr, 8 * B, hipMemcpyHostToDevice, s));
    HGX_TRY(hipMemcpyAsync(m + o_tx0, tx0.data(), 8 * (B + 1), hipMemcpyHostToDevice, s));
    HGX_TRY(hipMemcpyAsync(m + o_nil, nil, 4 * B, hipMemcpyHostToDevice, s));
    if (T) HGX_TRY(hipMemcpyAsync(m + o_blk, tx_blk.data(), 4 * T, hipMemcpyHostToDevice, s));
    BlkArgs a{count, (int64_t)T, (const int64_t*)(m + o_rr), (const int64_t*)(m + o_tx0), (const int32_t*)(m + o_nil),
              (const int32_t*)(m + o_blk), d_off, d_bytes, (uint32_t*)sc.blk_sz.p, (int64_t*)(m + o_st)};
    const size_t work = std::max(B, T);
    hipLaunchKernelGGL(k_blk_size, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, s, a);
    launch_scan_u32(s, a.sz, (int64_t)ne, (uint32_t*)(sc.blk_sz.p + up256(4 * ne)));
    hipLaunchKernelGGL(k_blk_starts, dim3((unsigned)((B + 1 + 255) / 256)), dim3(256), 0, s, a);
    HGX_TRY(hipGetLastError());
    std::vector<int64_t> starts(B + 1);
    HGX_TRY(hipMemcpyAsync(starts.data(), a.starts, 8 * (B + 1), hipMemcpyDeviceToHost, s));
    HGX_TRY(hipStreamSynchronize(s));   // (also: the host vectors above have been read)
    // the positions are 32-bit: the callers refused a batch whose text could reach 4 GiB
    // (block_text_fits, on the host in 64 bits), so the device's total is the true one
    if (!block_text_fits(starts[B])) return hipErrorInvalidValue;
    for (size_t b = 0; b < B; b++)
        if (starts[b + 1] < starts[b]) return hipErrorInvalidValue;
    for (int64_t lo = 0; lo < count;) {
        int64_t hi = lo + 1;
        while (hi < count && starts[(size_t)hi + 1] - starts[(size_t)lo] <= kBlkTextGroup) hi++;
        const int64_t base = starts[(size_t)lo], bytes = starts[(size_t)hi] - base;
        HGX_TRY(sc.blk_text.need((size_t)bytes + 64));
        hipLaunchKernelGGL(k_blk_heads, dim3((unsigned)((hi - lo + 255) / 256)), dim3(256), 0, s, a, lo, hi, base,
                           sc.blk_text.p);
        const int64_t t_lo = tx0[(size_t)lo], t_hi = tx0[(size_t)hi];
        if (t_hi > t_lo)
            hipLaunchKernelGGL(k_blk_txs, dim3((unsigned)((t_hi - t_lo + 3) / 4)), dim3(256), 0, s, a, t_lo, t_hi, base,
                               sc.blk_text.p);
        hipLaunchKernelGGL(k_blk_digest, dim3((unsigned)((hi - lo + 255) / 256)), dim3(256), 0, s, a, lo, hi, base,
                           (const uint8_t*)sc.blk_text.p, sc.blk_out.p);
        HGX_TRY(hipGetLastError());
        lo = hi;
    }
    HGX_TRY(hipMemcpyAsync(out32_host, sc.blk_out.p, 32 * B, hipMemcpyDeviceToHost, s));
    return hipStreamSynchronize(s);
}

// hgx_find_order on a keeping context: the call's new blocks are contiguous ranges of the device order
// (graph-major, rr ascending). Their transactions are gathered from the body store straight from the
// order's gids (device to device), encoded and hashed; 32 bytes per block come back.
hipError_t Engine::order_block_hashes(int64_t n_events, const int64_t* rr, const int32_t* ntx, const int32_t* nil,
                                      int64_t count, uint8_t* out32, bool* too_large) {
    *too_large = false;
    if (bodies_state != kBodiesComplete || count <= 0) return hipErrorInvalidValue;
    if (!ev_scratch) ev_scratch = new EvScratch();
    BodyPlan plan;
    HGX_TRY(bodies_measure(nullptr, nullptr, order_gid.p, n_events, plan));
    int64_t want = 0;
    for (int64_t b = 0; b < count; b++) want += ntx[b];
    if (plan.too_large || !block_text_fits(block_text_bound(count, plan.n_tx, plan.n_bytes))) {
        *too_large = true;
        return hipSuccess;
    }
    if (plan.n_tx != want) return hipErrorInvalidValue;   // (the store and the blocks disagree: a bug)
    const size_t o_by = up256(8 * ((size_t)plan.n_tx + 1));
    HGX_TRY(ev_scratch->blk_in.need(o_by + up256((size_t)plan.n_bytes + 16)));
    int64_t* d_off = (int64_t*)ev_scratch->blk_in.p;
    if (n_events > 0) HGX_TRY(bodies_copy(plan, nullptr, nullptr, nullptr, d_off, ev_scratch->blk_in.p + o_by));
    else HGX_TRY(hipMemsetAsync(d_off, 0, 8, stream));
    return block_hashes_run(stream, *ev_scratch, rr, ntx, nil, count, d_off, ev_scratch->blk_in.p + o_by, out32);
}

}  // namespace hgx

// ---- the encoder alone ----------------------------------------------------------------------
namespace {

void set_err(hgx_error* err, int32_t code, const char* msg) {
    if (!err) return;
    err->code = code;
    std::snprintf(err->msg, sizeof(err->msg), "%s", msg);
}

int32_t invalid(hgx_error* err, const char* msg) {
    set_err(err, HGX_ERR_INVALID, msg);
    return HGX_ERR_INVALID;
}

}  // namespace

extern "C" int32_t hgx_event_json_batch(int32_t device, const hgx_event_bodies* evb, int64_t count, const uint8_t* keys65,
                                        int32_t n_keys, const uint8_t* sp_id32, const uint8_t* op_id32, uint8_t* out,
                                        int64_t out_cap, int64_t* offsets, hgx_error* err) {
    set_err(err, HGX_OK, "");
    if (!evb || count < 0 || !offsets || n_keys < 0 || (count > 0 && (!keys65 || !sp_id32 || !op_id32)) ||
        (out && out_cap < 0))
        return invalid(err, "hgx_event_json_batch: bad arguments");
    const hgx::BodiesIn ev{evb->creator, evb->index, evb->self_parent, evb->other_parent, evb->timestamp_ns,
                           evb->sig_r, evb->sig_s, evb->ntx, evb->tx_off, evb->tx_bytes};
    std::vector<int64_t> txi;
    if (const char* why = hgx::bodies_check(ev, count, txi)) {
        char msg[128];
        std::snprintf(msg, sizeof(msg), "hgx_event_json_batch: %s", why);
        return invalid(err, msg);
    }
    for (int64_t k = 0; k < count; k++)
        if (ev.creator[k] < 0 || ev.creator[k] >= n_keys) return invalid(err, "hgx_event_json_batch: creator without a key");
    offsets[0] = 0;
    if (count == 0) return HGX_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_err(err, HGX_ERR_DEVICE, "no HIP device available (libhgx has no CPU fallback)");
        return HGX_ERR_DEVICE;
    }
    hipDeviceProp_t prop;
    if (device < 0 || device >= ndev || hipGetDeviceProperties(&prop, device) != hipSuccess ||
        std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_err(err, HGX_ERR_DEVICE, "libhgx is built for gfx950 (MI355X) only");
        return HGX_ERR_DEVICE;
    }
    int prev = 0;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(device);
    hipStream_t s = nullptr;
    hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    bool fits = true;
    {
        hgx::EvScratch sc;
        int64_t done = 0, at = 0;
        while (e == hipSuccess && done < count) {
            int64_t bound = 0;
            const int64_t hi = hgx::bodies_chunk_end(ev, txi, done, count, &bound);
            const int64_t m = hi - done;
            e = sc.stage(ev, txi, done, hi, nullptr, keys65, n_keys, sp_id32, op_id32, false, 0, 1, s);
            if (e == hipSuccess) e = sc.size_and_scan(m, 1, s);
            if (e == hipSuccess)
                e = hipMemcpyAsync(offsets + done + 1, sc.d_off + 1, 8 * (size_t)m, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) break;
            const int64_t bytes = offsets[hi];   // (chunk-relative until rebased below)
            for (int64_t k = done + 1; k <= hi; k++) offsets[k] += at;
            if (out && fits && at + bytes <= out_cap) {
                e = sc.write(m, (size_t)bytes, false, s);
                if (e == hipSuccess && bytes)
                    e = hipMemcpyAsync(out + at, sc.text.p, (size_t)bytes, hipMemcpyDeviceToHost, s);
                if (e == hipSuccess) e = hipStreamSynchronize(s);
            } else if (out) {
                fits = false;
            }
            at += bytes;
            done = hi;
        }
    }
    if (s) (void)hipStreamDestroy(s);
    (void)hipSetDevice(prev);
    if (e != hipSuccess) {
        set_err(err, HGX_ERR_DEVICE, hipGetErrorString(e));
        return HGX_ERR_DEVICE;
    }
    if (!fits) return invalid(err, "hgx_event_json_batch: out_cap is smaller than the batch's text");
    return HGX_OK;
}

extern "C" int32_t hgx_block_hash_batch(int32_t device, const int64_t* round_received, const int32_t* ntx,
                                        const int32_t* tx_nil, const int64_t* tx_off, const uint8_t* tx_bytes,
                                        int64_t count, uint8_t* out32, hgx_error* err) {
    set_err(err, HGX_OK, "");
    if (count < 0 || (count > 0 && (!round_received || !ntx || !tx_nil || !out32)))
        return invalid(err, "hgx_block_hash_batch: bad arguments");
    int64_t T = 0;
    for (int64_t b = 0; b < count; b++) {
        if (ntx[b] < 0) return invalid(err, "hgx_block_hash_batch: negative ntx");
        T += ntx[b];
    }
    if (T > 0 && !tx_off) return invalid(err, "hgx_block_hash_batch: null tx_off");
    for (int64_t j = 0; j < T; j++)
        if (tx_off[j + 1] < tx_off[j]) return invalid(err, "hgx_block_hash_batch: tx_off decreases");
    const int64_t nbytes = T > 0 ? tx_off[T] - tx_off[0] : 0;
    if (nbytes > 0 && !tx_bytes) return invalid(err, "hgx_block_hash_batch: null tx_bytes");
    int64_t text = 0;   // the encoder's positions are 32-bit: the batch's text, summed here in 64 bits
    for (int64_t b = 0, t = 0; b < count && hgx::block_text_fits(text); t += ntx[b], b++)
        text += hgx::block_text_len(round_received[b], ntx[b], tx_nil[b] != 0, tx_off ? tx_off + t : nullptr);
    if (!hgx::block_text_fits(text)) {
        set_err(err, HGX_ERR_CAPACITY, "hgx_block_hash_batch: the blocks' text reaches 4 GiB (hash fewer blocks per call)");
        return HGX_ERR_CAPACITY;
    }
    if (count == 0) return HGX_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_err(err, HGX_ERR_DEVICE, "no HIP device available (libhgx has no CPU fallback)");
        return HGX_ERR_DEVICE;
    }
    hipDeviceProp_t prop;
    if (device < 0 || device >= ndev || hipGetDeviceProperties(&prop, device) != hipSuccess ||
        std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_err(err, HGX_ERR_DEVICE, "libhgx is built for gfx950 (MI355X) only");
        return HGX_ERR_DEVICE;
    }
    int prev = 0;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(device);
    hipStream_t s = nullptr;
    hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    {
        hgx::EvScratch sc;
        const size_t o_by = hgx::up256(8 * ((size_t)T + 1));
        if (e == hipSuccess) e = sc.blk_in.need(o_by + hgx::up256((size_t)nbytes + 16));
        const int64_t zero = 0;
        if (e == hipSuccess)
            e = hipMemcpyAsync(sc.blk_in.p, T > 0 ? tx_off : &zero, 8 * ((size_t)T + 1), hipMemcpyHostToDevice, s);
        if (e == hipSuccess && nbytes > 0)
            e = hipMemcpyAsync(sc.blk_in.p + o_by, tx_bytes + (T > 0 ? tx_off[0] : 0), (size_t)nbytes, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        // (the offsets keep the caller's base: the bytes are addressed from it)
        if (e == hipSuccess)
            e = hgx::block_hashes_run(s, sc, round_received, ntx, tx_nil, count, (const int64_t*)sc.blk_in.p,
                                      sc.blk_in.p + o_by - (T > 0 ? tx_off[0] : 0), out32);
    }
    if (s) (void)hipStreamDestroy(s);
    (void)hipSetDevice(prev);
    if (e != hipSuccess) {
        set_err(err, HGX_ERR_DEVICE, hipGetErrorString(e));
        return HGX_ERR_DEVICE;
    }
    return HGX_OK;
}
