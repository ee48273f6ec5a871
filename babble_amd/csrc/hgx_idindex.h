// The event-id index (hgx_keep_id_index): an open-addressing table over the id column
// g_id, so that Store.GetEvent(hash) and Body.Parents are answered where the ids already are.
//
// Table: `slots` = the smallest power of two >= 2 x the context's capacity (load <= 0.5), one 8-byte word
// per slot. 0 = empty, else (tag << 32) | (value + 1), value = the event's gid (the resident table) or its
// batch position (the scratch table of hgx_insert_events_by_id). Contract:
//   home slot = id bytes 0..7 as a little-endian u64, masked with slots - 1;
//   tag       = id bytes 8..11 as a little-endian u32;
//   linear probing by +1 with wrap-around.
// A match needs the tag AND all 32 bytes of the value's id row; the tag only saves the row read.
// Memory: 8 bytes per slot = 16 bytes per event of capacity at an exact power of two, just under 32 at
// the worst rounding: 256 MiB at a capacity of 10 M events (2^25 slots).
//
// For linear probing the set of occupied slots, and so the sum of displacements and the number of
// entries stored below their home slot, depend on the set of keys alone, not on the order of the
// inserts: the concurrent device inserts and this header's sequential model agree on them
// (tools/id_index_check.cpp, tests/idindexref.py).
//
// The functions below are the contract itself, shared by the kernels (hgx_idindex.hip) and the host
// check. Every probe loop is bounded by `slots`.
#pragma once

#include <cstdint>
#include <cstring>

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define HGX_IDX_HD __host__ __device__
#else
#define HGX_IDX_HD
#endif

namespace hgx {

constexpr int64_t kIdxNone = -1;      // no row matches
constexpr int64_t kIdxCorrupt = -2;   // a probe met no empty slot within `slots` steps
constexpr int64_t kIdxMaxCapacity = (int64_t)1 << 31;   // value + 1 fits the word's low half

// the sizing rule: the smallest power of two >= 2 x capacity (capacity >= 1)
HGX_IDX_HD inline uint64_t idx_slots_for(int64_t capacity) {
    uint64_t s = 2;
    while (s < 2 * (uint64_t)capacity) s <<= 1;
    return s;
}

HGX_IDX_HD inline uint64_t idx_home(const uint8_t* id, uint64_t slots) {
    uint64_t h = 0;
    for (int b = 7; b >= 0; b--) h = (h << 8) | id[b];
    return h & (slots - 1);
}

HGX_IDX_HD inline uint32_t idx_tag(const uint8_t* id) {
    return (uint32_t)id[8] | ((uint32_t)id[9] << 8) | ((uint32_t)id[10] << 16) | ((uint32_t)id[11] << 24);
}

HGX_IDX_HD inline uint64_t idx_word(uint32_t tag, int64_t value) { return ((uint64_t)tag << 32) | (uint32_t)(value + 1); }
HGX_IDX_HD inline uint32_t idx_word_tag(uint64_t w) { return (uint32_t)(w >> 32); }
HGX_IDX_HD inline int64_t idx_word_value(uint64_t w) { return (int64_t)(uint32_t)w - 1; }

HGX_IDX_HD inline uint64_t idx_displacement(uint64_t slot, uint64_t home, uint64_t slots) {
    return (slot - home) & (slots - 1);
}

HGX_IDX_HD inline bool idx_row_eq(const uint8_t* a, const uint8_t* b) {
#if defined(__HIP_DEVICE_COMPILE__)
    // (device rows are 32-byte rows of 256-byte aligned buffers)
    const uint4 a0 = ((const uint4*)a)[0], a1 = ((const uint4*)a)[1], b0 = ((const uint4*)b)[0], b1 = ((const uint4*)b)[1];
    return a0.x == b0.x && a0.y == b0.y && a0.z == b0.z && a0.w == b0.w && a1.x == b1.x && a1.y == b1.y &&
           a1.z == b1.z && a1.w == b1.w;
#else
    return std::memcmp(a, b, 32) == 0;
#endif
}

// The lookup: from the home slot to the first empty one, the LOWEST value below `limit` whose tag and
// whole row (rows + 32 x value) equal `id`. Two entries can share an id (the wide insert takes hashes
// on trust; a batch may repeat a claimed id), so the scan does not stop at the first match.
// kIdxNone: no match; kIdxCorrupt: no empty slot within `slots` steps, or a value at or beyond `rows_n`.
HGX_IDX_HD inline int64_t idx_probe(const uint64_t* tab, uint64_t slots, const uint8_t* rows, int64_t rows_n,
                                    const uint8_t* id, int64_t limit) {
    const uint32_t tag = idx_tag(id);
    uint64_t s = idx_home(id, slots);
    int64_t best = kIdxNone;
    for (uint64_t i = 0; i < slots; i++, s = (s + 1) & (slots - 1)) {
        const uint64_t w = tab[s];
        if (w == 0) return best;
        if (idx_word_tag(w) != tag) continue;
        const int64_t v = idx_word_value(w);
        if (v < 0 || v >= rows_n) return kIdxCorrupt;
        if (v < limit && (best < 0 || v < best) && idx_row_eq(rows + 32 * v, id)) best = v;
    }
    return kIdxCorrupt;
}

// The sequential model of an insert (the host check; the device claims the slot with a 64-bit
// atomicCAS instead): false = no empty slot within `slots` steps.
inline bool idx_model_insert(uint64_t* tab, uint64_t slots, const uint8_t* id, int64_t value) {
    uint64_t s = idx_home(id, slots);
    for (uint64_t i = 0; i < slots; i++, s = (s + 1) & (slots - 1))
        if (tab[s] == 0) {
            tab[s] = idx_word(idx_tag(id), value);
            return true;
        }
    return false;
}

// hgx_id_index_state's reduction over one slot: false = the slot's value names no row
struct IdxStats {
    uint64_t entries = 0, displacement = 0, wrapped = 0;
};
HGX_IDX_HD inline bool idx_slot_stats(const uint64_t* tab, uint64_t slots, const uint8_t* rows, int64_t rows_n, uint64_t s,
                                      uint64_t* disp, uint64_t* wrapped) {
    const int64_t v = idx_word_value(tab[s]);
    if (v < 0 || v >= rows_n) return false;
    const uint64_t home = idx_home(rows + 32 * v, slots);
    *disp = idx_displacement(s, home, slots);
    *wrapped = s < home ? 1 : 0;
    return true;
}

}  // namespace hgx
