// The host column forms of an event batch (include/hgx.h: hgx_events, hgx_events32, hgx_events_packed)
// in one table: which columns a form has, how wide they are, which are structure (what validation and
// DivideRounds wait for) and which payload, and the order in which they cross PCIe.
// Host only, no HIP: the engine maps a column to its staging buffer, tools/ingest_cols_check.cpp
// checks the table on its own.
#pragma once

#include <cstddef>
#include <cstdint>

namespace hgx {

enum class Form : uint8_t { wide, compact, packed };

// A column, which is also its staging destination (Engine::stage_buf) and its InsertIn field
enum ColId : uint8_t {
    kColCreator, kColIndex, kColSp, kColOp, kColTs, kColHash, kColS, kColNtx, kColNil,   // hgx_events
    kColIndex32, kColSp32, kColOp32, kColCoin,                                           // hgx_events32
    kColCreator16, kColSpBack, kColOpBack, kColExcPos, kColExcSp, kColExcOp,             // hgx_events_packed
    kNumCols
};

// kColException: a structure column with one entry per exception, not per event. kColPayloadLate:
// copied behind the payload's other columns and straight into the event store, not the staging (S of
// the compact payload: only FindOrder's sort reads it)
enum ColKind : uint8_t { kColStructure, kColException, kColPayload, kColPayloadLate };

struct ColSpec {
    ColId id;
    uint8_t bytes;   // per event (per exception entry: kColException)
    ColKind kind;
};

constexpr int kMaxFormCols = 11;

struct FormSpec {
    int n;
    // the order of the copies of a split insert: the structure, then the payload
    ColSpec col[kMaxFormCols];
    // the order (indices into col) of a batch staged whole: the one-copy layout of a sync-sized batch,
    // and the payload's copies behind the structure's of a larger one
    uint8_t whole[kMaxFormCols];
};

inline const FormSpec& form_spec(Form f) {
    static const FormSpec wide = {9,
                                  {{kColCreator, 4, kColStructure}, {kColIndex, 8, kColStructure},
                                   {kColSp, 8, kColStructure}, {kColOp, 8, kColStructure},
                                   {kColTs, 8, kColPayload}, {kColHash, 32, kColPayload}, {kColS, 32, kColPayload},
                                   {kColNtx, 4, kColPayload}, {kColNil, 4, kColPayload}},
                                  {0, 1, 2, 3, 4, 5, 6, 7, 8}};
    static const FormSpec compact = {8,
                                     {{kColCreator, 4, kColStructure}, {kColIndex32, 4, kColStructure},
                                      {kColSp32, 4, kColStructure}, {kColOp32, 4, kColStructure},
                                      {kColTs, 8, kColPayload}, {kColCoin, 1, kColPayload}, {kColNtx, 4, kColPayload},
                                      {kColS, 32, kColPayloadLate}},
                                     {0, 1, 2, 3, 4, 5, 7, 6}};
    static const FormSpec packed = {11,
                                    {{kColCreator16, 2, kColStructure}, {kColIndex32, 4, kColStructure},
                                     {kColSpBack, 2, kColStructure}, {kColOpBack, 2, kColStructure},
                                     {kColExcPos, 8, kColException}, {kColExcSp, 4, kColException},
                                     {kColExcOp, 4, kColException},
                                     {kColTs, 8, kColPayload}, {kColCoin, 1, kColPayload}, {kColNtx, 4, kColPayload},
                                     {kColS, 32, kColPayloadLate}},
                                    {0, 1, 2, 3, 7, 8, 10, 9, 4, 5, 6}};
    return f == Form::wide ? wide : f == Form::compact ? compact : packed;
}

inline bool is_payload(const ColSpec& c) { return c.kind >= kColPayload; }

// One batch in host memory: the form and its columns' pointers by ColId (the others null).
// Trivially copyable: the copier threads take it by value.
struct HostCols {
    Form form;
    int64_t n_exc;   // packed: entries of the exception columns
    const void* col[kNumCols];
};

inline size_t col_bytes(const ColSpec& c, int64_t count, int64_t n_exc) {
    return (size_t)c.bytes * (size_t)(c.kind == kColException ? n_exc : count);
}

// bytes per event (per exception entry) of the columns of one kind
inline size_t form_bytes(Form f, ColKind kind) {
    const FormSpec& fs = form_spec(f);
    size_t b = 0;
    for (int i = 0; i < fs.n; i++)
        if (fs.col[i].kind == kind) b += fs.col[i].bytes;
    return b;
}

// The one-copy layout of a batch staged whole: off[i] = byte offset of col[i], the columns in `whole`
// order, each rounded up to 256 bytes. Returns the total.
inline size_t one_copy_layout(const FormSpec& fs, int64_t count, int64_t n_exc, size_t* off) {
    size_t total = 0;
    for (int k = 0; k < fs.n; k++) {
        const int i = fs.whole[k];
        off[i] = total;
        total += (col_bytes(fs.col[i], count, n_exc) + 255) & ~(size_t)255;
    }
    return total;
}

}  // namespace hgx
