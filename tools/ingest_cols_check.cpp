// Stand-alone check of the host column table (babble_amd/csrc/hgx_ingest_cols.h): no HIP, no context.
// Prints, for every form, the bytes per event of each kind, the columns in the order of a split
// insert and of a batch staged whole, the late payload columns, and the one-copy layout for a few
// batch sizes (tests/test_ingest_cols_host.py compares them with the documented figures). The layout
// is also exercised: every column's bytes are written into a buffer of exactly the layout's size and
// read back, so a sanitizer build (-fsanitize=address,undefined) sees an overlap or an overrun.
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

#include "hgx_ingest_cols.h"

using namespace hgx;

static_assert(std::is_trivially_copyable<HostCols>::value, "the copier threads take HostCols by value");

static const char* const kColName[kNumCols] = {"creator", "index", "sp", "op", "ts", "hash", "S", "ntx", "nil",
                                               "index32", "sp32", "op32", "coin", "creator16", "sp_back", "op_back",
                                               "exc_pos", "exc_sp", "exc_op"};
static const char* const kKindName[] = {"structure", "exception", "payload", "late"};
static const char* const kFormName[] = {"wide", "compact", "packed"};

static int fail(const char* what, const char* form) {
    std::printf("FAILED %s (%s)\n", what, form);
    return 1;
}

int main() {
    for (Form f : {Form::wide, Form::compact, Form::packed}) {
        const char* fn = kFormName[(int)f];
        const FormSpec& fs = form_spec(f);
        if (fs.n < 1 || fs.n > kMaxFormCols) return fail("column count", fn);
        std::printf("bytes %s structure %zu exception %zu payload %zu\n", fn, form_bytes(f, kColStructure),
                    form_bytes(f, kColException), form_bytes(f, kColPayload) + form_bytes(f, kColPayloadLate));
        std::printf("split %s", fn);
        bool seen[kNumCols] = {}, payload = false;
        for (int i = 0; i < fs.n; i++) {
            const ColSpec& c = fs.col[i];
            if (c.id >= kNumCols || seen[c.id]) return fail("a column twice", fn);
            if (payload && !is_payload(c)) return fail("structure behind payload", fn);
            seen[c.id] = true;
            payload = is_payload(c);
            std::printf(" %s:%d:%s", kColName[c.id], (int)c.bytes, kKindName[c.kind]);
        }
        std::printf("\nwhole %s", fn);
        bool used[kMaxFormCols] = {};
        for (int k = 0; k < fs.n; k++) {
            if (fs.whole[k] >= fs.n || used[fs.whole[k]]) return fail("whole is no permutation", fn);
            used[fs.whole[k]] = true;
            std::printf(" %s", kColName[fs.col[fs.whole[k]].id]);
        }
        std::printf("\nlate %s", fn);
        for (int i = 0; i < fs.n; i++)
            if (fs.col[i].kind == kColPayloadLate) std::printf(" %s", kColName[fs.col[i].id]);
        std::printf("\n");
        for (int64_t count : {(int64_t)1, (int64_t)1000, (int64_t)65536})
            for (int64_t n_exc : {(int64_t)0, (int64_t)3}) {
                if (n_exc && f != Form::packed) continue;
                size_t off[kMaxFormCols];
                const size_t total = one_copy_layout(fs, count, n_exc, off);
                std::printf("layout %s %lld %lld %zu", fn, (long long)count, (long long)n_exc, total);
                std::vector<unsigned char> buf(total, 0xFF);
                for (int i = 0; i < fs.n; i++) {
                    const size_t b = col_bytes(fs.col[i], count, n_exc);
                    std::printf(" %s:%zu:%zu", kColName[fs.col[i].id], off[i], b);
                    if (off[i] + b > total) return fail("a column ends past the layout", fn);
                    if (b) std::memset(buf.data() + off[i], i, b);
                }
                std::printf("\n");
                for (int i = 0; i < fs.n; i++) {
                    const size_t b = col_bytes(fs.col[i], count, n_exc);
                    for (size_t x = 0; x < b; x++)
                        if (buf[off[i] + x] != (unsigned char)i) return fail("columns overlap", fn);
                }
            }
    }
    std::printf("ok\n");
    return 0;
}
