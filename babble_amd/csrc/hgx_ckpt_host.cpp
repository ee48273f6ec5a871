// Version-3 checkpoint files: parser, validator and piece planner (hgx_ckpt_host.h). No HIP, no context.
#include "hgx_ckpt_host.h"

namespace hgx {

uint64_t ckpt_fnv1a(uint64_t h, const void* p, size_t n) {
    const uint8_t* b = (const uint8_t*)p;
    for (size_t i = 0; i < n; i++) {
        h ^= b[i];
        h *= kFnvPrime;
    }
    return h;
}

namespace {

// a cursor over the image's body (the closing checksum cut off): take() never passes the end
struct Cursor {
    const uint8_t* buf;
    size_t end, pos;
    // `count` elements of `width` bytes: their start, or null when they do not fit
    const uint8_t* take(int64_t count, size_t width) {
        if (count < 0) return nullptr;
        const size_t left = end - pos;
        if (width && (uint64_t)count > left / width) return nullptr;
        const uint8_t* p = buf + pos;
        pos += (size_t)count * width;
        return p;
    }
};

bool all_zero(const uint8_t* p, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (p[i]) return false;
    return true;
}

}  // namespace

const char* ckpt3_parse(const uint8_t* buf, size_t len, int32_t want_n, int32_t want_G, Ckpt3& f, std::string& why) {
    static const char kMagic[8] = {'H', 'G', 'X', 'C', 'K', 'P', 'T', '1'};
    auto bad = [&](const std::string& w) {
        why = w;
        return why.c_str();
    };
    f = Ckpt3();
    if (!buf || len < kCkptHeaderBytes + 8) return bad("truncated file");
    if (ckpt_fnv1a(kFnvBasis, buf, len - 8) != ckpt_rd<uint64_t>(buf + len - 8)) return bad("checksum mismatch");
    if (std::memcmp(buf, kMagic, 8) != 0) return bad("not a checkpoint file");
    const uint32_t version = ckpt_rd<uint32_t>(buf + 8);
    if (version != 3) return bad("unsupported version " + std::to_string(version));
    f.n = ckpt_rd<int32_t>(buf + 12);
    f.G = ckpt_rd<int32_t>(buf + 16);
    f.flags = ckpt_rd<int32_t>(buf + 20);
    f.E = ckpt_rd<int64_t>(buf + 24);
    const int32_t need = kCkIds | kCkKeys | kCkBodies;
    if ((f.flags & need) != need || (f.flags & ~(need | kCkRooted))) return bad("unsupported flags");
    if (f.n <= 0 || f.G <= 0 || (int64_t)f.n * f.G > (1 << 24)) return bad("bad participant counts");
    if ((want_n && f.n != want_n) || (want_G && f.G != want_G))
        return bad("file has " + std::to_string(f.G) + " x " + std::to_string(f.n) + " participants, the context " +
                   std::to_string(want_G) + " x " + std::to_string(want_n));
    f.C = (int64_t)f.n * f.G;
    Cursor c{buf, len - 8, kCkptHeaderBytes};
    if (f.E < 0 || (uint64_t)f.E > (c.end - c.pos) / 138) return bad("truncated file");   // (138 bytes per event at least)
    const int64_t C = f.C, E = f.E;
    if (f.flags & kCkRooted) {
        if (f.G != 1) return bad("roots need a single-graph context");
        f.root_index = c.take(C, 4);
        f.root_round = c.take(C, 4);
        f.root_y = c.take((C + 3) & ~(int64_t)3, 1);
        const uint8_t* no = c.take(1, 8);
        if (!f.root_index || !f.root_round || !f.root_y || !no) return bad("truncated file");
        if (!all_zero(f.root_y + C, (size_t)(((C + 3) & ~(int64_t)3) - C))) return bad("root padding is not zero");
        f.n_others = ckpt_rd<int64_t>(no);
        f.others = c.take(f.n_others, 32);
        if (!f.others) return bad("truncated file");
        f.kept.resize((size_t)f.G);
        for (Ckpt3Kept& k : f.kept) {
            const uint8_t *hdr = c.take(4, 4), *cnt = c.take(2, 8);
            if (!hdr || !cnt) return bad("truncated file");
            k.has_lcr = ckpt_rd<int32_t>(hdr, 0);
            k.lcr = ckpt_rd<int32_t>(hdr, 1);
            k.lcre = ckpt_rd<int32_t>(hdr, 2);
            k.consensus_tx = ckpt_rd<int64_t>(cnt, 0);
            k.n_blocks = ckpt_rd<int64_t>(cnt, 1);
            k.blocks = c.take(k.n_blocks, kCkptBlockBytes);
            if (!k.blocks) return bad("truncated file");
        }
        // the roots' ids and the Root.Others pairs
        f.has_x = c.take(C, 1);
        f.has_y = c.take(C, 1);
        const int64_t pad = ((2 * C + 3) & ~(int64_t)3) - 2 * C;
        const uint8_t* pz = c.take(pad, 1);
        f.x_id = c.take(C, 32);
        f.y_id = c.take(C, 32);
        const uint8_t* np = c.take(1, 8);
        if (!f.has_x || !f.has_y || !pz || !f.x_id || !f.y_id || !np) return bad("truncated file");
        if (!all_zero(pz, (size_t)pad)) return bad("root id padding is not zero");
        for (int64_t p = 0; p < C; p++) {
            if (f.has_x[p] > 1 || f.has_y[p] > 1) return bad("root id flags must be 0 or 1");
            if (f.has_y[p] != (f.root_y[p] ? 1 : 0))
                return bad("has_y[" + std::to_string(p) + "] disagrees with the root's root_y_is_event");
            if ((!f.has_x[p] && !all_zero(f.x_id + 32 * p, 32)) || (!f.has_y[p] && !all_zero(f.y_id + 32 * p, 32)))
                return bad("a root id without its flag is not zero");
        }
        f.n_pairs = ckpt_rd<int64_t>(np);
        f.pair_event = c.take(f.n_pairs, 32);
        f.pair_parent = c.take(f.n_pairs, 32);
        if (!f.pair_event || !f.pair_parent) return bad("truncated file");
        if (f.n_pairs != f.n_others || std::memcmp(f.pair_event, f.others, (size_t)f.n_others * 32) != 0)
            return bad("root pairs and Root.Others keys disagree");
        for (int64_t j = 1; j < f.n_pairs; j++)
            if (std::memcmp(f.pair_event + 32 * (j - 1), f.pair_event + 32 * j, 32) >= 0)
                return bad("root pairs are not sorted by event id");
        for (Ckpt3Kept& k : f.kept) {
            k.hashes = c.take(k.n_blocks, kCkptBlockHashBytes);
            if (!k.hashes) return bad("truncated file");
            for (int64_t b = 0; b < k.n_blocks; b++) {
                const uint8_t* h = k.hashes + kCkptBlockHashBytes * b;
                if (h[0] > 1 || h[1] || h[2] || h[3] || (!h[0] && !all_zero(h + 4, 32))) return bad("bad block hash record");
            }
        }
    }
    f.creator = c.take(E, 4);
    f.index = c.take(E, 8);
    f.sp = c.take(E, 8);
    f.op = c.take(E, 8);
    f.ts = c.take(E, 8);
    f.sig_s = c.take(E, 32);
    f.coin = c.take(E, 1);
    f.ntx = c.take(E, 4);
    f.nil = c.take(E, 1);
    f.ids = c.take(E, 32);
    f.keys = c.take(C, 65);
    f.sig_r = c.take(E, 32);
    const uint8_t* nt = c.take(1, 8);
    if (!f.creator || !f.index || !f.sp || !f.op || !f.ts || !f.sig_s || !f.coin || !f.ntx || !f.nil || !f.ids ||
        !f.keys || !f.sig_r || !nt)
        return bad("truncated file");
    int64_t sum = 0;
    for (int64_t i = 0; i < E; i++) {
        const int32_t x = ckpt_rd<int32_t>(f.ntx, i);
        if (x < 0) return bad("negative ntx at event " + std::to_string(i));
        if (f.nil[i] > 1 || (f.nil[i] && x)) return bad("tx_nil and ntx disagree at event " + std::to_string(i));
        if ((f.ids[32 * i + 16] != 0) != (f.coin[i] != 0)) return bad("event id and coin disagree at event " + std::to_string(i));
        sum += x;
    }
    f.T = ckpt_rd<int64_t>(nt);
    if (f.T != sum) return bad("T is not the sum of ntx");
    f.tx_off = c.take(f.T + 1, 8);
    if (!f.tx_off) return bad("truncated file");
    if (ckpt_rd<int64_t>(f.tx_off, 0) != 0) return bad("tx_off must start at 0");
    for (int64_t t = 0; t < f.T; t++)
        if (ckpt_rd<int64_t>(f.tx_off, t + 1) < ckpt_rd<int64_t>(f.tx_off, t)) return bad("tx_off decreases");
    f.n_bytes = ckpt_rd<int64_t>(f.tx_off, f.T);
    f.tx_bytes = c.take(f.n_bytes, 1);
    if (!f.tx_bytes) return bad("truncated file");
    if (c.pos != c.end) return bad("size mismatch");
    return nullptr;
}

void ckpt3_piece(const Ckpt3& f, int64_t lo, int64_t t_lo, int64_t max_events, int64_t max_bytes, int64_t* hi,
                 int64_t* t_hi) {
    int64_t k = lo, t = t_lo;
    if (lo < 0 || lo >= f.E || t_lo < 0 || t_lo > f.T) {   // (nothing to read)
        *hi = lo;
        *t_hi = t_lo;
        return;
    }
    const int64_t b0 = ckpt_rd<int64_t>(f.tx_off, t_lo);
    while (k < f.E && k - lo < max_events) {
        const int64_t t1 = t + ckpt_rd<int32_t>(f.ntx, k);
        if (t1 > f.T) break;   // (a validated image never gets here)
        if (k > lo && ckpt_rd<int64_t>(f.tx_off, t1) - b0 > max_bytes) break;
        t = t1;
        k++;
    }
    *hi = k;
    *t_hi = t;
}

int64_t ckpt3_find_pair(const Ckpt3& f, const uint8_t* id32) {
    int64_t lo = 0, hi = f.n_pairs;
    while (lo < hi) {   // first event id >= id32
        const int64_t mid = (lo + hi) >> 1;
        if (std::memcmp(f.pair_event + 32 * mid, id32, 32) < 0) lo = mid + 1; else hi = mid;
    }
    return lo < f.n_pairs && std::memcmp(f.pair_event + 32 * lo, id32, 32) == 0 ? lo : -1;
}

}  // namespace hgx
