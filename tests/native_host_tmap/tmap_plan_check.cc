// tmap_plan_check.cc -- CPU check of the host typemap steps' DMA plans (lampi_amd/csrc/host_tmap_plan.h), no GPU.
//
// For a list of typemaps, windows, fragment lengths and chunk caps the plans are made exactly as host_tmap.cc makes
// them and every planned transfer is executed with memcpy between a host arena and a stand-in of the packed device
// chunk.  The yardstick is the header's address rule, applied byte by byte to the caller's own pairs.
//   send, pieces route: every byte read is a piece byte of the window, read once; the chunk ends up as the packed
//         window; no transfer leaves the chunk's announced size; a 2D transfer has pitches >= its width.
//   send, span route:   the one transfer stays inside the announced staging size and reads only piece bytes of the
//         window's elements and gaps under kTmapSpanGap bounded by such bytes on both sides (so only pages a piece
//         touches, at any page alignment); the gather by the merged pairs the device is given yields the packed
//         window.
//   receive: runs of passed fragments (some dropped at the start, middle and end) go down by the pieces route; the
//         arena ends up as its before-image plus exactly the passed fragments' pieces, every written byte written
//         once.
// Prints one line per case and "bad N done"; exits 1 on any failure.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../lampi_amd/csrc/host_tmap_plan.h"

using namespace lampi;

static int g_bad = 0;
static void report(const std::string &what, bool ok) {
    std::printf("%s %s\n", what.c_str(), ok ? "ok" : "BAD");
    if (!ok) ++g_bad;
}

struct Type {
    std::string name;
    std::vector<lampi_tmap_elt> pairs;
    int64_t extent;
    bool recv;  // elements do not overlap: deliveries are defined
    uint64_t ps() const {
        uint64_t s = 0;
        for (auto &p : pairs) s += p.size;
        return s;
    }
};

static Type make(const std::string &name, std::vector<uint64_t> sizes, std::vector<int64_t> offs, int64_t extent,
                 bool recv = true) {
    Type t{name, {}, extent, recv};
    int64_t seq = 0;
    for (size_t i = 0; i < sizes.size(); ++i) {
        t.pairs.push_back(lampi_tmap_elt{sizes[i], offs[i], seq});
        seq += (int64_t)sizes[i];
    }
    return t;
}

static Type scattered(const std::string &name, size_t n, uint64_t seed) {
    std::mt19937_64 rng(seed);
    std::vector<uint64_t> sizes(n);
    std::vector<int64_t> offs(n);
    std::vector<size_t> perm(n);
    for (size_t i = 0; i < n; ++i) sizes[i] = 1 + rng() % 40, perm[i] = i;
    std::shuffle(perm.begin(), perm.end(), rng);
    int64_t cur = 0;
    for (size_t j : perm) {
        offs[j] = cur + (int64_t)(rng() % 8);
        cur = offs[j] + (int64_t)sizes[j];
    }
    return make(name, sizes, offs, cur + 5);
}

// the address rule: host offset (from the origin) of packed byte p
static int64_t addr_of(const Type &t, uint64_t p) {
    const uint64_t ps = t.ps(), e = p / ps, r = p % ps;
    size_t i = 0;
    while (i + 1 < t.pairs.size() && (uint64_t)t.pairs[i + 1].seq_offset <= r) ++i;
    return (int64_t)e * t.extent + t.pairs[i].offset + (int64_t)(r - (uint64_t)t.pairs[i].seq_offset);
}

struct Arena {
    std::vector<uint8_t> bytes;
    int64_t origin;
};

static Arena arena_for(const Type &t, uint64_t count) {
    int64_t lo = 0, hi = 0;
    for (uint64_t e : {(uint64_t)0, count - 1})
        for (auto &p : t.pairs) {
            lo = std::min(lo, (int64_t)e * t.extent + p.offset);
            hi = std::max(hi, (int64_t)e * t.extent + p.offset + (int64_t)p.size);
        }
    Arena a;
    a.origin = 32 - lo;
    a.bytes.resize((size_t)(a.origin + hi + 32));
    for (size_t i = 0; i < a.bytes.size(); ++i) a.bytes[i] = (uint8_t)(i * 131 + (i >> 8) * 7 + 1);
    return a;
}

static lampi_host_tmap host_tmap_of(const Type &t, uint64_t count) {
    return lampi_host_tmap{t.pairs.data(), (uint64_t)t.extent, t.ps(), count, (uint32_t)t.pairs.size(), 0};
}

// Executes the pieces route between the arena and a chunk; to_host: chunk -> arena.  touched[i]: times arena byte i
// was read / written.  False when a transfer is malformed or leaves the arena or the chunk.
static bool run_pieces(const std::vector<TmapXfer> &xf, Arena &a, std::vector<uint8_t> &chunk, bool to_host,
                       std::vector<uint32_t> &touched) {
    for (const TmapXfer &x : xf) {
        if (x.width == 0 || x.rows == 0) return false;
        if (x.rows > 1 && (x.hpitch < x.width || x.dpitch < x.width || (int64_t)x.hpitch <= 0)) return false;
        for (uint64_t r = 0; r < x.rows; ++r) {
            const int64_t h = a.origin + (int64_t)(x.hoff + r * x.hpitch);
            const uint64_t d = x.doff + r * x.dpitch;
            if (h < 0 || (uint64_t)h + x.width > a.bytes.size() || d + x.width > chunk.size()) return false;
            if (to_host) std::memcpy(&a.bytes[(size_t)h], &chunk[d], x.width);
            else std::memcpy(&chunk[d], &a.bytes[(size_t)h], x.width);
            for (uint64_t k = 0; k < x.width; ++k) ++touched[(size_t)h + k];
        }
    }
    return true;
}

// The send step's staging of the window [w0, w0 + wlen) in chunks of fpc fragments, as host_tmap.cc does it.
static void check_send(const Type &t, uint64_t count, uint64_t w0, uint64_t wlen, uint64_t frag_len, uint64_t cap,
                       int want_route /* -1 any, 0 pieces, 1 span, 2: the pieces route alone */, const std::string &tag) {
    Arena a = arena_for(t, count);
    const lampi_host_tmap ht = host_tmap_of(t, count);
    bool ok = tmap_consistent(ht);
    const TmapPlan plan(ht);
    const uint64_t fpc = std::max<uint64_t>(1, cap / frag_len), cb = fpc * frag_len;
    const uint64_t span_cap = want_route == 2 ? 0 : std::min(plan.span_need(cb), plan.span_need(wlen));
    const uint64_t nfr = wlen ? (wlen - 1) / frag_len + 1 : 1;
    size_t nspan = 0, npieces = 0;
    Type merged = t;
    merged.pairs = plan.merged();
    for (uint64_t f0 = 0; f0 < nfr && ok; f0 += fpc) {
        const uint64_t p0 = w0 + f0 * frag_len, p1 = std::min(w0 + wlen, p0 + cb);
        if (p1 <= p0) break;
        std::vector<uint8_t> chunk(cb, 0xEE);  // the announced chunk size
        std::vector<uint32_t> touched(a.bytes.size(), 0), piece(a.bytes.size(), 0);
        for (uint64_t p = p0; p < p1; ++p) ++piece[(size_t)(a.origin + addr_of(t, p))];
        TmapSpan sp;
        if (plan.span(p0, p1, span_cap, sp)) {
            ++nspan;
            std::vector<uint8_t> stage(span_cap, 0xDD);  // the announced staging size
            const int64_t h = a.origin + (int64_t)sp.lo;
            if (sp.bytes > span_cap || h < 0 || (uint64_t)h + sp.bytes > a.bytes.size()) {
                ok = false;
                break;
            }
            std::memcpy(stage.data(), &a.bytes[(size_t)h], sp.bytes);
            // what may be read: piece bytes of the window's ELEMENTS, and short gaps between them
            std::vector<uint8_t> el(a.bytes.size(), 0);
            for (uint64_t p = p0 / t.ps() * t.ps(); p < ((p1 - 1) / t.ps() + 1) * t.ps(); ++p)
                el[(size_t)(a.origin + addr_of(t, p))] = 1;
            uint64_t gap = 0;
            ok = ok && el[(size_t)h] && el[(size_t)h + sp.bytes - 1];
            for (uint64_t k = 0; k < sp.bytes && ok; ++k) {
                gap = el[(size_t)h + k] ? 0 : gap + 1;
                if (gap >= kTmapSpanGap) ok = false;
            }
            // the gather the device runs: the address rule over the merged pairs, from the staging area
            for (uint64_t p = p0; p < p1 && ok; ++p) {
                const uint64_t s = (uint64_t)addr_of(merged, p) - sp.lo;
                if (s >= sp.bytes) ok = false;
                else chunk[p - p0] = stage[s];
            }
        } else {
            ++npieces;
            std::vector<TmapXfer> xf;
            plan.pieces(p0, p1, 0, xf);
            ok = ok && run_pieces(xf, a, chunk, false, touched);
            ok = ok && touched == piece;  // exactly the pieces' bytes, each as often as the window holds it
        }
        for (uint64_t p = p0; p < p1 && ok; ++p)
            if (chunk[p - p0] != a.bytes[(size_t)(a.origin + addr_of(t, p))]) ok = false;
    }
    if ((want_route == 0 || want_route == 2) && nspan) ok = false;
    if (want_route == 1 && (!nspan || npieces)) ok = false;
    report("send " + t.name + " " + tag + " span=" + std::to_string(nspan) + " pieces=" + std::to_string(npieces), ok);
}

// The receive step's deliveries: the window's fragments, some dropped, the runs of the others cut at `cap` bytes.
static void check_recv(const Type &t, uint64_t count, uint64_t w0, uint64_t wlen, uint64_t frag_len, uint64_t cap,
                       const std::string &tag) {
    Arena a = arena_for(t, count);
    const lampi_host_tmap ht = host_tmap_of(t, count);
    const TmapPlan plan(ht);
    const uint64_t nfr = wlen ? (wlen - 1) / frag_len + 1 : 1;
    std::vector<uint8_t> drop(nfr, 0);
    // dropped: the first fragment, one in the middle of a run, two neighbours, the last
    for (uint64_t j : {(uint64_t)0, nfr / 3, nfr / 2, nfr / 2 + 1, nfr - 1})
        if (nfr > 6) drop[j] = 1;
    std::vector<uint8_t> packed(wlen), want = a.bytes;
    std::vector<uint32_t> touched(a.bytes.size(), 0), expect(a.bytes.size(), 0);
    for (uint64_t i = 0; i < wlen; ++i) packed[i] = (uint8_t)(i * 29 + 3);
    bool ok = true;
    uint64_t run0 = 0, run1 = 0;  // the open run, fragments [run0, run1)
    auto flush = [&]() {
        if (run1 > run0) {
            const uint64_t p0 = w0 + run0 * frag_len, p1 = std::min(w0 + wlen, w0 + run1 * frag_len);
            const uint64_t doff = 256 + run0 % 7;  // anywhere in the output chunk
            std::vector<uint8_t> chunk(doff + (p1 - p0), 0xEE);
            std::memcpy(&chunk[doff], &packed[p0 - w0], p1 - p0);
            std::vector<TmapXfer> xf;
            plan.pieces(p0, p1, doff, xf);
            ok = ok && run_pieces(xf, a, chunk, true, touched);
            for (uint64_t p = p0; p < p1; ++p) {
                const size_t h = (size_t)(a.origin + addr_of(t, p));
                want[h] = packed[p - w0];
                ++expect[h];
            }
        }
        run0 = run1;
    };
    for (uint64_t j = 0; j < nfr; ++j) {
        if (drop[j]) {
            flush();
            run0 = run1 = j + 1;
            continue;
        }
        if ((run1 - run0 + 1) * frag_len > cap && run1 > run0) flush();
        run1 = j + 1;
    }
    flush();
    ok = ok && touched == expect && a.bytes == want;
    report("recv " + t.name + " " + tag, ok);
}

// 65 pieces of 64 bytes two bytes apart -- the last one behind a gap of gap_in bytes --, the next element's first
// piece gap_between bytes behind the last: about 130 host bytes per DMA row, two per packed byte
static Type gap_type(const std::string &name, uint64_t gap_in, uint64_t gap_between) {
    std::vector<uint64_t> sizes(65, 64);
    std::vector<int64_t> offs(65);
    for (int j = 0; j < 64; ++j) offs[j] = 66 * j;
    offs[64] = 66 * 63 + 64 + (int64_t)gap_in;
    return make(name, sizes, offs, offs[64] + 64 + (int64_t)gap_between);
}

int main() {
    const uint64_t G = kTmapSpanGap, R = kTmapSpanRatio, RB = kTmapSpanRowBytes;
    std::vector<Type> types = {
        make("T1", {8}, {3}, 24),
        make("T2", {1, 13, 51}, {70, -16, 0}, 128),
        make("T3", {5000, 3001}, {5, 6001}, 12288),
        make("T5", {48}, {0}, 48),
        make("S1", {1}, {0}, 3),
        [] {
            std::vector<uint64_t> s(65, 1);
            std::vector<int64_t> o(65);
            for (int j = 0; j < 65; ++j) o[j] = 2 * (64 - j);
            return make("S65", s, o, 131);
        }(),
        scattered("T4a", 64, 41),
        make("touching", {8, 4, 12}, {0, 8, 12}, 40),  // merged into one piece
        make("extent0", {8}, {0}, 0, false),
        make("extent<size", {16}, {0}, 8, false),
        make("negative", {8, 3}, {0, 9}, -24),
    };
    const uint64_t frag_lens[] = {52, 100, 1976, 4200};
    const uint64_t caps[] = {4096, 65536, 32u << 20};
    const int lasts[] = {1, 15, 17, 0};
    int k = 0;
    for (const Type &t : types) {
        const uint64_t ps = t.ps();
        uint64_t big = 0;  // 7 bytes into the first pair of at least 8 bytes, in element 1
        for (auto &p : t.pairs)
            if (p.size >= 8) {
                big = (uint64_t)p.seq_offset + 7;
                break;
            }
        const uint64_t offs[] = {0, ps + big, 2 * ps};
        for (uint64_t w0 : offs)
            for (int last : lasts) {
                const uint64_t L = frag_lens[k % 4], cap = caps[k % 3];
                ++k;
                const uint64_t nf = 23, wlen = last ? (nf - 1) * L + (uint64_t)last : nf * L;
                const uint64_t count = (w0 + wlen + ps - 1) / ps + 1;
                const std::string tag = "off=" + std::to_string(w0) + " L=" + std::to_string(L) + " last=" +
                                        std::to_string(last) + " cap=" + std::to_string(cap);
                check_send(t, count, w0, wlen, L, cap, -1, tag);
                check_send(t, count, w0, wlen, L, cap, 2, tag + " (pieces alone)");
                if (t.recv) check_recv(t, count, w0, wlen, L, cap, tag);
            }
        check_send(t, 3, ps, 0, 100, 4096, -1, "empty window");
    }
    // every cap with one type, both directions
    for (uint64_t cap : {(uint64_t)4096, (uint64_t)8192, (uint64_t)65536, (uint64_t)1 << 20, (uint64_t)32 << 20}) {
        const Type &t = types[1];
        check_send(t, 2000, 7, 100000, 1976, cap, -1, "cap=" + std::to_string(cap));
        check_recv(t, 2000, 7, 100000, 1976, cap, "cap=" + std::to_string(cap));
    }
    // one type either side of each span rule, built from the header's constants; windows of whole elements
    struct Rule {
        Type t;
        int route;
    };
    const std::vector<Rule> rules = {
        {gap_type("gap-in-footprint<G", G - 1, 3), 1},
        {gap_type("gap-in-footprint=G", G, 3), 0},
        {gap_type("gap-between<G", 2, G - 1), 1},
        {gap_type("gap-between=G", 2, G), 0},
        {make("rowbytes=RB", {8}, {0}, (int64_t)RB), 1},
        {make("rowbytes>RB", {8}, {0}, (int64_t)RB + 1), 0},
        {make("ratio=R", {1, 1, 1, 1}, {0, 2, 4, 6}, (int64_t)(4 * R)), 1},
        {make("ratio>R", {1, 1, 1, 1}, {0, 2, 4, 6}, (int64_t)(4 * R + 4)), 0},
    };
    for (const Rule &r : rules) {
        const uint64_t ps = r.t.ps(), n = 64;
        check_send(r.t, n + 2, ps, n * ps, ps * 4, 32u << 20, r.route, "rule, one chunk");
        check_recv(r.t, n + 2, ps, n * ps, ps * 4, 32u << 20, "rule");
    }
    // T1 over whole elements is one 2D transfer per chunk, T2 three; touching pairs one
    for (auto &c : {std::make_pair(0, 1), std::make_pair(1, 3), std::make_pair(7, 1)}) {
        const Type &t = types[(size_t)c.first];
        const lampi_host_tmap ht = host_tmap_of(t, 100);
        std::vector<TmapXfer> xf;
        TmapPlan(ht).pieces(2 * t.ps(), 50 * t.ps(), 0, xf);
        bool ok = xf.size() == (size_t)c.second;
        for (auto &x : xf) ok = ok && x.rows == 48 && x.hpitch == (uint64_t)t.extent && x.dpitch == t.ps();
        report("whole elements of " + t.name + ": " + std::to_string(xf.size()) + " 2D transfers", ok);
    }
    // inconsistent typemaps
    {
        Type t = types[1];
        auto bad = [&](const char *what, void (*f)(Type &)) {
            Type u = t;
            f(u);
            lampi_host_tmap ht = host_tmap_of(u, 4);
            ht.packed_size = t.ps();
            report(std::string("inconsistent: ") + what, !tmap_consistent(ht));
        };
        bad("seq_offset[0] != 0", [](Type &u) { u.pairs[0].seq_offset = 1; });
        bad("seq_offset[2] off by one", [](Type &u) { u.pairs[2].seq_offset += 1; });
        bad("a size of 0", [](Type &u) { u.pairs[1].size = 0; });
        bad("sizes short of packed_size", [](Type &u) { u.pairs.pop_back(); });
        bad("sizes past packed_size", [](Type &u) { u.pairs[2].size += 1; });
        report("consistent", tmap_consistent(host_tmap_of(t, 4)));
    }
    std::printf("bad %d done\n", g_bad);
    return g_bad ? 1 : 0;
}
