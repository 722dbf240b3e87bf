// unpack_plan_check.cc -- CPU check of the host receive step's DMA plan (lampi_amd/csrc/host_pack_items.h on
// lampi_amd/csrc/host_plan.h), no GPU.
//
// Random batches of lampi_host_recv_slot records -- GM / IB / Quadrics headers, slots with the payload behind the
// header, headers apart, Quadrics inline payloads, fragments with nothing to deliver, ring order and shuffled -- are planned chunk by chunk exactly as lampi_host_recv_unpack_batch plans them, and the plan
// is executed on the CPU: every H2D transfer a memcpy into a stand-in of the input chunk of the size the planner
// announced, every fragment's lengthToCopy bytes moved from where the library will tell the kernel to read them
// to the fragment's place in the output chunk, every D2H transfer a memcpy into the application arena.
// Checked: no transfer leaves the ring or the announced chunk sizes; each header and each payload arrives where
// the descriptors will point; the application arena ends up with exactly the deliveries; a batch larger than the
// chunk size is cut into chunks, each starting at a fragment's first item.
// Prints "bad N done"; exits 1 on any failure.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../lampi_amd/csrc/host_pack_items.h"

using namespace lampi;

static int g_bad = 0;
static void report(const std::string &what, bool ok) {
    std::printf("%s %s\n", what.c_str(), ok ? "ok" : "BAD");
    if (!ok) ++g_bad;
}

struct Shape {
    const char *name;
    bool quadrics;
    size_t max_len, stride, grh;
    bool apart;
};

static void run(const Shape &sh, bool shuffled, size_t n, size_t cap, std::mt19937_64 &rng) {
    const size_t hb = sh.quadrics ? 128 : 72;
    const size_t hdr_region = sh.apart ? 3 + n * (hb + 8) + 61 : 0;
    const size_t ring_bytes = hdr_region + 5 + n * sh.stride + sh.grh;
    std::vector<uint8_t> ring(ring_bytes);
    for (size_t i = 0; i < ring_bytes; ++i) ring[i] = (uint8_t)(i * 131 + (i >> 9) * 7 + 1);
    std::vector<size_t> slot(n);
    for (size_t j = 0; j < n; ++j) slot[j] = j;
    if (shuffled) std::shuffle(slot.begin(), slot.end(), rng);
    size_t app_bytes = 64;
    std::vector<lampi_host_recv_slot> f(n);
    std::vector<size_t> aoff(n);
    for (size_t j = 0; j < n; ++j) {
        lampi_host_recv_slot &x = f[j];
        const size_t s = hdr_region + 5 + slot[j] * sh.stride + sh.grh;
        x.hdr_off = sh.apart ? 3 + j * (hb + 8) : s;
        x.frag_off = s + hb;
        x.length = (uint32_t)std::min<uint64_t>(sh.max_len, rng() % 5 == 0 ? rng() % 60 : rng() % (sh.max_len + 1));
        switch (rng() % 4) {
            case 0: x.app_len = (int64_t)x.length + 9; break;
            case 1: x.app_len = x.length / 2; break;
            case 2: x.app_len = x.length; break;
            default: x.app_len = -(int64_t)(rng() % 7);
        }
        x.reserved = 0;
        aoff[j] = app_bytes;
        app_bytes += to_copy(x) + (rng() % 3 ? 0 : rng() % 40);  // touching deliveries and gaps
    }
    app_bytes += 64;
    std::vector<uint8_t> app(app_bytes, 0xA5), want(app_bytes, 0xA5);
    for (size_t j = 0; j < n; ++j) f[j].app = app.data() + aoff[j];

    const UnpackItems items{f.data(), n, hb, sh.quadrics};
    PlanRules R;
    R.ring = true;
    R.ring_bytes = ring_bytes;
    std::vector<size_t> din(2 * n), dout(2 * n);
    StreamPlanner<UnpackItems> pl(items, R, cap, din.data(), dout.data());
    std::vector<uint8_t> dev_in(pl.in_need()), dev_out(pl.out_need());
    ChunkPlan c;
    std::vector<InXfer> in;
    std::vector<OutXfer> out;
    bool ok = true;
    size_t nchunks = 0, next_j = 0, nin = 0, nout = 0;
    uint64_t moved = 0;
    while (ok && pl.next(c, in, out)) {
        ++nchunks;
        ok = c.j0 == next_j && c.j0 % 2 == 0 && c.j1 % 2 == 0 && c.in_used <= dev_in.size() &&
             c.out_used <= dev_out.size();
        next_j = c.j1;
        std::fill(dev_in.begin(), dev_in.end(), 0xEE);
        std::fill(dev_out.begin(), dev_out.end(), 0xDD);
        for (const InXfer &t : in) {
            ++nin;
            for (size_t r = 0; ok && r < t.rows; ++r) {
                const size_t h = t.hoff + r * t.hpitch, d = t.doff + r * t.dpitch;
                ok = h + t.width <= ring_bytes && d + t.width <= dev_in.size();
                if (ok) std::memcpy(dev_in.data() + d, ring.data() + h, t.width);
                moved += t.width;
            }
        }
        for (size_t j = c.j0 / 2; ok && j < c.j1 / 2; ++j) {
            const lampi_host_recv_slot &x = f[j];
            const Payload w = items.where(x);
            const uint32_t cp = to_copy(x);
            // the header, where the pre-pass will read it
            ok = din[2 * j] + hb <= dev_in.size() && !std::memcmp(dev_in.data() + din[2 * j], ring.data() + x.hdr_off, hb);
            if (!ok || w == Payload::kNone) continue;
            const size_t at = items.payload_at(j, din.data());
            const size_t src = w == Payload::kInHeader ? x.hdr_off + kQPayloadOff : x.frag_off;
            const size_t nread = x.length;  // (every received byte is checksummed)
            ok = at + nread <= dev_in.size() && !std::memcmp(dev_in.data() + at, ring.data() + src, nread);
            const size_t to = dout[items.data_item(j)];
            ok = ok && to + cp <= dev_out.size();
            if (ok) {
                std::memcpy(dev_out.data() + to, dev_in.data() + at, cp);
                std::memcpy(want.data() + aoff[j], ring.data() + src, cp);
            }
        }
        for (const OutXfer &t : out) {
            ++nout;
            for (size_t r = 0; ok && r < t.rows; ++r) {
                uint8_t *h = t.h + r * t.hpitch;
                const size_t d = t.doff + r * t.dpitch;
                ok = h >= app.data() && h + t.width <= app.data() + app.size() && d + t.width <= dev_out.size();
                if (ok) std::memcpy(h, dev_out.data() + d, t.width);
            }
        }
    }
    ok = ok && next_j == 2 * n && app == want;
    // a batch several times the chunk size is cut up: never one chunk that outgrows the buffers
    if (ok && moved > 4 * (uint64_t)cap) ok = nchunks >= 3;
    char tail[200];
    std::snprintf(tail, sizeof tail, "%s %s n %zu cap %zu chunks %zu h2d %zu d2h %zu", sh.name,
                  shuffled ? "shuffled" : "ring_order", n, cap, nchunks, nin, nout);
    report(tail, ok);
}

int main() {
    std::mt19937_64 rng(20240);
    const Shape shapes[] = {
        {"gm_64k", false, 65456, 65536, 0, false},
        {"ib_2k_grh", false, 1976, 2048 + 40, 40, false},
        {"ib_odd_stride", false, 1976, 2051, 0, false},
        {"gm_4k_in_64k", false, 4096, 65536, 0, false},
        {"headers_apart", false, 1976, 2176, 0, true},
        {"quadrics_2k", true, 2048, 2304, 0, false},
        {"quadrics_inline", true, 52, 128, 0, false},
        {"quadrics_apart", true, 1976, 2176, 0, true},
    };
    for (const Shape &sh : shapes)
        for (int shuffled = 0; shuffled < 2; ++shuffled)
            for (size_t cap : {(size_t)4096, (size_t)65536, (size_t)1 << 20, (size_t)32 << 20})
                for (size_t n : {(size_t)1, (size_t)65, (size_t)400}) run(sh, shuffled != 0, n, cap, rng);
    std::printf("bad %d done\n", g_bad);
    return g_bad != 0;
}
