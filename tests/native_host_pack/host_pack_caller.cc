// host_pack_caller.cc -- a native C++ caller of the host-memory one-call steps (lampi_host_msg_send_pack,
// lampi_host_recv_unpack_batch; include/lampi_csum.h) as gmPath::send's loop and gmPath::receive's drain would use
// them.
//
// Per kind (GM 65,456-byte fragments in 64 KiB buffers, IB 1,976 in 2 KiB, Quadrics 2,048 behind 128-byte envelopes
// with an inline tail) and mode (CRC, SUM, checksumming off): a message in host memory is packed into a host ring
// in three gated calls; every slot is rebuilt here from the oracle (oracle/libcsum_ref.so, test infrastructure) and
// compared byte for byte, the bytes between the slots' contents with the pattern the ring held.  Then headers and
// payloads are corrupted, the ring is drained by one receive call, and every verdict, count, checksum and application
// byte is compared with the reference's rules restated on the oracle.  Both calls run on two threads at once, then on
// the main thread after lampi_host_release(); pinned and scratch bytes must be 0 after the last release.  The pipeline
// chunk is 256 KiB (LAMPI_HOST_CHUNK_BYTES), so every call spans several chunks.
// Prints one line per call and "bad N done"; exits 1 on any mismatch.  Build: make -C tests/native_host_pack.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "lampi_csum.h"
#include "../../oracle/csum_ref.h"

static std::mutex g_out;
static int g_bad = 0;

static void report(const std::string &line, bool ok) {
    std::lock_guard<std::mutex> g(g_out);
    std::printf("%s %s\n", line.c_str(), ok ? "ok" : "BAD");
    if (!ok) ++g_bad;
}

static uint32_t rd32(const uint8_t *p) {
    uint32_t v;
    std::memcpy(&v, p, 4);
    return v;
}
static void wr32(uint8_t *p, uint32_t v) { std::memcpy(p, &v, 4); }
static void wr64(uint8_t *p, uint64_t v) { std::memcpy(p, &v, 8); }

struct Shape {
    const char *name;
    int kind;
    size_t L, S, msg_len;
};

static uint32_t data_csum(const uint8_t *p, size_t len, int mode) {
    if (mode == LAMPI_CSUM_CRC32) return oracle_uicrc(p, len, ORACLE_CRC_INIT);
    uint32_t pi = 0, pl = 0;
    return oracle_uicsum(p, len, &pi, &pl);
}

static size_t hdr_bytes(int kind) { return kind == LAMPI_SEND_HDR_QUADRICS ? 128 : 72; }
static bool inline_frag(int kind, size_t len) { return kind == LAMPI_SEND_HDR_QUADRICS && len > 0 && len <= 52; }

// Slot k's header as the send step must leave it (the tables of include/lampi_csum.h, restated on the oracle).
static std::vector<uint8_t> want_header(const Shape &s, const lampi_send_hdr_fill &fill, const uint8_t *msg, size_t k,
                                        int mode) {
    const size_t hb = hdr_bytes(s.kind), off = k * s.L;
    const size_t len = s.msg_len > off ? std::min(s.L, s.msg_len - off) : 0;
    std::vector<uint8_t> h(hb, 0);
    std::memcpy(h.data(), fill.tmpl, 72);
    wr32(h.data() + 20, (uint32_t)len);
    wr64(h.data() + 32, fill.frag_seq0 + k * fill.frag_seq_step);
    wr64(h.data() + 48, fill.desc_ptr0 + k * fill.desc_ptr_stride);
    wr64(h.data() + 56, fill.seq_offset0 + (uint64_t)off);
    const bool none = mode == LAMPI_CSUM_NONE, crc = mode == LAMPI_CSUM_CRC32;
    const uint32_t v = none ? 0u : data_csum(msg + off, len, mode);
    if (s.kind == LAMPI_SEND_HDR_QUADRICS) {
        wr32(h.data() + 68, rd32(fill.tmpl + 68) + (uint32_t)off);
        if (inline_frag(s.kind, len)) std::memcpy(h.data() + 72, msg + off, len);
        if (len) wr32(h.data() + 64, v);  // (an empty fragment keeps the template's word; off: 0)
        wr32(h.data() + 124, none ? 0u : oracle_header_checksum(h.data(), 124, 32, crc));
        return h;
    }
    if (s.kind == LAMPI_SEND_HDR_GM) {
        if (!none) wr32(h.data() + 64, v);
        wr32(h.data() + 68, 0);
        if (!none) wr32(h.data() + 68, oracle_header_checksum(h.data(), 68, 18, crc));
    } else {
        wr32(h.data() + 64, len ? v : 0u);
        wr32(h.data() + 68, none ? 0u : data_csum(h.data(), 68, mode));
    }
    return h;
}

static bool header_bad(const uint8_t *h, int kind, int mode) {
    if (mode == LAMPI_CSUM_NONE) return false;
    const size_t hb = hdr_bytes(kind);
    if (kind == LAMPI_SEND_HDR_IB) return data_csum(h, 68, mode) != rd32(h + 68);
    if (mode == LAMPI_CSUM_CRC32) return oracle_uicrc(h, hb, ORACLE_CRC_INIT) != 0;
    uint32_t v = 0;
    for (size_t w = 0; w < hb / 4; ++w) v += rd32(h + 4 * w);
    return v != 2 * rd32(h + hb - 4);
}

static bool bit(const std::vector<uint32_t> &m, size_t i) { return (m[i / 32] >> (i % 32)) & 1u; }

struct Buf {  // 4096-aligned host memory, optionally page-locked
    std::vector<uint8_t> store;
    uint8_t *p;
    size_t bytes;
    bool pinned;
    Buf(size_t n, bool pin) : store(n + 8192), bytes(n), pinned(pin) {
        p = store.data() + (4096 - ((uintptr_t)store.data() & 4095));
        if (pin && lampi_host_register(p, n) != 0) pinned = false;
    }
    ~Buf() {
        if (pinned) lampi_host_unregister(p);
    }
};

static void run_case(int tid, const Shape &s, int mode, bool pin, uint64_t seed) {
    char tag[160];
    std::snprintf(tag, sizeof tag, "t%d %s mode %d ring_%s", tid, s.name, mode, pin ? "pinned" : "pageable");
    const size_t hb = hdr_bytes(s.kind);
    const size_t n = s.msg_len ? (s.msg_len - 1) / s.L + 1 : 1;
    std::vector<uint8_t> msg(s.msg_len + 1);
    oracle_fill_stream(msg.data(), seed, 0, s.msg_len);
    Buf ring(n * s.S, pin);
    oracle_fill_stream(ring.p, seed + 1, 0, ring.bytes);
    const std::vector<uint8_t> before(ring.p, ring.p + ring.bytes);
    lampi_send_hdr_fill fill;
    oracle_fill_stream(fill.tmpl, seed + 2, 0, 72);
    fill.frag_seq0 = 0x1122334455667788ull + seed;
    fill.frag_seq_step = 3;
    fill.desc_ptr0 = 0x00007F0012345000ull;
    fill.desc_ptr_stride = 0x1A8;
    fill.seq_offset0 = 0x100000010ull;

    // send: the message through a gated window, three calls
    const size_t cuts[4] = {0, std::min<size_t>(3, n), std::min<size_t>(4, n), n};
    int rc = 0;
    for (int c = 2; c >= 0 && rc == 0; --c)  // (the calls in any order give the same ring)
        rc = lampi_host_msg_send_pack(msg.data(), s.msg_len, s.L, cuts[c], cuts[c + 1] - cuts[c], ring.p + cuts[c] * s.S,
                                      s.S, &fill, s.kind, mode);
    bool ok = rc == 0;
    std::vector<uint8_t> want(before);
    for (size_t k = 0; k < n; ++k) {
        const size_t off = k * s.L, len = s.msg_len > off ? std::min(s.L, s.msg_len - off) : 0;
        const std::vector<uint8_t> h = want_header(s, fill, msg.data(), k, mode);
        std::memcpy(want.data() + k * s.S, h.data(), hb);
        if (len && !inline_frag(s.kind, len)) std::memcpy(want.data() + k * s.S + hb, msg.data() + off, len);
    }
    ok = ok && !std::memcmp(want.data(), ring.p, ring.bytes);
    report(std::string("send ") + tag + " frags " + std::to_string(n), ok);

    // corrupt some headers and payloads, then drain the ring in one call
    std::mt19937_64 rng(seed * 5 + 1);
    if (mode != LAMPI_CSUM_NONE)
        for (size_t k = 0; k < n; ++k) {
            uint8_t *h = ring.p + k * s.S;
            const size_t len = rd32(h + 20);
            const uint64_t r = k == 1 ? 0 : k == 2 ? 150 : rng() % 1000;
            if (r < 100) h[rng() % hb] ^= (uint8_t)(1 + rng() % 255);
            else if (r < 200 && len && !inline_frag(s.kind, len)) h[hb + rng() % len] ^= (uint8_t)(1 + rng() % 255);
        }
    std::vector<lampi_host_recv_slot> slots(n);
    std::vector<uint8_t> app(s.msg_len + 64, 0x5A), want_app(app.size(), 0x5A), tmp;
    for (size_t k = 0; k < n; ++k) {
        lampi_host_recv_slot &x = slots[k];
        x.hdr_off = k * s.S;
        x.frag_off = k * s.S + hb;
        x.length = (uint32_t)(s.msg_len > k * s.L ? std::min(s.L, s.msg_len - k * s.L) : 0);
        x.app = app.data() + k * s.L;
        x.app_len = k % 5 == 3 ? (int64_t)x.length / 2 : k % 5 == 4 ? 0 : (int64_t)x.length;
        x.reserved = 0;
    }
    std::vector<int64_t> copied(n + 1, 0x7777);
    std::vector<uint32_t> csum(n + 1, 0xDEADBEEFu), hmask((n + 31) / 32 + 1, 0xDEADBEEFu),
        dmask((n + 31) / 32 + 1, 0xDEADBEEFu);
    uint32_t nbad[3] = {0xDEADBEEFu, 0xDEADBEEFu, 0xDEADBEEFu};
    rc = lampi_host_recv_unpack_batch(ring.p, ring.bytes, slots.data(), n, s.kind, copied.data(), csum.data(),
                                      hmask.data(), dmask.data(), nbad, mode);
    ok = rc == 0 && copied[n] == 0x7777 && csum[n] == 0xDEADBEEFu && hmask.back() == 0xDEADBEEFu &&
         dmask.back() == 0xDEADBEEFu && nbad[2] == 0xDEADBEEFu;
    uint32_t wh = 0, wd = 0;
    for (size_t k = 0; ok && k < n; ++k) {
        const lampi_host_recv_slot &x = slots[k];
        const uint8_t *h = ring.p + x.hdr_off;
        if (header_bad(h, s.kind, mode)) {
            ++wh;
            ok = copied[k] == LAMPI_RECV_HDR_BAD && csum[k] == 0 && bit(hmask, k) && !bit(dmask, k);
            continue;
        }
        const uint8_t *frag = inline_frag(s.kind, x.length) ? h + 72 : ring.p + x.frag_off;
        const uint32_t c = x.app_len <= 0 ? 0u : (uint32_t)std::min<int64_t>(x.app_len, x.length);
        int64_t wc = c;
        uint32_t ws = mode == LAMPI_CSUM_CRC32 ? ORACLE_CRC_INIT : 0u;
        if (c && mode != LAMPI_CSUM_NONE) {
            tmp.resize(c);
            uint32_t pi = 0, pl = 0;
            ws = mode == LAMPI_CSUM_CRC32 ? oracle_bcopy_uicrc(frag, tmp.data(), c, x.length, ORACLE_CRC_INIT)
                                          : oracle_bcopy_uicsum(frag, tmp.data(), c, x.length, &pi, &pl);
            if (ws != rd32(h + 64)) {
                wc = LAMPI_RECV_DATA_BAD;
                ++wd;
            }
        }
        if (c) std::memcpy(want_app.data() + k * s.L, frag, c);
        ok = copied[k] == wc && csum[k] == ws && !bit(hmask, k) && bit(dmask, k) == (wc == LAMPI_RECV_DATA_BAD);
        if (!ok)
            std::printf("  frag %zu len %u app_len %lld: copied %lld/%lld csum %08x/%08x\n", k, x.length,
                        (long long)x.app_len, (long long)copied[k], (long long)wc, csum[k], ws);
    }
    ok = ok && nbad[0] == wh && nbad[1] == wd && app == want_app;
    for (size_t i = n; ok && i < ((n + 31) / 32) * 32; ++i) ok = !bit(hmask, i) && !bit(dmask, i);
    report(std::string("recv ") + tag + " hdr_bad " + std::to_string(wh) + " data_bad " + std::to_string(wd), ok);
}

static void run_suite(int tid, const std::vector<Shape> &shapes) {
    uint64_t seed = 2000 + 97 * (uint64_t)tid;
    for (const Shape &s : shapes)
        for (int mode : {LAMPI_CSUM_CRC32, LAMPI_CSUM_SUM32, LAMPI_CSUM_NONE})
            for (int pin = 0; pin < 2; ++pin) run_case(tid, s, mode, pin != 0, seed += 3);
}

// Invalid arguments write nothing; empty calls.
static void run_edges() {
    std::vector<uint8_t> msg(4096, 0x33), ring(1 << 16, 0x11), app(4096, 0x5A);
    lampi_send_hdr_fill fill{};
    bool ok = lampi_host_msg_send_pack(msg.data(), 4096, 512, 0, 8, ring.data(), 1024, nullptr, 0, 0) != 0 &&
              lampi_host_msg_send_pack(msg.data(), 4096, 512, 0, 8, ring.data(), 1024, &fill, 2, 0) != 0 &&
              lampi_host_msg_send_pack(msg.data(), 4096, 512, 0, 8, ring.data(), 1024, &fill, 0, 3) != 0 &&
              lampi_host_msg_send_pack(msg.data(), 4096, 512, 0, 8, ring.data(), 583, &fill, 0, 0) != 0 &&
              lampi_host_msg_send_pack(msg.data(), 4096, 512, 0, 9, ring.data(), 1024, &fill, 0, 0) != 0 &&
              lampi_host_msg_send_pack(msg.data(), 4096, 512, 0, 0, ring.data(), 1024, &fill, 0, 0) == 0;
    lampi_host_recv_slot x{};
    x.hdr_off = 0;
    x.frag_off = 72;
    x.length = 512;
    x.app = app.data();
    x.app_len = 512;
    int64_t copied = 0x7777;
    uint32_t csum = 0xDEADBEEFu, hm = 0xDEADBEEFu, dm = 0xDEADBEEFu, nbad[2] = {0xDEADBEEFu, 0xDEADBEEFu};
    ok = ok && lampi_host_recv_unpack_batch(ring.data(), 500, &x, 1, 0, &copied, &csum, &hm, &dm, nbad, 0) != 0 &&
         lampi_host_recv_unpack_batch(ring.data(), ring.size(), &x, 1, 2, &copied, &csum, &hm, &dm, nbad, 0) != 0 &&
         lampi_host_recv_unpack_batch(ring.data(), ring.size(), &x, 1, 0, &copied, &csum, &hm, &dm, nullptr, 0) != 0 &&
         lampi_host_recv_unpack_batch(ring.data(), ring.size(), &x, 0, 0, nullptr, &csum, &hm, &dm, nbad, 0) != 0;
    x.reserved = 1;
    ok = ok && lampi_host_recv_unpack_batch(ring.data(), ring.size(), &x, 1, 0, &copied, &csum, &hm, &dm, nbad, 0) != 0;
    ok = ok && copied == 0x7777 && csum == 0xDEADBEEFu && hm == 0xDEADBEEFu && dm == 0xDEADBEEFu &&
         nbad[0] == 0xDEADBEEFu && nbad[1] == 0xDEADBEEFu;
    for (uint8_t b : ring) ok = ok && b == 0x11;
    for (uint8_t b : app) ok = ok && b == 0x5A;
    report("invalid_arguments_refused", ok);
    ok = lampi_host_recv_unpack_batch(nullptr, 0, nullptr, 0, 0, &copied, &csum, &hm, &dm, nbad, 0) == 0 &&
         nbad[0] == 0 && nbad[1] == 0 && copied == 0x7777;
    report("empty_batch", ok);
}

int main(int argc, char **argv) {
    const int nthreads = argc > 1 ? std::atoi(argv[1]) : 2;
    setenv("LAMPI_HOST_CHUNK_BYTES", "262144", 1);
    const std::vector<Shape> shapes = {
        {"gm65456", LAMPI_SEND_HDR_GM, 65456, 65536, 40 * 65456 + 1234},
        {"ib1976", LAMPI_SEND_HDR_IB, 1976, 2048, 1200 * 1976 + 7},
        {"quadrics2048", LAMPI_SEND_HDR_QUADRICS, 2048, 2304, 1000 * 2048 + 40},
        {"quadrics52", LAMPI_SEND_HDR_QUADRICS, 52, 128, 5000 * 52 + 17},
        {"empty_gm", LAMPI_SEND_HDR_GM, 65456, 65536, 0},
    };
    run_edges();
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; ++t) th.emplace_back(run_suite, t + 1, std::cref(shapes));
    for (auto &t : th) t.join();
    lampi_host_release();
    run_suite(0, shapes);
    lampi_host_release();
    std::printf("pinned_after_release %lld scratch_after_release %lld\n", (long long)lampi_host_pinned_bytes(),
                (long long)lampi_device_scratch_bytes());
    std::printf("bad %d done\n", g_bad);
    return g_bad != 0;
}
