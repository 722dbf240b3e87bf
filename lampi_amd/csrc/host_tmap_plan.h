// host_tmap_plan.h -- DMA planning for the host-memory typemap steps of liblampi_csum.so (host_tmap.cc:
// lampi_host_tmap_send_pack, lampi_host_tmap_recv_unpack_batch).  Internal; host code with no HIP
// call in it, so the CPU check of the plan (tests/native_host_tmap/tmap_plan_check.cc) includes it as it is and
// executes every transfer with memcpy.
//
// A window [p0, p1) of a message's packed bytes sits in a device chunk in packed layout.  Two routes move it:
//
//   pieces (either direction, always legal): over the window's whole elements one 2D transfer per typemap pair --
//          width size_i, host pitch extent, device pitch packed_size, device offset seq_offset_i --; the partial
//          first and last elements 1D copies; touching pairs merged first.  Where a 2D transfer is not legal
//          (extent < size_i, an extent of 0 or "negative", a single row) the rows go as 1D copies.  Exactly the
//          pieces' bytes are read (send) or written (receive).
//   span   (send only): one 1D transfer of the footprints of the window's elements into a staging area; the
//          copy-only rows of the device typemap step then gather from it.  Legal only when every gap inside an
//          element's footprint and between consecutive footprints is under a page: every byte read then lies on a
//          page that a piece of those elements touches.  Taken when, besides, an element is at most
//          kTmapSpanRowBytes host bytes per DMA row of the pieces route (measured, below) and the span at most
//          kTmapSpanRatio times the window (a bound on staging memory).  Without it an 8-byte-block vector is one
//          DMA row per block: 2.2 GiB/s against 16-23.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/lampi_csum.h"

namespace lampi {

// One transfer between host memory and the packed chunk: rows x width bytes, row r at h_base + hoff + r * hpitch
// (mod 2^64: offsets may be negative) and at chunk offset doff + r * dpitch.  rows == 1: a 1D copy.
struct TmapXfer {
    uint64_t hoff, doff;
    uint64_t width, rows, hpitch, dpitch;
};

// The span route's one transfer: host bytes [h_base + lo, + bytes) to the staging area's start.
struct TmapSpan {
    uint64_t lo, bytes;
};

// A gap the span route may read over: under a page, so no page is read that no piece touches.  A condition.
constexpr uint64_t kTmapSpanGap = 4096;
// The span route is taken for types whose elements cost the pieces route a DMA row per at most this many host
// bytes (extent / merged pairs).  Measured (tools/microbench/host_tmap_ab.py --sweep, profiles/r13/host_tmap_ab.txt,
// one MI355X box): the pitched route pays per ROW -- 8-byte rows move 2.1-2.2 GiB/s of packed bytes at every stride,
// 3.4 ns a row, 512-byte rows 22-34 GiB/s -- and the span route per HOST byte, 5.1-5.5 ms per 256 MiB whatever the
// type; 8-byte blocks cross over between strides 136 (span 5.1 ms, pieces 7.0) and 264 (5.1 and 3.7), at 177 by
// the two rates, and 512-byte blocks never do (stride 768: pieces 4.9 ms, span 5.5).  A ratio to the packed bytes,
// the first guess here, fits neither: its crossover is 22 for 8-byte blocks and under 1.5 for 512-byte blocks.
#ifndef LAMPI_TMAP_SPAN_ROW_BYTES
#define LAMPI_TMAP_SPAN_ROW_BYTES 176
#endif
constexpr uint64_t kTmapSpanRowBytes = LAMPI_TMAP_SPAN_ROW_BYTES;
// ... and only up to this many staged bytes per byte of the window: a bound on the staging memory (3 chunks of 32 MiB
// times this), not a tuning value; it lies past the 8-byte blocks' crossover.
// The sweep's two columns are two builds of the library, -DLAMPI_TMAP_SPAN_RATIO=0 (the pieces route alone) and
// -DLAMPI_TMAP_SPAN_RATIO=1000000 -DLAMPI_TMAP_SPAN_ROW_BYTES=1000000000 (the span route wherever it is legal), loaded
// through LAMPI_CSUM_LIB; no run-time switch exists.
#ifndef LAMPI_TMAP_SPAN_RATIO
#define LAMPI_TMAP_SPAN_RATIO 24
#endif
constexpr uint64_t kTmapSpanRatio = LAMPI_TMAP_SPAN_RATIO;

// True when the pairs are in packed order and cover packed_size: seq_offset[0] = 0, seq_offset[i+1] =
// seq_offset[i] + size[i], size >= 1, the sizes sum to packed_size.
inline bool tmap_consistent(const lampi_host_tmap &t) {
    uint64_t run = 0;
    for (uint32_t i = 0; i < t.num_pairs; ++i) {
        const lampi_tmap_elt &e = t.h_pairs[i];
        if (e.size == 0 || (uint64_t)e.seq_offset != run || e.size > t.packed_size - run) return false;
        run += e.size;
    }
    return run == t.packed_size;
}

class TmapPlan {
  public:
    // t: checked (tmap_consistent, num_pairs >= 1, count * packed_size < 2^63); its pairs are copied.
    // ratio: the span route's bound (0: never; the CPU check of the plan passes its own).
    explicit TmapPlan(const lampi_host_tmap &t, uint64_t ratio = kTmapSpanRatio)
        : ext_(t.extent), ps_(t.packed_size), count_(t.count), ratio_(ratio) {
        for (uint32_t i = 0; i < t.num_pairs; ++i) {
            const lampi_tmap_elt &e = t.h_pairs[i];
            if (!m_.empty() && (uint64_t)m_.back().offset + m_.back().size == (uint64_t)e.offset)
                m_.back().size += e.size;  // touching pieces are one
            else
                m_.push_back(e);
        }
        // the span route's condition, for the type: a positive extent, the footprint and its gaps
        using i128 = __int128;
        std::vector<std::pair<i128, i128>> iv;
        for (const lampi_tmap_elt &e : m_) iv.emplace_back((i128)e.offset, (i128)e.offset + (i128)e.size);
        std::sort(iv.begin(), iv.end());
        i128 lo = iv[0].first, hi = iv[0].second;
        bool ok = (int64_t)ext_ > 0;
        for (size_t i = 1; i < iv.size() && ok; ++i) {
            if (iv[i].first > hi && iv[i].first - hi >= (i128)kTmapSpanGap) ok = false;
            hi = std::max(hi, iv[i].second);
        }
        const i128 lim = (i128)1 << 62;
        if (ok && (lo <= -lim || hi >= lim || hi - lo >= lim)) ok = false;
        if (ok && (i128)ext_ + lo - hi >= (i128)kTmapSpanGap) ok = false;  // between consecutive footprints
        // a contiguous type is one 1D copy by the pieces route; so are rows of more than kTmapSpanRowBytes host bytes
        if (ok && m_.size() == 1 && ext_ == ps_) ok = false;
        if (ok && (unsigned __int128)ext_ > (unsigned __int128)kTmapSpanRowBytes * m_.size()) ok = false;
        span_ok_ = ok && ratio_ > 0;
        if (ok) {
            fp_lo_ = (int64_t)lo;
            fp_ = (uint64_t)(hi - lo);
        }
    }

    const std::vector<lampi_tmap_elt> &merged() const { return m_; }
    uint64_t total() const { return count_ * ps_; }

    // The pieces route for the window [p0, p1), p1 <= total(), whose byte p0 is at chunk offset doff0: appended to
    // out, in packed order.
    void pieces(uint64_t p0, uint64_t p1, uint64_t doff0, std::vector<TmapXfer> &out) const {
        if (p1 <= p0) return;
        const uint64_t e0 = p0 / ps_, r0 = p0 - e0 * ps_, e1 = p1 / ps_, r1 = p1 - e1 * ps_;
        const uint64_t at0 = doff0 - p0;  // (mod 2^64) chunk offset of packed byte 0
        if (r0) part(e0, r0, std::min(ps_, r0 + (p1 - p0)), at0, out);
        const uint64_t ea = e0 + (r0 ? 1 : 0);
        if (e1 > ea) whole(ea, e1, at0, out);
        if (r1 && (e1 > e0 || r0 == 0)) part(e1, 0, r1, at0, out);
    }

    // The span route for the window [p0, p1): true when it is legal and taken, with the transfer and the gather's
    // base offset -- the staging area's first byte stands for h_base + s.lo.  cap: staging bytes available.
    bool span(uint64_t p0, uint64_t p1, uint64_t cap, TmapSpan &s) const {
        if (!span_ok_ || p1 <= p0) return false;
        const uint64_t ea = p0 / ps_, eb = (p1 - 1) / ps_;  // the elements the window touches
        const unsigned __int128 bytes = (unsigned __int128)(eb - ea) * ext_ + fp_;
        if (bytes > (unsigned __int128)ratio_ * (p1 - p0) || bytes > cap) return false;
        s.lo = ea * ext_ + (uint64_t)fp_lo_;
        s.bytes = (uint64_t)bytes;
        return true;
    }
    // The most staging bytes span() can ask for with windows of at most `window` bytes.
    uint64_t span_need(uint64_t window) const {
        if (!span_ok_) return 0;
        // by the ratio, and by the footprints of the elements such a window can touch
        const unsigned __int128 a = (unsigned __int128)ratio_ * window;
        const unsigned __int128 b = (unsigned __int128)(window / ps_ + 1) * ext_ + fp_;
        const unsigned __int128 n = a < b ? a : b;
        return n > ((uint64_t)1 << 40) ? (uint64_t)1 << 40 : (uint64_t)n;
    }

  private:
    // bytes [ra, rb) of element e
    void part(uint64_t e, uint64_t ra, uint64_t rb, uint64_t at0, std::vector<TmapXfer> &out) const {
        size_t a = 0, b = m_.size();  // the last merged piece with seq_offset <= ra
        while (b - a > 1) {
            const size_t mid = a + (b - a) / 2;
            if ((uint64_t)m_[mid].seq_offset <= ra) a = mid;
            else b = mid;
        }
        for (size_t i = a; i < m_.size() && (uint64_t)m_[i].seq_offset < rb; ++i) {
            const uint64_t seq = (uint64_t)m_[i].seq_offset;
            const uint64_t x = std::max(seq, ra), y = std::min(seq + m_[i].size, rb);
            if (y <= x) continue;
            out.push_back(TmapXfer{e * ext_ + (uint64_t)m_[i].offset + (x - seq), at0 + e * ps_ + x, y - x, 1, y - x,
                                   y - x});
        }
    }
    // whole elements [ea, eb)
    void whole(uint64_t ea, uint64_t eb, uint64_t at0, std::vector<TmapXfer> &out) const {
        const uint64_t rows = eb - ea;
        if (m_.size() == 1 && ext_ == ps_) {  // contiguous
            out.push_back(TmapXfer{ea * ext_ + (uint64_t)m_[0].offset, at0 + ea * ps_, rows * ps_, 1, rows * ps_,
                                   rows * ps_});
            return;
        }
        for (const lampi_tmap_elt &m : m_) {
            const uint64_t h = ea * ext_ + (uint64_t)m.offset, d = at0 + ea * ps_ + (uint64_t)m.seq_offset;
            if (rows > 1 && (int64_t)ext_ > 0 && ext_ >= m.size) {
                out.push_back(TmapXfer{h, d, m.size, rows, ext_, ps_});
                continue;
            }
            for (uint64_t r = 0; r < rows; ++r)
                out.push_back(TmapXfer{h + r * ext_, d + r * ps_, m.size, 1, m.size, m.size});
        }
    }

    std::vector<lampi_tmap_elt> m_;  // the pairs, touching ones merged
    uint64_t ext_, ps_, count_, ratio_;
    bool span_ok_ = false;
    int64_t fp_lo_ = 0;  // an element's footprint: [fp_lo_, fp_lo_ + fp_) from its origin
    uint64_t fp_ = 0;
};

}  // namespace lampi
