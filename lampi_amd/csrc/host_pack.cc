// host_pack.cc -- the one-call send and receive steps over host memory (lampi_host_msg_send_pack,
// lampi_host_recv_unpack_batch; include/lampi_csum.h).
//
// Both run on the calling thread's pipeline (host_msg.cc, host_pipe.h) and put the device forms' own
// launches between the DMA transfers:
//
//   send    s_in : H2D of chunk i's message bytes
//           s_k  : launch_msg_send_pack into a device image of the chunk's slots (headers and payloads, a compact
//                  8-byte-aligned stride), the fill shifted to the chunk's first fragment
//           s_out: one pitched D2H of header + payload rows into the caller's ring (1D where the slots are dense)
//   receive s_in : H2D of the ring bytes under chunk i's headers and payloads (host_plan.h: a header right before
//                  its payload is one item, so GM / IB / Quadrics slots are the DMA runs they were without headers)
//           s_k  : launch_host_recv_hdr (the header tests, at whatever alignment the runs left the headers), a small
//                  D2H of its verdicts, then the unchanged launch_copy_to_app into the packed output chunk
//           s_out: D2H of the delivered bytes -- queued by the host once it has chunk i's verdicts, and only for the
//                  fragments whose header passed; chunk i + 1 is already queued by then
//           With checksumming off no header is read: the call is lampi_host_copy_to_app_batch's copy (host_recv.cc).
//
// The CPU reads the caller's records and no ring or message byte.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>

#include "../../include/lampi_csum.h"
#include "frag_csum_kernels.h"
#include "host_internal.h"
#include "host_pack_items.h"
#include "host_pipe.h"
#include "host_plan.h"

namespace lampi {
namespace {

#define TRY LAMPI_TRY

size_t hdr_bytes_of(int kind) { return kind == LAMPI_SEND_HDR_QUADRICS ? 128 : 72; }
bool kind_ok(int kind) {
    return kind == LAMPI_SEND_HDR_GM || kind == LAMPI_SEND_HDR_IB || kind == LAMPI_SEND_HDR_QUADRICS;
}
bool mode_ok(int mode) { return mode == LAMPI_CSUM_CRC32 || mode == LAMPI_CSUM_SUM32 || mode == LAMPI_CSUM_NONE; }

// ---- send ---------------------------------------------------------------------------------------------

// What a slot holds after the step: its header, and the payload unless it travels inside a Quadrics
// envelope (at most 52 bytes) or is not copied at all (a bare envelope queue).
struct SlotShape {
    size_t hb;
    bool quadrics, bare;
    size_t row(size_t len) const { return quadrics && (bare || len <= kQInlineMax) ? hb : hb + len; }
};

// the series of lampi_send_hdr_fill moved on by k fragments
lampi_send_hdr_fill shifted_fill(const lampi_send_hdr_fill &f, size_t k, size_t frag_len, bool quadrics) {
    lampi_send_hdr_fill g = f;
    g.frag_seq0 += (uint64_t)k * f.frag_seq_step;
    g.desc_ptr0 += (uint64_t)k * f.desc_ptr_stride;
    g.seq_offset0 += (uint64_t)k * frag_len;
    if (quadrics) {  // dataElanAddr @68: tmpl's + k * frag_len mod 2^32
        uint32_t w;
        std::memcpy(&w, g.tmpl + 68, 4);
        w += (uint32_t)((uint64_t)k * frag_len);
        std::memcpy(g.tmpl + 68, &w, 4);
    }
    return g;
}

}  // namespace

hipError_t host_send_pack(const uint8_t *h_msg, size_t msg_len, size_t frag_len, size_t k_first, size_t k_count,
                          uint8_t *h_ring, size_t stride, const lampi_send_hdr_fill &fill, int kind, int mode,
                          const SendSource *src) {
    PipeState *pp = nullptr;
    TRY(pipe_ctx(&pp));
    PipeState &p = *pp;
    const uint32_t *img = nullptr;
    TRY(device_tables(p.dev, &img));

    const bool quadrics = kind == LAMPI_SEND_HDR_QUADRICS;
    const SlotShape sh{hdr_bytes_of(kind), quadrics, quadrics && stride == 128};
    const size_t b0 = k_first * frag_len;
    const size_t b1 = std::min(msg_len, (k_first + k_count) * frag_len);
    const size_t last = b1 - (b0 + (k_count - 1) * frag_len);  // bytes of the call's last fragment
    const size_t width = sh.row(frag_len);                      // bytes of a full fragment's slot
    const size_t dstride = align_up(width, 8);                  // slots of the device image
    const size_t fpc = std::max<size_t>(1, chunk_target(true) / frag_len);  // fragments per chunk
    const size_t stage_off = align_up(fpc * frag_len, 256);  // (a source's staging bytes, behind the chunk's own)
    TRY(ensure_chunks(p, src ? stage_off + src->extra : fpc * frag_len));
    TRY(ensure_out_chunks(p, fpc * dstride));

    PipeDrain drain(p);  // any early return below leaves nothing in flight
    const size_t nchunks = (k_count + fpc - 1) / fpc;
    for (size_t i = 0; i < nchunks; ++i) {
        const int b = (int)(i % kBufs);
        const size_t f0 = i * fpc, nf = std::min(fpc, k_count - f0);
        const size_t off = b0 + f0 * frag_len, nb = std::min(nf * frag_len, b1 - off);
        uint8_t *d = p.dchunk + (size_t)b * p.chunk_bytes;
        uint8_t *dimg = p.dout + (size_t)b * p.out_bytes;
        // chunk b is free once chunk i - kBufs was packed and its slots were sent back
        if (i >= (size_t)kBufs) {
            TRY(hipStreamWaitEvent(p.s_in, p.k_done[b], 0));
            TRY(hipStreamWaitEvent(p.s_k, p.out_done[b], 0));
        }
        if (nb && src)
            TRY(src->in(src->ctx, off, nb, d, d + stage_off, p.s_in));
        else if (nb)
            TRY(hipMemcpyAsync(d, h_msg + off, nb, hipMemcpyHostToDevice, p.s_in));
        TRY(hipEventRecord(p.in_done[b], p.s_in));
        TRY(hipStreamWaitEvent(p.s_k, p.in_done[b], 0));
        if (nb && src && src->gather) TRY(src->gather(src->ctx, off, nb, d, d + stage_off, p.s_k));
        const lampi_send_hdr_fill g = shifted_fill(fill, k_first + f0, frag_len, quadrics);
        TRY(launch_msg_send_pack(d, nb, frag_len, dimg, dstride, g, nf, kind, mode, img, p.s_k));
        TRY(hipEventRecord(p.k_done[b], p.s_k));
        TRY(hipStreamWaitEvent(p.s_out, p.k_done[b], 0));
        // the slots: full fragments as rows of one copy, a shorter last one (fewer bytes to write) on its own
        const size_t tail = f0 + nf == k_count ? sh.row(last) : width;
        const size_t full = nf - (tail != width ? 1 : 0);
        uint8_t *h = h_ring + f0 * stride;
        if (full == 1 || (full > 1 && stride == width && dstride == width))
            TRY(hipMemcpyAsync(h, dimg, full * width, hipMemcpyDeviceToHost, p.s_out));
        else if (full > 1)
            TRY(hipMemcpy2DAsync(h, stride, dimg, dstride, width, full, hipMemcpyDeviceToHost, p.s_out));
        if (full != nf)
            TRY(hipMemcpyAsync(h + full * stride, dimg + full * dstride, tail, hipMemcpyDeviceToHost, p.s_out));
        TRY(hipEventRecord(p.out_done[b], p.s_out));
    }
    TRY(hipStreamSynchronize(p.s_k));
    TRY(hipStreamSynchronize(p.s_out));
    drain.armed = false;
    return hipSuccess;
}

namespace {

// ---- receive ------------------------------------------------------------------------------------------

// Per-thread planning scratch, kept between calls.
struct UnpackScratch {
    std::vector<size_t> din, dout;
    std::vector<InXfer> in;
    std::vector<OutXfer> out[2];  // a chunk's deliveries wait for its verdicts while the next chunk is planned
    std::vector<lampi_host_recv_frag> frags;  // checksumming off: the batch as lampi_host_copy_to_app_batch takes it
};
thread_local UnpackScratch t_unpack;

struct Pending {
    bool any = false;
    int b = 0;
    size_t f0 = 0, f1 = 0;
    const std::vector<OutXfer> *out = nullptr;
};

}  // namespace

hipError_t host_recv_unpack(const uint8_t *h_ring, size_t ring_bytes, const lampi_host_recv_slot *f, size_t n,
                            int kind, int64_t *h_copied, uint32_t *h_csum, uint32_t *h_hmask, uint32_t *h_dmask,
                            uint32_t *h_nbad, int mode, const OutSink *sink) {
    UnpackScratch &us = t_unpack;
    if (us.din.size() < 2 * n) {
        us.din.resize(2 * n);
        us.dout.resize(2 * n);
    }
    const UnpackItems items{f, n, hdr_bytes_of(kind), kind == LAMPI_SEND_HDR_QUADRICS};
    PlanRules rules;
    rules.ring = true;
    rules.ring_bytes = ring_bytes;
    StreamPlanner<UnpackItems> pl(items, rules, chunk_target(true), us.din.data(), us.dout.data());
    PipeState *pp = nullptr;
    TRY(pipe_ctx(&pp));
    PipeState &p = *pp;
    const uint32_t *img = nullptr;
    TRY(device_tables(p.dev, &img));
    TRY(ensure_chunks(p, std::max<size_t>(pl.in_need(), 256)));
    TRY(ensure_out_chunks(p, std::max<size_t>(pl.out_need(), 256)));

    // descriptors, header addresses (both go up with their chunk), header verdicts (they come back with it), the
    // copy's results (one D2H at the end) and its own mask and count, which the host never reads
    const size_t o_hdr = align_up(n * sizeof(lampi_recv_desc), 256);
    const size_t o_bad = align_up(o_hdr + n * sizeof(uint64_t), 256);
    const size_t o_copied = align_up(o_bad + n * sizeof(uint32_t), 256);
    const size_t o_csum = align_up(o_copied + n * sizeof(int64_t), 256);
    const size_t o_scratch = align_up(o_csum + n * sizeof(uint32_t), 256);
    const size_t total = o_scratch + ((n + 31) / 32 + 2) * sizeof(uint32_t);
    TRY(ensure_meta(p, total));
    lampi_recv_desc *hd = (lampi_recv_desc *)p.hmeta;
    uint64_t *hh = (uint64_t *)(p.hmeta + o_hdr);
    uint32_t *hbad = (uint32_t *)(p.hmeta + o_bad);
    uint8_t *dm = p.dmeta;
    uint32_t *dmask = (uint32_t *)(dm + o_scratch), *dnbad = dmask + (n + 31) / 32 + 1;

    PipeDrain drain(p);  // any early return below leaves nothing in flight

    // A chunk's deliveries, once its verdicts are known: the planner's transfers as they are when every header
    // passed; otherwise a copy per run of passed fragments that touch in the application buffer and in the chunk.
    auto deliver = [&](const Pending &q) -> hipError_t {
        if (!q.any) return hipSuccess;
        const uint8_t *dout = p.dout + (size_t)q.b * p.out_bytes;
        bool dropped = false;
        TRY(hipEventSynchronize(p.v_done[q.b]));
        for (size_t j = q.f0; j < q.f1 && !dropped; ++j) dropped = hbad[j] != 0;
        TRY(hipStreamWaitEvent(p.s_out, p.k_done[q.b], 0));
        const auto put = [&](uint8_t *h, const uint8_t *d, size_t len) -> hipError_t {
            return sink ? sink->run(sink->ctx, h, d, len, p.s_out)
                        : hipMemcpyAsync(h, d, len, hipMemcpyDeviceToHost, p.s_out);
        };
        if (!dropped && sink) {
            TRY(issue_out_rows(*q.out, dout, put));
        } else if (!dropped) {
            TRY(issue_out(*q.out, dout, p.s_out));
        } else {
            uint8_t *h = nullptr;
            size_t doff = 0, len = 0;
            for (size_t j = q.f0; j <= q.f1; ++j) {
                const size_t c = j < q.f1 && !hbad[j] ? to_copy(f[j]) : 0;
                if (c && len && (uint8_t *)f[j].app == h + len && us.dout[items.data_item(j)] == doff + len) {
                    len += c;
                    continue;
                }
                if (j < q.f1 && !c) continue;  // dropped, or nothing to deliver: the open run stays open
                if (len) TRY(put(h, dout + doff, len));
                h = c ? (uint8_t *)f[j].app : nullptr;
                doff = c ? us.dout[items.data_item(j)] : 0;
                len = c;
            }
        }
        TRY(hipEventRecord(p.out_done[q.b], p.s_out));
        return hipSuccess;
    };

    ChunkPlan k;
    Pending prev;
    for (size_t c = 0; pl.next(k, us.in, us.out[c % 2]); ++c) {
        const int b = (int)(c % kBufs);
        uint8_t *din = p.dchunk + (size_t)b * p.chunk_bytes;
        uint8_t *dout = p.dout + (size_t)b * p.out_bytes;
        const size_t f0 = k.j0 / 2, f1 = k.j1 / 2;
        uint64_t payload = 0;
        size_t nread = 0;
        for (size_t j = f0; j < f1; ++j) {
            const Payload w = items.where(f[j]);
            const uint8_t *hdr = din + us.din[2 * j];
            const size_t jd = items.data_item(j);  // the item that carries the delivery
            const uint8_t *frag = din + items.payload_at(j, us.din.data());  // (inline: the pre-pass sets it too)
            hd[j] = lampi_recv_desc{(uint64_t)(uintptr_t)frag,
                                    (uint64_t)(uintptr_t)(w != Payload::kNone ? dout + us.dout[jd] : dout),
                                    f[j].app_len, f[j].length, 0u};
            hh[j] = (uint64_t)(uintptr_t)hdr;
            if (w != Payload::kNone) {
                payload += f[j].length;
                ++nread;
            }
        }
        // chunk b's buffers are free once chunk c - kBufs was copied to the app and sent back
        if (c >= (size_t)kBufs) {
            TRY(hipStreamWaitEvent(p.s_in, p.k_done[b], 0));
            TRY(hipStreamWaitEvent(p.s_in, p.out_done[b], 0));
        }
        if (f1 > f0) {
            TRY(hipMemcpyAsync(dm + f0 * sizeof(lampi_recv_desc), hd + f0, (f1 - f0) * sizeof(lampi_recv_desc),
                               hipMemcpyHostToDevice, p.s_in));
            TRY(hipMemcpyAsync(dm + o_hdr + f0 * sizeof(uint64_t), hh + f0, (f1 - f0) * sizeof(uint64_t),
                               hipMemcpyHostToDevice, p.s_in));
        }
        TRY(issue_in(us.in, h_ring, din, p.s_in));
        TRY(hipEventRecord(p.in_done[b], p.s_in));
        TRY(hipStreamWaitEvent(p.s_k, p.in_done[b], 0));
        lampi_recv_desc *dd = (lampi_recv_desc *)dm + f0;
        if (f1 > f0) {
            uint32_t *dbad = (uint32_t *)(dm + o_bad) + f0;
            TRY(launch_host_recv_hdr(dd, (const uint64_t *)(dm + o_hdr) + f0, f1 - f0, kind, mode, img, dbad, p.s_k));
            TRY(hipMemcpyAsync(hbad + f0, dbad, (f1 - f0) * sizeof(uint32_t), hipMemcpyDeviceToHost, p.s_k));
        }
        TRY(hipEventRecord(p.v_done[b], p.s_k));
        // rows per fragment for the copy's row-group schedule: the mean payload in 4 KiB rows (host_recv.cc)
        const uint64_t rows = nread ? (payload / nread + 4095) / 4096 : 1;
        const uint32_t hint = rows >= 2 ? (uint32_t)std::min<uint64_t>(rows, 0xFFF) : 1u;
        TRY(launch_copy_to_app(dd, f1 - f0, (const uint8_t *)dd + offsetof(lampi_recv_desc, reserved),
                               sizeof(lampi_recv_desc), (int64_t *)(dm + o_copied) + f0,
                               (uint32_t *)(dm + o_csum) + f0, dmask, dnbad, mode, img, p.s_k, hint));
        TRY(hipEventRecord(p.k_done[b], p.s_k));
        // chunk c is queued: now wait for chunk c - 1's verdicts and queue its deliveries
        TRY(deliver(prev));
        prev = Pending{true, b, f0, f1, &us.out[c % 2]};
    }
    TRY(deliver(prev));
    TRY(hipMemcpyAsync(p.hmeta + o_copied, dm + o_copied, o_scratch - o_copied, hipMemcpyDeviceToHost, p.s_k));
    TRY(hipStreamSynchronize(p.s_k));
    TRY(hipStreamSynchronize(p.s_out));
    drain.armed = false;

    // the header verdicts over the copy's results
    const int64_t *hc = (const int64_t *)(p.hmeta + o_copied);
    const uint32_t *hs = (const uint32_t *)(p.hmeta + o_csum);
    std::memset(h_hmask, 0, (n + 31) / 32 * sizeof(uint32_t));
    std::memset(h_dmask, 0, (n + 31) / 32 * sizeof(uint32_t));
    uint32_t nh = 0, nd = 0;
    for (size_t i = 0; i < n; ++i) {
        if (hbad[i]) {
            h_copied[i] = LAMPI_RECV_HDR_BAD;
            h_csum[i] = 0u;
            h_hmask[i / 32] |= 1u << (i % 32);
            ++nh;
            continue;
        }
        h_copied[i] = hc[i];
        h_csum[i] = hs[i];
        if (hc[i] < 0) {
            h_dmask[i / 32] |= 1u << (i % 32);
            ++nd;
        }
    }
    h_nbad[0] = nh;
    h_nbad[1] = nd;
    return hipSuccess;
}

}  // namespace lampi

using namespace lampi;

extern "C" {

int lampi_host_msg_send_pack(const void *h_msg, size_t msg_len, size_t frag_len, size_t k_first, size_t k_count,
                             void *h_ring, size_t slot_stride, const lampi_send_hdr_fill *h_fill, int hdr_kind,
                             int mode) {
    if (!mode_ok(mode) || !kind_ok(hdr_kind)) return (int)hipErrorInvalidValue;
    if (frag_len == 0 || frag_len > kHostMaxFrag) return (int)hipErrorInvalidValue;
    const size_t nfr = msg_len ? (msg_len - 1) / frag_len + 1 : 1;
    if (k_first > nfr || k_count > nfr - k_first) return (int)hipErrorInvalidValue;
    if (!h_fill || !h_ring || (msg_len && !h_msg)) return (int)hipErrorInvalidValue;
    const size_t hb = hdr_bytes_of(hdr_kind);
    const bool bare = hdr_kind == LAMPI_SEND_HDR_QUADRICS && slot_stride == 128;
    if (!bare && (slot_stride < hb || slot_stride - hb < frag_len)) return (int)hipErrorInvalidValue;
    if (k_count == 0) return 0;
    return (int)host_send_pack((const uint8_t *)h_msg, msg_len, frag_len, k_first, k_count, (uint8_t *)h_ring,
                               slot_stride, *h_fill, hdr_kind, mode);
}

int lampi_host_recv_unpack_batch(const void *h_ring, size_t ring_bytes, const lampi_host_recv_slot *h_slots, size_t n,
                                 int hdr_kind, int64_t *h_copied, uint32_t *h_csum, uint32_t *h_hdr_mask,
                                 uint32_t *h_data_mask, uint32_t *h_nbad, int mode) {
    if (!mode_ok(mode) || !kind_ok(hdr_kind)) return (int)hipErrorInvalidValue;
    if (!h_copied || !h_csum || !h_hdr_mask || !h_data_mask || !h_nbad || n > 0xFFFFFFFFull)
        return (int)hipErrorInvalidValue;
    if (n && (!h_ring || !h_slots)) return (int)hipErrorInvalidValue;
    const size_t hb = hdr_bytes_of(hdr_kind);
    for (size_t j = 0; j < n; ++j) {
        const lampi_host_recv_slot &x = h_slots[j];
        if (x.reserved || x.length > kHostMaxFrag) return (int)hipErrorInvalidValue;
        if (x.hdr_off > ring_bytes || hb > ring_bytes - x.hdr_off) return (int)hipErrorInvalidValue;
        if (to_copy(x) == 0) continue;  // its payload is never read: no constraint on frag_off / app
        if (!x.app) return (int)hipErrorInvalidValue;
        if (hdr_kind == LAMPI_SEND_HDR_QUADRICS && x.length <= kQInlineMax) continue;  // inside its header
        if (x.frag_off > ring_bytes || x.length > ring_bytes - x.frag_off) return (int)hipErrorInvalidValue;
    }
    if (n == 0) {
        h_nbad[0] = h_nbad[1] = 0;
        return 0;
    }
    if (mode == LAMPI_CSUM_NONE) {
        // Checksumming off: no header is read or tested, so the step is lampi_host_copy_to_app_batch's copy of the
        // lengthToCopy bytes (host_recv.cc), an inline Quadrics payload read from its envelope.
        std::vector<lampi_host_recv_frag> &fr = t_unpack.frags;
        fr.resize(n);
        for (size_t j = 0; j < n; ++j) {
            const lampi_host_recv_slot &x = h_slots[j];
            const bool inl = hdr_kind == LAMPI_SEND_HDR_QUADRICS && x.length <= kQInlineMax;
            fr[j] = lampi_host_recv_frag{inl ? x.hdr_off + kQPayloadOff : x.frag_off, x.app, x.app_len, x.length, 0u};
        }
        uint32_t nbad = 0;
        const int rc = lampi_host_copy_to_app_batch(h_ring, ring_bytes, fr.data(), n, h_copied, h_csum, h_data_mask,
                                                    &nbad, LAMPI_CSUM_NONE);
        if (rc) return rc;
        std::memset(h_hdr_mask, 0, (n + 31) / 32 * sizeof(uint32_t));
        h_nbad[0] = 0;
        h_nbad[1] = nbad;
        return 0;
    }
    return (int)host_recv_unpack((const uint8_t *)h_ring, ring_bytes, h_slots, n, hdr_kind, h_copied, h_csum,
                                 h_hdr_mask, h_data_mask, h_nbad, mode);
}

}  // extern "C"
