// host_tmap.cc -- the one-call send and receive steps for a non-contiguous datatype in host memory
// (lampi_host_tmap_send_pack, lampi_host_tmap_recv_unpack_batch; include/lampi_csum.h).
//
// The DMA engines gather and scatter, the kernels see packed bytes.  Both calls are the host one-call steps of
// host_pack.cc with their host side replaced (host_internal.h: SendSource, OutSink):
//
//   send    a chunk's packed window is staged into the device chunk in packed layout -- by the pieces route of
//           host_tmap_plan.h, or by its span route and the copy-only rows of the device typemap step
//           (launch_tmap_gather) --, then launch_msg_send_pack and the pitched D2H run as for a contiguous message;
//   receive the headers and payloads go up and are tested, the payloads are copied and checksummed into a packed
//           output chunk exactly as lampi_host_recv_unpack_batch does it for an application buffer in which packed
//           byte p has the address p; only the D2H differs: every run of passed fragments that are consecutive in
//           packed order goes down by the pieces route, the other way round.
//
// No kernel is new.  The CPU reads the caller's records and the typemap, and no ring or message byte.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/lampi_csum.h"
#include "frag_csum_kernels.h"
#include "host_internal.h"
#include "host_pack_items.h"
#include "host_pipe.h"
#include "host_tmap_plan.h"

namespace lampi {
namespace {

#define TRY LAMPI_TRY

size_t hdr_bytes_of(int kind) { return kind == LAMPI_SEND_HDR_QUADRICS ? 128 : 72; }
bool kind_ok(int kind) {
    return kind == LAMPI_SEND_HDR_GM || kind == LAMPI_SEND_HDR_IB || kind == LAMPI_SEND_HDR_QUADRICS;
}
bool mode_ok(int mode) { return mode == LAMPI_CSUM_CRC32 || mode == LAMPI_CSUM_SUM32 || mode == LAMPI_CSUM_NONE; }

// The typemap rules of both calls; *total = count * packed_size.
bool tmap_ok(const lampi_host_tmap *t, uint64_t *total) {
    if (!t || !t->h_pairs || t->num_pairs == 0 || t->packed_size == 0 || t->reserved) return false;
    const unsigned __int128 n = (unsigned __int128)t->count * t->packed_size;
    if (n >= ((unsigned __int128)1 << 63)) return false;
    *total = (uint64_t)n;
    return tmap_consistent(*t);
}

hipError_t issue(const std::vector<TmapXfer> &v, uint8_t *h_base, uint8_t *d, bool to_host, hipStream_t s) {
    for (const TmapXfer &t : v) {
        uint8_t *h = (uint8_t *)((uintptr_t)h_base + t.hoff);
        uint8_t *dd = d + t.doff;
        const hipMemcpyKind k = to_host ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice;
        if (t.rows == 1)
            TRY(to_host ? hipMemcpyAsync(h, dd, t.width, k, s) : hipMemcpyAsync(dd, h, t.width, k, s));
        else
            TRY(to_host ? hipMemcpy2DAsync(h, t.hpitch, dd, t.dpitch, t.width, t.rows, k, s)
                        : hipMemcpy2DAsync(dd, t.dpitch, h, t.hpitch, t.width, t.rows, k, s));
    }
    return hipSuccess;
}

// ---- send ---------------------------------------------------------------------------------------------

struct SendCtx {
    const TmapPlan *plan;
    uint8_t *h_base;
    uint64_t pack_off;  // the window's first packed byte: the step's message byte 0
    uint64_t span_cap;
    lampi_tmap dtm;     // the merged pairs on the device (the span route's gather)
    std::vector<TmapXfer> xf;
};

hipError_t send_in(void *c, uint64_t off, size_t nb, uint8_t *d, uint8_t *stage, hipStream_t s) {
    SendCtx &x = *(SendCtx *)c;
    const uint64_t p0 = x.pack_off + off;
    TmapSpan sp;
    if (x.plan->span(p0, p0 + nb, x.span_cap, sp))
        return hipMemcpyAsync(stage, (const uint8_t *)((uintptr_t)x.h_base + sp.lo), sp.bytes, hipMemcpyHostToDevice,
                              s);
    x.xf.clear();
    x.plan->pieces(p0, p0 + nb, 0, x.xf);
    return issue(x.xf, x.h_base, d, false, s);
}

hipError_t send_gather(void *c, uint64_t off, size_t nb, uint8_t *d, uint8_t *stage, hipStream_t s) {
    SendCtx &x = *(SendCtx *)c;
    const uint64_t p0 = x.pack_off + off;
    TmapSpan sp;
    if (!x.plan->span(p0, p0 + nb, x.span_cap, sp)) return hipSuccess;  // the pieces are in place
    // the staging area's first byte stands for h_base + sp.lo
    const uint8_t *base = (const uint8_t *)((uintptr_t)stage - sp.lo);
    return launch_tmap_gather(base, x.dtm, p0, nb, d, s);
}

hipError_t host_tmap_send(const uint8_t *h_base, const lampi_host_tmap &t, uint64_t pack_off, uint64_t pack_len,
                          size_t frag_len, uint8_t *h_ring, size_t stride, const lampi_send_hdr_fill &fill, int kind,
                          int mode) {
    const TmapPlan plan(t);
    const size_t fpc = std::max<size_t>(1, chunk_target(true) / frag_len);  // host_send_pack's fragments per chunk
    SendCtx x{&plan, const_cast<uint8_t *>(h_base), pack_off, 0, lampi_tmap{}, {}};
    x.span_cap = std::min<uint64_t>(plan.span_need((uint64_t)fpc * frag_len), plan.span_need(pack_len));
    SendSource src{&x, (size_t)x.span_cap, send_in, nullptr};
    if (x.span_cap) {
        // the merged pairs go up once, ahead of the first chunk (the pipeline's streams are idle between calls)
        PipeState *pp = nullptr;
        TRY(pipe_ctx(&pp));
        const std::vector<lampi_tmap_elt> &m = plan.merged();
        const size_t bytes = m.size() * sizeof(lampi_tmap_elt);
        TRY(ensure_meta(*pp, bytes));
        std::memcpy(pp->hmeta, m.data(), bytes);
        TRY(hipMemcpyAsync(pp->dmeta, pp->hmeta, bytes, hipMemcpyHostToDevice, pp->s_k));
        x.dtm = lampi_tmap{(const lampi_tmap_elt *)pp->dmeta, t.extent, t.packed_size, t.count, (uint32_t)m.size(), 0};
        src.gather = send_gather;
    }
    const size_t nfr = pack_len ? (size_t)((pack_len - 1) / frag_len + 1) : 1;
    return host_send_pack(nullptr, (size_t)pack_len, frag_len, 0, nfr, h_ring, stride, fill, kind, mode, &src);
}

// ---- receive ------------------------------------------------------------------------------------------

// The application buffer the receive step sees: packed byte p at kPackedBase + p.  Never dereferenced -- the
// planner compares and subtracts these addresses, the sink turns them back into packed offsets.
constexpr uintptr_t kPackedBase = (uintptr_t)1 << 62;

struct RecvCtx {
    const TmapPlan *plan;
    uint8_t *h_base;
    std::vector<TmapXfer> xf;
};

hipError_t recv_run(void *c, uint8_t *h, const uint8_t *d, size_t len, hipStream_t s) {
    RecvCtx &x = *(RecvCtx *)c;
    const uint64_t p0 = (uint64_t)((uintptr_t)h - kPackedBase);
    x.xf.clear();
    x.plan->pieces(p0, p0 + len, 0, x.xf);
    return issue(x.xf, x.h_base, const_cast<uint8_t *>(d), true, s);
}

struct TmapRecvScratch {
    std::vector<lampi_host_recv_slot> slots;
    std::vector<lampi_host_recv_frag> frags;
};
thread_local TmapRecvScratch t_scratch;

}  // namespace
}  // namespace lampi

using namespace lampi;

extern "C" {

int lampi_host_tmap_send_pack(const void *h_base, const lampi_host_tmap *h_tmap, uint64_t pack_off,
                              uint64_t pack_len, size_t frag_len, void *h_ring, size_t slot_stride,
                              const lampi_send_hdr_fill *h_fill, int hdr_kind, int mode) {
    if (!mode_ok(mode) || !kind_ok(hdr_kind)) return (int)hipErrorInvalidValue;
    if (frag_len == 0 || frag_len > kHostMaxFrag) return (int)hipErrorInvalidValue;
    if (!h_fill || !h_ring) return (int)hipErrorInvalidValue;
    const size_t hb = hdr_bytes_of(hdr_kind);
    const bool bare = hdr_kind == LAMPI_SEND_HDR_QUADRICS && slot_stride == 128;
    if (!bare && (slot_stride < hb || slot_stride - hb < frag_len)) return (int)hipErrorInvalidValue;
    uint64_t total = 0;
    if (!tmap_ok(h_tmap, &total)) return (int)hipErrorInvalidValue;
    if (pack_off > total || pack_len > total - pack_off) return (int)hipErrorInvalidValue;
    if (pack_len && (pack_len - 1) / frag_len + 1 > 0xFFFFFFFFull) return (int)hipErrorInvalidValue;
    return (int)host_tmap_send((const uint8_t *)h_base, *h_tmap, pack_off, pack_len, frag_len, (uint8_t *)h_ring,
                               slot_stride, *h_fill, hdr_kind, mode);
}

int lampi_host_tmap_recv_unpack_batch(const void *h_ring, size_t ring_bytes, const lampi_host_tmap_slot *h_slots,
                                      size_t n, int hdr_kind, void *h_base, const lampi_host_tmap *h_tmap,
                                      int64_t *h_copied, uint32_t *h_csum, uint32_t *h_hdr_mask,
                                      uint32_t *h_data_mask, uint32_t *h_nbad, int mode) {
    if (!mode_ok(mode) || !kind_ok(hdr_kind)) return (int)hipErrorInvalidValue;
    if (!h_copied || !h_csum || !h_hdr_mask || !h_data_mask || !h_nbad || n > 0xFFFFFFFFull)
        return (int)hipErrorInvalidValue;
    if (n && (!h_ring || !h_slots)) return (int)hipErrorInvalidValue;
    uint64_t total = 0;
    if (!tmap_ok(h_tmap, &total)) return (int)hipErrorInvalidValue;
    const size_t hb = hdr_bytes_of(hdr_kind);
    const bool quadrics = hdr_kind == LAMPI_SEND_HDR_QUADRICS;
    for (size_t j = 0; j < n; ++j) {
        const lampi_host_tmap_slot &x = h_slots[j];
        if (x.reserved || x.length > kHostMaxFrag) return (int)hipErrorInvalidValue;
        if (x.hdr_off > ring_bytes || hb > ring_bytes - x.hdr_off) return (int)hipErrorInvalidValue;
        if (x.pack_off >= total || x.length == 0) continue;  // nothing to copy: its payload is never read
        if (quadrics && x.length <= kQInlineMax) continue;   // inside its header
        if (x.frag_off > ring_bytes || x.length > ring_bytes - x.frag_off) return (int)hipErrorInvalidValue;
    }
    if (n == 0) {
        h_nbad[0] = h_nbad[1] = 0;
        return 0;
    }
    const TmapPlan plan(*h_tmap);
    RecvCtx ctx{&plan, (uint8_t *)h_base, {}};
    const OutSink sink{&ctx, recv_run};
    // the batch as the contiguous step takes it: app_len_i = total - pack_off_i (0 at or past the end)
    const auto app_of = [](uint64_t p) { return (void *)(kPackedBase + (uintptr_t)p); };
    const auto room_of = [&](uint64_t p) { return p >= total ? (int64_t)0 : (int64_t)(total - p); };
    if (mode == LAMPI_CSUM_NONE) {
        // checksumming off: no header is read; the copy of lampi_host_copy_to_app_batch (host_recv.cc), an inline
        // Quadrics payload read from its envelope
        std::vector<lampi_host_recv_frag> &fr = t_scratch.frags;
        fr.resize(n);
        for (size_t j = 0; j < n; ++j) {
            const lampi_host_tmap_slot &x = h_slots[j];
            const bool inl = quadrics && x.length <= kQInlineMax;
            fr[j] = lampi_host_recv_frag{inl ? x.hdr_off + kQPayloadOff : x.frag_off, app_of(x.pack_off),
                                         room_of(x.pack_off), x.length, 0u};
        }
        uint32_t nbad = 0;
        const hipError_t e = host_recv((const uint8_t *)h_ring, ring_bytes, fr.data(), n, h_copied, h_csum,
                                       h_data_mask, &nbad, LAMPI_CSUM_NONE, 0, &sink);
        if (e != hipSuccess) return (int)e;
        std::memset(h_hdr_mask, 0, (n + 31) / 32 * sizeof(uint32_t));
        h_nbad[0] = 0;
        h_nbad[1] = nbad;
        return 0;
    }
    std::vector<lampi_host_recv_slot> &sl = t_scratch.slots;
    sl.resize(n);
    for (size_t j = 0; j < n; ++j) {
        const lampi_host_tmap_slot &x = h_slots[j];
        sl[j] = lampi_host_recv_slot{x.hdr_off, x.frag_off, app_of(x.pack_off), room_of(x.pack_off), x.length, 0u};
    }
    return (int)host_recv_unpack((const uint8_t *)h_ring, ring_bytes, sl.data(), n, hdr_kind, h_copied, h_csum,
                                 h_hdr_mask, h_data_mask, h_nbad, mode, &sink);
}

}  // extern "C"
