// host_pack_items.h -- how the host receive step (host_pack.cc: lampi_host_recv_unpack_batch) presents a batch of
// lampi_host_recv_slot records to the DMA planner (host_plan.h).  Internal; host code only, so the CPU check of the
// plan (tests/native_host_pack/unpack_plan_check.cc) includes it as it is.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/lampi_csum.h"
#include "host_plan.h"

namespace lampi {

constexpr size_t kQInlineMax = 52, kQPayloadOff = 72;  // Quadrics: data[52] @72 of the 128-byte envelope

inline uint32_t to_copy(const lampi_host_recv_slot &x) {
    return x.app_len <= 0 ? 0u : (x.app_len < (int64_t)x.length ? (uint32_t)x.app_len : x.length);
}

// Where fragment j's payload is read from.
enum class Payload { kNone, kInHeader, kBehindHeader, kApart };

// The batch as the planner sees it, two items per fragment; a chunk may start only at a fragment's first item,
// which always has bytes (the planner passes over empty items before it looks for a chunk boundary):
//   2j     the header's 72 / 128 bytes -- with the payload when that starts where the header ends, so the pair is
//          one source range and slots at a constant pitch still make one 2D copy;
//   2j + 1 the delivery of lengthToCopy bytes, and the payload's own source range when it sits apart.
// A Quadrics payload of 1..52 bytes is part of its header.  (Checksumming off reads no header and does not come
// here: lampi_host_copy_to_app_batch's items, host_recv.cc.)
struct UnpackItems {
    const lampi_host_recv_slot *f;
    size_t n;
    size_t hb;  // header bytes of the kind
    bool quadrics;
    size_t size() const { return 2 * n; }
    // the item whose offset in the output chunk (and, for a payload apart, in the input chunk) is fragment j's
    size_t data_item(size_t j) const { return 2 * j + 1; }
    Payload where(const lampi_host_recv_slot &x) const {
        if (to_copy(x) == 0) return Payload::kNone;
        if (quadrics && x.length <= kQInlineMax) return Payload::kInHeader;
        return x.frag_off == x.hdr_off + hb ? Payload::kBehindHeader : Payload::kApart;
    }
    PlanItem get(size_t i) const {
        const lampi_host_recv_slot &x = f[i / 2];
        const Payload w = where(x);
        if (i % 2 == 0) return PlanItem{x.hdr_off, hb + (w == Payload::kBehindHeader ? x.length : 0u), nullptr, 0};
        if (w == Payload::kNone) return PlanItem{0, 0, nullptr, 0};
        const uint32_t c = to_copy(x);
        if (w == Payload::kApart) return PlanItem{x.frag_off, x.length, (uint8_t *)x.app, c};
        return PlanItem{0, 0, (uint8_t *)x.app, c};
    }
    bool boundary(size_t i) const { return i % 2 == 0; }
    // fragment j's payload in the input chunk, from the planner's input offsets (0 when nothing is read)
    size_t payload_at(size_t j, const size_t *din) const {
        const Payload w = where(f[j]);
        if (w == Payload::kNone) return 0;
        if (w == Payload::kApart) return din[2 * j + 1];
        return din[2 * j] + (w == Payload::kInHeader ? kQPayloadOff : hb);
    }
};

}  // namespace lampi
