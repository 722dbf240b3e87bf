// host_internal.h -- helpers shared by the C-ABI translation units of liblampi_csum.so (internal).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/lampi_csum.h"

namespace lampi {

// The calling thread's current device, range-checked against the per-device table slots.
hipError_t current_device(int *dev);
// The per-device table image (built once per process, uploaded once per device).
hipError_t device_tables(int dev, const uint32_t **out);
// Both: what a device entry point asks for once its arguments have passed (tables false: the device alone, for
// the entry points whose kernels read no table -- they must not start the upload).
struct DeviceCall {
    int dev;
    const uint32_t *img;
    hipError_t err;
};
DeviceCall device_call(bool tables = true);

// Pinned host memory held by the library's own staging (all threads), for leak checks
// (lampi_host_pinned_bytes).  Every hipHostMalloc of the host paths goes through these two.
hipError_t pinned_alloc(void **p, size_t bytes, unsigned flags);
void pinned_free(void *p, size_t bytes);

// The host-message pipeline's per-thread state (host_msg.cc), released with the rest of the
// thread's staging by lampi_host_release() and at thread exit.
void release_pipeline();

// The host one-call steps with their host side replaced (host_tmap.cc: a datatype's pieces in place of a contiguous
// message or of the records' application addresses).
// SendSource: where a chunk's message bytes [off, off + nb) come from.  `in` queues the H2D transfers on s_in --
// into the chunk d, or into the `extra` staging bytes behind every chunk (stage) --, and `gather`, when set, runs on
// s_k once they are done and before the pack.
struct SendSource {
    void *ctx;
    size_t extra;
    hipError_t (*in)(void *ctx, uint64_t off, size_t nb, uint8_t *d, uint8_t *stage, hipStream_t s_in);
    hipError_t (*gather)(void *ctx, uint64_t off, size_t nb, uint8_t *d, uint8_t *stage, hipStream_t s_k);
};
// OutSink: what becomes of a run of delivered bytes, d in the output chunk, that the records place at h.
struct OutSink {
    void *ctx;
    hipError_t (*run)(void *ctx, uint8_t *h, const uint8_t *d, size_t len, hipStream_t s_out);
};
// host_pack.cc (arguments already checked; src: h_msg is not read, sink: the records' app is only a key)
hipError_t host_send_pack(const uint8_t *h_msg, size_t msg_len, size_t frag_len, size_t k_first, size_t k_count,
                          uint8_t *h_ring, size_t stride, const lampi_send_hdr_fill &fill, int kind, int mode,
                          const SendSource *src = nullptr);
hipError_t host_recv_unpack(const uint8_t *h_ring, size_t ring_bytes, const lampi_host_recv_slot *f, size_t n,
                            int kind, int64_t *h_copied, uint32_t *h_csum, uint32_t *h_hmask, uint32_t *h_dmask,
                            uint32_t *h_nbad, int mode, const OutSink *sink = nullptr);
// host_recv.cc
hipError_t host_recv(const uint8_t *h_ring, size_t ring_bytes, const lampi_host_recv_frag *f, size_t n,
                     int64_t *h_copied, uint32_t *h_csum, uint32_t *h_mask, uint32_t *h_nbad, int mode,
                     uint32_t hint_override, const OutSink *sink = nullptr);

[[noreturn]] void die(const char *what, hipError_t e);

}  // namespace lampi
