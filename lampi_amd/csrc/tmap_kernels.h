// tmap_kernels.h -- the typemap forms of the one-call send and receive steps (lampi_tmap_send_pack,
// lampi_tmap_recv_unpack).  Part of frag_csum.hip's translation unit: included there once, inside namespace
// lampi, after the kernels and launchers it builds on (light_chunk and the light tables, crc_light_join_kernel,
// send_stamp_kernel, recv_hdr_test_kernel, zero_verdicts2, the stream's pooled buffers).
//
// The non-contiguous branch of gmSendFragDesc::init (ref src/path/gm/sendFrag.cc:157-217, ib/sendFrag.cc:140-203)
// packs typemap pieces into payloadp + len_copied and chains the checksum over them; non_contiguous_copy
// (src/path/common/BaseDesc.cc:72-163) reads src + len_copied.  One side is always contiguous and the chained
// checksum is the checksum of the packed bytes, so a fragment runs on crc_light_copy_kernel's shape: work items
// are (fragment, 4 KiB row of its packed bytes), one row per wave in 4-wave workgroups; lane l holds the 16-byte
// chunks at frame offsets 1024q + 16l of its row (q = 0..3), gathered through the typemap (send) or loaded from
// the slot (receive), stored once, and checksummed from those registers.
//
// Frames.  CRC: the fragment's L bytes are right-aligned in R = ceil(frag_len / 4096) rows (front padding
// P = 4096R - L of any byte count reads as zeros, free for a zero register); the register enters as data --
// CRC_INITIAL_REGISTER XORed into the fragment's first four bytes, or for a fragment under four bytes its
// image four bytes back, x^-32 * CRC_INITIAL_REGISTER, placed in the padding at P - 4 -- so an empty fragment's
// last row gives CRC_INITIAL_REGISTER itself.  SUM / NONE: left-aligned (P = 0), the chunks on the fragment's
// word grid and the bytes past L zero.  Either way a chunk cut by the fragment's start or end holds zeros there
// and moves only its bytes inside.
//
// Addresses.  Packed byte p of the message lives at base + (p / packed_size) * extent + pairs[i].offset +
// (r - pairs[i].seq_offset), r = p % packed_size, i the last pair with seq_offset <= r.  The wave divides once,
// for its row's first byte; a lane adds its chunk's distance (under 4,112 bytes: one conditional subtraction, or
// a 32-bit division for elements of at most 8 KiB) and finds the pair by binary search over seq_offset.  Typemaps
// of at most kTmapLdsPairs pairs are staged in LDS beside the tables (40,640 bytes with them: four workgroups per
// CU still fit); longer ones are read through L2.  A chunk wholly inside one piece moves as one 16-byte access;
// otherwise piece by piece in 8-, 4-, 2- and 1-byte accesses, never touching a byte outside the pieces.
//
// Descriptor forms (lampi_tmap_send_pack_batch, lampi_tmap_recv_unpack_batch).  The same rows with the fragment
// resolved from a record instead of from arithmetic on pack_off: the wave reads its lampi_tmap_frag and that
// record's lampi_tmap_msg as wave-uniform values, tests them (tmap_record: the host never saw the tables) and runs
// the frame, locate, tmap_move and checksum code above unchanged; R = max(1, ceil(max_len / 4096)) for every
// fragment of the call.  The four waves of a workgroup may name four messages, so the typemap is staged only when
// the workgroup's items share one message entry of at most kTmapLdsPairs pairs; otherwise it is read through L2 by
// the same TmapView -- no LDS added, four workgroups per CU as before.

namespace {

constexpr uint32_t kTmapLdsPairs = 64;

// x^-32 * r: the register four zero bytes before r (the polynomial's low bit is set, so a step's low bit tells
// whether it reduced)
constexpr uint32_t crc_back4(uint32_t r) {
    for (int k = 0; k < 32; ++k) {
        const uint32_t b = r & 1u;
        r = ((r ^ (b ? cx::kPoly : 0u)) >> 1) | (b << 31);
    }
    return r;
}
constexpr uint32_t kCrcInitBack4 = crc_back4(kCrcInit);
static_assert(cx::zero_byte(cx::zero_byte(cx::zero_byte(cx::zero_byte(kCrcInitBack4)))) == kCrcInit,
              "four zero bytes after crc_back4 give the register back");

typedef uint64_t u64_a1 __attribute__((aligned(1)));
typedef uint32_t u32_a1 __attribute__((aligned(1)));
typedef uint16_t u16_a1 __attribute__((aligned(1)));
typedef __attribute__((address_space(1))) const u64_a1 gu64_a1;
typedef __attribute__((address_space(1))) const u32_a1 gu32_a1;
typedef __attribute__((address_space(1))) const u16_a1 gu16_a1;
typedef __attribute__((address_space(1))) u64_a1 gwu64_a1;
typedef __attribute__((address_space(1))) u32_a1 gwu32_a1;
typedef __attribute__((address_space(1))) u16_a1 gwu16_a1;
typedef __attribute__((address_space(1))) const uint64_t gu64;

// A 16-byte chunk as two named 64-bit halves (byte k of the chunk = bits 8k.. of lo, 8(k - 8).. of hi): bytes go
// in and come out by shifts, no indexed registers.  v: zero-extended, at most 16 - k bytes.
__device__ __forceinline__ void chunk_put(uint64_t &lo, uint64_t &hi, uint32_t k, uint64_t v) {
    if (k < 8u) {
        lo |= v << (8u * k);
        if (k) hi |= v >> (64u - 8u * k);
    } else {
        hi |= v << (8u * (k - 8u));
    }
}
__device__ __forceinline__ uint64_t chunk_get(uint64_t lo, uint64_t hi, uint32_t k) {
    if (k < 8u) return k ? (lo >> (8u * k)) | (hi << (64u - 8u * k)) : lo;
    return hi >> (8u * (k - 8u));
}
__device__ __forceinline__ u32x4 chunk_words(uint64_t lo, uint64_t hi) {
    return u32x4{(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
}

// n <= 16 bytes at p <-> chunk bytes [k, k + n), the widest accesses n allows (any address)
__device__ __forceinline__ void span_load(gbyte *p, uint32_t k, uint32_t n, uint64_t &lo, uint64_t &hi) {
    while (n >= 8u) {
        chunk_put(lo, hi, k, *(gu64_a1 *)p);
        p += 8, k += 8u, n -= 8u;
    }
    if (n & 4u) {
        chunk_put(lo, hi, k, *(gu32_a1 *)p);
        p += 4, k += 4u;
    }
    if (n & 2u) {
        chunk_put(lo, hi, k, *(gu16_a1 *)p);
        p += 2, k += 2u;
    }
    if (n & 1u) chunk_put(lo, hi, k, *p);
}
__device__ __forceinline__ void span_store(gwbyte *p, uint32_t k, uint32_t n, uint64_t lo, uint64_t hi) {
    while (n >= 8u) {
        *(gwu64_a1 *)p = chunk_get(lo, hi, k);
        p += 8, k += 8u, n -= 8u;
    }
    if (n & 4u) {
        *(gwu32_a1 *)p = (uint32_t)chunk_get(lo, hi, k);
        p += 4, k += 4u;
    }
    if (n & 2u) {
        *(gwu16_a1 *)p = (uint16_t)chunk_get(lo, hi, k);
        p += 2, k += 2u;
    }
    if (n & 1u) *p = (uint8_t)chunk_get(lo, hi, k);
}

// Everything a row needs (a kernel argument).
struct TmapJob {
    const lampi_tmap_elt *pairs;  // device
    uint64_t extent, packed_size;
    uint32_t num_pairs;
    uint32_t R;       // rows of a fragment's frame
    uint8_t *base;    // the application buffer: read by the send step, written by the receive step
    uint8_t *ring;    // slot f = header at ring + f * slot_stride, payload at +72
    size_t slot_stride;
    size_t nitems;    // fragments x R
    uint64_t pack_off, pack_len;  // send: the window of packed bytes, fragment f = frag_len bytes from f * frag_len
    uint32_t frag_len;
    const RecvHdrRec *rec;        // receive: the header pre-pass's records
    uint64_t seq0, app_len;       //          dataSeqOffset of packed byte 0; count * packed_size
    const uint32_t *img;
    uint32_t *rows;   // row values: [f] when R == 1, else [f * R + r] for the join
    // the descriptor form: fragment f = frags[f] of the message msgs[frags[f].msg], whose typemap, base and
    // app_len replace the fields above; R rows from max_len; rec null with checksumming off (no header is tested)
    const lampi_tmap_frag *frags;
    const lampi_tmap_msg *msgs;
    uint32_t nmsgs, max_len;
};

// The descriptor form's record f with its message entry, tested before anything is computed from it (the tables
// are device memory the host never saw): false for msg >= nmsgs, length > max_len (the frame holds max_len bytes),
// an entry without pairs or with packed_size 0 (the rows divide by it) and, on send, a window past the message.
__device__ __forceinline__ bool tmap_record(const lampi_tmap_frag *__restrict__ frags,
                                            const lampi_tmap_msg *__restrict__ msgs, uint32_t nmsgs, uint32_t max_len,
                                            size_t f, bool send, lampi_tmap_frag &fr, lampi_tmap_msg &m) {
    fr = frags[f];
    if (fr.msg >= nmsgs || fr.length > max_len) return false;
    m = msgs[fr.msg];
    if (!m.d_pairs || m.num_pairs == 0u || m.packed_size == 0u) return false;
    if (send) {
        const uint64_t total = m.count * m.packed_size;
        if (fr.pack_off > total || fr.length > total - fr.pack_off) return false;
    }
    return true;
}

// The typemap's fields (k = 0 size, 1 offset, 2 seq_offset of pair i), from LDS when staged
struct TmapView {
    gu64 *g;
    const uint64_t *l;
    bool staged;
    __device__ __forceinline__ uint64_t at(uint32_t i, uint32_t k) const {
        return staged ? l[3u * i + k] : g[3u * (size_t)i + k];
    }
};

// Chunk bytes [k0, k1) <-> the typemap side, from byte r (< packed_size) of element e on.  kStore: the chunk's
// bytes are scattered (receive); otherwise gathered into lo / hi (send), which enter as zeros.
template <bool kStore>
__device__ __forceinline__ void tmap_move(const TmapJob &J, const TmapView &tm, uint64_t e, uint64_t r, uint32_t k0,
                                          uint32_t k1, uint64_t &lo, uint64_t &hi) {
    uint32_t i = 0;
    if (J.num_pairs > 1u) {  // the last pair with seq_offset <= r
        uint32_t a = 0, b = J.num_pairs;
        while (b - a > 1u) {
            const uint32_t m = a + (b - a) / 2u;
            if (tm.at(m, 2u) <= r) a = m;
            else b = m;
        }
        i = a;
    }
    const uint64_t within = r - (J.num_pairs > 1u ? tm.at(i, 2u) : 0u);
    uint64_t avail = tm.at(i, 0u) - within;
    uint64_t eb = (uint64_t)(uintptr_t)J.base + e * J.extent;  // (mod 2^64: offsets may be negative)
    uint64_t addr = eb + tm.at(i, 1u) + within;
    if (k0 == 0u && k1 == 16u && avail >= 16u) {  // wholly inside one piece: one 16-byte access
        if constexpr (kStore) {
            st16u((gwu32x4_a1 *)(uintptr_t)addr, chunk_words(lo, hi));
        } else {
            const u32x4 v = ld16u((gu32x4_a1 *)(uintptr_t)addr);
            lo = v.x | ((uint64_t)v.y << 32);
            hi = v.z | ((uint64_t)v.w << 32);
        }
        return;
    }
    uint32_t k = k0;
    for (;;) {
        const uint32_t n = (uint32_t)min(avail, (uint64_t)(k1 - k));
        if constexpr (kStore) span_store((gwbyte *)(uintptr_t)addr, k, n, lo, hi);
        else span_load((gbyte *)(uintptr_t)addr, k, n, lo, hi);
        k += n;
        if (k >= k1) break;
        if (++i == J.num_pairs) {  // the next element
            i = 0;
            eb += J.extent;
        }
        avail = tm.at(i, 0u);
        addr = eb + tm.at(i, 1u);
    }
}

// One (fragment, row) per wave: item = item0 + 4 * blockIdx.x + wave.  kMode: lampi_csum_mode; kRecv: the receive
// step (slot -> typemap) instead of the send step (typemap -> slot).  kDesc: the descriptor form -- the wave's
// fragment, typemap and base come from its record and that record's message entry (wave-uniform loads), tested by
// tmap_record first; an invalid record's rows run as a dropped fragment's (nothing read, nothing written, row
// value 0).  The typemap is staged in LDS when every item of the workgroup names the same message entry and that
// has at most kTmapLdsPairs pairs; a workgroup whose waves name different messages reads them through L2 (no LDS
// added: four workgroups per CU as before).
template <int kMode, bool kRecv, bool kDesc = false>
__global__ void __launch_bounds__(256) tmap_row_kernel(const TmapJob Ja, size_t item0) {
    constexpr bool kCrc = kMode == LAMPI_CSUM_CRC32, kSum = kMode == LAMPI_CSUM_SUM32;
    __shared__ __attribute__((aligned(16))) uint32_t lds[kCrc ? kLtBytes / 4 : 4];
    __shared__ uint64_t tml[3 * kTmapLdsPairs];
    TmapJob J = Ja;
    const uint32_t t = threadIdx.x, lane = t & 63u;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(t >> 6);
    const size_t item = item0 + (size_t)blockIdx.x * 4 + wv;
    const bool in = item < J.nitems;
    size_t f = 0;
    uint32_t r = 0;
    bool ok = true;          // (descriptor form: the record is valid)
    bool stage_desc = false; //  ... and the workgroup's items share one typemap that fits the LDS
    lampi_tmap_frag fr{};
    if constexpr (!kDesc) {
        f = in ? item / J.R : 0;
        r = in ? (uint32_t)(item - f * J.R) : 0u;
    } else {
        // the workgroup's first item is always inside; the others' fragments follow from it without dividing again
        const size_t wg0 = item0 + (size_t)blockIdx.x * 4;
        const size_t f0 = wg0 / J.R;
        const uint32_t r0 = (uint32_t)(wg0 - f0 * J.R);
        const uint32_t m0 = J.frags[f0].msg;
        bool same = m0 < J.nmsgs;
        for (uint32_t w = 1; w < 4u; ++w) {
            size_t fw = f0;
            uint32_t rw = r0 + w;
            while (rw >= J.R) rw -= J.R, ++fw;
            if (wg0 + w < J.nitems && J.frags[fw].msg != m0) same = false;
            if (w == wv) f = fw, r = rw;
        }
        if (wv == 0u) f = f0, r = r0;
        if (!in) f = 0, r = 0u;
        J.pairs = nullptr;
        J.num_pairs = 0u;
        J.packed_size = J.extent = 0u;
        J.base = nullptr;
        J.app_len = 0u;
        if (same) {  // (workgroup-uniform: every wave read the same records)
            const lampi_tmap_msg &e0 = J.msgs[m0];
            const lampi_tmap_elt *p0 = e0.d_pairs;
            const uint32_t np0 = e0.num_pairs;
            if (p0 && np0 >= 1u && np0 <= kTmapLdsPairs) {
                stage_desc = true;
                if (t < 3u * np0) tml[t] = ((gu64 *)(uintptr_t)p0)[t];
            }
        }
        lampi_tmap_msg m{};
        ok = in && tmap_record(J.frags, J.msgs, J.nmsgs, J.max_len, f, !kRecv, fr, m);
        if (ok) {
            J.pairs = m.d_pairs;
            J.num_pairs = m.num_pairs;
            J.packed_size = m.packed_size;
            J.extent = m.extent;
            J.base = (uint8_t *)(uintptr_t)m.base;
            J.app_len = m.count * m.packed_size;
        }
    }
    // the tables' image loads first, as crc_light_copy_kernel
    constexpr uint32_t kNibPieces = kLightTables * kLightTableWords / 4;
    const uint32_t t2 = min(256u + t, kNibPieces - 1);
    u32x4 nib{}, nib2{}, bs[4]{};
    if constexpr (kCrc) {
        nib = reinterpret_cast<const u32x4 *>(J.img + kImgLightNib)[min(t, kNibPieces - 1)];
        nib2 = reinterpret_cast<const u32x4 *>(J.img + kImgLightNib)[t2];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            bs[i] = reinterpret_cast<const u32x4 *>(J.img + kImgSliceBasis)[((t & 7u) >> 1) * 4 + i];
    }
    // the fragment (wave-uniform): L bytes checksummed, the first ncopy of them moved, packed byte p0 its first
    uint8_t *slot = kDesc ? nullptr : J.ring + f * J.slot_stride;
    uint64_t p0 = 0;
    uint32_t L = 0, ncopy = 0;
    if constexpr (kDesc) {
        if (ok) {
            p0 = fr.pack_off;
            if constexpr (!kRecv) {
                L = ncopy = fr.length;
            } else {  // CopyToApp's rules, the length from the record
                const bool pass = !J.rec || J.rec[f].ok != 0u;
                const uint64_t room = p0 >= J.app_len ? 0u : J.app_len - p0;
                ncopy = pass ? (uint32_t)min((uint64_t)fr.length, room) : 0u;
                L = kMode == LAMPI_CSUM_NONE ? ncopy : (ncopy ? fr.length : 0u);
            }
        }
    } else if (in) {
        if constexpr (!kRecv) {
            const uint64_t off = (uint64_t)f * J.frag_len;
            const uint64_t rem = J.pack_len > off ? J.pack_len - off : 0u;
            L = (uint32_t)min(rem, (uint64_t)J.frag_len);
            ncopy = L;
            p0 = J.pack_off + off;
        } else {  // MsgRecvSource::get's rules
            const RecvHdrRec rc = J.rec[f];
            const uint32_t len = *(guint *)(slot + 4 * kRecvLenWord);
            const uint32_t so_lo = *(guint *)(slot + 4 * kRecvSeqOffWord);
            const uint32_t so_hi = *(guint *)(slot + 4 * kRecvSeqOffWord + 4);
            const uint64_t off = (((uint64_t)so_hi << 32) | so_lo) - J.seq0;
            const uint64_t room = off >= J.app_len ? 0u : J.app_len - off;
            ncopy = rc.ok ? (uint32_t)min((uint64_t)len, room) : 0u;
            L = kMode == LAMPI_CSUM_NONE ? ncopy : (ncopy ? len : 0u);
            p0 = off;
        }
    }
    uint8_t *payload = kDesc ? (uint8_t *)(uintptr_t)fr.payload : slot + kSendHdrBytes;
    const bool staged = kDesc ? stage_desc : J.num_pairs <= kTmapLdsPairs;
    if (staged) {
        if constexpr (!kDesc)
            if (t < 3u * J.num_pairs) tml[t] = ((gu64 *)(uintptr_t)J.pairs)[t];
        __syncthreads();
    }
    const TmapView tm{(gu64 *)(uintptr_t)J.pairs, tml, staged};
    // the row's bytes in frame coordinates: the fragment is [P, P + L), this row [fs, fs + 4096)
    const uint64_t P = kCrc ? (uint64_t)J.R * kRowBytes - L : 0u;
    const uint64_t fs = (uint64_t)r * kRowBytes;
    const uint64_t fa = max(fs, P), fb = min(fs + kRowBytes, P + L);
    const bool live = in && fb > fa;
    // (send, CRC: an empty fragment's last row still runs -- the register's image in its padding is the value)
    const bool run = live || (kCrc && !kRecv && in && ok && L == 0u && r == J.R - 1u);
    uint64_t e0 = 0, r0 = 0;  // element and byte in it of the row's first byte
    if (live) {
        const uint64_t ps = p0 + (fa - P);
        e0 = ps / J.packed_size;
        r0 = ps - e0 * J.packed_size;
    }
    // element and byte in it of the fragment byte d (< 4,112) bytes after the row's first
    auto locate = [&](uint64_t d, uint64_t &e, uint64_t &rr) {
        e = e0;
        rr = r0 + d;
        if (rr >= J.packed_size) {
            if (J.packed_size > 8192u) {
                rr -= J.packed_size;
                ++e;
            } else {
                const uint32_t q = (uint32_t)rr / (uint32_t)J.packed_size;
                e += q;
                rr -= (uint64_t)q * J.packed_size;
            }
        }
    };
    uint64_t lo[4], hi[4];
    uint32_t k0[4], k1[4];  // the chunk's bytes inside the fragment
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        lo[q] = hi[q] = 0u;
        const uint64_t x = fs + 1024u * q + 16u * lane;
        const uint64_t va = max(x, fa), vb = min(x + 16u, fb);
        const bool any = live && vb > va;
        k0[q] = any ? (uint32_t)(va - x) : 0u;
        k1[q] = any ? (uint32_t)(vb - x) : 0u;
        if (!any) continue;
        if constexpr (kRecv) {
            gbyte *p = (gbyte *)(payload + (va - P));
            if (k0[q] == 0u && k1[q] == 16u) {
                const u32x4 v = ld16u((gu32x4_a1 *)p);
                lo[q] = v.x | ((uint64_t)v.y << 32);
                hi[q] = v.z | ((uint64_t)v.w << 32);
            } else {
                span_load(p, k0[q], k1[q] - k0[q], lo[q], hi[q]);
            }
        } else {
            uint64_t e, rr;
            locate(va - fa, e, rr);
            tmap_move<false>(J, tm, e, rr, k0[q], k1[q], lo[q], hi[q]);
        }
    }
    if constexpr (kCrc) {  // the tables, while the row's loads fly
        build_slices_light<256>(reinterpret_cast<char *>(lds), bs);
        reinterpret_cast<u32x4 *>(reinterpret_cast<char *>(lds) + kLtNib)[min(t, kNibPieces - 1)] = nib;
        reinterpret_cast<u32x4 *>(reinterpret_cast<char *>(lds) + kLtNib)[t2] = nib2;
        __syncthreads();
    }
    uint32_t *out = J.rows + (J.R == 1u ? f : item);
    if (!run) {  // a row of padding, an empty or dropped fragment: nothing to add
        if (kMode != LAMPI_CSUM_NONE && in && lane == 63u) *out = 0u;
        return;
    }
    // each byte stored once
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (k1[q] <= k0[q]) continue;
        const uint64_t x = fs + 1024u * q + 16u * lane;
        if constexpr (kRecv) {
            const uint64_t end = min(x + k1[q], P + ncopy);  // (truncation: nothing past the posted elements)
            if (end <= x + k0[q]) continue;
            uint64_t e, rr;
            locate(x + k0[q] - fa, e, rr);
            uint64_t a = lo[q], b = hi[q];
            tmap_move<true>(J, tm, e, rr, k0[q], (uint32_t)(end - x), a, b);
        } else {
            gwbyte *p = (gwbyte *)(payload + (x + k0[q] - P));
            if (k0[q] == 0u && k1[q] == 16u) st16u((gwu32x4_a1 *)p, chunk_words(lo[q], hi[q]));
            else span_store(p, k0[q], k1[q] - k0[q], lo[q], hi[q]);
        }
    }
    if constexpr (kSum) {
        uint32_t sm = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            sm += (uint32_t)lo[q] + (uint32_t)(lo[q] >> 32) + (uint32_t)hi[q] + (uint32_t)(hi[q] >> 32);
        sm = wave_add(sm);
        if (lane == 63u) *out = sm;
    }
    if constexpr (kCrc) {
        // the register as data: four bytes at frame offset Q, their first the register's top byte
        const bool tiny = L < 4u;
        const uint64_t Q = tiny ? P - 4u : P;
        const uint64_t V = __builtin_bswap32(tiny ? kCrcInitBack4 : kCrcInit);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t dl = (int64_t)(Q - (fs + 1024u * q + 16u * lane));
            if (dl >= 16 || dl <= -4) continue;
            if (dl < 0) {
                lo[q] ^= V >> (8u * (uint32_t)(-dl));
            } else if (dl < 8) {
                lo[q] ^= V << (8u * (uint32_t)dl);
                if (dl > 4) hi[q] ^= V >> (64u - 8u * (uint32_t)dl);
            } else {
                hi[q] ^= V << (8u * (uint32_t)(dl - 8));
            }
        }
        // crc_light_copy_kernel's row: four chunks from a zero register, Horner over the 1024-byte step, lane tree
        const uint32_t c8 = (lane & 7u) * 8u;
        const uint32_t lanec2 = c8 | ((c8 + 64u) << 8) | ((c8 + 128u) << 16) | ((c8 + 192u) << 24);
        const uint32_t g = (lane >> 3) & 3u;
        uint32_t sel[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t j = (uint32_t)q ^ g;
            sel[q] = j | ((4u + j) << 8) | 0x0C0C0000u;
        }
        const uint32_t c0 = light_chunk(lds, lanec2, sel, chunk_words(lo[0], hi[0]));
        const uint32_t c1 = light_chunk(lds, lanec2, sel, chunk_words(lo[1], hi[1]));
        const uint32_t c2 = light_chunk(lds, lanec2, sel, chunk_words(lo[2], hi[2]));
        const uint32_t c3 = light_chunk(lds, lanec2, sel, chunk_words(lo[3], hi[3]));
        uint32_t v = light_shift<0>(lds, light_shift<0>(lds, light_shift<0>(lds, c0) ^ c1) ^ c2) ^ c3;
        v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)light_shift<1>(lds, v), 0x111, 0xF, 0xF, false);  // row_shr:1
        v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)light_shift<2>(lds, v), 0x112, 0xF, 0xF, false);  // row_shr:2
        v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)light_shift<3>(lds, v), 0x114, 0xF, 0xF, false);  // row_shr:4
        const uint32_t grp = lane >> 3;
        if (grp < 7u) v = light_shift_at(lds, kLtNib + kLtTab * (4u + grp), v);
        v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false);  // row_shr:8
        v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);  // row_bcast:15
        v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);  // row_bcast:31
        if (lane == 63u) *out = __builtin_bswap32(v);
    }
}

// out[f] = the sum of fragment f's R row sums (R > 1): a thread per fragment up to kJoinThreadRows rows, a wave above
__global__ void __launch_bounds__(256) tmap_sum_join_kernel(const uint32_t *__restrict__ rows, size_t n, uint32_t R,
                                                            uint32_t *__restrict__ out) {
    if (R <= kJoinThreadRows) {
        const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
        if (f >= n) return;
        uint32_t acc = 0;
        for (uint32_t r = 0; r < R; ++r) acc += rows[f * R + r];
        out[f] = acc;
        return;
    }
    const size_t f = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= n) return;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t acc = 0;
    for (uint32_t r = lane; r < R; r += 64) acc += rows[f * R + r];
    acc = wave_add(acc);
    if (lane == 0) out[f] = acc;
}

// The receive step's verdicts, one thread per slot after the rows (and their join): RecvHdrBase::verdict's
// outputs and emit's d_csum (0 for a dropped fragment or with checksumming off, the empty value when nothing was
// delivered).  The masks and counts were zeroed by zero_verdicts2.
__global__ void __launch_bounds__(256) tmap_recv_verdict_kernel(const uint8_t *__restrict__ ring, size_t stride,
                                                                uint32_t n, const RecvHdrRec *__restrict__ rec,
                                                                const uint32_t *__restrict__ vals, uint64_t seq0,
                                                                uint64_t app_len, int mode, int64_t *copied,
                                                                uint32_t *csum, uint32_t *hmask, uint32_t *dmask,
                                                                uint32_t *nbad) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const RecvHdrRec rc = rec[i];
    if (!rc.ok) {
        copied[i] = (int64_t)LAMPI_RECV_HDR_BAD;
        csum[i] = 0u;
        atomicOr(hmask + (i >> 5), 1u << (i & 31u));
        atomicAdd(nbad, 1u);
        return;
    }
    const uint8_t *h = ring + (size_t)i * stride;
    const uint32_t len = *(guint *)(h + 4 * kRecvLenWord);
    const uint64_t so = ((uint64_t) * (guint *)(h + 4 * kRecvSeqOffWord + 4) << 32) | *(guint *)(h + 4 * kRecvSeqOffWord);
    const uint64_t off = so - seq0;
    const uint64_t room = off >= app_len ? 0u : app_len - off;
    const uint32_t c = (uint32_t)min((uint64_t)len, room);
    const bool none = mode == LAMPI_CSUM_NONE;
    const uint32_t v = none ? 0u : c ? vals[i] : mode == LAMPI_CSUM_CRC32 ? kCrcInit : 0u;
    const bool bad = !none && c != 0u && v != rc.expected;
    csum[i] = v;
    copied[i] = bad ? (int64_t)LAMPI_RECV_DATA_BAD : (int64_t)c;
    if (bad) {
        atomicOr(dmask + (i >> 5), 1u << (i & 31u));
        atomicAdd(nbad + 1, 1u);
    }
}

// tmap_row_kernel over n fragments of R rows, then the join of their rows into vals (R > 1).  Launches of at most
// 2^24 - 1 workgroups (a grid has under 2^32 threads).
template <bool kRecv, bool kDesc = false>
hipError_t launch_tmap_rows(TmapJob J, size_t n, uint32_t *vals, int mode, hipStream_t s) {
    const bool none = mode == LAMPI_CSUM_NONE;
    uint32_t *rows = nullptr;
    J.nitems = n * J.R;
    J.rows = vals;
    if (!none && J.R > 1u) {
        const hipError_t e = stream_scratch(s, J.nitems * sizeof(uint32_t), (void **)&rows);
        if (e != hipSuccess) return e;
        J.rows = rows;
    }
    constexpr size_t kMaxItems = 4 * (((size_t)1 << 24) - 1);
    for (size_t item0 = 0; item0 < J.nitems; item0 += kMaxItems) {
        const dim3 grid((unsigned)((std::min(J.nitems - item0, kMaxItems) + 3) / 4));
        if (mode == LAMPI_CSUM_CRC32)
            hipLaunchKernelGGL((tmap_row_kernel<LAMPI_CSUM_CRC32, kRecv, kDesc>), grid, dim3(256), 0, s, J, item0);
        else if (mode == LAMPI_CSUM_SUM32)
            hipLaunchKernelGGL((tmap_row_kernel<LAMPI_CSUM_SUM32, kRecv, kDesc>), grid, dim3(256), 0, s, J, item0);
        else
            hipLaunchKernelGGL((tmap_row_kernel<LAMPI_CSUM_NONE, kRecv, kDesc>), grid, dim3(256), 0, s, J, item0);
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && rows) {
        const size_t per_wg = J.R <= kJoinThreadRows ? 256 : 4;  // fragments per workgroup
        const dim3 grid((unsigned)((n + per_wg - 1) / per_wg));
        if (mode == LAMPI_CSUM_CRC32)
            hipLaunchKernelGGL(crc_light_join_kernel, grid, dim3(256), 0, s, rows, n, J.R, vals);
        else
            hipLaunchKernelGGL(tmap_sum_join_kernel, grid, dim3(256), 0, s, rows, n, J.R, vals);
        e = hipGetLastError();
    }
    return e;
}

// The descriptor form's stamp: send_stamp_kernel<false>'s route (the prefix read from the header, on the LDS
// slice tables) with fragment i's emptiness taken from its record; an invalid record's header stays as it is.
__global__ void __launch_bounds__(256) tmap_send_stamp_kernel(uint8_t *hdrs, size_t stride, uint32_t n,
                                                              const uint32_t *__restrict__ vals,
                                                              const lampi_tmap_frag *__restrict__ frags,
                                                              const lampi_tmap_msg *__restrict__ msgs, uint32_t nmsgs,
                                                              uint32_t max_len, int kind, int mode,
                                                              const uint32_t *__restrict__ img) {
    __shared__ uint32_t S[1024];
    if (mode == LAMPI_CSUM_CRC32) stage_slices(S, img);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    lampi_tmap_frag fr;
    lampi_tmap_msg m;
    if (!tmap_record(frags, msgs, nmsgs, max_len, i, true, fr, m)) return;
    uint8_t *h = hdrs + (size_t)i * stride;
    if (mode == LAMPI_CSUM_NONE) {
        send_stamp(h, 0u, true, kind, mode, 0u);
        return;
    }
    send_stamp(h, vals[i], fr.length == 0u, kind, mode, send_hdr_prefix(h, mode, SliceLds{S}));
}

// The descriptor form's verdicts: tmap_recv_verdict_kernel with pack_off, length and the message from the
// records; an invalid record is a dropped fragment in every mode (rec null: checksumming off, every header passes).
__global__ void __launch_bounds__(256) tmap_batch_verdict_kernel(const lampi_tmap_frag *__restrict__ frags, uint32_t n,
                                                                 const lampi_tmap_msg *__restrict__ msgs,
                                                                 uint32_t nmsgs, uint32_t max_len,
                                                                 const RecvHdrRec *__restrict__ rec,
                                                                 const uint32_t *__restrict__ vals, int mode,
                                                                 int64_t *copied, uint32_t *csum, uint32_t *hmask,
                                                                 uint32_t *dmask, uint32_t *nbad) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    lampi_tmap_frag fr;
    lampi_tmap_msg m;
    const bool valid = tmap_record(frags, msgs, nmsgs, max_len, i, false, fr, m);
    RecvHdrRec rc{1u, 0u};
    if (rec) rc = rec[i];
    if (!valid || !rc.ok) {
        copied[i] = (int64_t)LAMPI_RECV_HDR_BAD;
        csum[i] = 0u;
        atomicOr(hmask + (i >> 5), 1u << (i & 31u));
        atomicAdd(nbad, 1u);
        return;
    }
    const uint64_t app_len = m.count * m.packed_size;
    const uint64_t room = fr.pack_off >= app_len ? 0u : app_len - fr.pack_off;
    const uint32_t c = (uint32_t)min((uint64_t)fr.length, room);
    const bool none = mode == LAMPI_CSUM_NONE;
    const uint32_t v = none ? 0u : c ? vals[i] : mode == LAMPI_CSUM_CRC32 ? kCrcInit : 0u;
    const bool bad = !none && c != 0u && v != rc.expected;
    csum[i] = v;
    copied[i] = bad ? (int64_t)LAMPI_RECV_DATA_BAD : (int64_t)c;
    if (bad) {
        atomicOr(dmask + (i >> 5), 1u << (i & 31u));
        atomicAdd(nbad + 1, 1u);
    }
}

// The descriptor form's job: no ring, no single typemap -- the records and the message table, R from max_len
TmapJob tmap_batch_job(const lampi_tmap_frag *frags, const lampi_tmap_msg *msgs, size_t nmsgs, uint32_t max_len,
                       const uint32_t *img) {
    TmapJob J{};
    J.R = (uint32_t)std::max<size_t>(1, ((size_t)max_len + kRowBytes - 1) / kRowBytes);
    J.frags = frags;
    J.msgs = msgs;
    J.nmsgs = (uint32_t)nmsgs;
    J.max_len = max_len;
    J.img = img;
    return J;
}

TmapJob tmap_job(const lampi_tmap &tm, uint8_t *base, uint8_t *ring, size_t slot_stride, size_t payload_room,
                 const uint32_t *img) {
    TmapJob J{};
    J.pairs = tm.d_pairs;
    J.extent = tm.extent;
    J.packed_size = tm.packed_size;
    J.num_pairs = tm.num_pairs;
    J.R = (uint32_t)std::max<size_t>(1, (payload_room + kRowBytes - 1) / kRowBytes);
    J.base = base;
    J.ring = ring;
    J.slot_stride = slot_stride;
    J.img = img;
    return J;
}

}  // namespace

// The send step through a typemap (lampi_tmap_send_pack): the rows gather fragment j's packed bytes into slot j
// with their checksums in the stream's pooled values, then send_stamp_kernel<true> builds and stamps the headers
// as lampi_msg_send_pack's (msg_len = pack_len).  kind: GM or IB.
hipError_t launch_tmap_send_pack(const uint8_t *base, const lampi_tmap &tm, uint64_t pack_off, uint64_t pack_len,
                                 size_t frag_len, uint8_t *ring, size_t slot_stride, const lampi_send_hdr_fill &fill,
                                 size_t n, int kind, int mode, const uint32_t *img, hipStream_t s) {
    if (n == 0) return hipSuccess;
    if (!img) return hipErrorInvalidValue;
    const SendFill f = send_fill(fill);
    uint32_t *vals = nullptr;
    hipError_t e = stream_vals(s, n, &vals);
    if (e != hipSuccess) return e;
    if (!(mode == LAMPI_CSUM_NONE && pack_len == 0)) {  // (nothing to copy, no checksum)
        TmapJob J = tmap_job(tm, const_cast<uint8_t *>(base), ring, slot_stride, frag_len, img);
        J.pack_off = pack_off;
        J.pack_len = pack_len;
        J.frag_len = (uint32_t)frag_len;
        e = launch_tmap_rows<false>(J, n, vals, mode, s);
    }
    if (e == hipSuccess)
        e = launch_per_item(send_stamp_kernel<true>, n, s, ring, slot_stride, (uint32_t)n, (const uint32_t *)vals,
                            (const lampi_copy_desc *)nullptr, f, (size_t)pack_len, frag_len, kind, mode, img);
    return e;
}

// Packed bytes [pack_off, pack_off + pack_len) gathered to dst, nothing else: the copy-only rows of the send step
// over one-row fragments 4096 bytes apart (no header is written, no value kept).  For the host typemap form's span
// route (host_tmap.cc), whose base is a staged copy of the elements' footprints.
hipError_t launch_tmap_gather(const uint8_t *base, const lampi_tmap &tm, uint64_t pack_off, uint64_t pack_len,
                              uint8_t *dst, hipStream_t s) {
    if (pack_len == 0) return hipSuccess;
    TmapJob J = tmap_job(tm, const_cast<uint8_t *>(base), dst - kSendHdrBytes, kRowBytes, kRowBytes, nullptr);
    J.pack_off = pack_off;
    J.pack_len = pack_len;
    J.frag_len = (uint32_t)kRowBytes;
    return launch_tmap_rows<false>(J, (size_t)((pack_len + kRowBytes - 1) / kRowBytes), nullptr, LAMPI_CSUM_NONE, s);
}

// The receive step through a typemap (lampi_tmap_recv_unpack): the verdicts zeroed, recv_hdr_test_kernel over the
// slots (max_len = slot_stride - 72; in every mode -- it tests the length), the rows of the slots that passed --
// scattered through the typemap, cut at app_len = count * packed_size --, their join, and one verdict launch.
hipError_t launch_tmap_recv_unpack(const uint8_t *ring, size_t nslots, size_t slot_stride, int kind, uint8_t *base,
                                   const lampi_tmap &tm, uint64_t seq0, int64_t *copied, uint32_t *csum,
                                   uint32_t *hmask, uint32_t *dmask, uint32_t *nbad, int mode, const uint32_t *img,
                                   hipStream_t s) {
    if (nslots == 0) return hipMemsetAsync(nbad, 0, 2 * sizeof(uint32_t), s);
    if (!img) return hipErrorInvalidValue;
    hipError_t e = zero_verdicts2(hmask, dmask, nslots, nbad, s);
    if (e != hipSuccess) return e;
    uint32_t *buf = nullptr;  // the records (two words a slot), then the fragments' values
    e = stream_vals(s, 3 * nslots, &buf);
    if (e != hipSuccess) return e;
    RecvHdrRec *rec = (RecvHdrRec *)buf;
    uint32_t *vals = buf + 2 * nslots;
    const size_t room = std::min<size_t>(slot_stride - kSendHdrBytes, 0xFFFFFFFEull);
    e = launch_per_item(recv_hdr_test_kernel, nslots, s, ring, slot_stride, (uint32_t)nslots, kind, mode, (uint32_t)room,
                        img, rec);
    if (e == hipSuccess) {
        TmapJob J = tmap_job(tm, base, const_cast<uint8_t *>(ring), slot_stride, room, img);
        J.rec = rec;
        J.seq0 = seq0;
        J.app_len = tm.count * tm.packed_size;
        e = launch_tmap_rows<true>(J, nslots, vals, mode, s);
        if (e == hipSuccess)
            e = launch_per_item(tmap_recv_verdict_kernel, nslots, s, ring, slot_stride, (uint32_t)nslots,
                                (const RecvHdrRec *)rec, (const uint32_t *)vals, seq0, J.app_len, mode, copied, csum,
                                hmask, dmask, nbad);
    }
    return e;
}

// The send step over fragment records (lampi_tmap_send_pack_batch): the rows of every record gather its window
// through its own message's typemap, then tmap_send_stamp_kernel stamps the headers the caller prefilled (GM with
// checksumming off writes no header word: no stamp launch, hdrs may be null).
hipError_t launch_tmap_send_pack_batch(const lampi_tmap_frag *frags, size_t n, const lampi_tmap_msg *msgs, size_t nmsgs,
                                       uint32_t max_len, uint8_t *hdrs, size_t hdr_stride, int kind, int mode,
                                       const uint32_t *img, hipStream_t s) {
    if (n == 0) return hipSuccess;
    if (!img) return hipErrorInvalidValue;
    uint32_t *vals = nullptr;
    hipError_t e = stream_vals(s, n, &vals);
    if (e != hipSuccess) return e;
    e = launch_tmap_rows<false, true>(tmap_batch_job(frags, msgs, nmsgs, max_len, img), n, vals, mode, s);
    if (e == hipSuccess && !(mode == LAMPI_CSUM_NONE && kind == LAMPI_SEND_HDR_GM))
        e = launch_per_item(tmap_send_stamp_kernel, n, s, hdrs, hdr_stride, (uint32_t)n, (const uint32_t *)vals, frags,
                            msgs, (uint32_t)nmsgs, max_len, kind, mode, img);
    return e;
}

// The receive step over fragment records (lampi_tmap_recv_unpack_batch): the verdicts zeroed, recv_hdr_test_kernel
// over the headers (no length limit of its own: the record's length counts; not run with checksumming off, when no
// header is read), the rows of the valid records that passed, their join, and one verdict launch.
hipError_t launch_tmap_recv_unpack_batch(const lampi_tmap_frag *frags, size_t n, const lampi_tmap_msg *msgs,
                                         size_t nmsgs, uint32_t max_len, const uint8_t *hdrs, size_t hdr_stride,
                                         int kind, int64_t *copied, uint32_t *csum, uint32_t *hmask, uint32_t *dmask,
                                         uint32_t *nbad, int mode, const uint32_t *img, hipStream_t s) {
    if (n == 0) return hipMemsetAsync(nbad, 0, 2 * sizeof(uint32_t), s);
    if (!img) return hipErrorInvalidValue;
    hipError_t e = zero_verdicts2(hmask, dmask, n, nbad, s);
    if (e != hipSuccess) return e;
    uint32_t *buf = nullptr;  // the records (two words a fragment), then the fragments' values
    e = stream_vals(s, 3 * n, &buf);
    if (e != hipSuccess) return e;
    const bool none = mode == LAMPI_CSUM_NONE;
    RecvHdrRec *rec = none ? nullptr : (RecvHdrRec *)buf;
    uint32_t *vals = buf + 2 * n;
    if (!none)
        e = launch_per_item(recv_hdr_test_kernel, n, s, hdrs, hdr_stride, (uint32_t)n, kind, mode, 0xFFFFFFFFu, img,
                            rec);
    if (e == hipSuccess) {
        TmapJob J = tmap_batch_job(frags, msgs, nmsgs, max_len, img);
        J.rec = rec;
        e = launch_tmap_rows<true, true>(J, n, vals, mode, s);
        if (e == hipSuccess)
            e = launch_per_item(tmap_batch_verdict_kernel, n, s, frags, (uint32_t)n, msgs, (uint32_t)nmsgs, max_len,
                                (const RecvHdrRec *)rec, (const uint32_t *)vals, mode, copied, csum, hmask, dmask, nbad);
    }
    return e;
}
