"""GPU: the receive step through a typemap over host memory (lampi_host_tmap_recv_unpack_batch).

The host rings, lengths and planted faults of tests/test_gpu_host_recv_unpack.py (Batch: GM / IB / Quadrics, a bit
flipped in header bytes [0, 64), in the word @64, in the header checksum, in the payload, in a Quadrics inline
byte), delivered through a typemap instead of to application addresses: fragment i's first byte is packed byte
pack_off_i of a message of `count` elements, so app_len_i = count * packed_size - pack_off_i.  The fragments tile the
packed message in record order; the message ends inside a fragment (a truncating delivery), fragments behind it lie
past the end, and one starts exactly at the end.

The five outputs are compared with the model of the contiguous step (recv_unpack_model.expect,
quadrics_model.recv_expect: the oracle alone) for those app_len_i, and the WHOLE base buffer -- pieces, the gaps
between them, the elements past `count`, the margins -- with its before-image plus tmap_model.recv_pieces (the
reference's own walk restated) of every fragment whose header passed.

The pipeline chunk is 4 KiB (LAMPI_HOST_CHUNK_BYTES, its minimum), so batches of 63 fragments and more span well over
7 chunks.
"""
import numpy as np
import pytest

import quadrics_model as qm
import recv_unpack_model as rm
import tmap_model as tmm
from test_gpu_host_recv_unpack import CHUNK, QUADRICS, Batch, _hb
from test_gpu_send_pack import CRC, FILL, GM, HDR, IB, NONE, SUM

pytestmark = pytest.mark.gpu

KINDS = pytest.mark.parametrize("kind", [GM, IB, QUADRICS], ids=["gm", "ib", "quadrics"])
MODES = pytest.mark.parametrize("mode", [CRC, SUM, NONE], ids=["crc", "sum", "none"])
TYPEMAPS = [tmm.T1, tmm.T2, tmm.T3, tmm.T5, tmm.S1, tmm.S65, tmm.T4A]


class TmapBatch:
    """A Batch whose deliveries go through a typemap: its ring, records and faults as they are, the model re-run
    for app_len_i = total - pack_off_i over a packed image, and the base buffer the pieces land in."""

    def __init__(self, oracle, tm, kind, mode, n, shuffled=False, placement="slots", truncate=True, seed=1600):
        b = Batch(oracle, kind, mode, n, placement=placement, shuffled=shuffled, seed=seed)
        self.b, self.tm, self.kind, self.mode, self.n = b, tm, kind, mode, n
        ps = tm.packed_size
        self.pack_off = np.concatenate([[0], np.cumsum(b.ln)[:-1]]).astype(np.int64)
        sent = int(b.ln.sum())
        if truncate and n >= 16:
            # the message ends inside fragment n - 4 (or at the element boundary before its end); n - 3 and n - 2 lie
            # past the end; n - 1 starts exactly at the end
            cut = int(self.pack_off[n - 4]) + int(b.ln[n - 4]) // 2
            self.count = max(1, cut // ps)

            def truncates(count):
                c = np.minimum(b.ln[:n - 1], np.maximum(count * ps - self.pack_off[:n - 1], 0))
                return bool(((c > 0) & (c < b.ln[:n - 1])).any())

            while self.count > 1 and not truncates(self.count):  # (the end fell between two fragments)
                self.count -= 1
            self.pack_off[n - 1] = self.count * ps
        else:
            self.count = max(1, tmm.count_for(tm, sent))
        self.total = self.count * ps
        self.room = np.maximum(self.total - self.pack_off, 0)
        # the contiguous step's model on a packed image
        image = np.zeros(max(self.total, 1), np.uint8)
        args = (oracle, b.ring, b.poff, b.ln, b.H, np.ones(n, bool), image, np.minimum(self.pack_off, self.total),
                self.room)
        self.want = qm.recv_expect(*args, mode) if kind == QUADRICS else rm.expect(*args, kind, mode)
        # the base buffer: two elements past `count` and 32 bytes of margin must stay as they are
        self.base_before, self.origin = tmm.host_buffer(tm, self.count + 2, seed + 9)
        self.base_want = self.base_before.copy()
        copied = self.want[0]
        for i in range(n):
            if copied[i] == -2:  # dropped: nothing written
                continue
            c = int(min(b.ln[i], self.room[i]))
            for dest, off, m in tmm.recv_pieces(tm, int(self.pack_off[i]), c, self.total):
                src = int(b.poff[i]) + off
                self.base_want[self.origin + dest:self.origin + dest + m] = b.ring[src:src + m]

    def run(self):
        from lampi_amd import host

        base = self.base_before.copy()
        htm = host.make_host_tmap(self.tm.size, self.tm.offset, self.tm.extent, self.count)
        slots = host.make_tmap_slots(self.b.hdr_off, self.b.frag_off, self.pack_off, self.b.ln)
        got = host.host_tmap_recv_unpack_batch(self.b.ring, slots, base, self.origin, htm, kind=self.kind,
                                               mode=self.mode)
        return got, base

    def check(self, got, base):
        copied, csum, hmask, dmask, nbad = got
        wc, ws, wh, wd = self.want
        n = self.n
        bad = np.nonzero(copied != wc)[0]
        assert bad.size == 0, ("copied", bad[:4], copied[bad[:4]], wc[bad[:4]])
        assert np.array_equal(csum, ws), ("csum", np.nonzero(csum != ws)[0][:4])
        bits = lambda m: (np.asarray(m, np.uint32)[np.arange(n) // 32] >> (np.arange(n) % 32).astype(np.uint32)) & 1
        assert np.array_equal(bits(hmask).astype(bool), wh), "hdr mask"
        assert np.array_equal(bits(dmask).astype(bool), wd), "data mask"
        words = (n + 31) // 32  # (no stray bits past the last fragment's)
        assert sum(bin(int(x)).count("1") for x in hmask[:words]) == int(wh.sum()), "hdr bits"
        assert sum(bin(int(x)).count("1") for x in dmask[:words]) == int(wd.sum()), "data bits"
        assert [int(x) for x in nbad] == [int(wh.sum()), int(wd.sum())], "counts"
        d = np.nonzero(base != self.base_want)[0]
        assert d.size == 0, ("base", self.tm.name, int(d[0]) - self.origin, int(d.size))


@pytest.fixture
def chunked(monkeypatch):
    monkeypatch.setenv("LAMPI_HOST_CHUNK_BYTES", str(CHUNK))


@KINDS
@MODES
@pytest.mark.parametrize("shuffled", [False, True], ids=["ring_order", "shuffled"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 100])
def test_batches(cuda, oracle, chunked, kind, mode, n, shuffled):
    tm = TYPEMAPS[(n + 2 * kind + mode + 3 * shuffled) % len(TYPEMAPS)]
    t = TmapBatch(oracle, tm, kind, mode, n, shuffled=shuffled)
    if mode != NONE and n > 5:
        t.b.assert_classes()
    if n >= 63:
        c = np.minimum(t.b.ln, t.room)
        assert int(c.sum()) >= 7 * CHUNK  # (at least 7 chunks, in every mode)
        # a truncating fragment, fragments past the end and one exactly at it
        assert ((c > 0) & (c < t.b.ln)).any() and (t.pack_off > t.total).any() and (t.pack_off == t.total).any()
    got, base = t.run()
    t.check(got, base)


def test_every_typemap_ran():
    seen = {(n + 2 * kind + mode + 3 * s) % len(TYPEMAPS) for n in (1, 63, 64, 65, 100) for kind in (GM, IB, QUADRICS)
            for mode in (CRC, SUM, NONE) for s in (0, 1)}
    assert seen == set(range(len(TYPEMAPS)))


@KINDS
@MODES
def test_headers_at_every_alignment(cuda, oracle, chunked, kind, mode):
    """Slots 8k + 1 bytes apart from byte 5: hdr_off % 8 takes every value."""
    t = TmapBatch(oracle, TYPEMAPS[(kind + mode) % len(TYPEMAPS)], kind, mode, 100, placement="odd")
    assert set(int(x) % 8 for x in t.b.hdr_off) == set(range(8))
    got, base = t.run()
    t.check(got, base)


@KINDS
@MODES
def test_default_chunk(cuda, oracle, kind, mode):
    """The library's own chunk size: one chunk, runs of passed fragments around the dropped ones."""
    t = TmapBatch(oracle, TYPEMAPS[(kind + mode + 3) % len(TYPEMAPS)], kind, mode, 100, shuffled=True)
    got, base = t.run()
    t.check(got, base)


ROUND_TRIPS = {  # kind: (frag_len, slot_stride, chunk)
    GM: (4200, 4272, 4200),
    IB: (1976, 2048, 4096),
    QUADRICS: (2048, 2304, 4096),
}


@KINDS
@MODES
@pytest.mark.parametrize("tm", [tmm.T1, tmm.T2, tmm.T3], ids=["T1", "T2", "T3"])
def test_round_trip(cuda, oracle, monkeypatch, kind, mode, tm):
    """Host typemap send, then host typemap receive into a buffer of another pattern: every header passes, every
    checksum matches, the window's pieces are the sender's and every other byte is as it was.  The window ends 40
    bytes into a fragment, so a Quadrics tail travels inside its envelope."""
    from lampi_amd import host

    Lf, stride, chunk = ROUND_TRIPS[kind]
    monkeypatch.setenv("LAMPI_HOST_CHUNK_BYTES", str(chunk))
    total = 15 * Lf + 40  # the window [0, total) of the message
    count = tmm.count_for(tm, total) + 1
    n = (total + Lf - 1) // Lf
    src, origin = tmm.host_buffer(tm, count, 1700)
    dst_before, origin2 = tmm.host_buffer(tm, count, 1701)
    assert origin == origin2
    htm = host.make_host_tmap(tm.size, tm.offset, tm.extent, count)
    ring = np.ascontiguousarray(oracle.stream(1702, 0, n * stride))
    fill = host.make_fill(np.random.default_rng(1703).integers(0, 256, size=HDR, dtype=np.uint8), **FILL)
    host.host_tmap_send_pack(src, origin, htm, 0, total, Lf, ring, stride, fill, kind=kind, mode=mode)
    k = np.arange(n, dtype=np.int64)
    lens = np.minimum(Lf, total - k * Lf)
    slots = host.make_tmap_slots(k * stride, k * stride + _hb(kind), k * Lf, lens)
    dst = dst_before.copy()
    copied, csum, hmask, dmask, nbad = host.host_tmap_recv_unpack_batch(ring, slots, dst, origin, htm, kind=kind,
                                                                       mode=mode)
    assert [int(x) for x in nbad] == [0, 0] and not hmask.any() and not dmask.any()
    assert np.array_equal(copied, lens)
    idx = origin + tmm.index_map(tm, np.arange(total, dtype=np.int64))
    want = dst_before.copy()
    want[idx] = src[idx]
    assert np.array_equal(dst, want)
    if mode != NONE:
        msg = np.ascontiguousarray(src[idx])
        ref = oracle.desc_batch(msg, (k * Lf).astype(np.uint64), lens.astype(np.uint32),
                                np.full(n, 0xFFFFFFFF, np.uint32) if mode == CRC else None, mode)
        assert np.array_equal(csum, ref)


def test_refusals_write_nothing(cuda, oracle):
    """With a device present: refusals return hipErrorInvalidValue and leave the outputs and the base buffer as they
    were; n == 0 zeroes the two counts."""
    from lampi_amd import host, lib

    t = TmapBatch(oracle, tmm.T2, GM, CRC, 8, truncate=False)
    base = t.base_before.copy()
    f = lib().lampi_host_tmap_recv_unpack_batch
    outs = [np.full(16, 0xA5A5A5A5, np.uint32) for _ in range(5)]
    o = [x.ctypes.data for x in outs]
    htm = host.make_host_tmap(t.tm.size, t.tm.offset, t.tm.extent, t.count)

    def call(slots, n=8, ring_bytes=t.b.ring.size, kind=GM, mode=CRC, outs=o, tmap=htm):
        return f(t.b.ring.ctypes.data, ring_bytes, slots.ctypes.data, n, kind, base.ctypes.data + t.origin,
                 tmap.addr() if tmap else None, *outs, mode)

    good = host.make_tmap_slots(t.b.hdr_off, t.b.frag_off, t.pack_off, t.b.ln)
    for field, value in [("reserved", 1), ("length", (1 << 30) + 1), ("hdr_off", t.b.ring.size - 71),
                         ("frag_off", t.b.ring.size - 10)]:
        bad = good.copy()
        bad[field][4] = value  # (fragment 4 is long and has room: its payload is read)
        assert call(bad) == 1, field
    assert call(good, kind=2) == 1 and call(good, mode=3) == 1 and call(good, mode=CRC | (16 << 16)) == 1
    assert call(good, tmap=None) == 1
    broken = host.make_host_tmap(t.tm.size, t.tm.offset, t.tm.extent, t.count)
    broken.pairs["size"][1] = 0
    assert call(good, tmap=broken) == 1
    for i in range(5):
        assert call(good, outs=o[:i] + [None] + o[i + 1:]) == 1
        assert call(good, n=0, outs=o[:i] + [None] + o[i + 1:]) == 1
    assert all((x == 0xA5A5A5A5).all() for x in outs) and np.array_equal(base, t.base_before)
    assert call(good, n=0) == 0
    assert list(outs[4][:3]) == [0, 0, 0xA5A5A5A5] and all((x == 0xA5A5A5A5).all() for x in outs[:4])
