"""GPU: the receive step in one call over host memory (lampi_host_recv_unpack_batch).

Host NIC rings built by pack_slots_at (tests/recv_unpack_model.py; Quadrics: _slots of tests/test_gpu_quadrics_recv.py),
faults planted from a fixed seed, and every result -- copied, the calculated checksum, both masks, both counts, the
whole prefilled application buffer -- compared with the model of the device form (recv_unpack_model.expect,
quadrics_model.recv_expect: the oracle alone) and with the device form lampi_recv_unpack_batch run on the same bytes.

Fault classes: a bit flipped in header bytes [0, 64), in the word @64, in the header checksum word (all three drop
the fragment: LAMPI_RECV_HDR_BAD, no application byte written), in the payload (LAMPI_RECV_DATA_BAD, delivered
all the same), and in a Quadrics inline data[] byte (the header's checksum covers it: LAMPI_RECV_HDR_BAD).

The pipeline chunk is 4 KiB (LAMPI_HOST_CHUNK_BYTES, its minimum), so batches of 63 fragments and more span well over
7 chunks: the 3-deep ring of device buffers wraps and the last chunk is partial.
"""
import numpy as np
import pytest

import quadrics_model as qm
import recv_unpack_model as rm
from test_gpu_quadrics_recv import _slots as q_slots
from test_gpu_send_pack import CRC, FILL, GM, HDR, IB, NONE, SUM

pytestmark = pytest.mark.gpu

QUADRICS = 3
CHUNK = 4096
L = 1976  # the longest fragment of the batches
KINDS = pytest.mark.parametrize("kind", [GM, IB, QUADRICS], ids=["gm", "ib", "quadrics"])
MODES = pytest.mark.parametrize("mode", [CRC, SUM, NONE], ids=["crc", "sum", "none"])
HDR_OK, HDR_HEAD, HDR_DCSUM, HDR_HCSUM, PAYLOAD, INLINE_DATA = range(6)


def _hb(kind):
    return qm.HDR if kind == QUADRICS else HDR


def _lengths(rng, n, kind):
    """Ragged lengths 0..L with the edges planted; fragments 1..5 long enough to carry their planted fault
    (fragment 5 a Quadrics inline payload)."""
    ln = rng.integers(0, L + 1, size=n).astype(np.int64)
    edges = [0, 1, 3, 51, 52, 53, 64, L - 1, L]
    if n > 16:
        ln[rng.choice(np.arange(6, n), size=len(edges), replace=False)] = edges
    if n > 5:
        ln[1:5] = [L, 700, 53, L]
        ln[5] = 40 if kind == QUADRICS else 300
    if kind == QUADRICS and n > 16:
        ln[6:12] = rng.integers(1, qm.INLINE + 1, size=6)  # (uniform lengths would hold next to no inline payload)
    return ln


def _app_lens(ln):
    """AppBufferLen by fragment index mod 4: above the length, below it, equal to it, <= 0."""
    j = np.arange(len(ln))
    al = np.where(j % 4 == 0, ln + 9, np.where(j % 4 == 1, ln // 2, np.where(j % 4 == 2, ln, -(j % 7)))).astype(np.int64)
    return al


class Batch:
    """A host ring of n slots, the slot records, the application buffer before the call, and the model's results.

    placement: "slots" (header, then payload; IB behind a 40-byte GRH), "apart" (headers in a region of their own,
    80 / 136 bytes apart from byte 3), "odd" (a slot stride of 8k + 1 from byte 5: hdr_off % 8 takes every value).
    order: the records in ring order or shuffled.  dense_app: the deliveries touch in the application buffer."""

    def __init__(self, oracle, kind, mode, n, placement="slots", shuffled=False, dense_app=False, faults=True,
                 seed=1300):
        rng = np.random.default_rng(seed + 16 * kind + mode + 7 * n)
        self.kind, self.mode, self.n = kind, mode, n
        hb = _hb(kind)
        ln = _lengths(rng, n, kind)
        grh = 40 if (kind == IB and placement == "slots") else 0
        stride = {"slots": 2176, "apart": 2176, "odd": 2177}[placement]
        base = 5 if placement == "odd" else 0
        assert grh + hb + L <= stride
        packed = np.ascontiguousarray(oracle.stream(seed + 1, 0, base + n * stride + grh))
        slot_of = rng.permutation(n)  # fragment k sits in slot slot_of[k]: arrival order is not ring order
        view = packed[base + grh:]
        if kind == QUADRICS:
            q_slots(oracle, rng, view, ln, np.zeros(n, np.int64), stride, slot_of, mode)
        else:
            offs = np.arange(n, dtype=np.int64) * L
            m = oracle.stream(seed + 2, 0, n * L)
            rm.pack_slots_at(oracle, rng, view, m, offs, ln, stride, 0, kind, mode, order=slot_of)
        hdr_off = base + grh + slot_of.astype(np.int64) * stride
        frag_off = hdr_off + hb
        if placement == "apart":  # the headers move to a region of their own in front of the slots
            hstep = hb + 8
            region = 3 + n * hstep + 61
            ring = np.concatenate([oracle.stream(seed + 3, 0, region), packed])
            for k in range(n):
                ring[3 + k * hstep:3 + k * hstep + hb] = packed[hdr_off[k]:hdr_off[k] + hb]
            frag_off = frag_off + region
            hdr_off = 3 + np.arange(n, dtype=np.int64) * hstep
        else:
            ring = packed
        self.ring = np.ascontiguousarray(ring)
        inline = (kind == QUADRICS) & (ln > 0) & (ln <= qm.INLINE)
        al = _app_lens(ln)
        copy = np.minimum(ln, np.maximum(al, 0))

        # the planted faults
        cls = np.zeros(n, np.int64)
        if faults and mode != NONE and n > 5:
            u = rng.random(n)
            cls = np.where(u < 0.04, HDR_HEAD, np.where(u < 0.08, HDR_DCSUM, np.where(u < 0.12, HDR_HCSUM,
                           np.where(u < 0.24, PAYLOAD, HDR_OK))))
            cls[0] = cls[n - 1] = HDR_OK
            cls[1:5] = [HDR_HEAD, HDR_DCSUM, HDR_HCSUM, PAYLOAD]
            cls[5] = INLINE_DATA if kind == QUADRICS else HDR_OK
            cls[(cls == PAYLOAD) & ((ln == 0) | inline)] = HDR_OK  # (an inline payload's flip is a header fault)
        csum_at = qm.HCSUM if kind == QUADRICS else rm.HCSUM
        for k in np.nonzero(cls)[0]:
            k = int(k)
            if cls[k] == HDR_HEAD:
                rm.flip_bit(self.ring, int(hdr_off[k]), rng, 0, 64)
            elif cls[k] == HDR_DCSUM:
                rm.flip_bit(self.ring, int(hdr_off[k]), rng, 64, 68)
            elif cls[k] == HDR_HCSUM:
                rm.flip_bit(self.ring, int(hdr_off[k]), rng, csum_at, csum_at + 4)
            elif cls[k] == PAYLOAD:
                rm.flip_bit(self.ring, int(frag_off[k]), rng, 0, int(ln[k]))
            else:
                rm.flip_bit(self.ring, int(hdr_off[k]) + qm.DATA, rng, 0, int(ln[k]))
        self.cls = cls

        # the records, in ring order (by slot) or in arrival order (fragment k: shuffled over the slots)
        rec = np.argsort(slot_of) if not shuffled else np.arange(n)
        self.hdr_off, self.frag_off, self.ln, self.al = hdr_off[rec], frag_off[rec], ln[rec], al[rec]
        self.cls, copy, inline = cls[rec], copy[rec], inline[rec]
        if dense_app:
            self.aoff = np.concatenate([[0], np.cumsum(copy)[:-1]]).astype(np.int64) + 7
        else:
            self.aoff = np.arange(n, dtype=np.int64) * (L + 32) + (np.arange(n) + 5) % 16
        self.app_before = np.ascontiguousarray(oracle.stream(seed + 4, 0, n * (L + 32) + 64))

        # the model, over the bytes as they are
        self.poff = np.where(inline, self.hdr_off + qm.DATA, self.frag_off)
        self.H = self.ring[self.hdr_off[:, None] + np.arange(hb)]
        self.app_want = self.app_before.copy()
        args = (oracle, self.ring, self.poff, self.ln, self.H, np.ones(n, bool), self.app_want, self.aoff, self.al)
        self.want = qm.recv_expect(*args, mode) if kind == QUADRICS else rm.expect(*args, kind, mode)

    def assert_classes(self):
        """Every verdict class is there and at least half of the fragments are clean."""
        copied = self.want[0]
        assert (copied == -2).any() and (copied == -1).any() and (copied > 0).any() and (copied == 0).any()
        assert (copied >= 0).sum() * 2 >= self.n
        hdr_faults = np.isin(self.cls, [HDR_HEAD, HDR_DCSUM, HDR_HCSUM, INLINE_DATA])
        assert np.array_equal(copied == -2, hdr_faults)
        for c in [HDR_HEAD, HDR_DCSUM, HDR_HCSUM, PAYLOAD] + ([INLINE_DATA] if self.kind == QUADRICS else []):
            assert (self.cls == c).any(), c

    def run_host(self):
        from lampi_amd import host

        app = self.app_before.copy()
        slots = host.make_recv_slots(self.hdr_off, self.frag_off, app, self.aoff, self.ln, self.al)
        got = host.host_recv_unpack_batch(self.ring, slots, kind=self.kind, mode=self.mode)
        return got, app

    def run_device(self, cuda):
        """lampi_recv_unpack_batch on the same bytes: the ring uploaded, the headers packed in record order."""
        import torch

        from lampi_amd import device as dv

        hb = _hb(self.kind)
        ring = torch.from_numpy(self.ring).to(cuda)
        hdrs = torch.from_numpy(np.ascontiguousarray(self.H).reshape(-1)).to(cuda)
        app = torch.from_numpy(self.app_before).to(cuda)
        descs = dv.make_recv_descs(ring, self.frag_off, app, self.aoff, self.ln, self.al)
        copied, csum, hmask, dmask, nbad = dv.recv_unpack_batch(descs, hdrs, hb, kind=self.kind, mode=self.mode)
        torch.cuda.synchronize()
        return ((copied.cpu().numpy(), dv.as_u32(csum), hmask.cpu().numpy().view(np.uint32),
                 dmask.cpu().numpy().view(np.uint32), nbad.cpu().numpy().view(np.uint32)), app.cpu().numpy())

    def check(self, got, app, what):
        copied, csum, hmask, dmask, nbad = got
        wc, ws, wh, wd = self.want
        n = self.n
        assert np.array_equal(copied, wc), (what, "copied", np.nonzero(copied != wc)[0][:4], copied[copied != wc][:4],
                                            wc[copied != wc][:4])
        assert np.array_equal(csum, ws), (what, "csum", np.nonzero(csum != ws)[0][:4])
        bits = lambda m: (np.asarray(m, np.uint32)[np.arange(n) // 32] >> (np.arange(n) % 32).astype(np.uint32)) & 1
        assert np.array_equal(bits(hmask).astype(bool), wh), (what, "hdr mask")
        assert np.array_equal(bits(dmask).astype(bool), wd), (what, "data mask")
        words = (n + 31) // 32  # (no stray bits past the last fragment's)
        assert sum(bin(int(x)).count("1") for x in hmask[:words]) == int(wh.sum()), (what, "hdr bits")
        assert sum(bin(int(x)).count("1") for x in dmask[:words]) == int(wd.sum()), (what, "data bits")
        assert [int(x) for x in nbad] == [int(wh.sum()), int(wd.sum())], (what, "counts")
        d = np.nonzero(app != self.app_want)[0]
        assert d.size == 0, (what, "app", int(d[0]), int(d.size))


@pytest.fixture
def chunked(monkeypatch):
    monkeypatch.setenv("LAMPI_HOST_CHUNK_BYTES", str(CHUNK))


@KINDS
@MODES
@pytest.mark.parametrize("shuffled", [False, True], ids=["ring_order", "shuffled"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 100])
def test_batches(cuda, oracle, chunked, kind, mode, n, shuffled):
    b = Batch(oracle, kind, mode, n, shuffled=shuffled)
    if mode != NONE and n > 5:
        b.assert_classes()
    if n >= 63:
        assert int(np.minimum(b.ln, np.maximum(b.al, 0)).sum()) >= 7 * CHUNK  # (at least 7 chunks, in every mode)
    got, app = b.run_host()
    b.check(got, app, "host")
    dgot, dapp = b.run_device(cuda)
    b.check(dgot, dapp, "device")


@KINDS
@MODES
@pytest.mark.parametrize("placement", ["apart", "odd"])
def test_header_placements(cuda, oracle, chunked, kind, mode, placement):
    """Headers in a region of their own (runs of their own on the way up), and slots 8k + 1 bytes apart so that a
    header's address takes every residue mod 8."""
    b = Batch(oracle, kind, mode, 100, placement=placement, shuffled=placement == "apart")
    if placement == "odd":
        assert set(int(x) % 8 for x in b.hdr_off) == set(range(8))
    if mode != NONE:
        b.assert_classes()
    got, app = b.run_host()
    b.check(got, app, "host")
    dgot, dapp = b.run_device(cuda)
    b.check(dgot, dapp, "device")


@KINDS
@MODES
@pytest.mark.parametrize("registered", [False, True], ids=["pageable", "registered"])
def test_deliveries_that_touch(cuda, oracle, chunked, kind, mode, registered):
    """The deliveries packed end to end in the application buffer, so that a chunk's passed fragments go back as
    runs around the dropped ones; the ring pageable and page-locked."""
    from lampi_amd import host

    b = Batch(oracle, kind, mode, 100, dense_app=True)
    if mode != NONE:
        b.assert_classes()
    if registered:
        host.host_register(b.ring)
    try:
        got, app = b.run_host()
    finally:
        if registered:
            host.host_unregister(b.ring)
    b.check(got, app, "host")


@KINDS
@MODES
def test_default_chunk(cuda, oracle, kind, mode):
    """The library's own chunk size: one chunk."""
    b = Batch(oracle, kind, mode, 100, shuffled=True)
    got, app = b.run_host()
    b.check(got, app, "host")


ROUND_TRIPS = {  # kind: (frag_len, slot_stride, msg_len, chunk)
    GM: (65456, 65536, 9 * 65456 + 1234, 65536),
    IB: (1976, 2048, 300 * 1976 + 7, 40 * 1976),
    QUADRICS: (2048, 2304, 60 * 2048 + 40, 8 * 2048),  # (a 40-byte tail travels inside its envelope)
}


@KINDS
@MODES
def test_round_trip(cuda, oracle, monkeypatch, kind, mode):
    """Host send, then host receive: every header passes, every checksum matches, the application buffer is the
    message."""
    from lampi_amd import host

    Lf, stride, mlen, chunk = ROUND_TRIPS[kind]
    monkeypatch.setenv("LAMPI_HOST_CHUNK_BYTES", str(chunk))
    rng = np.random.default_rng(1400 + mode)
    msg = np.ascontiguousarray(oracle.stream(1401, 0, mlen))
    n = (mlen + Lf - 1) // Lf
    ring = np.ascontiguousarray(oracle.stream(1402, 0, n * stride))
    fill = host.make_fill(rng.integers(0, 256, size=HDR, dtype=np.uint8), **FILL)
    host.host_msg_send_pack(msg, Lf, ring, stride, fill, kind=kind, mode=mode)
    k = np.arange(n, dtype=np.int64)
    lens = np.minimum(Lf, mlen - k * Lf)
    app = np.zeros(mlen, np.uint8)
    slots = host.make_recv_slots(k * stride, k * stride + _hb(kind), app, k * Lf, lens, lens)
    copied, csum, hmask, dmask, nbad = host.host_recv_unpack_batch(ring, slots, kind=kind, mode=mode)
    assert [int(x) for x in nbad] == [0, 0] and not hmask.any() and not dmask.any()
    assert np.array_equal(copied, lens)
    assert np.array_equal(app, msg)
    if mode != NONE:
        want = oracle.desc_batch(msg, (k * Lf).astype(np.uint64), lens.astype(np.uint32),
                                 np.full(n, 0xFFFFFFFF, np.uint32) if mode == CRC else None, mode)
        assert np.array_equal(csum, want)


def test_refusals_write_nothing(cuda, oracle):
    """With a device present: refusals return hipErrorInvalidValue and leave the outputs and the application buffer
    as they were; n == 0 zeroes the two counts."""
    from lampi_amd import host, lib

    b = Batch(oracle, GM, CRC, 8, faults=False)
    app = b.app_before.copy()
    f = lib().lampi_host_recv_unpack_batch
    outs = [np.full(16, 0xA5A5A5A5, np.uint32) for _ in range(5)]
    o = [x.ctypes.data for x in outs]

    def call(slots, n=8, ring_bytes=b.ring.size, kind=GM, mode=CRC, outs=o):
        return f(b.ring.ctypes.data, ring_bytes, slots.ctypes.data, n, kind, *outs, mode)

    good = host.make_recv_slots(b.hdr_off, b.frag_off, app, b.aoff, b.ln, b.al)
    for field, value in [("reserved", 1), ("length", (1 << 30) + 1), ("hdr_off", b.ring.size - 71),
                         ("frag_off", b.ring.size - 10)]:
        bad = good.copy()
        bad[field][4] = value  # (fragment 4 is long and has room: its payload is read)
        assert call(bad) == 1, field
    assert call(good, kind=2) == 1 and call(good, mode=3) == 1 and call(good, mode=CRC | (16 << 16)) == 1
    assert call(good, ring_bytes=int(b.hdr_off.max()) + 71) == 1
    for i in range(5):
        assert call(good, outs=o[:i] + [None] + o[i + 1:]) == 1
        assert call(good, n=0, outs=o[:i] + [None] + o[i + 1:]) == 1
    assert all((x == 0xA5A5A5A5).all() for x in outs) and np.array_equal(app, b.app_before)
    assert call(good, n=0) == 0
    assert list(outs[4][:3]) == [0, 0, 0xA5A5A5A5] and all((x == 0xA5A5A5A5).all() for x in outs[:4])
