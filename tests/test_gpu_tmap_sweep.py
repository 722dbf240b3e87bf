"""GPU: the typemap steps swept over every frame, span and row class (tests/tmap_model.py: SEND_SWEEP, RECV_SWEEP).

tests/test_tmap_classes.py proves on the CPU which geometry classes these cases reach -- every placement of the CRC
register in a chunk and over two chunks or rows, fragments of 0..3 bytes, every (start, length) of a piece inside a
chunk, pieces of 15 / 16 / 17 bytes, up to fifteen element wraps in a chunk, locate's three ways, R = 1, 2, 3, 33, 70
with the join's thread and wave branches, one to three live waves in the last workgroup, 63 / 65 pairs, every cut of
a chunk by a fragment's ends and by app_len.  Here they run: the send side through _Send.check of
test_gpu_tmap_send.py (the whole ring byte for byte, the source unchanged, the sentinel past every payload), the
receive side through expect_ring over rings built by pack_slots_at, mapped through the address rule (d_copied,
d_csum, both masks and counts, the whole application buffer with the sentinel in every gap).  Every comparison is
exact.  GM and IB headers alternate by case: the headers are not the subject.
"""
import numpy as np
import pytest

import tmap_model as tmm
from recv_unpack_model import check, expect_ring, pack_slots_at
from test_gpu_send_pack import CRC, GM, HDR, IB, NONE, SUM
from test_gpu_tmap_recv import SEQ0
from test_gpu_tmap_send import _Send, _stride

pytestmark = pytest.mark.gpu

MODES = pytest.mark.parametrize("mode", [CRC, SUM, NONE], ids=["crc", "sum", "none"])
assert (CRC, SUM, NONE) == (tmm.CRC, tmm.SUM, tmm.NONE) and HDR == tmm.HDR_BYTES


def _dv():
    from lampi_amd import device as dv

    return dv


def _by_typemap(cases, typemaps):
    return [pytest.param([c for c in cases if c[0] is tm], id=tm.name) for tm in typemaps]


def _send_all(cuda, oracle, cases, mode, seed):
    """The cases of one typemap through one source buffer and one ring, each slot pitch in turn."""
    tm = cases[0][0]
    count = max(tmm.count_for(tm, off + plen) for _, off, plen, _ in cases) + 1
    slots = max(len(tmm.fragments(off, plen, L)) * _stride(L) for _, off, plen, L in cases)
    s = _Send(cuda, tm, count, 1, slots // _stride(1) + 1, seed)
    for j, (_, off, plen, L) in enumerate(cases):
        s.L, s.stride = L, _stride(L)
        s.check(oracle, (GM, IB)[j % 2], mode, off, plen, f"{tm.name} frag_len {L} pack_off {off} pack_len {plen}")


@MODES
@pytest.mark.parametrize("cases", _by_typemap(tmm.SEND_FRAMES, tmm.FRAME_TYPEMAPS))
def test_send_every_frame_length(cuda, oracle, cases, mode):
    """frag_len 1..80, 4090..4102, 8189..8195: two whole fragments and a last one of 0..3 or frag_len - 1 bytes."""
    assert len(cases) == len(tmm.FRAME_LENS)
    _send_all(cuda, oracle, cases, mode, seed=2000 + mode)


@MODES
@pytest.mark.parametrize("cases", _by_typemap(tmm.SEND_PHASES, tmm.SWEEP_TYPEMAPS))
def test_send_every_phase_and_span(cuda, oracle, cases, mode):
    """Every sweep typemap at fragment lengths coprime to its packed_size, from pack_off 0 and 1, over every phase."""
    _send_all(cuda, oracle, cases, mode, seed=2100 + mode)


@MODES
@pytest.mark.parametrize("cases", _by_typemap(tmm.SEND_ROWS, tmm.ROW_TYPEMAPS))
def test_send_row_classes(cuda, oracle, cases, mode):
    """R = 33 and 70 (the joins' wave branch, one and two trips), one to three fragments at R = 1 and 2, the empty
    window at each."""
    _send_all(cuda, oracle, cases, mode, seed=2200 + mode)


class _RecvAt:
    """A receive case of tests/tmap_model.py -- (typemap, count, slot_stride, [(packed offset, bytes)]) -- as a ring
    of good slots in shuffled order over random packed bytes, the typemap-shaped application buffer of sentinel
    bytes, and the model's outputs and buffer."""

    def __init__(self, cuda, oracle, case, kind, mode, seed):
        import torch

        dv = _dv()
        tm, count, stride, frags = case
        rng = np.random.default_rng(seed)
        self.tm, self.count, self.stride, self.kind, self.mode = tm, count, stride, kind, mode
        self.n = n = len(frags)
        self.app_len = count * tm.packed_size
        offs, lens = [o for o, _ in frags], [c for _, c in frags]
        m = rng.integers(0, 256, size=max(o + c for o, c in frags), dtype=np.uint8)
        ring_t = torch.empty(n * stride, dtype=torch.uint8, device=cuda)
        dv.fill_stream(ring_t, seed=seed + 1)
        hring = ring_t.cpu().numpy()
        _, self.order = pack_slots_at(oracle, rng, hring, m, offs, lens, stride, SEQ0, kind, mode, rng.permutation(n))
        self.hring = hring
        self.ring = torch.from_numpy(hring).to(cuda)
        self.hbuf, self.origin = tmm.host_buffer(tm, count, seed + 2)
        self.buf = torch.from_numpy(self.hbuf).to(cuda)
        self.dtm = dv.make_tmap(tm.pairs(), tm.extent, count, cuda)
        idx = self.origin + tmm.index_map(tm, np.arange(self.app_len, dtype=np.int64))
        app = self.hbuf[idx]
        self.want = expect_ring(oracle, hring, n, stride, app, self.app_len, SEQ0, kind, mode)
        self.want_buf = self.hbuf.copy()
        self.want_buf[idx] = app
        # the ring is good: what the model delivers is what the case says
        copied = self.want[0]
        cut = np.clip(self.app_len - np.asarray(offs), 0, None)
        assert np.array_equal(copied[self.order], np.minimum(lens, cut)), "the model's deliveries"

    def run(self, what):
        got = _dv().tmap_recv_unpack(self.ring, self.n, self.stride, self.buf, self.dtm, kind=self.kind, mode=self.mode,
                                     seq_offset0=SEQ0, base_offset=self.origin)
        check(got, self.want, self.n, self.buf, self.want_buf, self.tm.extent, what)
        assert np.array_equal(self.ring.cpu().numpy(), self.hring), (what, "ring changed")


def _recv_ids(cases):
    return [pytest.param(j, c, id=f"{c[0].name}-R{tmm.frame_rows(c[2] - HDR)}") for j, c in enumerate(cases)]


@MODES
@pytest.mark.parametrize("j,case", _recv_ids(tmm.RECV_LENGTHS))
def test_recv_every_length(cuda, oracle, j, case, mode):
    """Slots of 0..95 bytes (and the row-edge lengths) back to back in shuffled order, in slots of 1, 2 and 3 rows."""
    _RecvAt(cuda, oracle, case, (GM, IB)[j % 2], mode, seed=2300 + 10 * j + mode).run(f"case {j}")


@MODES
@pytest.mark.parametrize("tm", tmm.RECV_CLIP_TYPEMAPS, ids=[t.name for t in tmm.RECV_CLIP_TYPEMAPS])
def test_recv_every_clip(cuda, oracle, tm, mode):
    """app_len cuts the third of five fragments after c = 0..33 bytes; the last two lie wholly beyond it."""
    cases = [c for c in tmm.RECV_CLIPS if c[0] is tm]
    assert len(cases) == 34
    for c, case in enumerate(cases):
        r = _RecvAt(cuda, oracle, case, (GM, IB)[c % 2], mode, seed=2400 + 10 * c + mode)
        assert [int(x) for x in r.want[0][r.order][2:]] == [c, 0, 0]
        r.run(f"{tm.name} c {c}")


@MODES
@pytest.mark.parametrize("j,case", _recv_ids(tmm.RECV_ROWS))
def test_recv_row_classes(cuda, oracle, j, case, mode):
    """Slots of 33 and 70 rows: lengths over all the rows, one row, one byte, none."""
    _RecvAt(cuda, oracle, case, (GM, IB)[j % 2], mode, seed=2500 + 10 * j + mode).run(f"case {j}")


@MODES
@pytest.mark.parametrize("j,case", [pytest.param(j, c, id=c[0].name) for j, c in enumerate(tmm.RECV_PHASES)])
def test_recv_every_phase_and_span(cuda, oracle, j, case, mode):
    """Every sweep typemap on the scattering side, equal fragments over every phase."""
    _RecvAt(cuda, oracle, case, (GM, IB)[j % 2], mode, seed=2600 + 10 * j + mode).run(case[0].name)
