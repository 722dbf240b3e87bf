"""The model of the one-call receive step (lampi_recv_unpack_batch, lampi_msg_recv_unpack), from the oracle alone,
and the fixtures tests/test_gpu_recv_unpack*.py share.

  header test   GM: uicrc(H, 72) == 0 / the sum of words 0..17 == 2 x the word @68 (ref src/path/gm/path.cc:364-393)
                IB: the word @68 == uicrc(H, 68) / uicsum(H, 68) (ref src/path/ib/path.cc:652-680)
                -- in bulk from oracle.desc_batch, a spread re-checked with oracle.uicrc / uicsum / header_checksum
  header fails  dropped: copied -2, checksum 0, nothing delivered (gm/path.cc:453-, ib/path.cc:702-717)
  otherwise     RecvDesc_t::CopyToApp against the word @64 (ref src/path/common/BaseDesc.cc:288-342) -- the values in
                bulk from oracle.desc_batch, a spread re-checked with oracle.copy_to_app / copy_to_app_nochecksum
"""
import numpy as np

from test_gpu_send_pack import CRC, DCSUM, GM, HCSUM, HDR, IB, NONE, WORDS, _first_diff, _put_words, _stamp_all

LEN_AT, SEQOFF_AT = 20, 56
M64 = (1 << 64) - 1


def _dv():
    from lampi_amd import device as dv

    return dv


def _u32(rows):
    return np.ascontiguousarray(rows).view("<u4").reshape(len(rows))


def header_ok(oracle, H, kind, mode):
    """The receiver's verdict on n headers (H: n x 72 bytes): True = passes."""
    n = len(H)
    if mode == NONE or n == 0:
        return np.ones(n, bool)
    H = np.ascontiguousarray(H)
    w17 = _u32(H[:, HCSUM:HDR])
    v = oracle.desc_batch(H.reshape(-1), np.arange(n, dtype=np.uint64) * np.uint64(HDR),
                          np.full(n, HDR if kind == GM else HDR - 4, np.uint32),
                          np.full(n, 0xFFFFFFFF, np.uint32) if mode == CRC else None, mode)
    if kind == IB:
        ok = v == w17
    elif mode == CRC:
        ok = v == 0
    else:
        ok = v == ((w17.astype(np.uint64) * 2) & 0xFFFFFFFF).astype(np.uint32)
    for i in sorted(set(int(x) for x in np.arange(32) * n // 32)):
        h = H[i]
        if kind == IB:
            s = (oracle.uicrc(h, HDR - 4) if mode == CRC else oracle.uicsum(h, HDR - 4)[0]) == int(w17[i])
        else:  # the sender's value over the 68 bytes, the word @68 taken as 0 (gm/sendFrag.cc:134, :219-225)
            z = h.copy()
            z[HCSUM:] = 0
            s = oracle.header_checksum(z, HDR - 4, WORDS, mode == CRC) == int(w17[i])
        assert bool(s) == bool(ok[i]), i
    return ok


def expect(oracle, base, poffs, lens, H, ok_extra, app, aoffs, alens, kind, mode):
    """The model over the bytes as they are: fragment i = lens[i] bytes at base[poffs[i]], header H[i], delivered to
    app[aoffs[i]] with alens[i] bytes of room.  ok_extra: False drops the fragment whatever its checksum says (the
    ring form's malformed headers).  Writes the deliveries into app (numpy, in place) and returns
    (copied int64, csum uint32, hdr bad bool, data bad bool)."""
    from oracle.oracle import copy_to_app, copy_to_app_nochecksum

    n = len(lens)
    ok = header_ok(oracle, H, kind, mode) & np.asarray(ok_extra, bool)
    exp = _u32(np.ascontiguousarray(H)[:, DCSUM:HCSUM])
    crc = mode == CRC
    ln = np.where(ok, np.asarray(lens, np.uint64), 0).astype(np.uint32)
    vals = np.zeros(n, np.uint32)
    if mode != NONE:
        vals = oracle.desc_batch(base, np.where(ok, np.asarray(poffs, np.uint64), 0).astype(np.uint64), ln,
                                 np.full(n, 0xFFFFFFFF, np.uint32) if crc else None, mode)
    copied = np.empty(n, np.int64)
    csum = np.zeros(n, np.uint32)
    empty = 0 if mode == NONE else (0xFFFFFFFF if crc else 0)
    spread = set(int(x) for x in np.arange(24) * n // 24)
    for i in range(n):
        if not ok[i]:
            copied[i] = -2
            continue
        a, L, room = int(poffs[i]), int(ln[i]), int(alens[i])
        c = 0 if room <= 0 else min(L, room)
        if c == 0:
            copied[i], csum[i] = 0, empty
        else:
            t = int(aoffs[i])
            app[t:t + c] = base[a:a + c]
            if mode == NONE:
                copied[i] = c
            else:
                csum[i] = vals[i]
                copied[i] = c if vals[i] == exp[i] else -1
        if i in spread:
            frag = base[a:a + L]
            r = (copy_to_app_nochecksum(frag, L, room) if mode == NONE else
                 copy_to_app(oracle, frag if L else np.zeros(1, np.uint8), L, room, int(exp[i]), crc))
            assert (int(r[0]), int(r[1])) == (int(copied[i]), int(csum[i])), (i, r[:2], copied[i], csum[i])
            assert np.array_equal(r[2], base[a:a + c]), i
    return copied, csum, ~ok, copied == -1


def check(got, want, n, app_t, app_want, unit, what=""):
    """got: what the device call returned; want: expect()'s tuple; the application buffer compared whole."""
    import torch

    dv = _dv()
    copied, csum, hmask, dmask, nbad = got
    torch.cuda.synchronize()
    wc, ws, wh, wd = want
    gc, gs = copied.cpu().numpy(), dv.as_u32(csum)
    assert np.array_equal(gc, wc), (what, "copied", int(np.nonzero(gc != wc)[0][0]), gc[gc != wc][:4], wc[gc != wc][:4])
    assert np.array_equal(gs, ws), (what, "csum", int(np.nonzero(gs != ws)[0][0]))
    assert np.array_equal(dv.mask_bits(hmask, n), wh), (what, "hdr mask")
    assert np.array_equal(dv.mask_bits(dmask, n), wd), (what, "data mask")
    # (the words past the last fragment's bit are overwritten too: no stray bits)
    for m, w in ((hmask, wh), (dmask, wd)):
        assert int(sum(bin(int(x) & 0xFFFFFFFF).count("1") for x in m.cpu().numpy())) == int(w.sum()), (what, "bits")
    assert [int(x) for x in nbad.cpu().numpy()] == [int(wh.sum()), int(wd.sum())], (what, "counts")
    want_t = app_want if isinstance(app_want, torch.Tensor) else torch.from_numpy(app_want).to(app_t.device)
    assert torch.equal(app_t, want_t), (what, "app", _first_diff(app_t, want_t, unit))


def flip_bit(buf, at, rng, lo, hi):
    """One bit flipped in buf[at + lo .. at + hi)."""
    buf[at + int(rng.integers(lo, hi))] ^= np.uint8(1 << int(rng.integers(0, 8)))


HDR_FAULTS = [(0, DCSUM), (DCSUM, HCSUM), (HCSUM, HDR)]  # a bit in bytes [0, 64), in the word @64, in the word @68


class RecvRing:
    """The descriptor form's fixture: a ring of n slots of `slot` bytes -- header i at i*slot (hdr=(stride, offset):
    in a tensor of their own), payload i at i*slot + 72 + i % 16 --, an application buffer with a region of `slot`
    bytes per fragment, destination i at i*slot + (i + 5) % 16, both prefilled with the synthetic stream."""

    def __init__(self, cuda, n, slot, seed, hdr=None):
        import torch

        dv = _dv()
        self.n, self.slot, self.cuda = n, slot, cuda
        self.ring = torch.empty(n * slot, dtype=torch.uint8, device=cuda)
        dv.fill_stream(self.ring, seed=seed)
        self.hring0 = self.ring.cpu().numpy()
        self.app = torch.empty(n * slot + 64, dtype=torch.uint8, device=cuda)
        dv.fill_stream(self.app, seed=seed + 1)
        self.app_before = self.app.clone()
        self.happ0 = self.app.cpu().numpy()
        self.hdr_stride, self.hdr_off, self.hdr_t, self.hhdr0 = slot, 0, self.ring, None
        if hdr is not None:
            self.hdr_stride, self.hdr_off = hdr
            self.hdr_t = torch.empty(self.hdr_off + n * self.hdr_stride + 8, dtype=torch.uint8, device=cuda)
            dv.fill_stream(self.hdr_t, seed=seed + 2)
            self.hhdr0 = self.hdr_t.cpu().numpy()
        k = np.arange(n, dtype=np.uint64)
        self.poffs = k * np.uint64(slot) + np.uint64(HDR) + k % np.uint64(16)
        self.aoffs = k * np.uint64(slot) + (k + np.uint64(5)) % np.uint64(16)
        self.hat = self.hdr_off + np.arange(n, dtype=np.int64) * self.hdr_stride

    def batch(self, oracle, rng, lens, kind, mode, cls, app_lens=None, last_byte=(), roomy=()):
        """A batch of fragments of `lens` bytes with valid headers, then faults by class (cls[i]: 0 clean, 1 header
        bad -- one bit flipped in bytes [0, 64), the word @64 or the word @68 in turn --, 2 data bad -- one payload
        byte flipped or, every other one, a header consistent with a wrong dataChecksum --, 3 both); app_lens:
        default three classes in turn -- <= 0, < length, > length (roomy: fragments given > length) --; last_byte: fragments whose payload flip is their
        last byte.  Returns a dict: descs, ring / hdrs (device tensors to copy in place), want (expect()'s tuple),
        app (the expected application buffer, device)."""
        import torch

        dv = _dv()
        n = self.n
        ln = np.asarray(lens, np.uint64)
        assert int(ln.max()) + HDR + 15 <= self.slot
        hring = self.hring0.copy()
        hh = hring if self.hhdr0 is None else self.hhdr0.copy()
        if app_lens is None:
            k = np.arange(n) % 3
            al = np.where(k == 0, -(np.arange(n) % 7), np.where(k == 1, (ln // 2).astype(np.int64),
                                                               ln.astype(np.int64) + 9)).astype(np.int64)
            al[ln == 0] = np.where(k[ln == 0] == 0, 0, 5)
            al[list(roomy)] = ln[list(roomy)].astype(np.int64) + 9
        else:
            al = np.asarray(app_lens, np.int64)
        cls = np.asarray(cls)
        vals = np.zeros(n, np.uint32)
        if mode != NONE:
            vals = oracle.desc_batch(hring, self.poffs, ln.astype(np.uint32), np.full(n, 0xFFFFFFFF, np.uint32)
                                     if mode == CRC else None, mode)
            wrong = np.nonzero(((cls == 2) | (cls == 3)) & (np.arange(n) % 2 == 1) & (ln > 0))[0]
            wrong = np.array([i for i in wrong if i not in set(last_byte)], np.int64)
            vals2 = vals.copy()
            vals2[wrong] ^= (np.uint32(1) << rng.integers(0, 32, size=wrong.size).astype(np.uint32))
            w = _stamp_all(oracle, hh[self.hat[:, None] + np.arange(DCSUM)], vals2, ln == 0, kind, mode)
            _put_words(hh, self.hat + DCSUM, w[0])
            _put_words(hh, self.hat + HCSUM, w[1])
        else:
            wrong = np.zeros(0, np.int64)
        nh = 0
        for i in np.nonzero(cls != 0)[0]:
            i = int(i)
            if cls[i] in (1, 3):
                lo, hi = HDR_FAULTS[nh % 3]
                nh += 1
                flip_bit(hh, int(self.hat[i]), rng, lo, hi)
            if cls[i] in (2, 3) and i not in set(int(x) for x in wrong) and ln[i] > 0:
                at = int(ln[i]) - 1 if i in last_byte else int(rng.integers(0, int(ln[i])))
                hring[int(self.poffs[i]) + at] ^= np.uint8(0x10)
        app = self.happ0.copy()
        want = expect(oracle, hring, self.poffs, ln, hh[self.hat[:, None] + np.arange(HDR)], np.ones(n, bool), app,
                      self.aoffs, al, kind, mode)
        descs = dv.make_recv_descs(self.ring, self.poffs, self.app, self.aoffs, ln, al)
        return dict(descs=descs, ring=torch.from_numpy(hring).to(self.cuda),
                    hdrs=None if self.hhdr0 is None else torch.from_numpy(hh).to(self.cuda), want=want,
                    app=torch.from_numpy(app).to(self.cuda), cls=cls, lens=ln)

    def load(self, b):
        """The batch's bytes in place, the application buffer as before any call."""
        self.ring.copy_(b["ring"])
        if b["hdrs"] is not None:
            self.hdr_t.copy_(b["hdrs"])
        self.app.copy_(self.app_before)

    def recv(self, descs, kind, mode, hdrs=True, **kw):
        return _dv().recv_unpack_batch(descs, self.hdr_t if hdrs else None, self.hdr_stride, offset=self.hdr_off,
                                       kind=kind, mode=mode, **kw)

    def check(self, got, b, what=""):
        check(got, b["want"], self.n, self.app, b["app"], self.slot, what)


def fault_classes(rng, n, ends):
    """About 10% header bad, 10% data bad, 3% both, the rest clean; ends = (class of fragment 0, of fragment n - 1)."""
    u = rng.random(n)
    cls = np.where(u < 0.10, 1, np.where(u < 0.20, 2, np.where(u < 0.23, 3, 0)))
    cls[0], cls[n - 1] = ends
    return cls


def pack_slots(oracle, rng, hring, m, L, stride, seq0, kind, mode, order=None):
    """The message m as header + payload slots written into hring (numpy): fragment k -- m[k*L : (k+1)*L], one empty
    fragment for an empty message -- in slot order[k], its header random bytes with dataLength @20, dataSeqOffset
    @56 = seq0 + k*L (mod 2^64) and, with checksumming on, the valid words @64 / @68 of `kind`.  Returns
    (n, the slot of each fragment)."""
    mlen = len(m)
    n = (mlen + L - 1) // L if mlen else 1
    order = np.arange(n) if order is None else np.asarray(order)
    lens = np.minimum(L, mlen - np.arange(n, dtype=np.int64) * L).astype(np.uint64)
    h = rng.integers(0, 256, size=(n, HDR), dtype=np.uint8)
    h[:, LEN_AT:LEN_AT + 4] = lens.astype("<u4").view(np.uint8).reshape(n, 4)
    h[:, SEQOFF_AT:SEQOFF_AT + 8] = np.array([(seq0 + k * L) & M64 for k in range(n)], "<u8").view(np.uint8).reshape(n, 8)
    if mode != NONE:
        vals = oracle.desc_batch(m if mlen else np.zeros(1, np.uint8), np.arange(n, dtype=np.uint64) * np.uint64(L),
                                 lens.astype(np.uint32), np.full(n, 0xFFFFFFFF, np.uint32) if mode == CRC else None,
                                 mode)
        w = _stamp_all(oracle, h[:, :DCSUM], vals, lens == 0, kind, mode)
        h[:, DCSUM:HCSUM] = w[0].astype("<u4").view(np.uint8).reshape(n, 4)
        h[:, HCSUM:] = w[1].astype("<u4").view(np.uint8).reshape(n, 4)
    for k in range(n):
        s, c = int(order[k]) * stride, int(lens[k])
        hring[s:s + HDR] = h[k]
        hring[s + HDR:s + HDR + c] = m[k * L:k * L + c]
    return n, order


def expect_ring(oracle, hring, nslots, stride, app, app_len, seq0, kind, mode):
    """The ring form's model over the ring bytes as they are (every field from the headers); deliveries written
    into app (numpy, in place)."""
    H = hring[:nslots * stride].reshape(nslots, stride)[:, :HDR]
    lens = _u32(H[:, LEN_AT:LEN_AT + 4]).astype(np.uint64)
    well = lens <= stride - HDR
    so = np.ascontiguousarray(H[:, SEQOFF_AT:SEQOFF_AT + 8]).view("<u8").reshape(nslots)
    off = [(int(x) - seq0) & M64 for x in so]
    room = np.array([0 if o >= app_len else app_len - o for o in off], np.int64)
    aoffs = np.array([o if r > 0 else 0 for o, r in zip(off, room)], np.uint64)
    poffs = np.arange(nslots, dtype=np.uint64) * np.uint64(stride) + np.uint64(HDR)
    return expect(oracle, hring, poffs, np.where(well, lens, 0), H, well, app, aoffs, room, kind, mode)


def pack_slots_at(oracle, rng, hring, m, offs, lens, stride, seq0, kind, mode, order=None):
    """pack_slots with a packed offset and a length of its own per fragment: fragment k -- m[offs[k] : offs[k] +
    lens[k]] -- in slot order[k], dataLength @20 = lens[k], dataSeqOffset @56 = seq0 + offs[k] (mod 2^64).  No two
    fragments' packed ranges may overlap (a call's result must not depend on the order its rows run in).  Returns
    (n, the slot of each fragment)."""
    offs, lens = np.asarray(offs, np.int64), np.asarray(lens, np.int64)
    n = len(lens)
    assert n >= 1 and len(offs) == n and int(lens.min()) >= 0 and int(lens.max()) <= stride - HDR
    assert int((offs + lens).max()) <= len(m)
    by = np.argsort(offs, kind="stable")
    full = by[lens[by] > 0]
    assert np.all((offs + lens)[full][:-1] <= offs[full][1:]), "packed ranges overlap"
    order = np.arange(n) if order is None else np.asarray(order)
    assert sorted(int(x) for x in order) == list(range(n))
    h = rng.integers(0, 256, size=(n, HDR), dtype=np.uint8)
    h[:, LEN_AT:LEN_AT + 4] = lens.astype("<u4").view(np.uint8).reshape(n, 4)
    h[:, SEQOFF_AT:SEQOFF_AT + 8] = np.array([(seq0 + int(o)) & M64 for o in offs], "<u8").view(np.uint8).reshape(n, 8)
    if mode != NONE:
        vals = oracle.desc_batch(m if len(m) else np.zeros(1, np.uint8), np.where(lens > 0, offs, 0).astype(np.uint64),
                                 lens.astype(np.uint32), np.full(n, 0xFFFFFFFF, np.uint32) if mode == CRC else None,
                                 mode)
        w = _stamp_all(oracle, h[:, :DCSUM], vals, lens == 0, kind, mode)
        h[:, DCSUM:HCSUM] = w[0].astype("<u4").view(np.uint8).reshape(n, 4)
        h[:, HCSUM:] = w[1].astype("<u4").view(np.uint8).reshape(n, 4)
    for k in range(n):
        s, c = int(order[k]) * stride, int(lens[k])
        hring[s:s + HDR] = h[k]
        hring[s + HDR:s + HDR + c] = m[int(offs[k]):int(offs[k]) + c]
    return n, order
