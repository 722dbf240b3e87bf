"""CPU: the two statements of the typemap forms' model agree (tests/tmap_model.py).

(a) the address rule as an index map and (b) the reference's own walks restated -- gmSendFragDesc::init's
non-contiguous branch (ref src/path/gm/sendFrag.cc:165-214) and non_contiguous_copy (ref
src/path/common/BaseDesc.cc:93-160) -- must give the same bytes for every fragment of every typemap, a window that
starts in the middle of a pair included; and the checksum the reference chains piece by piece over (b) must be the
oracle's checksum of (a)'s packed bytes, which is what the device computes.
"""
import numpy as np
import pytest

import tmap_model as tmm
from oracle.oracle import CRC_INIT, non_contiguous_copy_to_app

NFRAG = {100: 9, 1976: 5, 4096: 4, 65456: 2}  # fragments per window: enough to cross elements, quick on the CPU


def _cases():
    for tm in tmm.TYPEMAPS:
        for k, L in enumerate(tmm.FRAG_LENS):
            yield pytest.param(tm, L, tmm.LAST_LENS[k % 4], id=f"{tm.name}-{L}")


@pytest.mark.parametrize("tm,frag_len,last", list(_cases()))
def test_walks_equal_the_address_rule(oracle, tm, frag_len, last):
    for w, pack_off in enumerate(tmm.pack_offsets(tm)):
        pack_len = tmm.window_len(frag_len, NFRAG[frag_len], tmm.LAST_LENS[(tmm.LAST_LENS.index(last) + w) % 4])
        count = tmm.count_for(tm, pack_off + pack_len) + 1
        buf, origin = tmm.host_buffer(tm, count, seed=frag_len + w)
        msg_len = count * tm.packed_size
        frags = tmm.fragments(pack_off, pack_len, frag_len)
        spread = set(int(x) for x in np.arange(4) * len(frags) // 4)
        for j, (off, n) in enumerate(frags):
            want = tmm.packed(tm, buf, origin, off, n)
            sp = tmm.send_pieces(tm, off, n, msg_len)
            rp = tmm.recv_pieces(tm, off, n, msg_len)
            src = [buf[origin + a:origin + a + c] for a, c in sp]
            assert np.array_equal(np.concatenate(src) if src else np.zeros(0, np.uint8), want), (pack_off, j)
            # the receive walk scatters payload bytes [at, at + c) to the same addresses, in order, without a gap
            assert [(a, c) for a, _, c in rp] == sp, (pack_off, j)
            assert [at for _, at, _ in rp] == list(np.cumsum([0] + [c for _, c in sp[:-1]]))[:len(rp)], (pack_off, j)
            assert sum(c for _, c in sp) == n
            if j not in spread:
                continue
            # the reference's chained checksum over (b) == the oracle's value of (a)'s packed bytes
            crc = CRC_INIT
            sm, pi, pl = 0, 0, 0
            for p in src:
                crc = oracle.bcopy_uicrc(p, np.zeros(p.size, np.uint8), p.size, p.size, crc)
                r, pi, pl = oracle.bcopy_uicsum(p, np.zeros(p.size, np.uint8), p.size, p.size, pi, pl)
                sm = (sm + r) & 0xFFFFFFFF
            whole = want if n else np.zeros(1, np.uint8)
            assert crc == oracle.uicrc(whole, n), (pack_off, j)
            assert sm == oracle.uicsum(whole, n)[0], (pack_off, j)
            # ... and on the receive side (CopyToApp's non-contiguous branch as oracle.py restates it)
            pieces = [want[at:at + c] for _, at, c in rp]
            assert non_contiguous_copy_to_app(oracle, pieces, crc, 0) == (n, crc)
            assert non_contiguous_copy_to_app(oracle, pieces, sm, 1) == (n, sm)


def test_address_rule_by_hand():
    """T2 spelled out: packed bytes 0, 1..13, 14..64 of element 0, then element 1."""
    idx = tmm.index_map(tmm.T2, np.arange(66))
    assert idx[0] == 70 and list(idx[1:14]) == list(range(-16, -3)) and list(idx[14:65]) == list(range(51))
    assert idx[65] == 128 + 70
    assert tmm.first_pair(tmm.T2, 65 + 8) == 1 and tmm.first_pair(tmm.T2, 64) == 2
    assert tmm.send_pieces(tmm.T2, 8, 10, 130) == [(-16 + 7, 6), (0, 4)]
