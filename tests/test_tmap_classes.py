"""CPU: the class ledger of the typemap sweep (tests/tmap_model.py: classes, SEND_SWEEP, RECV_SWEEP).

classes() restates the frame and address rules of the header comment of lampi_amd/csrc/tmap_kernels.h and names, for
one call, every geometry class its fragments fall in: where the CRC register lands in a chunk, which byte spans of a
chunk come from one piece, how many elements a chunk crosses, how a chunk's element is found, the rows per fragment
and their join, the live waves of the last workgroup, the bytes at which a fragment or app_len cuts a chunk.  These
are conditions on the inputs of tests/test_gpu_tmap_sweep.py, checked here without a GPU: the union over the sweep
must hold every required class, and the union over the six typemaps x four lengths x last fragments of the older
tests must not hold the ones the sweep was written for.

("wraps", 16) cannot occur: sixteen one-byte elements in a 16-byte chunk are fifteen passes from one element to the
next, so the ledger requires 15, the most a chunk can hold.
"""
import numpy as np
import pytest

import tmap_model as tmm
from oracle.oracle import CRC_INIT
from tmap_model import CRC, NONE, SUM

MODES = (CRC, SUM, NONE)


@pytest.fixture(scope="module")
def send_union():
    return {m: set().union(*(tmm.send_classes(c, m) for c in tmm.SEND_SWEEP)) for m in MODES}


@pytest.fixture(scope="module")
def recv_union():
    return {m: set().union(*(tmm.recv_classes(c, m) for c in tmm.RECV_SWEEP)) for m in MODES}


def _required(u):
    """The classes both directions must reach; u: {mode: union}."""
    every = u[CRC] | u[SUM] | u[NONE]
    need = {("dl", d) for d in range(-3, 16)} | {("dl_rows",)}
    assert need <= u[CRC], sorted(need - u[CRC])
    need = {("span", k, n) for n in range(1, 16) for k in range(0, 17 - n)}
    assert len(need) == 135 and need <= every, sorted(need - every)
    need = {("fast", 16), ("fast", 17), ("near", 15)}
    need |= {("wraps", w) for w in (1, 2, 3, 8, 15)}
    need |= {("locate", "sub"), ("locate", "in")} | {("locate", "div", q) for q in (1, 2, 3)}
    need |= {("R", R) for R in (1, 2, 3, 33, 70)}
    need |= {("tailwaves", w) for w in (1, 2, 3)}
    need |= {("staged", True), ("staged", False)}
    need |= {("cut", k, end) for k in range(1, 16) for end in ("first", "last")} | {("cut", k) for k in range(1, 16)}
    assert need <= every, sorted(need - every)
    for m in (CRC, SUM):
        assert {("join", j) for j in ("thread", "wave", "wave2")} <= u[m], m
    assert not any(t[0] == "join" for t in u[NONE])
    assert not any(t[0] in ("dl", "dl_rows", "tiny") for t in u[SUM] | u[NONE])


def test_send_sweep_reaches_every_required_class(send_union):
    _required(send_union)
    assert {("tiny", L) for L in range(4)} <= send_union[CRC]


def test_recv_sweep_reaches_every_required_class(recv_union):
    _required(recv_union)
    # (an empty fragment delivers nothing on receive: its rows do not run, the verdict gives the register itself)
    assert {("tiny", L) for L in (1, 2, 3)} <= recv_union[CRC] and ("tiny", 0) not in recv_union[CRC]
    for m in (CRC, SUM):
        clips = {t for t in recv_union[m] if t[0] == "clip"}
        assert {c for _, c, _ in clips} == set(range(16)), m
        assert len({c for _, c, b in clips if b}) >= 3 and len({c for _, c, b in clips if not b}) >= 3, m
    assert not any(t[0] == "clip" for t in recv_union[NONE])  # (with checksumming off L = ncopy: nothing to cut)


def test_pair_counts_either_side_of_the_lds_cut():
    assert sorted(t.num_pairs for t in (tmm.S63, tmm.T4A, tmm.S65)) == [63, 64, 65]
    used = {c[0].name for c in tmm.SEND_SWEEP} | {"T4a"}
    assert {"S63", "T4a", "S65"} <= used
    assert {c[0].name for c in tmm.RECV_SWEEP} >= {"S63", "S65"}
    assert [t.packed_size for t in tmm.SWEEP_LONG] == [8192, 8193, 4111]


def test_every_sweep_typemap_visits_every_phase():
    """frag_len coprime to packed_size and at least packed_size fragments (capped at 130) from both window starts."""
    for tm in tmm.SWEEP_TYPEMAPS:
        if tm in tmm.SWEEP_LONG:
            continue
        cases = [c for c in tmm.SEND_PHASES if c[0] is tm]
        assert len(cases) == 6 and {c[1] for c in cases} == {0, 1}
        for _, off, plen, L in cases:
            assert np.gcd(L, tm.packed_size) == 1
            phases = {o % tm.packed_size for o, _ in tmm.fragments(off, plen, L)}
            assert len(phases) == min(tm.packed_size, 131), (tm.name, L)


def test_the_older_cases_do_not_reach_them():
    """What the sweep adds: the six typemaps x four lengths x last fragments x window starts of
    test_gpu_tmap_send.py / test_gpu_tmap_recv.py (three fragments each: these classes depend on a fragment's length
    alone) and the empty window hold none of these."""
    old = set()
    for tm in tmm.TYPEMAPS:
        for L in tmm.FRAG_LENS:
            for last in tmm.LAST_LENS:
                for off in tmm.pack_offsets(tm):
                    for m in (CRC, SUM):
                        old |= tmm.classes(tm, off, tmm.window_len(L, 3, last), L, m)
                        old |= tmm.classes(tm, off, tmm.window_len(L, 3, last), L, m, recv_room=(L + 8 + 7) // 8 * 8)
    old |= tmm.classes(tmm.T2, 72, 0, 1976, CRC)
    assert {t[1] for t in old if t[0] == "dl"} == {0, 1, 8, 11, 12, 15, -1}
    missing = {("dl", 5), ("dl", 6), ("dl", 7), ("dl_rows",), ("join", "wave"), ("join", "wave2"), ("tiny", 2),
               ("tiny", 3), ("R", 3), ("R", 33), ("wraps", 3), ("wraps", 8)}
    assert not (missing & old), sorted(missing & old)
    assert max(t[1] for t in old if t[0] == "R") == 16


def test_classes_by_hand():
    """Three calls spelled out."""
    base = {("R", 1), ("tailwaves", 1), ("staged", True)}
    # T1 (8-byte blocks), one fragment of 20 bytes.  SUM: chunk 0 = two blocks, chunk 1 = bytes 16..19 of the third
    # block, found two elements on from the row's first byte
    assert tmm.classes(tmm.T1, 0, 20, 20, SUM) == base | {
        ("span", 0, 8), ("span", 8, 8), ("span", 0, 4), ("cut", 4), ("cut", 4, "last"), ("wraps", 1), ("locate", "in"),
        ("locate", "div", 2)}
    # CRC: P = 4076 = 16 * 254 + 12, so the chunk at 4064 holds the register from its byte 12 on and the fragment's
    # first four bytes; the chunk at 4080 holds the rest of block 0, block 1 and half of block 2
    assert tmm.classes(tmm.T1, 0, 20, 20, CRC) == base | {
        ("dl", 12), ("cut", 12), ("cut", 12, "first"), ("span", 12, 4), ("span", 0, 4), ("span", 4, 8), ("wraps", 2),
        ("locate", "in")}
    # S17 (17-byte blocks), two elements posted (34 bytes), slots of two rows, SUM.  Slot 0 = 20 bytes: a whole chunk
    # from a piece with 17 bytes left, then byte 16 of block 0 and three of block 1.  Slot 1 = 30 bytes from packed
    # byte 20, cut after 14: bytes [0, 14) of its first chunk from one piece, its second chunk not delivered
    got = tmm.classes(tmm.S17, 0, 0, 0, SUM, recv_room=8192, app_len=34, frags=[(0, 20), (20, 30)])
    assert got == {("R", 2), ("join", "thread"), ("tailwaves", 0), ("staged", True), ("fast", 17), ("span", 0, 1),
                   ("span", 1, 3), ("cut", 4), ("cut", 4, "last"), ("wraps", 1), ("locate", "in"), ("span", 0, 14),
                   ("clip", 14, False), ("cut", 14), ("cut", 14, "last")}
    # a register over two rows: L = 4097 in two rows, P = 4095
    assert {("dl", 15), ("dl", -1), ("dl_rows",), ("R", 2)} <= tmm.classes(tmm.T5, 0, 4097, 4097, CRC)
    assert tmm.classes(tmm.T5, 0, 0, 100, CRC) == base | {("tiny", 0), ("dl", 12)}


def _walk_cases():
    for tm in tmm.SWEEP_TYPEMAPS:
        for L in tmm.phase_frag_lens(tm)[-2:]:
            yield pytest.param(tm, L, id=f"{tm.name}-{L}")


@pytest.mark.parametrize("tm,frag_len", list(_walk_cases()))
def test_walks_equal_the_address_rule_on_the_sweep_typemaps(oracle, tm, frag_len):
    """test_tmap_model.py's property on SWEEP_TYPEMAPS: the reference's walks give the index map's bytes, and the
    checksum chained over their pieces is the oracle's value of the packed bytes."""
    from oracle.oracle import non_contiguous_copy_to_app

    nf = 6
    for w, pack_off in enumerate((0, 1, 2 * tm.packed_size - 40 if tm.packed_size > 40 else 3 * tm.packed_size)):
        pack_len = tmm.window_len(frag_len, nf, [1, 2, 3][w])
        count = tmm.count_for(tm, pack_off + pack_len) + 1
        buf, origin = tmm.host_buffer(tm, count, seed=frag_len + w)
        msg_len = count * tm.packed_size
        for j, (off, n) in enumerate(tmm.fragments(pack_off, pack_len, frag_len)):
            want = tmm.packed(tm, buf, origin, off, n)
            sp = tmm.send_pieces(tm, off, n, msg_len)
            rp = tmm.recv_pieces(tm, off, n, msg_len)
            src = [buf[origin + a:origin + a + c] for a, c in sp]
            assert np.array_equal(np.concatenate(src), want), (pack_off, j)
            assert [(a, c) for a, _, c in rp] == sp, (pack_off, j)
            assert [at for _, at, _ in rp] == list(np.cumsum([0] + [c for _, c in sp[:-1]])), (pack_off, j)
            if j not in (0, nf - 2, nf - 1):
                continue
            crc, sm, pi, pl = CRC_INIT, 0, 0, 0
            for p in src:
                crc = oracle.bcopy_uicrc(p, np.zeros(p.size, np.uint8), p.size, p.size, crc)
                r, pi, pl = oracle.bcopy_uicsum(p, np.zeros(p.size, np.uint8), p.size, p.size, pi, pl)
                sm = (sm + r) & 0xFFFFFFFF
            assert crc == oracle.uicrc(want, n) and sm == oracle.uicsum(want, n)[0], (pack_off, j)
            pieces = [want[at:at + c] for _, at, c in rp]
            assert non_contiguous_copy_to_app(oracle, pieces, crc, 0) == (n, crc)
            assert non_contiguous_copy_to_app(oracle, pieces, sm, 1) == (n, sm)
