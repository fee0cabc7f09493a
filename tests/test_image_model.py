"""CPU: tests/image_model.py is the consumers' view of the sequence images, so that byte equality with it (tests/test_gpu_sequence_images.py)
means something; and every block of tests/image_blocks.py is in the regime it names (DESIGN.md 4.1').

 - ref2: the 16 bytes at and the 16 below the anchor's group, addressed as cut_ctx (probe.hip) and the packed filter (extend.hip)
   address them, lie inside one 128-byte line and inside the copy and decode to the bases around the anchor;
 - 4-bit copies: byte (q >> 1) - s of copy (q & 1, s) starts with base q;
 - 2-bit shifted copies: the 64-base window at any position is four aligned dwords of its own copy, and of copy 0 with a funnel shift;
 - class_scores: sound for every pair of present codes, and equal to the rule as documented."""
import numpy as np
import pytest

import image_blocks as B
import image_model as M
from extend_regimes import simple_matrix

MODEL_LENGTHS = [1, 3, 127, 128, 129, 383, 384, 385, 769, 4099]


def some_codes(n, seed=0):
    """mostly A/C/G/T with a few codes >= 4, none of them 0 where it could hide a shift"""
    rng = np.random.default_rng(n + seed)
    c = rng.integers(0, 4, n).astype(np.uint8)
    c[rng.integers(0, n, max(n // 50, 1))] = rng.integers(4, 8, max(n // 50, 1))
    return c


def bases_of(b):
    """the four 2-bit bases of every byte, low bits first"""
    b = np.asarray(b, dtype=np.uint8)
    return ((b[:, None] >> np.array([0, 2, 4, 6], dtype=np.uint8)) & 3).reshape(-1)


def window(c2, lo, n):
    """2-bit codes lo .. lo + n - 1 of a block, 0 outside"""
    return M._at(c2, np.arange(lo, lo + n, dtype=np.int64), 0)


@pytest.mark.parametrize("n", MODEL_LENGTHS)
def test_ref2_windows_of_every_anchor_lie_in_one_line_and_hold_the_bases_around_it(n):
    c = some_codes(n)
    c2 = M.two_bit(c)
    img = M.ref2_image(c)
    nphys = M.ref2_nphys(n)
    assert img.shape == (4, nphys) and nphys % 128 == 0
    for a in range(n + 1):
        jj0 = (a >> 2) + M.PACK2_BIAS
        copy = img[a & 3]
        # the packed filter: both windows out of the line chosen for the left one
        line = (jj0 - 16) // M.PACK2_PAYLOAD
        p = jj0 + 32 * line
        assert (p - 16) >> 7 == (p + 15) >> 7 == line and p + 16 <= nphys, (n, a)
        assert np.array_equal(bases_of(copy[p:p + 16]), window(c2, a, 64)), (n, a)
        assert np.array_equal(bases_of(copy[p - 16:p]), window(c2, a - 64, 64)), (n, a)
        # cut_ctx: each window out of the line chosen for its own first byte
        for jj, lo in ((jj0, a), (jj0 - 16, a - 64)):
            p = jj + 32 * (jj // M.PACK2_PAYLOAD)
            assert p >> 7 == (p + 15) >> 7 and p + 16 <= nphys, (n, a)
            assert np.array_equal(bases_of(copy[p:p + 16]), window(c2, lo, 64)), (n, a)
    # the last 32 bytes of every line repeat the first 32 of the next
    lines = img.reshape(4, -1, 128)
    assert np.array_equal(lines[:, :-1, 96:], lines[:, 1:, :32])


@pytest.mark.parametrize("n", MODEL_LENGTHS)
def test_pack4_byte_of_every_base_and_shift_starts_with_that_base(n):
    c = some_codes(n)
    img = M.pack4_image(c)
    nb, stride = M.pack4_nbytes(n), M.pack4_stride(n)
    assert img.shape == (8, stride) and stride % 128 == 0 and stride >= nb + 2 * M.PACK_PAD
    c7 = np.concatenate([c & 7, [7]])
    for q in range(n):
        for s in range(4):
            j = (q >> 1) - s
            if j < -M.PACK4_FRONT:
                continue
            byte = int(img[(q & 1) + 2 * s, M.PACK_PAD + j])
            assert (byte & 15, byte >> 4) == (c7[q], c7[q + 1]), (n, q, s)
    # what no base reaches is the pad: code 7 in both nibbles
    assert np.all(img[:, :M.PACK_PAD - M.PACK4_FRONT] == 0x77) and np.all(img[:, M.PACK_PAD + nb:] == 0x77)
    # the high nibble of byte len / 2 of the unshifted copies: the base behind the block
    assert int(img[0, M.PACK_PAD + n // 2]) >> 4 == 7 and int(img[1, M.PACK_PAD + n // 2]) >> 4 == 7


@pytest.mark.parametrize("n", MODEL_LENGTHS)
def test_q2_window_at_any_position_is_four_aligned_dwords_of_its_copy_and_a_funnel_shift_of_copy_0(n):
    c = some_codes(n)
    c2 = M.two_bit(c)
    img = M.q2_image(c, 16)
    stride = M.q2_stride(n)
    assert img.shape == (16, stride) and stride % 128 == 0
    assert np.array_equal(img[:1], M.q2_image(c, 1))
    dw0 = img[0].view("<u4").astype(np.uint64)
    for pos in range(n):
        want = window(c2, pos, 64)
        byte = (pos >> 2) - ((pos >> 2) & 3)
        cp = (pos & 3) + 4 * ((pos >> 2) & 3)
        assert byte % 4 == 0 and byte + 16 <= stride, (n, pos)
        assert np.array_equal(bases_of(img[cp, byte:byte + 16]), want), (n, pos)
        w, sh = pos >> 4, 2 * (pos & 15)
        assert 4 * (w + 5) <= stride, (n, pos)
        five = dw0[w:w + 5]
        four = ((five[:4] >> np.uint64(sh)) | (five[1:] << np.uint64(32 - sh))) & np.uint64(0xFFFFFFFF)
        assert np.array_equal(bases_of(four.astype("<u4").view(np.uint8)), want), (n, pos)
    # zero where the first base of a dword lies past the end; Q2_TAIL zero bytes behind the last base of every copy
    for cp in range(16):
        last_byte = max((n - 1 - (cp & 3)) // 4 - (cp >> 2), -1)
        assert not img[cp, last_byte + 1:].any() and stride - (last_byte + 1) >= M.Q2_TAIL, (n, cp)


def test_codes_guards_rows_and_reverse_complement():
    a = np.arange(256, dtype=np.uint8)
    c = M.codes(a)
    for ch, v in zip("ACGTacgtnN&", (0, 1, 2, 3, 4, 4, 4, 4, 5, 5, 7)):
        assert c[ord(ch)] == v
    assert np.count_nonzero(c == 6) == 256 - 11
    assert list(M.rev_comp(np.array([0, 1, 2, 3, 4, 5, 6, 7], dtype=np.uint8))) == [7, 6, 5, 4, 0, 1, 2, 3]
    img, rows = M.seq_image(c), M.seq_image(c, rows=True)
    assert img.size == rows.size == 256 + 192
    assert np.all(img[:64] == 0x47) and np.all(img[320:] == 0x47) and np.all(rows[:64] == 0x78) and np.all(rows[320:] == 0x78)
    assert np.array_equal(rows[64:320], c << 3) and np.array_equal(img[64:320], c)
    # a guard reads as the separator in the buffer's own coding, with the terminator bit above it
    assert 0x47 & 7 == 7 and (0x78 >> 3) & 7 == 7 and 0x47 & 0x40 and 0x78 & 0x40
    assert M.presence(c) == 0xFF and M.presence(np.array([0, 0, 5], dtype=np.uint8)) == 0b100001 and M.presence(np.zeros(0, np.uint8)) == 0


def test_model_codes_equal_the_oracles(oracle):
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, 5000).astype(np.uint8)
    assert np.array_equal(M.codes(a), oracle.encode(a.tobytes()))
    c = M.codes(a)
    assert np.array_equal(M.rev_comp(c), oracle.rev_comp_codes(c))


# ---- class scores ---------------------------------------------------------------------------------------------------------
def matrices(oracle):
    return {"HOXD70": oracle.build_sub_mat(910), "simple": simple_matrix().reshape(64), "N above": B.n_matrix()}


def class_scores_as_written(m, pt, pq):
    """the rule once more, pair by pair, independent of image_model's list comprehension"""
    m = np.asarray(m).reshape(8, 8)
    cls = [-10 ** 9] * 4
    for r in range(4):
        for q in range(4):
            cls[r ^ q] = max(cls[r ^ q], int(m[r, q]))
    joins = -10 ** 9
    for r in range(8):
        for q in range(8):
            if r < 4 and q < 4:
                continue
            if (r >= 4 and not pt >> r & 1) or (q >= 4 and not pq >> q & 1):
                continue
            joins = max(joins, int(m[r, q]))
    return [max(v, joins, -255) for v in cls]


@pytest.mark.parametrize("name", ["HOXD70", "simple", "N above"])
def test_class_scores_bound_every_pair_of_present_codes_and_equal_the_rule(oracle, name):
    m = matrices(oracle)[name].reshape(8, 8)
    for hi_t in range(16):
        for hi_q in range(16):
            pt, pq = 0x0F | hi_t << 4, 0x0F | hi_q << 4
            cls = M.class_scores(m, pt, pq)
            assert cls == class_scores_as_written(m, pt, pq), (name, pt, pq)
            for r in range(8):
                for q in range(8):
                    if pt >> r & 1 and pq >> q & 1:
                        x = (r if r < 4 else 0) ^ (q if q < 4 else 0)
                        assert cls[x] >= m[r, q], (name, pt, pq, r, q)   # (the -255 floor only raises a score)
            # the A/C/G/T bits of a mask change nothing: those codes always count
            assert cls == M.class_scores(m, hi_t << 4, hi_q << 4)


def test_hoxd70_class_scores_without_other_codes_are_the_documented_ones(oracle):
    assert M.class_scores(oracle.build_sub_mat(910), 0x0F, 0x0F) == [100, -114, -31, -123]


# ---- the blocks are in their regimes --------------------------------------------------------------------------------------
def test_planted_letters_reach_every_place_in_every_kind():
    """over the blocks of all lengths: every special at base 0, at the last base, and at each of the four phases on either side of a base
    384 m and of the boundary between vector body and tail"""
    seen = set()
    for n in B.LENGTHS:
        v = B.LENGTHS.index(n)
        for variant, sparse in ((v, True), (v, False), (v + 5, True), (v + 9, False), (v + 11, True), (v + 13, False)):
            got = B.planted(n, variant, sparse)
            blk = B.block(n, variant, sparse)
            pl = B.places(n)
            for pos, name in pl.items():
                if (name, int(blk[pos])) in got and int(blk[pos]) in B.SPECIALS:
                    seen.add((name, int(blk[pos])))
    kinds = ["first", "last"] + ["%s%+d" % (k, o) for k in ("line", "tail") for o in range(-4, 4)]
    missing = [(k, s) for k in kinds for s in B.SPECIALS if (k, s) not in seen]
    assert not missing, missing
    assert {int(v) for v in M.codes(np.array(B.SPECIALS, dtype=np.uint8))} == {4, 5, 6, 7}


@pytest.mark.parametrize("n", [n for n in B.LENGTHS if n])
def test_blocks_of_a_length_keep_real_bases_at_the_edges_and_their_poison_differs_everywhere(n):
    for group in B.blocks_of(n):
        for blk in group:
            assert blk.size == n
            p = B.poison(blk)
            assert p.size > n + 1400 and not np.any(M.codes(p)[:n] == M.codes(blk))
            assert np.all(M.codes(p)[n:] != 0) and np.all(M.codes(p) < 4)
    sparse = B.blocks_of(n)[0][0]
    if n >= 15:
        assert np.count_nonzero(M.codes(sparse) < 4) > n // 2


def test_presence_blocks_hold_one_code_where_they_say():
    for name, (blk, code, pos) in B.presence_blocks().items():
        c = M.codes(blk)
        assert blk.size == B.PRESENCE_LEN and list(np.flatnonzero(c >= 4)) == [pos] and c[pos] == code, name
        body = B.PRESENCE_LEN - B.PRESENCE_LEN % 16
        assert ("tail" in name) == (body <= pos < B.PRESENCE_LEN - 1) or "last" in name or "first" in name, name
        assert "body" not in name or 0 < pos < body, name
        assert M.presence(c) == 0x0F | 1 << code


def test_large_blocks_wrap_the_loops_they_name():
    sweep = B.GRID_BLOCKS * B.BLOCK_THREADS
    n = B.LONG_QUERY
    assert (M.pack4_nbytes(n) + M.PACK4_FRONT) * M.PACK4_COPIES > sweep        # pack4_phase_kernel: a thread per byte of every copy
    assert 4 * M.ref2_nphys(n) > sweep                                         # pack2_phase_kernel: a thread per physical byte
    assert M.q2_stride(n) // 4 * 16 > sweep                                    # pack2_shifted_kernel: a thread per dword of every copy
    n = B.LONG_TARGET
    assert n // 16 > sweep and n % 16 == 1                                     # encode / row code / presence: a thread per 16 bytes
    t = B.long_target()
    c = M.codes(t)
    assert list(np.flatnonzero(c == 7)) == [(1 << 23) + 4321] and 16 * sweep <= (1 << 23) + 4321 < n - n % 16
    assert list(np.flatnonzero(c == 5)) == [n - 1]
    assert M.presence(c) == 0xFF


def test_island_case_hangs_on_the_n_bit(oracle):
    """the oracle keeps the HSP; under the full mask the class bound of every hit inside the island passes, without the N bit it falls
    below hspthresh with both sides dropped: the class filter would reject what it owes"""
    from helpers import Case
    ic = B.IslandCase()
    q = M.codes(ic.query)
    assert q.size % 16 == ic.TAIL and list(np.flatnonzero(q >= 4)) == list(range(*ic.n_run)) and ic.n_run[0] >= q.size - q.size % 16
    assert set(q[ic.n_run[0]:ic.n_run[1]]) == {5}
    m = B.n_matrix()
    acgt = m.reshape(8, 8)[:4, :4].max()
    assert m.reshape(8, 8)[5, 5] > acgt and m.reshape(8, 8)[4:6, :6].min() > acgt and m.reshape(8, 8)[:6, 4:6].min() > acgt and m.max() <= 127
    c = Case(ic.target, ic.query, chunk=1000, xdrop=ic.XDROP, hspthresh=ic.HSPTHRESH, noentropy=True, sub_mat=m).oracle_setup(oracle)
    (s, e), = c.chunks()
    want, st = c.oracle_saf(c.host_seeds(s, e, False), False)
    assert want.size >= 2 and all(tuple(int(v) for v in r) == ic.hsp for r in want[1:]), want
    t2, q2 = M.two_bit(M.codes(ic.target)), M.two_bit(q)
    pt, pq = M.presence(M.codes(ic.target)), M.presence(q)
    assert (pt, pq) == (0x0F, 0x2F)
    assert len(ic.anchors()) == ic.ISLAND - ic.SEED + 1
    for at, aq in ic.anchors():
        ok, rec, _ = oracle.extend_hit(c.o_ref, c.o_q, m, at, aq, xdrop=ic.XDROP, hspthresh=ic.HSPTHRESH, noentropy=True)
        assert ok and rec == ic.hsp
        full, _ = B.class_bound(t2, q2, M.class_scores(m, pt, pq), at, aq, ic.SEED, ic.XDROP)
        assert full >= ic.HSPTHRESH
        lost, dropped = B.class_bound(t2, q2, M.class_scores(m, pt, pq & ~(1 << 5)), at, aq, ic.SEED, ic.XDROP)
        assert lost <= 40 * ic.ISLAND < ic.HSPTHRESH and dropped, (at, aq, lost, dropped)
