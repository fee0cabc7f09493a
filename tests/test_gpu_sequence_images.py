"""GPU: every byte of every image the send entries build from a block -- encode_kernel, rev_comp_codes_kernel, row_code_kernel, the
three packers and code_presence_kernel (encode.hip) behind SeqBuf / PackedBuf (engine_internal.h) -- read back whole through the test
entry sa_copy_image and compared with tests/image_model.py: codes with their guards, the row-coded target, the overlapped lines of the
target's 2-bit phase copies, the eight 4-bit copies of either strand with their pads, the shifted 2-bit copies with their zero tails,
the repeat masker's five, the presence masks and the class scores made of them (DESIGN.md 4.1').  Every block is sent behind a longer
block of complementary content in the same grow-only buffers and again after a clear.  tests/test_image_model.py shows on the CPU that
the model is what the consumers address and that every block of tests/image_blocks.py is in the regime it names."""
import numpy as np
import pytest

import image_blocks as B
import image_model as M
from extend_regimes import simple_matrix
from helpers import Case, seg_equal

pytestmark = pytest.mark.gpu

SHAPE = "TTT0T00TT00T0T0TTTT"
TARGET_IMAGES = ("ref", "ref8", "ref2")
QUERY_IMAGES = ("query", "query_rc", "query4", "query4_rc", "query2", "query2_rc")
RM_IMAGES = ("ref_rc", "ref4", "ref4_rc", "refq2", "refq2_rc")
_state = {"mode": None}


def ready(E, one_copy_option, sub_mat=None):
    """an interface and a processor under option cls_one_copy, set up once for all the tests that share it: the buffers then carry
    what earlier tests left in them, as they do in a run over many blocks"""
    key = (one_copy_option, None if sub_mat is None else bytes(np.asarray(sub_mat, np.int32)))
    if _state["mode"] != key:
        E.ShutdownProcessor()
        E.reset_option(None)
        E.set_option("cls_one_copy", one_copy_option)
        E.InitializeInterface(1)
        assert E.GenerateShapePos(SHAPE) == 12
        E.InitializeProcessor(True, 1000, len(SHAPE), B.n_matrix() if sub_mat is None else sub_mat, 910, 3000, True)
        _state["mode"] = key
    return 16 if one_copy_option == 2 else 1


@pytest.fixture(scope="module", autouse=True)
def leave_nothing_behind(engine):
    yield
    engine.ClearRef()
    engine.ShutdownProcessor()
    engine.reset_option(None)
    _state["mode"] = None


def hold(E, name, block, buffer=0, copies=1):
    """one image against the model: geometry, then every byte of the span"""
    got = E.copy_image(name, buffer)
    assert got is not None, (name, buffer, "not resident")
    info, data = got
    geo, want = M.expected(name, M.codes(block), copies)
    assert info == geo, (name, buffer, info, geo)
    bad = np.flatnonzero(data != want)
    if bad.size:
        at = int(bad[0])
        copy, off = divmod(at, geo["stride"])
        raise AssertionError("%s of buffer %d, %d bases: %d bytes differ, the first at copy %d byte %d (span offset %d): device 0x%02x, model 0x%02x"
                             % (name, buffer, block.size, bad.size, copy, off - geo["origin"], at, data[at], want[at]))


def hold_target(E, block):
    for name in TARGET_IMAGES:
        hold(E, name, block)
    assert E.code_presence()[0] == M.presence(M.codes(block)), block.size
    assert np.array_equal(E.copy_ref_codes(), M.codes(block))


def hold_query(E, block, buffer, copies):
    for name in QUERY_IMAGES:
        hold(E, name, block, buffer, copies)
    assert E.code_presence()[1][buffer] == M.presence(M.codes(block)), (block.size, buffer)


def send_target(E, block):
    return E.SendRefWriteRequest(block, 0, block.size)


def send_query(E, block, buffer):
    E.SendQueryWriteRequest(block, 0, block.size, buffer)


def missing(E, names, buffer=0):
    return [E.copy_image(name, buffer) for name in names] == [None] * len(names)


@pytest.mark.parametrize("option,n", [(o, n) for o in (0, 2) for n in B.LENGTHS],
                         ids=["%d bases, %s" % (n, "sixteen 2-bit copies" if o else "one 2-bit copy") for o in (0, 2) for n in B.LENGTHS])
def test_images_of_a_block_behind_a_longer_one_and_after_a_clear(engine, n, option):
    E = engine
    copies = ready(E, option)
    (t1, a1, b1), (t2, a2, b2) = B.blocks_of(n)
    # behind a longer block of complementary content, in the same buffers
    send_target(E, B.poison(t1))
    send_query(E, B.poison(a1), 0)
    send_query(E, B.poison(b1), 1)
    send_target(E, t1)
    send_query(E, a1, 0)
    send_query(E, b1, 1)
    hold_target(E, t1)
    hold_query(E, a1, 0, copies)
    hold_query(E, b1, 1, copies)
    # cleared: gone; the other buffer stays
    E.ClearRef()
    E.ClearQuery(0)
    assert missing(E, TARGET_IMAGES) and missing(E, QUERY_IMAGES, 0)
    hold_query(E, b1, 1, copies)
    # after the clear: other blocks of the same length
    send_target(E, t2)
    send_query(E, a2, 0)
    hold_target(E, t2)
    hold_query(E, a2, 0, copies)
    hold_query(E, b1, 1, copies)        # untouched by the target and by buffer 0
    send_query(E, b2, 1)
    hold_query(E, b2, 1, copies)
    hold_query(E, a2, 0, copies)        # ... and the other way round
    hold_target(E, t2)


@pytest.mark.parametrize("kind", ["lower case", "separators"])
def test_blocks_without_a_single_plain_base(engine, kind):
    E = engine
    copies = ready(E, 2)
    block = B.lower_case(777) if kind == "lower case" else B.uniform(777, "&")
    send_target(E, B.poison(block))
    send_query(E, B.poison(block), 0)
    send_target(E, block)
    send_query(E, block, 0)
    hold_target(E, block)
    hold_query(E, block, 0, copies)
    assert E.code_presence()[0] == (1 << 4 if kind == "lower case" else 1 << 7)


@pytest.mark.parametrize("n", B.RM_LENGTHS)
def test_repeat_masker_images_behind_a_longer_target(engine, n):
    E = engine
    copies = ready(E, 2)
    E.RmClearQuery()
    assert missing(E, RM_IMAGES)                    # before sa_rm_send_query_write_request: none of the five
    t1, t2 = B.blocks_of(n)[0][0], B.blocks_of(n)[1][0]
    send_target(E, B.poison(t1))
    E.RmSendQueryWriteRequest()
    for name in RM_IMAGES:
        hold(E, name, B.poison(t1), copies=copies)
    send_target(E, t1)                              # a shorter target, and the second call
    E.RmSendQueryWriteRequest()
    for name in RM_IMAGES:
        hold(E, name, t1, copies=copies)
    hold_target(E, t1)
    send_target(E, t2)
    E.RmSendQueryWriteRequest()
    for name in RM_IMAGES:
        hold(E, name, t2, copies=copies)
    E.RmClearQuery()
    assert missing(E, RM_IMAGES)
    hold_target(E, t2)


def test_long_block_wraps_the_loops_of_the_packers(engine):
    E = engine
    copies = ready(E, 2)
    assert copies == 16
    block = B.long_query()
    p = B.poison(block)
    send_target(E, p)
    send_query(E, p, 0)
    send_target(E, block)
    send_query(E, block, 0)
    hold_target(E, block)
    hold_query(E, block, 0, copies)


def test_long_target_wraps_the_loops_of_the_encoder_the_row_coder_and_the_presence_kernel(engine):
    E = engine
    ready(E, 0)
    block = B.long_target()
    send_target(E, B.poison(block))
    assert E.code_presence()[0] == 0x0F
    send_target(E, block)
    hold_target(E, block)
    assert E.code_presence()[0] == 0xFF
    send_target(E, B.plain(100, 1))                 # (and leave a small target behind)


# ---- presence ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(B.presence_blocks()))
def test_presence_of_one_code_in_one_place(engine, name):
    E = engine
    ready(E, 0)
    block, code, pos = B.presence_blocks()[name]
    everything = np.frombuffer(b"ACGTgNR&" * 8, dtype=np.uint8)
    for send, slot in ((send_target, None), (lambda E, b: send_query(E, b, 0), 0), (lambda E, b: send_query(E, b, 1), 1)):
        send(E, everything)                          # every bit set: the ones the block lacks must disappear
        masks = E.code_presence()
        assert (masks[0] if slot is None else masks[1][slot]) == 0xFF
        send(E, block)
        masks = E.code_presence()
        assert (masks[0] if slot is None else masks[1][slot]) == 0x0F | 1 << code, (name, slot)


def test_presence_slots_are_independent(engine):
    E = engine
    ready(E, 0)
    P = B.presence_blocks()
    send_target(E, P["code 4 tail"][0])
    send_query(E, P["code 5 tail"][0], 0)
    send_query(E, P["code 6 body"][0], 1)
    assert E.code_presence() == (0x1F, [0x2F, 0x4F])
    send_query(E, B.plain(45, 2), 0)                 # the N bit of buffer 0 goes, nothing else moves
    assert E.code_presence() == (0x1F, [0x0F, 0x4F])
    send_target(E, P["code 7 last"][0])
    assert E.code_presence() == (0x8F, [0x0F, 0x4F])
    send_query(E, P["code 7 first"][0], 1)
    assert E.code_presence() == (0x8F, [0x0F, 0x8F])
    send_query(E, np.zeros(0, dtype=np.uint8), 0)    # an empty block holds no code at all
    assert E.code_presence() == (0x8F, [0x00, 0x8F])


@pytest.mark.parametrize("name", ["HOXD70", "simple", "N above"])
def test_class_scores_of_the_resident_matrix_equal_the_rule(engine, oracle, name):
    E = engine
    m = {"HOXD70": oracle.build_sub_mat(910), "simple": simple_matrix().reshape(64), "N above": B.n_matrix()}[name]
    ready(E, 0, sub_mat=m)
    for hi_t in range(16):
        for hi_q in range(16):
            for low in (0x0F, 0x00, 0x05):           # (the A/C/G/T bits of a mask count for nothing)
                pt, pq = hi_t << 4 | low, hi_q << 4 | low
                assert E.class_scores(pt, pq) == M.class_scores(m, pt, pq), (name, pt, pq)


# ---- why presence exists ------------------------------------------------------------------------------------------------------
def test_real_call_keeps_the_hsp_that_hangs_on_an_n_in_the_scalar_tail(engine, oracle):
    """tests/image_blocks.py IslandCase under the matrix that scores N pairs above every A/C/G/T pair: the query's only N lie in its last
    len % 16 bytes, and without their bit in the mask the class filter's bound of every hit inside the island stays below hspthresh
    (tests/test_image_model.py shows that on the CPU).  The call returns the oracle's HSPs and its audit holds no hit the oracle keeps."""
    E = engine
    ic = B.IslandCase()
    E.ShutdownProcessor()
    E.reset_option(None)
    _state["mode"] = None
    E.set_option("audit_cap", 1 << 16)
    try:
        c = Case(ic.target, ic.query, chunk=1000, xdrop=ic.XDROP, hspthresh=ic.HSPTHRESH, noentropy=True, sub_mat=B.n_matrix())
        c.oracle_setup(oracle).engine_setup(E)
        assert E.lookup_mode() == 2
        assert E.code_presence()[0] == 0x0F and E.code_presence()[1][0] == 0x2F
        hold_query(E, ic.query, 0, 1)
        (s, e), = c.chunks()
        want, _ = c.oracle_saf(c.host_seeds(s, e, False), False)
        assert want.size >= 2 and tuple(int(v) for v in want[1]) == ic.hsp
        got = E.SeedAndFilterRange(s, e, False, 0)
        assert seg_equal(got, want), (got, want)
        st = E.last_call_stats()
        assert st["lookup_path"] == 2 and st["num_hits"] >= len(ic.anchors()), st
        pairs, n = E.get_audit()
        assert n == pairs.shape[0]
        ok, recs = oracle.extend_hits_pass(c.o_ref, c.o_q, c.sub_mat, pairs, xdrop=ic.XDROP, hspthresh=ic.HSPTHRESH, noentropy=True)
        assert not ok.any(), (pairs[ok][:5], recs[ok][:5])
    finally:
        E.ShutdownProcessor()
        E.reset_option(None)
