"""GPU: option gapped_pieces (continuation of sides that end at max_extent; include/segalign_amd.h) against the model
of tests/gapped_pieces_model.py: the three gapped entries at gapped_pieces = 1 set explicitly, raw records, paths and counts at
P = 2, 3 and 64, selection mode, the flags of every way a chain ends, greedy over pieces, trace batching, concurrency and the host."""
import bisect
import contextlib
import functools
import threading

import numpy as np
import pytest

import gapped_model as G
import gapped_pieces_model as PM
import gapped_trace_model as T
from gapped_model import SUB
from helpers import Case
from test_gapped_pieces_checker import later_piece_pair

pytestmark = pytest.mark.gpu

SETS = {"chain": PM.CHAIN, "dry": PM.DRY, "band": PM.BAND}
PIECES = (2, 3, 64)


def setup(E):
    t, qs = PM.block_pair()
    Case(t, qs[0], chunk=100_000, sub_mat=SUB).engine_setup(E, num_gpu=1)
    E.SendQueryWriteRequest(qs[1], 0, qs[1].size, 1)


@contextlib.contextmanager
def options(E, **opts):
    """The engine restarted under the given options; on leaving, restarted with them reset."""
    E.ShutdownProcessor()
    try:
        for k, v in opts.items():
            E.set_option(k, v)
        setup(E)
        yield
    finally:
        E.ShutdownProcessor()
        for k in opts:
            E.lib().sa_reset_option(k.encode())
        setup(E)


@pytest.fixture(scope="module")
def pcase(engine):
    E = engine
    setup(E)
    _, _, tc, codes, hsps = PM.inputs()
    assert np.array_equal(E.copy_ref_codes(), tc)
    for buf, rev in PM.KEYS:
        assert np.array_equal(E.copy_query_codes(buf, rev), codes[(buf, rev)])
    yield E, tc, codes, hsps
    E.ShutdownProcessor()


@functools.lru_cache(maxsize=None)
def model(name, key, pieces):
    """(raw records, paths, sides) of the model for parameter set `name` on strand `key`."""
    _, _, tc, codes, hsps = PM.inputs()
    return PM.align(tc, codes[key], SUB, hsps[key], pieces, **SETS[name])


def test_inputs_reach_every_stop_reason_and_long_chains(pcase):
    """On the CPU, with the model: a vacuous input fails here."""
    _, tc, codes, _ = pcase
    seen, longest, ends, lengths = {}, 0, set(), set()
    for name in SETS:
        for key in PM.KEYS:
            for pieces in PIECES:
                recs, _, sides = model(name, key, pieces)
                s, n = PM.stop_reasons(sides)
                longest = max(longest, n)
                lengths |= {len(x[1]) for pair in sides for x in pair}
                for a, b in s.items():
                    seen[a] = seen.get(a, 0) + b
                for r, (L, R) in zip(recs, sides):
                    ends |= {PM.end_kind(tc, codes[key], r, d) for d, S in ((-1, L), (1, R)) if S[2] == PM.STOP_END}
    assert {PM.STOP_P, PM.STOP_BAND, PM.STOP_STUCK, PM.STOP_END} <= set(seen), seen
    assert {"separator", "block end"} <= ends
    assert longest >= 8 and {2, 3} <= lengths and max(lengths) > 10


def three_entries(E, h, rev, buf, **kw):
    return (E.GappedExtend(h, rev, buf, raw=True, **kw)[0], E.GappedExtend(h, rev, buf, **kw)[0], *E.GappedAlign(h, rev, buf, raw=True, **kw)[:3],
            *E.GappedAlign(h, rev, buf, **kw)[:3], *E.GappedAlignGreedy(h, rev, buf, **kw)[:3])


def test_one_piece_set_explicitly_is_the_default(pcase):
    E, tc, codes, hsps = pcase
    assert E.get_option("gapped_pieces") == 1
    jobs = [(hsps[(buf, rev)], rev, buf, kw) for (buf, rev), kw in zip(PM.KEYS, (PM.CHAIN, PM.DRY, PM.BAND, {}))]
    want = [three_entries(E, h, rev, buf, **kw) for h, rev, buf, kw in jobs]
    with options(E, gapped_pieces=1):
        got = [three_entries(E, h, rev, buf, **kw) for h, rev, buf, kw in jobs]
    for g, w in zip(got, want):
        assert len(g) == len(w) and all(np.array_equal(a, b) for a, b in zip(g, w))
    # and the default is the one-piece model: no record is continued
    assert np.array_equal(want[0][0], model("chain", PM.KEYS[0], 1)[0]) and not np.any(want[0][0]["flags"] & PM.CONTINUED)
    assert E.get_option("gapped_pieces") == 1


@pytest.mark.parametrize("pieces", PIECES)
def test_raw_records_and_paths_equal_the_model(pcase, pieces):
    E, tc, codes, hsps = pcase
    with options(E, gapped_pieces=pieces):
        assert E.get_option("gapped_pieces") == pieces
        for name, kw in SETS.items():
            for key in PM.KEYS:
                buf, rev = key
                h = hsps[key]
                want, wpaths, sides = model(name, key, pieces)
                ext, est = E.GappedExtend(h, rev, buf, raw=True, **kw)
                assert np.array_equal(ext, want), (name, key, ext[:3], want[:3])  # score, extents, flags, cells of every record
                recs, paths, ops, st = E.GappedAlign(h, rev, buf, raw=True, **kw)
                assert np.array_equal(recs, want)
                wp, wops = T.pack(wpaths)
                assert np.array_equal(paths, wp), (name, key)  # n_left / n_right and the counts
                assert np.array_equal(ops, wops), (name, key)  # op for op
                # selection mode: both entries, and the rules applied to the raw records
                sel = G.select(want, 3000)
                srecs, spaths, sops, _ = E.GappedAlign(h, rev, buf, **kw)
                assert np.array_equal(E.GappedExtend(h, rev, buf, **kw)[0], sel) and np.array_equal(srecs, sel)
                sp, so = T.pack([wpaths[int(r["hsp_index"])] for r in sel])
                assert np.array_equal(spaths, sp) and np.array_equal(sops, so)
                # what the flags say about how each chain ended
                for k, (L, R) in enumerate(sides):
                    for joined, chain, stop in (L, R):
                        if stop == PM.STOP_P:
                            assert joined[4] & PM.EXTENT_CAP and joined[4] & PM.CONTINUED
                        if stop == PM.STOP_END:  # a separator, the block's end or the y-drop
                            assert joined[4] & PM.CONTINUED and not joined[4] & PM.EXTENT_CAP
                    assert int(recs[k]["flags"]) == L[0][4] | R[0][4]
                assert est["extent_capped"] == int(np.count_nonzero(want["flags"] & PM.EXTENT_CAP))


def greedy_input(hsps, key, tc, codes):
    """A strand's anchors, a few of them twice, and on strand (0, +) the pair of test_gapped_pieces_checker.later_piece_pair."""
    h = hsps[key]
    h = np.concatenate([h, h[::5]])
    if key == PM.KEYS[0]:
        h = np.concatenate([later_piece_pair(tc, codes, hsps)[0], h])
    return h


def check_greedy(E, tc, codes, hsps, pieces, keys, kw):
    for key in keys:
        buf, rev = key
        h = greedy_input(hsps, key, tc, codes)
        got = E.GappedAlignGreedy(h, rev, buf, **kw)
        sel, sel_paths, want = PM.greedy(tc, codes[key], SUB, h, 3000, pieces, **kw)
        recs, paths, ops, st = got
        assert np.array_equal(recs, sel), (key, recs[:3], sel[:3])
        wp, wops = T.pack(sel_paths)
        assert np.array_equal(paths, wp) and np.array_equal(ops, wops)
        assert (st["returned"], st["covered"], st["below_thresh"]) == (want["returned"], want["covered"], want["below_thresh"])
        assert want["covered"] > 0
        # every returned record and path is raw mode's for its HSP under the same gapped_pieces
        rrecs, rpaths, rops, _ = E.GappedAlign(h, rev, buf, raw=True, **kw)
        for k in range(recs.size):
            i = int(recs[k]["hsp_index"])
            assert recs[k] == rrecs[i]
            for a, b in zip(T.record_ops(paths, ops, k), T.record_ops(rpaths, rops, i)):
                assert np.array_equal(a, b)


def test_greedy_equals_the_model_at_every_batch_size(pcase):
    E, tc, codes, hsps = pcase
    pair, qc = later_piece_pair(tc, codes, hsps)
    # one piece: the first alignment ends before the second anchor, which is extended and returned
    recs, _, _, st = E.GappedAlignGreedy(pair, False, 0, **PM.CHAIN)
    assert recs.size == 2 and st["covered"] == 0
    for pieces, batch in ((64, None), (64, 1), (64, 3), (64, 1 << 20), (3, 3)):
        opts = dict(gapped_pieces=pieces, **({} if batch is None else {"gapped_greedy_batch": batch}))
        with options(E, **opts):
            check_greedy(E, tc, codes, hsps, pieces, PM.KEYS if batch is None else PM.KEYS[:2], PM.CHAIN)
            if batch in (None, 3):
                check_greedy(E, tc, codes, hsps, pieces, PM.KEYS[2:], PM.DRY)
            if pieces == 64:  # the second anchor lies on a later piece of the first alignment: covered
                recs, _, _, st = E.GappedAlignGreedy(pair, False, 0, **PM.CHAIN)
                assert recs.size == 1 and int(recs[0]["hsp_index"]) == 0 and st["covered"] == 1
                assert recs[0]["flags"] & PM.CONTINUED


def test_trace_budget_of_one_mib_gives_identical_results(pcase):
    E, tc, codes, hsps = pcase
    key = PM.KEYS[3]
    h = np.concatenate([hsps[key], hsps[key]])
    with options(E, gapped_pieces=64):
        want = E.GappedAlign(h, True, 1, raw=True, **PM.CHAIN)
        wantg = E.GappedAlignGreedy(h, True, 1, **PM.CHAIN)
    with options(E, gapped_pieces=64, gapped_trace_mb=1):
        got = E.GappedAlign(h, True, 1, raw=True, **PM.CHAIN)
        gotg = E.GappedAlignGreedy(h, True, 1, **PM.CHAIN)
    assert want[3]["trace_batches"] < got[3]["trace_batches"] and got[3]["trace_bytes"] == want[3]["trace_bytes"]
    for a, b in zip(got[:3] + gotg[:3], want[:3] + wantg[:3]):
        assert np.array_equal(a, b)
    assert np.array_equal(want[0][:hsps[key].size], model("chain", key, 64)[0])


def test_concurrent_callers_get_the_serial_results(pcase):
    E, tc, codes, hsps = pcase
    with options(E, gapped_pieces=16):
        jobs = []
        for k in range(6):
            key = PM.KEYS[k % 4]
            jobs.append((k % 3, hsps[key], key[1], key[0], dict(max_extent=700 + 300 * k)))

        def call(kind, h, rev, buf, kw):
            if kind == 0:
                return (E.GappedExtend(h, rev, buf, raw=True, **kw)[0],)
            if kind == 1:
                return E.GappedAlign(h, rev, buf, **kw)[:3]
            return E.GappedAlignGreedy(h, rev, buf, **kw)[:3]

        serial = [call(*j) for j in jobs]
        assert any(np.any(s[0]["flags"] & PM.CONTINUED) for s in serial)
        results = [None] * len(jobs)

        def run(i):
            for _ in range(3):
                r = call(*jobs[i])
                if results[i] is None or all(np.array_equal(a, b) for a, b in zip(results[i], r)):
                    results[i] = r
                else:
                    results[i] = "differs"
        th = [threading.Thread(target=run, args=(i,)) for i in range(len(jobs))]
        for t in th:
            t.start()
        for t in th:
            t.join()
        for i in range(len(jobs)):
            assert results[i] != "differs" and all(np.array_equal(a, b) for a, b in zip(results[i], serial[i])), i


def test_host_writes_continued_alignments(tmp_path):
    """segalign_host --gpu_gapped --gpu_maf --gpu_max_extent=2000 --gpu_pieces=N: the .gapped and .maf files equal those rendered from
    the model; without --gpu_pieces they are byte for byte those of --gpu_pieces=1."""
    from host_model import Arena, write_fasta
    from segalign_amd import synth
    from segalign_amd.build import build_host
    from test_gpu_gapped_host import encode, rc_codes, run
    from test_gpu_gapped_maf_host import rc_text

    t_recs = [("chrA", synth.random_dna(40000, 961)), ("chrB", synth.random_dna(30000, 962))]
    q_recs = [("qry%d" % (i + 1), synth.mutate(s, 970 + i, 0.06, indel_every=400)) for i, (_, s) in enumerate(t_recs)]
    tf, qf = tmp_path / "target.fa", tmp_path / "query.fa"
    write_fasta(tf, t_recs)
    write_fasta(qf, q_recs)
    exe = build_host()
    base = ["--gpu_gapped", "--gpu_maf", "--gpu_max_extent=2000"]
    plain, plain_out = run(exe, tf, qf, tmp_path / "plain", base)
    one, one_out = run(exe, tf, qf, tmp_path / "one", base + ["--gpu_pieces=1"])
    assert plain == one and plain_out == one_out

    R = Arena([(n, s.tobytes()) for n, s in t_recs], 500_000_000, 19, 10_000_000, False)
    Q = Arena([(n, s.tobytes()) for n, s in q_recs], 500_000_000, 19, 10_000_000, True)
    t_codes = encode(R.buf[:R.block_len[0]])
    q_codes = encode(Q.buf[:Q.block_len[0]])
    r_text = bytes(R.buf[:R.block_len[0]]).decode()
    q_text = bytes(Q.buf[:Q.block_len[0]]).decode()
    fasta = {n: s.tobytes().decode() for n, s in t_recs + q_recs}
    for pieces, files in ((1, plain), (8, run(exe, tf, qf, tmp_path / "eight", base + ["--gpu_pieces=8"])[0])):
        assert all(files[f] == plain[f] for f in plain if f.endswith(".segments"))
        n_lines = continued = 0
        for f in sorted(x for x in files if x.endswith(".gapped")):
            rev = ".minus." in f
            names, starts = (Q.rc_name, Q.rc_start) if rev else (Q.chr_name, Q.chr_start)
            hsps = []
            for line in files[f[:-len("gapped")] + "segments"].splitlines():
                rn, rs, re_, qn, qs, qe, _, sc = line.split("\t")
                ri, qi = R.chr_name.index(rn), names.index(qn)
                hsps.append((R.chr_start[ri] + int(rs) - 1, starts[qi] + int(qs) - 1, int(re_) - int(rs), int(sc)))
            if rev:
                hsps = hsps[::-1]
            h = np.array(hsps, dtype=G.SEG_DTYPE)
            qc = rc_codes(q_codes) if rev else q_codes
            qt = rc_text(q_text) if rev else q_text
            raw, paths, _ = PM.align(t_codes, qc, G.SUB, h, pieces, max_extent=2000)
            sel, sel_paths = T.select(raw, paths, 3000)
            continued += int(np.count_nonzero(sel["flags"] & PM.CONTINUED))
            lines, blocks = [], []
            for a, (lo, ro, _) in zip(sel.tolist(), sel_paths):
                r0, r1, q0, q1, score = a[0], a[1], a[2], a[3], a[4]
                ri = bisect.bisect_right(R.chr_start, r0) - 1
                qi = bisect.bisect_right(starts, q0) - 1
                lines.append("%s\t%d\t%d\t%s\t%d\t%d\t%s\t%d\n" % (R.chr_name[ri], r0 + 1 - R.chr_start[ri], r1 - R.chr_start[ri], names[qi],
                                                                 q0 + 1 - starts[qi], q1 - starts[qi], "-" if rev else "+", score))
                ta, qa = T.maf_texts(r_text, qt, r0, q0, np.concatenate([lo, ro]))
                blocks.append("a score=%d\ns %s %d %d + %d %s\ns %s %d %d %s %d %s\n\n" % (
                    score, R.chr_name[ri], r0 - R.chr_start[ri], r1 - r0, len(fasta[R.chr_name[ri]]), ta,
                    names[qi], q0 - starts[qi], q1 - q0, "-" if rev else "+", len(fasta[names[qi]]), qa))
            if rev:
                lines, blocks = lines[::-1], blocks[::-1]
            assert files[f] == "".join(lines), (pieces, f)
            assert files[f[:-len("gapped")] + "maf"] == "".join(blocks), (pieces, f)
            n_lines += len(lines)
        assert n_lines > 0 and (continued > 0) == (pieces > 1)
