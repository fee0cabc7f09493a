"""GPU: segalign_host --gpu_chain[=diag,anti] [--gpu_chain_gap=N].  Next to every .segments file a .chain file holds the best collinear
chain of every (target record, query record) pair of that file (sa_chain_hsps) in the .segments line format, in the
order the entry returns; it must equal the rendering of tests/hsp_chain_model.py on the file's HSPs.  With --gpu_gapped --gpu_maf the
.gapped and .maf files hold the alignments of the chains' HSPs alone, in their original order: GappedAlign on the model's members.
Without the flag the host writes what tests/host_model.py says, and with it every file it wrote before stays byte for byte."""
import bisect

import numpy as np
import pytest

import gapped_model as G
import gapped_trace_model as T
import hsp_chain_model as M
from helpers import Case
from host_model import Arena, expected_outputs, write_fasta
from segalign_amd import synth
from segalign_amd.build import build_host
from test_gpu_gapped_host import run
from test_gpu_gapped_maf_host import rc_text

pytestmark = pytest.mark.gpu

SEG_LINE = "%s\t%d\t%d\t%s\t%d\t%d\t%s\t%d\n"


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    """Two target records x two query records.  qry1 is chrA's copy with its halves swapped (two collinear lines, one chain takes
    one), then a piece of chrB's copy (a second group with chrB in the same file); qry2 is chrB's copy with inverted blocks."""
    d = tmp_path_factory.mktemp("chain_host")
    a, b = synth.random_dna(40000, 981), synth.random_dna(30000, 982)
    ma, mb = synth.mutate(a, 983, 0.07, indel_every=500), synth.mutate(b, 984, 0.07, indel_every=500)
    h = ma.size // 2
    t_recs = [("chrA", a), ("chrB", b)]
    q_recs = [("qry1", np.concatenate([ma[h:], ma[:h], mb[:8000]])), ("qry2", synth.invert_blocks(mb, 985, block=5000, frac=0.4))]
    tf, qf = d / "target.fa", d / "query.fa"
    write_fasta(tf, t_recs)
    write_fasta(qf, q_recs)
    R = Arena([(n, s.tobytes()) for n, s in t_recs], 500_000_000, 19, 10_000_000, False)
    Q = Arena([(n, s.tobytes()) for n, s in q_recs], 500_000_000, 19, 10_000_000, True)
    return d, tf, qf, t_recs, q_recs, R, Q


def file_hsps(text, rev, R, Q):
    """A .segments file's HSPs in the host's vector order (block coordinates), and each one's (target record, query record)."""
    names, starts = (Q.rc_name, Q.rc_start) if rev else (Q.chr_name, Q.chr_start)
    hsps, recs = [], []
    for line in text.splitlines():
        rn, rs, re_, qn, qs, _, _, sc = line.split("\t")
        ri, qi = R.chr_name.index(rn), names.index(qn)
        hsps.append((R.chr_start[ri] + int(rs) - 1, starts[qi] + int(qs) - 1, int(re_) - int(rs), int(sc)))
        recs.append((ri, qi))
    if rev:  # the file holds the minus-strand vector in reverse order
        hsps, recs = hsps[::-1], recs[::-1]
    pairs = sorted(set(recs))
    return np.array(hsps, dtype=M.SEG), np.array([pairs.index(p) for p in recs], dtype=np.uint32)


def seg_line(R, names, starts, rev, r0, r1, q0, q1, score):
    """One line for block coordinates [r0, r1) x [q0, q1)."""
    ri, qi = bisect.bisect_right(R.chr_start, r0) - 1, bisect.bisect_right(starts, q0) - 1
    return SEG_LINE % (R.chr_name[ri], r0 + 1 - R.chr_start[ri], r1 - R.chr_start[ri], names[qi], q0 + 1 - starts[qi], q1 - starts[qi],
                       "-" if rev else "+", score)


def chain_text(h, members, rev, R, Q):
    names, starts = (Q.rc_name, Q.rc_start) if rev else (Q.chr_name, Q.chr_start)
    out = []
    for k in members["hsp_index"].tolist():
        r0, q0, ln, sc = (int(x) for x in h[k].tolist())
        out.append(seg_line(R, names, starts, rev, r0, r0 + ln + 1, q0, q0 + ln + 1, sc))
    return "".join(out)


def check_chain_files(got, base, R, Q, **kw):
    """Every .chain file of `got` against the model on the .segments file beside it; every other file as in `base`.
    -> {segments file: (hsps, the model's members)}"""
    segs = sorted(f for f in base if f.endswith(".segments"))
    assert segs and sorted(got) == sorted(list(base) + [f[:-len("segments")] + "chain" for f in segs])
    assert all(got[f] == base[f] for f in base if not f.endswith((".gapped", ".maf")))
    res, dropped, groups = {}, 0, 0
    for f in segs:
        rev = ".minus." in f
        h, g = file_hsps(got[f], rev, R, Q)
        _, _, members = M.chain(h, g, **kw)
        assert got[f[:-len("segments")] + "chain"] == chain_text(h, members, rev, R, Q), f
        res[f] = (h, members)
        dropped += h.size - members.size
        groups = max(groups, int(g.max()) + 1)
    assert dropped > 0 and groups >= 2, "the input must leave HSPs off the chains and hold two record pairs in one file"
    return res


def test_host_writes_chain_files(oracle, pair):
    d, tf, qf, t_recs, q_recs, R, Q = pair
    exe = build_host()
    plain, plain_out = run(exe, tf, qf, d / "plain", [])
    files, cmds = expected_outputs(oracle, [(n, s.tobytes()) for n, s in t_recs], [(n, s.tobytes()) for n, s in q_recs], chunk=20000)
    assert plain == files and plain_out == sorted(cmds + [""])  # without the flag: the reference host's files and lines
    got, got_out = run(exe, tf, qf, d / "chain", ["--gpu_chain"])
    assert got_out == plain_out
    res = check_chain_files(got, plain, R, Q)
    assert any(".minus." in f and m.size for f, (_, m) in res.items()) and any(".plus." in f and m.size for f, (_, m) in res.items())


def test_host_aligns_the_chains_only(engine, pair):
    d, tf, qf, t_recs, q_recs, R, Q = pair
    exe = build_host()
    flags = ["--gpu_gapped", "--gpu_maf"]
    base, base_out = run(exe, tf, qf, d / "gapped", flags)
    got, got_out = run(exe, tf, qf, d / "chain_gapped", flags + ["--gpu_chain=2,1", "--gpu_chain_gap=3000"])
    assert got_out == base_out
    res = check_chain_files(got, base, R, Q, diag_pen=2, anti_pen=1, max_gap=3000)

    E = engine
    target = np.frombuffer(bytes(R.buf[:R.block_len[0]]), dtype=np.uint8)
    query = np.frombuffer(bytes(Q.buf[:Q.block_len[0]]), dtype=np.uint8)
    Case(target, query, chunk=20000, sub_mat=G.SUB).engine_setup(E, num_gpu=1)
    r_text, q_text = target.tobytes().decode(), query.tobytes().decode()
    fasta = {n: s.tobytes().decode() for n, s in t_recs + q_recs}
    n_blocks = fewer = 0
    try:
        for f, (h, members) in res.items():
            rev = ".minus." in f
            names, starts = (Q.rc_name, Q.rc_start) if rev else (Q.chr_name, Q.chr_start)
            qt = rc_text(q_text) if rev else q_text
            keep = np.sort(members["hsp_index"])  # the chains' HSPs in their original relative order
            recs, paths, ops, _ = E.GappedAlign(h[keep].astype(E.SEG_DTYPE), rev, 0)
            lines, blocks = [], []
            for a, p in zip(recs.tolist(), paths.tolist()):
                r0, r1, q0, q1, score = a[:5]
                lines.append(seg_line(R, names, starts, rev, r0, r1, q0, q1, score))
                ri, qi = bisect.bisect_right(R.chr_start, r0) - 1, bisect.bisect_right(starts, q0) - 1
                ta, qa = T.maf_texts(r_text, qt, r0, q0, ops[p[0]:p[0] + p[1] + p[2]])
                blocks.append("a score=%d\ns %s %d %d + %d %s\ns %s %d %d %s %d %s\n\n" % (
                    score, R.chr_name[ri], r0 - R.chr_start[ri], r1 - r0, len(fasta[R.chr_name[ri]]), ta,
                    names[qi], q0 - starts[qi], q1 - q0, "-" if rev else "+", len(fasta[names[qi]]), qa))
            if rev:
                lines, blocks = lines[::-1], blocks[::-1]
            stem = f[:-len("segments")]
            assert got[stem + "gapped"] == "".join(lines), f
            assert got[stem + "maf"] == "".join(blocks), f
            n_blocks += len(blocks)
            fewer += got[stem + "gapped"] != base[stem + "gapped"]
    finally:
        E.ShutdownProcessor()
    assert n_blocks > 0 and fewer > 0, "the chains must change at least one file's alignments"
