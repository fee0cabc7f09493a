"""GPU: segalign_host --gpu_gapped --gpu_skip_covered [--gpu_maf].  The .gapped and .maf files hold sa_gapped_align_greedy's
alignments; they must equal files built from the sequential rule (tests/gapped_greedy_model.py) over the serial path checker on the
same HSPs.  The .segments files and stdout stay what a --gpu_gapped run writes."""
import bisect

import numpy as np
import pytest

import gapped_greedy_model as GR
import gapped_model as G
import gapped_trace_model as T
from host_model import Arena, write_fasta
from segalign_amd import synth
from segalign_amd.build import build_host
from test_gpu_gapped_host import encode, rc_codes, run

pytestmark = pytest.mark.gpu


def rc_text(s):
    return s[::-1].translate(str.maketrans("ACGTacgt", "TGCAtgca"))


def test_host_skip_covered_files(tmp_path):
    base = synth.random_dna(50000, 961)
    # a tandem-duplicated stretch gives the query many hits on one region
    t_recs = [("chrA", np.concatenate([base[:30000], base[20000:30000], base[30000:]])), ("chrB", synth.random_dna(30000, 962))]
    q_recs = []
    for i, (_, s) in enumerate(t_recs):
        m = synth.mutate(s, 970 + i, 0.06, indel_every=350)
        q_recs.append(("qry%d" % (i + 1), synth.soft_mask(m, 980 + i, 0.1, 100, 500)))
    tf, qf = tmp_path / "target.fa", tmp_path / "query.fa"
    write_fasta(tf, t_recs)
    write_fasta(qf, q_recs)
    exe = build_host()
    plain, plain_out = run(exe, tf, qf, tmp_path / "plain", ["--gpu_gapped"])
    gapped, gapped_out = run(exe, tf, qf, tmp_path / "greedy", ["--gpu_gapped", "--gpu_skip_covered"])
    got, got_out = run(exe, tf, qf, tmp_path / "maf", ["--gpu_gapped", "--gpu_skip_covered", "--gpu_maf"])
    assert got_out == gapped_out == plain_out
    gfiles = sorted(f for f in plain if f.endswith(".gapped"))
    assert gfiles and sorted(gapped) == sorted(plain)
    assert all(gapped[f] == plain[f] for f in plain if f.endswith(".segments"))
    assert all(got[f] == gapped[f] for f in gapped)
    assert sorted(got) == sorted(list(gapped) + [f[:-len("gapped")] + "maf" for f in gfiles])

    R = Arena([(n, s.tobytes()) for n, s in t_recs], 500_000_000, 19, 10_000_000, False)
    Q = Arena([(n, s.tobytes()) for n, s in q_recs], 500_000_000, 19, 10_000_000, True)
    t_codes = encode(R.buf[:R.block_len[0]])
    q_codes = encode(Q.buf[:Q.block_len[0]])
    r_text = bytes(R.buf[:R.block_len[0]]).decode()
    q_text = bytes(Q.buf[:Q.block_len[0]]).decode()
    fasta = {n: s.tobytes().decode() for n, s in t_recs + q_recs}
    n_lines = n_covered = 0
    for f in gfiles:
        rev = ".minus." in f
        names, starts = (Q.rc_name, Q.rc_start) if rev else (Q.chr_name, Q.chr_start)
        hsps = []
        for line in got[f[:-len("gapped")] + "segments"].splitlines():
            rn, rs, re_, qn, qs, qe, _, sc = line.split("\t")
            ri, qi = R.chr_name.index(rn), names.index(qn)
            hsps.append((R.chr_start[ri] + int(rs) - 1, starts[qi] + int(qs) - 1, int(re_) - int(rs), int(sc)))
        if rev:
            hsps = hsps[::-1]
        h = np.array(hsps, dtype=G.SEG_DTYPE)
        qc = rc_codes(q_codes) if rev else q_codes
        qt = rc_text(q_text) if rev else q_text
        sel, sel_paths, st = GR.from_checker(t_codes, qc, G.SUB, h, 3000)
        assert st["returned"] + st["covered"] + st["below_thresh"] == h.size
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
        assert got[f] == "".join(lines), f
        assert got[f[:-len("gapped")] + "maf"] == "".join(blocks), f
        n_lines += len(lines)
        n_covered += st["covered"]
    assert n_lines > 0 and n_covered > 0
