"""GPU: segalign_host --gpu_gapped --gpu_maf.  Next to every .gapped file a .maf file holds the same alignments in LASTZ's maf-
layout (sa_gapped_align); every block must equal a model built from the serial path checker and the FASTA.  The .segments and
.gapped files and stdout stay what a --gpu_gapped run writes."""
import bisect
import os

import numpy as np
import pytest

import gapped_model as G
import gapped_trace_model as T
from host_model import Arena, write_fasta
from segalign_amd import synth
from segalign_amd.build import build_host
from test_gpu_gapped_host import encode, rc_codes, run

pytestmark = pytest.mark.gpu


def rc_text(s):
    return s[::-1].translate(str.maketrans("ACGTacgt", "TGCAtgca"))


def test_host_writes_maf_files(tmp_path):
    t_recs = [("chrA", synth.random_dna(60000, 931)), ("chrB", synth.random_dna(45000, 932))]
    q_recs = []
    for i, (_, s) in enumerate(t_recs):
        m = synth.mutate(s, 940 + i, 0.08, indel_every=300)
        q_recs.append(("qry%d" % (i + 1), synth.soft_mask(m, 950 + i, 0.1, 100, 500)))
    tf, qf = tmp_path / "target.fa", tmp_path / "query.fa"
    write_fasta(tf, t_recs)
    write_fasta(qf, q_recs)
    exe = build_host()
    gapped, gapped_out = run(exe, tf, qf, tmp_path / "gapped", ["--gpu_gapped"])
    got, got_out = run(exe, tf, qf, tmp_path / "maf", ["--gpu_gapped", "--gpu_maf"])
    assert got_out == gapped_out
    assert all(got[f] == gapped[f] for f in gapped)
    gfiles = sorted(f for f in gapped if f.endswith(".gapped"))
    assert gfiles and sorted(got) == sorted(list(gapped) + [f[:-len("gapped")] + "maf" for f in gfiles])

    R = Arena([(n, s.tobytes()) for n, s in t_recs], 500_000_000, 19, 10_000_000, False)
    Q = Arena([(n, s.tobytes()) for n, s in q_recs], 500_000_000, 19, 10_000_000, True)
    t_codes = encode(R.buf[:R.block_len[0]])
    q_codes = encode(Q.buf[:Q.block_len[0]])
    r_text = bytes(R.buf[:R.block_len[0]]).decode()
    q_text = bytes(Q.buf[:Q.block_len[0]]).decode()
    fasta = {n: s.tobytes().decode() for n, s in t_recs + q_recs}
    n_blocks = 0
    for f in gfiles:
        rev = ".minus." in f
        names, starts = (Q.rc_name, Q.rc_start) if rev else (Q.chr_name, Q.chr_start)
        seg = got[f[:-len("gapped")] + "segments"]
        hsps = []
        for line in seg.splitlines():
            rn, rs, re_, qn, qs, qe, _, sc = line.split("\t")
            ri, qi = R.chr_name.index(rn), names.index(qn)
            hsps.append((R.chr_start[ri] + int(rs) - 1, starts[qi] + int(qs) - 1, int(re_) - int(rs), int(sc)))
        if rev:
            hsps = hsps[::-1]
        h = np.array(hsps, dtype=G.SEG_DTYPE)
        qc = rc_codes(q_codes) if rev else q_codes
        qt = rc_text(q_text) if rev else q_text
        raw, paths = T.align(t_codes, qc, G.SUB, h)
        sel, sel_paths = T.select(raw, paths, 3000)
        blocks = []
        for a, (lo, ro, _) in zip(sel.tolist(), sel_paths):
            r0, r1, q0, q1, score = a[0], a[1], a[2], a[3], a[4]
            ri = bisect.bisect_right(R.chr_start, r0) - 1
            qi = bisect.bisect_right(starts, q0) - 1
            ta, qa = T.maf_texts(r_text, qt, r0, q0, np.concatenate([lo, ro]))
            blocks.append("a score=%d\ns %s %d %d + %d %s\ns %s %d %d %s %d %s\n\n" % (
                score, R.chr_name[ri], r0 - R.chr_start[ri], r1 - r0, len(fasta[R.chr_name[ri]]), ta,
                names[qi], q0 - starts[qi], q1 - q0, "-" if rev else "+", len(fasta[names[qi]]), qa))
        if rev:
            blocks = blocks[::-1]
        maf = got[f[:-len("gapped")] + "maf"]
        assert maf == "".join(blocks), f
        # every text without its gaps is the FASTA substring (reverse-complemented on '-'), every score the .gapped line's
        glines = got[f].splitlines()
        mblocks = [b for b in maf.split("\n\n") if b]
        assert len(mblocks) == len(glines)
        for b, gl in zip(mblocks, glines):
            al, sr, sq = b.split("\n")
            assert al == "a score=" + gl.split("\t")[-1]
            for s_line in (sr, sq):
                _, name, start, size, strand, src, text = s_line.split(" ")
                seq = fasta[name] if strand == "+" else rc_text(fasta[name])
                assert int(src) == len(fasta[name])
                assert text.replace("-", "") == seq[int(start):int(start) + int(size)]
            assert len(sr.split(" ")[-1]) == len(sq.split(" ")[-1])
        n_blocks += len(mblocks)
    assert n_blocks > 0
