"""GPU: segalign_host --gpu_gapped.  Next to every .segments file a .gapped file holds the gapped extension of the same HSPs
(sa_gapped_extend, selection mode), printed like the segments; it must equal a model built from the .segments file, the arena
layout of tests/host_model.py and the serial checker.  The .segments files and the lastz lines stay what a run without the flag
writes."""
import bisect
import os
import subprocess

import numpy as np
import pytest

import gapped_model as G
from host_model import Arena, write_fasta
from segalign_amd import synth
from segalign_amd.build import build_host

pytestmark = pytest.mark.gpu

_LUT = np.full(256, 6, dtype=np.uint8)
for _ch, _c in zip(b"ACGTacgtnN&", [0, 1, 2, 3, 4, 4, 4, 4, 5, 5, 7]):
    _LUT[_ch] = _c


def encode(ascii_bytes):
    return _LUT[np.frombuffer(bytes(ascii_bytes), dtype=np.uint8)]


def rc_codes(c):
    c = c[::-1].copy()
    m = c < 4
    c[m] = 3 - c[m]
    return c


def run(exe, tf, qf, outdir, extra):
    os.makedirs(outdir)
    cmd = [exe, str(tf), str(qf), "./", "--outdir=%s" % outdir, "--num_threads=2", "--num_gpu=1", "--wga_chunk=20000"] + extra
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    return {f: open(os.path.join(outdir, f)).read() for f in os.listdir(outdir)}, sorted(res.stdout.decode().split("\n"))


def test_host_writes_gapped_files(tmp_path):
    t_recs = [("chrA", synth.random_dna(60000, 901)), ("chrB", synth.random_dna(45000, 902))]
    q_recs = []
    for i, (_, s) in enumerate(t_recs):
        m = synth.mutate(s, 910 + i, 0.08, indel_every=600)
        q_recs.append(("qry%d" % (i + 1), synth.soft_mask(m, 920 + i, 0.1, 100, 500)))
    tf, qf = tmp_path / "target.fa", tmp_path / "query.fa"
    write_fasta(tf, t_recs)
    write_fasta(qf, q_recs)
    exe = build_host()
    plain, plain_out = run(exe, tf, qf, tmp_path / "plain", [])
    got, got_out = run(exe, tf, qf, tmp_path / "gapped", ["--gpu_gapped"])
    assert got_out == plain_out
    segs = sorted(f for f in plain if f.endswith(".segments"))
    assert segs and all(got[f] == plain[f] for f in plain)
    assert sorted(got) == sorted(list(plain) + [f[:-len("segments")] + "gapped" for f in segs])

    R = Arena([(n, s.tobytes()) for n, s in t_recs], 500_000_000, 19, 10_000_000, False)
    Q = Arena([(n, s.tobytes()) for n, s in q_recs], 500_000_000, 19, 10_000_000, True)
    t_codes = encode(R.buf[:R.block_len[0]])
    q_codes = encode(Q.buf[:Q.block_len[0]])
    n_lines = 0
    for f in segs:
        rev = ".minus." in f
        names, starts = (Q.rc_name, Q.rc_start) if rev else (Q.chr_name, Q.chr_start)
        hsps = []
        for line in plain[f].splitlines():
            rn, rs, re_, qn, qs, qe, _, sc = line.split("\t")
            ri, qi = R.chr_name.index(rn), names.index(qn)
            hsps.append((R.chr_start[ri] + int(rs) - 1, starts[qi] + int(qs) - 1, int(re_) - int(rs), int(sc)))
        if rev:
            hsps = hsps[::-1]  # the file holds the minus-strand vector in reverse order
        h = np.array(hsps, dtype=G.SEG_DTYPE)
        sel = G.select(G.extend(t_codes, rc_codes(q_codes) if rev else q_codes, G.SUB, h), 3000)
        lines = []
        for a in sel.tolist():
            r0, r1, q0, q1, score = a[0], a[1], a[2], a[3], a[4]
            ri = bisect.bisect_right(R.chr_start, r0) - 1
            qi = bisect.bisect_right(starts, q0) - 1
            lines.append("%s\t%d\t%d\t%s\t%d\t%d\t%s\t%d\n" % (R.chr_name[ri], r0 + 1 - R.chr_start[ri], r1 - R.chr_start[ri], names[qi],
                                                             q0 + 1 - starts[qi], q1 - starts[qi], "-" if rev else "+", score))
        if rev:
            lines = lines[::-1]
        want = "".join(lines)
        assert got[f[:-len("segments")] + "gapped"] == want, f
        n_lines += len(lines)
    assert n_lines > 0
