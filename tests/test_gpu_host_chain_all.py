"""GPU: segalign_host --gpu_chain_all[=diag,anti] [--gpu_chain_gap=N] [--gpu_chain_min=N], on the input of test_gpu_host_chain.py.  Next
to every .segments file a .chains file holds all collinear chains of every (target record, query record) pair of that file
(sa_chain_hsps_all): a '#chain' line and the members in the .segments line format per kept chain, in the order the entry
returns; it must equal the rendering of tests/hsp_chain_all_model.py on the file's HSPs.  With --gpu_gapped the .gapped files hold the
alignments of the kept chains' HSPs, in their original order: GappedAlign on the model's members.  Without the flag the host writes
what tests/host_model.py says, and with it every file it wrote before stays byte for byte."""
import subprocess

import numpy as np
import pytest

import gapped_model as G
import hsp_chain_all_model as A
from helpers import Case
from host_model import expected_outputs
from segalign_amd.build import build_host
from test_gpu_gapped_host import run
from test_gpu_host_chain import file_hsps, pair, seg_line  # noqa: F401  (pair: the module's fixture, built anew here)

pytestmark = pytest.mark.gpu


def chains_text(h, chains, members, rev, R, Q):
    names, starts = (Q.rc_name, Q.rc_start) if rev else (Q.chr_name, Q.chr_start)
    out = []
    for k, c in enumerate(chains):
        out.append("#chain %d group=%d score=%d members=%d joined=%d\n" % (k, c["group"], c["score"], c["n_members"], c["joined"] >= 0))
        for i in members["hsp_index"][c["first_member"]:c["first_member"] + c["n_members"]].tolist():
            r0, q0, ln, sc = (int(x) for x in h[i].tolist())
            out.append(seg_line(R, names, starts, rev, r0, r0 + ln + 1, q0, q0 + ln + 1, sc))
    return "".join(out)


def check_chains_files(got, base, R, Q, **kw):
    """Every .chains file of `got` against the model on the .segments file beside it; every other file as in `base`.
    -> {segments file: (hsps, the model's members)}"""
    segs = sorted(f for f in base if f.endswith(".segments"))
    assert segs and sorted(got) == sorted(list(base) + [f[:-len("segments")] + "chains" for f in segs])
    assert all(got[f] == base[f] for f in base if not f.endswith(".gapped"))
    res, counts = {}, []
    for f in segs:
        rev = ".minus." in f
        h, g = file_hsps(got[f], rev, R, Q)
        _, _, chains, members, _ = A.chain_all(h, g, **kw)
        assert got[f[:-len("segments")] + "chains"] == chains_text(h, chains, members, rev, R, Q), f
        res[f] = (h, members)
        per_group = np.bincount(chains["group"]) if chains.size else np.zeros(1, dtype=np.int64)
        counts.append((f, int(h.size), int(chains.size), int((chains["joined"] >= 0).sum()), int(members.size), int(per_group.max())))
    print("file, HSPs, chains kept, of them joined, members kept, most chains kept in one group:", counts)
    assert max(c[5] for c in counts) >= 2, "the input must yield two kept chains in one group"
    return res, counts


@pytest.fixture(scope="module")
def plain(pair):
    d, tf, qf = pair[:3]
    return run(build_host(), tf, qf, d / "plain", [])


def test_host_writes_chains_files(oracle, pair, plain):
    d, tf, qf, t_recs, q_recs, R, Q = pair
    files, cmds = expected_outputs(oracle, [(n, s.tobytes()) for n, s in t_recs], [(n, s.tobytes()) for n, s in q_recs], chunk=20000)
    assert plain[0] == files and plain[1] == sorted(cmds + [""])  # without the flag: the reference host's files and lines
    got, got_out = run(build_host(), tf, qf, d / "chains", ["--gpu_chain_all"])
    assert got_out == plain[1]
    res, counts = check_chains_files(got, plain[0], R, Q)
    assert any(".minus." in c[0] and c[2] for c in counts) and any(".plus." in c[0] and c[2] for c in counts)
    assert sum(c[3] for c in counts) > 0, "no joined chain"


def test_host_aligns_the_kept_chains(engine, pair, plain):
    d, tf, qf, t_recs, q_recs, R, Q = pair
    kw = dict(diag_pen=2, anti_pen=1, max_gap=3000)
    scores = []  # min_score: the median chain score of the model on the files the plain run wrote, so that it drops chains and keeps chains
    for f in sorted(f for f in plain[0] if f.endswith(".segments")):
        scores += A.chain_all(*file_hsps(plain[0][f], ".minus." in f, R, Q), min_score=-2 ** 62, **kw)[2]["score"].tolist()
    kw["min_score"] = int(np.median(scores)) + 1
    got, got_out = run(build_host(), tf, qf, d / "chains_gapped",
                       ["--gpu_gapped", "--gpu_chain_all=2,1", "--gpu_chain_gap=3000", "--gpu_chain_min=%d" % kw["min_score"]])
    assert got_out == plain[1]
    base = dict(plain[0])
    base.update({f[:-len("segments")] + "gapped": None for f in plain[0] if f.endswith(".segments")})
    print("min_score", kw["min_score"])
    res, counts = check_chains_files(got, base, R, Q, **kw)
    assert any(c[4] < c[1] for c in counts), "min_score must leave HSPs off the chains"

    E = engine
    target = np.frombuffer(bytes(R.buf[:R.block_len[0]]), dtype=np.uint8)
    query = np.frombuffer(bytes(Q.buf[:Q.block_len[0]]), dtype=np.uint8)
    Case(target, query, chunk=20000, sub_mat=G.SUB).engine_setup(E, num_gpu=1)
    n_lines = 0
    try:
        for f, (h, members) in res.items():
            rev = ".minus." in f
            names, starts = (Q.rc_name, Q.rc_start) if rev else (Q.chr_name, Q.chr_start)
            keep = np.sort(members["hsp_index"])  # the kept chains' HSPs in their original relative order
            recs = E.GappedAlign(h[keep].astype(E.SEG_DTYPE), rev, 0)[0]
            lines = [seg_line(R, names, starts, rev, *a[:5]) for a in recs.tolist()]
            if rev:
                lines = lines[::-1]
            assert got[f[:-len("segments")] + "gapped"] == "".join(lines), f
            n_lines += len(lines)
    finally:
        E.ShutdownProcessor()
    assert n_lines > 0


@pytest.mark.parametrize("flags,message", [
    (["--gpu_chain", "--gpu_chain_all"], b"exclude each other"),
    (["--gpu_chain_min=10"], b"--gpu_chain_min needs --gpu_chain_all"),
    (["--gpu_chain", "--gpu_chain_min=10"], b"--gpu_chain_min needs --gpu_chain_all"),
    (["--gpu_chain_all=1", "--gpu_chain_min=10"], b"bad --gpu_chain_all"),
    (["--gpu_chain_all", "--gpu_chain_min=x"], b"bad --gpu_chain_min"),
])
def test_flag_errors(pair, flags, message):
    d, tf, qf = pair[:3]
    r = subprocess.run([build_host(), str(tf), str(qf), "./", "--outdir=%s" % d] + flags, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and message in r.stderr
