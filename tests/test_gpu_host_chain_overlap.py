"""GPU: segalign_host --gpu_chain_overlap[=N] with --gpu_chain or --gpu_chain_all, on the input of
tests/test_gpu_host_chain.py.  The DP runs under the allowance (tests/hsp_chain_overlap_model.py) and the chains are trimmed
(tests/chain_trim_model.py): the .chain / .chains files hold the trimmed members with their exact scores and the exact chain scores, and
--gpu_stitch gets the trimmed chains (tests/stitch_model.py).  Every file the host wrote before stays byte for byte, and without the flag
it writes what tests/host_model.py says."""
import bisect
import subprocess

import numpy as np
import pytest

import chain_trim_model as TR
import gapped_model as G
import gapped_trace_model as T
import hsp_chain_model as M
import hsp_chain_overlap_model as O
import stitch_model as S
from helpers import Case
from host_model import expected_outputs
from segalign_amd.build import build_host
from test_gpu_gapped_host import run
from test_gpu_gapped_maf_host import rc_text
from test_gpu_host_chain import chain_text, file_hsps, pair  # noqa: F401  (pair: the module's fixture, built anew here)
from test_gpu_host_chain_all import chains_text

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def plain(pair):
    d, tf, qf = pair[:3]
    return run(build_host(), tf, qf, d / "plain", [])


@pytest.fixture(scope="module")
def codes(engine, pair):
    """The codes of the resident target block and of both query strands, as the entries see them."""
    R, Q = pair[5], pair[6]
    target = np.frombuffer(bytes(R.buf[:R.block_len[0]]), dtype=np.uint8)
    query = np.frombuffer(bytes(Q.buf[:Q.block_len[0]]), dtype=np.uint8)
    Case(target, query, chunk=20000, sub_mat=G.SUB).engine_setup(engine, num_gpu=1)
    try:
        return engine.copy_ref_codes(), {rev: engine.copy_query_codes(0, rev) for rev in (False, True)}, target, query
    finally:
        engine.ShutdownProcessor()


def test_without_the_flag_the_host_writes_what_it_wrote(oracle, pair, plain):
    _, _, _, t_recs, q_recs, _, _ = pair
    files, cmds = expected_outputs(oracle, [(n, s.tobytes()) for n, s in t_recs], [(n, s.tobytes()) for n, s in q_recs], chunk=20000)
    assert plain[0] == files and plain[1] == sorted(cmds + [""])


def test_best_chains_under_the_default_allowance_are_trimmed(pair, plain, codes):
    d, tf, qf, _, _, R, Q = pair
    ref, qc, _, _ = codes
    base, base_out = plain
    got, got_out = run(build_host(), tf, qf, d / "overlap", ["--gpu_chain", "--gpu_chain_overlap"])
    assert got_out == base_out
    segs = sorted(f for f in base if f.endswith(".segments"))
    assert segs and sorted(got) == sorted(list(base) + [f[:-len("segments")] + "chain" for f in segs])
    assert all(got[f] == base[f] for f in base)
    old, _ = run(build_host(), tf, qf, d / "chain", ["--gpu_chain"])
    seen = set()
    for f in segs:
        rev = ".minus." in f
        h, g = file_hsps(got[f], rev, R, Q)
        _, _, members = O.chain(h, g, max_overlap=64)
        assert members.size > M.chain(h, g)[2].size  # the regime: the allowance lengthens the chains
        mem = members["hsp_index"].astype(np.uint32)
        starts = np.flatnonzero(np.concatenate([[True], members["group"][1:] != members["group"][:-1]]))
        first = np.concatenate([starts, [mem.size]]).astype(np.uint32)
        out, chains, links = TR.trim(ref, qc[rev], G.SUB, h, mem, first)
        assert (links["o"] > 0).sum() >= 1 and (links["x"] > 0).any() and not np.array_equal(out, h[mem])
        idx = np.zeros(out.size, dtype=M.MEMBER)
        idx["hsp_index"] = np.arange(out.size)
        stem = f[:-len("segments")]
        assert got[stem + "chain"] == chain_text(out, idx, rev, R, Q), f
        assert got[stem + "chain"] != old[stem + "chain"]
        seen.add(rev)
    assert seen == {False, True}


def test_all_chains_under_an_allowance_are_trimmed_and_stitched(pair, plain, codes):
    d, tf, qf, t_recs, q_recs, R, Q = pair
    ref, qc, target, query = codes
    base, base_out = plain
    got, got_out = run(build_host(), tf, qf, d / "overlap_all", ["--gpu_chain_all", "--gpu_chain_overlap=32", "--gpu_stitch"])
    assert got_out == base_out
    segs = sorted(f for f in base if f.endswith(".segments"))
    assert sorted(got) == sorted(list(base) + [f[:-len("segments")] + e for f in segs for e in ("chains", "stitched.maf")])
    assert all(got[f] == base[f] for f in base)
    r_text, q_text = target.tobytes().decode(), query.tobytes().decode()
    fasta = {n: s.tobytes().decode() for n, s in t_recs + q_recs}
    seen = set()
    for f in segs:
        rev = ".minus." in f
        h, g = file_hsps(got[f], rev, R, Q)
        _, _, chains, members, _ = O.chain_all(h, g, max_overlap=32)
        mem = members["hsp_index"].astype(np.uint32)
        first = np.concatenate([chains["first_member"], [members.size]]).astype(np.uint32)
        out, tchains, links = TR.trim(ref, qc[rev], G.SUB, h, mem, first)
        assert (links["o"] > 0).sum() >= 1 and int(links["o"].max()) <= 32
        exact, idx = chains.copy(), members.copy()
        exact["score"] = tchains["score"]
        idx["hsp_index"] = np.arange(out.size)
        assert not np.array_equal(exact["score"], chains["score"])  # the DP's values are estimates where a link overlaps
        stem = f[:-len("segments")]
        assert got[stem + "chains"] == chains_text(out, exact, idx, rev, R, Q), f
        recs, ops, _, _ = S.stitch(ref, qc[rev], G.SUB, out, np.arange(out.size, dtype=np.uint32), first)
        names, starts = (Q.rc_name, Q.rc_start) if rev else (Q.chr_name, Q.chr_start)
        qt = rc_text(q_text) if rev else q_text
        blocks = []
        for k in range(recs.size):
            r = recs[k]
            r0, r1, q0, q1 = int(r["ref_start"]), int(r["ref_end"]), int(r["query_start"]), int(r["query_end"])
            ri, qi = bisect.bisect_right(R.chr_start, r0) - 1, bisect.bisect_right(starts, q0) - 1
            ta, qa = T.maf_texts(r_text, qt, r0, q0, S.record_ops(recs, ops, k))
            blocks.append("a score=%d\ns %s %d %d + %d %s\ns %s %d %d %s %d %s\n\n" % (
                int(r["score"]), R.chr_name[ri], r0 - R.chr_start[ri], r1 - r0, len(fasta[R.chr_name[ri]]), ta,
                names[qi], q0 - starts[qi], q1 - q0, "-" if rev else "+", len(fasta[names[qi]]), qa))
        assert got[stem + "stitched.maf"] == "".join(blocks), f
        seen.add(rev)
    assert seen == {False, True}


@pytest.mark.parametrize("flags,message", [
    (["--gpu_chain_overlap"], b"--gpu_chain_overlap needs --gpu_chain or --gpu_chain_all"),
    (["--gpu_chain_overlap=16", "--gpu_gapped"], b"--gpu_chain_overlap needs --gpu_chain or --gpu_chain_all"),
    (["--gpu_chain", "--gpu_chain_overlap=0"], b"bad --gpu_chain_overlap=0"),
    (["--gpu_chain_all", "--gpu_chain_overlap=4097"], b"bad --gpu_chain_overlap=4097"),
    (["--gpu_chain", "--gpu_chain_overlap=x"], b"bad --gpu_chain_overlap=x"),
])
def test_flag_errors(pair, flags, message):
    d, tf, qf = pair[:3]
    r = subprocess.run([build_host(), str(tf), str(qf), "./", "--outdir=%s" % d] + flags, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and message in r.stderr
