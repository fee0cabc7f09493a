"""GPU: segalign_host --gpu_chain_fill[=thresh[,xdrop]] with --gpu_chain or --gpu_chain_all, on the input of
tests/test_gpu_host_chain.py.  Next to every .chain / .chains file a .filled.chain / .filled.chains file holds the chains with the
fills of tests/chain_fill_model.py spliced in, --gpu_stitch gets the filled chains (tests/stitch_model.py), and every file the host
wrote before stays byte for byte."""
import bisect
import subprocess

import numpy as np
import pytest

import chain_fill_model as F
import gapped_model as G
import gapped_trace_model as T
import hsp_chain_model as M
import hsp_chain_overlap_model as O
import stitch_model as S
from helpers import Case
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


def model_all(h, g, ref, q, **kw):
    """All chains of a file's HSPs, filled: -> (chains, first, the model's fill result, the filled chains' records and members)."""
    _, _, chains, members, _ = O.chain_all(h, g)
    mem = members["hsp_index"].astype(np.uint32)
    first = np.concatenate([chains["first_member"], [members.size]]).astype(np.uint32)
    res = F.fill(ref, q, G.SUB, h, mem, first, **kw)
    out, first_out = res[0], res[1]
    rec = chains.copy()
    rec["score"], rec["first_member"], rec["n_members"] = res[3]["score"], first_out[:-1], np.diff(first_out)
    idx = np.zeros(out.size, dtype=members.dtype)
    idx["hsp_index"] = np.arange(out.size)
    return mem, first, res, rec, idx


def test_all_chains_are_filled_and_every_other_file_stays(pair, plain, codes):
    d, tf, qf, _, _, R, Q = pair
    ref, qc, _, _ = codes
    base, base_out = plain
    old, old_out = run(build_host(), tf, qf, d / "all", ["--gpu_chain_all"])
    got, got_out = run(build_host(), tf, qf, d / "fill_all", ["--gpu_chain_all", "--gpu_chain_fill"])
    assert got_out == old_out == base_out
    segs = sorted(f for f in base if f.endswith(".segments"))
    assert len(segs) == 2 and sorted(got) == sorted(list(old) + [f[:-len("segments")] + "filled.chains" for f in segs])
    assert all(got[f] == old[f] for f in old)
    for f in segs:
        rev = ".minus." in f
        h, g = file_hsps(got[f], rev, R, Q)
        _, _, res, rec, idx = model_all(h, g, ref, qc[rev])
        links = res[4]
        # the regime, from the model: most links hold an HSP at the main path's own threshold, a few swept ones hold none
        assert (links["n_fill"] > 0).sum() >= (20 if rev else 40) and ((links["cells"] > 0) & (links["n_fill"] == 0)).sum() >= 1
        stem = f[:-len("segments")]
        assert got[stem + "filled.chains"] == chains_text(res[0], rec, idx, rev, R, Q), f
        assert got[stem + "filled.chains"] != got[stem + "chains"]


def test_a_side_limit_and_other_thresholds_reach_the_entry(pair, plain, codes):
    d, tf, qf, _, _, R, Q = pair
    ref, qc, _, _ = codes
    got, _ = run(build_host(), tf, qf, d / "fill_side", ["--gpu_chain_all", "--gpu_chain_fill=2500,600", "--gpu_chain_fill_side=600"])
    for f in sorted(f for f in got if f.endswith(".segments")):
        rev = ".minus." in f
        h, g = file_hsps(got[f], rev, R, Q)
        _, _, res, rec, idx = model_all(h, g, ref, qc[rev], thresh=2500, xdrop=600, max_side=600)
        assert (res[4]["flags"] == F.LONG).sum() >= 1 and (res[4]["n_fill"] > 0).sum() >= 10
        assert got[f[:-len("segments")] + "filled.chains"] == chains_text(res[0], rec, idx, rev, R, Q), f


def test_best_chains_are_filled(pair, plain, codes):
    d, tf, qf, _, _, R, Q = pair
    ref, qc, _, _ = codes
    base, base_out = plain
    got, got_out = run(build_host(), tf, qf, d / "fill_best", ["--gpu_chain", "--gpu_chain_fill"])
    assert got_out == base_out and all(got[f] == base[f] for f in base)
    segs = sorted(f for f in base if f.endswith(".segments"))
    assert sorted(got) == sorted(list(base) + [f[:-len("segments")] + e for f in segs for e in ("chain", "filled.chain")])
    for f in segs:
        rev = ".minus." in f
        h, g = file_hsps(got[f], rev, R, Q)
        _, _, members = M.chain(h, g)
        mem = members["hsp_index"].astype(np.uint32)
        starts = np.flatnonzero(np.concatenate([[True], members["group"][1:] != members["group"][:-1]]))
        first = np.concatenate([starts, [mem.size]]).astype(np.uint32)
        res = F.fill(ref, qc[rev], G.SUB, h, mem, first)
        assert (res[4]["n_fill"] > 0).sum() >= 2
        idx = np.zeros(res[0].size, dtype=M.MEMBER)
        idx["hsp_index"] = np.arange(res[0].size)
        stem = f[:-len("segments")]
        assert got[stem + "chain"] == chain_text(h, members, rev, R, Q) and got[stem + "filled.chain"] == chain_text(res[0], idx, rev, R, Q), f


def test_the_filled_chains_are_stitched_with_fewer_long_links(pair, plain, codes):
    d, tf, qf, t_recs, q_recs, R, Q = pair
    ref, qc, target, query = codes
    got, _ = run(build_host(), tf, qf, d / "fill_stitch", ["--gpu_chain_all", "--gpu_chain_fill", "--gpu_stitch=500"])
    r_text, q_text = target.tobytes().decode(), query.tobytes().decode()
    fasta = {n: s.tobytes().decode() for n, s in t_recs + q_recs}
    for f in sorted(f for f in got if f.endswith(".segments")):
        rev = ".minus." in f
        h, g = file_hsps(got[f], rev, R, Q)
        mem, first, res, rec, idx = model_all(h, g, ref, qc[rev])
        out = res[0]
        recs, ops, links, _ = S.stitch(ref, qc[rev], G.SUB, out, np.arange(out.size, dtype=np.uint32), res[1], max_link=500)
        before = S.stitch(ref, qc[rev], G.SUB, h, mem, first, max_link=500)
        long_after, long_before = int(((links["flags"] & S.LONG) != 0).sum()), int(((before[2]["flags"] & S.LONG) != 0).sum())
        assert long_after < long_before and recs.size < before[0].size, (long_after, long_before)
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
        assert got[f[:-len("segments")] + "stitched.maf"] == "".join(blocks), f


def test_the_later_stages_take_the_filled_chains(pair, plain):
    d, tf, qf = pair[:3]
    flags = ["--gpu_chain_all", "--gpu_net", "--gpu_net_subset", "--gpu_stitch"]
    old, _ = run(build_host(), tf, qf, d / "net", flags)
    got, _ = run(build_host(), tf, qf, d / "fill_net", flags + ["--gpu_chain_fill"])
    stems = [f[:-len("segments")] for f in got if f.endswith(".segments")]
    for s in stems:
        assert got[s + "chains"] == old[s + "chains"] and got[s + "net"] != old[s + "net"]
        # what lower chains held inside the gaps of a top-level chain is now that chain's own: its aligned bases grow
        top = [sum(int(ln.split("ali=")[1]) for ln in t[s + "net"].splitlines() if ln.startswith("fill ")) for t in (old, got)]
        assert top[1] > top[0]
        assert got[s + "net.chains"] != old[s + "net.chains"] and got[s + "net.maf"] != old[s + "net.maf"]


@pytest.mark.parametrize("flags,message", [
    (["--gpu_chain_fill"], b"--gpu_chain_fill needs --gpu_chain or --gpu_chain_all"),
    (["--gpu_chain_fill=2000", "--gpu_gapped"], b"--gpu_chain_fill needs --gpu_chain or --gpu_chain_all"),
    (["--gpu_chain", "--gpu_chain_fill=0"], b"bad --gpu_chain_fill=0"),
    (["--gpu_chain_all", "--gpu_chain_fill=3000,-1"], b"bad --gpu_chain_fill=3000,-1"),
    (["--gpu_chain", "--gpu_chain_fill=x"], b"bad --gpu_chain_fill=x"),
    (["--gpu_chain", "--gpu_chain_fill_side=100"], b"--gpu_chain_fill_side needs --gpu_chain_fill"),
    (["--gpu_chain", "--gpu_chain_fill", "--gpu_chain_fill_side=1048577"], b"bad --gpu_chain_fill_side=1048577"),
])
def test_flag_errors(pair, flags, message):
    d, tf, qf = pair[:3]
    r = subprocess.run([build_host(), str(tf), str(qf), "./", "--outdir=%s" % d] + flags, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and message in r.stderr
