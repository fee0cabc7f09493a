"""GPU: segalign_host --gpu_stitch[=max_link] [--gpu_stitch_min=N] with --gpu_chain_all, on the input of test_gpu_host_chain.py.  Next to
every .chains file a .stitched.maf file holds one block per record of sa_stitch_chains in --gpu_maf's block layout, in
the order the entry returns; it must equal the records of tests/stitch_model.py on the chains of tests/hsp_chain_all_model.py, rendered
with gapped_trace_model.maf_texts.  Every other file and stdout stay byte for byte."""
import bisect
import subprocess

import numpy as np
import pytest

import gapped_model as G
import gapped_trace_model as T
import hsp_chain_all_model as A
import stitch_model as S
from helpers import Case
from segalign_amd.build import build_host
from test_gpu_gapped_host import run
from test_gpu_gapped_maf_host import rc_text
from test_gpu_host_chain import file_hsps, pair  # noqa: F401  (pair: the module's fixture, built anew here)

pytestmark = pytest.mark.gpu


def test_host_writes_stitched_maf_files(engine, pair):
    d, tf, qf, t_recs, q_recs, R, Q = pair
    exe = build_host()
    base, base_out = run(exe, tf, qf, d / "chains", ["--gpu_chain_all"])
    got, got_out = run(exe, tf, qf, d / "stitched", ["--gpu_chain_all", "--gpu_stitch=500"])
    assert got_out == base_out
    segs = sorted(f for f in base if f.endswith(".segments"))
    assert segs and sorted(got) == sorted(list(base) + [f[:-len("segments")] + "stitched.maf" for f in segs])
    assert all(got[f] == base[f] for f in base)

    E = engine
    target = np.frombuffer(bytes(R.buf[:R.block_len[0]]), dtype=np.uint8)
    query = np.frombuffer(bytes(Q.buf[:Q.block_len[0]]), dtype=np.uint8)
    Case(target, query, chunk=20000, sub_mat=G.SUB).engine_setup(E, num_gpu=1)
    try:
        ref = E.copy_ref_codes()
        codes = {rev: E.copy_query_codes(0, rev) for rev in (False, True)}
    finally:
        E.ShutdownProcessor()
    r_text, q_text = target.tobytes().decode(), query.tobytes().decode()
    fasta = {n: s.tobytes().decode() for n, s in t_recs + q_recs}
    seen = set()
    for f in segs:
        rev = ".minus." in f
        h, g = file_hsps(got[f], rev, R, Q)
        _, _, chains, members, _ = A.chain_all(h, g)
        mem = members["hsp_index"].astype(np.uint32)
        first = np.concatenate([chains["first_member"], [members.size]]).astype(np.uint32)
        assert np.array_equal(first[1:] - first[:-1], chains["n_members"])
        recs, ops, links, cnt = S.stitch(ref, codes[rev], G.SUB, h, mem, first, max_link=500)
        # the regime: both outcomes occur -- at least a tenth of the links exceed max_link, and many are short, most of those one-sided
        side = np.maximum(links["dt"], links["dq"])
        within = side <= 256
        empty = within & ((links["dt"] == 0) | (links["dq"] == 0))
        print(f, "links", links.size, "long", cnt["long_links"], "within 256", int(within.sum()), "one side 0", int(empty.sum()),
              "records", recs.size)
        need = (11, 9) if rev else (19, 15)
        assert 10 * cnt["long_links"] >= links.size and int(within.sum()) >= need[0] and int(empty.sum()) >= need[1]
        assert np.any(recs["n_members"] > 1) and np.any(recs["flags"] == S.LONG)
        S.check_invariants(ref, codes[rev], G.SUB, recs, ops)
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
        assert got[f[:-len("segments")] + "stitched.maf"] == "".join(blocks), f  # the entry's order on both strands
        seen.add(rev)
    assert seen == {False, True}


@pytest.mark.parametrize("flags,message", [
    (["--gpu_stitch"], b"--gpu_stitch needs --gpu_chain or --gpu_chain_all"),
    (["--gpu_stitch=300", "--gpu_gapped"], b"--gpu_stitch needs --gpu_chain or --gpu_chain_all"),
    (["--gpu_chain", "--gpu_stitch_min=-500"], b"--gpu_stitch_min needs --gpu_stitch"),
    (["--gpu_chain_all", "--gpu_stitch=2049"], b"bad --gpu_stitch=2049"),
    (["--gpu_chain_all", "--gpu_stitch=0"], b"bad --gpu_stitch=0"),
    (["--gpu_chain_all", "--gpu_stitch", "--gpu_stitch_min=x"], b"bad --gpu_stitch_min=x"),
])
def test_flag_errors(pair, flags, message):
    d, tf, qf = pair[:3]
    r = subprocess.run([build_host(), str(tf), str(qf), "./", "--outdir=%s" % d] + flags, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and message in r.stderr
