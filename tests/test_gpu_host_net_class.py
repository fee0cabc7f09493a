"""GPU: segalign_host --gpu_chain_all --gpu_net --gpu_net_class / --gpu_net_syn=..., on the input of test_gpu_host_chain.py.  Next to every
.net file a .net.class file holds the .net file's lines with the class of every fill (sa_net_classify, DESIGN.md 22: the query as the
other axis, ogroup = the query record of the chain's pair, every ostrand 0).  It must equal the rendering of tests/net_class_model.py on
the chains of tests/hsp_chain_all_model.py and the fills of tests/net_model.py.  With --gpu_net_syn the file holds the kept fills only,
and --gpu_net_subset --gpu_stitch work on them: .net.chains and .net.maf must equal the models on net_class_model.select's fills.  Every
other file equals a run without the new flags, byte for byte.

The thresholds of the --gpu_net_syn run were chosen on the CPU, from the models on the oracle's .segments files of this input: every
file keeps a fill and drops one, on its own account and with its parent (the test asserts it from the model and prints the regime)."""
import bisect
import subprocess

import numpy as np
import pytest

import gapped_model as G
import gapped_trace_model as T
import hsp_chain_all_model as A
import net_class_model as NC
import net_subset_model as NS
import stitch_model as S
from segalign_amd.build import build_host
from test_gpu_gapped_host import run
from test_gpu_gapped_maf_host import rc_text
from test_gpu_host_chain import file_hsps, pair  # noqa: F401  (pair: the module's fixture, built anew here)
from test_gpu_host_net import file_net

pytestmark = pytest.mark.gpu
MAX_LINK = 500
SYN = dict(min_score=30_000, min_top_score=300_000, min_size=300, min_ali=280, max_far=0)
SYN_FLAG = "--gpu_net_syn=%d,%d,%d,%d,%d" % tuple(SYN[k] for k in NC.THRESHOLDS)


def file_class(text, rev, R, Q, filter=None):
    """The models on one .segments file: -> dict with the .net text, the HSPs, the CSR, the fills and (classes, stats)."""
    names, starts = (Q.rc_name, Q.rc_start) if rev else (Q.chr_name, Q.chr_start)
    net_text, fills, _ = file_net(text, rev, R, Q)
    h, g = file_hsps(text, rev, R, Q)
    pairs = sorted({(bisect.bisect_right(R.chr_start, int(x["ref_start"])) - 1, bisect.bisect_right(starts, int(x["query_start"])) - 1) for x in h})
    _, _, chains, members, _ = A.chain_all(h, g)
    mem = members["hsp_index"].astype(np.uint32)
    first = np.concatenate([chains["first_member"], [members.size]]).astype(np.uint32)
    bs, be = NS.blocks(h, mem, "target")
    obs, obe = NC.other_blocks(h, mem, first, "target")
    ogroup = np.array([pairs[c][1] for c in chains["group"]], dtype=np.uint32)
    cls, st = NC.classify(first, bs, be, obs, obe, fills, ogroup, None, filter)
    return dict(net=net_text, h=h, mem=mem, first=first, fills=fills, classes=cls, stats=st)


def regime(fills, cls):
    """(kept, dropped on their own account under a kept parent or none, dropped with their parent)."""
    own = sum(1 for f, c in zip(fills, cls) if not c["keep"] and (int(f["parent"]) < 0 or cls[int(f["parent"])]["keep"]))
    return int(cls["keep"].sum()), own, int((cls["keep"] == 0).sum()) - own


@pytest.fixture(scope="module")
def netted(pair):
    d, tf, qf = pair[:3]
    return run(build_host(), tf, qf, d / "net_only", ["--gpu_chain_all", "--gpu_net", "--gpu_net_subset", "--gpu_stitch=%d" % MAX_LINK])


def test_host_writes_net_class_files(pair, netted):
    d, tf, qf, t_recs, q_recs, R, Q = pair
    base, base_out = netted
    segs = sorted(f for f in base if f.endswith(".segments"))
    assert len(segs) == 2 and {".minus." in f for f in segs} == {False, True}
    want = {}
    for f in segs:
        m = file_class(base[f], ".minus." in f, R, Q)
        assert m["net"] == base[f[:-len("segments")] + "net"]
        print(f, {k: m["stats"][k] for k in NC.COUNTS})
        assert m["stats"]["n_type"][NC.SYN] >= 1 and m["stats"]["n_type"][NC.INV] == 0  # a file holds one strand: no inv
        want[f[:-len("segments")] + "net.class"] = NC.render_class(m["net"], m["classes"])
    got, got_out = run(build_host(), tf, qf, d / "net_class", ["--gpu_chain_all", "--gpu_net", "--gpu_net_subset", "--gpu_stitch=%d" % MAX_LINK,
                                                             "--gpu_net_class"])
    assert got_out == base_out
    assert sorted(got) == sorted(list(base) + list(want))
    assert all(got[f] == base[f] for f in base)
    for f, text in want.items():
        assert got[f] == text, f


def test_the_syntenic_nets_alignments(pair, netted):
    d, tf, qf, t_recs, q_recs, R, Q = pair
    base, base_out = netted
    segs = sorted(f for f in base if f.endswith(".segments"))
    lens = {n: s.size for n, s in t_recs + q_recs}
    r_text, q_text = bytes(R.buf[:R.block_len[0]]).decode(), bytes(Q.buf[:Q.block_len[0]]).decode()
    want = {}
    for f in segs:
        rev = ".minus." in f
        names, starts = (Q.rc_name, Q.rc_start) if rev else (Q.chr_name, Q.chr_start)
        m = file_class(base[f], rev, R, Q, filter=SYN)
        kept, own, below = regime(m["fills"], m["classes"])
        print(f, "kept, dropped on their own account, dropped with their parent:", (kept, own, below), "per class:", m["stats"]["n_type"])
        assert kept >= 1 and own >= 1 and below >= 1, (f, kept, own, below)  # the regime the thresholds were chosen for
        stem = f[:-len("segments")]
        want[stem + "net.class"] = NC.render_class(m["net"], m["classes"], kept_only=True)
        sel, _ = NC.select(m["fills"], m["classes"]["keep"])
        qt = rc_text(q_text) if rev else q_text
        t, q = NS.encode(r_text.encode()), NS.encode(qt.encode())
        hs, ch, st = NS.subset(t, q, G.SUB, m["h"], m["mem"], m["first"], sel)
        want[stem + "net.chains"] = NS.render_chains(hs, ch, rev, R.chr_name, R.chr_start, names, starts)
        smem, sfirst = NS.csr(ch)
        recs, ops, _, _ = S.stitch(t, q, G.SUB, hs, smem, sfirst, max_link=MAX_LINK)
        texts = [T.maf_texts(r_text, qt, int(r["ref_start"]), int(r["query_start"]), S.record_ops(recs, ops, k)) for k, r in enumerate(recs)]
        want[stem + "net.maf"] = NS.render_maf(recs, texts, rev, R.chr_name, R.chr_start, [lens[n] for n in R.chr_name], names, starts,
                                               [lens[n] for n in names])
        assert want[stem + "net.chains"] != base[stem + "net.chains"]
    got, got_out = run(build_host(), tf, qf, d / "net_syn", ["--gpu_chain_all", "--gpu_net", "--gpu_net_subset", "--gpu_stitch=%d" % MAX_LINK, SYN_FLAG])
    assert got_out == base_out
    assert sorted(got) == sorted(list(base) + [f for f in want if f.endswith(".net.class")])
    assert all(got[f] == base[f] for f in base if f not in want)
    for f, text in want.items():
        assert got[f] == text, f


@pytest.mark.parametrize("flags,message", [
    (["--gpu_net_class"], b"--gpu_net_class needs --gpu_net and --gpu_chain_all"),
    (["--gpu_chain_all", "--gpu_net_class"], b"--gpu_net_class needs --gpu_net"),
    (["--gpu_chain_all", "--gpu_net_syn=1,2,3,4,5"], b"--gpu_net_syn needs --gpu_net"),
    (["--gpu_chain_all", "--gpu_net", "--gpu_net_class=3"], b"unknown option --gpu_net_class=3"),
    (["--gpu_chain_all", "--gpu_net", "--gpu_net_syn=1,2,3,4"], b"bad --gpu_net_syn"),
    (["--gpu_chain_all", "--gpu_net", "--gpu_net_syn=1,2,3,4,5,6"], b"bad --gpu_net_syn"),
    (["--gpu_chain_all", "--gpu_net", "--gpu_net_syn=1,2,-3,4,5"], b"bad --gpu_net_syn"),
    (["--gpu_chain_all", "--gpu_net", "--gpu_net_syn=1,2,3,4,2147483649"], b"bad --gpu_net_syn"),
])
def test_flag_errors(pair, flags, message):
    d, tf, qf = pair[:3]
    r = subprocess.run([build_host(), str(tf), str(qf), "./", "--outdir=%s" % d] + flags, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and message in r.stderr
