"""GPU: segalign_host --gpu_chain_all --gpu_net --gpu_net_subset [--gpu_stitch], on the input of test_gpu_host_chain.py.  Next to every
.net file a .net.chains file holds the sub-chains sa_net_subset cuts the fills into, with --gpu_stitch a .net.maf file
their stitch.  Both must equal the rendering of tests/net_subset_model.py on the chains of tests/hsp_chain_all_model.py and the fills
of tests/net_model.py; every other file equals a run with --gpu_net alone, byte for byte.

The regime, from the model first: at least one cut member and one split in each strand's file.  The default thresholds give them on
this input (38 cut members and 36 splits on the plus strand, 20 and 17 on the minus strand; the test prints them), so it runs at the
defaults."""
import subprocess

import numpy as np
import pytest

import gapped_model as G
import gapped_trace_model as T
import hsp_chain_all_model as A
import hsp_chain_gap_model as GM
import net_model as N
import net_subset_model as NS
import stitch_model as S
from segalign_amd.build import build_host
from test_gpu_gapped_host import run
from test_gpu_gapped_maf_host import rc_text
from test_gpu_host_chain import file_hsps, pair  # noqa: F401  (pair: the module's fixture, built anew here)

pytestmark = pytest.mark.gpu
MAX_LINK = 500


def file_subset(text, rev, R, Q, t_recs, q_recs, stitch=True, **net_kw):
    """The model's two files for one .segments file: -> (.net.chains text, .net.maf text or None, the subset's stats)."""
    names, starts = (Q.rc_name, Q.rc_start) if rev else (Q.chr_name, Q.chr_start)
    r_text = bytes(R.buf[:R.block_len[0]]).decode()
    q_text = bytes(Q.buf[:Q.block_len[0]]).decode()
    qt = rc_text(q_text) if rev else q_text
    t, q = NS.encode(r_text.encode()), NS.encode(qt.encode())
    h, g = file_hsps(text, rev, R, Q)
    pairs = sorted({(int(np.searchsorted(R.chr_start, int(x["ref_start"]), side="right")) - 1,
                     int(np.searchsorted(starts, int(x["query_start"]), side="right")) - 1) for x in h})
    _, _, chains, members, _ = A.chain_all(h, g)
    mem = members["hsp_index"].astype(np.uint32)
    first = np.concatenate([chains["first_member"], [members.size]]).astype(np.uint32)
    bs, be = NS.blocks(h, mem, "target")
    target = np.array([pairs[c][0] for c in chains["group"]], dtype=np.uint32)
    fills, _ = N.net(first, bs, be, chains["score"], target, **net_kw)
    hs, ch, st = NS.subset(t, q, G.SUB, h, mem, first, fills)
    chains_text = NS.render_chains(hs, ch, rev, R.chr_name, R.chr_start, names, starts)
    if not stitch:
        return chains_text, None, st
    smem, sfirst = NS.csr(ch)
    recs, ops, _, _ = S.stitch(t, q, G.SUB, hs, smem, sfirst, max_link=MAX_LINK)
    texts = [T.maf_texts(r_text, qt, int(r["ref_start"]), int(r["query_start"]), S.record_ops(recs, ops, k)) for k, r in enumerate(recs)]
    lens = {n: s.size for n, s in t_recs + q_recs}
    maf = NS.render_maf(recs, texts, rev, R.chr_name, R.chr_start, [lens[n] for n in R.chr_name], names, starts, [lens[n] for n in names])
    return chains_text, maf, st


@pytest.fixture(scope="module")
def netted(pair):
    d, tf, qf = pair[:3]
    return run(build_host(), tf, qf, d / "net_only", ["--gpu_chain_all", "--gpu_net", "--gpu_stitch=%d" % MAX_LINK])


def test_host_writes_net_chains_and_net_maf_files(pair, netted):
    d, tf, qf, t_recs, q_recs, R, Q = pair
    base, base_out = netted
    segs = sorted(f for f in base if f.endswith(".segments"))
    assert len(segs) == 2 and {".minus." in f for f in segs} == {False, True}
    want = {}
    for f in segs:
        chains_text, maf, st = file_subset(base[f], ".minus." in f, R, Q, t_recs, q_recs)
        print(f, {k: st[k] for k in NS.COUNTS})
        assert st["cut_members"] >= 1 and st["splits"] >= 1, (f, st)  # the regime, at the default thresholds
        want[f[:-len("segments")] + "net.chains"] = chains_text
        want[f[:-len("segments")] + "net.maf"] = maf
    got, got_out = run(build_host(), tf, qf, d / "net_subset", ["--gpu_chain_all", "--gpu_net", "--gpu_stitch=%d" % MAX_LINK, "--gpu_net_subset"])
    assert got_out == base_out
    assert sorted(got) == sorted(list(base) + list(want))
    assert all(got[f] == base[f] for f in base)
    for f, text in want.items():
        assert got[f] == text, f


def test_without_the_stitch_there_is_no_maf_file(pair):
    d, tf, qf, t_recs, q_recs, R, Q = pair
    got, _ = run(build_host(), tf, qf, d / "net_subset_plain", ["--gpu_chain_all=2,1", "--gpu_net=25", "--gpu_net_fill=12", "--gpu_net_subset",
                                                                  "--gpu_chain_costs=loose"])
    segs = sorted(f for f in got if f.endswith(".segments"))
    assert not any(f.endswith(".maf") for f in got) and sorted(f for f in got if f.endswith(".net.chains")) == [f[:-len("segments")] + "net.chains" for f in segs]
    for f in segs:  # the penalties and the table are those of the chains
        rev = ".minus." in f
        names, starts = (Q.rc_name, Q.rc_start) if rev else (Q.chr_name, Q.chr_start)
        r_text, q_text = bytes(R.buf[:R.block_len[0]]).decode(), bytes(Q.buf[:Q.block_len[0]]).decode()
        t, q = NS.encode(r_text.encode()), NS.encode((rc_text(q_text) if rev else q_text).encode())
        h, g = file_hsps(got[f], rev, R, Q)
        _, _, chains, members, _ = GM.chain_all(h, g, diag_pen=2, anti_pen=1, gap_costs="loose")
        mem = members["hsp_index"].astype(np.uint32)
        first = np.concatenate([chains["first_member"], [members.size]]).astype(np.uint32)
        pairs = sorted({(int(np.searchsorted(R.chr_start, int(x["ref_start"]), side="right")) - 1,
                         int(np.searchsorted(starts, int(x["query_start"]), side="right")) - 1) for x in h})
        bs, be = NS.blocks(h, mem, "target")
        fills, _ = N.net(first, bs, be, chains["score"], np.array([pairs[c][0] for c in chains["group"]], dtype=np.uint32), min_space=25, min_fill=12)
        hs, ch, st = NS.subset(t, q, G.SUB, h, mem, first, fills, diag_pen=2, anti_pen=1, gap_costs="loose")
        assert got[f[:-len("segments")] + "net.chains"] == NS.render_chains(hs, ch, rev, R.chr_name, R.chr_start, names, starts), f


@pytest.mark.parametrize("flags,message", [
    (["--gpu_net_subset"], b"--gpu_net_subset needs --gpu_net and --gpu_chain_all"),
    (["--gpu_chain_all", "--gpu_net_subset"], b"--gpu_net_subset needs --gpu_net"),
    (["--gpu_chain", "--gpu_net_subset"], b"--gpu_net_subset needs --gpu_net"),
    (["--gpu_chain_all", "--gpu_net", "--gpu_net_subset=3"], b"unknown option --gpu_net_subset=3"),
])
def test_flag_errors(pair, flags, message):
    d, tf, qf = pair[:3]
    r = subprocess.run([build_host(), str(tf), str(qf), "./", "--outdir=%s" % d] + flags, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and message in r.stderr
