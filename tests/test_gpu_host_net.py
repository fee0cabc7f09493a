"""GPU: segalign_host --gpu_chain_all --gpu_net[=min_space] [--gpu_net_fill=N], on the input of test_gpu_host_chain.py.  Next to every
.chains file a .net file holds the target-axis net of the file's kept chains (sa_net_chains): group = the target record of
the chain's pair, score = the chain record's score.  It must equal the rendering of tests/net_model.py on the chains that
tests/hsp_chain_all_model.py makes of the file's HSPs; every other file equals a run with --gpu_chain_all alone, byte for byte."""
import bisect
import subprocess

import numpy as np
import pytest

import hsp_chain_all_model as A
import net_model as N
from segalign_amd.build import build_host
from test_gpu_gapped_host import run
from test_gpu_host_chain import file_hsps, pair  # noqa: F401  (pair: the module's fixture, built anew here)

pytestmark = pytest.mark.gpu


def file_net(text, rev, R, Q, **kw):
    """The model's net of one .segments file: -> (lines of the .net file, fills, number of chains per target record)."""
    names, starts = (Q.rc_name, Q.rc_start) if rev else (Q.chr_name, Q.chr_start)
    h, g = file_hsps(text, rev, R, Q)
    pairs = sorted({(bisect.bisect_right(R.chr_start, int(x["ref_start"])) - 1, bisect.bisect_right(starts, int(x["query_start"])) - 1) for x in h})
    _, _, chains, members, _ = A.chain_all(h, g)
    idx = members["hsp_index"]
    first = np.concatenate([chains["first_member"], [members.size]]).astype(np.uint32)
    assert np.array_equal(first[1:], chains["first_member"] + chains["n_members"])
    bs = h["ref_start"][idx].astype(np.int64)
    be = bs + h["len"][idx] + 1
    target = np.array([pairs[c][0] for c in chains["group"]], dtype=np.uint32)
    fills, st = N.net(first, bs, be, chains["score"], target, **kw)
    lines, last = [], None
    for f in fills:
        ri = int(f["group"])
        if ri != last:
            lines.append("net %s %d\n" % (R.chr_name[ri], R.chr_len[ri]))
            last = ri
        k0, k1 = int(f["first_block"]), int(f["first_block"]) + int(f["n_blocks"]) - 1
        q0 = int(h["query_start"][idx[k0]]) + int(f["start"]) - int(bs[k0])
        q1 = int(h["query_start"][idx[k1]]) + int(f["end"]) - int(bs[k1])
        qi = bisect.bisect_right(starts, q0) - 1
        lines.append("%sfill %d %d %s %s %d %d chain=%d score=%d ali=%d\n" % (
            " " * int(f["depth"]), int(f["start"]) - R.chr_start[ri], int(f["end"]) - int(f["start"]), names[qi], "-" if rev else "+",
            q0 - starts[qi], q1 - q0, int(f["chain"]), int(f["score"]), int(f["ali"])))
    return "".join(lines), fills, {R.chr_name[ri]: int((target == ri).sum()) for ri in np.unique(target)}


@pytest.fixture(scope="module")
def chained(pair):
    d, tf, qf = pair[:3]
    return run(build_host(), tf, qf, d / "chains_only", ["--gpu_chain_all"])


@pytest.mark.parametrize("flags,kw", [(["--gpu_net"], {}), (["--gpu_net=25", "--gpu_net_fill=12"], dict(min_space=25, min_fill=12))])
def test_host_writes_net_files(pair, chained, flags, kw):
    d, tf, qf, t_recs, q_recs, R, Q = pair
    base, base_out = chained
    segs = sorted(f for f in base if f.endswith(".segments"))
    assert len(segs) == 2

    # the regime, from the model: each file holds a fill of depth >= 1, a chain with no fill and a chain with more than one fill
    want, table = {}, []
    for f in segs:
        text, fills, chains = file_net(base[f], ".minus." in f, R, Q, **kw)
        want[f[:-len("segments")] + "net"] = text
        for ri in np.unique(fills["group"]):
            mine = fills[fills["group"] == ri]
            counts = np.unique(mine["chain"], return_counts=True)[1]
            table.append((f, R.chr_name[ri], chains[R.chr_name[ri]], int(mine.size), chains[R.chr_name[ri]] - int(counts.size), int((counts > 1).sum()),
                          int(mine["depth"].max())))
    print("file, target record, chains, fills, chains with no fill, chains with more than one fill, max depth:", table)
    for f in segs:
        rows = [r for r in table if r[0] == f]
        assert max(r[6] for r in rows) >= 1 and sum(r[4] for r in rows) >= 1 and sum(r[5] for r in rows) >= 1, rows

    got, got_out = run(build_host(), tf, qf, d / ("net" + "".join(c for c in "".join(flags) if c.isdigit())), ["--gpu_chain_all"] + flags)
    assert got_out == base_out
    assert sorted(got) == sorted(list(base) + list(want))
    assert all(got[f] == base[f] for f in base)
    for f, text in want.items():
        assert got[f] == text, f


@pytest.mark.parametrize("flags,message", [
    (["--gpu_net"], b"--gpu_net needs --gpu_chain_all"),
    (["--gpu_chain", "--gpu_net=5"], b"--gpu_net needs --gpu_chain_all"),
    (["--gpu_net_fill=3"], b"--gpu_net_fill needs --gpu_net and --gpu_chain_all"),
    (["--gpu_chain_all", "--gpu_net_fill=3"], b"--gpu_net_fill needs --gpu_net"),
    (["--gpu_chain_all", "--gpu_net=0"], b"bad --gpu_net"),
    (["--gpu_chain_all", "--gpu_net", "--gpu_net_fill=x"], b"bad --gpu_net_fill"),
])
def test_flag_errors(pair, flags, message):
    d, tf, qf = pair[:3]
    r = subprocess.run([build_host(), str(tf), str(qf), "./", "--outdir=%s" % d] + flags, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and message in r.stderr
