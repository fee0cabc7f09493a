"""GPU: segalign_host --gpu_chain_all --gpu_net --gpu_net_subset --gpu_lift=FILE[,num/den], on the input of test_gpu_host_chain.py.  Next
to every .net.chains file a .lifted.bed and an .unlifted.bed file hold the BED lines of FILE lifted through that file's sub-chains
(sa_lift_intervals, DESIGN.md 23: the query as the other axis, group = the target record, ogroup = the query record, every ostrand 0).
Both must equal the rendering of tests/lift_model.py on the sub-chains of tests/net_subset_model.py; every other file equals a run
without the flag, byte for byte.

The BED file is generated here, with a fixed seed, from the oracle's .segments files of this input: pieces of HSPs, HSPs with margins of
several lengths, random intervals of a fixed length mix, and lines that no file takes (an unknown record, an end past the record).  The
sub-chains of a net have disjoint hulls, so a line is Duplicated only under a ratio of at most 1/2: the run uses 1/4.  The test asserts
from the models first that MAPPED and each of the three reasons occur in each strand's files, and prints the counts."""
import subprocess

import numpy as np
import pytest

import gapped_model as G
import hsp_chain_all_model as A
import lift_model as L
import net_model as N
import net_subset_model as NS
from host_model import expected_outputs
from segalign_amd.build import build_host
from test_gpu_gapped_host import run
from test_gpu_gapped_maf_host import rc_text
from test_gpu_host_chain import file_hsps, pair  # noqa: F401  (pair: the module's fixture, built anew here)

pytestmark = pytest.mark.gpu
RATIO = (1, 4)
FLAGS = ["--gpu_chain_all", "--gpu_net", "--gpu_net_subset"]


def make_bed(segments, R):
    """segments: {name: text} of the .segments files.  -> the BED text."""
    rng = np.random.default_rng(2391)
    out = []
    for f in sorted(segments):
        rows = segments[f].splitlines()
        for k in rng.choice(len(rows), size=min(40, len(rows)), replace=False):
            name, rs, re_ = rows[int(k)].split("\t")[:3]
            a, b, top = int(rs) - 1, int(re_), R.chr_len[R.chr_name.index(name)]
            out.append((name, a + (b - a) // 4, b - (b - a) // 4))  # a piece of the HSP
            for margin in (2, (b - a) // 3, 2 * (b - a), 30 * (b - a)):  # the HSP and so much on both sides
                out.append((name, max(0, a - margin), min(top, b + margin)))
    for name, n in zip(R.chr_name, R.chr_len):
        for length in (1, 100, 10_000):
            for s in rng.integers(0, n - length, 25):
                out.append((name, int(s), int(s) + length))
        out.append((name, n - 10, n + 5))  # past the record's end: in no file
    out.append(("chrZ", 10, 20))  # no record of the target: in no file
    order = rng.permutation(len(out))
    lines = ["# made by the test"]
    for i, k in enumerate(order):
        name, s, e = out[int(k)]
        lines.append("%s\t%d\t%d" % (name, s, e) + ("\tiv%d\t%d\t+" % (i, i % 1000) if i % 3 else ""))
    return "".join(x + "\n" for x in lines)


def file_lift(text, rev, R, Q, bed):
    """The models on one .segments file: -> (.lifted.bed text, .unlifted.bed text, the lift's stats)."""
    names, starts = (Q.rc_name, Q.rc_start) if rev else (Q.chr_name, Q.chr_start)
    r_text = bytes(R.buf[:R.block_len[0]]).decode()
    q_text = bytes(Q.buf[:Q.block_len[0]]).decode()
    t, q = NS.encode(r_text.encode()), NS.encode((rc_text(q_text) if rev else q_text).encode())
    h, g = file_hsps(text, rev, R, Q)
    pairs = sorted({(int(np.searchsorted(R.chr_start, int(x["ref_start"]), side="right")) - 1,
                     int(np.searchsorted(starts, int(x["query_start"]), side="right")) - 1) for x in h})
    _, _, chains, members, _ = A.chain_all(h, g)
    mem = members["hsp_index"].astype(np.uint32)
    first = np.concatenate([chains["first_member"], [members.size]]).astype(np.uint32)
    bs, be = NS.blocks(h, mem, "target")
    fills, _ = N.net(first, bs, be, chains["score"], np.array([pairs[c][0] for c in chains["group"]], dtype=np.uint32))
    hs, ch, _ = NS.subset(t, q, G.SUB, h, mem, first, fills)
    smem, sfirst = NS.csr(ch)
    group = np.searchsorted(R.chr_start, ch["ref_start"], side="right") - 1
    ogroup = np.searchsorted(starts, ch["query_start"], side="right") - 1
    lines = []
    for x in L.parse_bed(bed):
        if x[1] in R.chr_name and x[3] <= R.chr_len[R.chr_name.index(x[1])]:  # one target block: every line of a record inside it
            lines.append(x)
    rec_of = [R.chr_name.index(x[1]) for x in lines]
    ivs = [R.chr_start[r] + x[2] for r, x in zip(rec_of, lines)]
    ive = [R.chr_start[r] + x[3] for r, x in zip(rec_of, lines)]
    rec, _, _, st = L.lift(sfirst, *(NS.blocks(hs, smem, "target") + NS.blocks(hs, smem, "query")), ivs, ive, group=group, ogroup=ogroup,
                           iv_group=rec_of, min_match=RATIO)
    return L.render_bed(lines, rec, names, starts, "-" if rev else "+") + (st,)


def test_host_writes_lifted_and_unlifted_files(oracle, pair):
    d, tf, qf, t_recs, q_recs, R, Q = pair
    files, _ = expected_outputs(oracle, [(n, s.tobytes()) for n, s in t_recs], [(n, s.tobytes()) for n, s in q_recs], chunk=20000)
    segs = sorted(f for f in files if f.endswith(".segments"))
    assert len(segs) == 2 and {".minus." in f for f in segs} == {False, True} and len(R.block_len) == 1
    bed = make_bed({f: files[f] for f in segs}, R)
    want = {}
    for f in segs:
        lifted, unlifted, st = file_lift(files[f], ".minus." in f, R, Q, bed)
        print(f, dict(zip(L.NAMES, st["n_status"])), "candidates", st["candidates"])
        assert all(n >= 1 for n in st["n_status"]), (f, st)  # MAPPED and each of the three reasons
        assert all(unlifted.count(r + "\n") == st["n_status"][k] for k, r in L.REASONS.items()) and lifted.count("\n") == st["n_status"][L.MAPPED]
        want[f[:-len("segments")] + "lifted.bed"] = lifted
        want[f[:-len("segments")] + "unlifted.bed"] = unlifted
    bed_file = d / "intervals.bed"
    bed_file.write_text(bed)
    base, base_out = run(build_host(), tf, qf, d / "lift_base", FLAGS)
    assert all(base[f] == files[f] for f in segs)  # the oracle's files are the host's
    got, got_out = run(build_host(), tf, qf, d / "lift", FLAGS + ["--gpu_lift=%s,%d/%d" % ((bed_file,) + RATIO)])
    assert got_out == base_out
    assert sorted(got) == sorted(list(base) + list(want))
    assert all(got[f] == base[f] for f in base)
    for f, text in want.items():
        assert got[f] == text, f
    # the default ratio, 95/100: no line is Duplicated, and the lifted lines are among those of the run above
    strict, _ = run(build_host(), tf, qf, d / "lift_strict", FLAGS + ["--gpu_lift=%s" % bed_file])
    for f in want:
        assert "#Duplicated" not in strict[f] and (not f.endswith(".lifted.bed") or 0 < strict[f].count("\n") <= got[f].count("\n"))


@pytest.mark.parametrize("flags,message", [
    (["--gpu_lift=x.bed"], b"--gpu_lift needs --gpu_net_subset, --gpu_net and --gpu_chain_all"),
    (["--gpu_chain_all", "--gpu_net", "--gpu_lift=x.bed"], b"--gpu_lift needs --gpu_net_subset"),
    (FLAGS + ["--gpu_lift=x.bed,3/2"], b"bad --gpu_lift=x.bed,3/2"),
    (FLAGS + ["--gpu_lift=x.bed,1/0"], b"bad --gpu_lift=x.bed,1/0"),
    (FLAGS + ["--gpu_lift=x.bed,1/1048577"], b"bad --gpu_lift=x.bed,1/1048577"),
    (FLAGS + ["--gpu_lift="], b"bad --gpu_lift="),
    (FLAGS + ["--gpu_lift"], b"unknown option --gpu_lift"),
])
def test_flag_errors(pair, flags, message):
    d, tf, qf = pair[:3]
    r = subprocess.run([build_host(), str(tf), str(qf), "./", "--outdir=%s" % d] + flags, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and message in r.stderr


def test_a_missing_and_a_malformed_bed_file(pair):
    d, tf, qf = pair[:3]
    r = subprocess.run([build_host(), str(tf), str(qf), "./", "--outdir=%s" % d, "--num_gpu=1"] + FLAGS + ["--gpu_lift=%s" % (d / "none.bed")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode != 0 and b"none.bed" in r.stderr
    bad = d / "bad.bed"
    bad.write_text("chrA\t10\t20\nchrA\t30\t30\n")
    r = subprocess.run([build_host(), str(tf), str(qf), "./", "--outdir=%s" % d, "--num_gpu=1"] + FLAGS + ["--gpu_lift=%s" % bad],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 1 and b"line 2 is no BED line" in r.stderr
