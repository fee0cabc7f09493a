"""GPU: segalign_host --gpu_chain_costs=loose|medium|FILE with --gpu_chain or --gpu_chain_all, on the input of test_gpu_host_chain.py.
The .chain / .chains files must equal the rendering of tests/hsp_chain_gap_model.py on the HSPs of the .segments file beside them
(sa_chain_hsps_costs, sa_chain_hsps_all_costs).  The model first shows that the table changes the chains of a file: the
.chains files, which carry the chains' scores and order; on this input every HSP scores above the presets' costs of the gaps between
neighbours, so the best chains keep their members and the .chain files, which show members only, stay as they were.  Without the flag the host writes what tests/host_model.py says, and with it every file it wrote before stays byte for byte."""
import subprocess

import pytest

import hsp_chain_gap_model as GM
import hsp_chain_model as M
from host_model import expected_outputs
from segalign_amd.build import build_host
from test_gpu_gapped_host import run
from test_gpu_host_chain import chain_text, file_hsps, pair  # noqa: F401  (pair: the module's fixture, built anew here)
from test_gpu_host_chain_all import chains_text

pytestmark = pytest.mark.gpu

HAND = {"pos": [2, 10, 100, 1000], "q_gap": [5, 50, 60, 60], "t_gap": [7, 7, 700, 800], "both_gap": [20, 30, 300, 3000]}
HAND_FILE = """# four break points
tableSize    4
smallSize    111
position 2 10 100 1000
qGap 5 50 60 60
tGap 7 7 700 800
bothGap 20 30 300 3000
"""


@pytest.fixture(scope="module")
def plain(pair):
    d, tf, qf = pair[:3]
    return run(build_host(), tf, qf, d / "plain", [])


def segments(files):
    return sorted(f for f in files if f.endswith(".segments"))


def test_the_best_chains_under_the_medium_table(oracle, pair, plain):
    d, tf, qf, t_recs, q_recs, R, Q = pair
    files, cmds = expected_outputs(oracle, [(n, s.tobytes()) for n, s in t_recs], [(n, s.tobytes()) for n, s in q_recs], chunk=20000)
    assert plain[0] == files and plain[1] == sorted(cmds + [""])  # without the flag: the reference host's files and lines
    want, lower = {}, 0
    for f in segments(plain[0]):
        rev = ".minus." in f
        h, g = file_hsps(plain[0][f], rev, R, Q)
        members = GM.chain(h, g, diag_pen=1, gap_costs="medium")[2]
        want[f[:-len("segments")] + "chain"] = chain_text(h, members, rev, R, Q)
        lower += int(members["f"][-1]) < int(M.chain(h, g, diag_pen=1)[2]["f"][-1])
    assert lower > 0, "the table must cost a chain something"
    got, got_out = run(build_host(), tf, qf, d / "chain_medium", ["--gpu_chain=1,0", "--gpu_chain_costs=medium"])
    assert got_out == plain[1]
    assert sorted(got) == sorted(list(plain[0]) + list(want)) and all(got[f] == plain[0][f] for f in plain[0])
    for f in want:
        assert got[f] == want[f], f


def test_all_chains_under_a_table_from_a_file(pair, plain):
    d, tf, qf, t_recs, q_recs, R, Q = pair
    table = d / "hand.linearGap"
    table.write_text(HAND_FILE)
    kw = dict(max_gap=3000, min_score=6000)
    want, differ = {}, 0
    for f in segments(plain[0]):
        rev = ".minus." in f
        h, g = file_hsps(plain[0][f], rev, R, Q)
        _, _, chains, members, _ = GM.chain_all(h, g, gap_costs=HAND, **kw)
        want[f[:-len("segments")] + "chains"] = chains_text(h, chains, members, rev, R, Q)
        _, _, chains, members, _ = GM.chain_all(h, g, **kw)
        differ += want[f[:-len("segments")] + "chains"] != chains_text(h, chains, members, rev, R, Q)
    assert differ > 0, "the table must change the chains of a file"
    got, got_out = run(build_host(), tf, qf, d / "chains_file",
                       ["--gpu_chain_all", "--gpu_chain_gap=3000", "--gpu_chain_min=6000", "--gpu_chain_costs=%s" % table])
    assert got_out == plain[1]
    assert sorted(got) == sorted(list(plain[0]) + list(want)) and all(got[f] == plain[0][f] for f in plain[0])
    for f in want:
        assert got[f] == want[f], f


@pytest.mark.parametrize("flags,text,message", [
    (["--gpu_chain_costs=medium"], None, b"--gpu_chain_costs needs --gpu_chain or --gpu_chain_all"),
    (["--gpu_gapped", "--gpu_chain_costs=loose"], None, b"--gpu_chain_costs needs --gpu_chain or --gpu_chain_all"),
    (["--gpu_chain", "--gpu_chain_costs=tight"], None, b"bad --gpu_chain_costs=tight"),
    (["--gpu_chain_all", "--gpu_chain_costs=FILE"], HAND_FILE.replace("tableSize    4", "tableSize    5"), b"tableSize values"),
    (["--gpu_chain_all", "--gpu_chain_costs=FILE"], HAND_FILE.replace("tableSize    4", "tableSize    17"), b"tableSize is not in 1 .. 16"),
    (["--gpu_chain", "--gpu_chain_costs=FILE"], HAND_FILE.replace("qGap 5 50 60 60", "qGap 5 50 60 sixty"), b"not an integer"),
    (["--gpu_chain", "--gpu_chain_costs=FILE"], HAND_FILE.replace("tGap", "uGap"), b"unknown or repeated line uGap"),
    (["--gpu_chain", "--gpu_chain_costs=FILE"], HAND_FILE.replace("bothGap 20 30 300 3000\n", ""), b"no bothGap line"),
    (["--gpu_chain", "--gpu_chain_costs=FILE"], HAND_FILE.replace("position 2 10", "position 10 10"), b"position must ascend"),
    (["--gpu_chain", "--gpu_chain_costs=FILE"], HAND_FILE.replace("qGap 5 50", "qGap 50 5"), b"qGap must be non-decreasing"),
    (["--gpu_chain", "--gpu_chain_costs=FILE"], HAND_FILE.replace("bothGap 20 30 300", "bothGap 20 16404 16404"), b"bothGap rises by 2048 or more per base"),
], ids=["no chain flag", "gapped only", "unknown preset", "too few values", "too many points", "not an integer", "unknown line", "missing line",
        "positions", "costs descend", "too steep"])
def test_flag_errors(tmp_path, pair, flags, text, message):
    d, tf, qf = pair[:3]
    if text is not None:
        (tmp_path / "table").write_text(text)
        flags = [x.replace("FILE", str(tmp_path / "table")) for x in flags]
    r = subprocess.run([build_host(), str(tf), str(qf), "./", "--outdir=%s" % tmp_path] + flags, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and message in r.stderr
    assert not list(tmp_path.glob("*.segments")), "the run must end before any work"
