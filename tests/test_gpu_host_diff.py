"""GPU: segalign_host --gpu_diff[=base], on the input of test_gpu_host_chain.py.  Next to every .maf, .stitched.maf and .net.maf file a
.diff file holds the differences of that file's alignments (sa_diff_alignments); it must equal the rendering of
tests/diff_model.py on the MAF file beside it, whose rows hold every alignment's bases and ops.  Every other file and the host's
output stay byte for byte, and the flag alone is an error."""
import subprocess

import pytest

import diff_model as D
from segalign_amd.build import build_host
from test_gpu_gapped_host import run
from test_gpu_host_chain import pair  # noqa: F401  (the module's fixture, built anew here)

pytestmark = pytest.mark.gpu


def check(pair, name, flags, diff_flag, per_base, mafs):
    d, tf, qf = pair[:3]
    base, base_out = run(build_host(), tf, qf, d / (name + "_base"), flags)
    got, got_out = run(build_host(), tf, qf, d / name, flags + [diff_flag])
    assert got_out == base_out
    maf = sorted(f for f in base if f.endswith(".maf"))
    assert maf and {f.split(".", 4)[-1] for f in maf} == mafs
    assert sorted(got) == sorted(list(base) + [f[:-3] + "diff" for f in maf])
    assert all(got[f] == base[f] for f in base)
    lines = {"sub": 0, "other": 0, "ins": 0, "del": 0, "#a": 0}
    for f in maf:
        text = got[f[:-3] + "diff"]
        assert text == D.render_maf(base[f], per_base), f
        for ln in text.splitlines():
            lines[ln.split()[0]] += 1
    print(name, lines)
    assert lines["#a"] and lines["sub"] and lines["ins"] and lines["del"]
    assert any(".minus." in f and base[f] for f in maf) and any(".plus." in f and base[f] for f in maf)
    return lines


def test_diff_files_beside_the_maf_files(pair):
    check(pair, "diff_maf", ["--gpu_gapped", "--gpu_maf"], "--gpu_diff", False, {"maf"})


def test_diff_files_per_base_beside_the_stitched_files(pair):
    each = check(pair, "diff_stitch", ["--gpu_chain_all", "--gpu_stitch"], "--gpu_diff=base", True, {"stitched.maf"})
    runs = check(pair, "diff_stitch_runs", ["--gpu_chain_all", "--gpu_stitch"], "--gpu_diff", False, {"stitched.maf"})
    assert each["sub"] > runs["sub"] and each["ins"] == runs["ins"]


def test_diff_files_beside_the_net_maf_files(pair):
    check(pair, "diff_net", ["--gpu_chain_all", "--gpu_net", "--gpu_net_subset", "--gpu_stitch"], "--gpu_diff", False, {"stitched.maf", "net.maf"})


@pytest.mark.parametrize("flags,message", [
    (["--gpu_diff"], b"--gpu_diff needs --gpu_maf or --gpu_stitch"),
    (["--gpu_gapped", "--gpu_diff=base"], b"--gpu_diff needs --gpu_maf or --gpu_stitch"),
    (["--gpu_gapped", "--gpu_maf", "--gpu_diff=run"], b"bad --gpu_diff=run"),
])
def test_flag_errors(pair, flags, message):
    d, tf, qf = pair[:3]
    r = subprocess.run([build_host(), str(tf), str(qf), "./", "--outdir=%s" % d] + flags, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and message in r.stderr
