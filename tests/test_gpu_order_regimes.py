"""GPU: sa_order_hsps_segs -- the ordering stage as a call runs it: dedup_seg_kernel with its workgroup size, capacity, device-side count and
the host step that closes its gaps, or the library sorts with unique_kernel / the tiled unique kernels and strip_kernel -- on the
hand-built inputs of tests/order_regimes.py, held to tests/order_model.py: the records, the segment of every record and the per-segment
counts, field for field.  tests/test_order_regimes.py shows on the CPU that each input is in the regime it names, and
tests/test_order_model.py that the model equals the oracle on all of them.  The entry needs no sequence."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import order_regimes as R
from test_gpu_thrust_order import build_thrust_order, thrust_chain

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREADS = (0, 64, 192, 1024)


@pytest.fixture(scope="module")
def E(engine):
    engine.InitializeInterface(1)
    return engine


def same(got, want, what):
    recs, seg, counts, refused = got
    assert not refused, what
    assert np.array_equal(counts, want["counts"]), what
    assert np.array_equal(seg, want["seg"]), what
    assert recs.shape == want["records"].shape and np.array_equal(recs, want["records"]), what


def run(E, reg, rm=False, path=1, **kw):
    return E.OrderHspsSegs(reg.recs, reg.seg, reg.nsegs, rm=rm, path=path, **kw)


def hold(E, reg, threads=THREADS, seg_max=0):
    """path 0 under every workgroup size with the count on the host and on the device where the input fits it, path 1 always"""
    if reg.lds:
        for t in threads:
            for dev in (False, True):
                same(run(E, reg, path=0, threads=t, seg_max=seg_max, count_on_device=dev), reg.model(), (reg, "path 0", t, dev))
    same(run(E, reg, path=1), reg.model(), (reg, "path 1"))
    if reg.rm_too:
        same(run(E, reg, rm=True, path=1), reg.model(True), (reg, "path 1 rm"))


@pytest.mark.parametrize("m", R.LDS_SIZES)
def test_lds_chain_sizes(E, m):
    regs = [R.size_distinct(m), R.size_tower(m)] + [R.size_across(m, m2) for m2 in (1025, 1024, 1023) if 1024 < m and m2 < m]
    for reg in regs:
        hold(E, reg)


@pytest.mark.parametrize("kind", ["drop", "chain", "corner"])
@pytest.mark.parametrize("T", R.LDS_THREADS)
def test_lds_unique_tile_edges(E, T, kind):
    hold(E, R.lds_tile_edge(T, kind))      # (under T its edges are tile edges; under the other sizes they lie inside a tile)


@pytest.mark.parametrize("n", R.LIB_SIZES)
def test_library_unique_edges(E, n):
    for v in (0, 1):
        hold(E, R.lib_edges(n, v))
        hold(E, R.lib_edges_rm(n, v))


@pytest.mark.parametrize("nsegs", R.SEG_COUNTS)
def test_lds_segments(E, nsegs):
    hold(E, R.seg_mix(nsegs))


def test_lds_segment_511_alone(E):
    hold(E, R.seg_last_only())


def test_lds_every_segment_at_capacity_at_the_total_limit(E):
    hold(E, R.seg_full())


@pytest.mark.parametrize("kind", R.REFUSALS)
def test_refusals_and_the_fallback(E, kind):
    reg = R.refusal(kind)
    f = reg.facts
    for t in THREADS:
        for dev in ((False, True) if f["on_device"] == "both" else (True,)):
            got = run(E, reg, path=0, threads=t, seg_max=f["seg_max"], count_on_device=dev)
            if f["refused"]:
                assert got[3] and got[0].size == 0 and got[1].size == 0 and not got[2].any(), (reg, t, dev)
            else:
                same(got, reg.model(), (reg, t, dev))
    same(run(E, reg, path=1), reg.model(), (reg, "path 1 after the refusal"))


@pytest.mark.parametrize("n", [9000, 40961])
def test_library_segment_breaks(E, n):
    hold(E, R.lib_seg_breaks(n))


@pytest.mark.parametrize("rm", [False, True])
def test_strip_kernel_strides(E, rm):
    reg = R.lib_strip_stride()
    same(run(E, reg, rm=rm, path=1), reg.model(rm), (reg, rm))


@pytest.mark.parametrize("kind", R.MAGNITUDES)
def test_magnitudes(E, kind, tmp_path):
    reg = R.magnitudes(kind)
    exe = build_thrust_order()
    for rm in (False, True):
        want = thrust_chain(exe, reg.recs, rm, tmp_path)      # rocThrust's own answer pins the model here as well
        assert np.array_equal(want, reg.model(rm)["records"]), (reg, rm)
    hold(E, reg)


def test_eight_threads_get_the_serial_results(E):
    jobs = [(R.size_across(2048, 1023), False, 0, 64), (R.seg_mix(8), False, 0, 192), (R.seg_mix(512), False, 0, 0),
            (R.lib_edges(16385, 0), False, 1, 0), (R.lib_edges_rm(16385, 1), True, 1, 0), (R.lib_seg_breaks(40961), False, 1, 0),
            (R.refusal("one-oversized"), False, 0, 1024), (R.lds_tile_edge(192, "chain"), False, 0, 192)]
    out, errors = [None] * 8, []

    def work(i):
        try:
            reg, rm, path, t = jobs[i]
            out[i] = run(E, reg, rm=rm, path=path, threads=t, count_on_device=bool(i & 1))
        except Exception as ex:  # pragma: no cover
            errors.append(ex)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    for i, (reg, rm, path, t) in enumerate(jobs):
        if reg.facts.get("refused"):
            assert out[i][3] and out[i][0].size == 0
        else:
            same(out[i], reg.model(rm), (reg, "thread", i))


CHILD = """
import sys
sys.path.insert(0, %r)
import numpy as np
from segalign_amd import engine as E
E.InitializeInterface(1)
n, nsegs, rm, top = %d, %d, %d, %d
h = np.zeros(n, dtype=E.SEG_DTYPE)
h["ref_start"] = 100 * np.arange(n)
seg = (np.arange(n) %% nsegs).astype(np.uint32)
seg[-1] = top
E.OrderHspsSegs(h, seg, nsegs, rm=bool(rm), path=0)
print("returned")
"""


@pytest.mark.parametrize("what,n,nsegs,rm,top", [("rm", 10, 2, 1, 1), ("segments", 1000, 513, 0, 512), ("count", 131073, 65, 0, 64),
                                                 ("segment id", 10, 2, 0, 2)])
def test_input_no_call_would_pass_fails_with_a_message(what, n, nsegs, rm, top):
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, n, nsegs, rm, top)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and b"returned" not in r.stdout, r.stderr
    assert b"sa_order_hsps_segs" in r.stderr
