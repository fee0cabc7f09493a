"""CPU: the contract of sa_diff_alignments (include/segalign_amd.h).  Three statements of it are held equal on random
spans: the model by column expansion (tests/diff_model.py), the serial checker that walks the op entries (tests/cpp/diff_check.c, run
as a stand-alone program under the sanitizers and never loaded into Python) and a brute force written here that takes one column at a
time.  Then one hand case per clause, the messages of checked_spans through a small g++ program of its own, and the engine's
Python layer held to the model's layouts."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import diff_model as D

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
M, I, Dl = D.OP_M, D.OP_I, D.OP_D


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc")
    exe = str(tmp_path_factory.mktemp("diff_check") / "diff_check_san")
    subprocess.check_call([cc, "-g", "-O1", "-std=c99", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "cpp", "diff_check.c"), os.path.join(HERE, "cpp", "diff_check_main.c"), "-o", exe])
    return exe


def run_checker(exe, tmp, ref, qry, spans, ops, per_base=False, cap=1 << 20):
    """The checker on exactly these arrays: a read past any of them is the sanitizer's error."""
    ops = np.asarray(ops, dtype=np.uint32)
    src, dst = str(tmp / "in.bin"), str(tmp / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<6I", ref.size, qry.size, len(spans), ops.size, int(per_base), cap))
        f.write(np.asarray(ref, dtype=np.uint8).tobytes() + np.asarray(qry, dtype=np.uint8).tobytes() + spans.tobytes() + ops.tobytes())
    r = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-800:])
    raw = open(dst, "rb").read()
    n = struct.unpack_from("<Q", raw)[0]
    kept = min(n, cap)
    ev = np.frombuffer(raw, dtype=D.EVENT_DTYPE, count=kept, offset=8)
    sm = np.frombuffer(raw, dtype=D.SUMMARY_DTYPE, count=len(spans), offset=8 + 24 * kept)
    pairs = np.frombuffer(raw, dtype=np.uint64, count=64, offset=8 + 24 * kept + 48 * len(spans))
    assert len(raw) == 8 + 24 * kept + 48 * len(spans) + 512
    return n, ev, sm, pairs


def brute(ref, qry, spans, ops, per_base=False):
    """One column at a time, written without a look at the model: -> (events as tuples, summaries as dicts, pairs)."""
    events, sums, pairs = [], [], [0] * 64
    for k, sp in enumerate(spans):
        r, q, col, prev = int(sp["ref_start"]), int(sp["query_start"]), 0, None
        s = dict(first_event=len(events), columns=0, matches=0, transitions=0, transversions=0, others=0, ins_runs=0, ins_bases=0,
                 del_runs=0, del_bases=0)
        for word in ops[int(sp["op_offset"]):int(sp["op_offset"]) + int(sp["n_ops"])]:
            code = int(word) & 3
            for _ in range(int(word) >> 2):
                if code == M:
                    x, y = int(ref[r]) & 7, int(qry[q]) & 7
                    pairs[x * 8 + y] += 1
                    if x > 3 or y > 3:
                        kind, name = D.OTHER, "others"
                    elif x == y:
                        kind, name = None, "matches"
                    else:
                        kind, name = D.SUB, "transitions" if {x, y} in ({0, 2}, {1, 3}) else "transversions"
                    s[name] += 1
                elif code == I:
                    kind, x, y = D.INS, 8, int(qry[q]) & 7
                    s["ins_bases"] += 1
                else:
                    kind, x, y = D.DEL, int(ref[r]) & 7, 8
                    s["del_bases"] += 1
                if kind is not None:
                    if kind == prev and not (per_base and kind == D.SUB):
                        events[-1][3] += 1
                    else:
                        events.append([k, r, q, 1, col, kind, x, y, 0])
                    if kind != prev and kind == D.INS:
                        s["ins_runs"] += 1
                    if kind != prev and kind == D.DEL:
                        s["del_runs"] += 1
                prev = kind
                r, q, col = r + (code != I), q + (code != Dl), col + 1
        s["columns"], s["n_events"] = col, len(events) - s["first_event"]
        sums.append(s)
    return [tuple(e) for e in events], sums, pairs


def random_case(rng, n_spans=40, size=600):
    """Sequences of every code, short runs of equal codes so that matches occur, and spans of a few entries each with holes between
    their op ranges."""
    codes = np.array([0, 1, 2, 3, 0, 1, 2, 3, 0, 2, 4, 5, 6, 7], dtype=np.uint8)
    ref = codes[rng.integers(0, codes.size, size)] | (rng.integers(0, 2, size) << 3).astype(np.uint8)  # a high bit no one may read
    qry = ref.copy()
    hit = rng.random(size) < 0.35
    qry[hit] = codes[rng.integers(0, codes.size, int(hit.sum()))]
    rows, ops = [], []
    for _ in range(n_spans):
        runs = [(int(rng.integers(1, 30)), int(rng.choice([M, M, M, I, Dl]))) for _ in range(int(rng.integers(0, 7)))]
        tb, qb = sum(n for n, c in runs if c != I), sum(n for n, c in runs if c != Dl)
        rs = int(rng.integers(0, size - tb + 1))
        qs = int(np.clip(rs + rng.integers(-2, 3), 0, size - qb))
        ops += [D.op(9, 3)] * int(rng.integers(0, 3))  # ops no span names
        rows.append((rs, qs, len(ops), len(runs)))
        ops += [D.op(n, c) for n, c in runs]
    return ref, qry, D.make_spans(rows), np.array(ops, dtype=np.uint32)


@pytest.mark.parametrize("per_base", [False, True])
def test_model_checker_and_brute_force_agree_on_random_spans(checker, tmp_path, per_base):
    rng = np.random.default_rng(11 + per_base)
    kinds = set()
    for _ in range(12):
        ref, qry, spans, ops = random_case(rng)
        ev, sm, pairs = D.diff(ref, qry, spans, ops, per_base)
        n, c_ev, c_sm, c_pairs = run_checker(checker, tmp_path, ref, qry, spans, ops, per_base)
        assert n == ev.size and np.array_equal(c_ev, ev) and np.array_equal(c_sm, sm) and np.array_equal(c_pairs, pairs)
        b_ev, b_sm, b_pairs = brute(ref, qry, spans, ops, per_base)
        assert [tuple(int(x) for x in e) for e in ev] == b_ev and pairs.tolist() == b_pairs
        for k, s in enumerate(b_sm):
            assert {f: int(sm[k][f]) for f in D.SUMMARY_DTYPE.names} == s
        kinds |= set(ev["kind"].tolist())
        assert np.all(sm["columns"] == sm["matches"] + sm["transitions"] + sm["transversions"] + sm["others"] + sm["ins_bases"] + sm["del_bases"])
    assert kinds == {D.SUB, D.OTHER, D.INS, D.DEL}


def test_the_checker_counts_past_a_small_output_array(checker, tmp_path):
    ref, qry, spans, ops = random_case(np.random.default_rng(3))
    ev, sm, pairs = D.diff(ref, qry, spans, ops)
    n, c_ev, c_sm, _ = run_checker(checker, tmp_path, ref, qry, spans, ops, cap=5)
    assert n == ev.size > 5 and np.array_equal(c_sm, sm) and np.array_equal(c_ev[:4], ev[:4])


# ---- one hand case per clause: target and query as strings, codes as the engine makes them ----

CODE = {c: k for k, c in enumerate("ACGT")}
CODE.update({"a": 4, "N": 5, "R": 6, "&": 7})


def hand(t, q, alignments, per_base=False):
    ref, qry = np.array([CODE[c] for c in t], dtype=np.uint8), np.array([CODE[c] for c in q], dtype=np.uint8)
    spans, ops = D.pack(alignments)
    ev, sm, pairs = D.diff(ref, qry, spans, ops, per_base)
    return [tuple(int(x) for x in e)[:8] for e in ev], sm, pairs


def test_classes():
    ev, sm, pairs = hand("ACGTAAAA" "aNR&A", "ACGTGCTA" "AAAAN", [(0, 0, [(13, M)])])
    s = sm[0]
    assert (int(s["matches"]), int(s["transitions"]), int(s["transversions"]), int(s["others"])) == (5, 1, 2, 5)
    assert pairs[0 * 8 + 2] == 1 and pairs[4 * 8 + 0] == pairs[5 * 8 + 0] == pairs[6 * 8 + 0] == pairs[7 * 8 + 0] == pairs[0 * 8 + 5] == 1
    assert int(pairs.sum()) == 13
    assert hand("aN", "aN", [(0, 0, [(2, M)])])[1][0]["others"] == 2  # equal codes of 4 or more are no match


def test_columns_consume_as_their_ops_say_and_events_report_the_next_bases():
    ev, sm, _ = hand("AACCGG", "AATTTCCGG", [(0, 0, [(2, M), (3, I), (2, M), (2, Dl)])])
    assert ev == [(0, 2, 2, 3, 2, D.INS, 8, 3), (0, 4, 7, 2, 7, D.DEL, 2, 8)]  # the insertion sits in front of target base 2
    assert (int(sm[0]["columns"]), int(sm[0]["matches"]), int(sm[0]["ins_bases"]), int(sm[0]["del_bases"])) == (9, 4, 3, 2)


def test_runs_cross_entries_and_never_spans():
    t, q = "AAAAAAAA", "AACCAAAA"
    assert hand(t, q, [(0, 0, [(3, M), (5, M)])])[0] == [(0, 2, 2, 2, 2, D.SUB, 0, 1)]           # one run over two M entries
    assert hand(t, q, [(0, 0, [(3, M)]), (3, 3, [(5, M)])])[0] == [(0, 2, 2, 1, 2, D.SUB, 0, 1), (1, 3, 3, 1, 0, D.SUB, 0, 1)]
    ev, sm, _ = hand(t, t, [(0, 0, [(2, M), (1, I), (2, I), (1, Dl), (2, M)])])
    assert [(e[3], e[5]) for e in ev] == [(3, D.INS), (1, D.DEL)] and int(sm[0]["ins_runs"]) == 1 and int(sm[0]["del_runs"]) == 1
    ev, sm, _ = hand(t, t, [(0, 0, [(1, I), (1, Dl), (1, I)])])
    assert [(e[3], e[5], e[4]) for e in ev] == [(1, D.INS, 0), (1, D.DEL, 1), (1, D.INS, 2)] and int(sm[0]["ins_runs"]) == 2


def test_kinds_split_runs_but_transitions_and_transversions_do_not():
    assert [e[3:6] for e in hand("AAAA", "AGCA", [(0, 0, [(4, M)])])[0]] == [(2, 1, D.SUB)]
    assert [e[3:6] for e in hand("AAAAA", "ACNCA", [(0, 0, [(5, M)])])[0]] == [(1, 1, D.SUB), (1, 2, D.OTHER), (1, 3, D.SUB)]
    assert [e[3:6] for e in hand("AAAAA", "ACCCA", [(0, 0, [(5, M)])])[0]] == [(3, 1, D.SUB)]


def test_per_base_splits_substitutions_only():
    ev, sm, _ = hand("AAAAAAAA", "ACGNNAAA", [(0, 0, [(5, M), (2, I)])], per_base=True)
    assert [e[3:6] for e in ev] == [(1, 1, D.SUB), (1, 2, D.SUB), (2, 3, D.OTHER), (2, 5, D.INS)] and int(sm[0]["n_events"]) == 4


def test_empty_spans_and_first_event():
    ev, sm, _ = hand("AAAA", "ACAC", [(0, 0, []), (0, 0, [(4, M)]), (2, 2, []), (0, 0, [(2, M)])])
    assert sm["n_events"].tolist() == [0, 2, 0, 1] and sm["first_event"].tolist() == [0, 0, 2, 2] and sm["columns"].tolist() == [0, 4, 0, 2]


def test_work_items():
    spans, ops = D.pack([(0, 0, [(4096, M), (4097, M), (9, I), (1, M), (70000, Dl)])])
    assert D.work_items(spans, ops) == 1 + 2 + 1 + 1 + 1 and D.work_items(spans, ops, 64) == 64 + 65 + 1 + 1 + 1


# ---- checked_spans ----

CHECKS_SRC = os.path.join(HERE, "cpp", "diff_checks_main.cpp")
GOOD = {"ok": "5 40", "no_spans": "0 0", "chunk_64_and_both_flags": "5 40", "chunk_65536": "5 40", "most_columns": "4294967295"}
BAD = {
    "too_many_spans": "4194305 spans: at most 1 << 22",
    "too_many_ops": "268435457 ops: at most 1 << 28",
    "ranges_overlap": "span 0: its ops overlap those of span 1 or lie behind them",
    "ranges_descend": "span 1: its ops overlap those of span 2 or lie behind them",
    "last_range_leaves_the_array": "span 2: its ops leave the array of 6",
    "range_wraps": "span 2: its ops leave the array of 6",
    "code_3": "span 0: op 1 has code 3",
    "zero_run": "span 2: op 1 has a zero run",
    "overlap_before_code_3": "span 0: its ops overlap those of span 1 or lie behind them",
    "past_the_target": "span 2 does not lie inside the block",
    "past_the_query": "span 2 does not lie inside the block",
    "past_the_target_by_a_deletion": "span 0 does not lie inside the block",
    "code_3_before_past_the_target": "span 0: op 0 has code 3",
    "too_many_columns": "span 0 has 4294967296 columns: fewer than 2^32",
    "chunk_32": "chunk = 32: 0 or a power of two in 64 .. 65536",
    "chunk_96": "chunk = 96: 0 or a power of two in 64 .. 65536",
    "chunk_131072": "chunk = 131072: 0 or a power of two in 64 .. 65536",
    "unknown_flag": "flags = 4: unknown bits",
    "bad_chunk_before_unknown_flag": "chunk = 100: 0 or a power of two in 64 .. 65536",
}


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("diff_checks") / "diff_checks_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "segalign_amd", "csrc"), CHECKS_SRC, "-o", exe])
    return exe


@pytest.mark.parametrize("case", sorted(GOOD))
def test_good_spans_pass_with_their_totals(probe, case):
    r = subprocess.run([probe, case], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert (r.returncode, r.stdout, r.stderr) == (0, GOOD[case].encode() + b"\n", b"")


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_spans_end_in_exactly_their_message(probe, case):
    r = subprocess.run([probe, case], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert (r.returncode, r.stdout, r.stderr) == (1, b"", b"Error: Probe: " + BAD[case].encode() + b"\n")


def test_every_case_of_the_probe_is_held():
    with open(CHECKS_SRC) as f:
        cases = re.findall(r'if \(c == "(\w+)"\)', f.read())
    assert sorted(cases) == sorted(list(GOOD) + list(BAD)) and len(cases) == len(set(cases))


# ---- the Python layer ----

def test_the_engine_layer_has_the_models_layouts_and_the_entry():
    from segalign_amd import engine as E
    assert E.DIFF_SPAN_DTYPE == D.SPAN_DTYPE and E.DIFF_EVENT_DTYPE == D.EVENT_DTYPE and E.DIFF_SUMMARY_DTYPE == D.SUMMARY_DTYPE
    assert callable(E.DiffAlignments) and {"sa_diff_alignments", "sa_free_diff"} <= set(E.C_ABI_SYMBOLS)
    assert (E.DIFF_SUB, E.DIFF_OTHER, E.DIFF_INS, E.DIFF_DEL, E.DIFF_NO_CODE) == (D.SUB, D.OTHER, D.INS, D.DEL, D.NO_CODE)
    stitch = np.zeros(2, dtype=E.STITCH_RECORD_DTYPE)
    stitch["ref_start"], stitch["query_start"], stitch["op_offset"], stitch["n_ops"] = [5, 9], [6, 10], [0, 3], [3, 2]
    sp = E.diff_spans(stitch)
    assert sp.dtype == D.SPAN_DTYPE and sp["op_offset"].tolist() == [0, 3] and sp["n_ops"].tolist() == [3, 2] and sp["query_start"].tolist() == [6, 10]
    rec = np.zeros(1, dtype=E.GAPPED_DTYPE)
    path = np.zeros(1, dtype=E.PATH_DTYPE)
    rec["ref_start"], rec["query_start"], path["op_offset"], path["n_left"], path["n_right"] = 7, 8, 4, 2, 3
    sp = E.diff_spans(rec, path)
    assert (int(sp[0]["ref_start"]), int(sp[0]["query_start"]), int(sp[0]["op_offset"]), int(sp[0]["n_ops"])) == (7, 8, 4, 5)
