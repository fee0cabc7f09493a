"""CPU: the input rules the post-processing entries share (segalign_amd/csrc/post_checks.h), each held to the whole line
it prints.  tests/cpp/post_checks_main.cpp builds a case's input and calls one check under the entry name "Probe"; plain g++ compiles it,
which is also the check that the header needs neither HIP nor the engine's headers.  The expected lines are the format strings the entries
carried before the header existed (api_stitch.hip, api_chaintrim.hip, api_fill.hip, api_netsubset.hip, api_netclass.hip, api_lift.hip),
filled in by hand: the GPU tests of those entries pin words of these messages through the real entries, this file pins every byte."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "post_checks_main.cpp")

# case -> what a good input prints
GOOD = {
    "first_ok": "5",
    "first_no_chains": "0",
    "first_empty_chain": "3",
    "member_ok": "90 70 9",                       # ends on ref_len and on query_len
    "pairs_ok": "5",
    "pairs_no_chains": "0",
    "pairs_no_ostrand": "2",
    "pairs_other_touches_on_strand_1": "5",
    "fill_ok": "ok",
}

# case -> the message after "Error: Probe: "
BAD = {
    "first_too_many_chains": "4194305 chains: at most 1 << 22",
    "first_not_zero": "first[0] = 1, not 0",
    "first_descends": "first[] decreases at chain 1",
    "first_too_many_members": "4194305 members: at most 1 << 22",
    "first_not_zero_and_descends": "first[0] = 1, not 0",
    "member_not_in_input": "member 1 names HSP 3, which is not in the input",
    "member_past_ref": "member 2 (HSP 2) does not lie inside the block",
    "member_past_query": "member 2 (HSP 2) does not lie inside the block",
    "member_not_in_input_and_outside": "member 0 names HSP 3, which is not in the input",
    "pairs_too_many_chains": "4194305 chains: at most 1 << 22",
    "pairs_first_not_zero": "first[0] = 1, not 0",
    "pairs_first_descends": "first[] decreases at chain 1",
    "pairs_too_many_blocks": "67108865 blocks: at most 1 << 26",
    "pairs_ostrand_2": "ostrand[1] = 2: 0 or 1",
    "pairs_empty_block": "chain 0, block 1: start >= end",
    "pairs_ends_at_top": "chain 1, block 4 ends at or past 2^31",
    "pairs_overlap": "chain 0: its blocks overlap or descend at block 1",
    "pairs_other_empty_block": "chain 1, block 3: start >= end on the other axis",
    "pairs_other_ends_at_top": "chain 0, block 1 ends at or past 2^31 on the other axis",
    "pairs_lengths_differ": "chain 0, block 1: the lengths on the two axes differ",
    "pairs_other_descends_on_strand_0": "chain 0 (ostrand 0): its other blocks overlap or descend at block 1",
    "pairs_other_overlaps_on_strand_0": "chain 0 (ostrand 0): its other blocks overlap or descend at block 1",
    "pairs_other_ascends_on_strand_1": "chain 1 (ostrand 1): its other blocks overlap or ascend at block 4",
    "pairs_other_overlaps_on_strand_1": "chain 1 (ostrand 1): its other blocks overlap or ascend at block 4",
    "pairs_empty_on_both_axes": "chain 0, block 1: start >= end",                               # the axis before the other axis
    "pairs_overlap_and_later_ostrand_2": "chain 0: its blocks overlap or descend at block 1",   # chain 0 before chain 1
    "fill_empty": "fill 3: start >= end",
    "fill_names_chain_n": "fill 3 names chain 2, which is not in the input",
    "fill_no_blocks": "fill 3: its blocks leave chain 1",
    "fill_starts_before_chain": "fill 3: its blocks leave chain 1",
    "fill_runs_past_chain": "fill 3: its blocks leave chain 0",
    "fill_empty_and_names_chain_n": "fill 3: start >= end",
}


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("post_checks") / "post_checks_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "segalign_amd", "csrc"), SRC, "-o", exe])
    return exe


def run(probe, case):
    return subprocess.run([probe, case], stdout=subprocess.PIPE, stderr=subprocess.PIPE)


@pytest.mark.parametrize("case", sorted(GOOD))
def test_good_input_passes_and_returns_its_count(probe, case):
    r = run(probe, case)
    assert (r.returncode, r.stdout, r.stderr) == (0, GOOD[case].encode() + b"\n", b"")


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_input_ends_in_exactly_its_message(probe, case):
    r = run(probe, case)
    assert (r.returncode, r.stdout, r.stderr) == (1, b"", b"Error: Probe: " + BAD[case].encode() + b"\n")


def test_every_case_of_the_program_is_held():
    with open(SRC) as f:
        cases = re.findall(r'if \(c == "(\w+)"\)', f.read())
    assert sorted(cases) == sorted(list(GOOD) + list(BAD)) and len(cases) == len(set(cases))


def test_no_entry_keeps_a_copy_of_its_own():
    csrc = os.path.join(ROOT, "segalign_amd", "csrc")
    for name in sorted(os.listdir(csrc)):
        if name.startswith("api_") and name.endswith(".hip"):
            with open(os.path.join(csrc, name)) as f:
                # a definition starts in column 0 with its return type; calls are indented
                assert not re.findall(r"^\w[\w:<>\* ]*\b(fail|checked_first|checked_blocks|checked_block_pairs)\(", f.read(), re.M), name


def test_the_header_needs_nothing_of_hip_or_the_engine():
    with open(os.path.join(ROOT, "segalign_amd", "csrc", "post_checks.h")) as f:
        inc = re.findall(r'^#include\s+(\S+)', f.read(), re.M)
    assert [i for i in inc if i.startswith('"')] == ['"../../include/segalign_amd.h"'] and not [i for i in inc if "hip" in i]
