// diff_checks_main.cpp -- tests/test_diff_model.py's probe of checked_spans (segalign_amd/csrc/post_checks.h): one named case per run,
// its input built here, the check called under the entry name "Probe" for a block of 100 by 80 bases.  Good input prints the totals and
// exits 0; bad input ends in the check's own message and exit 1; an unknown case exits 2.
#include <string>
#include <vector>

#include "post_checks.h"

using namespace sa;

namespace {

const Fail fail{"Probe"};
uint32_t op(uint32_t run, uint32_t code) { return run << 2 | code; }

// Three spans over six ops: the second is empty, the third ends on the last base of both sequences.
struct Input {
    std::vector<sa_diff_span> spans = {{10, 10, 0, 3, 0}, {0, 0, 3, 0, 0}, {90, 69, 4, 2, 0}};
    std::vector<uint32_t> ops = {op(20, 0), op(5, 1), op(4, 2), op(7, 3), op(10, 0), op(1, 1)};
    size_t n = 3, n_ops = 6;
    uint32_t flags = 0, chunk = 0;
    int run() const {
        const SpanTotals t = checked_spans(fail, spans.data(), n, ops.data(), n_ops, 100, 80, flags, chunk);
        printf("%llu %llu\n", (unsigned long long)t.ops, (unsigned long long)t.columns);
        return 0;
    }
};

}  // namespace

int main(int argc, char** argv) {
    const std::string c = argc > 1 ? argv[1] : "";
    Input p;
    if (c == "ok") return p.run();
    if (c == "no_spans") return p.n = 0, p.run();
    if (c == "chunk_64_and_both_flags") return p.chunk = 64, p.flags = 3, p.run();
    if (c == "chunk_65536") return p.chunk = 65536, p.run();
    if (c == "too_many_spans") return p.n = (1u << 22) + 1, p.run();  // fires before any array is read
    if (c == "too_many_ops") return p.n_ops = (1u << 28) + 1, p.run();
    if (c == "ranges_overlap") return p.spans[0].n_ops = 4, p.run();
    if (c == "ranges_descend") return p.spans[1].op_offset = 5, p.run();
    if (c == "last_range_leaves_the_array") return p.spans[2].n_ops = 3, p.run();
    if (c == "range_wraps") return p.spans[2].op_offset = ~(uint64_t)0, p.run();
    if (c == "code_3") return p.ops[1] = op(5, 3), p.run();
    if (c == "zero_run") return p.ops[5] = op(0, 1), p.run();
    if (c == "overlap_before_code_3") return p.spans[0].n_ops = 4, p.ops[1] = op(5, 3), p.run();
    if (c == "past_the_target") return p.spans[2].ref_start = 91, p.run();
    if (c == "past_the_query") return p.spans[2].query_start = 70, p.run();
    if (c == "past_the_target_by_a_deletion") return p.ops[2] = op(71, 2), p.run();
    if (c == "code_3_before_past_the_target") return p.ops[0] = op(500, 3), p.run();
    if (c == "too_many_columns") {  // 2^31 deleted and 2^31 inserted bases fit a block of 2^32 - 1 bases a side and are 2^32 columns
        const uint32_t R = (1u << 30) - 1;
        p.spans = {{0, 0, 0, 6, 0}};
        p.ops = {op(R, 2), op(R, 2), op(2, 2), op(R, 1), op(R, 1), op(2, 1)};
        const SpanTotals t = checked_spans(fail, p.spans.data(), 1, p.ops.data(), 6, 0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0);
        printf("%llu\n", (unsigned long long)t.columns);
        return 0;
    }
    if (c == "most_columns") {  // one fewer
        const uint32_t R = (1u << 30) - 1;
        p.spans = {{0, 0, 0, 6, 0}};
        p.ops = {op(R, 2), op(R, 2), op(2, 2), op(R, 1), op(R, 1), op(1, 1)};
        const SpanTotals t = checked_spans(fail, p.spans.data(), 1, p.ops.data(), 6, 0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0);
        printf("%llu\n", (unsigned long long)t.columns);
        return 0;
    }
    if (c == "chunk_32") return p.chunk = 32, p.run();
    if (c == "chunk_96") return p.chunk = 96, p.run();
    if (c == "chunk_131072") return p.chunk = 131072, p.run();
    if (c == "unknown_flag") return p.flags = 4, p.run();
    if (c == "bad_chunk_before_unknown_flag") return p.chunk = 100, p.flags = 4, p.run();
    fprintf(stderr, "diff_checks_main: no case '%s'\n", c.c_str());
    return 2;
}
