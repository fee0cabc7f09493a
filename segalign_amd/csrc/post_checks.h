// post_checks.h -- the input rules that the post-processing entries share, written once: chains in CSR form, their
// member HSPs, block pairs on two axes, the head of the fill rules and the spans of sa_diff_alignments, each with the message its entry
// prints (tests/test_post_checks.py and tests/test_diff_model.py pin every one of them).  Host code only and free of HIP:
// include/segalign_amd.h and the standard library, so a plain g++ compiles it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../include/segalign_amd.h"

namespace sa {

// The limits the messages below name; a unit with constants of its own for them static_asserts that they are these.
constexpr uint32_t POST_MAX_CHAINS = 1u << 22;   // chains of one call
constexpr uint32_t POST_MAX_MEMBERS = 1u << 22;  // member entries of a chain list
constexpr uint32_t POST_MAX_BLOCKS = 1u << 26;   // blocks of a block list
constexpr uint32_t POST_TOP = 1u << 31;          // every block coordinate is below it

// An entry's error for input that breaks a rule: "Error: <who>: <message>" and exit 1.
struct Fail {
    const char* who;
    [[noreturn]] void operator()(const char* fmt, long long a = 0, long long b = 0) const {
        fprintf(stderr, "Error: %s: ", who);
        fprintf(stderr, fmt, a, b);
        fprintf(stderr, "\n");
        exit(1);
    }
};

// The checks of a chain list first[0 .. n_chains]; returns the number of member entries, 0 for no chain.
inline size_t checked_first(const Fail& fail, const uint32_t* first, size_t n_chains) {
    if (n_chains > POST_MAX_CHAINS) fail("%lld chains: at most 1 << 22", (long long)n_chains);
    if (n_chains == 0) return 0;
    if (first[0] != 0) fail("first[0] = %lld, not 0", first[0]);
    for (size_t c = 0; c < n_chains; c++)
        if (first[c + 1] < first[c]) fail("first[] decreases at chain %lld", (long long)c);
    const size_t M = first[n_chains];
    if (M > POST_MAX_MEMBERS) fail("%lld members: at most 1 << 22", (long long)M);
    return M;
}

// The HSP of member entry k, checked to be one of the input that lies inside the block of ref_len by query_len bases.
inline const sa_segment_pair& checked_member(const Fail& fail, const sa_segment_pair* hsps, size_t n_hsps, const uint32_t* members, size_t k,
                                             uint32_t ref_len, uint32_t query_len) {
    if (members[k] >= n_hsps) fail("member %lld names HSP %lld, which is not in the input", (long long)k, members[k]);
    const sa_segment_pair& h = hsps[members[k]];
    if ((uint64_t)h.ref_start + h.len + 1 > ref_len || (uint64_t)h.query_start + h.len + 1 > query_len)
        fail("member %lld (HSP %lld) does not lie inside the block", (long long)k, members[k]);
    return h;
}

// The CSR and block rules of sa_net_chains and the rules of the other axis, in one pass over n chains: blocks [bs, be) ascending on the
// axis, [obs, obe) of the same lengths on the other axis, ascending for ostrand 0 (or no ostrand) and descending for 1.  Returns the
// number of blocks.
inline uint32_t checked_block_pairs(const Fail& fail, const uint32_t* first, const uint32_t* bs, const uint32_t* be, const uint32_t* obs,
                                    const uint32_t* obe, const uint8_t* ostrand, size_t n) {
    if (n > POST_MAX_CHAINS) fail("%lld chains: at most 1 << 22", (long long)n);
    if (n == 0) return 0;
    if (first[0] != 0) fail("first[0] = %lld, not 0", first[0]);
    for (size_t c = 0; c < n; c++) {
        if (first[c + 1] < first[c]) fail("first[] decreases at chain %lld", (long long)c);
        if (first[c + 1] > POST_MAX_BLOCKS) fail("%lld blocks: at most 1 << 26", first[c + 1]);
        const uint32_t strand = ostrand ? ostrand[c] : 0;
        if (strand > 1) fail("ostrand[%lld] = %lld: 0 or 1", (long long)c, strand);
        for (size_t k = first[c]; k < first[c + 1]; k++) {
            if (bs[k] >= be[k]) fail("chain %lld, block %lld: start >= end", (long long)c, (long long)k);
            if (be[k] >= POST_TOP) fail("chain %lld, block %lld ends at or past 2^31", (long long)c, (long long)k);
            if (k > first[c] && be[k - 1] > bs[k]) fail("chain %lld: its blocks overlap or descend at block %lld", (long long)c, (long long)k);
            if (obs[k] >= obe[k]) fail("chain %lld, block %lld: start >= end on the other axis", (long long)c, (long long)k);
            if (obe[k] >= POST_TOP) fail("chain %lld, block %lld ends at or past 2^31 on the other axis", (long long)c, (long long)k);
            if (obe[k] - obs[k] != be[k] - bs[k]) fail("chain %lld, block %lld: the lengths on the two axes differ", (long long)c, (long long)k);
            if (k > first[c] && (strand ? obe[k] > obs[k - 1] : obe[k - 1] > obs[k]))
                fail(strand ? "chain %lld (ostrand 1): its other blocks overlap or ascend at block %lld"
                            : "chain %lld (ostrand 0): its other blocks overlap or descend at block %lld",
                     (long long)c, (long long)k);
        }
    }
    return first[n];
}

// The rules every fill of a net keeps whatever its chains are made of: fill k is not empty, names a chain of the input and takes its
// blocks first_block .. first_block + n_blocks - 1 from that chain's entries of first[].
inline void checked_fill_in_chain(const Fail& fail, const sa_net_fill& f, size_t k, const uint32_t* first, size_t n_chains) {
    if (f.start >= f.end) fail("fill %lld: start >= end", (long long)k);
    if (f.chain >= n_chains) fail("fill %lld names chain %lld, which is not in the input", (long long)k, f.chain);
    if (f.n_blocks < 1 || f.first_block < first[f.chain] || (uint64_t)f.first_block + f.n_blocks > first[f.chain + 1])
        fail("fill %lld: its blocks leave chain %lld", (long long)k, f.chain);
}

// The limits of sa_diff_alignments.
constexpr uint32_t DIFF_MAX_SPANS = 1u << 22;
constexpr uint32_t DIFF_MAX_OPS = 1u << 28;
constexpr uint32_t DIFF_DEFAULT_CHUNK = 4096;

struct SpanTotals {
    uint64_t ops, columns;  // over all spans
};

// The rules of sa_diff_alignments in the contract's order: the counts; the op ranges, ascending and disjoint inside the array; then per
// span its op codes and runs, its place inside the block of ref_len by query_len bases and its columns; chunk (0 = the default); flags.
inline SpanTotals checked_spans(const Fail& fail, const sa_diff_span* spans, size_t n, const uint32_t* ops, size_t n_ops_total, uint32_t ref_len,
                                uint32_t query_len, uint32_t flags, uint32_t chunk) {
    if (n > DIFF_MAX_SPANS) fail("%lld spans: at most 1 << 22", (long long)n);
    if (n_ops_total > DIFF_MAX_OPS) fail("%lld ops: at most 1 << 28", (long long)n_ops_total);
    for (size_t k = 0; k < n; k++) {
        const uint64_t end = spans[k].op_offset + spans[k].n_ops;
        if (end < spans[k].op_offset || end > (k + 1 < n ? spans[k + 1].op_offset : (uint64_t)n_ops_total)) {
            if (k + 1 < n) fail("span %lld: its ops overlap those of span %lld or lie behind them", (long long)k, (long long)(k + 1));
            fail("span %lld: its ops leave the array of %lld", (long long)k, (long long)n_ops_total);
        }
    }
    SpanTotals t = {0, 0};
    for (size_t k = 0; k < n; k++) {
        const sa_diff_span& s = spans[k];
        uint64_t r = s.ref_start, q = s.query_start, cols = 0;
        for (uint64_t e = s.op_offset; e < s.op_offset + s.n_ops; e++) {
            const uint32_t op = ops[e] & 3u, run = ops[e] >> 2;
            if (op == 3u) fail("span %lld: op %lld has code 3", (long long)k, (long long)(e - s.op_offset));
            if (run == 0) fail("span %lld: op %lld has a zero run", (long long)k, (long long)(e - s.op_offset));
            if (op != SA_GAPPED_OP_I) r += run;
            if (op != SA_GAPPED_OP_D) q += run;
            cols += run;
        }
        if (r > ref_len || q > query_len) fail("span %lld does not lie inside the block", (long long)k);
        if (cols >= ((uint64_t)1 << 32)) fail("span %lld has %lld columns: fewer than 2^32", (long long)k, (long long)cols);
        t.ops += s.n_ops;
        t.columns += cols;
    }
    if (chunk != 0 && (chunk < 64 || chunk > 65536 || (chunk & (chunk - 1)))) fail("chunk = %lld: 0 or a power of two in 64 .. 65536", chunk);
    if (flags & ~(SA_DIFF_PER_BASE | SA_DIFF_NO_EVENTS)) fail("flags = %lld: unknown bits", flags);
    return t;
}

}  // namespace sa
