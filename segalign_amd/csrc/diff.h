// diff.h -- what diff.hip (the kernels) and api_diff.hip (sa_diff_alignments) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/segalign_amd.h"

namespace sa {

constexpr uint32_t DIFF_NO_SPAN = 0xFFFFFFFFu;  // span_of[] of an op entry that no span names

struct DiffArgs {
    const uint8_t* ref;  // plain codes of the resident target block
    uint32_t ref_len;
    const uint8_t* query;  // plain codes of the query strand
    uint32_t query_len;
    const int* sub_mat;  // resident_block sets it; the kernels do not read it
    const sa_diff_span* spans;
    uint32_t n_spans;
    const uint32_t* ops;
    uint32_t n_ops;  // of the whole array
    uint32_t chunk_shift;
    uint32_t per_base;
    // what the prepare step makes, one entry per op and one more: the exclusive sums of target bases, query bases, columns and work
    // items over ops[0, e), and the span that names op e
    const uint64_t *tsum, *qsum, *csum, *isum;
    const uint32_t* span_of;
};

// The counts of one work item, in the arrays of DiffCounts at its index.
struct DiffCounts {
    uint32_t *starts, *ends;       // events that start / end in the item
    uint32_t *match, *ts, *tv;     // its M columns by class (OTHER is the rest)
    uint32_t *ins_runs, *del_runs; // INS / DEL events that start in the item
};

// Prepare, step 1: span_of[e] for every op entry.
void launch_diff_span_of(const sa_diff_span* spans, uint32_t n_spans, uint32_t n_ops, uint32_t* span_of, hipStream_t s);
// Prepare, step 2: val[e] = what op e adds to sum `which` (0 target bases, 1 query bases, 2 columns, 3 work items; an entry outside
// every span makes no item).
void launch_diff_values(const uint32_t* ops, const uint32_t* span_of, uint32_t n_ops, int which, uint32_t chunk_shift, uint32_t* val,
                        hipStream_t s);
// One wavefront per work item w in [0, n_items).  item_entry[w] is the op entry of item w.
void launch_diff_items(const uint64_t* isum, uint32_t n_ops, uint32_t n_items, uint32_t* item_entry, hipStream_t s);
// The count pass: the counts of every item, and pairs[64] += the items' M columns by code pair.
void launch_diff_count(const DiffArgs& a, const uint32_t* item_entry, uint32_t n_items, const DiffCounts& c, uint64_t* pairs, hipStream_t s);
// The emit pass: the k-th start of the call writes every field of events[k] but len, the k-th end writes the column behind the event
// into events[k].len; launch_diff_finish turns that into the length.
void launch_diff_emit(const DiffArgs& a, const uint32_t* item_entry, uint32_t n_items, const uint64_t* start_off, const uint64_t* end_off,
                      sa_diff_event* events, hipStream_t s);
void launch_diff_finish(sa_diff_event* events, uint32_t n_events, hipStream_t s);
// One wavefront per span: its summary from the items' counts, the start offsets and the prepare step's sums.
void launch_diff_summaries(const DiffArgs& a, const DiffCounts& c, const uint64_t* start_off, sa_diff_summary* out, hipStream_t s);

}  // namespace sa
