// gapped.h -- what the kernel units gapped.hip and cover.hip share with the host code that launches them: api_gapped.hip (the three gapped
// entries), api_stitch.hip (the walk and the trace layout), api_hspchain.hip (cover.hip's rocPRIM wrappers) and post_host.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/segalign_amd.h"

namespace sa {

struct GappedSide {  // result of one one-sided extension
    int32_t best;    // best score (>= 0: the anchor cell scores 0)
    int32_t best_i;  // target bases of the best cell
    int32_t best_j;  // query bases of the best cell
    uint32_t cells;  // live cells, the anchor cell included
    uint32_t flags;  // SA_GAPPED_*
    uint32_t pad[3];
};

struct GappedArgs {
    const uint8_t* ref;  // plain codes of the resident target block (dc->ref)
    uint32_t ref_len;
    const uint8_t* query;  // plain codes of the query strand
    uint32_t query_len;
    const int* sub_mat;  // 64 entries on the device
    const sa_segment_pair* hsps;  // the batch's HSPs
    uint32_t num_tasks;  // 2 x HSPs of the batch: task 2h extends HSP h to the left, 2h + 1 to the right
    int gap_open, gap_extend, ydrop, max_extent, max_band;
    GappedSide* out;  // [num_tasks]
};

int gapped_cells_per_lane(int max_band);  // K of the kernel instance a band needs (64 K >= max_band + 1); -1: too wide
void launch_gapped(const GappedArgs& a, hipStream_t s);

// ---- continuation pieces (option gapped_pieces) ----
struct SideTask {  // one one-sided extension from an explicit origin: a piece after a side's first
    uint32_t ar, aq;  // origin (target, query): the previous piece's origin moved by its best cell
    int32_t dir;      // -1 left, +1 right
    uint32_t pad;
};
// Pass 1 of n such sides, one wave each: out[k] = the extension of tasks[k] (a.hsps, a.num_tasks and a.out are not read).
void launch_gapped_sides(const GappedArgs& a, const SideTask* tasks, uint32_t n, GappedSide* out, hipStream_t s);

// ---- trace sweep and path walk (sa_gapped_align) ----
struct TraceTask {  // one side to trace, or one piece of a continued side: its best cell is not its origin
    uint32_t ar, aq;     // origin: the anchor (a_r, a_q), or a later piece's own origin
    int32_t dir;         // -1 left, +1 right
    int32_t dstar;       // best_i + best_j of the side (pass 1): the trace covers antidiagonals 1 .. dstar
    int32_t best_i, best_j;
    uint64_t trace_off;  // byte offset of the side's trace area in the batch's trace buffer (256-aligned)
    uint64_t ops_off;    // first entry of the side's op area (dstar entries) in the batch's op buffer
};

struct TraceOut {  // what the walk of one side found
    uint32_t n_runs;  // run-length ops written, in walk order (best cell -> anchor)
    uint32_t matches, mismatches, gap_opens, gap_bases;
    uint32_t err;     // != 0: the walk left the traced cells (a broken invariant; the host aborts)
    uint32_t pad[2];
};

// Trace area of one side: dstar rows of 64 x ceil(K / 8) dwords (row d - 1 = antidiagonal d; dword w * 64 + l holds the 4-bit codes of
// lane l's cells 8 w .. 8 w + 7), then the window base of antidiagonals 0 .. dstar as int32.  Rounded up to 256 bytes.
size_t gapped_trace_bytes(int max_band, int dstar);
void launch_gapped_trace(const GappedArgs& a, const TraceTask* tasks, uint32_t n, uint8_t* area, hipStream_t s);
void launch_gapped_walk(const GappedArgs& a, const TraceTask* tasks, uint32_t n, const uint8_t* area, uint32_t* ops, TraceOut* out,
                        hipStream_t s);

// ---- cover index of sa_gapped_align_greedy (cover.hip) ----
// A point (t, q) of strand coordinates lies on diagonal diag = t - q + query_len; its key is diag << 32 | t.  An M run of a path is the
// segment [t_begin, t_end) of one diagonal, keyed by its first point.
constexpr uint64_t COVER_NONE = ~0ull;  // key of a segment slot that holds no M run (sorts last)
constexpr uint32_t COVER_RESOLVE_MAX = 1u << 20;  // survivors one resolve launch takes (accepted bits in dynamic LDS, 128 KB at most)

struct CoverSeg {
    uint64_t key;    // diag << 32 | t_begin, or COVER_NONE
    uint32_t t_end;  // one past the segment's last target base
    uint32_t owner;  // the survivor (rank in its priority batch) whose path holds the segment
};

struct CoverEmit {    // one traced side: where its segments go
    uint32_t seg_off;  // first of its n_runs segment slots
    uint32_t owner;
};

// One wave per traced side of a trace batch: the side's runs (d_ops, walk order) become n_runs segment slots, M runs keyed, the rest
// COVER_NONE.  Runs before the walk's buffers are reused by the next trace batch.
void launch_cover_emit(const TraceTask* tasks, const TraceOut* out, const uint32_t* ops, const CoverEmit* emit, uint32_t n,
                       uint32_t query_len, CoverSeg* segs, hipStream_t s);
// covered[k] = 1 when point key keys[k] lies on a segment of the index (key[], run[]: sorted keys and the running maximum of t_end
// within each diagonal, packed diag << 32 | max).
void launch_cover_query(const uint64_t* key, const uint64_t* run, uint32_t n_index, const uint64_t* keys, uint32_t n, uint8_t* covered,
                        hipStream_t s);
// Edges (owner a -> survivor h) of one resolve pass over the survivor ranks [lo, hi): every segment of a survivor a >= lo with
// eligible[a] != 0 and every survivor anchor h on it with a < h < hi.  akey / arank: the survivors' anchor keys sorted, with their ranks.
// Indices are local to the pass (h - lo, a - lo).  count != 0: deg[h - lo] += 1; otherwise src[cursor[h - lo]++] = a - lo.
void launch_cover_edges(const CoverSeg* segs, uint32_t n_segs, const uint64_t* akey, const uint32_t* arank, uint32_t n_anchors,
                        const uint8_t* eligible, uint32_t lo, uint32_t hi, uint32_t* deg, uint64_t* cursor, uint32_t* src, int count,
                        hipStream_t s);
// One wave sweeps the n survivors of a pass in rank order: state[h] = 1 accepted (eligible, no in-edge from an accepted survivor), 2
// covered (an in-edge from an accepted survivor), 0 below the threshold.  row: CSR offsets [n + 1] of the in-edges (local indices).
void launch_cover_resolve(const uint8_t* eligible, const uint64_t* row, const uint32_t* src, uint32_t n, uint8_t* state, hipStream_t s);
// The segments of accepted owners (state 1) with ranks in [lo, hi) appended to key[] / dt[] (dt = diag << 32 | t_end) at atomic
// positions; *count: how many.
void launch_cover_select(const CoverSeg* segs, uint32_t n_segs, const uint8_t* state, uint32_t lo, uint32_t hi, uint64_t* key, uint64_t* dt,
                         uint32_t* count, hipStream_t s);
// Merges (ka, va)[na] and (kb, vb)[nb], both sorted by key, into (ko, vo)[na + nb]; equal keys keep a's entries first.
void launch_cover_merge(const uint64_t* ka, const uint64_t* va, uint32_t na, const uint64_t* kb, const uint64_t* vb, uint32_t nb,
                        uint64_t* ko, uint64_t* vo, hipStream_t s);
// rocPRIM steps.  temp == nullptr: *bytes = temp storage needed.
void cover_sort_pairs(void* temp, size_t* bytes, const uint64_t* kin, uint64_t* kout, const uint64_t* vin, uint64_t* vout, uint32_t n,
                      hipStream_t s);
void cover_sort_anchors(void* temp, size_t* bytes, const uint64_t* kin, uint64_t* kout, const uint32_t* vin, uint32_t* vout, uint32_t n,
                        hipStream_t s);
void cover_scan_offsets(void* temp, size_t* bytes, const uint32_t* deg, uint64_t* row, uint32_t n, hipStream_t s);  // row[n + 1], 64-bit
void cover_scan_runmax(void* temp, size_t* bytes, const uint64_t* dt, uint64_t* run, uint32_t n, hipStream_t s);

}  // namespace sa
