// diff.hip -- the kernels of sa_diff_alignments (contract: include/segalign_amd.h).
//
// Prepare: every op entry learns its span (a binary search over the spans' ascending op ranges) and what it adds to four sums: target
// bases, query bases, columns and work items.  The exclusive sums, rebased at a span's first entry, give an entry its first target base,
// query base and column; the sum of work items lays the items out in span and column order.  A work item is up to `chunk` columns of
// one M entry, or one gap entry whole.
//
// Count and emit are one template, one wavefront per item, 64 consecutive columns per step, lane l on column base + l.  The kinds of a
// step's columns are two ballot masks (SUB, OTHER); a run starts where its bit is set and the bit before is not, and ends where the bit
// behind is not.  The bit before a step's first column and behind its last come from the step before and from one look at the next
// column: inside the item the neighbouring M column, at the item's edge the neighbouring column of the span, whatever entry holds it,
// and none at the span's edge.  The neighbour is always a column of the same span, so its bases are bases the span consumes: no load
// leaves the block.  Every event has one start and one end, events are ordered and disjoint, so the k-th start and the k-th end of
// the call are the same event's: the prefix sums of the items' start counts and of their end counts place both with no sort and no
// atomics, and an event may run through any number of items that hold neither.  The pair counts stay in registers (lane l counts
// pair l, found with one ballot per distinct pair of a step) and reach memory with one integer atomicAdd per lane and item.
#include "diff.h"

namespace sa {

namespace {

enum : uint32_t { CLS_MATCH = 0, CLS_TS = 1, CLS_TV = 2, CLS_OTHER = 3 };
constexpr uint32_t KIND_NONE = 4;  // a MATCH column, or no column at all

__device__ __forceinline__ uint32_t classify(uint32_t x, uint32_t y) {
    if ((x | y) >= 4) return CLS_OTHER;
    if (x == y) return CLS_MATCH;
    return (x ^ y) == 2 ? CLS_TS : CLS_TV;
}
__device__ __forceinline__ uint32_t kind_of_class(uint32_t c) { return c == CLS_MATCH ? KIND_NONE : c == CLS_OTHER ? SA_DIFF_OTHER : SA_DIFF_SUB; }
__device__ __forceinline__ uint32_t kind_of_gap(uint32_t op) { return op == SA_GAPPED_OP_I ? SA_DIFF_INS : SA_DIFF_DEL; }
__device__ __forceinline__ uint32_t pair_kind(const DiffArgs& a, uint32_t r, uint32_t q) {
    return kind_of_class(classify(a.ref[r] & 7, a.query[q] & 7));
}

struct Item {
    uint32_t span, op, n;    // the entry's op; the item's columns
    uint32_t r, q, col;      // the next base of each sequence and the column index at the item's first column
    uint32_t before, after;  // the kinds of the span's columns before the first and behind the last (KIND_NONE for none)
};

// Item w, which lies in op entry e.  Everything here is the same in all lanes.
__device__ __forceinline__ Item load_item(const DiffArgs& a, uint32_t e, uint32_t w) {
    Item it;
    const uint32_t word = a.ops[e], run = word >> 2;
    it.op = word & 3u;
    it.span = a.span_of[e];
    const sa_diff_span sp = a.spans[it.span];
    const uint32_t e0 = (uint32_t)sp.op_offset, e1 = e0 + sp.n_ops;
    const uint32_t re = sp.ref_start + (uint32_t)(a.tsum[e] - a.tsum[e0]);
    const uint32_t qe = sp.query_start + (uint32_t)(a.qsum[e] - a.qsum[e0]);
    const uint32_t ce = (uint32_t)(a.csum[e] - a.csum[e0]);
    uint32_t lo = 0, hi = run;
    if (it.op == SA_GAPPED_OP_M) {
        lo = (w - (uint32_t)a.isum[e]) << a.chunk_shift;
        hi = min(run, lo + (1u << a.chunk_shift));
    }
    it.n = hi - lo;
    it.r = re + (it.op == SA_GAPPED_OP_M ? lo : 0u);
    it.q = qe + (it.op == SA_GAPPED_OP_M ? lo : 0u);
    it.col = ce + lo;
    if (lo > 0) it.before = pair_kind(a, it.r - 1, it.q - 1);
    else if (e == e0) it.before = KIND_NONE;
    else {
        const uint32_t p = a.ops[e - 1] & 3u;  // its last column consumed the bases before (re, qe)
        it.before = p == SA_GAPPED_OP_M ? pair_kind(a, re - 1, qe - 1) : kind_of_gap(p);
    }
    if (hi < run) it.after = pair_kind(a, re + hi, qe + hi);
    else if (e + 1 == e1) it.after = KIND_NONE;
    else {
        const uint32_t nx = a.ops[e + 1] & 3u;  // its first column consumes the bases behind this entry's
        it.after = nx == SA_GAPPED_OP_M ? pair_kind(a, re + (it.op != SA_GAPPED_OP_I ? run : 0u), qe + (it.op != SA_GAPPED_OP_D ? run : 0u))
                                        : kind_of_gap(nx);
    }
    return it;
}

// Every field of an event but len, which its end writes.
__device__ __forceinline__ void write_start(sa_diff_event* ev, uint32_t span, uint32_t r, uint32_t q, uint32_t col, uint32_t kind, uint32_t tc,
                                            uint32_t qc) {
    uint32_t* p = reinterpret_cast<uint32_t*>(ev);
    p[0] = span;
    p[1] = r;
    p[2] = q;
    p[4] = col;
    p[5] = kind | tc << 8 | qc << 16;
}

template <bool EMIT>
__global__ __launch_bounds__(256) void diff_pass_kernel(DiffArgs a, const uint32_t* __restrict__ item_entry, uint32_t n_items, DiffCounts c,
                                                        uint64_t* __restrict__ pairs, const uint64_t* __restrict__ start_off,
                                                        const uint64_t* __restrict__ end_off, sa_diff_event* __restrict__ ev) {
    const uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= n_items) return;
    const uint32_t lane = threadIdx.x & 63;
    const Item it = load_item(a, item_entry[w], w);
    uint64_t so = 0, eo = 0;
    if (EMIT) {
        so = start_off[w];
        eo = end_off[w];
    }
    if (it.op != SA_GAPPED_OP_M) {  // a gap entry: one run of one kind
        const uint32_t kind = kind_of_gap(it.op);
        const bool start = it.before != kind, end = it.after != kind;
        if (lane == 0) {
            if (EMIT) {
                if (start)
                    write_start(ev + so, it.span, it.r, it.q, it.col, kind, kind == SA_DIFF_INS ? SA_DIFF_NO_CODE : a.ref[it.r] & 7,
                                kind == SA_DIFF_DEL ? SA_DIFF_NO_CODE : a.query[it.q] & 7);
                if (end) ev[eo].len = it.col + it.n;
            } else {
                c.starts[w] = start;
                c.ends[w] = end;
                c.match[w] = c.ts[w] = c.tv[w] = 0;
                c.ins_runs[w] = start && kind == SA_DIFF_INS;
                c.del_runs[w] = start && kind == SA_DIFF_DEL;
            }
        }
        return;
    }
    uint32_t n_start = 0, n_end = 0, n_match = 0, n_ts = 0, n_tv = 0, hist = 0;
    uint64_t prev_sub = it.before == SA_DIFF_SUB, prev_oth = it.before == SA_DIFF_OTHER;
    const uint64_t below = (1ull << lane) - 1;
    for (uint32_t base = 0; base < it.n; base += 64) {
        const uint32_t j = base + lane;
        const bool valid = j < it.n;
        uint32_t x = 0, y = 0, cls = CLS_MATCH;
        if (valid) {
            x = a.ref[it.r + j] & 7;
            y = a.query[it.q + j] & 7;
            cls = classify(x, y);
        }
        const uint64_t sub = __ballot(valid && (cls == CLS_TS || cls == CLS_TV)), oth = __ballot(valid && cls == CLS_OTHER);
        const uint32_t left = it.n - base, cnt = left < 64 ? left : 64;
        const uint32_t ak = left > 64 ? pair_kind(a, it.r + base + 64, it.q + base + 64) : it.after;
        const uint64_t last = 1ull << (cnt - 1);
        uint64_t s_sub = sub, e_sub = sub;
        if (!a.per_base) {
            s_sub = sub & ~(sub << 1 | prev_sub);
            e_sub = sub & ~(sub >> 1 | (ak == SA_DIFF_SUB ? last : 0));
        }
        const uint64_t s_oth = oth & ~(oth << 1 | prev_oth), e_oth = oth & ~(oth >> 1 | (ak == SA_DIFF_OTHER ? last : 0));
        const uint64_t starts = s_sub | s_oth, ends = e_sub | e_oth;
        if (EMIT) {
            if (starts >> lane & 1)
                write_start(ev + so + n_start + __popcll(starts & below), it.span, it.r + j, it.q + j, it.col + j,
                            (s_sub >> lane & 1) ? SA_DIFF_SUB : SA_DIFF_OTHER, x, y);
            if (ends >> lane & 1) ev[eo + n_end + __popcll(ends & below)].len = it.col + j + 1;
        } else {
            n_match += __popcll(__ballot(valid && cls == CLS_MATCH));
            n_ts += __popcll(__ballot(valid && cls == CLS_TS));
            n_tv += __popcll(__ballot(valid && cls == CLS_TV));
            const uint32_t bin = x * 8 + y;
            uint64_t rem = __ballot(valid);
            while (rem) {  // one round per distinct pair of the step
                const uint32_t b = __shfl(bin, __ffsll((unsigned long long)rem) - 1);
                const uint64_t m = __ballot(valid && bin == b);
                if (lane == b) hist += __popcll(m);
                rem &= ~m;
            }
        }
        n_start += __popcll(starts);
        n_end += __popcll(ends);
        prev_sub = sub >> 63;
        prev_oth = oth >> 63;
    }
    if (!EMIT) {
        if (lane == 0) {
            c.starts[w] = n_start;
            c.ends[w] = n_end;
            c.match[w] = n_match;
            c.ts[w] = n_ts;
            c.tv[w] = n_tv;
            c.ins_runs[w] = c.del_runs[w] = 0;
        }
        if (hist) atomicAdd(reinterpret_cast<unsigned long long*>(pairs) + lane, (unsigned long long)hist);
    }
}

__global__ __launch_bounds__(256) void diff_span_of_kernel(const sa_diff_span* __restrict__ spans, uint32_t n_spans, uint32_t n_ops,
                                                           uint32_t* __restrict__ span_of) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_ops) return;
    uint32_t lo = 0, hi = n_spans;  // the first span whose ops start behind e
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (spans[mid].op_offset <= e) lo = mid + 1;
        else hi = mid;
    }
    // of the spans that start at or before e only the last can be non-empty there
    span_of[e] = lo > 0 && e < spans[lo - 1].op_offset + spans[lo - 1].n_ops ? lo - 1 : DIFF_NO_SPAN;
}

__global__ __launch_bounds__(256) void diff_values_kernel(const uint32_t* __restrict__ ops, const uint32_t* __restrict__ span_of, uint32_t n_ops,
                                                          int which, uint32_t chunk_shift, uint32_t* __restrict__ val) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_ops) return;
    const uint32_t op = ops[e] & 3u, run = ops[e] >> 2;
    uint32_t v;
    if (which == 0) v = op != SA_GAPPED_OP_I ? run : 0;
    else if (which == 1) v = op != SA_GAPPED_OP_D ? run : 0;
    else if (which == 2) v = run;
    else v = span_of[e] == DIFF_NO_SPAN ? 0 : op == SA_GAPPED_OP_M ? (run + (1u << chunk_shift) - 1) >> chunk_shift : 1;
    val[e] = v;
}

__global__ __launch_bounds__(256) void diff_items_kernel(const uint64_t* __restrict__ isum, uint32_t n_ops, uint32_t n_items,
                                                         uint32_t* __restrict__ item_entry) {
    const uint32_t w = blockIdx.x * 256 + threadIdx.x;
    if (w >= n_items) return;
    uint32_t lo = 0, hi = n_ops + 1;  // the first entry whose items start behind w: isum[n_ops] = n_items > w, so lo <= n_ops
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (isum[mid] <= w) lo = mid + 1;
        else hi = mid;
    }
    item_entry[w] = lo - 1;  // isum[0] = 0 <= w, so lo >= 1; entries without items between are skipped
}

__global__ __launch_bounds__(256) void diff_finish_kernel(sa_diff_event* __restrict__ ev, uint32_t n) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    ev[k].len -= ev[k].column;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(256) void diff_summaries_kernel(DiffArgs a, DiffCounts c, const uint64_t* __restrict__ start_off,
                                                             sa_diff_summary* __restrict__ out) {
    const uint32_t k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= a.n_spans) return;
    const uint32_t lane = threadIdx.x & 63;
    const sa_diff_span sp = a.spans[k];
    const uint32_t e0 = (uint32_t)sp.op_offset, e1 = e0 + sp.n_ops;
    const uint64_t i0 = a.isum[e0], i1 = a.isum[e1];
    uint32_t match = 0, ts = 0, tv = 0, ins = 0, del = 0;  // a span has fewer than 2^32 columns
    for (uint64_t i = i0 + lane; i < i1; i += 64) {
        match += c.match[i];
        ts += c.ts[i];
        tv += c.tv[i];
        ins += c.ins_runs[i];
        del += c.del_runs[i];
    }
    match = wave_sum(match);
    ts = wave_sum(ts);
    tv = wave_sum(tv);
    ins = wave_sum(ins);
    del = wave_sum(del);
    if (lane) return;
    const uint64_t T = a.tsum[e1] - a.tsum[e0], Q = a.qsum[e1] - a.qsum[e0], C = a.csum[e1] - a.csum[e0];
    sa_diff_summary s;
    s.first_event = start_off[i0];
    s.n_events = (uint32_t)(start_off[i1] - start_off[i0]);
    s.columns = (uint32_t)C;
    s.matches = match;
    s.transitions = ts;
    s.transversions = tv;
    s.others = (uint32_t)(T + Q - C) - match - ts - tv;  // the M columns that are none of the three
    s.ins_runs = ins;
    s.ins_bases = (uint32_t)(C - T);
    s.del_runs = del;
    s.del_bases = (uint32_t)(C - Q);
    out[k] = s;
}

}  // namespace

void launch_diff_span_of(const sa_diff_span* spans, uint32_t n_spans, uint32_t n_ops, uint32_t* span_of, hipStream_t s) {
    if (n_ops == 0) return;
    hipLaunchKernelGGL(diff_span_of_kernel, dim3((n_ops + 255) / 256), dim3(256), 0, s, spans, n_spans, n_ops, span_of);
}

void launch_diff_values(const uint32_t* ops, const uint32_t* span_of, uint32_t n_ops, int which, uint32_t chunk_shift, uint32_t* val,
                        hipStream_t s) {
    if (n_ops == 0) return;
    hipLaunchKernelGGL(diff_values_kernel, dim3((n_ops + 255) / 256), dim3(256), 0, s, ops, span_of, n_ops, which, chunk_shift, val);
}

void launch_diff_items(const uint64_t* isum, uint32_t n_ops, uint32_t n_items, uint32_t* item_entry, hipStream_t s) {
    if (n_items == 0) return;
    hipLaunchKernelGGL(diff_items_kernel, dim3((n_items + 255) / 256), dim3(256), 0, s, isum, n_ops, n_items, item_entry);
}

void launch_diff_count(const DiffArgs& a, const uint32_t* item_entry, uint32_t n_items, const DiffCounts& c, uint64_t* pairs, hipStream_t s) {
    if (n_items == 0) return;
    hipLaunchKernelGGL(diff_pass_kernel<false>, dim3((n_items + 3) / 4), dim3(256), 0, s, a, item_entry, n_items, c, pairs, nullptr, nullptr,
                       nullptr);
}

void launch_diff_emit(const DiffArgs& a, const uint32_t* item_entry, uint32_t n_items, const uint64_t* start_off, const uint64_t* end_off,
                      sa_diff_event* events, hipStream_t s) {
    if (n_items == 0) return;
    hipLaunchKernelGGL(diff_pass_kernel<true>, dim3((n_items + 3) / 4), dim3(256), 0, s, a, item_entry, n_items, DiffCounts{}, nullptr,
                       start_off, end_off, events);
}

void launch_diff_finish(sa_diff_event* events, uint32_t n_events, hipStream_t s) {
    if (n_events == 0) return;
    hipLaunchKernelGGL(diff_finish_kernel, dim3((n_events + 255) / 256), dim3(256), 0, s, events, n_events);
}

void launch_diff_summaries(const DiffArgs& a, const DiffCounts& c, const uint64_t* start_off, sa_diff_summary* out, hipStream_t s) {
    if (a.n_spans == 0) return;
    hipLaunchKernelGGL(diff_summaries_kernel, dim3((a.n_spans + 3) / 4), dim3(256), 0, s, a, c, start_off, out);
}

}  // namespace sa
