/*
 * diff_check_main.c -- a stand-alone driver of diff_check.c, built with the sanitizers by tests/test_diff_model.py and never loaded
 * into Python.  Every array is allocated at its exact size, so that a read past a sequence, the spans or the ops is reported.
 *   diff_check_main IN OUT
 * IN:  uint32 ref_len, query_len, n_spans, n_ops, flags, cap; the target codes; the query codes; the spans (24 bytes each); the ops.
 * OUT: uint64 n_events; min(n_events, cap) events (24 bytes each); n_spans summaries (48 bytes each); 64 uint64 pair counts.
 *   cc -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/cpp/diff_check.c tests/cpp/diff_check_main.c -o diff_check_san
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

typedef struct {
    uint32_t ref_start, query_start;
    uint64_t op_offset;
    uint32_t n_ops, pad;
} dc_span;
typedef struct {
    uint32_t span, ref_pos, query_pos, len, column;
    uint8_t kind, tcode, qcode, pad;
} dc_event;
typedef struct {
    uint64_t first_event;
    uint32_t n_events, columns, matches, transitions, transversions, others, ins_runs, ins_bases, del_runs, del_bases;
} dc_summary;
uint64_t dc_diff(const uint8_t* ref, const uint8_t* qry, const dc_span* spans, uint32_t n, const uint32_t* ops, uint32_t flags, dc_event* ev,
                 uint64_t cap, dc_summary* sums, uint64_t* pairs);

static void* take(FILE* f, size_t bytes) {
    void* p = malloc(bytes ? bytes : 1);
    if (!p || fread(p, 1, bytes, f) != bytes) {
        fprintf(stderr, "diff_check_main: short input\n");
        exit(2);
    }
    return p;
}

int main(int argc, char** argv) {
    if (argc != 3 || sizeof(dc_span) != 24 || sizeof(dc_event) != 24 || sizeof(dc_summary) != 48) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    uint32_t* h = (uint32_t*)take(in, 6 * sizeof(uint32_t));
    const uint32_t ref_len = h[0], query_len = h[1], n = h[2], n_ops = h[3], flags = h[4], cap = h[5];
    uint8_t* ref = (uint8_t*)take(in, ref_len);
    uint8_t* qry = (uint8_t*)take(in, query_len);
    dc_span* spans = (dc_span*)take(in, (size_t)n * sizeof(dc_span));
    uint32_t* ops = (uint32_t*)take(in, (size_t)n_ops * sizeof(uint32_t));
    fclose(in);
    dc_event* ev = (dc_event*)malloc(cap ? (size_t)cap * sizeof(dc_event) : 1);
    dc_summary* sums = (dc_summary*)malloc(n ? (size_t)n * sizeof(dc_summary) : 1);
    uint64_t pairs[64];
    if (!ev || !sums) return 2;
    const uint64_t n_ev = dc_diff(ref, qry, spans, n, ops, flags, ev, cap, sums, pairs);
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    const size_t kept = (size_t)(n_ev < cap ? n_ev : cap);
    int ok = fwrite(&n_ev, sizeof(n_ev), 1, out) == 1;
    ok = ok && fwrite(ev, sizeof(dc_event), kept, out) == kept;
    ok = ok && fwrite(sums, sizeof(dc_summary), n, out) == n;
    ok = ok && fwrite(pairs, sizeof(uint64_t), 64, out) == 64;
    ok = fclose(out) == 0 && ok;
    free(h);
    free(ref);
    free(qry);
    free(spans);
    free(ops);
    free(ev);
    free(sums);
    printf("diff_check: %llu events\n", (unsigned long long)n_ev);
    return ok ? 0 : 2;
}
