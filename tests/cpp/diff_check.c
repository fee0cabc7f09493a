/*
 * diff_check.c -- a serial restatement of sa_diff_alignments (include/segalign_amd.h) that walks the op entries as they
 * are, without expanding them into columns: one open event is carried along, a gap entry lengthens it or opens the next in one step,
 * an M entry does so base by base.  Plain C99 with layouts of its own, so that it shares nothing with the engine but the contract.
 */
#include <stdint.h>
#include <string.h>

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

enum { DC_SUB = 0, DC_OTHER = 1, DC_INS = 2, DC_DEL = 3, DC_NONE = 4 };
enum { DC_PER_BASE = 1 };

/* Returns the number of events; the first cap of them are written to ev.  sums: one per span.  pairs: 64 counts, set here. */
uint64_t dc_diff(const uint8_t* ref, const uint8_t* qry, const dc_span* spans, uint32_t n, const uint32_t* ops, uint32_t flags, dc_event* ev,
                 uint64_t cap, dc_summary* sums, uint64_t* pairs) {
    uint64_t n_ev = 0;
    memset(pairs, 0, 64 * sizeof(uint64_t));
    for (uint32_t k = 0; k < n; k++) {
        dc_summary s;
        memset(&s, 0, sizeof(s));
        s.first_event = n_ev;
        uint32_t r = spans[k].ref_start, q = spans[k].query_start, col = 0;
        int open = DC_NONE; /* the kind of the column before */
        for (uint64_t e = spans[k].op_offset; e < spans[k].op_offset + spans[k].n_ops; e++) {
            const uint32_t op = ops[e] & 3u, run = ops[e] >> 2;
            if (op != 0) {
                const int kind = op == 1 ? DC_INS : DC_DEL;
                if (kind == open) {
                    if (n_ev - 1 < cap) ev[n_ev - 1].len += run;
                } else {
                    if (n_ev < cap) {
                        const dc_event x = {k, r, q, run, col, (uint8_t)kind, (uint8_t)(op == 1 ? 8 : ref[r] & 7), (uint8_t)(op == 2 ? 8 : qry[q] & 7), 0};
                        ev[n_ev] = x;
                    }
                    n_ev++;
                    if (op == 1) s.ins_runs++;
                    else s.del_runs++;
                }
                if (op == 1) {
                    s.ins_bases += run;
                    q += run;
                } else {
                    s.del_bases += run;
                    r += run;
                }
                col += run;
                open = kind;
                continue;
            }
            for (uint32_t i = 0; i < run; i++, r++, q++, col++) {
                const uint32_t x = ref[r] & 7, y = qry[q] & 7;
                int kind;
                pairs[x * 8 + y]++;
                if (x >= 4 || y >= 4) {
                    s.others++;
                    kind = DC_OTHER;
                } else if (x == y) {
                    s.matches++;
                    kind = DC_NONE;
                } else {
                    if ((x ^ y) == 2) s.transitions++;
                    else s.transversions++;
                    kind = DC_SUB;
                }
                if (kind != DC_NONE) {
                    if (kind == open && !(kind == DC_SUB && (flags & DC_PER_BASE))) {
                        if (n_ev - 1 < cap) ev[n_ev - 1].len++;
                    } else {
                        if (n_ev < cap) {
                            const dc_event z = {k, r, q, 1, col, (uint8_t)kind, (uint8_t)x, (uint8_t)y, 0};
                            ev[n_ev] = z;
                        }
                        n_ev++;
                    }
                }
                open = kind;
            }
        }
        s.columns = col;
        s.n_events = (uint32_t)(n_ev - s.first_event);
        sums[k] = s;
    }
    return n_ev;
}
