/*
 * gapped_trace_check.c -- serial restatement of sa_gapped_align's paths (include/segalign_amd.h).
 *
 * Plain C, one cell at a time, no shortcuts.  It runs the extension of tests/cpp/gapped_check.c once more, but keeps H, E and F of
 * every antidiagonal up to the side's end, and then walks back from the best cell to the anchor comparing VALUES under the tie rules
 * of the contract (the engine compares stored bits).  The tests hold its results against gapped_check.c's records, an unpruned
 * full-matrix Gotoh traceback, hand-worked cases and every path the engine returns.
 *
 * GT_VARIANT (compile-time, default 0 = the contract) builds a deliberately WRONG checker, used only to show that an input's result
 * hangs on a tie rule (tests/test_gapped_regimes.py): 1 = the source of H is taken F before E before M; 2 = of the cells of one
 * antidiagonal that reach a new maximum the last one (largest i) is the best cell, not the first.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define NEG (-(1 << 30)) /* minus infinity: every value is clamped at it, finite values stay above NEG / 2 */
#define SEP 7            /* E_NT, the record separator; positions outside the block read as it too */
#define FLAG_EXTENT 1u
#define FLAG_BAND 2u
#define OP_M 0u
#define OP_I 1u
#define OP_D 2u
#ifndef GT_VARIANT
#define GT_VARIANT 0
#endif

typedef struct {
    int32_t best, best_i, best_j;
    uint32_t cells, flags;
} gt_side_result;

typedef struct {
    uint32_t n_ops;                   /* runs written, in walk order (best cell -> anchor) */
    uint32_t matches, mismatches;     /* M pairs with equal codes < 4 / all other M pairs */
    uint32_t gap_opens, gap_bases;    /* I and D runs, bases in them */
    int32_t score;                    /* the side re-scored from its ops: must equal best */
    int32_t err;                      /* != 0: the walk met a cell that is not live (a broken invariant) */
} gt_walk;

typedef struct {
    int64_t lo, hi; /* candidate range (lo > hi: none) */
    int32_t *H, *E, *F;
} gt_diag;

static int max2(int a, int b) { return a > b ? a : b; }
static int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }
static int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }
static int code_at(const uint8_t* s, int64_t len, int64_t p) { return (p < 0 || p >= len) ? SEP : (s[p] & 7); }

/* value of antidiagonal d, cell i: minus infinity outside the stored range */
static int32_t val(const gt_diag* D, int64_t nd, int64_t d, int64_t i, int which) {
    if (d < 0 || d >= nd || i < D[d].lo || i > D[d].hi) return NEG;
    const int32_t* a = which == 0 ? D[d].H : which == 1 ? D[d].E : D[d].F;
    return a[i - D[d].lo];
}

/* One side: the extension result (equal to gapped_check.c's gc_side) and its path.  ops: room for best_i + best_j runs. */
void gt_side(const uint8_t* t, int64_t tlen, const uint8_t* q, int64_t qlen, const int32_t* sub, int64_t ar, int64_t aq, int dir,
             int gap_open, int gap_extend, int ydrop, int max_extent, int max_band, gt_side_result* res, uint32_t* ops, gt_walk* wk) {
    int64_t cap = 1024, nd = 1;
    gt_diag* D = (gt_diag*)malloc(cap * sizeof(gt_diag));
    int64_t llo[2] = {0, 1}, lhi[2] = {0, 0}; /* live ranges of d - 1 ([0]) and d - 2 ([1]) */
    D[0].lo = D[0].hi = 0;
    D[0].H = (int32_t*)malloc(sizeof(int32_t)); D[0].E = (int32_t*)malloc(sizeof(int32_t)); D[0].F = (int32_t*)malloc(sizeof(int32_t));
    D[0].H[0] = 0; D[0].E[0] = NEG; D[0].F[0] = NEG;
    int32_t best = 0, best_i = 0, best_j = 0;
    uint32_t cells = 1, flags = 0;
#define X_AT(i) ((i) >= 1 ? code_at(t, tlen, dir > 0 ? ar + (i) - 1 : ar - (i)) : 0)
#define Y_AT(j) ((j) >= 1 ? code_at(q, qlen, dir > 0 ? aq + (j) - 1 : aq - (j)) : 0)
    for (int64_t d = 1;; d++) {
        const int e1 = llo[0] > lhi[0], e2 = d < 2 || llo[1] > lhi[1];
        if (e1 && e2) break;
        int64_t lo = INT64_MAX, hi = INT64_MIN;
        if (!e1) { lo = min64(lo, llo[0]); hi = max64(hi, lhi[0] + 1); }
        if (!e2) { lo = min64(lo, llo[1] + 1); hi = max64(hi, lhi[1] + 1); }
        lo = max64(lo, max64(0, d - max_extent));
        hi = min64(hi, min64(d, max_extent));
        if (hi - lo + 1 > (int64_t)max_band + 1) { flags |= FLAG_BAND; break; }
        if (nd == cap) { cap *= 2; D = (gt_diag*)realloc(D, cap * sizeof(gt_diag)); }
        gt_diag* c = &D[d];
        const int64_t w = hi >= lo ? hi - lo + 1 : 0;
        c->lo = lo; c->hi = hi;
        c->H = (int32_t*)malloc((w + 1) * sizeof(int32_t));
        c->E = (int32_t*)malloc((w + 1) * sizeof(int32_t));
        c->F = (int32_t*)malloc((w + 1) * sizeof(int32_t));
        nd = d + 1;
        const int32_t floor_ = best - ydrop;
        int64_t nlo = INT64_MAX, nhi = INT64_MIN, dbest_i = -1;
        int32_t dbest = NEG;
        uint32_t dcells = 0, dflags = 0;
        for (int64_t i = lo; i <= hi; i++) {
            const int64_t j = d - i;
            const int x = X_AT(i), y = Y_AT(j);
            int32_t h = NEG, e = NEG, f = NEG;
            if (!((i >= 1 && x == SEP) || (j >= 1 && y == SEP))) {
                e = max2(max2(val(D, nd, d - 1, i, 1), val(D, nd, d - 1, i, 0) - gap_open) - gap_extend, NEG);
                f = max2(max2(val(D, nd, d - 1, i - 1, 2), val(D, nd, d - 1, i - 1, 0) - gap_open) - gap_extend, NEG);
                int32_t m = NEG;
                if (i >= 1 && j >= 1 && d >= 2) m = max2(val(D, nd, d - 2, i - 1, 0) + sub[x * 8 + y], NEG);
                h = max2(m, max2(e, f));
            }
            if (h > NEG / 2 && h >= floor_) {
                if (i < nlo) nlo = i;
                nhi = i;
                dcells++;
#if GT_VARIANT == 2
                if (h >= dbest) { dbest = h; dbest_i = i; }
#else
                if (h > dbest) { dbest = h; dbest_i = i; }
#endif
                if (i == max_extent || j == max_extent) dflags |= FLAG_EXTENT;
            } else {
                h = e = f = NEG;
            }
            c->H[i - lo] = h; c->E[i - lo] = e; c->F[i - lo] = f;
        }
        if (dcells && nhi - nlo + 1 > max_band) { flags |= FLAG_BAND; break; }
        llo[1] = llo[0]; lhi[1] = lhi[0];
        llo[0] = dcells ? nlo : 1;
        lhi[0] = dcells ? nhi : 0;
        cells += dcells;
        flags |= dflags;
        if (dcells && dbest > best) { best = dbest; best_i = (int32_t)dbest_i; best_j = (int32_t)(d - dbest_i); }
    }
    res->best = best; res->best_i = best_i; res->best_j = best_j; res->cells = cells; res->flags = flags;

    /* the walk: state 0 H, 1 E, 2 F */
    memset(wk, 0, sizeof(*wk));
    int64_t i = best_i, j = best_j;
    int st = 0, cur = -1;
    uint32_t len = 0;
    int32_t score = 0;
#define EMIT(op)                                                                  \
    do {                                                                          \
        if ((int)(op) == cur) { len++; break; }                                   \
        if (len) {                                                                \
            ops[wk->n_ops++] = len << 2 | (uint32_t)cur;                          \
            if (cur != (int)OP_M) { wk->gap_opens++; wk->gap_bases += len; score -= gap_open + (int32_t)len * gap_extend; } \
        }                                                                         \
        cur = (int)(op);                                                          \
        len = 1;                                                                  \
    } while (0)
    while (i + j > 0) {
        const int64_t d = i + j;
        if (i < 0 || j < 0) { wk->err = 1; break; }
        if (st == 0) {
            const int32_t h = val(D, nd, d, i, 0);
            if (h <= NEG / 2) { wk->err = 2; break; }
            int32_t m = NEG;
            const int x = X_AT(i), y = Y_AT(j);
            if (i >= 1 && j >= 1) m = max2(val(D, nd, d - 2, i - 1, 0) + sub[x * 8 + y], NEG);
#if GT_VARIANT == 1
            if (h == val(D, nd, d, i, 2)) {
                st = 2;
            } else if (h == val(D, nd, d, i, 1)) {
                st = 1;
            } else
#endif
            if (i >= 1 && j >= 1 && h == m) {
                EMIT(OP_M);
                score += sub[x * 8 + y];
                if (x == y && x < 4) wk->matches++;
                else wk->mismatches++;
                i--; j--;
            } else if (h == val(D, nd, d, i, 1)) {
                st = 1;
            } else {
                st = 2;
            }
        } else if (st == 1) {
            if (val(D, nd, d, i, 1) <= NEG / 2) { wk->err = 3; break; }
            EMIT(OP_I);
            st = val(D, nd, d - 1, i, 1) > val(D, nd, d - 1, i, 0) - gap_open ? 1 : 0;
            j--;
        } else {
            if (val(D, nd, d, i, 2) <= NEG / 2) { wk->err = 4; break; }
            EMIT(OP_D);
            st = val(D, nd, d - 1, i - 1, 2) > val(D, nd, d - 1, i - 1, 0) - gap_open ? 2 : 0;
            i--;
        }
    }
    if (!wk->err && (i != 0 || j != 0 || st != 0)) wk->err = 5;
    EMIT(-1); /* flush the last run */
    wk->score = score;
#undef EMIT
#undef X_AT
#undef Y_AT
    for (int64_t k = 0; k < nd; k++) { free(D[k].H); free(D[k].E); free(D[k].F); }
    free(D);
}
