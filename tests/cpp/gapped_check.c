/*
 * gapped_check.c -- serial restatement of the gapped y-drop extension contract (include/segalign_amd.h).
 *
 * Plain C, one cell at a time, no shortcuts: the tests compile it with the system C compiler into a temporary directory and
 * hold sa_gapped_extend's raw records against it field by field (cells and flags included).  It reads the byte codes the
 * engine itself holds (sa_copy_ref_codes / sa_copy_query_codes), so nothing outside the repository is needed.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define NEG (-(1 << 30)) /* minus infinity: every value is clamped at it, finite values stay above NEG / 2 */
#define SEP 7            /* E_NT, the record separator; positions outside the block read as it too */
#define FLAG_EXTENT 1u
#define FLAG_BAND 2u

typedef struct {
    uint32_t ref_start, query_start, len;
    int32_t score;
} gc_hsp;

typedef struct {
    uint32_t ref_start, ref_end, query_start, query_end;
    int32_t score;
    uint32_t hsp_index, flags, cells;
} gc_alignment;

typedef struct {
    int32_t best, best_i, best_j;
    uint32_t cells, flags;
} gc_side_result;

static int max2(int a, int b) { return a > b ? a : b; }
static int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }
static int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }

/* code of sequence position p (separator outside [0, len)) */
static int code_at(const uint8_t* s, int64_t len, int64_t p) { return (p < 0 || p >= len) ? SEP : (s[p] & 7); }

/* One one-sided extension from anchor (ar, aq): dir = +1 right (X[i] = T[ar + i]), -1 left (X[i] = T[ar - 1 - i]).
 * Arrays are indexed by absolute i; range[k] is the candidate range of the antidiagonal stored in slot k, outside of which a
 * read gives minus infinity. */
void gc_side(const uint8_t* t, int64_t tlen, const uint8_t* q, int64_t qlen, const int32_t* sub, int64_t ar, int64_t aq, int dir,
             int gap_open, int gap_extend, int ydrop, int max_extent, int max_band, gc_side_result* res) {
    const int64_t W = (int64_t)max_extent + 2;
    int32_t* H[3];
    int32_t* E[3];
    int32_t* F[3];
    int64_t rlo[3], rhi[3];       /* candidate range of the antidiagonal in each slot */
    int64_t llo[3], lhi[3];       /* live range (llo > lhi: none) */
    for (int k = 0; k < 3; k++) {
        H[k] = (int32_t*)malloc(W * sizeof(int32_t));
        E[k] = (int32_t*)malloc(W * sizeof(int32_t));
        F[k] = (int32_t*)malloc(W * sizeof(int32_t));
        rlo[k] = 1; rhi[k] = 0; llo[k] = 1; lhi[k] = 0;
    }
    /* antidiagonal 0: the anchor cell (0, 0) */
    H[0][0] = 0; E[0][0] = NEG; F[0][0] = NEG;
    rlo[0] = rhi[0] = 0; llo[0] = lhi[0] = 0;
    int32_t best = 0, best_i = 0, best_j = 0;
    uint32_t cells = 1, flags = 0; /* (0, 0) is a live cell */
#define GET(A, k, i) (((i) >= rlo[k] && (i) <= rhi[k]) ? A[k][i] : NEG)
    for (int64_t d = 1;; d++) {
        const int c = (int)(d % 3), p1 = (int)((d - 1) % 3), p2 = (int)((d + 1) % 3); /* (d - 2) % 3 */
        const int e1 = llo[p1] > lhi[p1], e2 = d < 2 || llo[p2] > lhi[p2];
        if (e1 && e2) break; /* two consecutive antidiagonals without a live cell */
        int64_t lo = INT64_MAX, hi = INT64_MIN;
        if (!e1) { lo = min64(lo, llo[p1]); hi = max64(hi, lhi[p1] + 1); }
        if (!e2) { lo = min64(lo, llo[p2] + 1); hi = max64(hi, lhi[p2] + 1); }
        lo = max64(lo, max64(0, d - max_extent));
        hi = min64(hi, min64(d, max_extent));
        if (hi - lo + 1 > (int64_t)max_band + 1) { flags |= FLAG_BAND; break; }
        const int32_t floor_ = best - ydrop; /* B_d - ydrop */
        int64_t nlo = INT64_MAX, nhi = INT64_MIN;
        int32_t dbest = NEG;
        int64_t dbest_i = -1;
        uint32_t dcells = 0, dflags = 0;
        rlo[c] = lo; rhi[c] = hi;
        for (int64_t i = lo; i <= hi; i++) {
            const int64_t j = d - i;
            const int x = i >= 1 ? code_at(t, tlen, dir > 0 ? ar + i - 1 : ar - i) : 0;
            const int y = j >= 1 ? code_at(q, qlen, dir > 0 ? aq + j - 1 : aq - j) : 0;
            int32_t h = NEG, e = NEG, f = NEG;
            if (!((i >= 1 && x == SEP) || (j >= 1 && y == SEP))) {
                e = max2(max2(GET(E, p1, i), GET(H, p1, i) - gap_open) - gap_extend, NEG);          /* from (i, j-1) */
                f = max2(max2(GET(F, p1, i - 1), GET(H, p1, i - 1) - gap_open) - gap_extend, NEG);  /* from (i-1, j) */
                int32_t m = NEG;
                if (i >= 1 && j >= 1 && d >= 2) m = max2(GET(H, p2, i - 1) + sub[x * 8 + y], NEG);  /* from (i-1, j-1) */
                h = max2(m, max2(e, f));
            }
            if (h > NEG / 2 && h >= floor_) { /* live */
                if (i < nlo) nlo = i;
                nhi = i;
                dcells++;
                if (h > dbest) { dbest = h; dbest_i = i; }
                if (i == max_extent || j == max_extent) dflags |= FLAG_EXTENT;
            } else {
                h = e = f = NEG;
            }
            H[c][i] = h; E[c][i] = e; F[c][i] = f;
        }
        if (dcells && nhi - nlo + 1 > max_band) { flags |= FLAG_BAND; break; }
        llo[c] = dcells ? nlo : 1;
        lhi[c] = dcells ? nhi : 0;
        cells += dcells;
        flags |= dflags;
        if (dcells && dbest > best) { best = dbest; best_i = (int32_t)dbest_i; best_j = (int32_t)(d - dbest_i); }
    }
#undef GET
    for (int k = 0; k < 3; k++) { free(H[k]); free(E[k]); free(F[k]); }
    res->best = best; res->best_i = best_i; res->best_j = best_j; res->cells = cells; res->flags = flags;
}

/* Raw records: one per HSP, in input order (the raw mode of sa_gapped_extend). */
void gc_extend(const uint8_t* t, int64_t tlen, const uint8_t* q, int64_t qlen, const int32_t* sub, const gc_hsp* hsps, size_t n,
               int gap_open, int gap_extend, int ydrop, int max_extent, int max_band, gc_alignment* out) {
    for (size_t k = 0; k < n; k++) {
        const int64_t ar = (int64_t)hsps[k].ref_start + hsps[k].len / 2, aq = (int64_t)hsps[k].query_start + hsps[k].len / 2;
        gc_side_result L, R;
        gc_side(t, tlen, q, qlen, sub, ar, aq, -1, gap_open, gap_extend, ydrop, max_extent, max_band, &L);
        gc_side(t, tlen, q, qlen, sub, ar, aq, +1, gap_open, gap_extend, ydrop, max_extent, max_band, &R);
        gc_alignment* o = &out[k];
        o->ref_start = (uint32_t)(ar - L.best_i);
        o->ref_end = (uint32_t)(ar + R.best_i);
        o->query_start = (uint32_t)(aq - L.best_j);
        o->query_end = (uint32_t)(aq + R.best_j);
        o->score = L.best + R.best;
        o->hsp_index = (uint32_t)k;
        o->flags = L.flags | R.flags;
        o->cells = L.cells + R.cells;
    }
}
