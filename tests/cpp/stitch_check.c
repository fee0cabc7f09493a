/*
 * stitch_check.c -- serial restatement of one link of sa_stitch_chains (include/segalign_amd.h).
 *
 * Plain C: a row-major full-matrix global Gotoh over the rectangle, one cell at a time, deliberately NOT in antidiagonal form, then the
 * walk from (dt, dq) back to (0, 0) comparing VALUES under the tie rules of the contract (the engine compares stored bits).  The tests
 * hold it against an enumeration of every alignment of small rectangles, hand-worked cases and every link the engine returns.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define NEG (-(1 << 30)) /* minus infinity: every value is clamped at it, finite values stay above NEG / 2 */
#define SEP 7            /* the record separator */
#define OP_M 0u
#define OP_I 1u
#define OP_D 2u

typedef struct {
    int32_t score;                /* H(dt, dq); NEG when it is not finite */
    int32_t dead;                 /* 1: H(dt, dq) is not finite */
    uint32_t n_ops;               /* runs written, in genome order */
    uint32_t matches, mismatches; /* M pairs with equal codes < 4 / all other M pairs */
    uint32_t gap_opens, gap_bases;
    int32_t rescore;              /* the link re-scored from its ops: must equal score */
    int32_t err;                  /* != 0: the walk met a value that is not finite, or out of memory */
} sc_link;

static int max2(int a, int b) { return a > b ? a : b; }

/* x: the dt target codes of the link, y: its dq query codes.  ops: room for dt + dq runs. */
void sc_align(const uint8_t* x, int dt, const uint8_t* y, int dq, const int32_t* sub, int gap_open, int gap_extend, uint32_t* ops,
              sc_link* out) {
    const size_t W = (size_t)dq + 1, N = ((size_t)dt + 1) * W;
    int32_t* H = (int32_t*)malloc(N * sizeof(int32_t));
    int32_t* E = (int32_t*)malloc(N * sizeof(int32_t));
    int32_t* F = (int32_t*)malloc(N * sizeof(int32_t));
    memset(out, 0, sizeof(*out));
    if (!H || !E || !F) {
        out->err = 9;
        goto done;
    }
    for (int i = 0; i <= dt; i++)
        for (int j = 0; j <= dq; j++) {
            const size_t c = (size_t)i * W + (size_t)j;
            if (i == 0 && j == 0) {
                H[c] = 0;
                E[c] = F[c] = NEG;
                continue;
            }
            const int dead = (i >= 1 && (x[i - 1] & 7) == SEP) || (j >= 1 && (y[j - 1] & 7) == SEP);
            const int e = j >= 1 ? max2(max2(E[c - 1], H[c - 1] - gap_open) - gap_extend, NEG) : NEG;
            const int f = i >= 1 ? max2(max2(F[c - W], H[c - W] - gap_open) - gap_extend, NEG) : NEG;
            const int m = (i >= 1 && j >= 1) ? max2(H[c - W - 1] + sub[(x[i - 1] & 7) * 8 + (y[j - 1] & 7)], NEG) : NEG;
            const int h = max2(m, max2(e, f));
            const int live = !dead && h > NEG / 2;
            H[c] = live ? h : NEG;
            E[c] = live ? e : NEG;
            F[c] = live ? f : NEG;
        }
    out->score = H[N - 1];
    if (H[N - 1] <= NEG / 2) {
        out->score = NEG;
        out->dead = 1;
        goto done;
    }
    {
        /* the walk: (i, j, state) from (dt, dq, H); runs collected backwards, then reversed */
        int i = dt, j = dq, st = 0, cur = -1;
        uint32_t len = 0, n = 0;
        int32_t rs = 0;
        while (i + j > 0) {
            const size_t c = (size_t)i * W + (size_t)j;
            int op;
            if (st == 0) {
                const int m = (i >= 1 && j >= 1) ? max2(H[c - W - 1] + sub[(x[i - 1] & 7) * 8 + (y[j - 1] & 7)], NEG) : NEG;
                if (H[c] <= NEG / 2) { out->err = 1; break; }
                if (H[c] == m) {
                    const int cx = x[i - 1] & 7, cy = y[j - 1] & 7;
                    op = OP_M;
                    rs += sub[cx * 8 + cy];
                    if (cx == cy && cx < 4) out->matches++; else out->mismatches++;
                    i--;
                    j--;
                } else if (H[c] == E[c]) {
                    st = 1;
                    continue;
                } else if (H[c] == F[c]) {
                    st = 2;
                    continue;
                } else {
                    out->err = 2;
                    break;
                }
            } else if (st == 1) {
                if (j < 1 || E[c] <= NEG / 2) { out->err = 3; break; }
                op = OP_I;
                st = E[c - 1] > H[c - 1] - gap_open ? 1 : 0; /* a tie opens */
                j--;
            } else {
                if (i < 1 || F[c] <= NEG / 2) { out->err = 4; break; }
                op = OP_D;
                st = F[c - W] > H[c - W] - gap_open ? 2 : 0;
                i--;
            }
            if (op == cur) {
                len++;
            } else {
                if (len) ops[n++] = len << 2 | (uint32_t)cur;
                cur = op;
                len = 1;
            }
        }
        if (!out->err && st != 0) out->err = 5;
        if (len) ops[n++] = len << 2 | (uint32_t)cur;
        for (uint32_t a = 0, b = n; a + 1 < b; a++, b--) {
            const uint32_t t = ops[a];
            ops[a] = ops[b - 1];
            ops[b - 1] = t;
        }
        out->n_ops = n;
        for (uint32_t k = 0; k < n; k++)
            if ((ops[k] & 3u) != OP_M) {
                out->gap_opens++;
                out->gap_bases += ops[k] >> 2;
                rs -= gap_open + (int32_t)(ops[k] >> 2) * gap_extend;
            }
        out->rescore = rs;
    }
done:
    free(H);
    free(E);
    free(F);
}
