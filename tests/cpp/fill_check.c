/*
 * fill_check.c -- serial restatement of the scan of one link of sa_fill_chains (include/segalign_amd.h).
 *
 * Plain C: one scalar loop per diagonal, the diagonals one after the other, deliberately NOT in the row-stepping form of the kernel
 * (fill.hip steps along the target rows with 64 diagonals side by side).  The tests hold it against a direct Python restatement of
 * the contract on small rectangles, hand-worked cases and every link the engine sweeps.
 */
#include <stdint.h>
#include <stddef.h>

#define SEP 7 /* the record separator */

typedef struct {
    uint32_t i, j, len; /* the first column's place inside the rectangle; columns - 1 */
    int32_t score;
} fc_hsp;

/* x: the dt target codes of the link, y: its dq query codes.  Writes at most cap HSPs in the contract's order (d ascending, then i
 * ascending) and returns how many there are, which may exceed cap. */
uint64_t fc_scan(const uint8_t* x, int64_t dt, const uint8_t* y, int64_t dq, const int32_t* sub, int32_t thresh, int32_t xdrop, fc_hsp* out,
                 uint64_t cap) {
    uint64_t found = 0;
    if (dt <= 0 || dq <= 0) return 0;
    for (int64_t d = -(dq - 1); d <= dt - 1; d++) {
        const int64_t i0 = d > 0 ? d : 0, j0 = d < 0 ? -d : 0;
        const int64_t n = (dt - i0) < (dq - j0) ? (dt - i0) : (dq - j0);
        int32_t s = 0, b = 0;
        int64_t start = 0, bend = 0;
        for (int64_t k = 0; k <= n; k++) {
            int flush = 0;
            if (k == n) {
                flush = 1; /* the diagonal's end */
            } else {
                const int a = x[i0 + k] & 7, c = y[j0 + k] & 7;
                if (a == SEP || c == SEP) {
                    flush = 1;
                } else {
                    if (s == 0 && b == 0) start = k;
                    s += sub[a * 8 + c];
                    if (s > b) {
                        b = s;
                        bend = k;
                    }
                    if (s <= 0 || b - s > xdrop) flush = 1;
                }
            }
            if (flush) {
                if (b >= thresh) {
                    if (found < cap) {
                        out[found].i = (uint32_t)(i0 + start);
                        out[found].j = (uint32_t)(j0 + start);
                        out[found].len = (uint32_t)(bend - start);
                        out[found].score = b;
                    }
                    found++;
                }
                s = b = 0;
            }
        }
    }
    return found;
}
