/*
 * fill_check_main.c -- a stand-alone driver of fill_check.c for sanitizer builds: rectangles from a fixed pseudo-random sequence,
 * with separators, empty sides, single rows and columns, and an output array smaller than what is found.  Prints a checksum.
 *   cc -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/cpp/fill_check.c tests/cpp/fill_check_main.c -o fill_check_san
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

typedef struct {
    uint32_t i, j, len;
    int32_t score;
} fc_hsp;
uint64_t fc_scan(const uint8_t* x, int64_t dt, const uint8_t* y, int64_t dq, const int32_t* sub, int32_t thresh, int32_t xdrop, fc_hsp* out,
                 uint64_t cap);

static uint32_t state = 12345u;
static uint32_t next(void) {
    state = state * 1664525u + 1013904223u;
    return state >> 8;
}

int main(void) {
    int32_t sub[64];
    uint64_t sum = 0, total = 0;
    for (int a = 0; a < 8; a++)
        for (int b = 0; b < 8; b++) sub[a * 8 + b] = (a == 7 || b == 7) ? -9100 : (a > 3 || b > 3) ? -100 : a == b ? 95 : -110;
    for (int round = 0; round < 400; round++) {
        const int64_t dt = round % 7 == 0 ? 1 : next() % 90, dq = round % 11 == 0 ? 1 : next() % 90;
        /* exact allocations, so that a read or write past either range is reported */
        uint8_t* x = (uint8_t*)malloc(dt ? (size_t)dt : 1);
        uint8_t* y = (uint8_t*)malloc(dq ? (size_t)dq : 1);
        const uint64_t cap = round % 5 == 0 ? 3 : 20000;
        fc_hsp* out = (fc_hsp*)malloc(cap * sizeof(fc_hsp));
        if (!x || !y || !out) return 2;
        for (int64_t k = 0; k < dt; k++) x[k] = next() % 50 == 0 ? 7 : (uint8_t)(next() % 2);
        for (int64_t k = 0; k < dq; k++) y[k] = next() % 50 == 0 ? 7 : (uint8_t)(next() % 2);
        const int32_t thresh = 1 + (int32_t)(next() % 400), xdrop = (int32_t)(next() % 300);
        const uint64_t n = fc_scan(x, dt, y, dq, sub, thresh, xdrop, out, cap);
        total += n;
        for (uint64_t k = 0; k < n && k < cap; k++) {
            if ((int64_t)out[k].i + out[k].len >= dt || (int64_t)out[k].j + out[k].len >= dq || out[k].score < thresh) {
                printf("bad HSP in round %d\n", round);
                return 1;
            }
            sum = sum * 31 + out[k].i + 7 * out[k].j + 13 * out[k].len + (uint64_t)out[k].score;
        }
        free(x);
        free(y);
        free(out);
    }
    printf("fill_check: %llu HSPs, checksum %llu\n", (unsigned long long)total, (unsigned long long)sum);
    return total > 1000 ? 0 : 1;
}
