/* tools/cabi_filter_check.c — pure-C consumer of bydb_consume_filter: one
 * filtered scan through include/bydb_gpu.h alone, the way a cgo binding
 * would map a measure query's conditions.
 *
 * Part: 2 blocks with a row-varying int status-code tag (slot 0) and a
 * string env tag (slot 1).  Query: 200 <= code < 500 AND env != "dev"
 * AND code NOT_IN (404), checked against a host loop over the same rows.
 * Compile:
 *   gcc -std=c99 -I include tools/cabi_filter_check.c -L banyandb_amd \
 *       -lbydb_gpu -Wl,-rpath,banyandb_amd -o cabi_filter_check        */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bydb_gpu.h"

#define N 1000
#define T0 1700000000000000000LL

#define CHECK(cond, what)                                                 \
    do {                                                                  \
        if (!(cond)) {                                                    \
            fprintf(stderr, "FAIL %s (%s:%d)\n", what, __FILE__,          \
                    __LINE__);                                            \
            return 1;                                                     \
        }                                                                 \
    } while (0)

static const int64_t CODES[5] = {-1, 200, 302, 404, 503};
static const char *ENVS[3] = {"prod", "dev", "qa"};

/* convert.Int64ToBytes: big-endian with the sign bit flipped */
static void i64_cell(int64_t v, uint8_t out[8]) {
    uint64_t u = (uint64_t)v ^ ((uint64_t)1 << 63);
    for (int i = 0; i < 8; i++) out[i] = (uint8_t)(u >> (56 - 8 * i));
}

int main(void) {
    static int64_t ts[N], ver[N], vals[N], lens[N];
    static uint8_t data[N * 8];
    int64_t want_sum = 0, want_cnt = 0;
    bydb_part_builder *b = bydb_part_builder_create();
    CHECK(b, "builder create");
    for (int i = 0; i < N; i++) {
        ts[i] = T0 + (int64_t)i * 1000000LL;
        ver[i] = 1;
        vals[i] = (int64_t)(i * 37 - 5000);
    }
    for (int blk = 0; blk < 2; blk++) {
        CHECK(bydb_part_builder_add_block_i64(b, (uint64_t)blk + 1, ts, ver,
                                              vals, N, 0) == BYDB_OK,
              "add_block");
        for (int i = 0; i < N; i++) {           /* slot 0: int code */
            i64_cell(CODES[(i / 5 + blk) % 5], data + 8 * i);
            lens[i] = 8;
        }
        CHECK(bydb_part_builder_set_block_tag(b, data, lens, N) == BYDB_OK,
              "set code tag");
        size_t off = 0;
        for (int i = 0; i < N; i++) {           /* slot 1: string env */
            const char *e = ENVS[(i / 11 + blk) % 3];
            size_t l = strlen(e);
            memcpy(data + off, e, l);
            off += l;
            lens[i] = (int64_t)l;
            int64_t code = CODES[(i / 5 + blk) % 5];
            if (code >= 200 && code < 500 && code != 404 &&
                strcmp(e, "dev") != 0) {
                want_sum += vals[i];
                want_cnt++;
            }
        }
        CHECK(bydb_part_builder_set_block_tag(b, data, lens, N) == BYDB_OK,
              "set env tag");
    }
    CHECK(want_cnt > 0 && want_cnt < 2 * N, "host reference is vacuous");

    bydb_session *s = bydb_session_create(0);
    if (!s) { fprintf(stderr, "no GPU session\n"); return 2; }
    uint64_t plen = bydb_part_builder_payload_len(b);
    int64_t nb = bydb_part_builder_n_blocks(b);
    CHECK(bydb_part_reserve(s, plen, nb) == BYDB_OK, "reserve");
    CHECK(bydb_part_append(s, bydb_part_builder_payload(b), plen,
                           bydb_part_builder_blocks(b), nb) == BYDB_OK,
          "append");
    CHECK(bydb_agg_configure(s, BYDB_VT_INT64,
                             (1u << BYDB_AGG_SUM) | (1u << BYDB_AGG_COUNT),
                             1, BYDB_MODE_ALL) == BYDB_OK,
          "configure");

    uint8_t lo[8], hi[8], c404[8];
    i64_cell(200, lo);
    i64_cell(500, hi);
    i64_cell(404, c404);
    const uint64_t offs8[2] = {0, 8};
    const uint64_t offs_dev[2] = {0, 3};
    bydb_tag_cond conds[4];
    memset(conds, 0, sizeof(conds));
    conds[0].slot = 0; conds[0].op = BYDB_OP_GE;
    conds[0].tag_type = BYDB_TAG_INT; conds[0].n_values = 1;
    conds[0].values = lo; conds[0].value_offs = offs8;
    conds[1].slot = 0; conds[1].op = BYDB_OP_LT;
    conds[1].tag_type = BYDB_TAG_INT; conds[1].n_values = 1;
    conds[1].values = hi; conds[1].value_offs = offs8;
    conds[2].slot = 1; conds[2].op = BYDB_OP_NE;
    conds[2].tag_type = BYDB_TAG_STRING; conds[2].n_values = 1;
    conds[2].values = (const uint8_t *)"dev"; conds[2].value_offs = offs_dev;
    conds[3].slot = 0; conds[3].op = BYDB_OP_NOT_IN;
    conds[3].tag_type = BYDB_TAG_INT; conds[3].n_values = 1;
    conds[3].values = c404; conds[3].value_offs = offs8;

    CHECK(bydb_consume_filter(s, INT64_MIN, INT64_MAX, conds, 4) == BYDB_OK,
          "consume_filter");
    bydb_result r;
    CHECK(bydb_finalize(s, &r, 1) == BYDB_OK, "finalize");
    CHECK(r.count == want_cnt, "filtered count");
    CHECK(r.sum_i == want_sum, "filtered sum");

    /* argument limits are loud and leave the session usable */
    conds[0].n_values = 0;
    CHECK(bydb_consume_filter(s, INT64_MIN, INT64_MAX, conds, 4) ==
              BYDB_ERR_BAD_ARG,
          "zero values rejected");
    conds[0].n_values = 1;
    CHECK(bydb_reset(s) == BYDB_OK, "reset");
    CHECK(bydb_consume_filter(s, INT64_MIN, INT64_MAX, conds, 0) == BYDB_OK,
          "unfiltered scan");
    CHECK(bydb_finalize(s, &r, 1) == BYDB_OK, "finalize 2");
    CHECK(r.count == 2 * N, "unfiltered count");

    bydb_session_destroy(s);
    bydb_part_builder_destroy(b);
    printf("filter consumer OK (count=%lld sum=%lld)\n",
           (long long)r.count, (long long)want_sum);
    return 0;
}
