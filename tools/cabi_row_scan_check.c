/* tools/cabi_row_scan_check.c — pure-C consumer of the time-ordered row scan
 * (bydb_rows_configure / bydb_rows_finalize / bydb_rows_merge): one
 * filtered, clamped "rows 5..16, latest first" through include/bydb_gpu.h
 * alone, the way a cgo binding would map a measure query with neither `agg`
 * nor `top`.
 *
 * Part: 3 blocks (series 3, 1, 2 in append order) on the same timestamps,
 * with a row-varying string env tag (slot 0).  Query: env != "dev" in a
 * clamp that cuts all three blocks, ordered by timestamp descending, then
 * series ascending; offset 5, limit 12.  Checked row for row against a host
 * loop over (timestamp, series).
 * Compile:
 *   gcc -std=c99 -I include tools/cabi_row_scan_check.c -L banyandb_amd \
 *       -lbydb_gpu -Wl,-rpath,banyandb_amd -o cabi_row_scan_check           */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bydb_gpu.h"

#define N 1000
#define NBLK 3
#define OFFSET 5
#define LIMIT 12
#define T0 1700000000000000000LL
#define MS 1000000LL

#define CHECK(cond, what)                                                 \
    do {                                                                  \
        if (!(cond)) {                                                    \
            fprintf(stderr, "FAIL %s (%s:%d)\n", what, __FILE__,          \
                    __LINE__);                                            \
            return 1;                                                     \
        }                                                                 \
    } while (0)

static const char *ENVS[3] = {"prod", "dev", "qa"};
static const uint64_t SERIES[NBLK] = {3, 1, 2};

static const char *env_of(int blk, int i) { return ENVS[(i / 7 + blk) % 3]; }
static int64_t val_of(int blk, int i) {
    return (int64_t)((i * 7919 + blk * 31) % 97) - 40;
}

int main(void) {
    static int64_t ts[N], ver[N], vals[N], lens[N];
    static uint8_t data[N * 8];
    const int64_t lo = T0 + 100 * MS, hi = T0 + 899 * MS;
    bydb_top_row want[OFFSET + LIMIT];
    int n_want = 0;
    bydb_part_builder *b = bydb_part_builder_create();
    CHECK(b, "builder create");
    for (int blk = 0; blk < NBLK; blk++) {
        size_t off = 0;
        for (int i = 0; i < N; i++) {
            ts[i] = T0 + (int64_t)i * MS;
            ver[i] = 1 + blk;
            vals[i] = val_of(blk, i);
            const char *e = env_of(blk, i);
            size_t l = strlen(e);
            memcpy(data + off, e, l);
            off += l;
            lens[i] = (int64_t)l;
        }
        CHECK(bydb_part_builder_add_block_i64(b, SERIES[blk], ts, ver, vals, N,
                                              0) == BYDB_OK, "add_block");
        CHECK(bydb_part_builder_set_block_tag(b, data, lens, N) == BYDB_OK,
              "set env tag");
    }
    /* host reference: timestamps descending, series 1, 2, 3 at each */
    for (int i = N - 1; i >= 0 && n_want < OFFSET + LIMIT; i--) {
        int64_t t = T0 + (int64_t)i * MS;
        if (t < lo || t > hi) continue;
        for (uint64_t sid = 1; sid <= NBLK && n_want < OFFSET + LIMIT; sid++) {
            int blk = 0;
            while (SERIES[blk] != sid) blk++;
            if (strcmp(env_of(blk, i), "dev") == 0) continue;
            want[n_want].series_id = sid;
            want[n_want].ts = t;
            want[n_want].version = 1 + blk;
            want[n_want].value_i = val_of(blk, i);
            want[n_want].value_f = 0.0;
            want[n_want].seq = ((uint64_t)blk << 13) | (uint64_t)i;
            n_want++;
        }
    }
    CHECK(n_want == OFFSET + LIMIT, "host reference is vacuous");

    bydb_session *s = bydb_session_create(0);
    if (!s) { fprintf(stderr, "no GPU session\n"); return 2; }
    uint64_t plen = bydb_part_builder_payload_len(b);
    int64_t nb = bydb_part_builder_n_blocks(b);
    CHECK(bydb_part_reserve(s, plen, nb) == BYDB_OK, "reserve");
    CHECK(bydb_part_append(s, bydb_part_builder_payload(b), plen,
                           bydb_part_builder_blocks(b), nb) == BYDB_OK,
          "append");

    /* argument limits are loud and leave the session usable */
    CHECK(bydb_rows_configure(s, BYDB_VT_INT64, 1, BYDB_TOP_ROWS_MAX,
                              BYDB_ORDER_TS_ASC) == BYDB_ERR_BAD_ARG,
          "window above the limit rejected");
    CHECK(bydb_rows_configure(s, BYDB_VT_INT64, -1, 3, BYDB_ORDER_TS_ASC) ==
              BYDB_ERR_BAD_ARG, "negative offset rejected");
    CHECK(bydb_rows_configure(s, BYDB_VT_INT64, 0, 3, 2) == BYDB_ERR_BAD_ARG,
          "unknown order rejected");
    CHECK(bydb_rows_configure(s, BYDB_VT_INT64, OFFSET, LIMIT,
                              BYDB_ORDER_TS_DESC) == BYDB_OK,
          "rows_configure");

    const uint64_t offs_dev[2] = {0, 3};
    bydb_tag_cond cond;
    memset(&cond, 0, sizeof(cond));
    cond.slot = 0; cond.op = BYDB_OP_NE;
    cond.tag_type = BYDB_TAG_STRING; cond.n_values = 1;
    cond.values = (const uint8_t *)"dev"; cond.value_offs = offs_dev;
    CHECK(bydb_consume_filter(s, lo, hi, &cond, 1) == BYDB_OK, "consume");
    CHECK(bydb_consume_filter(s, lo, hi, &cond, 1) == BYDB_ERR_STATE,
          "second consume in one epoch rejected");

    bydb_top_row got[LIMIT];
    int64_t n_got = -1;
    CHECK(bydb_rows_finalize(s, got, 1, &n_got) == BYDB_ERR_OOM &&
              n_got == LIMIT, "small cap reports the needed count");
    CHECK(bydb_rows_finalize(s, got, LIMIT, &n_got) == BYDB_OK,
          "rows_finalize");
    CHECK(n_got == LIMIT, "row count");
    for (int i = 0; i < LIMIT; i++) {
        const bydb_top_row *w = &want[OFFSET + i];
        CHECK(got[i].series_id == w->series_id, "series_id");
        CHECK(got[i].ts == w->ts, "ts");
        CHECK(got[i].version == w->version, "version");
        CHECK(got[i].value_i == w->value_i, "value_i");
        CHECK(got[i].value_f == 0.0, "value_f");
        CHECK(got[i].seq == w->seq, "seq");
    }

    /* the reduce side: the rows dealt out to two shards merge back, and the
     * window is cut after the merge */
    bydb_top_row even[LIMIT], odd[LIMIT];
    int n_even = 0, n_odd = 0;
    for (int i = 0; i < LIMIT; i++) {
        if (i % 2 == 0) even[n_even++] = got[i];
        else odd[n_odd++] = got[i];
    }
    const bydb_top_row *lists[2] = {odd, even};
    const int64_t llens[2] = {n_odd, n_even};
    bydb_top_row merged[LIMIT];
    int64_t n_merged = 0;
    CHECK(bydb_rows_merge(lists, llens, 2, 2, 7, BYDB_ORDER_TS_DESC, merged,
                          &n_merged) == BYDB_OK, "merge");
    CHECK(n_merged == 7, "merged count");
    for (int i = 0; i < 7; i++)
        CHECK(merged[i].seq == got[2 + i].seq, "merged order");
    CHECK(bydb_rows_merge(lists, llens, 2, 0, 3, 7, merged, &n_merged) ==
              BYDB_ERR_BAD_ARG, "merge rejects an unknown order");

    /* back to an aggregate on the same session */
    CHECK(bydb_agg_configure(s, BYDB_VT_INT64, 1u << BYDB_AGG_COUNT, 1,
                             BYDB_MODE_ALL) == BYDB_OK, "agg configure");
    CHECK(bydb_consume(s, INT64_MIN, INT64_MAX, NULL, 0) == BYDB_OK,
          "agg consume");
    bydb_result r;
    CHECK(bydb_finalize(s, &r, 1) == BYDB_OK, "agg finalize");
    CHECK(r.count == NBLK * N, "agg count");

    bydb_session_destroy(s);
    bydb_part_builder_destroy(b);
    printf("row scan consumer OK (first=series %llu at seq %llu)\n",
           (unsigned long long)got[0].series_id,
           (unsigned long long)got[0].seq);
    return 0;
}
