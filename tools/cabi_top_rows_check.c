/* tools/cabi_top_rows_check.c — pure-C consumer of the raw-row BatchTop
 * operator (bydb_top_configure / bydb_top_finalize / bydb_top_rows_merge):
 * one filtered, clamped top-10 through include/bydb_gpu.h alone, the way a
 * cgo binding would map a measure query with `top` and no `agg`.
 *
 * Part: 3 blocks with a row-varying string env tag (slot 0).  Query: the 10
 * highest values among env != "dev" in a clamp that cuts all three blocks,
 * checked row for row against a host loop (insertion sort in storage order,
 * a later equal value never displaces an earlier one).
 * Compile:
 *   gcc -std=c99 -I include tools/cabi_top_rows_check.c -L banyandb_amd \
 *       -lbydb_gpu -Wl,-rpath,banyandb_amd -o cabi_top_rows_check          */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bydb_gpu.h"

#define N 1000
#define NBLK 3
#define TOPN 10
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

int main(void) {
    static int64_t ts[N], ver[N], vals[N], lens[N];
    static uint8_t data[N * 8];
    const int64_t lo = T0 + 100 * MS, hi = T0 + 899 * MS;
    bydb_top_row want[TOPN];
    int n_want = 0;
    bydb_part_builder *b = bydb_part_builder_create();
    CHECK(b, "builder create");
    for (int blk = 0; blk < NBLK; blk++) {
        size_t off = 0;
        for (int i = 0; i < N; i++) {
            ts[i] = T0 + (int64_t)i * MS;
            ver[i] = 1 + blk;
            /* many equal values, so ties cross rows and blocks */
            vals[i] = (int64_t)((i * 7919 + blk * 31) % 97) - 40;
            const char *e = ENVS[(i / 7 + blk) % 3];
            size_t l = strlen(e);
            memcpy(data + off, e, l);
            off += l;
            lens[i] = (int64_t)l;
            if (ts[i] < lo || ts[i] > hi || strcmp(e, "dev") == 0) continue;
            /* host BatchTop: keep the TOPN highest, earlier row first */
            int at = n_want;
            while (at > 0 && want[at - 1].value_i < vals[i]) at--;
            if (at >= TOPN) continue;
            int last = n_want < TOPN ? n_want : TOPN - 1;
            for (int k = last; k > at; k--) want[k] = want[k - 1];
            want[at].series_id = (uint64_t)blk + 1;
            want[at].ts = ts[i];
            want[at].version = ver[i];
            want[at].value_i = vals[i];
            want[at].value_f = 0.0;
            want[at].seq = ((uint64_t)blk << 13) | (uint64_t)i;
            if (n_want < TOPN) n_want++;
        }
        CHECK(bydb_part_builder_add_block_i64(b, (uint64_t)blk + 1, ts, ver,
                                              vals, N, 0) == BYDB_OK,
              "add_block");
        CHECK(bydb_part_builder_set_block_tag(b, data, lens, N) == BYDB_OK,
              "set env tag");
    }
    CHECK(n_want == TOPN, "host reference is vacuous");

    bydb_session *s = bydb_session_create(0);
    if (!s) { fprintf(stderr, "no GPU session\n"); return 2; }
    uint64_t plen = bydb_part_builder_payload_len(b);
    int64_t nb = bydb_part_builder_n_blocks(b);
    CHECK(bydb_part_reserve(s, plen, nb) == BYDB_OK, "reserve");
    CHECK(bydb_part_append(s, bydb_part_builder_payload(b), plen,
                           bydb_part_builder_blocks(b), nb) == BYDB_OK,
          "append");

    /* argument limits are loud and leave the session usable */
    CHECK(bydb_top_configure(s, BYDB_VT_INT64, BYDB_TOP_ROWS_MAX + 1, 0) ==
              BYDB_ERR_BAD_ARG, "n above the limit rejected");
    CHECK(bydb_top_configure(s, BYDB_VT_INT64, -1, 0) == BYDB_ERR_BAD_ARG,
          "negative n rejected");
    CHECK(bydb_top_configure(s, BYDB_VT_INT64, TOPN, 0) == BYDB_OK,
          "top_configure");

    const uint64_t offs_dev[2] = {0, 3};
    bydb_tag_cond cond;
    memset(&cond, 0, sizeof(cond));
    cond.slot = 0; cond.op = BYDB_OP_NE;
    cond.tag_type = BYDB_TAG_STRING; cond.n_values = 1;
    cond.values = (const uint8_t *)"dev"; cond.value_offs = offs_dev;
    CHECK(bydb_consume_filter(s, lo, hi, &cond, 1) == BYDB_OK, "consume");
    CHECK(bydb_consume_filter(s, lo, hi, &cond, 1) == BYDB_ERR_STATE,
          "second consume in one epoch rejected");

    bydb_top_row got[TOPN];
    int64_t n_got = -1;
    CHECK(bydb_top_finalize(s, got, 1, &n_got) == BYDB_ERR_OOM && n_got == TOPN,
          "small cap reports the needed count");
    CHECK(bydb_top_finalize(s, got, TOPN, &n_got) == BYDB_OK, "top_finalize");
    CHECK(n_got == TOPN, "row count");
    for (int i = 0; i < TOPN; i++) {
        CHECK(got[i].series_id == want[i].series_id, "series_id");
        CHECK(got[i].ts == want[i].ts, "ts");
        CHECK(got[i].version == want[i].version, "version");
        CHECK(got[i].value_i == want[i].value_i, "value_i");
        CHECK(got[i].value_f == 0.0, "value_f");
        CHECK(got[i].seq == want[i].seq, "seq");
    }

    /* the reduce side: the result split in two shards merges back */
    const bydb_top_row *lists[2] = {got, got + 4};
    const int64_t llens[2] = {4, TOPN - 4};
    bydb_top_row merged[TOPN];
    int64_t n_merged = 0;
    CHECK(bydb_top_rows_merge(lists, llens, 2, BYDB_VT_INT64, TOPN, 0, merged,
                              &n_merged) == BYDB_OK, "merge");
    CHECK(n_merged == TOPN, "merged count");
    for (int i = 0; i < TOPN; i++)
        CHECK(merged[i].seq == got[i].seq, "merged order");

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
    printf("top rows consumer OK (best=%lld at seq %llu)\n",
           (long long)got[0].value_i, (unsigned long long)got[0].seq);
    return 0;
}
