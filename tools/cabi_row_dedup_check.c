/* tools/cabi_row_dedup_check.c — pure-C consumer of the cross-part version
 * dedup: the overlap planner and one deduped scan through
 * include/bydb_gpu.h alone, the way a cgo binding would turn on the
 * measure query's merge.
 *
 * Part: series 1 written as one block of N rows at version 1, then a
 * "newer part" block that re-sends rows [LO, HI) at version 2 with
 * corrected values, plus an untouched series 2.  Checked against a host
 * loop over the same rows.
 * Compile:
 *   gcc -std=c99 -I include tools/cabi_row_dedup_check.c -L banyandb_amd \
 *       -lbydb_gpu -Wl,-rpath,banyandb_amd -o cabi_row_dedup_check       */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bydb_gpu.h"

#define N 1000
#define LO 300
#define HI 650
#define T0 1700000000000000000LL

#define CHECK(cond, what)                                                 \
    do {                                                                  \
        if (!(cond)) {                                                    \
            fprintf(stderr, "FAIL %s (%s:%d)\n", what, __FILE__,          \
                    __LINE__);                                            \
            return 1;                                                     \
        }                                                                 \
    } while (0)

int main(void) {
    static int64_t ts[N], ver[N], vals[N], fix[N];
    int64_t all_sum = 0, want_sum = 0;
    bydb_part_builder *b = bydb_part_builder_create();
    CHECK(b, "builder create");
    for (int i = 0; i < N; i++) {
        ts[i] = T0 + (int64_t)i * 1000000LL;
        ver[i] = 1;
        vals[i] = (int64_t)(i * 37 - 5000);
        fix[i] = (int64_t)(1000000 + i);
    }
    /* block 0: series 1, version 1; block 1: series 2, untouched */
    CHECK(bydb_part_builder_add_block_i64(b, 1, ts, ver, vals, N, 0) ==
              BYDB_OK, "add series 1");
    CHECK(bydb_part_builder_add_block_i64(b, 2, ts, ver, vals, N, 0) ==
              BYDB_OK, "add series 2");
    /* block 2: the correction of rows [LO, HI) of series 1, version 2 */
    for (int i = 0; i < N; i++) ver[i] = 2;
    CHECK(bydb_part_builder_add_block_i64(b, 1, ts + LO, ver, fix + LO,
                                          HI - LO, 0) == BYDB_OK,
          "add correction");
    for (int i = 0; i < N; i++) {
        all_sum += 2 * vals[i];
        want_sum += vals[i];                              /* series 2 */
        want_sum += (i >= LO && i < HI) ? fix[i] : vals[i];
        if (i >= LO && i < HI) all_sum += fix[i];
    }
    const int64_t all_cnt = 2 * N + (HI - LO), want_cnt = 2 * N;

    /* the planner needs no GPU: blocks 0 and 2 are each other's peers */
    const bydb_block_desc *descs = bydb_part_builder_blocks(b);
    int64_t nb = bydb_part_builder_n_blocks(b);
    CHECK(nb == 3, "three blocks");
    uint64_t offs[4], n_peers = 99;
    uint32_t peers[2] = {77, 77};
    CHECK(bydb_row_dedup_peers(descs, nb, offs, NULL, 0, &n_peers) ==
              BYDB_ERR_OOM, "sizing call");
    CHECK(n_peers == 2, "required size");
    CHECK(bydb_row_dedup_peers(descs, nb, offs, peers, 2, &n_peers) ==
              BYDB_OK, "planner");
    CHECK(offs[0] == 0 && offs[1] == 1 && offs[2] == 1 && offs[3] == 2,
          "peer offsets");
    CHECK(peers[0] == 2 && peers[1] == 0, "peer lists");

    bydb_session *s = bydb_session_create(0);
    if (!s) { fprintf(stderr, "no GPU session\n"); return 2; }
    uint64_t plen = bydb_part_builder_payload_len(b);
    CHECK(bydb_part_reserve(s, plen, nb) == BYDB_OK, "reserve");
    CHECK(bydb_part_append(s, bydb_part_builder_payload(b), plen, descs,
                           nb) == BYDB_OK, "append");
    CHECK(bydb_agg_configure(s, BYDB_VT_INT64,
                             (1u << BYDB_AGG_SUM) | (1u << BYDB_AGG_COUNT),
                             1, BYDB_MODE_ALL) == BYDB_OK, "configure");

    /* off by default: every row folds, the stats are zero */
    bydb_result r;
    uint64_t st[4];
    CHECK(bydb_consume(s, INT64_MIN, INT64_MAX, NULL, 0) == BYDB_OK,
          "consume, dedup off");
    CHECK(bydb_finalize(s, &r, 1) == BYDB_OK, "finalize");
    CHECK(r.count == all_cnt && r.sum_i == all_sum, "dedup off folds all");
    CHECK(bydb_row_dedup_stats(s, st) == BYDB_OK, "stats");
    CHECK(!st[0] && !st[1] && !st[2] && !st[3], "stats zero while off");

    /* bad values are refused, the session stays usable */
    CHECK(bydb_set_row_dedup(s, 2) == BYDB_ERR_BAD_ARG, "2 rejected");
    CHECK(bydb_set_row_dedup(s, -1) == BYDB_ERR_BAD_ARG, "-1 rejected");
    CHECK(bydb_set_row_dedup(s, 1) == BYDB_OK, "dedup on");
    CHECK(bydb_row_dedup_stats(s, st) == BYDB_OK, "stats");
    CHECK(!st[0] && !st[1] && !st[2] && !st[3], "stats zero before a consume");

    CHECK(bydb_reset(s) == BYDB_OK, "reset");
    CHECK(bydb_consume(s, INT64_MIN, INT64_MAX, NULL, 0) == BYDB_OK,
          "consume, dedup on");
    CHECK(bydb_finalize(s, &r, 1) == BYDB_OK, "finalize");
    CHECK(r.count == want_cnt, "deduped count");
    CHECK(r.sum_i == want_sum, "deduped sum");
    CHECK(bydb_row_dedup_stats(s, st) == BYDB_OK, "stats");
    CHECK(st[0] == 2 && st[1] == 1 && st[2] == 0 &&
              st[3] == (uint64_t)(HI - LO), "dedup stats");

    /* a clamp inside the corrected stretch sees only the corrections */
    int64_t in_sum = 0;
    for (int i = LO + 10; i <= LO + 20; i++) in_sum += fix[i] + vals[i];
    CHECK(bydb_reset(s) == BYDB_OK, "reset");
    CHECK(bydb_consume(s, ts[LO + 10], ts[LO + 20], NULL, 0) == BYDB_OK,
          "clamped consume");
    CHECK(bydb_finalize(s, &r, 1) == BYDB_OK, "finalize");
    CHECK(r.count == 22 && r.sum_i == in_sum, "clamped deduped fold");

    /* and off again is the plain scan */
    CHECK(bydb_set_row_dedup(s, 0) == BYDB_OK, "dedup off");
    CHECK(bydb_reset(s) == BYDB_OK, "reset");
    CHECK(bydb_consume(s, INT64_MIN, INT64_MAX, NULL, 0) == BYDB_OK,
          "consume, off again");
    CHECK(bydb_finalize(s, &r, 1) == BYDB_OK, "finalize");
    CHECK(r.count == all_cnt && r.sum_i == all_sum, "off again folds all");

    bydb_session_destroy(s);
    bydb_part_builder_destroy(b);
    printf("row dedup consumer OK (count=%lld sum=%lld dropped=%llu)\n",
           (long long)want_cnt, (long long)want_sum,
           (unsigned long long)st[3]);
    return 0;
}
