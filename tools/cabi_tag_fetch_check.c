/* tools/cabi_tag_fetch_check.c — pure-C consumer of the tag projection
 * (bydb_rows_fetch_tags) through include/bydb_gpu.h alone: a row scan, then
 * the tags of the rows it returned, the way a cgo binding would fill the
 * TagValue columns of a raw-row result.
 *
 * Part: 2 blocks of 400 rows.  Slot 0 is a row-varying string env tag with
 * nil rows (a dictionary column), slot 1 a request id that never repeats (a
 * plain column: more than 256 distinct values).  Query: the 8 latest rows.
 * Slot 0 is fetched through the data_cap == 0 sizing call, slot 1 into a
 * buffer that is large enough at once; both are compared with what was
 * written.
 * Compile:
 *   gcc -std=c99 -I include tools/cabi_tag_fetch_check.c -L banyandb_amd \
 *       -lbydb_gpu -Wl,-rpath,banyandb_amd -o cabi_tag_fetch_check          */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bydb_gpu.h"

#define N 400
#define NBLK 2
#define LIMIT 8
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

/* NULL: a nil row */
static const char *env_of(int blk, int i) {
    if ((i / 5 + blk) % 4 == 3) return NULL;
    return ENVS[(i / 7 + blk) % 3];
}
static void req_of(int blk, int i, char *out) {
    sprintf(out, "req-%d-%04d", blk, i * 13);
}

int main(void) {
    static int64_t ts[N], ver[N], vals[N], lens[N];
    static uint8_t data[N * 16];
    char buf[32];
    bydb_part_builder *b = bydb_part_builder_create();
    CHECK(b, "builder create");
    for (int blk = 0; blk < NBLK; blk++) {
        for (int i = 0; i < N; i++) {
            ts[i] = T0 + (int64_t)(2 * i + blk) * MS;
            ver[i] = 1;
            vals[i] = (int64_t)i - 50;
        }
        CHECK(bydb_part_builder_add_block_i64(b, (uint64_t)(blk + 1), ts, ver,
                                              vals, N, 0) == BYDB_OK,
              "add_block");
        size_t off = 0;
        for (int i = 0; i < N; i++) {
            const char *e = env_of(blk, i);
            lens[i] = e ? (int64_t)strlen(e) : -1;
            if (e) { memcpy(data + off, e, strlen(e)); off += strlen(e); }
        }
        CHECK(bydb_part_builder_set_block_tag(b, data, lens, N) == BYDB_OK,
              "set env tag");
        off = 0;
        for (int i = 0; i < N; i++) {
            req_of(blk, i, buf);
            lens[i] = (int64_t)strlen(buf);
            memcpy(data + off, buf, strlen(buf));
            off += strlen(buf);
        }
        CHECK(bydb_part_builder_set_block_tag(b, data, lens, N) == BYDB_OK,
              "set request tag");
    }

    bydb_session *s = bydb_session_create(0);
    if (!s) { fprintf(stderr, "no GPU session\n"); return 2; }
    uint64_t seq0 = 0, offs[LIMIT + 1], total = 99;
    uint8_t nil[LIMIT];
    CHECK(bydb_rows_fetch_tags(s, &seq0, 1, 0, NULL, 0, offs, nil, &total) ==
              BYDB_ERR_STATE, "no part resident");
    uint64_t plen = bydb_part_builder_payload_len(b);
    int64_t nb = bydb_part_builder_n_blocks(b);
    CHECK(bydb_part_reserve(s, plen, nb) == BYDB_OK, "reserve");
    CHECK(bydb_part_append(s, bydb_part_builder_payload(b), plen,
                           bydb_part_builder_blocks(b), nb) == BYDB_OK,
          "append");

    CHECK(bydb_rows_configure(s, BYDB_VT_INT64, 0, LIMIT,
                              BYDB_ORDER_TS_DESC) == BYDB_OK, "rows_configure");
    CHECK(bydb_consume(s, INT64_MIN, INT64_MAX, NULL, 0) == BYDB_OK, "consume");
    bydb_top_row got[LIMIT];
    int64_t n_got = -1;
    CHECK(bydb_rows_finalize(s, got, LIMIT, &n_got) == BYDB_OK, "finalize");
    CHECK(n_got == LIMIT, "row count");
    uint64_t seqs[LIMIT];
    for (int i = 0; i < LIMIT; i++) {
        /* latest first: rows N-1, N-1, N-2, ... of blocks 1, 0, 1, ... */
        CHECK(got[i].ts == T0 + (int64_t)(2 * N - 1 - i) * MS, "ts");
        seqs[i] = got[i].seq;
    }

    /* argument limits are loud and leave the session usable */
    CHECK(bydb_rows_fetch_tags(s, seqs, LIMIT, 3, NULL, 0, offs, nil,
                               &total) == BYDB_ERR_BAD_ARG, "slot 3 rejected");
    CHECK(bydb_rows_fetch_tags(s, seqs, BYDB_TAG_FETCH_MAX + 1, 0, NULL, 0,
                               offs, nil, &total) == BYDB_ERR_BAD_ARG,
          "n above the limit rejected");

    /* slot 0: size the buffer with a first call, then fetch */
    CHECK(bydb_rows_fetch_tags(s, seqs, LIMIT, 0, NULL, 0, offs, nil,
                               &total) == BYDB_ERR_OOM, "sizing call");
    CHECK(total > 0 && offs[0] == 0 && offs[LIMIT] == total, "sized");
    uint8_t *env = (uint8_t *)malloc(total);
    CHECK(env, "malloc");
    uint64_t total2 = 0;
    CHECK(bydb_rows_fetch_tags(s, seqs, LIMIT, 0, env, total, offs, nil,
                               &total2) == BYDB_OK, "fetch slot 0");
    CHECK(total2 == total, "same total");
    int n_nil = 0;
    for (int i = 0; i < LIMIT; i++) {
        int blk = (int)(seqs[i] >> 13), row = (int)(seqs[i] & 8191);
        const char *e = env_of(blk, row);
        uint64_t len = offs[i + 1] - offs[i];
        if (!e) {
            CHECK(nil[i] == 1 && len == 0, "nil env");
            n_nil++;
            continue;
        }
        CHECK(nil[i] == 0 && len == strlen(e), "env length");
        CHECK(memcmp(env + offs[i], e, len) == 0, "env bytes");
    }
    CHECK(n_nil > 0 && n_nil < LIMIT, "both nil and valued rows fetched");

    /* slot 1: a buffer that is large enough at once */
    uint8_t req[LIMIT * 32];
    CHECK(bydb_rows_fetch_tags(s, seqs, LIMIT, 1, req, sizeof req, offs, nil,
                               &total) == BYDB_OK, "fetch slot 1");
    for (int i = 0; i < LIMIT; i++) {
        req_of((int)(seqs[i] >> 13), (int)(seqs[i] & 8191), buf);
        CHECK(nil[i] == 0 && offs[i + 1] - offs[i] == strlen(buf),
              "request id length");
        CHECK(memcmp(req + offs[i], buf, strlen(buf)) == 0,
              "request id bytes");
    }
    /* slot 2: no column, every row nil */
    CHECK(bydb_rows_fetch_tags(s, seqs, LIMIT, 2, NULL, 0, offs, nil,
                               &total) == BYDB_OK && total == 0,
          "absent slot");
    for (int i = 0; i < LIMIT; i++) CHECK(nil[i] == 1, "absent slot is nil");

    free(env);
    bydb_session_destroy(s);
    bydb_part_builder_destroy(b);
    printf("tag fetch consumer OK\n");
    return 0;
}
