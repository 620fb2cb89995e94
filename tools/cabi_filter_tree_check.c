/* tools/cabi_filter_tree_check.c — pure-C consumer of
 * bydb_consume_filter_tree: one OR-tree scan through include/bydb_gpu.h
 * alone, the way a cgo binding would flatten a modelv1.Criteria tree
 * (INTEGRATION.md).
 *
 * Part: 2 blocks with a row-varying int status-code tag (slot 0) and a
 * string env tag (slot 1).  Query: code >= 500 OR (env = "prod" AND
 * code != 404), checked against a host loop over the same rows.
 * Compile:
 *   gcc -std=c99 -I include tools/cabi_filter_tree_check.c -L banyandb_amd \
 *       -lbydb_gpu -Wl,-rpath,banyandb_amd -o cabi_filter_tree_check     */
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
            if (code >= 500 || (strcmp(e, "prod") == 0 && code != 404)) {
                want_sum += vals[i];
                want_cnt++;
            }
        }
        CHECK(bydb_part_builder_set_block_tag(b, data, lens, N) == BYDB_OK,
              "set env tag");
    }
    CHECK(want_cnt > 0 && want_cnt < 2 * N, "host reference is vacuous");

    uint8_t c500[8], c404[8];
    i64_cell(500, c500);
    i64_cell(404, c404);
    const uint64_t offs8[2] = {0, 8};
    const uint64_t offs_prod[2] = {0, 4};
    bydb_tag_cond conds[3];
    memset(conds, 0, sizeof(conds));
    conds[0].slot = 0; conds[0].op = BYDB_OP_GE;
    conds[0].tag_type = BYDB_TAG_INT; conds[0].n_values = 1;
    conds[0].values = c500; conds[0].value_offs = offs8;
    conds[1].slot = 1; conds[1].op = BYDB_OP_EQ;
    conds[1].tag_type = BYDB_TAG_STRING; conds[1].n_values = 1;
    conds[1].values = (const uint8_t *)"prod"; conds[1].value_offs = offs_prod;
    conds[2].slot = 0; conds[2].op = BYDB_OP_NE;
    conds[2].tag_type = BYDB_TAG_INT; conds[2].n_values = 1;
    conds[2].values = c404; conds[2].value_offs = offs8;
    /* post-order: c0, c1, c2, (c1 AND c2), (c0 OR that) */
    bydb_filter_node nodes[5] = {
        {BYDB_NODE_LEAF, 0, 0}, {BYDB_NODE_LEAF, 1, 0},
        {BYDB_NODE_LEAF, 2, 0}, {BYDB_NODE_AND, 1, 2},
        {BYDB_NODE_OR, 0, 3},
    };

    /* the truth table needs no GPU: bit sig = c0 | (c1 & c2) */
    uint64_t table[4];
    CHECK(bydb_filter_tree_table(nodes, 5, 3, table) == BYDB_OK, "table");
    CHECK(table[0] == 0xEA && !table[1] && !table[2] && !table[3],
          "truth table");
    nodes[4].right = 4;     /* a node as its own child */
    CHECK(bydb_filter_tree_table(nodes, 5, 3, table) == BYDB_ERR_BAD_ARG,
          "malformed tree rejected");
    nodes[4].right = 3;

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

    CHECK(bydb_consume_filter_tree(s, INT64_MIN, INT64_MAX, conds, 3, nodes,
                                   5) == BYDB_OK,
          "consume_filter_tree");
    bydb_result r;
    CHECK(bydb_finalize(s, &r, 1) == BYDB_OK, "finalize");
    CHECK(r.count == want_cnt, "tree count");
    CHECK(r.sum_i == want_sum, "tree sum");
    uint64_t stats[4];
    CHECK(bydb_filter_tree_stats(s, stats) == BYDB_OK, "stats");
    CHECK(stats[0] + stats[1] + stats[2] + stats[3] == (uint64_t)nb,
          "every block has a verdict");
    CHECK(stats[3] == (uint64_t)nb, "two varying slots: row-bitmap blocks");

    /* a malformed tree is loud and leaves the session usable */
    nodes[3].left = 0;      /* node 0 gets two parents, node 1 none */
    CHECK(bydb_consume_filter_tree(s, INT64_MIN, INT64_MAX, conds, 3, nodes,
                                   5) == BYDB_ERR_BAD_ARG,
          "two parents rejected");
    nodes[3].left = 1;
    CHECK(bydb_reset(s) == BYDB_OK, "reset");
    CHECK(bydb_consume_filter_tree(s, INT64_MIN, INT64_MAX, NULL, 0, NULL,
                                   0) == BYDB_OK,
          "unfiltered scan");
    bydb_result r2;
    CHECK(bydb_finalize(s, &r2, 1) == BYDB_OK, "finalize 2");
    CHECK(r2.count == 2 * N, "unfiltered count");

    bydb_session_destroy(s);
    bydb_part_builder_destroy(b);
    printf("filter tree consumer OK (count=%lld sum=%lld)\n",
           (long long)r.count, (long long)r.sum_i);
    return 0;
}
