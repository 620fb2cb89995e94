// banyandb_amd/csrc/kernels.hip — MI355X (gfx950) decode+fold kernels and
// the C-ABI session around them.
//
// Hot path replaced (apache/skywalking-banyandb):
//   blockCursor.loadData -> block.mustReadFrom (banyand/measure/block.go:818,
//   324) -> BytesToInt64List (pkg/encoding/int_list.go:57) ->
//   BatchAggregation.Consume fold (pkg/query/vectorized/measure/
//   aggregation.go:310-351,464-486; pkg/query/aggregation/function.go).
//
// Design (CDNA4-first, not a translation):
//  * one 64-lane WAVE per (series,block) — 1.2M blocks at the benchmark
//    configs is ~150 blocks per wave slot at full occupancy; no intra-block
//    sync, no LDS;
//  * the varint stream (zigzag, 7-bit groups LSB-first, terminator = high
//    bit clear — pkg/encoding/int.go:81-148) decodes in 256-byte quad
//    windows: four bytes per lane from one u32 load, __ballot terminator
//    masks, up to four 1-2-byte values decoded per lane with one 32-bit
//    DPP scan per window (shfl compiles to ds_bpermute — an LDS op — so
//    the scans use DPP row_shr + v_readlane instead); wider varints fall
//    back to a 64-byte ballot window;
//  * SUM/COUNT need no prefix reconstruction at all: for delta streams
//    sum(v_i, i=r0..r1) = nsel*first + sum_j w_j * d_j with closed-form
//    weights, so the kernel does a weighted fold of raw deltas (exact mod
//    2^64 — Go int64 addition wraps identically);
//  * MIN/MAX (and float64 restore) reconstruct values with a wave-wide
//    inclusive scan (__shfl_up, 6 steps) — the reference's serial carry
//    chain (delta.go:45-117) becomes a parallel prefix sum;
//  * float64 columns stay in the decimal-int domain in-kernel (monotone
//    restore, float.go:69-102 applied at finalize); the mantissa sum is
//    carried per block into a double;
//  * per-block partials land in dense per-group accumulators with one
//    device-scope atomic set per wave per block (Guideline 12).
#include "../../include/bydb_gpu.h"

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#define WAVE 64

// exact powers of ten for per-block decimal-exponent rescale
__device__ __constant__ int64_t c_pow10i[19] = {
    1LL, 10LL, 100LL, 1000LL, 10000LL, 100000LL, 1000000LL, 10000000LL,
    100000000LL, 1000000000LL, 10000000000LL, 100000000000LL,
    1000000000000LL, 10000000000000LL, 100000000000000LL,
    1000000000000000LL, 10000000000000000LL, 100000000000000000LL,
    1000000000000000000LL};

// Plain (non-dictionary) tag columns — the >256-distinct-values fallback
// (column.go:266-278, dictionary.go:58) — are zstd-compressed on disk; the
// host normalizes them at part registration (encode.cpp) into a sidecar
// arena, flagged in the stored descriptor by the top offset bit.
#define TAG_SIDECAR_BIT (1ull << 63)
#define PLAIN_BM_WORDS 128  // bitmap words per block (8192 rows max)
bool bydb_normalize_plain_tag(const uint8_t *src, uint64_t src_len,
                              uint64_t nrows, std::vector<uint8_t> &out);
bool bydb_normalize_dict_tag(const uint8_t *src, uint64_t src_len,
                             bool *needed, std::vector<uint8_t> &out);
bool bydb_normalize_plain_field(const uint8_t *src, uint64_t src_len,
                                uint64_t nrows, std::vector<uint8_t> &out);

// ---------------- device helpers ----------------

__device__ __forceinline__ int64_t zz_dec(uint64_t u) {
    return (int64_t)(u >> 1) ^ -(int64_t)(u & 1);
}

__device__ __forceinline__ uint64_t lanemask_lt(int lane) {
    return (lane == 0) ? 0ull : (~0ull >> (64 - lane));
}

// DPP row-shift: pure-VALU lane shift within 16-lane rows (bound_ctrl
// zero-fills lanes whose source is outside the row).  __shfl_up compiles
// to ds_bpermute (an LDS op, ~40-cycle latency); a 6-step shfl scan is a
// dependent LDS chain that dominates the scan kernels' wait time, so the
// scans below use 4 DPP row_shr steps + v_readlane cross-row fixup —
// zero LDS traffic.
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_mov32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF,
                                                 true);
}

__device__ __forceinline__ uint64_t readlane64(uint64_t v, int l) {
    uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
    uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32),
                                                      l);
    return ((uint64_t)hi << 32) | lo;
}

// A value every lane of the wave holds alike, moved to scalar registers:
// what depends on it becomes scalar loads and wave-uniform branches.
__device__ __forceinline__ uint64_t wave_uniform64(uint64_t v) {
    uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    uint32_t hi =
        (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

// wave-wide inclusive scan of a u64 (wrapping adds)
__device__ __forceinline__ uint64_t wave_incl_scan(uint64_t v, int lane) {
#define BYDB_SCAN_STEP64(C)                                                  \
    {                                                                        \
        uint64_t t = ((uint64_t)dpp_mov32<C>((uint32_t)(v >> 32)) << 32) |   \
                     dpp_mov32<C>((uint32_t)v);                              \
        v += t;                                                              \
    }
    BYDB_SCAN_STEP64(0x111)   // row_shr:1
    BYDB_SCAN_STEP64(0x112)   // row_shr:2
    BYDB_SCAN_STEP64(0x114)   // row_shr:4
    BYDB_SCAN_STEP64(0x118)   // row_shr:8
#undef BYDB_SCAN_STEP64
    uint64_t s15 = readlane64(v, 15);
    uint64_t s31 = readlane64(v, 31);
    uint64_t s47 = readlane64(v, 47);
    // branchless: nested ternaries here compile to exec-mask branch
    // cascades; mask-ANDs keep it pure VALU
    int r = lane >> 4;
    uint64_t m1 = (uint64_t)-(int64_t)(r >= 1);
    uint64_t m2 = (uint64_t)-(int64_t)(r >= 2);
    uint64_t m3 = (uint64_t)-(int64_t)(r >= 3);
    return v + (s15 & m1) + (s31 & m2) + (s47 & m3);
}

// reductions, DPP-style like the scans: 4 row_shr steps leave each
// 16-lane row's total at its last lane; v_readlane combines the rows.
// All lanes return the wave total (as the shfl_xor butterfly did).
__device__ __forceinline__ uint64_t wave_reduce_add(uint64_t v) {
#define BYDB_RSTEP64(C)                                                      \
    {                                                                        \
        uint64_t t = ((uint64_t)dpp_mov32<C>((uint32_t)(v >> 32)) << 32) |   \
                     dpp_mov32<C>((uint32_t)v);                              \
        v += t;                                                              \
    }
    BYDB_RSTEP64(0x111) BYDB_RSTEP64(0x112)
    BYDB_RSTEP64(0x114) BYDB_RSTEP64(0x118)
#undef BYDB_RSTEP64
    return readlane64(v, 15) + readlane64(v, 31) + readlane64(v, 47) +
           readlane64(v, 63);
}

__device__ __forceinline__ double wave_reduce_addf(double v) {
    uint64_t u;
    __builtin_memcpy(&u, &v, 8);
#define BYDB_RSTEPF(C)                                                       \
    {                                                                        \
        uint64_t tb = ((uint64_t)dpp_mov32<C>((uint32_t)(u >> 32)) << 32) |  \
                      dpp_mov32<C>((uint32_t)u);                             \
        double t;                                                            \
        __builtin_memcpy(&t, &tb, 8);                                        \
        v += t;                                                              \
        __builtin_memcpy(&u, &v, 8);                                         \
    }
    BYDB_RSTEPF(0x111) BYDB_RSTEPF(0x112)
    BYDB_RSTEPF(0x114) BYDB_RSTEPF(0x118)
#undef BYDB_RSTEPF
    double a, b, c, d;
    uint64_t x;
    x = readlane64(u, 15); __builtin_memcpy(&a, &x, 8);
    x = readlane64(u, 31); __builtin_memcpy(&b, &x, 8);
    x = readlane64(u, 47); __builtin_memcpy(&c, &x, 8);
    x = readlane64(u, 63); __builtin_memcpy(&d, &x, 8);
    return a + b + c + d;
}

__device__ __forceinline__ int64_t wave_reduce_min(int64_t v) {
    // row_shr moves are zero-filled out of row; feed the identity by
    // selecting against the shifted VALIDITY instead: use bound_ctrl 0's
    // zero fill and compare via a mask-free trick — shift lanes carry a
    // zero, so compare only where the source lane exists (lane%16 >= off)
    const int lane15 = (int)(threadIdx.x & 15);
#define BYDB_RMIN(C, OFF)                                                    \
    {                                                                        \
        int64_t t = (int64_t)(((uint64_t)dpp_mov32<C>((uint32_t)((uint64_t)v >> 32)) << 32) | \
                              dpp_mov32<C>((uint32_t)(uint64_t)v));          \
        if (lane15 >= OFF && t < v) v = t;                                   \
    }
    BYDB_RMIN(0x111, 1) BYDB_RMIN(0x112, 2)
    BYDB_RMIN(0x114, 4) BYDB_RMIN(0x118, 8)
#undef BYDB_RMIN
    int64_t a = (int64_t)readlane64((uint64_t)v, 15);
    int64_t b = (int64_t)readlane64((uint64_t)v, 31);
    int64_t c = (int64_t)readlane64((uint64_t)v, 47);
    int64_t d = (int64_t)readlane64((uint64_t)v, 63);
    int64_t m = a < b ? a : b;
    m = c < m ? c : m;
    return d < m ? d : m;
}

__device__ __forceinline__ int64_t wave_reduce_max(int64_t v) {
    const int lane15 = (int)(threadIdx.x & 15);
#define BYDB_RMAX(C, OFF)                                                    \
    {                                                                        \
        int64_t t = (int64_t)(((uint64_t)dpp_mov32<C>((uint32_t)((uint64_t)v >> 32)) << 32) | \
                              dpp_mov32<C>((uint32_t)(uint64_t)v));          \
        if (lane15 >= OFF && t > v) v = t;                                   \
    }
    BYDB_RMAX(0x111, 1) BYDB_RMAX(0x112, 2)
    BYDB_RMAX(0x114, 4) BYDB_RMAX(0x118, 8)
#undef BYDB_RMAX
    int64_t a = (int64_t)readlane64((uint64_t)v, 15);
    int64_t b = (int64_t)readlane64((uint64_t)v, 31);
    int64_t c = (int64_t)readlane64((uint64_t)v, 47);
    int64_t d = (int64_t)readlane64((uint64_t)v, 63);
    int64_t m = a > b ? a : b;
    m = c > m ? c : m;
    return d > m ? d : m;
}

// Decode one varint serially starting at p (used for wave-uniform headers:
// the DeltaConst stride and the delta-of-delta d1 — every lane runs the
// same loop on the same bytes, so the result is wave-uniform).
__device__ __forceinline__ int64_t decode_one_varint(const uint8_t *p, int *len) {
    uint8_t c = p[0];
    if (c < 0x80) { *len = 1; return zz_dec(c); }
    uint64_t u = (uint64_t)(c & 0x7f);
    int i = 1;
    unsigned shift = 0;
    while (c >= 0x80 && i <= 10) {
        c = p[i++];
        shift += 7;
        u |= (uint64_t)(c & 0x7f) << shift;
    }
    *len = i;
    return zz_dec(u);
}

// Triangular number T(m) = m(m+1)/2 for m <= 8192 (fits u32 domain widely).
__device__ __forceinline__ uint64_t tri(uint64_t m) { return m * (m + 1) / 2; }

struct DevErr {
    unsigned code;      // first error code seen (atomicCAS)
    unsigned block_lo;  // low 32 bits of the offending block index
};

enum {
    DERR_NONE = 0,
    DERR_BAD_STREAM = 1,    // no terminator in a 64-byte window
    DERR_BAD_ENC = 2,       // unsupported encode type in kernel
    DERR_DESC_TS = 3,       // descending timestamps (reference never writes them)
    DERR_GROUP_RANGE = 4,   // block group_code >= configured n_groups
    DERR_F64_SUM_OVF = 6,   // float64 block mantissa sum would exceed int64
    DERR_EXP_MISMATCH = 5,  // float64 block's decimal exponent differs from
                            // the configured session exponent (per-block
                            // rescale is a later row; silent mixing would
                            // corrupt sums and make min/max incomparable)
    DERR_TOP_NULL = 7,      // a top-rows consume selected a row of a
                            // null-bearing (Plain) field block
};

__device__ __forceinline__ void dev_set_err(DevErr *e, unsigned code, uint64_t bi) {
    if (atomicCAS(&e->code, DERR_NONE, code) == DERR_NONE)
        e->block_lo = (unsigned)bi;
}

// ---------------- per-block decode primitives ----------------

// ---- dense all-1-byte delta fold ----
// When the stream length equals the delta count, every varint is one byte
// (int.go:84-88), so the stream IS the zigzag byte array and the weighted
// fold becomes dense byte math: per dword, SWAR zigzag
// (d = (b>>1) ^ (-(b&1) as 0x00/0xff)) turns 4 bytes into 4 signed i8
// lanes, and v_dot4_i32_i8 folds them against {1,1,1,1} / {0,1,2,3}
// weights.  Per-lane accumulators stay in int32 for a whole block
// (<= 144 bytes/lane * |d| <= 64 * byte index <= 8205 is about 7.6e7,
// far below 2^31; see dense_region_t for the batched form).
__device__ __forceinline__ int32_t dot4_i8(uint32_t a, uint32_t b, int32_t c) {
#if defined(__gfx950__) || defined(__AMDGCN__)
    return __builtin_amdgcn_sdot4((int)a, (int)b, c, false);
#else
    int32_t r = c;
    for (int k = 0; k < 4; k++)
        r += (int32_t)(int8_t)(a >> (8 * k)) * (int32_t)(int8_t)(b >> (8 * k));
    return r;
#endif
}

__device__ __forceinline__ uint32_t swar_zigzag(uint32_t w) {
    uint32_t mag = (w >> 1) & 0x7f7f7f7fu;
    uint32_t sgn = w & 0x01010101u;
    return mag ^ (sgn * 0xffu);  // per-byte signed i8 delta
}

// The same decode without the quarter-rate 32-bit multiply, for the
// dense fold: 0x80 - {0,1} = {0x80,0x7f} borrows nothing across bytes,
// and ^ 0x80 turns that into the per-byte {0x00,0xff} sign mask.
__device__ __forceinline__ uint32_t swar_zigzag_sub(uint32_t w) {
    uint32_t mag = (w >> 1) & 0x7f7f7f7fu;
    uint32_t sgn = w & 0x01010101u;
    uint32_t neg = (0x80808080u - sgn) ^ 0x80808080u;
    return mag ^ neg;
}

// The payload arena is device (global) memory; saying so on the pointer
// keeps the dense loads global_load_dwordx4 even where the fold is not
// inlined into the kernel and `stream` arrives as a generic pointer.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) u32x4 *gptr_u4;

// A dense chunk is 1 KiB: 16 bytes per lane, one wave load instruction.
// A block's stream (<= 8191 bytes) plus its <= 15-byte head offset spans
// at most DENSE_CHUNKS_BLOCK of them.
#define DENSE_CHUNK_BYTES 1024
#define DENSE_CHUNKS_BLOCK 9
// The clamped closed-form instantiation carries the FindRange state next
// to the fold: with nine chunks in flight it spills 12 bytes, with five
// it has no scratch (108 VGPRs); a clamped block then takes two batches.
#define DENSE_CHUNKS_CLAMP 5
// Batch depth of the out-of-line fold that the value-scan instantiations
// and fold_range call: two chunks keep it inside the registers a device
// function may clobber without saving them, so those callers gain no
// scratch (three already cost fold_range 8 bytes, four cost 28-36).
#define DENSE_CHUNKS_CALL 2

// Byte-lane keep mask of the dword at chunk-relative offset r: 0xff for
// the bytes whose offset lies in [lo_rel, hi_rel), 0 for the rest.  A
// zeroed byte zigzag-decodes to delta 0 and adds nothing to either sum.
__device__ __forceinline__ uint32_t dense_keep(int32_t r, int32_t lo_rel,
                                               int32_t hi_rel) {
    int32_t a = lo_rel - r, b = hi_rel - r;
    a = a < 0 ? 0 : a > 4 ? 4 : a;   // bytes dropped at the low end
    b = b < 0 ? 0 : b > 4 ? 4 : b;   // bytes kept from the low end
    uint32_t m_hi = (uint32_t)((1ull << (8 * b)) - 1ull);
    uint32_t m_lo = (uint32_t)(0xffffffffull << (8 * a));
    return m_hi & m_lo;
}

// Fold one lane's 16 bytes: T = sum of the 16 deltas, K = sum of
// (byte offset within the 16) * delta.
__device__ __forceinline__ void dense_fold16(u32x4 w, int32_t *T, int32_t *K) {
    uint32_t s0 = swar_zigzag_sub(w.x), s1 = swar_zigzag_sub(w.y),
             s2 = swar_zigzag_sub(w.z), s3 = swar_zigzag_sub(w.w);
    *T = dot4_i8(s0, 0x01010101u, dot4_i8(s1, 0x01010101u,
         dot4_i8(s2, 0x01010101u, dot4_i8(s3, 0x01010101u, 0))));
    *K = dot4_i8(s0, 0x03020100u, dot4_i8(s1, 0x07060504u,
         dot4_i8(s2, 0x0b0a0908u, dot4_i8(s3, 0x0f0e0d0cu, 0))));
}

// Fold Sum(d_j) and Sum(bidx*d_j) over stream bytes bidx in [lo, hi)
// (delta j = bidx+1).  lo, hi and stream MUST be wave-uniform: they are
// taken from the first active lane, so a caller with per-lane ranges
// would get that lane's sums in every lane.  The region is read as
// 1-KiB chunks of 16 bytes per lane, starting at the 16-byte boundary at
// or below stream+lo; bytes outside [lo, hi) are zeroed in registers, so
// only the first and the last chunk are masked and nothing is folded by
// a single lane.  Chunks go in batches of NB, and all chunks of a batch
// are issued before the first is folded.  With NB = DENSE_CHUNKS_BLOCK a
// block is one batch: one memory round trip per block, and a full-length
// block folds under counted waits while its later chunks arrive.
// A chunk is issued only if it starts before hi (the last one only for
// the lanes that do), so the over-read stays below one chunk past hi —
// inside the arena's zeroed 4-KiB slack.
// Per-lane accumulators stay in int32 for a whole batch: with NB = 9,
// <= 144 bytes/lane * |d| <= 64 * batch-relative offset <= 9215 is about
// 8.5e7 < 2^31; the batch base is applied in int64.
// NT: the chunk loads are non-temporal (global_load_dwordx4 ... nt).  For
// a pass over more payload than the last-level cache holds, every line is
// read once and installing it in the caches only evicts what could still
// be reused; a part that fits is served from that cache pass after pass
// and keeps the plain loads (see bydb_stream_policy_pick).
template <int NB, bool NT>
__device__ __forceinline__ void dense_region_t(
    const uint8_t *stream, int64_t lo, int64_t hi, int lane,
    int64_t *out_sum_d, int64_t *out_sum_jd) {
    *out_sum_d = 0;
    *out_sum_jd = 0;
    lo = (int64_t)wave_uniform64((uint64_t)lo);
    hi = (int64_t)wave_uniform64((uint64_t)hi);
    if (hi <= lo) return;
    // the integer value of the pointer serves the alignment only
    const uint32_t mis = (uint32_t)__builtin_amdgcn_readfirstlane(
                             (int)((uint32_t)(uintptr_t)stream + (uint32_t)lo)) & 15u;
    int64_t a0 = lo - (int64_t)mis;
    int64_t sum_d = 0, sum_jd = 0;
    const int32_t lane_off = lane * 16;
    do {
        const gptr_u4 p = (gptr_u4)(stream + a0) + lane;
        const int64_t span = hi - a0;
        const int32_t hi_rel = span > NB * DENSE_CHUNK_BYTES
                                   ? NB * DENSE_CHUNK_BYTES
                                   : (int32_t)span;
        const int32_t lo_rel = lo > a0 ? (int32_t)(lo - a0) : 0;
        const int nch = (hi_rel + DENSE_CHUNK_BYTES - 1) / DENSE_CHUNK_BYTES;
        int32_t acc_d = 0, acc_c = 0, acc_k = 0;
        auto load = [&](int c) -> u32x4 {
            return NT ? __builtin_nontemporal_load(p + c * 64) : p[c * 64];
        };
        auto fold = [&](int c, u32x4 v, bool may_mask) {
            if (may_mask && ((c == 0 && lo_rel > 0) ||
                             (c + 1) * DENSE_CHUNK_BYTES > hi_rel)) {
                int32_t r = c * DENSE_CHUNK_BYTES + lane_off;
                v.x &= dense_keep(r, lo_rel, hi_rel);
                v.y &= dense_keep(r + 4, lo_rel, hi_rel);
                v.z &= dense_keep(r + 8, lo_rel, hi_rel);
                v.w &= dense_keep(r + 12, lo_rel, hi_rel);
            }
            int32_t T, K;
            dense_fold16(v, &T, &K);
            acc_d += T;
            acc_c += __mul24(c, T);   // |T| <= 16 * 64: full-rate 24-bit mad
            acc_k += K;
        };
        u32x4 w[NB];
        if (nch >= NB - 1) {
            // full batch: NB-1 unconditional loads back to back, the last
            // chunk only for the lanes that still start before hi; only
            // chunk 0 (head) and chunk NB-2 (tail) can need a mask here,
            // chunk NB-1 is folded below and always takes the tail mask
#pragma unroll
            for (int c = 0; c < NB - 1; c++) w[c] = load(c);
            w[NB - 1] = u32x4{0, 0, 0, 0};
            if ((NB - 1) * DENSE_CHUNK_BYTES + lane_off < hi_rel)
                w[NB - 1] = load(NB - 1);
#pragma unroll
            for (int c = 0; c < NB - 1; c++) {
                fold(c, w[c], c == 0 || c == NB - 2);
                // Keep the folds in issue order.  Left alone, the folds
                // sink below the tail-mask branch and the scheduler
                // starts with a late chunk, so the first wait covers most
                // of the batch.  The empty statement pins the running
                // sums after chunk c; the barrier stops the scheduler
                // from moving a later chunk's math above it.
                asm volatile("" : "+v"(acc_d), "+v"(acc_c), "+v"(acc_k));
                __builtin_amdgcn_sched_barrier(0);
            }
            if (nch > NB - 1) fold(NB - 1, w[NB - 1], true);
        } else {
            // short region: issue only the chunks (and lanes) that start
            // before hi, then fold them after a single wait
#pragma unroll
            for (int c = 0; c < NB - 2; c++) {
                w[c] = u32x4{0, 0, 0, 0};
                if (c * DENSE_CHUNK_BYTES + lane_off < hi_rel)
                    w[c] = load(c);
            }
#pragma unroll
            for (int c = 0; c < NB - 2; c++)
                if (nch > c) fold(c, w[c], true);
        }
        int32_t rel = lane_off * acc_d + DENSE_CHUNK_BYTES * acc_c + acc_k;
        sum_d += (int64_t)acc_d;
        sum_jd += a0 * (int64_t)acc_d + (int64_t)rel;
        a0 += NB * DENSE_CHUNK_BYTES;
    } while (a0 < hi);
    *out_sum_d = sum_d;
    *out_sum_jd = sum_jd;
}

__device__ void dense_region(const uint8_t *stream, int64_t lo, int64_t hi,
                             int lane, int64_t *out_sum_d, int64_t *out_sum_jd) {
    dense_region_t<DENSE_CHUNKS_CALL, false>(stream, lo, hi, lane, out_sum_d,
                                             out_sum_jd);
}

// ---- nibble-packed dense delta fold ----
// A dense block whose deltas all lie in [-8, 7] has a 4-bit copy in the
// packed arena (pack_build): nibble p of the slot (byte p/2, low nibble
// first) holds delta p+1 biased by 8, and every nibble from the block's
// last delta to the slot's end holds 8, that is delta 0.  A slot is a
// multiple of 128 bytes on a 128-byte boundary, so the fold reads whole
// 16-byte lane units and masks nothing.
#define PACK_SLOT_ALIGN 128
#define PACK_CHUNKS_BLOCK 4     // 8191 nibbles are exactly four 1-KiB chunks
#define PACK_MAX_ROWS 8192
#define PACK_PAD_WORD 0x88888888u

__host__ __device__ __forceinline__ uint32_t pack_slot_bytes(uint32_t count) {
    return (count / 2 + (PACK_SLOT_ALIGN - 1)) & ~(uint32_t)(PACK_SLOT_ALIGN - 1);
}

// Fold one lane's 16 bytes = 32 nibbles: T = sum of the 32 deltas, K = sum
// of (nibble position within the 32) * delta.  Two masks split a dword into
// its even and odd nibbles as byte lanes; the biased nibbles (0..15) and the
// position weights (0..31) are non-negative i8, so the signed dot4 folds
// them as they are, and the bias leaves through the accumulators' start
// values: 32 * 8 for T, 8 * (0 + 1 + ... + 31) for K.  The eight nibble
// lanes of one byte position sum to <= 120, so T takes a single dot4.
__device__ __forceinline__ void packed_fold16(u32x4 w, int32_t *T, int32_t *K) {
    const uint32_t m = 0x0f0f0f0fu;
    uint32_t e0 = w.x & m, o0 = (w.x >> 4) & m, e1 = w.y & m, o1 = (w.y >> 4) & m,
             e2 = w.z & m, o2 = (w.z >> 4) & m, e3 = w.w & m, o3 = (w.w >> 4) & m;
    *T = dot4_i8(((e0 + o0) + (e1 + o1)) + ((e2 + o2) + (e3 + o3)),
                 0x01010101u, -32 * 8);
    *K = dot4_i8(e0, 0x06040200u, dot4_i8(o0, 0x07050301u,
         dot4_i8(e1, 0x0e0c0a08u, dot4_i8(o1, 0x0f0d0b09u,
         dot4_i8(e2, 0x16141210u, dot4_i8(o2, 0x17151311u,
         dot4_i8(e3, 0x1e1c1a18u, dot4_i8(o3, 0x1f1d1b19u, -8 * 496))))))));
}

// Sum(d_j) and Sum(p * d_j) over a whole block's slot (delta j at nibble
// p = j - 1), per lane: the caller reduces.  n_rows must be wave-uniform.
// The loads are non-temporal (only the streaming instantiations come here)
// and, as in dense_region_t, all of a block's chunks are issued before the
// first is folded; a full-length block folds under counted waits.  Only the
// lanes whose 16 bytes lie inside the slot load, so nothing is read past it.
// int32 per lane: 128 nibbles * |d| <= 8 * position <= 8191 is about 8.4e6.
__device__ __forceinline__ void dense_region_packed(
    const uint8_t *slot, uint32_t n_rows, int lane, int64_t *out_sum_d,
    int64_t *out_sum_pd) {
    const int32_t slot_bytes = (int32_t)pack_slot_bytes(n_rows);
    const gptr_u4 p = (gptr_u4)slot + lane;
    const int32_t lane_off = lane * 16;
    int32_t acc_d = 0, acc_c = 0, acc_k = 0;
    auto fold = [&](int c, u32x4 v) {
        int32_t T, K;
        packed_fold16(v, &T, &K);
        acc_d += T;
        acc_c += __mul24(c, T);
        acc_k += K;
    };
    u32x4 w[PACK_CHUNKS_BLOCK];
    if (slot_bytes == PACK_CHUNKS_BLOCK * DENSE_CHUNK_BYTES) {
#pragma unroll
        for (int c = 0; c < PACK_CHUNKS_BLOCK; c++)
            w[c] = __builtin_nontemporal_load(p + c * 64);
#pragma unroll
        for (int c = 0; c < PACK_CHUNKS_BLOCK; c++) {
            fold(c, w[c]);
            // keep the folds in issue order (see dense_region_t)
            asm volatile("" : "+v"(acc_d), "+v"(acc_c), "+v"(acc_k));
            __builtin_amdgcn_sched_barrier(0);
        }
    } else {
#pragma unroll
        for (int c = 0; c < PACK_CHUNKS_BLOCK; c++) {
            w[c] = u32x4{PACK_PAD_WORD, PACK_PAD_WORD, PACK_PAD_WORD,
                         PACK_PAD_WORD};
            if (c * DENSE_CHUNK_BYTES + lane_off < slot_bytes)
                w[c] = __builtin_nontemporal_load(p + c * 64);
        }
#pragma unroll
        for (int c = 0; c < PACK_CHUNKS_BLOCK; c++)
            if (c * DENSE_CHUNK_BYTES < slot_bytes) fold(c, w[c]);
    }
    *out_sum_d = (int64_t)acc_d;
    *out_sum_pd = (int64_t)(2 * lane_off * acc_d +
                            2 * DENSE_CHUNK_BYTES * acc_c + acc_k);
}

// The whole-block weighted fold over a slot: delta j = p + 1 of an n-row
// block weighs n - j = n - 1 - p (dense_delta_weighted_t with r0 = 0,
// r1 = n - 1).
__device__ __forceinline__ uint64_t dense_packed_weighted(const uint8_t *slot,
                                                          uint32_t n_rows,
                                                          int lane) {
    int64_t sd, spd;
    dense_region_packed(slot, n_rows, lane, &sd, &spd);
    return (uint64_t)(n_rows - 1) * (uint64_t)sd - (uint64_t)spd;
}

// wave-wide inclusive scan of an int32 (per-window lane sums)
// row-masked DPP: rows outside ROWMASK receive `old` = 0, so `v += ...`
// is a no-op there — the canonical GCN cross-row scan combine.
template <int CTRL, int ROWMASK>
__device__ __forceinline__ uint32_t dpp_mov32_rm(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWMASK,
                                                 0xF, true);
}

__device__ __forceinline__ int32_t wave_incl_scan32(int32_t v, int lane) {
    v += (int32_t)dpp_mov32<0x111>((uint32_t)v);
    v += (int32_t)dpp_mov32<0x112>((uint32_t)v);
    v += (int32_t)dpp_mov32<0x114>((uint32_t)v);
    v += (int32_t)dpp_mov32<0x118>((uint32_t)v);
    // cross-row combine via row broadcasts instead of three readlanes +
    // masked adds: row_bcast15 adds lane 15 into row 1 and lane 47 into
    // row 3; row_bcast31 then adds lane 31 (= rows 0+1 total) into rows
    // 2 and 3 — two DPP ops, no SALU round trips
    v += (int32_t)dpp_mov32_rm<0x142, 0xa>((uint32_t)v);  // ROW_BCAST15
    v += (int32_t)dpp_mov32_rm<0x143, 0xc>((uint32_t)v);  // ROW_BCAST31
    (void)lane;
    return v;
}

// Dense min/max over an all-1-byte delta stream: fold min/max of the
// values v_j for delta bytes b in [b_lo, b_hi) (v after applying byte b),
// with base_val = v at delta index b_lo (carry-in).  256-byte windows,
// SWAR zigzag, per-window lane-sum scan — replaces the latency-chained
// 64-byte ballot scan for the dominant stream shape.
__device__ void dense_minmax(const uint8_t *stream, int64_t b_lo, int64_t b_hi,
                             int64_t base_val, int lane, int64_t *out_mn,
                             int64_t *out_mx) {
    int64_t lmn = INT64_MAX, lmx = INT64_MIN;
    if (b_hi > b_lo) {
        const uint32_t *wp =
            (const uint32_t *)((uintptr_t)(stream + b_lo) & ~(uintptr_t)3);
        int64_t wbase = (int64_t)((uintptr_t)wp - (uintptr_t)stream);
        uint64_t carry = (uint64_t)base_val;  // wrap-safe (Go int64 wraps)
        uint32_t w = wp[lane];
        while (wbase < b_hi) {
            uint32_t w_nxt = wp[64 + lane];   // next window, one ahead
            uint32_t sb = swar_zigzag(w);
            // mask bytes outside [b_lo, b_hi): zero their deltas and skip fold
            int64_t g0 = wbase + 4 * lane;
            uint32_t keep = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                int64_t g = g0 + k;
                if (g >= b_lo && g < b_hi) keep |= 0xffu << (8 * k);
            }
            sb &= keep;
            int32_t t = dot4_i8(sb, 0x01010101u, 0);
            int32_t incl = wave_incl_scan32(t, lane);
            uint64_t lane_base = carry + (uint64_t)(int64_t)(incl - t);
            int32_t cum = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                int32_t d = (int32_t)(int8_t)(sb >> (8 * k));
                cum += d;
                int64_t g = g0 + k;
                if (g >= b_lo && g < b_hi) {
                    int64_t v = (int64_t)(lane_base + (uint64_t)(int64_t)cum);
                    lmn = v < lmn ? v : lmn;
                    lmx = v > lmx ? v : lmx;
                }
            }
            carry += (uint64_t)(int64_t)__builtin_amdgcn_readlane(incl, 63);
            wp += 64;
            wbase += 256;
            w = w_nxt;
        }
    }
    *out_mn = wave_reduce_min(lmn);
    *out_mx = wave_reduce_max(lmx);
}

// Weighted fold over an all-1-byte delta stream:
//   sum_{j=1..jend} d_j * w(j),  w(j) = nsel (j<=r0) | r1-j+1 (else)
// via two dense regions (delta j lives at byte j-1):
//   region1 bytes [0, min(r0,jend)):          contributes nsel * S1d
//   region2 bytes [min(r0,jend), jend):       contributes (r1+1)*S2d - S2jd'
// where S2jd' uses delta index j = bidx+1.
template <int NB, bool NT>
__device__ __forceinline__ uint64_t dense_delta_weighted_t(
    const uint8_t *stream, int64_t n_deltas, int64_t r0, int64_t r1,
    int lane) {
    int64_t jend = r1 < n_deltas ? r1 : n_deltas;
    if (jend < 1) return 0;
    uint64_t nsel = (uint64_t)(r1 - r0 + 1);
    int64_t b1 = r0 < jend ? r0 : jend;  // deltas 1..b1 have weight nsel
    int64_t s1d = 0, s1jd = 0, s2d, s2jd;
    // whole-range queries have r0 == 0: no constant-weight region to read
    if (b1 > 0) dense_region_t<NB, NT>(stream, 0, b1, lane, &s1d, &s1jd);
    dense_region_t<NB, NT>(stream, b1, jend, lane, &s2d, &s2jd);
    // j = bidx + 1  =>  sum j*d = sum bidx*d + sum d
    uint64_t sum_jd2 = (uint64_t)s2jd + (uint64_t)s2d;
    uint64_t acc = nsel * (uint64_t)s1d;
    acc += (uint64_t)(r1 + 1) * (uint64_t)s2d - sum_jd2;
    return acc;
}

__device__ uint64_t dense_delta_weighted(const uint8_t *stream,
                                         int64_t n_deltas, int64_t r0,
                                         int64_t r1, int lane) {
    return dense_delta_weighted_t<DENSE_CHUNKS_CALL, false>(stream, n_deltas,
                                                            r0, r1, lane);
}

// The delta that ends at a terminator lane of the 64-byte window at `win`
// (b: the lane's own byte), for windows that START on a varint: the groups
// below the terminator are re-read from memory.
__device__ __forceinline__ int64_t varint_reread(const uint8_t *win,
                                                 uint64_t emask, uint8_t b,
                                                 int lane) {
    uint64_t below = emask & lanemask_lt(lane);
    int start = below ? (64 - __clzll(below)) : 0;
    uint64_t u = 0;
    unsigned sh = 0;
    for (int i = start; i < lane; ++i) {
        u |= (uint64_t)(win[i] & 0x7f) << sh;
        sh += 7;
    }
    u |= (uint64_t)b << sh;
    return zz_dec(u);
}

// Fast weighted delta fold: 256-byte windows (one dword per lane) with an
// all-1-byte fast case — the dominant shape for delta-encoded telemetry
// (zigzag deltas < 64 encode to one byte, int.go:84-88).  For a window
// fully inside the linear-weight region (j > r0, tail within [.., jend]),
//   sum d_j * (r1 - j + 1) = (r1+1) * S1 - S2,  S1 = sum d_j, S2 = sum j*d_j
// so the per-value work is 32-bit byte math folded into two lane
// accumulators.  Windows with multi-byte varints or boundary weights fall
// back to one 64-byte ballot step (exact same semantics), then resume.
// The next window's dwords are loaded before the current one is processed
// (the fast path's advance is a compile-time +256), hiding HBM latency.
// Inlined into its one caller, fold_rows, like fold_dod_weighted below: as
// calls they cost the clamped value-scan light pass 64 bytes of scratch.
__device__ __forceinline__ uint64_t fold_delta_weighted_fast(const uint8_t *stream,
                                             int64_t n_deltas, int64_t r0,
                                             int64_t r1, int lane, DevErr *derr,
                                             uint64_t bi) {
    uint64_t gen_acc = 0;   // generic-weight accumulator (boundary/slow)
    uint64_t s1 = 0;        // sum of d_j  (linear region)
    uint64_t s2 = 0;        // sum of j*d_j (linear region)
    uint64_t pos = 0;
    int64_t j = 1;
    int64_t jend = r1 < n_deltas ? r1 : n_deltas;
    uint64_t nsel = (uint64_t)(r1 - r0 + 1);
    // 256-byte windows at 4-byte-aligned absolute addresses; `off` is the
    // unconsumed-prefix length (bytes before the next value start).
    // (aligned down by pointer arithmetic, not through an integer, so the
    // window loads stay in the global address space)
    unsigned off = (unsigned)((uintptr_t)(stream + pos) & 3);
    const uint32_t *wp = (const uint32_t *)(stream + pos - off);
    uint32_t w = wp[lane];
    while (j <= jend) {
        uint32_t w_next = wp[64 + lane];               // prefetch next window
        uint32_t valid = (lane == 0 && off) ? (0xFFFFFFFFu << (8 * off))
                                            : 0xFFFFFFFFu;
        uint32_t want = 0x80808080u & valid;
        bool all_term = ((~w) & want) == want;
        int64_t nvals_window = 256 - (int64_t)off;
        bool fast = __all(all_term) && (jend - j + 1) >= nvals_window;
        if (fast) {
            bool linear = j > r0;   // whole window past the r0 boundary
            int32_t sum_d = 0, sum_kd = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                int32_t bidx = 4 * lane + k;
                uint32_t b = (w >> (8 * k)) & 0xffu;
                int32_t d = (int32_t)(b >> 1) ^ -(int32_t)(b & 1);
                if ((unsigned)bidx < off) d = 0;       // lane-0 masked prefix
                if (linear) {
                    sum_d += d;
                    sum_kd += (bidx - (int32_t)off) * d;
                } else {
                    int64_t myj = j + (bidx - (int64_t)off);
                    uint64_t wt = myj <= r0 ? nsel : (uint64_t)(r1 - myj + 1);
                    if ((unsigned)bidx >= off)
                        gen_acc += (uint64_t)(int64_t)d * wt;
                }
            }
            if (linear) {
                s1 += (uint64_t)(int64_t)sum_d;
                s2 += (uint64_t)j * (uint64_t)(int64_t)sum_d +
                      (uint64_t)(int64_t)sum_kd;
            }
            pos += (uint64_t)nvals_window;
            j += nvals_window;
            wp += 64;
            off = 0;
            w = w_next;
            continue;
        }
        // slow step: one 64-byte ballot window from pos (multi-byte
        // varints and/or the stream tail) — identical semantics to v1
        {
            uint8_t b = stream[pos + (uint64_t)lane];
            uint64_t emask = __ballot(b < 0x80);
            if (emask == 0) { dev_set_err(derr, DERR_BAD_STREAM, bi); break; }
            int rank = __popcll(emask & lanemask_lt(lane));
            int64_t myj = j + rank;
            bool is_term = (b < 0x80) && (myj <= jend);
            // <=2-byte window fast case: decode via the left neighbour,
            // no backward byte loop, no 64-bit bookkeeping
            uint64_t cont2 = ~emask;
            if ((cont2 & (cont2 << 1)) == 0 &&
                (int64_t)__popcll(emask) <= jend - j + 1) {
                uint32_t prevb = (uint32_t)__shfl_up((int)b, 1);
                bool is2b = lane > 0 && (prevb & 0x80u);
                uint32_t u2 = is2b ? ((prevb & 0x7fu) | ((uint32_t)b << 7))
                                   : (uint32_t)b;
                int32_t d32 = (int32_t)(u2 >> 1) ^ -(int32_t)(u2 & 1);
                if (b < 0x80) {
                    uint64_t wt = myj <= r0 ? nsel : (uint64_t)(r1 - myj + 1);
                    gen_acc += (uint64_t)(int64_t)d32 * wt;
                }
                int ll2 = 63 - __clzll(emask);
                int nterm2 = __popcll(emask);
                if (j + nterm2 > jend) { j = jend + 1; break; }
                j += nterm2;
                pos += (uint64_t)(ll2 + 1);
                off = (unsigned)((uintptr_t)(stream + pos) & 3);
                wp = (const uint32_t *)(stream + pos - off);
                w = wp[lane];
                continue;
            }
            int64_t d;
            if (emask == ~0ull) {
                d = zz_dec(b);
            } else if (is_term) {
                d = varint_reread(stream + pos, emask, b, lane);
            } else {
                d = 0;
            }
            if (is_term) {
                uint64_t wt = myj <= r0 ? nsel : (uint64_t)(r1 - myj + 1);
                gen_acc += (uint64_t)d * wt;
            }
            int nterm = __popcll(emask);
            if (j + nterm > jend) { j = jend + 1; break; }
            j += nterm;
            pos += (uint64_t)(64 - __clzll(emask));
            off = (unsigned)((uintptr_t)(stream + pos) & 3);
            wp = (const uint32_t *)(stream + pos - off);
            w = wp[lane];
        }
    }
    // fold the linear region: sum d_j*(r1-j+1) = (r1+1)*S1 - S2 (mod 2^64)
    return gen_acc + (uint64_t)(r1 + 1) * s1 - s2;
}

// Weighted delta-of-delta fold: sum_{i=r0..r1} v_i with
//   v_i = first + i*d1 + sum_{k=2..i} d2_k * (i-k+1)
// => contribution of d2_k (k in [2, r1]):  W_k = T(r1-k+1) - T(max(k,r0)-k).
__device__ __forceinline__ uint64_t fold_dod_weighted(const uint8_t *stream, int64_t n_deltas,
                                      int64_t r0, int64_t r1, int lane,
                                      DevErr *derr, uint64_t bi) {
    uint64_t acc = 0;
    uint64_t pos = 0;
    int64_t k = 2;                       // d2 indices run 2..n-1
    int64_t kend = r1 < n_deltas ? r1 : n_deltas;
    while (k <= kend) {
        uint8_t b = stream[pos + (uint64_t)lane];
        uint64_t emask = __ballot(b < 0x80);
        if (emask == 0) { dev_set_err(derr, DERR_BAD_STREAM, bi); return acc; }
        int rank = __popcll(emask & lanemask_lt(lane));
        int64_t myk = k + rank;
        bool is_term = (b < 0x80) && (myk <= kend);
        int64_t d;
        if (emask == ~0ull) {
            d = zz_dec(b);
        } else if (is_term) {
            d = varint_reread(stream + pos, emask, b, lane);
        } else {
            d = 0;
        }
        if (is_term) {
            int64_t a = myk > r0 ? myk : r0;
            uint64_t w = tri((uint64_t)(r1 - myk + 1)) - tri((uint64_t)(a - myk));
            acc += (uint64_t)d * w;
        }
        int nterm = __popcll(emask);
        if (k + nterm > kend) break;
        k += nterm;
        pos += (uint64_t)(64 - __clzll(emask));
    }
    return acc;
}

// ---------------- tag predicate (dictionary codes) ----------------
// The reference evaluates tag-equality predicates on decoded tag values
// per row (vec scan/filter; tags are dictionary-encoded per block,
// column.go:266-278, dictionary.go:79-115).  Here a resolve prepass maps
// the predicate value to a per-block CODE mask by comparing it against the
// block's dictionary values, and the scan walks the block's bit-packed RLE
// code runs (dictionary.go:158-260) to test rows — codes only, the value
// bytes are never expanded per row.

struct PredBlock {
    uint64_t mask[4];      // bit c: dict code c equals the predicate value
    uint64_t rle_bit_off;  // absolute bit offset of packed RLE entries
    uint32_t nentries;     // packed entry count (2 per run: value, count)
    uint8_t width;         // bits per packed entry
    uint8_t active;        // block has a tag column on this slot
    uint8_t err;           // unparseable on device -> error
    uint8_t uniform;       // single run covers the whole block
    uint8_t plain;         // plain (non-dictionary) column: rle_bit_off is
                           // the per-row match-bitmap WORD offset instead
    uint8_t disabled;      // slot carries no predicate (empty value)
};

// MSB-first bit read at an arbitrary bit offset (reader.go:39-79 order);
// n <= 32, so 8 gathered bytes always cover shift+n.
__device__ __forceinline__ uint64_t rd_bits_be(const uint8_t *p,
                                               uint64_t bitpos, uint32_t n) {
    uint64_t byte = bitpos >> 3;
    uint32_t sh = (uint32_t)(bitpos & 7);
    uint64_t acc = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) acc = (acc << 8) | p[byte + (uint64_t)i];
    return (acc >> (64 - sh - n)) & ((1ull << n) - 1);
}

// compress_block section header inside a dictionary stream: [0][u8 len]
// plain (<128 B, bytes.go:291-295) or [2][u32le len] raw — the framing the
// host normalization writes after decompressing a zstd'd section.  Returns
// the section start, or nullptr on an unparseable marker (zstd reaching
// the device unnormalized).
__device__ __forceinline__ const uint8_t *dict_section(const uint8_t *p,
                                                       const uint8_t *end,
                                                       uint64_t *len_out) {
    if (p >= end) return nullptr;
    if (*p == 0) {
        if (p + 2 > end) return nullptr;
        *len_out = p[1];
        return p + 2;
    }
    if (*p == 2) {
        if (p + 5 > end) return nullptr;
        *len_out = (uint64_t)p[1] | ((uint64_t)p[2] << 8) |
                   ((uint64_t)p[3] << 16) | ((uint64_t)p[4] << 24);
        return p + 5;
    }
    return nullptr;
}

struct PredWalk {
    const uint8_t *payload;
    const uint64_t *bm;        // plain columns: per-row match bitmap (O(1))
    uint64_t bit0;
    uint32_t nentries, width;
    uint64_t mask[4];
    uint32_t entry;            // next entry index (2 per run)
    int64_t run_lo, run_hi;    // rows [run_lo, run_hi) of the current run
    bool run_match;
};

__device__ __forceinline__ void pred_init(PredWalk *pw, const uint8_t *payload,
                                          const uint8_t *sidecar,
                                          const PredBlock *pb,
                                          const uint64_t *bm_arena) {
    // bit 63 of rle_bit_off: the dictionary stream was host-normalized
    // into the sidecar arena (zstd'd sections); offsets are sidecar-based
    pw->payload = (pb->rle_bit_off & TAG_SIDECAR_BIT) ? sidecar : payload;
    pw->bm = pb->plain ? bm_arena + pb->rle_bit_off : nullptr;
    pw->bit0 = pb->rle_bit_off & ~TAG_SIDECAR_BIT;
    pw->nentries = pb->nentries;
    pw->width = pb->width;
#pragma unroll
    for (int i = 0; i < 4; i++) pw->mask[i] = pb->mask[i];
    pw->entry = 0;
    pw->run_lo = 0;
    pw->run_hi = 0;
    pw->run_match = false;
}

__device__ __forceinline__ void pred_advance(PredWalk *pw) {
    if (pw->entry + 1 >= pw->nentries) {   // RLE exhausted: no-match tail
        pw->run_lo = pw->run_hi;
        pw->run_hi = INT64_MAX;
        pw->run_match = false;
        pw->entry = pw->nentries + 2;
        return;
    }
    uint64_t code = rd_bits_be(pw->payload, pw->bit0 + (uint64_t)pw->entry * pw->width,
                               pw->width);
    uint64_t cnt = rd_bits_be(pw->payload,
                              pw->bit0 + (uint64_t)(pw->entry + 1) * pw->width,
                              pw->width);
    pw->entry += 2;
    pw->run_lo = pw->run_hi;
    pw->run_hi += (int64_t)cnt;
    pw->run_match = (pw->mask[(code >> 6) & 3] >> (code & 63)) & 1;
}

// Assign `match` for each lane's row (rows ascend across calls).  `need`
// lanes get the run covering their row; the walker only moves forward.
__device__ __forceinline__ bool pred_match_rows(PredWalk *pw, int64_t row,
                                                bool need) {
    if (pw->bm) {   // plain column: stateless bitmap lookup, no wave sync
        if (!need) return false;
        return (pw->bm[row >> 6] >> (row & 63)) & 1;
    }
    bool match = false;
    while (true) {
        bool mine = need && row >= pw->run_lo && row < pw->run_hi;
        if (mine) { match = pw->run_match; need = false; }
        if (__all(!need)) break;
        pred_advance(pw);
    }
    return match;
}

// The conjunction of up to three walkers for each lane's row.  Every lane
// calls every walker (RLE walkers advance wave-wide); a lane that already
// failed a slot stops needing the later ones.
__device__ __forceinline__ bool walkers_match(PredWalk *w0, PredWalk *w1,
                                              PredWalk *w2, int64_t row,
                                              bool need) {
    bool ok = true;
    if (w0) ok = pred_match_rows(w0, row, need && ok) && ok;
    if (w1) ok = pred_match_rows(w1, row, need && ok) && ok;
    if (w2) ok = pred_match_rows(w2, row, need && ok) && ok;
    return ok;
}

// ---- per-row group-by on a dictionary tag ----
// The reference groups rows by the encoded tag-value key, materialising
// groups in first-seen order (computeKey/appendKeyComponent,
// vectorized/measure/aggregation.go:523, groupby.go:287-364).  Here the
// host supplies the group DOMAIN (value -> dense group id); a resolve
// prepass maps each block's dictionary codes to group ids — per-block
// uniform tags (entity tags, the common case) collapse to a single id and
// keep the fast fold paths; row-varying tags fold per RLE run.
struct GroupDomain {
    const uint8_t *blob;     // concatenated domain value bytes
    const uint64_t *offs;    // n+1 offsets into blob
    const uint64_t *hashes;  // open-addressing table: slot -> hash
    const uint32_t *gids;    // slot -> gid (0xFFFFFFFF empty)
    uint32_t table_size;     // power of two
    uint32_t n;
};

struct GroupBlock {
    uint32_t uniform_gid;   // gid when the whole block is one run;
                            // 0xFFFFFFFE = row-varying, 0xFFFFFFFF = no tag
    uint32_t map_off;       // offset into the code->gid arena (row-varying)
    uint64_t rle_bit_off;
    uint32_t nentries;
    uint8_t width;
    uint8_t err;
    uint8_t _p[2];
};

#define GID_NONE 0xFFFFFFFFu
#define GID_VARYING 0xFFFFFFFEu

// FNV-1a 64 over value bytes (hash choice is internal; equality is by
// bytes, mirroring the reference's "equality is on key bytes" note)
__device__ __host__ inline uint64_t fnv1a(const uint8_t *p, uint64_t n) {
    uint64_t h = 1469598103934665603ULL;
    for (uint64_t i = 0; i < n; i++) {
        h ^= p[i];
        h *= 1099511628211ULL;
    }
    return h;
}

__device__ inline uint32_t domain_lookup(const GroupDomain *d, const uint8_t *v,
                                         uint64_t len) {
    uint64_t h = fnv1a(v, len);
    uint32_t mask = d->table_size - 1;
    uint32_t slot = (uint32_t)h & mask;
    for (uint32_t probe = 0; probe <= mask; probe++) {
        uint32_t g = d->gids[slot];
        if (g == GID_NONE) return GID_NONE;
        if (d->hashes[slot] == h) {
            uint64_t lo = d->offs[g], hi = d->offs[g + 1];
            if (hi - lo == len) {
                bool eq = true;
                for (uint64_t k = 0; k < len; k++)
                    if (d->blob[lo + k] != v[k]) { eq = false; break; }
                if (eq) return g;
            }
        }
        slot = (slot + 1) & mask;
    }
    return GID_NONE;
}

// ---- tag stream openers shared by every resolve kernel ----
// offset / length of a block's tag stream on one slot
__device__ __forceinline__ void tag_slot(const bydb_block_desc *bd, int slot,
                                         uint64_t *off, uint64_t *len) {
    *off = slot == 0 ? bd->tag_off : slot == 1 ? bd->tag2_off : bd->tag3_off;
    *len = slot == 0 ? bd->tag_len : slot == 1 ? bd->tag2_len : bd->tag3_len;
}

// big-endian width-typed length i of a lengths list (bytes.go:205-235);
// the stored value is len+1, 0 marks a nil value
__device__ __forceinline__ uint64_t be_len(const uint8_t *lens, uint64_t i,
                                           uint32_t wbytes) {
    uint64_t v = 0;
    for (uint32_t b = 0; b < wbytes; b++) v = (v << 8) | lens[i * wbytes + b];
    return v;
}

__device__ __forceinline__ uint32_t len_width_bytes(uint8_t wt) {
    return wt == 0 ? 1 : wt == 1 ? 2 : wt == 2 ? 4 : 8;
}

#define TS_NIL 0     // block has no column on the slot: every row nil
#define TS_PLAIN 1   // plain (non-dictionary) column, see plain_open
#define TS_DICT 2
#define TS_ERR 3     // unparseable on device

struct DictStream {
    const uint8_t *base;   // payload or sidecar; bit0 is relative to it
    const uint8_t *lens;   // `count` lengths (be_len), wbytes each
    const uint8_t *vals;   // value bytes, back to back
    uint64_t count;        // dictionary values
    uint64_t bit0;         // bit offset of the first packed RLE entry
    uint32_t wbytes;
    uint32_t nentries;     // packed entries, 2 per run: code, count
    uint32_t width;        // bits per packed entry
    bool in_sidecar;       // host-normalized stream (TAG_SIDECAR_BIT)
};

// Classify a block's tag stream on one slot; for TS_DICT parse the stream
// header: [ENC_DICTIONARY][varuint count (int.go:152-199)][lengths section]
// [values section][32b entry count][8b width][entries...] (bit-packed
// MSB-first).  base / in_sidecar are set for every kind but TS_NIL.
__device__ int tag_open(const uint8_t *__restrict__ payload,
                        const uint8_t *__restrict__ sidecar,
                        const bydb_block_desc *__restrict__ bd, int slot,
                        DictStream *ds) {
    uint64_t toff, tlen;
    tag_slot(bd, slot, &toff, &tlen);
    if (tlen == 0) return TS_NIL;
    ds->in_sidecar = (toff & TAG_SIDECAR_BIT) != 0;
    ds->base = ds->in_sidecar ? sidecar : payload;
    const uint8_t *p = ds->base + (toff & ~TAG_SIDECAR_BIT);
    const uint8_t *end = p + tlen;
    if (*p == BYDB_ENC_PLAIN) return TS_PLAIN;
    if (*p != BYDB_ENC_DICTIONARY) return TS_ERR;
    p++;
    uint64_t count = 0;
    unsigned sh = 0;
    while (p < end) {
        uint8_t c = *p++;
        count |= (uint64_t)(c & 0x7f) << sh;
        if (c < 0x80) break;
        sh += 7;
    }
    ds->count = count;
    uint64_t ll = 0;
    const uint8_t *lens_blk = dict_section(p, end, &ll);
    if (!lens_blk) return TS_ERR;
    uint64_t vl = 0;
    ds->vals = dict_section(lens_blk + ll, end, &vl);
    if (!ds->vals) return TS_ERR;
    ds->wbytes = len_width_bytes(lens_blk[0]);
    ds->lens = lens_blk + 1;
    uint64_t hdr = ((uint64_t)(ds->vals + vl - ds->base)) * 8;
    ds->nentries = (uint32_t)rd_bits_be(ds->base, hdr, 32);
    ds->width = ds->nentries ? (uint32_t)rd_bits_be(ds->base, hdr + 32, 8) : 0;
    ds->bit0 = hdr + 40;
    return TS_DICT;
}

// the rle_bit_off a PredBlock / GroupBlock carries for this dictionary
__device__ __forceinline__ uint64_t dict_rle_bit_off(const DictStream &ds) {
    return ds.bit0 | (ds.in_sidecar ? TAG_SIDECAR_BIT : 0);
}

// Single-run check: one (code, count) pair whose count covers the whole
// block.  Returns that run's code, or -1 for a row-varying block.
__device__ __forceinline__ int64_t dict_uniform_code(
    const DictStream &ds, const bydb_block_desc *bd) {
    if (ds.nentries != 2) return -1;
    uint64_t code = rd_bits_be(ds.base, ds.bit0, ds.width);
    uint64_t cnt = rd_bits_be(ds.base, ds.bit0 + ds.width, ds.width);
    return cnt >= bd->count ? (int64_t)code : -1;
}

struct PlainStream {
    const uint8_t *lens;   // `n` lengths (be_len), wbytes each
    const uint8_t *vals;   // value bytes, back to back
    uint64_t n;            // rows
    uint32_t wbytes;
};

// Header of a host-normalized plain stream: [ENC_PLAIN][u32le n][wt]
// [lens BE][payload].  False when n disagrees with the block's row count.
__device__ __forceinline__ bool plain_open(
    const uint8_t *__restrict__ payload, const uint8_t *__restrict__ sidecar,
    const bydb_block_desc *__restrict__ bd, int slot, PlainStream *ps) {
    uint64_t toff, tlen;
    tag_slot(bd, slot, &toff, &tlen);
    const uint8_t *p = (toff & TAG_SIDECAR_BIT)
                           ? sidecar + (toff & ~TAG_SIDECAR_BIT)
                           : payload + toff;
    p++;  // ENC_PLAIN
    ps->n = (uint64_t)p[0] | ((uint64_t)p[1] << 8) | ((uint64_t)p[2] << 16) |
            ((uint64_t)p[3] << 24);
    ps->wbytes = len_width_bytes(p[4]);
    ps->lens = p + 5;
    ps->vals = ps->lens + ps->n * ps->wbytes;
    return ps->n == (uint64_t)bd->count;
}

// one lane's row of a 64-row chunk of a plain stream
struct PlainRow {
    bool valid;     // row < n
    uint64_t lp1;   // stored length: len+1, 0 = nil row
    uint64_t vlen;
    uint64_t off;   // value offset in PlainStream::vals
};

// Rows [base, base+64) of a plain stream, one per lane: a wave prefix scan
// over the value lengths gives the payload offsets.  *carry is the payload
// bytes consumed by the chunks before (0 at base 0) and is advanced.  The
// whole wave calls this together.
__device__ __forceinline__ PlainRow plain_chunk(const PlainStream &ps,
                                                uint64_t base, int lane,
                                                uint64_t *carry) {
    PlainRow r;
    uint64_t row = base + (uint64_t)lane;
    r.valid = row < ps.n;
    r.lp1 = r.valid ? be_len(ps.lens, row, ps.wbytes) : 0;
    r.vlen = r.lp1 ? r.lp1 - 1 : 0;
    uint64_t incl = wave_incl_scan(r.vlen, lane);
    r.off = *carry + incl - r.vlen;
    *carry += readlane64(incl, WAVE - 1);
    return r;
}

// Claim the next per-stream arena slot (bitmap words / run pairs) for the
// block this wave resolves; every lane gets the id.
__device__ __forceinline__ uint32_t claim_stream_slot(uint32_t *ctr, int lane) {
    uint32_t slot_id = 0;
    if (lane == 0) slot_id = atomicAdd(ctr, 1u);
    return (uint32_t)__shfl((int)slot_id, 0);
}

// one thread per block: parse the tag dictionary, map codes to gids
__global__ void k_resolve_groups(const uint8_t *__restrict__ payload,
                                 const uint8_t *__restrict__ sidecar,
                                 const bydb_block_desc *__restrict__ blocks,
                                 int64_t n_blocks, int slot, GroupDomain dom,
                                 GroupBlock *__restrict__ out,
                                 uint16_t *__restrict__ map_arena,
                                 uint32_t map_base) {
    int64_t bi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (bi >= n_blocks) return;
    const bydb_block_desc *bd = &blocks[bi];
    GroupBlock gb;
    gb.uniform_gid = GID_NONE;
    gb.map_off = map_base + (uint32_t)(bi * 256);
    gb.rle_bit_off = 0; gb.nentries = 0; gb.width = 0; gb.err = 0;
    gb._p[0] = gb._p[1] = 0;
    DictStream ds;
    int kind = tag_open(payload, sidecar, bd, slot, &ds);
    if (kind == TS_PLAIN) {
        // plain (>256-distinct) column: per-row gids are resolved by the
        // follow-up wave kernel (k_resolve_plain_groups) into (gid,count)
        // run pairs; width 0xFF + nentries 0 marks "pending" and the scan
        // errors loudly if it stays that way
        gb.width = 0xFF;
        gb.uniform_gid = GID_VARYING;
    }
    if (kind == TS_ERR) gb.err = 1;
    if (kind != TS_DICT) { out[bi] = gb; return; }
    uint64_t voff = 0;
    uint16_t *map = map_arena + gb.map_off;
    for (uint64_t v = 0; v < ds.count && v < 256; v++) {
        uint64_t alen = be_len(ds.lens, v, ds.wbytes);
        uint64_t vlen = alen ? alen - 1 : 0;
        uint32_t g = alen ? domain_lookup(&dom, ds.vals + voff, vlen) : GID_NONE;
        voff += vlen;
        map[v] = g == GID_NONE ? 0xFFFFu : (uint16_t)g;
    }
    gb.nentries = ds.nentries;
    gb.width = (uint8_t)ds.width;
    gb.rle_bit_off = dict_rle_bit_off(ds);
    int64_t code = dict_uniform_code(ds, bd);
    if (code >= 0) {
        uint16_t m = map[code < 256 ? code : 0];
        gb.uniform_gid = m == 0xFFFFu ? GID_NONE : m;
    } else {
        gb.uniform_gid = GID_VARYING;
    }
    out[bi] = gb;
}

// Per-row group-by on a PLAIN (>256-distinct) tag column — computeKey
// groups on any key column (groupby.go:287-364); the reference's plain
// fallback (column.go:266-278) stores a bytes block, host-normalized into
// the sidecar at part registration.  One wave per block: each row's value
// maps to its domain gid (equality by bytes, like appendKeyComponent);
// consecutive equal gids compress into (gid,count) u16 run pairs in the
// run arena, so the group merge walks them with the same cursor shape as
// dictionary RLE.  Single-run blocks collapse to a uniform gid and keep
// every fast fold path.  Nil and out-of-domain rows become gid 0xFFFF
// (dropped rows).
#define GRUN_ENTRIES_PER_STREAM (2 * (8192 + 1))
__global__ __launch_bounds__(WAVE) void k_resolve_plain_groups(
    const uint8_t *__restrict__ payload, const uint8_t *__restrict__ sidecar,
    const bydb_block_desc *__restrict__ blocks, int64_t n_blocks, int slot,
    GroupDomain dom, GroupBlock *__restrict__ out,
    uint16_t *__restrict__ gruns, uint64_t grun_cap_streams,
    uint32_t *__restrict__ ctr) {
    const int lane = threadIdx.x;
    for (int64_t bi = blockIdx.x; bi < n_blocks; bi += gridDim.x) {
        GroupBlock gb = out[bi];
        if (gb.width != 0xFF || gb.err) continue;
        const bydb_block_desc *bd = &blocks[bi];
        PlainStream ps;
        if (!plain_open(payload, sidecar, bd, slot, &ps)) {
            if (lane == 0) out[bi].err = 1;
            continue;
        }
        const uint64_t n = ps.n;
        uint32_t slot_id = claim_stream_slot(ctr, lane);
        if (slot_id >= grun_cap_streams) {
            if (lane == 0) out[bi].err = 1;   // arena exhausted: loud
            continue;
        }
        uint16_t *rp = gruns + (uint64_t)slot_id * GRUN_ENTRIES_PER_STREAM;
        uint64_t carry_bytes = 0;
        uint32_t n_pairs = 0;
        int32_t cur_gid = -2;   // no open run yet
        uint32_t cur_cnt = 0;
        for (uint64_t base = 0; base < n; base += WAVE) {
            PlainRow r = plain_chunk(ps, base, lane, &carry_bytes);
            int32_t g = -1;     // nil or out-of-domain: dropped row
            if (r.valid && r.lp1) {
                uint32_t gg = domain_lookup(&dom, ps.vals + r.off, r.vlen);
                g = gg == GID_NONE ? -1 : (int32_t)gg;
            }
            int32_t prev = __shfl_up(g, 1);
            if (lane == 0) prev = cur_gid;
            bool is_start = r.valid && g != prev;
            uint64_t starts = __ballot(is_start);
            uint32_t chunk_rows =
                (uint32_t)(n - base < WAVE ? n - base : (uint64_t)WAVE);
            if (starts == 0) {
                cur_cnt += chunk_rows;
            } else {
                int F = (int)__builtin_ctzll(starts);
                bool head = (cur_cnt + (uint32_t)F) > 0;
                if (lane == 0 && head) {
                    rp[2 * n_pairs] =
                        cur_gid < 0 ? 0xFFFFu : (uint16_t)cur_gid;
                    rp[2 * n_pairs + 1] = (uint16_t)(cur_cnt + (uint32_t)F);
                }
                int last = 63 - __clzll(starts);
                int nst = __popcll(starts);
                if (is_start && lane != last) {
                    int rank = __popcll(starts & lanemask_lt(lane));
                    uint64_t hi = starts >> (lane + 1);   // lane < 63 here
                    int nxt = lane + 1 + (int)__builtin_ctzll(hi);
                    uint32_t idx = n_pairs + (head ? 1u : 0u) + (uint32_t)rank;
                    rp[2 * idx] = g < 0 ? 0xFFFFu : (uint16_t)g;
                    rp[2 * idx + 1] = (uint16_t)(nxt - lane);
                }
                n_pairs += (head ? 1u : 0u) + (uint32_t)(nst - 1);
                cur_gid = __shfl(g, last);
                cur_cnt = chunk_rows - (uint32_t)last;
            }
        }
        if (cur_cnt > 0) {
            if (lane == 0) {
                rp[2 * n_pairs] = cur_gid < 0 ? 0xFFFFu : (uint16_t)cur_gid;
                rp[2 * n_pairs + 1] = (uint16_t)cur_cnt;
            }
            n_pairs++;
        }
        if (lane == 0) {
            GroupBlock *o = &out[bi];
            if (n_pairs == 1) {
                // whole block one run: uniform fast path, no runs walked
                uint16_t g16 = rp[0];
                o->uniform_gid = g16 == 0xFFFFu ? GID_NONE : (uint32_t)g16;
                o->width = 0;
                o->nentries = 0;
            } else {
                o->uniform_gid = GID_VARYING;
                o->rle_bit_off =
                    (uint64_t)slot_id * GRUN_ENTRIES_PER_STREAM;
                o->nentries = 2 * n_pairs;
            }
        }
    }
}

// ---------------- tag condition resolve ----------------
// The reference evaluates a measure query's tag conditions per row through
// the TagFilter tree parseFilter builds (pkg/query/logical/
// tag_filter.go:144-193).  The scan never sees tag values — it consumes
// PredBlocks and the combined flag byte — so one resolve stage serves every
// consume entry point (equality predicates are its BYDB_OP_EQ case): a
// one-thread-per-block prepass evaluates every condition of a slot against
// each dictionary value and ANDs the results into the slot's code mask; a
// one-wave-per-block prepass does the same per row of a plain column into
// a match bitmap.  Only plain (<128 B) compress_block sections are
// parseable on device (bytes.go:291-303); zstd'd dictionaries are
// host-normalized at part registration, and one that reaches the device
// anyway is surfaced as a device error.  Match rules (header comment of
// include/bydb_gpu.h restates them with the full citations):
//   EQ  bytes equal, nil never (eqTag.Match :426-432)
//   NE / NOT_IN  notTag over EQ / IN — TRUE on nil (:168, :189, :370-376)
//   IN  BelongTo, nil never (:405-411; expr_literal.go:84-92, 260-268)
//   GT/GE/LT/LE  c = literal.Compare(value): c<0 / c<=0 / c>0 / c>=0, nil
//       never (rangeTag.Match :465-503); string c = strings.Compare, int
//       c = int(lit - val) with wrapping int64 subtraction
//       (expr_literal.go:65-70, 241-246)
// k_resolve_filter ANDs the conditions (andLogicalNode); AND / OR criteria
// trees resolve through k_resolve_tree / k_resolve_tree_rows further down,
// which write the same PredBlocks and flag byte.
// Slot verdicts, and the values of the combined per-block flag byte:
#define PF_CLEAR 0   // every row matches -> fold unpredicated
#define PF_SKIP 1    // no row matches -> skip block
#define PF_WALK 2    // row-varying -> full walker path
#define PF_ERR 3     // unparseable tag stream -> device error
struct FilterCond {
    GroupDomain set;        // IN / NOT_IN: open-addressing value set
    const uint8_t *lit;     // every other op: the single literal
    uint64_t lit_len;
    int64_t lit_i;          // decoded int literal (int-typed ranges)
    uint8_t op;             // BYDB_OP_*
    uint8_t is_int;         // BYDB_TAG_INT
    uint8_t _p[6];
};

// conditions sorted by slot: slot sl owns c[first[sl] .. first[sl+1])
struct FilterSet {
    FilterCond c[BYDB_FILTER_MAX_CONDS];
    int first[4];
    uint8_t all_neg[3];     // every condition of the slot is NE / NOT_IN
    uint8_t _p;
    int n_slots;            // highest conditioned slot + 1
};

// strings.Compare(a, b) on raw bytes: a proper prefix sorts first
__device__ __forceinline__ int bytes_compare(const uint8_t *a, uint64_t alen,
                                             const uint8_t *b, uint64_t blen) {
    uint64_t n = alen < blen ? alen : blen;
    for (uint64_t k = 0; k < n; k++)
        if (a[k] != b[k]) return a[k] < b[k] ? -1 : 1;
    return alen < blen ? -1 : alen > blen ? 1 : 0;
}

// convert.BytesToInt64 (number.go:33-46): BE cell with the sign bit flipped
__device__ __forceinline__ int64_t i64_from_cell(const uint8_t *p) {
    uint64_t u = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) u = (u << 8) | p[i];
    return (int64_t)(u ^ (1ull << 63));
}

// One condition against one tag value (nil: v unused).
__device__ __forceinline__ bool cond_match(const FilterCond &c,
                                           const uint8_t *v, uint64_t len,
                                           bool nil) {
    if (c.op == BYDB_OP_EQ || c.op == BYDB_OP_NE) {
        bool eq = !nil && len == c.lit_len &&
                  bytes_compare(c.lit, c.lit_len, v, len) == 0;
        return c.op == BYDB_OP_EQ ? eq : !eq;
    }
    if (c.op == BYDB_OP_IN || c.op == BYDB_OP_NOT_IN) {
        bool in = !nil && domain_lookup(&c.set, v, len) != GID_NONE;
        return c.op == BYDB_OP_IN ? in : !in;
    }
    if (nil) return false;      // Compare returns ok=false
    int cmp;                    // sign of literal.Compare(value)
    if (c.is_int) {
        if (len != 8) return false;
        // Go int64 subtraction wraps: take the sign of the
        // two's-complement difference, not of the true one
        int64_t d = (int64_t)((uint64_t)c.lit_i - (uint64_t)i64_from_cell(v));
        cmp = d < 0 ? -1 : d > 0 ? 1 : 0;
    } else {
        cmp = bytes_compare(c.lit, c.lit_len, v, len);
    }
    return c.op == BYDB_OP_GT   ? cmp < 0
           : c.op == BYDB_OP_GE ? cmp <= 0
           : c.op == BYDB_OP_LT ? cmp > 0
                                : cmp >= 0;
}

// All of one slot's conditions against one tag value: the AND of them.
__device__ bool filter_match(const FilterSet &fs, int slot, const uint8_t *v,
                             uint64_t len, bool nil) {
    for (int i = fs.first[slot]; i < fs.first[slot + 1]; i++)
        if (!cond_match(fs.c[i], v, len, nil)) return false;
    return true;
}

// Resolve one conditioned slot of one block; fills *out for the walker
// path and returns the slot verdict.  Dictionary columns: all of the
// slot's conditions are evaluated per dictionary value into the code mask.
// A mask covering every code the dictionary defines is CLEAR and an empty
// mask is SKIP even when the block has many runs (a value the block never
// holds, NE of an absent value, or a wide range, must not push row-varying
// blocks onto the walker path); otherwise a single-run block is CLEAR or
// SKIP by its one code.  A block without the column is all-nil — CLEAR
// when every condition of the slot is negated, else SKIP.  A CLEAR slot is
// marked `disabled` for this block, so a walk forced by another slot
// treats it as no constraint.
__device__ int resolve_one_filter(const uint8_t *__restrict__ payload,
                                  const uint8_t *__restrict__ sidecar,
                                  const bydb_block_desc *__restrict__ bd,
                                  int slot, const FilterSet &fs,
                                  PredBlock *out) {
    PredBlock pb;
    for (int i = 0; i < 4; i++) pb.mask[i] = 0;
    pb.rle_bit_off = 0; pb.nentries = 0; pb.width = 0;
    pb.active = 0; pb.err = 0; pb.uniform = 0; pb.plain = 0;
    pb.disabled = 0;
    if (fs.first[slot] == fs.first[slot + 1]) {   // no condition on the slot
        pb.disabled = 1;
        *out = pb;
        return PF_CLEAR;
    }
    DictStream ds;
    int kind = tag_open(payload, sidecar, bd, slot, &ds);
    if (kind == TS_NIL) {                         // all-nil block
        pb.disabled = fs.all_neg[slot];
        *out = pb;
        return fs.all_neg[slot] ? PF_CLEAR : PF_SKIP;
    }
    // a plain column must be host-normalized: k_resolve_plain_filter fills
    // its match bitmap (an unnormalized plain stream is a loud error)
    if (kind == TS_ERR || (kind == TS_PLAIN && !ds.in_sidecar)) {
        pb.err = 1;
        *out = pb;
        return PF_ERR;
    }
    pb.active = 1;
    if (kind == TS_PLAIN) {
        pb.plain = 1;
        *out = pb;
        return PF_WALK;
    }
    uint64_t voff = 0;
    bool any = false, all = true;
    for (uint64_t v = 0; v < ds.count && v < 256; v++) {
        uint64_t alen = be_len(ds.lens, v, ds.wbytes);
        uint64_t vlen = alen ? alen - 1 : 0;
        if (filter_match(fs, slot, ds.vals + voff, vlen, alen == 0)) {
            pb.mask[(v >> 6) & 3] |= 1ull << (v & 63);
            any = true;
        } else {
            all = false;
        }
        voff += vlen;
    }
    pb.nentries = ds.nentries;
    pb.width = (uint8_t)ds.width;
    pb.rle_bit_off = dict_rle_bit_off(ds);
    int verdict = PF_WALK;
    if (!any) {
        verdict = PF_SKIP;
    } else if (all && ds.count <= 256) {
        pb.disabled = 1;
        verdict = PF_CLEAR;
    } else {
        int64_t code = dict_uniform_code(ds, bd);
        if (code >= 0) {
            pb.uniform = 1;
            bool match = (pb.mask[(code >> 6) & 3] >> (code & 63)) & 1;
            verdict = match ? PF_CLEAR : PF_SKIP;
        }
    }
    *out = pb;
    return verdict;
}

// One fused launch over blocks: every conditioned slot of a block resolves
// against one read of its descriptor and writes the combined flag byte the
// scan's hot loop prices a non-matching block at.  Every lane stays alive
// for the ballot of the walk-block census, which lets the heavy scan pass
// exit immediately when every verdict is uniform (the dominant entity-tag
// case).
__global__ void k_resolve_filter(
    const uint8_t *__restrict__ payload, const uint8_t *__restrict__ sidecar,
    const bydb_block_desc *__restrict__ blocks, int64_t n_blocks,
    FilterSet fs, PredBlock *__restrict__ out, uint8_t *__restrict__ flags,
    uint32_t *__restrict__ walk_count) {
    int64_t bi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint8_t f = PF_CLEAR;
    if (bi < n_blocks) {
        const bydb_block_desc *bd = &blocks[bi];
        for (int sl = 0; sl < fs.n_slots; sl++) {
            PredBlock pb;
            int v = resolve_one_filter(payload, sidecar, bd, sl, fs, &pb);
            out[(int64_t)sl * n_blocks + bi] = pb;
            if (v == PF_ERR) { f = PF_ERR; break; }
            if (v == PF_SKIP) { f = PF_SKIP; break; }
            if (v == PF_WALK) f = PF_WALK;
        }
        flags[bi] = f;
    }
    uint64_t wmask = __ballot(bi < n_blocks && f == PF_WALK);
    if ((threadIdx.x & 63) == 0 && wmask)
        atomicAdd(walk_count, (uint32_t)__popcll(wmask));
}

// Plain-column stage: one wave per block evaluates all of the slot's
// conditions on every row of the normalized stream (nil rows — stored
// length 0 — follow the nil rules) and writes one ballot word per 64 rows
// into the bitmap arena.  The residual-predicate pushdown the reference
// performs row-by-row on decoded [][]byte (aggregation.go:310 over
// column.go:410 Plain columns) becomes 64 rows per step.
__global__ __launch_bounds__(WAVE) void k_resolve_plain_filter(
    const uint8_t *__restrict__ payload, const uint8_t *__restrict__ sidecar,
    const bydb_block_desc *__restrict__ blocks, int64_t n_blocks,
    FilterSet fs, int slot, PredBlock *__restrict__ out,
    uint64_t *__restrict__ bm, uint32_t *__restrict__ ctr,
    uint64_t bm_cap_streams) {
    const int lane = threadIdx.x;
    for (int64_t bi = blockIdx.x; bi < n_blocks; bi += gridDim.x) {
        PredBlock pb = out[bi];
        if (!pb.plain || pb.err) continue;
        PlainStream ps;
        if (!plain_open(payload, sidecar, &blocks[bi], slot, &ps) ||
            ps.n > (uint64_t)PLAIN_BM_WORDS * 64) {
            if (lane == 0) out[bi].err = 1;
            continue;
        }
        uint32_t slot_id = claim_stream_slot(ctr, lane);
        if (slot_id >= bm_cap_streams) {
            if (lane == 0) out[bi].err = 1;   // arena exhausted: loud
            continue;
        }
        uint64_t w0 = (uint64_t)slot_id * PLAIN_BM_WORDS;
        uint64_t carry = 0;
        for (uint64_t base = 0; base < ps.n; base += WAVE) {
            PlainRow r = plain_chunk(ps, base, lane, &carry);
            bool match = r.valid && filter_match(fs, slot, ps.vals + r.off,
                                                 r.vlen, r.lp1 == 0);
            uint64_t word = __ballot(match);
            if (lane == 0) bm[w0 + (base >> 6)] = word;
        }
        if (lane == 0) out[bi].rle_bit_off = w0;
    }
}

// ---------------- criteria tree resolve ----------------
// The reference's BuildTagFilter (tag_filter.go:84-142) nests
// andLogicalNode / orLogicalNode over the per-condition filters; a node
// folds its children's results left to right (isMatch :259-274) with
// merge = all (:288-295) or any (:323-330).  The host flattens the tree
// into a 256-bit truth table indexed by the conditions' result signature
// (bit i = condition i), so the device never walks a tree: it evaluates
// leaves with cond_match, assembles the signature and looks one bit up.
// Every leaf keeps its own nil rule, so NE / NOT_IN leaves are true on nil
// rows under OR exactly as under AND.
//
// Per block, a conditioned slot is CONSTANT (no column: the leaves take
// their nil result; single-run dictionary: the leaves on the one value) or
// VARYING (multi-run dictionary, plain column).  Three verdict classes:
//   no varying slot       one lookup -> CLEAR / SKIP (entity tags)
//   one varying dict slot per-code lookup -> that slot's code mask, walked
//                         by the scan's RLE walker (or CLEAR / SKIP when
//                         the mask is full / empty)
//   anything else         CLEAR / SKIP when the table is constant over the
//                         signatures the block can reach, else a ROW-BITMAP
//                         block: k_resolve_tree_rows writes one match bit
//                         per row and the scan's bitmap walker consumes it
//                         as a plain-column predicate on slot 0
// The scan kernel sees PredBlocks and the flag byte only, as before.
struct TreeSpec {
    uint64_t tt[4];     // bit sig: the tree's result
    uint32_t bits;      // nibble k: signature bit of FilterSet::c[k]
    uint32_t _p;
};

__device__ __forceinline__ uint32_t tree_leaf_bit(const TreeSpec &ts, int k) {
    return 1u << ((ts.bits >> (4 * k)) & 7);
}

__device__ __forceinline__ bool tree_lookup(const TreeSpec &ts, uint32_t sig) {
    uint32_t w = (sig >> 6) & 3;
    uint64_t word = w == 0 ? ts.tt[0] : w == 1 ? ts.tt[1]
                    : w == 2 ? ts.tt[2] : ts.tt[3];
    return (word >> (sig & 63)) & 1;
}

// signature bits one slot's leaves contribute for one tag value
__device__ uint32_t slot_sig(const FilterSet &fs, const TreeSpec &ts, int slot,
                             const uint8_t *v, uint64_t len, bool nil) {
    uint32_t sig = 0;
    for (int k = fs.first[slot]; k < fs.first[slot + 1]; k++)
        if (cond_match(fs.c[k], v, len, nil)) sig |= tree_leaf_bit(ts, k);
    return sig;
}

#define TK_CONST 0   // contributes fixed signature bits for the whole block
#define TK_DICT 1    // multi-run dictionary: signature varies by code
#define TK_PLAIN 2   // plain column: signature varies by row
#define TK_ERR 3

// Classify one slot of one block; a constant slot ORs its bits into
// *const_sig, a dictionary slot leaves its parsed header in *ds.
__device__ __forceinline__ int tree_classify_slot(
    const uint8_t *__restrict__ payload, const uint8_t *__restrict__ sidecar,
    const bydb_block_desc *__restrict__ bd, int slot, const FilterSet &fs,
    const TreeSpec &ts, DictStream *ds, uint32_t *const_sig) {
    if (fs.first[slot] == fs.first[slot + 1]) return TK_CONST;
    int kind = tag_open(payload, sidecar, bd, slot, ds);
    if (kind == TS_NIL) {
        *const_sig |= slot_sig(fs, ts, slot, nullptr, 0, true);
        return TK_CONST;
    }
    if (kind == TS_ERR || (kind == TS_PLAIN && !ds->in_sidecar)) return TK_ERR;
    if (kind == TS_PLAIN) return TK_PLAIN;
    if (ds->count > 256) return TK_ERR;
    int64_t code = dict_uniform_code(*ds, bd);
    if (code < 0) return TK_DICT;
    if ((uint64_t)code >= ds->count) return TK_ERR;
    uint64_t voff = 0, alen = 0;
    for (int64_t v = 0; v <= code; v++) {
        alen = be_len(ds->lens, (uint64_t)v, ds->wbytes);
        if (v < code) voff += alen ? alen - 1 : 0;
    }
    *const_sig |= slot_sig(fs, ts, slot, ds->vals + voff, alen ? alen - 1 : 0,
                           alen == 0);
    return TK_CONST;
}

__device__ __forceinline__ void sigset_add(uint64_t set[4], uint32_t sig) {
    uint32_t w = (sig >> 6) & 3;
    uint64_t b = 1ull << (sig & 63);
    set[0] |= w == 0 ? b : 0;
    set[1] |= w == 1 ? b : 0;
    set[2] |= w == 2 ? b : 0;
    set[3] |= w == 3 ? b : 0;
}

// next member of a signature set at or above `from`, 256 when none
__device__ __forceinline__ uint32_t sigset_next(const uint64_t set[4],
                                                uint32_t from) {
    for (uint32_t w = from >> 6; w < 4; w++) {
        uint64_t m = w == 0 ? set[0] : w == 1 ? set[1]
                     : w == 2 ? set[2] : set[3];
        if (w == (from >> 6)) m &= ~0ull << (from & 63);
        if (m) return w * 64 + (uint32_t)__builtin_ctzll(m);
    }
    return 256;
}

// reach := { r | p : r in reach, p in part } — at most 256 pairs, since
// the slots' signature bits are disjoint
__device__ __forceinline__ void sigset_cross(uint64_t reach[4],
                                             const uint64_t part[4]) {
    uint64_t next[4] = {0, 0, 0, 0};
    for (uint32_t p = sigset_next(part, 0); p < 256;
         p = sigset_next(part, p + 1))
        for (uint32_t r = sigset_next(reach, 0); r < 256;
             r = sigset_next(reach, r + 1))
            sigset_add(next, r | p);
    reach[0] = next[0]; reach[1] = next[1];
    reach[2] = next[2]; reach[3] = next[3];
}

// One thread per block: classify, then decide by the truth table.  Writes
// what k_resolve_filter writes — PredBlock[3][n_blocks], the flag byte, the
// walk census — plus the per-class block counts in stats[4] (clear, skip,
// code-mask walk, row-bitmap walk); stats[3] sizes the bitmap arena.
__global__ void k_resolve_tree(
    const uint8_t *__restrict__ payload, const uint8_t *__restrict__ sidecar,
    const bydb_block_desc *__restrict__ blocks, int64_t n_blocks,
    FilterSet fs, TreeSpec ts, PredBlock *__restrict__ out,
    uint8_t *__restrict__ flags, uint32_t *__restrict__ walk_count,
    uint32_t *__restrict__ stats) {
    int64_t bi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint8_t f = PF_CLEAR;
    bool rows_blk = false;
    if (bi < n_blocks) {
        const bydb_block_desc *bd = &blocks[bi];
        PredBlock off;
        for (int i = 0; i < 4; i++) off.mask[i] = 0;
        off.rle_bit_off = 0; off.nentries = 0; off.width = 0;
        off.active = 0; off.err = 0; off.uniform = 0; off.plain = 0;
        off.disabled = 1;
        PredBlock walk = off;
        int walk_slot = -1;
        uint32_t const_sig = 0;
        int kinds[3] = {TK_CONST, TK_CONST, TK_CONST};
        DictStream ds[3];
        int n_var = 0, var_slot = 0, var_kind = TK_CONST;
        bool err = false;
#pragma unroll
        for (int sl = 0; sl < 3; sl++) {
            if (sl >= fs.n_slots) continue;
            kinds[sl] = tree_classify_slot(payload, sidecar, bd, sl, fs, ts,
                                           &ds[sl], &const_sig);
            if (kinds[sl] == TK_ERR) err = true;
            if (kinds[sl] == TK_DICT || kinds[sl] == TK_PLAIN) {
                n_var++;
                var_slot = sl;
                var_kind = kinds[sl];
            }
        }
        if (err) {
            f = PF_ERR;
        } else if (n_var == 0) {
            f = tree_lookup(ts, const_sig) ? PF_CLEAR : PF_SKIP;
        } else if (n_var == 1 && var_kind == TK_DICT) {
            // the single-slot shape of resolve_one_filter: one code mask
            bool any = false, all = true;
#pragma unroll
            for (int sl = 0; sl < 3; sl++) {
                if (sl != var_slot) continue;
                const DictStream &d = ds[sl];
                uint64_t voff = 0;
                for (uint64_t v = 0; v < d.count; v++) {
                    uint64_t alen = be_len(d.lens, v, d.wbytes);
                    uint64_t vlen = alen ? alen - 1 : 0;
                    uint32_t sig = const_sig | slot_sig(fs, ts, sl,
                                                        d.vals + voff, vlen,
                                                        alen == 0);
                    if (tree_lookup(ts, sig)) {
                        sigset_add(walk.mask, (uint32_t)v);
                        any = true;
                    } else {
                        all = false;
                    }
                    voff += vlen;
                }
                walk.nentries = d.nentries;
                walk.width = (uint8_t)d.width;
                walk.rle_bit_off = dict_rle_bit_off(d);
            }
            if (!any) {
                f = PF_SKIP;
            } else if (all) {
                f = PF_CLEAR;
            } else {
                f = PF_WALK;
                walk.active = 1;
                walk.disabled = 0;
                walk_slot = var_slot;
            }
        } else {
            // signatures the block can reach: constant bits, times what
            // each dictionary actually produces, times every combination
            // of a plain slot's leaves
            uint64_t reach[4] = {0, 0, 0, 0};
            sigset_add(reach, const_sig);
#pragma unroll
            for (int sl = 0; sl < 3; sl++) {
                if (kinds[sl] != TK_DICT && kinds[sl] != TK_PLAIN) continue;
                uint64_t part[4] = {0, 0, 0, 0};   // this slot's signatures
                if (kinds[sl] == TK_DICT) {
                    uint64_t voff = 0;
                    for (uint64_t v = 0; v < ds[sl].count; v++) {
                        uint64_t alen = be_len(ds[sl].lens, v, ds[sl].wbytes);
                        uint64_t vlen = alen ? alen - 1 : 0;
                        sigset_add(part, slot_sig(fs, ts, sl,
                                                  ds[sl].vals + voff, vlen,
                                                  alen == 0));
                        voff += vlen;
                    }
                } else {
                    uint32_t m = 0;
                    for (int k = fs.first[sl]; k < fs.first[sl + 1]; k++)
                        m |= tree_leaf_bit(ts, k);
                    uint32_t sub = 0;
                    do {          // every subset of the slot's leaf bits
                        sigset_add(part, sub);
                        sub = (sub - m) & m;
                    } while (sub != 0);
                }
                sigset_cross(reach, part);
            }
            bool any = false, all = true;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                if (reach[i] & ts.tt[i]) any = true;
                if (reach[i] & ~ts.tt[i]) all = false;
            }
            if (!any) {
                f = PF_SKIP;
            } else if (all) {
                f = PF_CLEAR;
            } else {
                // row-bitmap block: slot 0 carries the bitmap as a plain
                // predicate; k_resolve_tree_rows fills rle_bit_off
                f = PF_WALK;
                rows_blk = true;
                walk.active = 1;
                walk.plain = 1;
                walk.disabled = 0;
                walk_slot = 0;
            }
        }
        if (f == PF_ERR) off.err = 1;
#pragma unroll
        for (int sl = 0; sl < 3; sl++)
            if (sl < fs.n_slots) {
                if (sl == walk_slot) out[(int64_t)sl * n_blocks + bi] = walk;
                else out[(int64_t)sl * n_blocks + bi] = off;
            }
        flags[bi] = f;
    }
    const bool live = bi < n_blocks;
    uint64_t wmask = __ballot(live && f == PF_WALK);
    uint64_t rmask = __ballot(live && rows_blk);
    uint64_t cmask = __ballot(live && f == PF_CLEAR);
    uint64_t smask = __ballot(live && f == PF_SKIP);
    if ((threadIdx.x & 63) == 0) {
        if (wmask) atomicAdd(walk_count, (uint32_t)__popcll(wmask));
        if (cmask) atomicAdd(&stats[0], (uint32_t)__popcll(cmask));
        if (smask) atomicAdd(&stats[1], (uint32_t)__popcll(smask));
        if (wmask & ~rmask)
            atomicAdd(&stats[2], (uint32_t)__popcll(wmask & ~rmask));
        if (rmask) atomicAdd(&stats[3], (uint32_t)__popcll(rmask));
    }
}

// wave-uniform forward cursor over a dictionary slot's bit-packed RLE runs
struct CodeWalk {
    const uint8_t *base;
    uint64_t bit0;
    uint32_t nentries, width;
    uint32_t entry;            // next entry index (2 per run)
    int64_t run_lo, run_hi;    // rows [run_lo, run_hi) of the current run
    uint32_t run_code;
};

#define CODE_NONE 0xFFFFFFFFu  // row past the last run

// The dictionary code of each lane's row (rows ascend across calls): the
// shape of pred_match_rows, returning the run's code instead of its match.
__device__ __forceinline__ uint32_t code_of_rows(CodeWalk *cw, int64_t row,
                                                 bool need) {
    uint32_t code = CODE_NONE;
    while (true) {
        bool mine = need && row >= cw->run_lo && row < cw->run_hi;
        if (mine) { code = cw->run_code; need = false; }
        if (__all(!need)) break;
        if (cw->entry + 1 >= cw->nentries) {   // RLE exhausted
            cw->run_lo = cw->run_hi;
            cw->run_hi = INT64_MAX;
            cw->run_code = CODE_NONE;
            continue;
        }
        uint64_t c = rd_bits_be(cw->base,
                                cw->bit0 + (uint64_t)cw->entry * cw->width,
                                cw->width);
        uint64_t cnt = rd_bits_be(
            cw->base, cw->bit0 + (uint64_t)(cw->entry + 1) * cw->width,
            cw->width);
        cw->entry += 2;
        cw->run_lo = cw->run_hi;
        cw->run_hi += (int64_t)cnt;
        cw->run_code = (uint32_t)c;
    }
    return code;
}

// Row-bitmap stage: one wave per row-bitmap block.  Setup re-classifies
// the block's slots (cheap, wave-uniform), claims a 128-word bitmap and
// builds a code -> signature byte table in LDS per varying dictionary slot
// (lanes take dictionary values lane, lane+64, ...; value offsets come
// from the wave prefix scan in plain_chunk over the dictionary's length
// list).  Then 64 rows per step: each lane gets its row's code from the
// forward RLE cursor (dictionary slots) or its row's value (plain slots),
// assembles the signature, looks the truth table up, and the ballot is the
// bitmap word.  Rows whose code no run covers, or whose code the
// dictionary does not define, match nothing — the RLE walker's no-match
// tail.  That is a rule for malformed streams only (runs that do not add
// up to the block's row count), and on such a block the two kernels can
// disagree: k_resolve_tree reasons over dictionary values, not rows, so it
// may call the block CLEAR (say through a NE leaf on another slot) where
// this kernel, had the block reached it, would drop the uncovered rows.
// Unparseable streams, over-long blocks and an exhausted arena set
// err and turn the block's flag byte to PF_ERR, which the scan reports.
__global__ __launch_bounds__(WAVE) void k_resolve_tree_rows(
    const uint8_t *__restrict__ payload, const uint8_t *__restrict__ sidecar,
    const bydb_block_desc *__restrict__ blocks, int64_t n_blocks,
    FilterSet fs, TreeSpec ts, PredBlock *__restrict__ out,
    uint8_t *__restrict__ flags, uint64_t *__restrict__ bm,
    uint32_t *__restrict__ ctr, uint64_t bm_cap_streams) {
    __shared__ uint8_t sigtab[3][256];
    const int lane = threadIdx.x;
    for (int64_t bi = blockIdx.x; bi < n_blocks; bi += gridDim.x) {
        if (flags[bi] != PF_WALK || !out[bi].plain) continue;
        const bydb_block_desc *bd = &blocks[bi];
        const uint64_t n = bd->count;
        uint32_t const_sig = 0;
        int kinds[3] = {TK_CONST, TK_CONST, TK_CONST};
        DictStream ds[3];
        PlainStream ps[3];
        CodeWalk cw[3];
        uint64_t carry[3] = {0, 0, 0};
        bool bad = n > (uint64_t)PLAIN_BM_WORDS * 64;
#pragma unroll
        for (int sl = 0; sl < 3; sl++) {
            if (sl >= fs.n_slots) continue;
            kinds[sl] = tree_classify_slot(payload, sidecar, bd, sl, fs, ts,
                                           &ds[sl], &const_sig);
            if (kinds[sl] == TK_ERR) bad = true;
            if (kinds[sl] == TK_PLAIN &&
                !plain_open(payload, sidecar, bd, sl, &ps[sl]))
                bad = true;
        }
        uint32_t slot_id = 0;
        if (!bad) {
            slot_id = claim_stream_slot(ctr, lane);
            if (slot_id >= bm_cap_streams) bad = true;  // arena exhausted
        }
        if (bad) {
            if (lane == 0) {
                out[bi].err = 1;
                flags[bi] = PF_ERR;
            }
            continue;
        }
        __syncthreads();   // the previous block's table reads are done
#pragma unroll
        for (int sl = 0; sl < 3; sl++) {
            if (kinds[sl] != TK_DICT) continue;
            PlainStream dv;    // the dictionary's value list, read as rows
            dv.lens = ds[sl].lens;
            dv.vals = ds[sl].vals;
            dv.n = ds[sl].count;
            dv.wbytes = ds[sl].wbytes;
            uint64_t dcarry = 0;
            for (uint64_t base = 0; base < dv.n; base += WAVE) {
                PlainRow r = plain_chunk(dv, base, lane, &dcarry);
                if (r.valid)
                    sigtab[sl][base + (uint64_t)lane] = (uint8_t)slot_sig(
                        fs, ts, sl, dv.vals + r.off, r.vlen, r.lp1 == 0);
            }
            cw[sl].base = ds[sl].base;
            cw[sl].bit0 = ds[sl].bit0;
            cw[sl].nentries = ds[sl].nentries;
            cw[sl].width = ds[sl].width;
            cw[sl].entry = 0;
            cw[sl].run_lo = 0;
            cw[sl].run_hi = 0;
            cw[sl].run_code = CODE_NONE;
        }
        __syncthreads();
        const uint64_t w0 = (uint64_t)slot_id * PLAIN_BM_WORDS;
        for (uint64_t base = 0; base < n; base += WAVE) {
            const uint64_t row = base + (uint64_t)lane;
            const bool valid = row < n;
            uint32_t sig = const_sig;
            bool ok = valid;
#pragma unroll
            for (int sl = 0; sl < 3; sl++) {
                if (kinds[sl] == TK_DICT) {
                    uint32_t code = code_of_rows(&cw[sl], (int64_t)row, valid);
                    if ((uint64_t)code < ds[sl].count)
                        sig |= sigtab[sl][code];
                    else
                        ok = false;
                } else if (kinds[sl] == TK_PLAIN) {
                    PlainRow r = plain_chunk(ps[sl], base, lane, &carry[sl]);
                    if (r.valid)
                        sig |= slot_sig(fs, ts, sl, ps[sl].vals + r.off,
                                        r.vlen, r.lp1 == 0);
                }
            }
            uint64_t word = __ballot(ok && tree_lookup(ts, sig));
            if (lane == 0) bm[w0 + (base >> 6)] = word;
        }
        if (lane == 0) out[bi].rle_bit_off = w0;
    }
}

// Fold arithmetic-progression blocks (Const dd=0 / DeltaConst) under a
// per-row predicate: walk rows 64 at a time through the RLE runs.
__device__ void fold_arith_pred(int64_t first, int64_t dd, int64_t r0,
                                int64_t r1, int lane, PredWalk *pw0,
                                PredWalk *pw1, PredWalk *pw2,
                                uint64_t *out_sum, uint64_t *out_cnt,
                                int64_t *out_mn, int64_t *out_mx) {
    uint64_t lsum = 0, lcnt = 0;
    int64_t lmn = INT64_MAX, lmx = INT64_MIN;
    for (int64_t base = r0; base <= r1; base += 64) {
        int64_t row = base + lane;
        bool need = row <= r1;
        bool match = walkers_match(pw0, pw1, pw2, row, need);
        if (need && match) {
            int64_t v = (int64_t)((uint64_t)first + (uint64_t)row * (uint64_t)dd);
            lsum += (uint64_t)v;
            lcnt++;
            lmn = v < lmn ? v : lmn;
            lmx = v > lmx ? v : lmx;
        }
    }
    *out_sum = wave_reduce_add(lsum);
    *out_cnt = wave_reduce_add(lcnt);
    *out_mn = wave_reduce_min(lmn);
    *out_mx = wave_reduce_max(lmx);
}

// Full value reconstruction over a delta or delta-of-delta stream with a
// per-value callback encoded as flags (fold min/max/sum/sumf, or count
// ts-range bounds).  dod=false: values are rows j=1..n-1 (row 0 = first,
// handled by the caller).  dod=true: stream holds d2 for rows 2..n-1 and
// d1_init has been parsed; rows 0,1 handled by the caller.
struct ScanFold {
    uint64_t sum;       // wrapping sum of selected values
    int64_t mn, mx;     // min/max of selected values
    uint64_t nsel;      // selected row count
};

// full: compile-time promise that [r0, r1] covers every streamed row
// (the clamp-free instantiations pass the template constant !EN_CLAMP),
// letting the per-value selection branch dead-code out of the quad fold
// — less register pressure for the 7-wave build.
__device__ void scan_stream(const uint8_t *stream, int64_t n_deltas, bool dod,
                            int64_t first_plus /* v at row (dod?1:0) */,
                            int64_t d1_init, int64_t r0, int64_t r1,
                            int lane, ScanFold *f, DevErr *derr, uint64_t bi,
                            PredWalk *pw0, PredWalk *pw1, PredWalk *pw2,
                            bool full = false) {
    uint64_t pos = 0;
    int64_t j = dod ? 2 : 1;
    int64_t jmax = n_deltas;            // always scan the whole stream
    uint64_t v_carry = (uint64_t)first_plus;
    uint64_t d1_carry = (uint64_t)d1_init;
    uint64_t l_sum = 0, l_nsel = 0;
    int64_t l_mn = INT64_MAX, l_mx = INT64_MIN;
    // Fixed-size window advance with a cross-window varint carry
    // (carry_u holds the carried low groups, carry_n its byte count), so
    // window addresses are induction variables.  The primary window is
    // 256 B with FOUR bytes per lane (one u32 load): when every varint is
    // 1-2 bytes — the dominant telemetry shape — each lane decodes up to
    // four values and one 32-bit scan covers 256 B, a quarter of the 64-B
    // window's per-byte instruction and load counts.  Windows that fail
    // the pattern (longer varints, walkers, delta-of-delta, the stream
    // tail, a multi-byte carry) take one 64-B window below: its 1-2-byte
    // fast shape, or the generic step.  Terminators past jmax (bytes of
    // the following stream / the part's slack) fold as zeros, so the
    // wave-wide scans read their totals at lane 63.
    uint64_t carry_u = 0;
    uint32_t carry_n = 0;
    const bool no_walk = pw0 == nullptr && pw1 == nullptr && pw2 == nullptr;
#define QLEAD 4
    uint32_t wq[QLEAD];  // wq[q] = this lane's u32 of the window at pos+256q
    bool done = false;
    while (j <= jmax) {
        // The quad path is a SELF-CONTAINED inner loop: with the 64-B
        // fallback in the same loop body, the compiler hoists the
        // fallback's byte load above the quad branch and fences it with
        // s_waitcnt vmcnt(0) — draining the whole QLEAD window pipeline
        // every iteration (measured: the scan ran at full memory latency
        // per 256-B window).  Inside this loop the only vector loads are
        // the window dwords, so the waits stay at vmcnt(QLEAD-1).
        if (!dod && no_walk && carry_n <= 1) {
            // pipeline fill: QLEAD windows in flight, then exactly ONE
            // load per steady-state iteration (at the bottom, QLEAD-1
            // windows ahead of its use)
#pragma unroll
            for (int q = 0; q < QLEAD; q++)
                __builtin_memcpy(&wq[q],
                                 stream + pos + 256 * (uint64_t)q +
                                     4 * (uint64_t)lane, 4);
            // Ring by PHASE, not by shifting: moving wq[q+1] into wq[q]
            // would make every iteration wait on the NEWEST outstanding
            // load (vmcnt(0) to read the register being shifted),
            // re-serialising the pipeline.  The unrolled phase loop keeps
            // indices static, so reading wq[ph] waits only for the load
            // issued QLEAD-1 iterations ago.
            bool quad_exit = false;
            while (!quad_exit) {
#pragma unroll
            for (int ph = 0; ph < QLEAD; ph++) {
            // 256-B quad window: FOUR bytes per lane (one u32 load), each
            // lane decoding up to four 1-2-byte varints; one 32-bit scan
            // covers 256 B.
            const uint32_t w_cur = wq[ph];
            uint32_t b0 = w_cur & 0xffu, b1 = (w_cur >> 8) & 0xffu,
                     b2 = (w_cur >> 16) & 0xffu, b3 = w_cur >> 24;
            uint64_t e0 = __ballot(b0 < 0x80);
            uint64_t e1 = __ballot(b1 < 0x80);
            uint64_t e2 = __ballot(b2 < 0x80);
            uint64_t e3 = __ballot(b3 < 0x80);
            uint64_t c0 = ~e0, c1 = ~e1, c2 = ~e2, c3 = ~e3;
            int nt = __popcll(e0) + __popcll(e1) + __popcll(e2) +
                     __popcll(e3);
            if (((c0 & c1) | (c1 & c2) | (c2 & c3)) == 0 &&
                (c3 & (c0 >> 1)) == 0 &&
                (int64_t)nt <= jmax - j + 1 &&
                (carry_n == 0 || (e0 & 1))) {
                // previous lane's b3 heads a value ending at my b0
                uint32_t pb3 = dpp_mov32<0x111>(b3);
                uint32_t q15 = (uint32_t)__builtin_amdgcn_readlane((int)b3, 15);
                uint32_t q31 = (uint32_t)__builtin_amdgcn_readlane((int)b3, 31);
                uint32_t q47 = (uint32_t)__builtin_amdgcn_readlane((int)b3, 47);
                if ((lane & 15) == 0 && lane)
                    pb3 = lane == 16 ? q15 : lane == 32 ? q31 : q47;
                if (lane == 0)
                    pb3 = carry_n ? ((uint32_t)carry_u | 0x80u) : 0;
                bool t0 = b0 < 0x80, t1 = b1 < 0x80, t2 = b2 < 0x80,
                     t3 = b3 < 0x80;
                uint32_t u0 = (pb3 & 0x80u) ? ((pb3 & 0x7fu) | (b0 << 7)) : b0;
                uint32_t u1 = (b0 & 0x80u) ? ((b0 & 0x7fu) | (b1 << 7)) : b1;
                uint32_t u2 = (b1 & 0x80u) ? ((b1 & 0x7fu) | (b2 << 7)) : b2;
                uint32_t u3 = (b2 & 0x80u) ? ((b2 & 0x7fu) | (b3 << 7)) : b3;
                int32_t dA = t0 ? ((int32_t)(u0 >> 1) ^ -(int32_t)(u0 & 1)) : 0;
                int32_t dB = t1 ? ((int32_t)(u1 >> 1) ^ -(int32_t)(u1 & 1)) : 0;
                int32_t dC = t2 ? ((int32_t)(u2 >> 1) ^ -(int32_t)(u2 & 1)) : 0;
                int32_t dD = t3 ? ((int32_t)(u3 >> 1) ^ -(int32_t)(u3 & 1)) : 0;
                int32_t sl = dA + dB + dC + dD;
                int32_t S = wave_incl_scan32(sl, lane);
                int32_t cum = S - sl;
                if (full || (j >= r0 && j + nt - 1 <= r1)) {
                    // whole window selected (the dominant shape once the
                    // block-level clamp resolved): no per-value index
                    // bookkeeping — every terminator folds
#define BYDB_QVF(tk, dk)                                                     \
                    if (tk) {                                                \
                        cum += dk;                                           \
                        int64_t sv =                                         \
                            (int64_t)(v_carry + (uint64_t)(int64_t)cum);     \
                        l_sum += (uint64_t)sv;                               \
                        l_mn = sv < l_mn ? sv : l_mn;                        \
                        l_mx = sv > l_mx ? sv : l_mx;                        \
                    }
                    BYDB_QVF(t0, dA)
                    BYDB_QVF(t1, dB)
                    BYDB_QVF(t2, dC)
                    BYDB_QVF(t3, dD)
#undef BYDB_QVF
                    l_nsel += (uint64_t)((int)t0 + (int)t1 + (int)t2 +
                                         (int)t3);
                } else {
                    int rb = __popcll(e0 & lanemask_lt(lane)) +
                             __popcll(e1 & lanemask_lt(lane)) +
                             __popcll(e2 & lanemask_lt(lane)) +
                             __popcll(e3 & lanemask_lt(lane));
                    int64_t idx = j + rb;
#define BYDB_QVAL(tk, dk)                                                    \
                    if (tk) {                                                \
                        cum += dk;                                           \
                        int64_t sv =                                         \
                            (int64_t)(v_carry + (uint64_t)(int64_t)cum);     \
                        if (idx >= r0 && idx <= r1) {                        \
                            l_sum += (uint64_t)sv;                           \
                            l_nsel++;                                        \
                            l_mn = sv < l_mn ? sv : l_mn;                    \
                            l_mx = sv > l_mx ? sv : l_mx;                    \
                        }                                                    \
                        idx++;                                               \
                    }
                    BYDB_QVAL(t0, dA)
                    BYDB_QVAL(t1, dB)
                    BYDB_QVAL(t2, dC)
                    BYDB_QVAL(t3, dD)
#undef BYDB_QVAL
                }
                v_carry +=
                    (uint64_t)(int64_t)__builtin_amdgcn_readlane(S, 63);
                if (e3 >> 63) {
                    carry_n = 0;
                    carry_u = 0;
                } else {
                    carry_n = 1;
                    carry_u = (uint64_t)(
                        (uint32_t)__builtin_amdgcn_readlane((int)b3, 63) &
                        0x7f);
                }
                j += nt;
                pos += 256;
                if (j > jmax) { done = true; quad_exit = true; break; }
                // refill this phase's slot with the window QLEAD-1 ahead
                __builtin_memcpy(&wq[ph],
                                 stream + pos + 256 * (uint64_t)(QLEAD - 1) +
                                     4 * (uint64_t)lane, 4);
                continue;
            }
            quad_exit = true;  // pattern failed: 64-B fallback below
            break;
            }        // phase loop
            }        // inner quad loop
            if (done) break;
        }
        uint8_t b = stream[pos + (uint64_t)lane];
        uint64_t emask = __ballot(b < 0x80);
        if (emask == 0) { dev_set_err(derr, DERR_BAD_STREAM, bi); break; }
        int rank = __popcll(emask & lanemask_lt(lane));
        int64_t myj = j + rank;
        bool is_term = (b < 0x80) && (myj <= jmax);
        int nterm = __popcll(emask);
        // fast window: every varint is 1 or 2 bytes (no two consecutive
        // continuation bits), not the tail window, and any carried byte
        // completes at lane 0 — decode via the left neighbour's byte
        // (shfl) and scan in 32-bit (window delta sums fit: <= 64 * 2^21)
        uint64_t cont = ~emask;
        if (pw0 == nullptr && pw1 == nullptr && pw2 == nullptr &&
            (cont & (cont << 1)) == 0 &&
            (int64_t)nterm <= jmax - j + 1 &&
            (carry_n == 0 || (carry_n == 1 && (emask & 1)))) {
            uint32_t prev = (uint32_t)__shfl_up((int)b, 1);
            bool is2 = lane > 0 && (prev & 0x80u);
            uint32_t u = is2 ? ((prev & 0x7fu) | ((uint32_t)b << 7)) : b;
            if (lane == 0 && carry_n)
                u = (uint32_t)carry_u | ((uint32_t)b << 7);
            int32_t d32 = (int32_t)(u >> 1) ^ -(int32_t)(u & 1);
            if (!(b < 0x80)) d32 = 0;          // continuation lanes carry 0
            int32_t s32 = wave_incl_scan32(d32, lane);
            uint64_t sv_u;
            if (dod) {
                // delta-of-delta in two 32-bit scans regardless of the
                // 64-bit d1 carry:  v_j = v_carry + cnt_j*d1_carry + t_j
                // with t_j = scan over terminators of (scan of d2)
                int32_t t32 = wave_incl_scan32((b < 0x80) ? s32 : 0, lane);
                sv_u = v_carry + (uint64_t)(int64_t)(rank + 1) * d1_carry +
                       (uint64_t)(int64_t)t32;
                int32_t t_tot = __builtin_amdgcn_readlane(t32, 63);
                int32_t s_tot = __builtin_amdgcn_readlane(s32, 63);
                v_carry += (uint64_t)(int64_t)nterm * d1_carry +
                           (uint64_t)(int64_t)t_tot;
                d1_carry += (uint64_t)(int64_t)s_tot;
            } else {
                sv_u = v_carry + (uint64_t)(int64_t)s32;
                v_carry += (uint64_t)(int64_t)__builtin_amdgcn_readlane(s32, 63);
            }
            if (b < 0x80) {
                int64_t sv = (int64_t)sv_u;
                if (full || (myj >= r0 && myj <= r1)) {
                    l_sum += (uint64_t)sv;
                    l_nsel++;
                    l_mn = sv < l_mn ? sv : l_mn;
                    l_mx = sv > l_mx ? sv : l_mx;
                }
            }
            if (emask >> 63) {
                carry_n = 0;
                carry_u = 0;
            } else {
                carry_n = 1;
                carry_u = (uint64_t)((uint32_t)__builtin_amdgcn_readlane((int)b, 63) & 0x7f);
            }
            j += nterm;
            pos += 64;
            continue;
        }
        // The generic step.  clamp_count_stream and dedup_decode_stream
        // hold the same lines from here to the carry-out: a codec fix goes
        // into all three (why they are not one routine yet:
        // profiles/varint_walk.txt).
        uint64_t d = 0;
        if (emask == ~0ull && carry_n == 0) {
            d = (uint64_t)zz_dec(b);
        } else {
            // assemble each terminator's varint from the bytes already in
            // registers: byte k back arrives by one __shfl_up at a
            // wave-uniform distance (trip count = longest in-window varint
            // from the widest terminator gap); the first terminator also
            // prepends the carried bytes.  LSB-first groups
            // (int.go:81-103): the byte k back holds bits (len-1-k)*7.
            uint64_t below = emask & lanemask_lt(lane);
            int start = below ? (64 - __clzll(below)) : 0;
            int mylen = lane - start + 1;        // in-window bytes
            if (mylen > 10) mylen = 10;  // valid varints are <=10 B; longer
                                         // gaps only occur on corrupt input
            // wave-uniform max varint length over terminator lanes
            int maxlen = (b < 0x80) ? mylen : 1;
            for (int off2 = 32; off2 > 0; off2 >>= 1) {
                int t = __shfl_xor(maxlen, off2);
                maxlen = t > maxlen ? t : maxlen;
            }
            uint64_t u = (uint64_t)(b & 0x7f) << (7 * (mylen - 1));
            for (int k = 1; k < maxlen; ++k) {
                uint32_t bk = (uint32_t)__shfl_up((int)b, k);
                if (k < mylen)
                    u |= (uint64_t)(bk & 0x7f) << (7 * (mylen - 1 - k));
            }
            if (below == 0 && carry_n)
                u = carry_u | (u << (7 * carry_n));
            if (is_term) d = (uint64_t)zz_dec(u);
        }
        if (!is_term) d = 0;
        uint64_t val;
        if (dod) {
            // first scan: d1_j = d1_carry + incl_scan(d2)
            uint64_t s1 = wave_incl_scan(d, lane);
            uint64_t d1j = is_term ? (d1_carry + s1) : 0;
            // second scan: v_j = v_carry + incl_scan(d1_j over values)
            uint64_t s2 = wave_incl_scan(d1j, lane);
            val = v_carry + s2;
            v_carry += readlane64(s2, 63);
            d1_carry += readlane64(s1, 63);
        } else {
            uint64_t sscan = wave_incl_scan(d, lane);
            val = v_carry + sscan;
            v_carry += readlane64(sscan, 63);
        }
        bool in_sel = is_term && (full || (myj >= r0 && myj <= r1));
        if (pw0) in_sel = pred_match_rows(pw0, myj, in_sel) && in_sel;
        if (pw1) in_sel = pred_match_rows(pw1, myj, in_sel) && in_sel;
        if (pw2) in_sel = pred_match_rows(pw2, myj, in_sel) && in_sel;
        if (in_sel) {
            int64_t sv = (int64_t)val;
            l_sum += val;
            l_nsel++;
            l_mn = sv < l_mn ? sv : l_mn;
            l_mx = sv > l_mx ? sv : l_mx;
        }
        if (j + nterm > jmax) break;
        // carry out: bytes after the last terminator head the next value
        int last_lane = 63 - __clzll(emask);
        int n_tail = 63 - last_lane;
        if (n_tail) {
            uint64_t tail = 0;
            if (lane > last_lane) {
                int sh2 = lane - last_lane - 1;
                if (sh2 > 9) sh2 = 9;        // corrupt-input guard
                tail = (uint64_t)(b & 0x7f) << (7 * sh2);
            }
            for (int off2 = 32; off2 > 0; off2 >>= 1)
                tail |= (uint64_t)__shfl_xor((long long)tail, off2);
            carry_u = tail;
            carry_n = n_tail > 9 ? 9 : (uint32_t)n_tail;
        } else {
            carry_u = 0;
            carry_n = 0;
        }
        j += nterm;
        pos += 64;
    }
    f->sum = l_sum;
    f->mn = l_mn;
    f->mx = l_mx;
    f->nsel = l_nsel;
}

// Count rows of a delta / delta-of-delta stream whose value falls below
// lo_bound (n_lo) or above hi_bound (n_hi) — all the FindRange clamp
// needs (range.go:143-170; ascending blocks).  This is the ONLY consumer
// of value bounds, kept OUT of scan_stream so the fold kernels (incl.
// the closed-form-only headline instantiation, which needs the clamp but
// not value folds) carry none of the scan's fast-window register state.
// Correctness path: it runs only on boundary blocks whose ts range
// partially overlaps the query; generic 64-B ballot windows.  Totals are
// wave-reduced; all lanes return them.
__device__ void clamp_count_stream(
    const uint8_t *stream, int64_t n_deltas,
                                   bool dod, int64_t first_plus,
                                   int64_t d1_init, int64_t lo_bound,
                                   int64_t hi_bound, int lane,
                                   uint64_t *out_nlo, uint64_t *out_nhi,
                                   DevErr *derr, uint64_t bi) {
    uint64_t pos = 0;
    int64_t j = dod ? 2 : 1;
    int64_t jmax = n_deltas;
    uint64_t v_carry = (uint64_t)first_plus;
    uint64_t d1_carry = (uint64_t)d1_init;
    uint64_t l_nlo = 0, l_nhi = 0;
    uint64_t carry_u = 0;
    uint32_t carry_n = 0;
    while (j <= jmax) {
        uint8_t b = stream[pos + (uint64_t)lane];
        uint64_t emask = __ballot(b < 0x80);
        if (emask == 0) { dev_set_err(derr, DERR_BAD_STREAM, bi); break; }
        int rank = __popcll(emask & lanemask_lt(lane));
        int64_t myj = j + rank;
        bool is_term = (b < 0x80) && (myj <= jmax);
        int nterm = __popcll(emask);
        uint64_t d = 0;
        if (emask == ~0ull && carry_n == 0) {
            d = (uint64_t)zz_dec(b);
        } else {
            uint64_t below = emask & lanemask_lt(lane);
            int start = below ? (64 - __clzll(below)) : 0;
            int mylen = lane - start + 1;
            if (mylen > 10) mylen = 10;
            int maxlen = (b < 0x80) ? mylen : 1;
            for (int off2 = 32; off2 > 0; off2 >>= 1) {
                int t = __shfl_xor(maxlen, off2);
                maxlen = t > maxlen ? t : maxlen;
            }
            uint64_t u = (uint64_t)(b & 0x7f) << (7 * (mylen - 1));
            for (int k = 1; k < maxlen; ++k) {
                uint32_t bk = (uint32_t)__shfl_up((int)b, k);
                if (k < mylen)
                    u |= (uint64_t)(bk & 0x7f) << (7 * (mylen - 1 - k));
            }
            if (below == 0 && carry_n)
                u = carry_u | (u << (7 * carry_n));
            if (is_term) d = (uint64_t)zz_dec(u);
        }
        if (!is_term) d = 0;
        uint64_t val;
        if (dod) {
            uint64_t s1 = wave_incl_scan(d, lane);
            uint64_t d1j = is_term ? (d1_carry + s1) : 0;
            uint64_t s2 = wave_incl_scan(d1j, lane);
            val = v_carry + s2;
            v_carry += readlane64(s2, 63);
            d1_carry += readlane64(s1, 63);
        } else {
            uint64_t sscan = wave_incl_scan(d, lane);
            val = v_carry + sscan;
            v_carry += readlane64(sscan, 63);
        }
        if (is_term) {
            int64_t sv = (int64_t)val;
            if (sv < lo_bound) l_nlo++;
            if (sv > hi_bound) l_nhi++;
        }
        if (j + nterm > jmax) break;
        int last_lane = 63 - __clzll(emask);
        int n_tail = 63 - last_lane;
        if (n_tail) {
            uint64_t tail = 0;
            if (lane > last_lane) {
                int sh2 = lane - last_lane - 1;
                if (sh2 > 9) sh2 = 9;
                tail = (uint64_t)(b & 0x7f) << (7 * sh2);
            }
            for (int off2 = 32; off2 > 0; off2 >>= 1)
                tail |= (uint64_t)__shfl_xor((long long)tail, off2);
            carry_u = tail;
            carry_n = n_tail > 9 ? 9 : (uint32_t)n_tail;
        } else {
            carry_u = 0;
            carry_n = 0;
        }
        j += nterm;
        pos += 64;
    }
    *out_nlo = wave_reduce_add(l_nlo);
    *out_nhi = wave_reduce_add(l_nhi);
}

// ---------------- the scan+aggregate kernel ----------------

enum {
    KF_NEED_VALUES = 1,  // min/max requested -> reconstruct values
    KF_FLOAT = 2,        // float64 field: also accumulate mantissa sum as double
                         // (bits 16-31 of flags carry the configured
                         // decimal exponent for the per-block guard)
    KF_WALK_ONLY = 4,    // process ONLY PF_WALK blocks (the heavy pass of
                         // the light/heavy predicate split below)
};

// What folding rows [a, b] of one block's field column gives.  sum is the
// wrapping sum (in a raw-float session: the bits of the double sum) and is
// wave-uniform, as are the rest.
struct RowFold {
    uint64_t sum;
    uint64_t cnt;       // rows folded: selected, matching and not null
    int64_t mn, mx;
    bool have_mm;       // mn/mx hold values
};

// How fold_rows reaches the dense one-byte Delta closed form.
enum {
    DENSE_CALL,         // the out-of-line dense_delta_weighted
    DENSE_INLINE,       // dense_delta_weighted_t inlined, whole block in flight
    DENSE_INLINE_NT,    // the same with non-temporal loads
};

// Fold rows [a, b] of a block's field column — the one field fold, for the
// scan kernel's [r0, r1] and for the sub-ranges of the grouped run merge.
// w0..w2: optional row-varying predicate walkers; rows must ascend, which
// they do within one call.  plain_norm: the host-normalized cells of a
// Plain block (nullptr when the block was not normalized).
// Compile-time: EN_VALUES — min/max reconstruction can be asked for at all;
// FULL — [a, b] is promised to cover every streamed row (scan_stream drops
// its selection branch); DENSE — see the enum above.
template <bool EN_VALUES, bool FULL, int DENSE>
__device__ __forceinline__ RowFold fold_rows(
    const uint8_t *fstream, const uint8_t *plain_norm, uint8_t fenc,
    int64_t first, uint64_t field_len, int64_t n, int64_t a, int64_t b,
    bool need_values, bool raw_f64, int lane, PredWalk *w0, PredWalk *w1,
    PredWalk *w2, DevErr *derr, uint64_t bi,
    const uint8_t *packed = nullptr) {
    need_values = EN_VALUES && need_values;
    const uint64_t nsel = (uint64_t)(b - a + 1);
    const bool pred_on = w0 || w1 || w2;
    RowFold f = {0, nsel, INT64_MAX, INT64_MIN, false};
    if (fenc == BYDB_ENC_PLAIN) {
        // null-bearing Plain column, host-normalized into the sidecar
        // ([u32 n][pad][validity bitmap][8-B sign-flip cells]): fold
        // valid selected rows, decoding cells in-lane
        // (convert/number.go:95-108); nulls drop from count and every
        // aggregate (aggregation.go:310).
        uint32_t nn = 0;
        if (plain_norm)
            nn = (uint32_t)plain_norm[0] | ((uint32_t)plain_norm[1] << 8) |
                 ((uint32_t)plain_norm[2] << 16) |
                 ((uint32_t)plain_norm[3] << 24);
        if (!plain_norm || nn != (uint32_t)n) {
            dev_set_err(derr, DERR_BAD_ENC, bi);
            f.cnt = 0;
            return f;
        }
        const uint64_t *vbm = (const uint64_t *)(plain_norm + 8);
        const uint64_t *cells = vbm + ((uint64_t)nn + 63) / 64;
        uint64_t lsum = 0, lcnt = 0;
        double lsumf = 0.0;
        int64_t lmn = INT64_MAX, lmx = INT64_MIN;
        for (int64_t base = a; base <= b; base += WAVE) {
            int64_t row = base + lane;
            bool ok = row <= b && ((vbm[row >> 6] >> (row & 63)) & 1);
            ok = walkers_match(w0, w1, w2, row, ok) && ok;
            if (ok) {
                // cells are big-endian on the wire
                uint64_t u = __builtin_bswap64(cells[row]);
                int64_t v;
                if (raw_f64) {
                    // IEEE-754 bits: double sum + ordered-bits min/max
                    // (Float64ToOrderedBytes map,
                    // convert/number.go:148-157)
                    double dv;
                    __builtin_memcpy(&dv, &u, 8);
                    lsumf += dv;
                    // order-preserving map INTO THE SIGNED domain
                    // (min/max compare as int64): positives keep raw
                    // bits, negatives flip magnitude and sign
                    v = (u >> 63) ? (int64_t)(~u ^ 0x8000000000000000ull)
                                  : (int64_t)u;
                } else {
                    v = (u >> 63) ? (int64_t)(u & ~(1ull << 63))
                                  : -(int64_t)((1ull << 63) - u);
                    lsum += (uint64_t)v;
                }
                lmn = v < lmn ? v : lmn;
                lmx = v > lmx ? v : lmx;
                lcnt++;
            }
        }
        if (raw_f64) {
            double ds = wave_reduce_addf(lsumf);
            __builtin_memcpy(&f.sum, &ds, 8);
        } else {
            f.sum = wave_reduce_add(lsum);
        }
        f.cnt = wave_reduce_add(lcnt);
        f.mn = wave_reduce_min(lmn);
        f.mx = wave_reduce_max(lmx);
        f.have_mm = f.cnt > 0;
        return f;
    }
    if (fenc == BYDB_ENC_CONST || fenc == BYDB_ENC_DELTA_CONST) {
        int64_t dd = 0;
        if (fenc == BYDB_ENC_DELTA_CONST) {
            int vl;
            dd = decode_one_varint(fstream, &vl);
        }
        if (pred_on) {
            // the closed forms cannot filter rows: predicated row walk
            uint64_t psum, pcnt;
            int64_t pmn, pmx;
            fold_arith_pred(first, dd, a, b, lane, w0, w1, w2, &psum, &pcnt,
                            &pmn, &pmx);
            f.sum = psum;
            f.cnt = pcnt;
            f.mn = pmn;
            f.mx = pmx;
            f.have_mm = need_values && pcnt > 0;
            return f;
        }
        // sum_{i=a..b}(first + i*dd) = nsel*first + dd * sum i
        uint64_t si = (uint64_t)(a + b) * nsel / 2;
        f.sum = (uint64_t)first * nsel + (uint64_t)dd * si;
        if (fenc == BYDB_ENC_CONST) {
            f.mn = f.mx = first;
            f.have_mm = true;
        } else if (need_values) {
            // reconstruct min/max exactly (wrap-safe): walk rows by lanes
            int64_t lmn = INT64_MAX, lmx = INT64_MIN;
            for (int64_t base = a; base <= b; base += WAVE) {
                int64_t i = base + lane;
                if (i <= b) {
                    int64_t v = (int64_t)((uint64_t)first +
                                          (uint64_t)i * (uint64_t)dd);
                    lmn = v < lmn ? v : lmn;
                    lmx = v > lmx ? v : lmx;
                }
            }
            f.mn = wave_reduce_min(lmn);
            f.mx = wave_reduce_max(lmx);
            f.have_mm = true;
        }
        return f;
    }
    if (fenc != BYDB_ENC_DELTA && fenc != BYDB_ENC_DELTA_OF_DELTA) {
        dev_set_err(derr, DERR_BAD_ENC, bi);
        f.cnt = 0;
        return f;
    }
    const bool dod = fenc == BYDB_ENC_DELTA_OF_DELTA;
    // stream length == delta count -> every varint is one byte
    const bool dense = !dod && field_len == (uint64_t)(n - 1);
    if (!pred_on && (!need_values || dense)) {
        // closed forms: the weighted folds include first (and d1)
        uint64_t acc;
        int64_t d1 = 0;
        if (dod) {
            int vl;
            d1 = decode_one_varint(fstream, &vl);
            acc = fold_dod_weighted(fstream + vl, n - 1, a, b, lane, derr, bi);
        } else if (!dense) {
            acc = fold_delta_weighted_fast(fstream, n - 1, a, b, lane, derr,
                                           bi);
        } else if (DENSE == DENSE_CALL || need_values) {
            acc = dense_delta_weighted(fstream, n - 1, a, b, lane);
        } else if (DENSE == DENSE_INLINE_NT && packed != nullptr && a == 0 &&
                   b == n - 1) {
            // whole block with a 4-bit copy: half the bytes
            acc = dense_packed_weighted(packed, (uint32_t)n, lane);
        } else {
            // dense dot4 fold, the whole block in flight
            acc = dense_delta_weighted_t<FULL ? DENSE_CHUNKS_BLOCK
                                              : DENSE_CHUNKS_CLAMP,
                                         DENSE == DENSE_INLINE_NT>(
                fstream, n - 1, a, b, lane);
        }
        // nsel*first + d1 * sum_{i=a..b} i + the weighted deltas
        uint64_t si = (uint64_t)(a + b) * nsel / 2;
        f.sum = (uint64_t)first * nsel + (uint64_t)d1 * si +
                wave_reduce_add(acc);
        if (need_values) {
            // dense min/max (no serial window chain):
            // v at row a = first + sum of bytes [0, a)
            int64_t psd, psjd;
            dense_region(fstream, 0, a, lane, &psd, &psjd);
            int64_t va = (int64_t)((uint64_t)first +
                                   wave_reduce_add((uint64_t)psd));
            dense_minmax(fstream, a, b, va, lane, &f.mn, &f.mx);
            f.mn = va < f.mn ? va : f.mn;  // row a itself
            f.mx = va > f.mx ? va : f.mx;
            f.have_mm = true;
        }
        return f;
    }
    // value scan (predicated, or min/max over multi-byte varints)
    const uint8_t *s = fstream;
    int64_t d1 = 0;
    if (dod) {
        int vl;
        d1 = decode_one_varint(s, &vl);
        s += vl;
    }
    const int64_t row1 = (int64_t)((uint64_t)first + (uint64_t)d1);
    uint64_t lsum = 0, lcnt = 0;
    int64_t lmn = INT64_MAX, lmx = INT64_MIN;
    // the rows the stream does not carry: row 0 (value first) and, for
    // delta-of-delta, row 1 (value row1)
    auto head_rows = [&]() {
        for (int64_t row = 0; row <= (dod ? 1 : 0); row++) {
            int64_t v = row ? row1 : first;
            bool need = lane == 0 && a <= row && row <= b;
            if (walkers_match(w0, w1, w2, row, need) && need) {
                lsum += (uint64_t)v;
                lcnt++;
                lmn = v < lmn ? v : lmn;
                lmx = v > lmx ? v : lmx;
            }
        }
    };
    // walker rows must ascend: under a predicate they come before the scan.
    // Otherwise after it, so that nothing is live across its window loop.
    if (pred_on) head_rows();
    ScanFold ff;
    scan_stream(s, n - 1, dod, dod ? row1 : first, d1, a, b, lane, &ff, derr,
                bi, w0, w1, w2, FULL);
    lsum += ff.sum;
    lmn = ff.mn < lmn ? ff.mn : lmn;
    lmx = ff.mx > lmx ? ff.mx : lmx;
    if (!pred_on) head_rows();
    f.sum = wave_reduce_add(lsum);
    f.mn = wave_reduce_min(lmn);
    f.mx = wave_reduce_max(lmx);
    f.have_mm = true;
    if (pred_on) {
        f.cnt = wave_reduce_add(lcnt + ff.nsel);
        f.have_mm = f.cnt > 0;
    }
    return f;
}

// The out-of-line instantiation, for the row-varying group-by run merge:
// sub-ranges of a block, so never FULL.  Out of line because the grouped
// kernels' register budget depends on it, and with the result behind a
// pointer: returned by value it costs those kernels 150-290 bytes of
// scratch each.  Only BITMAP-mode walkers
// (plain >256-card tag columns, k_resolve_plain) reach here: their
// stateless O(1) per-row lookups filter any sub-range, while the run merge
// intersects the runs of RLE walkers into [a, b] instead.
__device__ void fold_range(const uint8_t *fstream,
                              const uint8_t *plain_norm, uint8_t fenc,
                              int64_t first, uint64_t field_len, int64_t n,
                              int64_t a, int64_t b, bool need_values,
                              bool raw_f64, int lane, PredWalk *bw0,
                              PredWalk *bw1, PredWalk *bw2, DevErr *derr,
                              uint64_t bi, RowFold *out) {
    *out = fold_rows<true, false, DENSE_CALL>(fstream, plain_norm, fenc, first,
                                              field_len, n, a, b, need_values,
                                              raw_f64, lane, bw0, bw1, bw2,
                                              derr, bi);
}

// The per-wave partial: one group's running aggregates in registers.
// One atomic set per BLOCK on a single group serialises on one cacheline
// (~88 atomics/us on one word) and dominates the whole scan; instead block
// totals fold into these registers and flush only when the group changes
// or the wave is done.
// first: the (block << 13 | row) key where this wave first ENTERED the
// group (rows that pass predicates and map to the group, before the
// null-field check — matching where the reference's computeKey
// materialises a group, aggregation.go:523).  The global atomicMin over
// these keys is the group's first appearance in storage order, which is
// the reference's first-seen materialisation order (blocks iterate in
// (sid, minTs) order, rows ascend).  ~0 = no entry this flush.
struct WavePartial {
    int64_t group = -1;
    uint64_t sum = 0, cnt = 0;
    uint64_t first = ~0ull;
    int64_t mn = INT64_MAX, mx = INT64_MIN;
    double sumf = 0.0;

    __device__ __forceinline__ void flush(bydb_partial *partials,
                                          uint64_t *first_seen,
                                          int lane) const {
        if (group < 0 || lane != 0) return;
        bydb_partial *p = &partials[group];
        if (first_seen != nullptr && first != ~0ull)
            atomicMin((unsigned long long *)&first_seen[group],
                      (unsigned long long)first);
        if (sum) atomicAdd((unsigned long long *)&p->sum_i, (unsigned long long)sum);
        if (cnt) atomicAdd((unsigned long long *)&p->count, (unsigned long long)cnt);
        if (mn != INT64_MAX) atomicMin((long long *)&p->min_i, (long long)mn);
        if (mx != INT64_MIN) atomicMax((long long *)&p->max_i, (long long)mx);
        if (sumf != 0.0) atomicAdd(&p->sum_f, sumf);
    }

    // Merge one fold into group g, entered at `key`.  fdiff: the block's
    // decimal exponent above the session's (float sessions): min/max
    // mantissas rescale exactly by 10^fdiff, the sum by the same factor as
    // a double.  A mantissa that overflows the rescale is a device error;
    // the fold is then dropped whole (ovf_drops, returns false) or merged
    // without its min/max.
    __device__ __forceinline__ bool add(int64_t g, uint64_t key, RowFold f,
                                        int flags, int fdiff, bool raw_f64,
                                        bool ovf_drops, bydb_partial *partials,
                                        uint64_t *first_seen, int lane,
                                        DevErr *derr, uint64_t bi) {
        double fscale = 1.0;
        if ((flags & KF_FLOAT) && fdiff) {
            int64_t mfac = c_pow10i[fdiff];
            fscale = (double)mfac;
            if (f.have_mm) {
                int64_t smin, smax;
                if (__builtin_mul_overflow(f.mn, mfac, &smin) ||
                    __builtin_mul_overflow(f.mx, mfac, &smax)) {
                    dev_set_err(derr, DERR_EXP_MISMATCH, bi);
                    if (ovf_drops) return false;
                    f.have_mm = false;
                } else {
                    f.mn = smin;
                    f.mx = smax;
                }
            }
        }
        if (g != group) {
            flush(partials, first_seen, lane);
            *this = WavePartial();
            group = g;
            first = key;
        } else if (first == ~0ull) {
            first = key;
        }
        sum += f.sum;
        cnt += f.cnt;
        if (f.have_mm) {
            mn = f.mn < mn ? f.mn : mn;
            mx = f.mx > mx ? f.mx : mx;
        }
        if (flags & KF_FLOAT) {
            if (raw_f64) {
                double db;
                __builtin_memcpy(&db, &f.sum, 8);
                sumf += db;
            } else {
                sumf += (double)(int64_t)f.sum * fscale;
            }
        }
        return true;
    }
};

// Compile-time specialization: the FAST instantiation (no value
// reconstruction, no predicates) sheds the scan/walker machinery and its
// register pressure; the full one keeps everything.  (EN_* are constant
// guards — dead branches are eliminated per instantiation.)
//
// EN_WALK — the light/heavy predicate split.  Row-varying predicate
// walkers (PredWalk x3, ~300 B of per-lane state) force scratch spills
// into the value-scan hot loop even when every block resolves to a
// uniform verdict (entity tags — the dominant case).  With predicates
// the host launches TWO passes on the same stream: a light kernel
// (EN_WALK=false) that folds every PF_CLEAR/PF_SKIP block and skips
// PF_WALK ones, carrying no walker state at all, then a heavy kernel
// (EN_WALK=true, flags & KF_WALK_ONLY) that folds only the PF_WALK
// blocks.  When no block needs a walker the heavy pass is a ~flag-byte
// sweep.
// EN_CLAMP — compile the FindRange row clamp only when the query's
// [min_ts, max_ts] does NOT already cover the whole resident part (the
// host tracks the part's ts extent and selects the instantiation).  The
// clamp's scan machinery otherwise inflates register pressure enough to
// spill scratch reloads into the dense fold loop (~7% on the headline).
// EN_STREAM — the closed-form instantiations only: the dense fold reads
// its chunks with non-temporal loads (dense_region_t).  The host picks it
// per pass from the session's stream-load policy.  These instantiations
// also read the nibble-packed copy of a block where `pack` has one, for a
// block folded whole; a block cut by the clamp folds from its byte stream.
template <bool EN_VALUES, bool EN_PREDS, bool EN_GROUPS, bool EN_WALK,
          bool EN_CLAMP, bool EN_STREAM = false>
// Occupancy: 4 waves/SIMD for the value-scan instantiations — requesting
// 6 forces scratch spills into the window loop and measured ~1.6x SLOWER.
// Occupancy: the clamp-free value-scan instantiations (the analytic
// full-range f64/min-max path) run at EIGHT waves/SIMD — swept 4..8 on
// hardware twice: 7 won before the compile-time full-range flag
// (6.40 -> 5.67 ms on configs[2]), 8 wins after it shed the selection
// branch's registers (-> ~5.25 ms); the extra waves hide the decode's
// dependency bubbles and the VGPR-spill cost stays below the win.  The
// other instantiations keep 4 (more state: clamp / groups).  So do the
// closed-form-only ones since the dense fold keeps a whole block (nine
// 16-byte loads per lane) in flight per wave: 16 waves/CU already hold
// ~144 KiB in flight, and 128 VGPRs leave the full-range one with no
// scratch.  Swept on hardware, headline kernel ms, two runs each:
// 4 waves 1.90/1.97, 6 waves 2.27/2.27 (32 B scratch), 8 waves 3.73/3.76
// (256 B scratch) — profiles/dense_wide_loads.txt.
// The predicate light pass without clamp (<0,1,0,0,0>) asks for 5: it
// skips most blocks on a flag byte and is bound by per-item latency; at
// 100 VGPRs / 4 waves it measured 15% slower than at 95 / 5 on the
// group4096_pred3 and mixed workloads.
__global__ __launch_bounds__(256, (EN_VALUES && !EN_CLAMP && !EN_GROUPS) ? 8 : (!EN_VALUES && EN_PREDS && !EN_GROUPS && !EN_WALK && !EN_CLAMP) ? 5 : 4) void k_scan_agg_t(
    const uint8_t *__restrict__ payload, const uint8_t *__restrict__ sidecar,
    const bydb_block_desc *__restrict__ blocks,
    int64_t n_blocks, int64_t min_ts, int64_t max_ts, int flags,
    const PredBlock *__restrict__ preds_in, int n_preds,
    const uint64_t *__restrict__ pred_bm,
    const uint8_t *__restrict__ pred_flags,
    const GroupBlock *__restrict__ groups_in,
    const uint16_t *__restrict__ gmap_in,
    const uint16_t *__restrict__ gruns_in, int n_gslots, int64_t gm0,
    int64_t gm1, int64_t gm2, int64_t n_groups,
    bydb_partial *__restrict__ partials, DevErr *derr,
    const uint32_t *__restrict__ walk_count,
    uint64_t *__restrict__ first_seen, const uint8_t *__restrict__ pack) {
    // heavy pass with no PF_WALK blocks anywhere: one scalar load, done
    if ((flags & KF_WALK_ONLY) && walk_count != nullptr &&
        *walk_count == 0)
        return;
    const int64_t gmul[3] = {gm0, gm1, gm2};
    const PredBlock *preds = EN_PREDS ? preds_in : nullptr;
    const GroupBlock *groups = EN_GROUPS ? groups_in : nullptr;
    const int lane = threadIdx.x & 63;
    // In the closed-form instantiations (no value reconstruction, tag
    // predicates or tag group-by) the per-item preamble is wave-uniform:
    // the wave index goes through readfirstlane, so the item index and the
    // descriptor live in scalar registers and the descriptor is fetched by
    // scalar loads (descriptors are written by host copies before the
    // launch, so the read-only scalar cache is safe for them).  The
    // packed-slot table at the head of `pack` goes the same way although a
    // kernel wrote it (k_pack_fields): that kernel ran in an EARLIER launch
    // on this stream, and the scalar cache holds nothing across a launch
    // boundary, so no entry can be read stale.
    // Not with EN_GROUPS: the run-merge state leaves no scalar registers
    // for two descriptors, and what spills there lands in scratch.  Not
    // with EN_PREDS: a skipped block costs one flag byte there, and
    // fetching every descriptor ahead measured 5% slower on the mixed
    // workload (profiles/dense_wide_loads.txt).
    constexpr bool UNI_DESC = !EN_VALUES && !EN_PREDS && !EN_GROUPS;
    const int wave_in_block =
        UNI_DESC ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))
                 : (int)(threadIdx.x >> 6);
    int64_t wave_id = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave_in_block;
    int64_t n_waves = (int64_t)gridDim.x * (blockDim.x >> 6);

    WavePartial part;   // flushed on group change / at the end

    // The work item is a block: one wave scans a whole block.
    // Strided assignment (not contiguous ranges): predicates skip blocks
    // in long runs, and contiguous ranges turn those runs into idle waves.
    // UNI_DESC: the descriptor of the block after this one is requested at
    // the top of each iteration and consumed only when the loop advances,
    // so its latency hides behind the current block's fold; a block pays
    // no descriptor round trip after the wave's first.
    // (Both stay unused, and vanish, in the other instantiations.)
    bydb_block_desc d_cur = {}, d_nxt = {};
    // PACKED: the block's entry of the packed-slot table (0: no 4-bit copy,
    // else the slot's offset from `pack` in 128-byte units) travels with
    // the descriptor, one block ahead.  pack is null when nothing is packed.
    constexpr bool PACKED = UNI_DESC && EN_STREAM;
    const uint32_t *pack_off = (const uint32_t *)pack;
    uint32_t po_cur = 0, po_nxt = 0;
    if (UNI_DESC && wave_id < n_blocks) {
        d_nxt = blocks[wave_id];
        if (PACKED && pack != nullptr) po_nxt = pack_off[wave_id];
    }
    for (int64_t bi = wave_id; bi < n_blocks; bi += n_waves) {
        if (UNI_DESC) {
            d_cur = d_nxt;   // requested one iteration ago
            // clamped to the last block, so the request is unconditional
            int64_t nx = bi + n_waves < n_blocks ? bi + n_waves : n_blocks - 1;
            d_nxt = blocks[nx];
            if (PACKED && pack != nullptr) {
                po_cur = po_nxt;
                po_nxt = pack_off[nx];
            }
        }
        // otherwise: issue the independent per-lane loads (descriptor,
        // predicate flag) back-to-back ahead of their first use
        const bydb_block_desc *bd = UNI_DESC ? &d_cur : &blocks[bi];
        const uint8_t pf_pre =
            (EN_PREDS && preds != nullptr) ? pred_flags[bi] : PF_CLEAR;
        // light/heavy split routing (see the template comment): the heavy
        // pass owns exactly the PF_WALK blocks, the light pass everything
        // else — checked before any clamp work so the off-pass blocks
        // cost one flag byte
        if (EN_PREDS && preds != nullptr) {
            if (flags & KF_WALK_ONLY) {
                if (pf_pre != PF_WALK) continue;
            } else if (!EN_WALK && pf_pre == PF_WALK) {
                continue;
            }
        }
        const int64_t n = (int64_t)bd->count;
        const int64_t ts_min = bd->ts_min, ts_max = bd->ts_max;
        // float64 blocks fold in the decimal-int domain; a block whose
        // exponent EXCEEDS the session's rescales its partials by
        // 10^(block_exp - cfg_exp) at the merge below (exact for the
        // monotone min/max mantissas; the sum factor is a double).  The
        // session exponent must be the part's minimum exponent — a block
        // BELOW it cannot be represented and errors loudly.
        int fdiff = 0;
        bool raw_f64 = false;
        if (flags & KF_FLOAT) {
            int16_t cfge = (int16_t)(uint16_t)((uint32_t)flags >> 16);
            if (cfge == INT16_MIN) {
                // raw-float session (nullable f64, IEEE-754 cells):
                // every block must be a Plain cell block
                raw_f64 = true;
                if (bd->field_enc != BYDB_ENC_PLAIN) {
                    dev_set_err(derr, DERR_EXP_MISMATCH, (uint64_t)bi);
                    continue;
                }
            } else if (bd->field_enc == BYDB_ENC_PLAIN) {
                // raw cells inside a decimal session: domains clash
                dev_set_err(derr, DERR_EXP_MISMATCH, (uint64_t)bi);
                continue;
            } else {
                fdiff = (int)bd->exp - (int)cfge;
                if (fdiff < 0 || fdiff > 18) {
                    dev_set_err(derr, DERR_EXP_MISMATCH, (uint64_t)bi);
                    continue;
                }
                // mantissa-sum overflow guard: the engine
                // carries each block's decimal-int mantissa sum in int64
                // (exact, then one double convert); the reference's
                // per-row float64 adds never wrap.  A block whose
                // |firstValue| alone implies the sum exceeds int64
                // (|mean| > 2^63/8192 ~ 1.1e15 — the realistic overflow
                // mode is a large baseline) errs loudly instead of
                // returning a silently wrong sum.  Delta-driven escapes
                // from a small firstValue remain a documented limit.
                uint64_t afirst = bd->field_first < 0
                                      ? (uint64_t)(-(uint64_t)bd->field_first)
                                      : (uint64_t)bd->field_first;
                if (afirst > (1ull << 63) / (uint64_t)(bd->count + 1u)) {
                    dev_set_err(derr, DERR_F64_SUM_OVF, (uint64_t)bi);
                    continue;
                }
            }
        }

        // ---- row clamp (timestamp.FindRange, range.go:143-170) ----
        int64_t r0 = 0, r1 = n - 1;
        if (ts_min > ts_max) { dev_set_err(derr, DERR_DESC_TS, (uint64_t)bi); continue; }
        if (EN_CLAMP && !(min_ts <= ts_min && max_ts >= ts_max)) {
            if (ts_min > max_ts || ts_max < min_ts) continue;  // no overlap
            uint8_t tenc = bd->ts_enc_with_version;
            // common type (encoding.GetCommonType)
            uint8_t tc = tenc >= BYDB_ENC_CONST_WV && tenc <= BYDB_ENC_DELTA_OF_DELTA_WV
                             ? tenc - 4 : tenc;
            const uint8_t *tstream = payload + bd->ts_off;
            if (tc == BYDB_ENC_CONST) {
                // all == ts_min; overlap already implies in-range
            } else if (tc == BYDB_ENC_DELTA_CONST) {
                int vl;
                int64_t dd = decode_one_varint(tstream, &vl);
                if (dd <= 0) { dev_set_err(derr, DERR_DESC_TS, (uint64_t)bi); continue; }
                // first i with ts_min + i*dd >= min_ts
                if (min_ts > ts_min)
                    r0 = (min_ts - ts_min + dd - 1) / dd;
                if (max_ts < ts_max)
                    r1 = (max_ts - ts_min) / dd;
                if (r1 > n - 1) r1 = n - 1;
            } else if (tc == BYDB_ENC_DELTA || tc == BYDB_ENC_DELTA_OF_DELTA) {
                bool dod = tc == BYDB_ENC_DELTA_OF_DELTA;
                const uint8_t *s = tstream;
                int64_t d1 = 0;
                int64_t vfirst = ts_min;
                if (dod) {
                    int vl;
                    d1 = decode_one_varint(s, &vl);
                    s += vl;
                }
                int64_t row1 = (int64_t)((uint64_t)ts_min + (uint64_t)d1);
                uint64_t nlo, nhi;
                clamp_count_stream(s, n - 1, dod, dod ? row1 : vfirst, d1,
                                   min_ts, max_ts, lane, &nlo, &nhi, derr,
                                   (uint64_t)bi);
                // rows 0 (and 1 for dod) were not in the stream
                if (ts_min < min_ts) nlo++;
                if (ts_min > max_ts) nhi++;
                if (dod) {
                    if (row1 < min_ts) nlo++;
                    if (row1 > max_ts) nhi++;
                }
                r0 = (int64_t)nlo;
                r1 = n - 1 - (int64_t)nhi;
            }
            if (r0 > r1) continue;
        }

        // ---- per-row tag predicates (conjunctive, dictionary codes) ----
        // One combined flag byte decides the common cases; only PF_WALK
        // blocks pay for walker setup.
        PredWalk pw0, pw1, pw2;
        PredWalk *wp0 = nullptr, *wp1 = nullptr, *wp2 = nullptr;
        if (preds != nullptr) {
            const uint8_t pf = pf_pre;
            if (pf == PF_SKIP) continue;
            if (pf == PF_ERR) {
                dev_set_err(derr, DERR_BAD_ENC, (uint64_t)bi);
                continue;
            }
            if (EN_WALK && pf == PF_WALK) {
                bool skip_block = false;
#pragma unroll
                for (int sl = 0; sl < 3; sl++) {
                    if (sl >= n_preds || skip_block) continue;
                    PredBlock pb = preds[(int64_t)sl * n_blocks + bi];
                    if (pb.disabled) continue;   // empty slot: no constraint
                    if (!pb.active) { skip_block = true; continue; }
                    PredWalk *w = sl == 0 ? &pw0 : sl == 1 ? &pw1 : &pw2;
                    pred_init(w, payload, sidecar, &pb, pred_bm);
                    if (pb.uniform) {
                        // block-uniform slot inside a varying conjunction
                        pred_advance(w);
                        if (!w->run_match) skip_block = true;
                        // uniform + match: walker dropped, slot is a no-op
                    } else {
                        if (sl == 0) wp0 = w;
                        else if (sl == 1) wp1 = w;
                        else wp2 = w;
                    }
                }
                if (skip_block) continue;
            }
            // PF_CLEAR: every slot uniform-match -> fold unpredicated
        }

        // ---- per-row group-by on dictionary tags (EN_GROUPS) ----
        // Composite keys over up to 3 tag slots: gid = g0 + n0*g1 +
        // n0*n1*g2 (computeKey's multi-component key, aggregation.go:523).
        // All-uniform blocks (entity tags) take the fast fold paths; any
        // row-varying slot folds per intersection of the RLE runs.
        int64_t block_group = (int64_t)bd->group_code;
        if (!EN_GROUPS && block_group >= n_groups) {
            dev_set_err(derr, DERR_GROUP_RANGE, (uint64_t)bi);
            continue;
        }
        if (EN_GROUPS && groups) {
            GroupBlock gb[3];
            bool varying = false, skip_blk = false, errd = false;
            for (int sl = 0; sl < n_gslots; sl++) {
                gb[sl] = groups[(int64_t)sl * n_blocks + bi];
                if (gb[sl].err) errd = true;
                else if (gb[sl].uniform_gid == GID_NONE) skip_blk = true;
                else if (gb[sl].uniform_gid == GID_VARYING) varying = true;
            }
            if (errd) { dev_set_err(derr, DERR_BAD_ENC, (uint64_t)bi); continue; }
            if (skip_blk) continue;   // nil/unmapped on a grouped slot
            if (!varying) {
                block_group = 0;
                for (int sl = 0; sl < n_gslots; sl++)
                    block_group += (int64_t)gb[sl].uniform_gid * gmul[sl];
            } else {
                // row-varying predicates join the run merge below:
                // RLE walkers as additional run cursors; BITMAP-mode
                // (plain-tag) walkers have no runs, so they filter
                // per-row inside the fold instead (stateless O(1)
                // lookups — heavy-pass (EN_WALK) instantiations only)
                PredWalk *bw0 = nullptr, *bw1 = nullptr, *bw2 = nullptr;
                if (EN_WALK) {
                    if (wp0 && wp0->bm) { bw0 = wp0; wp0 = nullptr; }
                    if (wp1 && wp1->bm) { bw1 = wp1; wp1 = nullptr; }
                    if (wp2 && wp2->bm) { bw2 = wp2; wp2 = nullptr; }
                }
                const uint8_t *gstream = payload + bd->field_off;
                const uint8_t *plain_norm =
                    (bd->field_enc == BYDB_ENC_PLAIN &&
                     (bd->field_off & TAG_SIDECAR_BIT))
                        ? sidecar + (bd->field_off & ~TAG_SIDECAR_BIT)
                        : nullptr;
                // per-slot run cursors (uniform slots are one infinite
                // run); plain slots (width 0xFF) walk (gid,count) u16
                // pairs from the run arena instead of bit-packed RLE
                const uint8_t *gsrc[3];
                uint64_t bit[3];
                uint32_t ent[3];
                int64_t run_hi_s[3];
                int64_t gid_s[3];
                bool bad_plain = false;
                for (int sl = 0; sl < n_gslots; sl++) {
                    gsrc[sl] = (gb[sl].rle_bit_off & TAG_SIDECAR_BIT)
                                   ? sidecar : payload;
                    if (gb[sl].uniform_gid != GID_VARYING) {
                        gid_s[sl] = (int64_t)gb[sl].uniform_gid;
                        run_hi_s[sl] = n;
                        ent[sl] = gb[sl].nentries;  // exhausted
                        bit[sl] = 0;
                    } else {
                        if (gb[sl].width == 0xFF && gb[sl].nentries == 0)
                            bad_plain = true;  // resolve pass never ran
                        bit[sl] = gb[sl].rle_bit_off & ~TAG_SIDECAR_BIT;
                        ent[sl] = 0;
                        run_hi_s[sl] = 0;
                        gid_s[sl] = -1;
                    }
                }
                if (bad_plain) {
                    dev_set_err(derr, DERR_BAD_ENC, (uint64_t)bi);
                    continue;
                }
                auto advance = [&](int sl) {
                    if (ent[sl] + 1 >= gb[sl].nentries) {
                        run_hi_s[sl] = n;
                        gid_s[sl] = -1;  // RLE exhausted: no group
                        return;
                    }
                    if (gb[sl].width == 0xFF) {
                        const uint16_t *rp = gruns_in + gb[sl].rle_bit_off;
                        uint16_t g16 = rp[ent[sl]];
                        uint16_t cnt16 = rp[ent[sl] + 1];
                        ent[sl] += 2;
                        gid_s[sl] = g16 == 0xFFFFu ? -1 : (int64_t)g16;
                        run_hi_s[sl] += (int64_t)cnt16;
                        return;
                    }
                    uint64_t code = rd_bits_be(gsrc[sl], bit[sl], gb[sl].width);
                    bit[sl] += gb[sl].width;
                    uint64_t cnt = rd_bits_be(gsrc[sl], bit[sl], gb[sl].width);
                    bit[sl] += gb[sl].width;
                    ent[sl] += 2;
                    uint16_t m = (gmap_in + gb[sl].map_off)[code < 256 ? code : 0];
                    gid_s[sl] = m == 0xFFFFu ? -1 : (int64_t)m;
                    run_hi_s[sl] += (int64_t)cnt;
                };
                for (int sl = 0; sl < n_gslots; sl++)
                    if (gb[sl].uniform_gid == GID_VARYING) advance(sl);
                int64_t lo = 0;
                while (lo < n) {
                    // predicate cursors advance lazily to cover `lo`
                    if (wp0) while (wp0->run_hi <= lo) pred_advance(wp0);
                    if (wp1) while (wp1->run_hi <= lo) pred_advance(wp1);
                    if (wp2) while (wp2->run_hi <= lo) pred_advance(wp2);
                    int64_t hi = n;
                    for (int sl = 0; sl < n_gslots; sl++)
                        hi = run_hi_s[sl] < hi ? run_hi_s[sl] : hi;
                    if (wp0 && wp0->run_hi < hi) hi = wp0->run_hi;
                    if (wp1 && wp1->run_hi < hi) hi = wp1->run_hi;
                    if (wp2 && wp2->run_hi < hi) hi = wp2->run_hi;
                    int64_t aa = lo > r0 ? lo : r0;
                    int64_t bb2 = (hi - 1) < r1 ? (hi - 1) : r1;
                    int64_t comp = 0;
                    bool ok = true;
                    for (int sl = 0; sl < n_gslots; sl++) {
                        if (gid_s[sl] < 0) ok = false;
                        else comp += gid_s[sl] * gmul[sl];
                    }
                    if (wp0) ok = ok && wp0->run_match;
                    if (wp1) ok = ok && wp1->run_match;
                    if (wp2) ok = ok && wp2->run_match;
                    if (ok && aa <= bb2) {
                        RowFold rf;
                        fold_range(
                            gstream, plain_norm, bd->field_enc,
                            bd->field_first, bd->field_len, n, aa, bb2,
                            EN_VALUES && (flags & KF_NEED_VALUES), raw_f64,
                            lane, bw0, bw1, bw2, derr, (uint64_t)bi, &rf);
                        part.add(comp, ((uint64_t)bi << 13) | (uint64_t)aa, rf,
                                 flags, fdiff, raw_f64, false, partials,
                                 first_seen, lane, derr, (uint64_t)bi);
                    }
                    for (int sl = 0; sl < n_gslots; sl++)
                        if (run_hi_s[sl] == hi && gb[sl].uniform_gid == GID_VARYING)
                            advance(sl);
                    if (hi <= lo) break;  // safety against stuck cursors
                    lo = hi;
                }
                continue;
            }
        }

        // ---- field fold ----
        const uint8_t fenc = bd->field_enc;
        const uint8_t *plain_norm =
            (fenc == BYDB_ENC_PLAIN && (bd->field_off & TAG_SIDECAR_BIT))
                ? sidecar + (bd->field_off & ~TAG_SIDECAR_BIT)
                : nullptr;
        const RowFold bf =
            fold_rows<EN_VALUES, !EN_CLAMP,
                      !UNI_DESC ? DENSE_CALL
                                : EN_STREAM ? DENSE_INLINE_NT : DENSE_INLINE>(
                payload + bd->field_off, plain_norm, fenc, bd->field_first,
                bd->field_len, n, r0, r1, (flags & KF_NEED_VALUES) != 0,
                raw_f64, lane, wp0, wp1, wp2, derr, (uint64_t)bi,
                (PACKED && po_cur != 0)
                    ? pack + (uint64_t)po_cur * PACK_SLOT_ALIGN
                    : nullptr);
        // a rescale overflow drops the block
        part.add(block_group, ((uint64_t)bi << 13) | (uint64_t)r0, bf, flags,
                 fdiff, raw_f64, true, partials, first_seen, lane, derr,
                 (uint64_t)bi);
    }
    part.flush(partials, first_seen, lane);
}

// ---------------- cross-part version dedup ----------------
// The reference's measure query merges the block cursors of every part
// through a heap: for equal (seriesID, timestamp) queryResult.Less orders
// versions descending and queryResult.merge keeps the first row, replacing
// it only by a later row of greater version (banyand/measure/
// query.go:913-943, 966-1026).  Exactly one row per (series, timestamp)
// survives: the one with the highest version.  The order of equal versions
// is arbitrary there (heap order of equal keys); here the row of the
// EARLIEST APPENDED block wins.
//
// Which rows survive depends on the resident part only, so it is computed
// once per part (dedup_build): the host plans which blocks overlap
// (bydb_row_dedup_peers), k_dedup_decode materialises the stream-coded
// timestamps / versions of those blocks, k_dedup_mark writes a survivor
// bitmap per block.  Per consume k_dedup_apply folds the bitmaps into the
// verdicts, masks and bitmaps the resolve stage wrote, so the scan kernel
// sees nothing new: a fully superseded block is PF_SKIP, a partially
// superseded one a row-bitmap predicate on slot 0.
#define DD_TS_CONST 0    // every row at ts_min
#define DD_TS_ARITH 1    // ts_min + row * dd (DeltaConst)
#define DD_TS_ARENA 2    // decoded rows in the arena
#define DD_NO_ARENA (~0ull)

// One block that overlaps another block of its series ("involved").
struct DedupInfo {
    uint32_t block;       // block index in append order
    uint32_t count;
    int64_t ts_min, ts_max;
    int64_t dd;           // DD_TS_ARITH stride (written by k_dedup_decode)
    int64_t ver_first;
    uint64_t ts_arena;    // first arena row of the timestamps (DD_TS_ARENA)
    uint64_t ver_arena;   // first arena row of the versions, DD_NO_ARENA
                          // when the version is Const (= ver_first)
    uint32_t ts_kind;     // DD_TS_*
    uint32_t _p;
};

// counters of the mark stage
#define DD_CTR_PARTIAL 1
#define DD_CTR_FULL 2
#define DD_CTR_ROWS 3

// Decode a delta / delta-of-delta varint stream into out[row] — the window
// walk of clamp_count_stream, storing every value instead of counting.
// Rows 0 (and 1 for dod) are the caller's.  Every 64-byte window is checked
// against `avail`, the bytes readable from `stream` on; asc: a negative
// step is a descending timestamp list (the reference never writes one).
__device__ void dedup_decode_stream(const uint8_t *stream, uint64_t avail,
                                    int64_t n_deltas, bool dod,
                                    int64_t first_plus, int64_t d1_init,
                                    bool asc, int lane, int64_t *out,
                                    DevErr *derr, uint64_t bi) {
    uint64_t pos = 0;
    int64_t j = dod ? 2 : 1;
    int64_t jmax = n_deltas;
    uint64_t v_carry = (uint64_t)first_plus;
    uint64_t d1_carry = (uint64_t)d1_init;
    uint64_t carry_u = 0;
    uint32_t carry_n = 0;
    while (j <= jmax) {
        if (pos + 64 > avail) { dev_set_err(derr, DERR_BAD_STREAM, bi); break; }
        uint8_t b = stream[pos + (uint64_t)lane];
        uint64_t emask = __ballot(b < 0x80);
        if (emask == 0) { dev_set_err(derr, DERR_BAD_STREAM, bi); break; }
        int rank = __popcll(emask & lanemask_lt(lane));
        int64_t myj = j + rank;
        bool is_term = (b < 0x80) && (myj <= jmax);
        int nterm = __popcll(emask);
        uint64_t d = 0;
        if (emask == ~0ull && carry_n == 0) {
            d = (uint64_t)zz_dec(b);
        } else {
            uint64_t below = emask & lanemask_lt(lane);
            int start = below ? (64 - __clzll(below)) : 0;
            int mylen = lane - start + 1;
            if (mylen > 10) mylen = 10;
            int maxlen = (b < 0x80) ? mylen : 1;
            for (int off2 = 32; off2 > 0; off2 >>= 1) {
                int t = __shfl_xor(maxlen, off2);
                maxlen = t > maxlen ? t : maxlen;
            }
            uint64_t u = (uint64_t)(b & 0x7f) << (7 * (mylen - 1));
            for (int k = 1; k < maxlen; ++k) {
                uint32_t bk = (uint32_t)__shfl_up((int)b, k);
                if (k < mylen)
                    u |= (uint64_t)(bk & 0x7f) << (7 * (mylen - 1 - k));
            }
            if (below == 0 && carry_n)
                u = carry_u | (u << (7 * carry_n));
            if (is_term) d = (uint64_t)zz_dec(u);
        }
        if (!is_term) d = 0;
        uint64_t val;
        bool desc;
        if (dod) {
            uint64_t s1 = wave_incl_scan(d, lane);
            uint64_t d1j = is_term ? (d1_carry + s1) : 0;
            uint64_t s2 = wave_incl_scan(d1j, lane);
            val = v_carry + s2;
            v_carry += readlane64(s2, 63);
            d1_carry += readlane64(s1, 63);
            desc = (int64_t)d1j < 0;
        } else {
            uint64_t sscan = wave_incl_scan(d, lane);
            val = v_carry + sscan;
            v_carry += readlane64(sscan, 63);
            desc = (int64_t)d < 0;
        }
        if (asc && __any(is_term && desc)) {
            dev_set_err(derr, DERR_DESC_TS, bi);
            break;
        }
        if (is_term) out[myj] = (int64_t)val;
        if (j + nterm > jmax) break;
        int last_lane = 63 - __clzll(emask);
        int n_tail = 63 - last_lane;
        if (n_tail) {
            uint64_t tail = 0;
            if (lane > last_lane) {
                int sh2 = lane - last_lane - 1;
                if (sh2 > 9) sh2 = 9;
                tail = (uint64_t)(b & 0x7f) << (7 * sh2);
            }
            for (int off2 = 32; off2 > 0; off2 >>= 1)
                tail |= (uint64_t)__shfl_xor((long long)tail, off2);
            carry_u = tail;
            carry_n = n_tail > 9 ? 9 : (uint32_t)n_tail;
        } else {
            carry_u = 0;
            carry_n = 0;
        }
        j += nterm;
        pos += 64;
    }
}

// One int64 list of `n` values (first value `first`, stream at payload +
// off) decoded into out[0..n).  DeltaConst lists are expanded, Const lists
// never get here.
__device__ void dedup_decode_list(const uint8_t *payload, uint64_t off,
                                  uint64_t limit, uint8_t enc, int64_t first,
                                  int64_t n, bool asc, int lane, int64_t *out,
                                  DevErr *derr, uint64_t bi) {
    if (off + 11 > limit) { dev_set_err(derr, DERR_BAD_STREAM, bi); return; }
    const uint8_t *s = payload + off;
    if (lane == 0) out[0] = first;
    if (n < 2) return;
    if (enc == BYDB_ENC_DELTA_CONST) {
        int vl;
        int64_t dd = decode_one_varint(s, &vl);
        for (int64_t i = 1 + lane; i < n; i += WAVE)
            out[i] = (int64_t)((uint64_t)first + (uint64_t)i * (uint64_t)dd);
        return;
    }
    const bool dod = enc == BYDB_ENC_DELTA_OF_DELTA;
    int64_t d1 = 0, first_plus = first;
    if (dod) {
        int vl;
        d1 = decode_one_varint(s, &vl);
        s += vl;
        off += (uint64_t)vl;
        first_plus = (int64_t)((uint64_t)first + (uint64_t)d1);
        if (asc && d1 < 0) { dev_set_err(derr, DERR_DESC_TS, bi); return; }
        if (lane == 0) out[1] = first_plus;
    }
    dedup_decode_stream(s, limit - off, n - 1, dod, first_plus, d1, asc, lane,
                        out, derr, bi);
}

// One wave per involved block: timestamps coded Delta / DeltaOfDelta and
// versions coded anything but Const are decoded into the arena (16 B per
// row when both are); Const / DeltaConst timestamps stay closed form and
// only leave their stride in the block's DedupInfo.  The version list
// follows the timestamp list in the block's timestamps payload
// (block.go:386-404): it starts at ts_off + ts_len and its length is not in
// the descriptor, so every read is bounded by `limit`, the end of the
// payload arena's readable bytes.
__global__ __launch_bounds__(WAVE) void k_dedup_decode(
    const uint8_t *__restrict__ payload, uint64_t limit,
    const bydb_block_desc *__restrict__ blocks, DedupInfo *__restrict__ infos,
    int64_t n_inv, int64_t *__restrict__ arena, DevErr *derr) {
    const int lane = threadIdx.x;
    for (int64_t ia = blockIdx.x; ia < n_inv; ia += gridDim.x) {
        const DedupInfo in = infos[ia];
        const bydb_block_desc *bd = &blocks[in.block];
        const int64_t n = (int64_t)in.count;
        if (in.ts_min > in.ts_max) {
            dev_set_err(derr, DERR_DESC_TS, (uint64_t)in.block);
            continue;
        }
        if (in.ts_kind == DD_TS_ARITH) {
            if (bd->ts_off + 11 > limit) {
                dev_set_err(derr, DERR_BAD_STREAM, (uint64_t)in.block);
                continue;
            }
            int vl;
            int64_t dd = decode_one_varint(payload + bd->ts_off, &vl);
            if (dd <= 0)
                dev_set_err(derr, DERR_DESC_TS, (uint64_t)in.block);
            if (lane == 0) infos[ia].dd = dd;
        } else if (in.ts_kind == DD_TS_ARENA) {
            uint8_t tenc = bd->ts_enc_with_version;
            uint8_t tc = tenc >= BYDB_ENC_CONST_WV ? tenc - 4 : tenc;
            dedup_decode_list(payload, bd->ts_off, limit, tc, in.ts_min, n,
                              true, lane, arena + in.ts_arena, derr,
                              (uint64_t)in.block);
        }
        if (in.ver_arena != DD_NO_ARENA)
            dedup_decode_list(payload, bd->ts_off + bd->ts_len, limit,
                              bd->version_enc, in.ver_first, n, false, lane,
                              arena + in.ver_arena, derr, (uint64_t)in.block);
    }
}

__device__ __forceinline__ int64_t dd_ts_of(const DedupInfo &in,
                                            const int64_t *arena, int64_t row) {
    if (in.ts_kind == DD_TS_ARENA) return arena[in.ts_arena + (uint64_t)row];
    return (int64_t)((uint64_t)in.ts_min + (uint64_t)row * (uint64_t)in.dd);
}

__device__ __forceinline__ int64_t dd_ver_of(const DedupInfo &in,
                                             const int64_t *arena,
                                             int64_t row) {
    if (in.ver_arena == DD_NO_ARENA) return in.ver_first;
    return arena[in.ver_arena + (uint64_t)row];
}

// Rows [*lo, *hi) of block `in` whose timestamp equals ts (ts lies inside
// the block's range).  Timestamps inside a block ascend; equal neighbours
// are tolerated by returning the whole equal run.
__device__ __forceinline__ void dd_find_ts(const DedupInfo &in,
                                           const int64_t *arena, int64_t ts,
                                           int64_t *lo, int64_t *hi) {
    *lo = 0;
    *hi = 0;
    if (in.ts_kind == DD_TS_CONST) {
        if (ts == in.ts_min) *hi = (int64_t)in.count;
        return;
    }
    if (in.ts_kind == DD_TS_ARITH) {
        if (in.dd <= 0) return;
        uint64_t off = (uint64_t)ts - (uint64_t)in.ts_min;
        uint64_t row = off / (uint64_t)in.dd;
        if (row * (uint64_t)in.dd == off && row < in.count) {
            *lo = (int64_t)row;
            *hi = (int64_t)row + 1;
        }
        return;
    }
    const int64_t *t = arena + in.ts_arena;
    int64_t a = 0, b = (int64_t)in.count;
    while (a < b) {               // first row with t[row] >= ts
        int64_t m = (a + b) >> 1;
        if (t[m] < ts) a = m + 1;
        else b = m;
    }
    int64_t e = a;
    while (e < (int64_t)in.count && t[e] == ts) e++;
    *lo = a;
    *hi = e;
}

// One wave per involved block A: a survivor bit per row.  A row is
// superseded when a peer block holds a row of the same timestamp with a
// greater version, or with an equal version and a smaller block index.
// 64 rows per step, one ballot word per step; a peer whose range misses the
// step's rows costs one compare.  The block is then classified: nothing
// dropped (untouched), everything dropped (listed in flist), or partial
// (listed in plist, its 128-word bitmap kept in the survivor arena at the
// list position).
__global__ __launch_bounds__(WAVE) void k_dedup_mark(
    const DedupInfo *__restrict__ infos, int64_t n_inv,
    const uint64_t *__restrict__ peer_offs, const uint32_t *__restrict__ peers,
    const int64_t *__restrict__ arena, uint64_t *__restrict__ surv,
    uint32_t *__restrict__ plist, uint32_t *__restrict__ flist,
    unsigned long long *__restrict__ ctr) {
    const int lane = threadIdx.x;
    for (int64_t ia = blockIdx.x; ia < n_inv; ia += gridDim.x) {
        const DedupInfo A = infos[ia];
        const int64_t n = (int64_t)A.count;
        const uint64_t p0 = peer_offs[ia], p1 = peer_offs[ia + 1];
        uint64_t w0 = 0, w1 = 0;     // words lane, lane + 64 of the bitmap
        uint64_t dropped = 0;
        for (int64_t base = 0; base < n; base += WAVE) {
            const int64_t row = base + lane;
            const bool valid = row < n;
            const int nvalid = (int)(n - base < WAVE ? n - base : WAVE);
            const int64_t ts = valid ? dd_ts_of(A, arena, row) : 0;
            const int64_t ver = valid ? dd_ver_of(A, arena, row) : 0;
            const int64_t c_lo = (int64_t)readlane64((uint64_t)ts, 0);
            const int64_t c_hi = (int64_t)__shfl((long long)ts, nvalid - 1);
            bool sup = false;
            for (uint64_t p = p0; p < p1; p++) {
                const DedupInfo B = infos[peers[p]];
                if (B.ts_max < c_lo || B.ts_min > c_hi) continue;
                if (valid && !sup && ts >= B.ts_min && ts <= B.ts_max) {
                    int64_t lo, hi;
                    dd_find_ts(B, arena, ts, &lo, &hi);
                    for (int64_t r = lo; r < hi && !sup; r++) {
                        int64_t vb = dd_ver_of(B, arena, r);
                        sup = vb > ver || (vb == ver && B.block < A.block);
                    }
                }
            }
            const uint64_t word = __ballot(valid && !sup);
            dropped += (uint64_t)(nvalid - __popcll(word));
            const int c = (int)(base >> 6);
            if (lane == (c & 63)) {
                if (c < 64) w0 = word;
                else w1 = word;
            }
        }
        if (dropped == 0) continue;
        unsigned long long k = 0;
        if (lane == 0) {
            k = atomicAdd(&ctr[dropped == (uint64_t)n ? DD_CTR_FULL
                                                      : DD_CTR_PARTIAL], 1ull);
            atomicAdd(&ctr[DD_CTR_ROWS], (unsigned long long)dropped);
        }
        k = readlane64(k, 0);
        if (dropped == (uint64_t)n) {
            if (lane == 0) flist[k] = A.block;
        } else {
            if (lane == 0) plist[k] = A.block;
            surv[k * PLAIN_BM_WORDS + (uint64_t)lane] = w0;
            surv[k * PLAIN_BM_WORDS + 64 + (uint64_t)lane] = w1;
        }
    }
}

// Per consume: fold the survivors into what the resolve stage wrote (or
// into an all-CLEAR flag table for an unfiltered consume, n_slots == 0).
// One thread per fully superseded block flags it PF_SKIP.  One wave per
// partially superseded block, unless its verdict is SKIP or ERR already:
// the block becomes PF_WALK with slot 0 a row-bitmap predicate and the
// other slots disabled; its bitmap, in the pred_bm arena from word bm_base
// on, is survivors & rows(slot 0) & rows(slot 1) & rows(slot 2), where
// rows(slot) is all ones for a disabled / CLEAR slot, the code mask
// expanded per row through the RLE cursor for a dictionary slot, and the
// existing bitmap for a plain or tree row-bitmap slot.  The walk census
// follows, so the heavy pass still exits early when nothing walks.
__global__ __launch_bounds__(WAVE) void k_dedup_apply(
    const uint8_t *__restrict__ payload, const uint8_t *__restrict__ sidecar,
    const bydb_block_desc *__restrict__ blocks, int64_t n_blocks,
    const uint32_t *__restrict__ plist, int64_t n_partial,
    const uint32_t *__restrict__ flist, int64_t n_full,
    const uint64_t *__restrict__ surv, PredBlock *preds, int n_slots,
    uint8_t *flags, uint64_t *pred_bm, uint64_t bm_base,
    uint32_t *walk_count) {
    const int lane = threadIdx.x;
    for (int64_t t = (int64_t)blockIdx.x * WAVE + lane; t < n_full;
         t += (int64_t)gridDim.x * WAVE) {
        const uint32_t bi = flist[t];
        if (flags[bi] == PF_WALK) atomicSub(walk_count, 1u);
        flags[bi] = PF_SKIP;
    }
    for (int64_t p = blockIdx.x; p < n_partial; p += gridDim.x) {
        const int64_t bi = (int64_t)plist[p];
        const uint8_t f = flags[bi];
        if (f == PF_SKIP || f == PF_ERR) continue;
        const int64_t n = (int64_t)blocks[bi].count;
        // per slot: 0 = no constraint, 1 = no row, 2 = bitmap, 3 = RLE mask
        int kind[3] = {0, 0, 0};
        uint64_t bm_off[3] = {0, 0, 0};
        uint64_t mask[3][4];
        CodeWalk cw[3];
#pragma unroll
        for (int sl = 0; sl < 3; sl++) {
            if (f != PF_WALK || sl >= n_slots) continue;
            const PredBlock pb = preds[(int64_t)sl * n_blocks + bi];
            if (pb.disabled) continue;
            if (!pb.active) { kind[sl] = 1; continue; }
            if (pb.plain) {
                kind[sl] = 2;
                bm_off[sl] = pb.rle_bit_off;
                continue;
            }
            kind[sl] = 3;
#pragma unroll
            for (int i = 0; i < 4; i++) mask[sl][i] = pb.mask[i];
            cw[sl].base = (pb.rle_bit_off & TAG_SIDECAR_BIT) ? sidecar
                                                             : payload;
            cw[sl].bit0 = pb.rle_bit_off & ~TAG_SIDECAR_BIT;
            cw[sl].nentries = pb.nentries;
            cw[sl].width = pb.width;
            cw[sl].entry = 0;
            cw[sl].run_lo = 0;
            cw[sl].run_hi = 0;
            cw[sl].run_code = CODE_NONE;
        }
        const uint64_t out0 = bm_base + (uint64_t)p * PLAIN_BM_WORDS;
        for (int64_t base = 0; base < n; base += WAVE) {
            const int64_t row = base + lane;
            const bool valid = row < n;
            const uint64_t c = (uint64_t)(base >> 6);
            uint64_t word = surv[(uint64_t)p * PLAIN_BM_WORDS + c];
#pragma unroll
            for (int sl = 0; sl < 3; sl++) {
                if (kind[sl] == 1) {
                    word = 0;
                } else if (kind[sl] == 2) {
                    word &= pred_bm[bm_off[sl] + c];
                } else if (kind[sl] == 3) {
                    uint32_t code = code_of_rows(&cw[sl], row, valid);
                    uint32_t w = (code >> 6) & 3;
                    uint64_t m = w == 0 ? mask[sl][0] : w == 1 ? mask[sl][1]
                                 : w == 2 ? mask[sl][2] : mask[sl][3];
                    word &= __ballot(valid && code != CODE_NONE &&
                                     ((m >> (code & 63)) & 1));
                }
            }
            if (lane == 0) pred_bm[out0 + c] = word;
        }
        if (lane == 0) {
            PredBlock pb;
            for (int i = 0; i < 4; i++) pb.mask[i] = 0;
            pb.rle_bit_off = 0; pb.nentries = 0; pb.width = 0;
            pb.active = 0; pb.err = 0; pb.uniform = 0; pb.plain = 0;
            pb.disabled = 1;
            for (int sl = 1; sl < n_slots; sl++)
                preds[(int64_t)sl * n_blocks + bi] = pb;
            pb.rle_bit_off = out0;
            pb.active = 1;
            pb.plain = 1;
            pb.disabled = 0;
            preds[bi] = pb;
            flags[bi] = PF_WALK;
            if (f == PF_CLEAR) atomicAdd(walk_count, 1u);
        }
    }
}

// init kernel: set partials to the fold identity (Map.Reset, function.go)
__global__ void k_reset_partials(bydb_partial *p, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        p[i].sum_i = 0;
        p[i].count = 0;
        p[i].min_i = INT64_MAX;
        p[i].max_i = INT64_MIN;
        p[i].sum_f = 0.0;
        p[i]._pad = 0.0;
    }
}

// ---------------- nibble-packed dense field streams ----------------
// A dense one-byte delta stream whose zigzag bytes are all <= 15 carries
// four bits of information per byte.  Parts are immutable and stay
// resident, so such streams get a 4-bit copy, built once per part
// (pack_build) and read by the streaming closed-form scan in place of the
// byte stream (dense_region_packed).  The planner decides from the
// descriptors alone which blocks get a slot; whether a slot is filled is
// decided here, from the bytes.

// A block is a candidate when its field stream is a dense one-byte delta
// stream in the payload arena.
__host__ __device__ __forceinline__ bool pack_candidate(
    const bydb_block_desc *bd) {
    return bd->field_enc == BYDB_ENC_DELTA && bd->count >= 2 &&
           bd->count <= PACK_MAX_ROWS &&
           bd->field_len == (uint64_t)bd->count - 1 &&
           !(bd->field_off & TAG_SIDECAR_BIT);
}

#define PACK_CTR_BLOCKS 0
#define PACK_CTR_BYTES 1

// One wave per planned block.  table[bi] arrives as the planner's slot
// (offset from `pack` in 128-byte units, 0: no slot) and leaves as 0 where
// a byte of the stream exceeds 15: that block stays with its byte stream,
// its slot is wasted.  The pad nibbles up to the slot's end are 8 (delta 0).
__global__ __launch_bounds__(WAVE) void k_pack_fields(
    const uint8_t *__restrict__ payload,
    const bydb_block_desc *__restrict__ blocks, int64_t n_blocks,
    uint8_t *__restrict__ pack, unsigned long long *__restrict__ ctr) {
    const int lane = threadIdx.x;
    uint32_t *table = (uint32_t *)pack;
    for (int64_t bi = blockIdx.x; bi < n_blocks; bi += gridDim.x) {
        const uint32_t unit = table[bi];
        if (unit == 0) continue;
        const bydb_block_desc *bd = &blocks[bi];
        const uint8_t *stream = payload + bd->field_off;
        const uint32_t len = bd->count - 1;
        uint32_t seen = 0;
        for (uint32_t i = lane; i < len; i += WAVE) seen |= stream[i];
        if (__any(seen > 15u)) {
            if (lane == 0) table[bi] = 0;
            continue;
        }
        uint8_t *slot = pack + (uint64_t)unit * PACK_SLOT_ALIGN;
        const uint32_t slot_bytes = pack_slot_bytes(bd->count);
        for (uint32_t q = lane; q < slot_bytes; q += WAVE) {
            // zigzag byte z <= 15 -> delta (z >> 1) ^ -(z & 1), biased by 8
            uint32_t nib[2];
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const uint32_t i = 2 * q + k;
                const uint32_t z = i < len ? stream[i] : 0;
                nib[k] = (uint32_t)((int32_t)((z >> 1) ^ (0u - (z & 1u))) + 8);
            }
            slot[q] = (uint8_t)(nib[0] | (nib[1] << 4));
        }
        if (lane == 0) {
            atomicAdd(&ctr[PACK_CTR_BLOCKS], 1ull);
            atomicAdd(&ctr[PACK_CTR_BYTES], (unsigned long long)((len + 1) / 2));
        }
    }
}

// ---------------- BatchTop over raw rows ----------------
// A measure query with `top` and no `agg` runs measure.BatchTop over every
// data point the scan yields (pkg/query/vectorized/measure/plan/
// analyzer.go:118-151, plan/top.go:28-46, top.go:30-199): a whole-result
// top-N by field value, equal values in input order.  Input order is storage
// order, seq = (block << 13) | row.
//
// The top rows lie in few blocks.  Give every block the key "its best
// selected value" and order blocks by (key, best first; index ascending).
// Every row of the true top-N lies in one of the N best blocks: were a row r
// of block B outside them, N other blocks would each hold a row that beats r
// (a better value, or the same value in a smaller block index and so a
// smaller seq).  Two exact selections are therefore enough — the N best
// blocks (k_top_bounds + top_select), then the N best rows inside those
// blocks (k_top_row_keys + top_select) — and no buffer grows with the data.
//
// Keys are order-preserving uint64: a larger key is better in both
// directions.  float64 mantissas are rescaled exactly to the session
// exponent first (the rescale WavePartial::add does for min/max).
#define TOP_BLOCK_ROWS 8192   // rows per block, at most (measure.go:41-46)
#define TOP_CHUNK 1024        // selector chunk: 256 threads x 4 entries

__host__ __device__ __forceinline__ uint64_t top_key(int64_t v, bool asc) {
    uint64_t k = (uint64_t)v ^ (1ull << 63);
    return asc ? ~k : k;
}

__host__ __device__ __forceinline__ int64_t top_unkey(uint64_t k, bool asc) {
    if (asc) k = ~k;
    return (int64_t)(k ^ (1ull << 63));
}

// What the scan's preamble decides for one block: the clamped rows
// [r0, r1], the float rescale and the row-varying walkers.
struct TopSel {
    int64_t r0, r1;
    int fdiff;
    PredWalk pw[3];
    PredWalk *wp[3];
};

// The preamble of k_scan_agg_t, restated in two halves (sharing it through
// a device function would have to change the scan kernel).  The first half:
// count and exponent checks and the FindRange row clamp.  Returns false when
// the block selects nothing (or erred).  A Plain field block skips the
// exponent check: the callers reject it once rows are selected.
// It calls clamp_count_stream, an out-of-line function the scan's clamped
// instantiations share, all of them __launch_bounds__(256, 4).  The compiler
// derives such a function's register budget from the kernels that call it,
// so only kernels with those launch bounds may call top_clamp: from a
// 64-thread kernel it moved the scan instantiations' spill counts
// (profiles/top_rows.txt).
__device__ __forceinline__ bool top_clamp(
    const uint8_t *__restrict__ payload, const bydb_block_desc *bd, int64_t bi,
    int64_t min_ts, int64_t max_ts, int flags, int lane, DevErr *derr,
    TopSel *ts) {
    const int64_t n = (int64_t)bd->count;
    const int64_t ts_min = bd->ts_min, ts_max = bd->ts_max;
    ts->fdiff = 0;
    if (n < 1 || n > TOP_BLOCK_ROWS) {
        dev_set_err(derr, DERR_BAD_ENC, (uint64_t)bi);
        return false;
    }
    if ((flags & KF_FLOAT) && bd->field_enc != BYDB_ENC_PLAIN) {
        int16_t cfge = (int16_t)(uint16_t)((uint32_t)flags >> 16);
        ts->fdiff = (int)bd->exp - (int)cfge;
        if (ts->fdiff < 0 || ts->fdiff > 18) {
            dev_set_err(derr, DERR_EXP_MISMATCH, (uint64_t)bi);
            return false;
        }
    }
    // ---- row clamp (timestamp.FindRange, range.go:143-170) ----
    int64_t r0 = 0, r1 = n - 1;
    if (ts_min > ts_max) {
        dev_set_err(derr, DERR_DESC_TS, (uint64_t)bi);
        return false;
    }
    if (!(min_ts <= ts_min && max_ts >= ts_max)) {
        if (ts_min > max_ts || ts_max < min_ts) return false;
        uint8_t tenc = bd->ts_enc_with_version;
        uint8_t tc = tenc >= BYDB_ENC_CONST_WV &&
                             tenc <= BYDB_ENC_DELTA_OF_DELTA_WV
                         ? tenc - 4 : tenc;
        const uint8_t *tstream = payload + bd->ts_off;
        if (tc == BYDB_ENC_CONST) {
            // all == ts_min; overlap already implies in-range
        } else if (tc == BYDB_ENC_DELTA_CONST) {
            int vl;
            int64_t dd = decode_one_varint(tstream, &vl);
            if (dd <= 0) {
                dev_set_err(derr, DERR_DESC_TS, (uint64_t)bi);
                return false;
            }
            if (min_ts > ts_min) r0 = (min_ts - ts_min + dd - 1) / dd;
            if (max_ts < ts_max) r1 = (max_ts - ts_min) / dd;
            if (r1 > n - 1) r1 = n - 1;
        } else if (tc == BYDB_ENC_DELTA || tc == BYDB_ENC_DELTA_OF_DELTA) {
            bool dod = tc == BYDB_ENC_DELTA_OF_DELTA;
            const uint8_t *s = tstream;
            int64_t d1 = 0;
            if (dod) {
                int vl;
                d1 = decode_one_varint(s, &vl);
                s += vl;
            }
            int64_t row1 = (int64_t)((uint64_t)ts_min + (uint64_t)d1);
            uint64_t nlo, nhi;
            clamp_count_stream(s, n - 1, dod, dod ? row1 : ts_min, d1, min_ts,
                               max_ts, lane, &nlo, &nhi, derr, (uint64_t)bi);
            if (ts_min < min_ts) nlo++;
            if (ts_min > max_ts) nhi++;
            if (dod) {
                if (row1 < min_ts) nlo++;
                if (row1 > max_ts) nhi++;
            }
            r0 = (int64_t)nlo;
            r1 = n - 1 - (int64_t)nhi;
        }
        if (r0 > r1) return false;
    }
    ts->r0 = r0;
    ts->r1 = r1;
    return true;
}

// The second half: tag predicates and dedup survivors — the flag byte, then
// the walkers.  Nothing here leaves the kernel (every helper is inlined).
__device__ __forceinline__ bool top_walkers(
    const uint8_t *__restrict__ payload, const uint8_t *__restrict__ sidecar,
    int64_t bi, int64_t n_blocks, const PredBlock *__restrict__ preds,
    int n_preds, const uint64_t *__restrict__ pred_bm,
    const uint8_t *__restrict__ pred_flags, DevErr *derr, TopSel *ts) {
    ts->wp[0] = ts->wp[1] = ts->wp[2] = nullptr;
    if (preds != nullptr) {
        const uint8_t pf = pred_flags[bi];
        if (pf == PF_SKIP) return false;
        if (pf == PF_ERR) {
            dev_set_err(derr, DERR_BAD_ENC, (uint64_t)bi);
            return false;
        }
        if (pf == PF_WALK) {
            bool skip_block = false;
#pragma unroll
            for (int sl = 0; sl < 3; sl++) {
                if (sl >= n_preds || skip_block) continue;
                PredBlock pb = preds[(int64_t)sl * n_blocks + bi];
                if (pb.disabled) continue;
                if (!pb.active) { skip_block = true; continue; }
                PredWalk *w = &ts->pw[sl];
                pred_init(w, payload, sidecar, &pb, pred_bm);
                if (pb.uniform) {
                    pred_advance(w);
                    if (!w->run_match) skip_block = true;
                } else {
                    ts->wp[sl] = w;
                }
            }
            if (skip_block) return false;
        }
    }
    return true;
}

// Does any row of [r0, r1] pass the walkers?  (Plain blocks only: the fold
// is never run on them.)
__device__ __forceinline__ bool top_any_row(TopSel *ts, int lane) {
    bool any = false;
    for (int64_t base = ts->r0; base <= ts->r1; base += WAVE) {
        int64_t row = base + lane;
        bool need = row <= ts->r1;
        bool ok = walkers_match(ts->wp[0], ts->wp[1], ts->wp[2], row, need) &&
                  need;
        any = any || __any(ok);
    }
    return any;
}

// Stage 1 — one wave per block, grid-stride: the key of the block's best
// selected value and a validity byte (pre-zeroed by the host).  It reads
// what a MIN/MAX scan over the same selection reads: the field fold is the
// scan's own, fold_rows<true, false, DENSE_CALL> with values requested.
// (launch bounds: those of the scan's clamped value instantiations, whose
// out-of-line helpers this kernel calls — see top_clamp)
__global__ __launch_bounds__(256, 4) void k_top_bounds(
    const uint8_t *__restrict__ payload, const uint8_t *__restrict__ sidecar,
    const bydb_block_desc *__restrict__ blocks, int64_t n_blocks,
    int64_t min_ts, int64_t max_ts, int flags, int asc,
    const PredBlock *__restrict__ preds, int n_preds,
    const uint64_t *__restrict__ pred_bm,
    const uint8_t *__restrict__ pred_flags, uint64_t *__restrict__ keys,
    uint8_t *__restrict__ valid, DevErr *derr) {
    const int lane = threadIdx.x & 63;
    const int64_t wave_id =
        (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t bi = wave_id; bi < n_blocks; bi += n_waves) {
        const bydb_block_desc *bd = &blocks[bi];
        TopSel ts;
        if (!top_clamp(payload, bd, bi, min_ts, max_ts, flags, lane, derr,
                       &ts) ||
            !top_walkers(payload, sidecar, bi, n_blocks, preds, n_preds,
                         pred_bm, pred_flags, derr, &ts))
            continue;
        const uint8_t fenc = bd->field_enc;
        if (fenc == BYDB_ENC_PLAIN) {
            // null-bearing block: never drop a null row silently
            if (top_any_row(&ts, lane))
                dev_set_err(derr, DERR_TOP_NULL, (uint64_t)bi);
            continue;
        }
        const RowFold f = fold_rows<true, false, DENSE_CALL>(
            payload + bd->field_off, nullptr, fenc, bd->field_first,
            bd->field_len, (int64_t)bd->count, ts.r0, ts.r1, true, false,
            lane, ts.wp[0], ts.wp[1], ts.wp[2], derr, (uint64_t)bi);
        if (f.cnt == 0 || !f.have_mm) continue;
        int64_t mn = f.mn, mx = f.mx;
        if (ts.fdiff) {
            const int64_t mfac = c_pow10i[ts.fdiff];
            if (__builtin_mul_overflow(mn, mfac, &mn) ||
                __builtin_mul_overflow(mx, mfac, &mx)) {
                dev_set_err(derr, DERR_EXP_MISMATCH, (uint64_t)bi);
                continue;
            }
        }
        if (lane == 0) {
            keys[bi] = top_key(asc ? mn : mx, asc != 0);
            valid[bi] = 1;
        }
    }
}

// ---- top_select: the N best of n entries, entirely on the device ----
// Best = key descending, index ascending; emitted in ascending index order.
// An MSB radix select fixes the N-th best key one byte per pass (an LDS
// histogram over the entries that match the prefix so far, then a pick that
// fixes the next digit and the remaining rank); a stable compaction then
// takes every greater entry and the first `remaining` equal ones.  Fewer
// than N valid entries selects them all.
struct TopSelState {
    uint64_t prefix;      // the digits fixed so far; after 8 passes the key
    uint32_t remaining;   // entries to take among those that match prefix
    uint32_t all;         // at most N valid entries: take every one
    uint32_t n_out;       // entries selected (written by k_sel_scan)
    uint32_t _p;
    uint32_t hist[256];
};

__global__ __launch_bounds__(256) void k_sel_hist(
    const uint64_t *__restrict__ keys, const uint8_t *__restrict__ valid,
    uint64_t n, TopSelState *st, int pass) {
    __shared__ uint32_t h[256];
    if (pass > 0 && st->all) return;
    const uint64_t prefix = st->prefix;
    const uint64_t mask = pass == 0 ? 0ull : ~0ull << (64 - 8 * pass);
    const int shift = 56 - 8 * pass;
    h[threadIdx.x] = 0;
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * 256) {
        if (!valid[i]) continue;
        const uint64_t k = keys[i];
        if ((k & mask) == prefix) atomicAdd(&h[(k >> shift) & 255], 1u);
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&st->hist[threadIdx.x], h[threadIdx.x]);
}

// One workgroup of 256.  Pass 0 also decides `all`.  Invariant: the entries
// that match the prefix number at least `remaining`.
__global__ __launch_bounds__(256) void k_sel_pick(TopSelState *st, int pass,
                                                  uint32_t want) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = st->hist[threadIdx.x];
    st->hist[threadIdx.x] = 0;
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (pass == 0) {
        uint64_t total = 0;
        for (int b = 0; b < 256; b++) total += h[b];
        st->prefix = 0;
        st->remaining = want;
        st->all = total <= (uint64_t)want;
        st->n_out = 0;
    }
    if (st->all) return;
    uint32_t rem = st->remaining, cum = 0;
    int digit = 0;
    for (int b = 255; b >= 0; b--) {
        if (cum + h[b] >= rem) { digit = b; break; }
        cum += h[b];
    }
    st->prefix |= (uint64_t)digit << (56 - 8 * pass);
    st->remaining = rem - cum;
}

// class of entry i against the selected threshold: 2 greater (always
// taken), 1 equal (taken while the rank lasts), 0 neither
__device__ __forceinline__ uint32_t sel_class(const uint64_t *keys,
                                              const uint8_t *valid, uint64_t i,
                                              uint64_t n, uint64_t thr,
                                              bool all) {
    if (i >= n || !valid[i]) return 0;
    if (all) return 2;
    const uint64_t k = keys[i];
    return k > thr ? 2 : k == thr ? 1 : 0;
}

// per-chunk counts of greater and equal entries
__global__ __launch_bounds__(256) void k_sel_count(
    const uint64_t *__restrict__ keys, const uint8_t *__restrict__ valid,
    uint64_t n, const TopSelState *st, uint32_t *__restrict__ cnt_gt,
    uint32_t *__restrict__ cnt_eq) {
    __shared__ uint32_t s_gt, s_eq;
    if (threadIdx.x == 0) { s_gt = 0; s_eq = 0; }
    __syncthreads();
    const uint64_t thr = st->prefix;
    const bool all = st->all != 0;
    const uint64_t i0 = (uint64_t)blockIdx.x * TOP_CHUNK + threadIdx.x * 4;
    uint32_t g = 0, e = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint32_t c = sel_class(keys, valid, i0 + k, n, thr, all);
        g += c == 2;
        e += c == 1;
    }
    if (g) atomicAdd(&s_gt, g);
    if (e) atomicAdd(&s_eq, e);
    __syncthreads();
    if (threadIdx.x == 0) {
        cnt_gt[blockIdx.x] = s_gt;
        cnt_eq[blockIdx.x] = s_eq;
    }
}

// One workgroup of 1024 over all chunks, in place: cnt_eq[c] becomes the
// equal entries before chunk c, cnt_gt[c] the selected entries before it.
__global__ __launch_bounds__(1024) void k_sel_scan(
    TopSelState *st, uint32_t *__restrict__ cnt_gt,
    uint32_t *__restrict__ cnt_eq, uint32_t n_chunks) {
    __shared__ uint32_t part[1024];
    const uint32_t per = (n_chunks + 1023) / 1024;
    const uint32_t c0 = threadIdx.x * per;
    const uint32_t c1 = c0 + per < n_chunks ? c0 + per : n_chunks;
    const uint32_t rem = st->all ? 0 : st->remaining;
    auto excl = [&](uint32_t mine) -> uint32_t {
        part[threadIdx.x] = mine;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t run = 0;
            for (int t = 0; t < 1024; t++) {
                uint32_t v = part[t];
                part[t] = run;
                run += v;
            }
        }
        __syncthreads();
        uint32_t r = part[threadIdx.x];
        __syncthreads();
        return r;
    };
    uint32_t sum = 0;
    for (uint32_t c = c0; c < c1; c++) sum += cnt_eq[c];
    uint32_t run = excl(sum);
    sum = 0;
    for (uint32_t c = c0; c < c1; c++) {
        const uint32_t e = cnt_eq[c];
        const uint32_t left = rem > run ? rem - run : 0;
        const uint32_t sel = cnt_gt[c] + (e < left ? e : left);
        cnt_eq[c] = run;
        cnt_gt[c] = sel;
        run += e;
        sum += sel;
    }
    run = excl(sum);
    for (uint32_t c = c0; c < c1; c++) {
        const uint32_t sel = cnt_gt[c];
        cnt_gt[c] = run;
        run += sel;
    }
    if (threadIdx.x == 1023) st->n_out = run;
}

// exclusive scan of one value per thread over a workgroup of 256
__device__ __forceinline__ uint32_t sel_block_scan(uint32_t v, uint32_t *w4) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t incl = (uint32_t)wave_incl_scan32((int32_t)v, lane);
    if (lane == 63) w4[w] = incl;
    __syncthreads();
    uint32_t base = 0;
    for (int i = 0; i < 4; i++)
        if (i < w) base += w4[i];
    __syncthreads();
    return base + incl - v;
}

// in-order emit: out[] receives the selected indices, ascending
__global__ __launch_bounds__(256) void k_sel_emit(
    const uint64_t *__restrict__ keys, const uint8_t *__restrict__ valid,
    uint64_t n, const TopSelState *st, const uint32_t *__restrict__ sel_before,
    const uint32_t *__restrict__ eq_before, uint32_t *__restrict__ out,
    uint32_t out_cap) {
    __shared__ uint32_t w4[4];
    const uint64_t thr = st->prefix;
    const bool all = st->all != 0;
    const uint32_t rem = all ? 0 : st->remaining;
    const uint64_t i0 = (uint64_t)blockIdx.x * TOP_CHUNK + threadIdx.x * 4;
    uint32_t cls[4], e = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        cls[k] = sel_class(keys, valid, i0 + k, n, thr, all);
        e += cls[k] == 1;
    }
    uint32_t eq_rank = eq_before[blockIdx.x] + sel_block_scan(e, w4);
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (cls[k] == 1) cls[k] = eq_rank++ < rem ? 2 : 0;
        s += cls[k] == 2;
    }
    uint32_t at = sel_before[blockIdx.x] + sel_block_scan(s, w4);
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (cls[k] == 2) {
            if (at < out_cap) out[at] = (uint32_t)(i0 + k);
            at++;
        }
}

// Stage 3a — one wave per chosen block: [r0, r1] recomputed, packed as
// r0 | r1 << 16 (TOP_NO_ROWS: nothing selected).  A kernel of its own for
// its launch bounds (see top_clamp); stage 3b decodes with the dedup
// build's out-of-line helpers, which belong to 64-thread kernels.
#define TOP_NO_ROWS 0xFFFFFFFFu
__global__ __launch_bounds__(256, 4) void k_top_row_range(
    const uint8_t *__restrict__ payload,
    const bydb_block_desc *__restrict__ blocks, int64_t n_blocks,
    int64_t min_ts, int64_t max_ts, int flags, const TopSelState *st,
    const uint32_t *__restrict__ chosen, uint32_t *__restrict__ range,
    uint32_t cap, DevErr *derr) {
    const int lane = threadIdx.x & 63;
    const uint32_t c = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (c >= st->n_out || c >= cap) return;
    const int64_t bi = (int64_t)chosen[c];
    TopSel ts;
    uint32_t r = TOP_NO_ROWS;
    if (bi < n_blocks && top_clamp(payload, &blocks[bi], bi, min_ts, max_ts,
                                   flags, lane, derr, &ts))
        r = (uint32_t)ts.r0 | ((uint32_t)ts.r1 << 16);
    if (lane == 0) range[c] = r;
}

// Stage 3b — one wave per chosen block (at most N, ascending block index):
// the field column decoded into the block's slot of the row grid, then every
// selected row's value replaced by its key.  The grid is chosen x 8192,
// block-major, so index order is seq order; rvalid is pre-zeroed.
__global__ __launch_bounds__(WAVE) void k_top_row_keys(
    const uint8_t *__restrict__ payload, const uint8_t *__restrict__ sidecar,
    uint64_t limit, const bydb_block_desc *__restrict__ blocks,
    int64_t n_blocks, int flags, int asc,
    const PredBlock *__restrict__ preds, int n_preds,
    const uint64_t *__restrict__ pred_bm,
    const uint8_t *__restrict__ pred_flags, const TopSelState *st,
    const uint32_t *__restrict__ chosen, const uint32_t *__restrict__ range,
    uint64_t *__restrict__ grid, uint8_t *__restrict__ rvalid, DevErr *derr) {
    const int lane = threadIdx.x;
    const uint32_t c = blockIdx.x;
    if (c >= st->n_out) return;
    const int64_t bi = (int64_t)chosen[c];
    if (bi >= n_blocks || range[c] == TOP_NO_ROWS) return;
    const bydb_block_desc *bd = &blocks[bi];
    TopSel ts;
    ts.r0 = (int64_t)(range[c] & 0xFFFFu);
    ts.r1 = (int64_t)(range[c] >> 16);
    ts.fdiff = 0;
    if (flags & KF_FLOAT)   // in 0..18: top_clamp accepted the block
        ts.fdiff = (int)bd->exp - (int)(int16_t)(uint16_t)((uint32_t)flags >> 16);
    if (!top_walkers(payload, sidecar, bi, n_blocks, preds, n_preds, pred_bm,
                     pred_flags, derr, &ts))
        return;
    const uint8_t fenc = bd->field_enc;
    const int64_t n = (int64_t)bd->count;
    int64_t *vals = (int64_t *)(grid + (uint64_t)c * TOP_BLOCK_ROWS);
    uint8_t *ok_out = rvalid + (uint64_t)c * TOP_BLOCK_ROWS;
    if (fenc == BYDB_ENC_CONST) {
        for (int64_t i = lane; i < n; i += WAVE) vals[i] = bd->field_first;
    } else if (fenc == BYDB_ENC_DELTA_CONST || fenc == BYDB_ENC_DELTA ||
               fenc == BYDB_ENC_DELTA_OF_DELTA) {
        if (bd->field_off & TAG_SIDECAR_BIT) {
            dev_set_err(derr, DERR_BAD_ENC, (uint64_t)bi);
            return;
        }
        dedup_decode_list(payload, bd->field_off, limit, fenc, bd->field_first,
                          n, false, lane, vals, derr, (uint64_t)bi);
    } else {
        return;   // Plain blocks never carry a valid bound
    }
    // the decode stores a row from whichever lane held its terminator
    __threadfence();
    const int64_t mfac = c_pow10i[ts.fdiff];
    for (int64_t base = ts.r0; base <= ts.r1; base += WAVE) {
        const int64_t row = base + lane;
        const bool need = row <= ts.r1;
        const bool ok =
            walkers_match(ts.wp[0], ts.wp[1], ts.wp[2], row, need) && need;
        if (ok) {
            int64_t v = vals[row];
            if (ts.fdiff && __builtin_mul_overflow(v, mfac, &v)) {
                dev_set_err(derr, DERR_EXP_MISMATCH, (uint64_t)bi);
            } else {
                vals[row] = (int64_t)top_key(v, asc != 0);
                ok_out[row] = 1;
            }
        }
    }
}

// One winner as the device hands it over; the host sorts the at most 1024
// of them and restores value_f.
struct TopRec {
    uint64_t series_id;
    int64_t ts, version;
    int64_t value;      // block-domain value / mantissa
    uint64_t key;       // session-domain order key
    uint64_t seq;
    int32_t exp;        // the block's decimal exponent
    int32_t _p;
};

// Stage 5a — one thread per winner: what the key grid and the descriptor
// hold.  It runs before 5b, which reuses the grid as decode scratch.
__global__ __launch_bounds__(256) void k_top_resolve_keys(
    const bydb_block_desc *__restrict__ blocks, int64_t n_blocks, int flags,
    int asc, const TopSelState *st_rows, const uint32_t *__restrict__ chosen,
    const uint32_t *__restrict__ winners, const uint64_t *__restrict__ grid,
    TopRec *__restrict__ recs, uint32_t cap) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= st_rows->n_out || i >= cap) return;
    const uint32_t idx = winners[i];
    const uint32_t row = idx & (TOP_BLOCK_ROWS - 1);
    const int64_t bi = (idx >> 13) < cap ? (int64_t)chosen[idx >> 13] : n_blocks;
    TopRec r = {};
    r.seq = ~0ull;   // no block: stage 5b leaves the record alone
    if (bi < n_blocks) {
        const bydb_block_desc *bd = &blocks[bi];
        const uint64_t key = grid[idx];
        int64_t v = top_unkey(key, asc != 0);
        if (flags & KF_FLOAT) {
            int16_t cfge = (int16_t)(uint16_t)((uint32_t)flags >> 16);
            int fdiff = (int)bd->exp - (int)cfge;
            if (fdiff > 0 && fdiff <= 18) v /= c_pow10i[fdiff];   // exact
        }
        r.series_id = bd->series_id;
        r.value = v;
        r.key = key;
        r.seq = ((uint64_t)bi << 13) | row;
        r.exp = bd->exp;
    }
    recs[i] = r;
}

// Stage 5b — one wave per winner: the row's timestamp and version.  Const /
// DeltaConst lists are closed form; a stream-coded list is decoded, as
// k_dedup_decode does, into the winner's own slot of the (now free) grid.
__global__ __launch_bounds__(WAVE) void k_top_resolve(
    const uint8_t *__restrict__ payload, uint64_t limit,
    const bydb_block_desc *__restrict__ blocks, int64_t n_blocks,
    const TopSelState *st_rows, uint64_t *__restrict__ grid,
    TopRec *__restrict__ recs, DevErr *derr) {
    const int lane = threadIdx.x;
    const uint32_t i = blockIdx.x;
    if (i >= st_rows->n_out) return;
    const uint64_t seq = recs[i].seq;
    const int64_t bi = (int64_t)(seq >> 13);
    const int64_t row = (int64_t)(seq & (TOP_BLOCK_ROWS - 1));
    if (bi >= n_blocks) return;
    const bydb_block_desc *bd = &blocks[bi];
    const int64_t n = (int64_t)bd->count;
    if (n < 1 || n > TOP_BLOCK_ROWS || row >= n) return;
    int64_t *scratch = (int64_t *)(grid + (uint64_t)i * TOP_BLOCK_ROWS);
    const uint8_t tenc = bd->ts_enc_with_version;
    const uint8_t tc = tenc >= BYDB_ENC_CONST_WV ? tenc - 4 : tenc;
    int64_t ts = bd->ts_min;
    if (tc == BYDB_ENC_DELTA_CONST) {
        if (bd->ts_off + 11 > limit) {
            dev_set_err(derr, DERR_BAD_STREAM, (uint64_t)bi);
            return;
        }
        int vl;
        int64_t dd = decode_one_varint(payload + bd->ts_off, &vl);
        ts = (int64_t)((uint64_t)bd->ts_min + (uint64_t)row * (uint64_t)dd);
    } else if (tc == BYDB_ENC_DELTA || tc == BYDB_ENC_DELTA_OF_DELTA) {
        dedup_decode_list(payload, bd->ts_off, limit, tc, bd->ts_min, n, true,
                          lane, scratch, derr, (uint64_t)bi);
        __threadfence();
        ts = scratch[row];
        __threadfence();   // read before the version decode reuses the slot
    } else if (tc != BYDB_ENC_CONST) {
        dev_set_err(derr, DERR_BAD_ENC, (uint64_t)bi);
        return;
    }
    int64_t ver = bd->version_first;
    const uint8_t venc = bd->version_enc;
    if (venc == BYDB_ENC_DELTA_CONST || venc == BYDB_ENC_DELTA ||
        venc == BYDB_ENC_DELTA_OF_DELTA) {
        dedup_decode_list(payload, bd->ts_off + bd->ts_len, limit, venc,
                          bd->version_first, n, false, lane, scratch, derr,
                          (uint64_t)bi);
        __threadfence();
        ver = scratch[row];
    } else if (venc != BYDB_ENC_CONST) {
        dev_set_err(derr, DERR_BAD_ENC, (uint64_t)bi);
        return;
    }
    if (lane == 0) {
        recs[i].ts = ts;
        recs[i].version = ver;
    }
}

// ---------------- Scan -> Limit over raw rows ----------------
// A measure query with neither `agg` nor `top` is Scan -> Limit
// (pkg/query/vectorized/measure/plan/analyzer.go:118-157): queryResult's
// heap merges the block cursors of all parts by timestamp, equal timestamps
// by seriesID ascending (banyand/measure/query.go:913-943, 962-1026;
// SORT_DESC walks the cursors backwards, :286-296), and BatchLimit keeps
// rows [offset, offset + limit) of that stream (limit.go:81-108).
//
// The order is total on selected rows: (ts in the requested direction,
// series_id ascending and unsigned, seq ascending).  N = offset + limit.
// The containment argument of the top-N section holds for any total order:
// key each block by its best selected row — the first one ascending, the
// last one descending, timestamps never fall inside a block — and order
// blocks by (key, index).  Were a row r of block B outside the N best
// blocks, N other blocks would each hold a row before r: a better
// (ts, series), or the same pair in a smaller block index and so a smaller
// seq.  So again two exact selections, N blocks and then N rows of their
// grid, but under a two-word key: hi = the timestamp key (top_key, larger
// is better in both directions), lo = ~series_id.
//
// The block-key pass opens no field stream, and no timestamp stream for a
// block the clamp covers whole and no walker filters: "latest N" over such
// a part is a sweep of the descriptors.
#define ROWS_DEFER 2   // validity byte: hi holds a row index, not yet a key

// Stage 1 — one wave per block, grid-stride: the two-word key of the
// block's best selected row.  Const / DeltaConst timestamps and the rows
// the descriptor knows (row 0, row count - 1) are closed form; any other
// row of a stream-coded list is left to k_rows_bounds_ts.
// (launch bounds: see top_clamp)
__global__ __launch_bounds__(256, 4) void k_rows_bounds(
    const uint8_t *__restrict__ payload, const uint8_t *__restrict__ sidecar,
    uint64_t limit, const bydb_block_desc *__restrict__ blocks,
    int64_t n_blocks, int64_t min_ts, int64_t max_ts, int flags, int desc,
    const PredBlock *__restrict__ preds, int n_preds,
    const uint64_t *__restrict__ pred_bm,
    const uint8_t *__restrict__ pred_flags, uint64_t *__restrict__ hi,
    uint64_t *__restrict__ lo, uint8_t *__restrict__ valid, DevErr *derr) {
    const int lane = threadIdx.x & 63;
    const int64_t wave_id =
        (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t bi = wave_id; bi < n_blocks; bi += n_waves) {
        const bydb_block_desc *bd = &blocks[bi];
        TopSel ts;
        if (!top_clamp(payload, bd, bi, min_ts, max_ts, flags, lane, derr,
                       &ts) ||
            !top_walkers(payload, sidecar, bi, n_blocks, preds, n_preds,
                         pred_bm, pred_flags, derr, &ts))
            continue;
        if (bd->field_enc == BYDB_ENC_PLAIN) {
            // null-bearing block: never return a null row as a value
            if (top_any_row(&ts, lane))
                dev_set_err(derr, DERR_TOP_NULL, (uint64_t)bi);
            continue;
        }
        int64_t row = -1;
        if (!ts.wp[0] && !ts.wp[1] && !ts.wp[2]) {
            row = desc ? ts.r1 : ts.r0;
        } else {
            // RLE walkers are forward cursors: descending keeps the last
            // match of the whole range, ascending stops at the first
            for (int64_t base = ts.r0; base <= ts.r1; base += WAVE) {
                const int64_t r = base + lane;
                const bool need = r <= ts.r1;
                const bool ok =
                    walkers_match(ts.wp[0], ts.wp[1], ts.wp[2], r, need) &&
                    need;
                const uint64_t m = __ballot(ok);
                if (!m) continue;
                if (desc) {
                    row = base + 63 - __clzll(m);
                } else {
                    row = base + __ffsll((unsigned long long)m) - 1;
                    break;
                }
            }
        }
        if (row < 0) continue;
        const int64_t n = (int64_t)bd->count;
        const uint8_t tenc = bd->ts_enc_with_version;
        const uint8_t tc = tenc >= BYDB_ENC_CONST_WV ? tenc - 4 : tenc;
        int64_t t = bd->ts_min;
        bool defer = false;
        if (row == 0 || tc == BYDB_ENC_CONST) {
            // ts_min
        } else if (row == n - 1) {
            t = bd->ts_max;
        } else if (tc == BYDB_ENC_DELTA_CONST) {
            if (bd->ts_off + 11 > limit) {
                dev_set_err(derr, DERR_BAD_STREAM, (uint64_t)bi);
                continue;
            }
            int vl;
            const int64_t dd = decode_one_varint(payload + bd->ts_off, &vl);
            t = (int64_t)((uint64_t)bd->ts_min + (uint64_t)row * (uint64_t)dd);
        } else if (tc == BYDB_ENC_DELTA || tc == BYDB_ENC_DELTA_OF_DELTA) {
            defer = true;
        } else {
            dev_set_err(derr, DERR_BAD_ENC, (uint64_t)bi);
            continue;
        }
        if (lane == 0) {
            lo[bi] = ~bd->series_id;
            hi[bi] = defer ? (uint64_t)row : top_key(t, desc == 0);
            valid[bi] = defer ? ROWS_DEFER : 1;
        }
    }
}

// Stage 1b — the deferred keys: one wave per workgroup, grid-stride, each
// workgroup decoding into its own slot of the (still free) row grid, as
// k_top_resolve does.  A 64-thread kernel for the decoder it calls.
__global__ __launch_bounds__(WAVE) void k_rows_bounds_ts(
    const uint8_t *__restrict__ payload, uint64_t limit,
    const bydb_block_desc *__restrict__ blocks, int64_t n_blocks, int desc,
    uint64_t *__restrict__ hi, uint8_t *__restrict__ valid,
    uint64_t *__restrict__ grid, DevErr *derr) {
    const int lane = threadIdx.x;
    int64_t *scratch = (int64_t *)(grid + (uint64_t)blockIdx.x * TOP_BLOCK_ROWS);
    // 64 validity bytes per step, one per lane; the deferred ones in turn
    for (int64_t base = (int64_t)blockIdx.x * WAVE; base < n_blocks;
         base += (int64_t)gridDim.x * WAVE) {
        uint64_t todo = __ballot(base + lane < n_blocks &&
                                 valid[base + lane] == ROWS_DEFER);
        for (; todo; todo &= todo - 1) {
            const int64_t bi = base + __ffsll((unsigned long long)todo) - 1;
            const bydb_block_desc *bd = &blocks[bi];
            const int64_t n = (int64_t)bd->count;
            const uint64_t row = hi[bi];
            if (n < 1 || n > TOP_BLOCK_ROWS || row >= (uint64_t)n) {
                dev_set_err(derr, DERR_BAD_ENC, (uint64_t)bi);
                if (lane == 0) valid[bi] = 0;
                continue;
            }
            const uint8_t tenc = bd->ts_enc_with_version;
            const uint8_t tc = tenc >= BYDB_ENC_CONST_WV ? tenc - 4 : tenc;
            dedup_decode_list(payload, bd->ts_off, limit, tc, bd->ts_min, n,
                              true, lane, scratch, derr, (uint64_t)bi);
            __threadfence();
            const int64_t t = scratch[row];
            __threadfence();   // read before the next block reuses the slot
            if (lane == 0) {
                hi[bi] = top_key(t, desc == 0);
                valid[bi] = 1;
            }
        }
    }
}

// ---- rows_select: top_select under a two-word key ----
// Best = hi descending, then lo descending, then index ascending.  The hi
// word goes through k_sel_hist / k_sel_pick unchanged: they leave the
// threshold T and the rank still open among entries with hi == T.  The
// same eight passes then run over lo for those entries only, and the stable
// count / scan / emit takes hi > T, or hi == T and lo above its threshold,
// or both equal in index order while the rank lasts.  lo is indexed through
// lo_map when given: entry i's word is lo[lo_map[i >> 13]] (a row's lo is
// its block's).
__device__ __forceinline__ uint64_t sel2_lo(const uint64_t *lo,
                                            const uint32_t *lo_map,
                                            uint64_t i) {
    return lo_map ? lo[lo_map[i >> 13]] : lo[i];
}

__global__ __launch_bounds__(256) void k_sel2_hist(
    const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo,
    const uint32_t *__restrict__ lo_map, const uint8_t *__restrict__ valid,
    uint64_t n, const TopSelState *st_hi, TopSelState *st, int pass) {
    __shared__ uint32_t h[256];
    if (st_hi->all) return;
    const uint64_t thr = st_hi->prefix;
    const uint64_t prefix = pass == 0 ? 0ull : st->prefix;
    const uint64_t mask = pass == 0 ? 0ull : ~0ull << (64 - 8 * pass);
    const int shift = 56 - 8 * pass;
    h[threadIdx.x] = 0;
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * 256) {
        if (!valid[i] || hi[i] != thr) continue;
        const uint64_t k = sel2_lo(lo, lo_map, i);
        if ((k & mask) == prefix) atomicAdd(&h[(k >> shift) & 255], 1u);
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&st->hist[threadIdx.x], h[threadIdx.x]);
}

// One workgroup of 256.  Pass 0 takes over the rank the hi passes left.
// Invariant: the entries with hi == T that match the prefix number at least
// `remaining`.
__global__ __launch_bounds__(256) void k_sel2_pick(const TopSelState *st_hi,
                                                   TopSelState *st, int pass) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = st->hist[threadIdx.x];
    st->hist[threadIdx.x] = 0;
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (pass == 0) {
        st->prefix = 0;
        st->remaining = st_hi->remaining;
        st->all = st_hi->all;
        st->n_out = 0;
    }
    if (st->all) return;
    uint32_t rem = st->remaining, cum = 0;
    int digit = 0;
    for (int b = 255; b >= 0; b--) {
        if (cum + h[b] >= rem) { digit = b; break; }
        cum += h[b];
    }
    st->prefix |= (uint64_t)digit << (56 - 8 * pass);
    st->remaining = rem - cum;
}

// sel_class under the two-word key
__device__ __forceinline__ uint32_t sel2_class(
    const uint64_t *hi, const uint64_t *lo, const uint32_t *lo_map,
    const uint8_t *valid, uint64_t i, uint64_t n, uint64_t thr_hi,
    uint64_t thr_lo, bool all) {
    if (i >= n || !valid[i]) return 0;
    if (all) return 2;
    const uint64_t h = hi[i];
    if (h != thr_hi) return h > thr_hi ? 2 : 0;
    const uint64_t l = sel2_lo(lo, lo_map, i);
    return l > thr_lo ? 2 : l == thr_lo ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_sel2_count(
    const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo,
    const uint32_t *__restrict__ lo_map, const uint8_t *__restrict__ valid,
    uint64_t n, const TopSelState *st_hi, const TopSelState *st,
    uint32_t *__restrict__ cnt_gt, uint32_t *__restrict__ cnt_eq) {
    __shared__ uint32_t s_gt, s_eq;
    if (threadIdx.x == 0) { s_gt = 0; s_eq = 0; }
    __syncthreads();
    const uint64_t thr_hi = st_hi->prefix, thr_lo = st->prefix;
    const bool all = st->all != 0;
    const uint64_t i0 = (uint64_t)blockIdx.x * TOP_CHUNK + threadIdx.x * 4;
    uint32_t g = 0, e = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint32_t c = sel2_class(hi, lo, lo_map, valid, i0 + k, n, thr_hi,
                                thr_lo, all);
        g += c == 2;
        e += c == 1;
    }
    if (g) atomicAdd(&s_gt, g);
    if (e) atomicAdd(&s_eq, e);
    __syncthreads();
    if (threadIdx.x == 0) {
        cnt_gt[blockIdx.x] = s_gt;
        cnt_eq[blockIdx.x] = s_eq;
    }
}

__global__ __launch_bounds__(256) void k_sel2_emit(
    const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo,
    const uint32_t *__restrict__ lo_map, const uint8_t *__restrict__ valid,
    uint64_t n, const TopSelState *st_hi, const TopSelState *st,
    const uint32_t *__restrict__ sel_before,
    const uint32_t *__restrict__ eq_before, uint32_t *__restrict__ out,
    uint32_t out_cap) {
    __shared__ uint32_t w4[4];
    const uint64_t thr_hi = st_hi->prefix, thr_lo = st->prefix;
    const bool all = st->all != 0;
    const uint32_t rem = all ? 0 : st->remaining;
    const uint64_t i0 = (uint64_t)blockIdx.x * TOP_CHUNK + threadIdx.x * 4;
    uint32_t cls[4], e = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        cls[k] = sel2_class(hi, lo, lo_map, valid, i0 + k, n, thr_hi, thr_lo,
                            all);
        e += cls[k] == 1;
    }
    uint32_t eq_rank = eq_before[blockIdx.x] + sel_block_scan(e, w4);
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (cls[k] == 1) cls[k] = eq_rank++ < rem ? 2 : 0;
        s += cls[k] == 2;
    }
    uint32_t at = sel_before[blockIdx.x] + sel_block_scan(s, w4);
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (cls[k] == 2) {
            if (at < out_cap) out[at] = (uint32_t)(i0 + k);
            at++;
        }
}

// Stage 3 — one wave per chosen block (ascending block index, so grid
// index order is seq order): the timestamp list decoded into the block's
// slot of the row grid, then every selected row's timestamp replaced by its
// key.  [r0, r1] comes from k_top_row_range; rvalid is pre-zeroed.
__global__ __launch_bounds__(WAVE) void k_rows_row_keys(
    const uint8_t *__restrict__ payload, const uint8_t *__restrict__ sidecar,
    uint64_t limit, const bydb_block_desc *__restrict__ blocks,
    int64_t n_blocks, int desc, const PredBlock *__restrict__ preds,
    int n_preds, const uint64_t *__restrict__ pred_bm,
    const uint8_t *__restrict__ pred_flags, const TopSelState *st,
    const uint32_t *__restrict__ chosen, const uint32_t *__restrict__ range,
    uint64_t *__restrict__ grid, uint8_t *__restrict__ rvalid, DevErr *derr) {
    const int lane = threadIdx.x;
    const uint32_t c = blockIdx.x;
    if (c >= st->n_out) return;
    const int64_t bi = (int64_t)chosen[c];
    if (bi >= n_blocks || range[c] == TOP_NO_ROWS) return;
    const bydb_block_desc *bd = &blocks[bi];
    TopSel ts;
    ts.r0 = (int64_t)(range[c] & 0xFFFFu);
    ts.r1 = (int64_t)(range[c] >> 16);
    ts.fdiff = 0;
    if (!top_walkers(payload, sidecar, bi, n_blocks, preds, n_preds, pred_bm,
                     pred_flags, derr, &ts))
        return;
    const int64_t n = (int64_t)bd->count;
    int64_t *tsv = (int64_t *)(grid + (uint64_t)c * TOP_BLOCK_ROWS);
    uint8_t *ok_out = rvalid + (uint64_t)c * TOP_BLOCK_ROWS;
    const uint8_t tenc = bd->ts_enc_with_version;
    const uint8_t tc = tenc >= BYDB_ENC_CONST_WV ? tenc - 4 : tenc;
    if (tc == BYDB_ENC_CONST) {
        for (int64_t i = lane; i < n; i += WAVE) tsv[i] = bd->ts_min;
    } else if (tc == BYDB_ENC_DELTA_CONST || tc == BYDB_ENC_DELTA ||
               tc == BYDB_ENC_DELTA_OF_DELTA) {
        dedup_decode_list(payload, bd->ts_off, limit, tc, bd->ts_min, n, true,
                          lane, tsv, derr, (uint64_t)bi);
    } else {
        dev_set_err(derr, DERR_BAD_ENC, (uint64_t)bi);
        return;
    }
    // the decode stores a row from whichever lane held its terminator
    __threadfence();
    for (int64_t base = ts.r0; base <= ts.r1; base += WAVE) {
        const int64_t row = base + lane;
        const bool need = row <= ts.r1;
        const bool ok =
            walkers_match(ts.wp[0], ts.wp[1], ts.wp[2], row, need) && need;
        if (ok) {
            tsv[row] = (int64_t)top_key(tsv[row], desc == 0);
            ok_out[row] = 1;
        }
    }
}

// Stage 5a — one thread per winner: series, seq and exponent from the grid
// index and the descriptor.  It runs before k_top_resolve (timestamp and
// version) and 5b, which reuse the grid as decode scratch.
__global__ __launch_bounds__(256) void k_rows_resolve_keys(
    const bydb_block_desc *__restrict__ blocks, int64_t n_blocks,
    const TopSelState *st_rows, const uint32_t *__restrict__ chosen,
    const uint32_t *__restrict__ winners, const uint64_t *__restrict__ grid,
    TopRec *__restrict__ recs, uint32_t cap) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= st_rows->n_out || i >= cap) return;
    const uint32_t idx = winners[i];
    const uint32_t row = idx & (TOP_BLOCK_ROWS - 1);
    const int64_t bi = (idx >> 13) < cap ? (int64_t)chosen[idx >> 13] : n_blocks;
    TopRec r = {};
    r.seq = ~0ull;   // no block: the later stages leave the record alone
    if (bi < n_blocks) {
        const bydb_block_desc *bd = &blocks[bi];
        r.series_id = bd->series_id;
        r.key = grid[idx];
        r.seq = ((uint64_t)bi << 13) | row;
        r.exp = bd->exp;
    }
    recs[i] = r;
}

// Stage 5b — one wave per winner, after k_top_resolve: the field value, in
// the winner's own block exponent, from a decode of the winner's field
// column into its slot of the grid (as k_top_row_keys decodes it).
__global__ __launch_bounds__(WAVE) void k_rows_resolve_field(
    const uint8_t *__restrict__ payload, uint64_t limit,
    const bydb_block_desc *__restrict__ blocks, int64_t n_blocks,
    const TopSelState *st_rows, uint64_t *__restrict__ grid,
    TopRec *__restrict__ recs, DevErr *derr) {
    const int lane = threadIdx.x;
    const uint32_t i = blockIdx.x;
    if (i >= st_rows->n_out) return;
    const uint64_t seq = recs[i].seq;
    const int64_t bi = (int64_t)(seq >> 13);
    const int64_t row = (int64_t)(seq & (TOP_BLOCK_ROWS - 1));
    if (bi >= n_blocks) return;
    const bydb_block_desc *bd = &blocks[bi];
    const int64_t n = (int64_t)bd->count;
    if (n < 1 || n > TOP_BLOCK_ROWS || row >= n) return;
    int64_t *scratch = (int64_t *)(grid + (uint64_t)i * TOP_BLOCK_ROWS);
    const uint8_t fenc = bd->field_enc;
    int64_t v = bd->field_first;
    if (fenc == BYDB_ENC_DELTA_CONST || fenc == BYDB_ENC_DELTA ||
        fenc == BYDB_ENC_DELTA_OF_DELTA) {
        if (bd->field_off & TAG_SIDECAR_BIT) {
            dev_set_err(derr, DERR_BAD_ENC, (uint64_t)bi);
            return;
        }
        dedup_decode_list(payload, bd->field_off, limit, fenc, bd->field_first,
                          n, false, lane, scratch, derr, (uint64_t)bi);
        __threadfence();
        v = scratch[row];
    } else if (fenc != BYDB_ENC_CONST) {
        // a Plain block never carries a valid key
        dev_set_err(derr, DERR_BAD_ENC, (uint64_t)bi);
        return;
    }
    if (lane == 0) recs[i].value = v;
}

// ---- tag projection for row results: fetch tag values by seq ----
// The reference decodes every projected tag column of each emitted row
// (blockCursor.copyTo / copyAllTo, block.go:509-776, through
// mustDecodeTagValue, query.go:641).  Here the winners of a top / row scan
// carry seq = (block << 13) | row, and this gather returns the stored cell
// bytes of up to BYDB_TAG_FETCH_MAX such rows on one tag slot: locate
// (one wave per row) -> offsets (one workgroup) -> copy (one wave per row).
// It reads the resident part only and writes none of the epoch's state.
//
// Bounds rule: every range is compared against its stream's end,
// [tag_off, tag_off + tag_len), before the load that would read it; a range
// that leaves the stream is TF_BAD_STREAM, never a read.
#define TF_VALUE 0
#define TF_NIL 1
#define TF_BAD_SEQ 2
#define TF_BAD_STREAM 3
#define TF_NONE 0xFFFFFFFFu

struct TagFetchRec {
    uint64_t src;      // arena offset of the value, TAG_SIDECAR_BIT as in descs
    uint32_t len;
    uint8_t status;    // TF_*
    uint8_t _p[3];
};

struct TagFetchResult {
    uint64_t total;         // bytes of all values
    uint32_t bad_seq;       // first request index with TF_BAD_SEQ, or TF_NONE
    uint32_t bad_stream;    // first request index with TF_BAD_STREAM
};

// rd_bits_be for a stream that ends at byte offset `end` of p: a byte at or
// past the end is not loaded and reads as 0 (rd_bits_be always gathers 8)
__device__ __forceinline__ uint64_t rd_bits_be_in(const uint8_t *p,
                                                  uint64_t bitpos, uint32_t n,
                                                  uint64_t end) {
    uint64_t byte = bitpos >> 3;
    uint32_t sh = (uint32_t)(bitpos & 7);
    uint64_t acc = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint64_t at = byte + (uint64_t)i;
        acc = (acc << 8) | (at < end ? p[at] : 0);
    }
    return (acc >> (64 - sh - n)) & ((1ull << n) - 1);
}

// The dictionary code of `row`: the bit-packed RLE (code, count) pairs 64
// runs per step, one pair per lane; a wave scan of the counts plus the total
// carried over from the steps before finds the first run whose running total
// exceeds `row`.  -1 when the runs end before the row.  The caller has
// checked that the entries lie inside the stream and that 1 <= width <= 32.
__device__ __forceinline__ int64_t tag_fetch_code(const DictStream &ds,
                                                  uint64_t end, uint32_t row,
                                                  int lane) {
    const uint32_t nruns = ds.nentries >> 1;
    uint64_t carried = 0;
    for (uint32_t r0 = 0; r0 < nruns; r0 += WAVE) {
        const uint32_t r = r0 + (uint32_t)lane;
        uint64_t code = 0, cnt = 0;
        if (r < nruns) {
            uint64_t bit = ds.bit0 + (uint64_t)(2 * r) * ds.width;
            code = rd_bits_be_in(ds.base, bit, ds.width, end);
            cnt = rd_bits_be_in(ds.base, bit + ds.width, ds.width, end);
        }
        uint64_t incl = carried + wave_incl_scan(cnt, lane);
        uint64_t hit = __ballot(r < nruns && incl > (uint64_t)row);
        if (hit)
            return (int64_t)__shfl((unsigned long long)code,
                                   (int)__builtin_ctzll(hit));
        carried = readlane64(incl, WAVE - 1);
    }
    return -1;
}

__global__ __launch_bounds__(WAVE) void k_tag_fetch_locate(
    const uint8_t *__restrict__ payload, const uint8_t *__restrict__ sidecar,
    const bydb_block_desc *__restrict__ blocks, int64_t n_blocks,
    const uint64_t *__restrict__ seqs, int64_t n, int slot,
    TagFetchRec *__restrict__ recs) {
    const int lane = threadIdx.x;
    const int64_t i = blockIdx.x;
    if (i >= n) return;
    const uint64_t seq = seqs[i];
    const uint64_t bi = seq >> 13;
    const uint32_t row = (uint32_t)(seq & 8191);
    TagFetchRec rec;
    rec.src = 0; rec.len = 0; rec.status = TF_NIL;
    rec._p[0] = rec._p[1] = rec._p[2] = 0;
    // every exit below is wave-uniform: seq, the descriptor and the stream
    // header are the same for all lanes
    if (bi >= (uint64_t)n_blocks || row >= blocks[bi].count) {
        rec.status = TF_BAD_SEQ;
        if (lane == 0) recs[i] = rec;
        return;
    }
    const bydb_block_desc *bd = &blocks[bi];
    DictStream ds;
    const int kind = tag_open(payload, sidecar, bd, slot, &ds);
    if (kind == TS_NIL) {
        if (lane == 0) recs[i] = rec;
        return;
    }
    rec.status = TF_BAD_STREAM;
    uint64_t toff, tlen;
    tag_slot(bd, slot, &toff, &tlen);
    const uint64_t side = toff & TAG_SIDECAR_BIT;
    const uint64_t end = (toff & ~TAG_SIDECAR_BIT) + tlen;  // offset in base
    if (kind == TS_DICT) {
        // sections in order, all inside the stream: lengths, values, the
        // 5-byte entry header, the packed entries
        const uint64_t lens_off = (uint64_t)(ds.lens - ds.base);
        const uint64_t vals_off = (uint64_t)(ds.vals - ds.base);
        const uint64_t ent_off = ds.bit0 >> 3;
        const uint64_t ent_bits = (uint64_t)ds.nentries * ds.width;
        bool ok = ds.count <= tlen && vals_off <= end && ent_off <= end &&
                  lens_off + ds.count * ds.wbytes <= vals_off &&
                  ds.width >= 1 && ds.width <= 32 &&
                  ent_bits <= (end - ent_off) * 8;
        int64_t code = ok ? tag_fetch_code(ds, end, row, lane) : -1;
        if (code >= 0 && (uint64_t)code < ds.count) {
            // the value's offset: the stored lengths of the values below
            // the code, lanes striding the list, one wave reduction
            uint64_t part = 0;
            for (uint64_t v = (uint64_t)lane; v < (uint64_t)code; v += WAVE) {
                uint64_t alen = be_len(ds.lens, v, ds.wbytes);
                part += alen ? alen - 1 : 0;
            }
            const uint64_t voff = wave_reduce_add(part);
            const uint64_t alen = be_len(ds.lens, (uint64_t)code, ds.wbytes);
            const uint64_t avail = ent_off - 5 - vals_off;   // values section
            if (alen == 0) {
                rec.status = TF_NIL;
            } else if (ent_off >= vals_off + 5 && voff <= avail &&
                       alen - 1 <= avail - voff) {
                rec.status = TF_VALUE;
                rec.len = (uint32_t)(alen - 1);
                rec.src = (vals_off + voff) | side;
            }
        }
    } else if (kind == TS_PLAIN && side && tlen >= 6) {
        // a plain column reaches the device only host-normalised
        PlainStream ps;
        if (plain_open(payload, sidecar, bd, slot, &ps)) {
            const uint64_t hdr = (toff & ~TAG_SIDECAR_BIT) + 6;
            const uint64_t vals_off = hdr + ps.n * ps.wbytes;   // n <= 8192
            if (vals_off <= end) {
                uint64_t carry = 0;
                PlainRow r = {};
                for (uint64_t base = 0; base <= (uint64_t)row; base += WAVE)
                    r = plain_chunk(ps, base, lane, &carry);
                const uint64_t lp1 =
                    __shfl((unsigned long long)r.lp1, (int)(row & 63));
                const uint64_t off =
                    __shfl((unsigned long long)r.off, (int)(row & 63));
                const uint64_t avail = end - vals_off;
                if (lp1 == 0) {
                    rec.status = TF_NIL;
                } else if (off <= avail && lp1 - 1 <= avail - off) {
                    rec.status = TF_VALUE;
                    rec.len = (uint32_t)(lp1 - 1);
                    rec.src = (vals_off + off) | side;
                }
            }
        }
    }
    if (lane == 0) recs[i] = rec;
}

// One workgroup: offs[0..n] is the exclusive scan of the n value lengths,
// nil[i] the nil flag; the first bad index of each kind goes to *res, so the
// host reads one struct.
__global__ __launch_bounds__(BYDB_TAG_FETCH_MAX) void k_tag_fetch_offsets(
    const TagFetchRec *__restrict__ recs, int64_t n,
    uint64_t *__restrict__ offs, uint8_t *__restrict__ nil,
    TagFetchResult *__restrict__ res) {
    __shared__ uint64_t wave_tot[BYDB_TAG_FETCH_MAX / WAVE];
    __shared__ uint32_t bad[2];
    const int t = threadIdx.x;
    const int lane = t & (WAVE - 1);
    const int w = t / WAVE;
    if (t < 2) bad[t] = TF_NONE;
    __syncthreads();
    uint64_t len = 0;
    if (t < n) {
        const TagFetchRec r = recs[t];
        if (r.status == TF_VALUE) len = r.len;
        nil[t] = r.status == TF_VALUE ? 0 : 1;
        if (r.status == TF_BAD_SEQ) atomicMin(&bad[0], (uint32_t)t);
        if (r.status == TF_BAD_STREAM) atomicMin(&bad[1], (uint32_t)t);
    }
    const uint64_t incl = wave_incl_scan(len, lane);
    if (lane == WAVE - 1) wave_tot[w] = incl;
    __syncthreads();
    uint64_t before = 0, total = 0;
    for (int k = 0; k < BYDB_TAG_FETCH_MAX / WAVE; k++) {
        if (k < w) before += wave_tot[k];
        total += wave_tot[k];
    }
    if (t < n) offs[t] = before + incl - len;
    if (t == 0) {
        offs[n] = total;
        res->total = total;
        res->bad_seq = bad[0];
        res->bad_stream = bad[1];
    }
}

// one wave per row: len bytes from the value to out + offs[i], 64 a step
__global__ __launch_bounds__(WAVE) void k_tag_fetch_copy(
    const uint8_t *__restrict__ payload, const uint8_t *__restrict__ sidecar,
    const TagFetchRec *__restrict__ recs, const uint64_t *__restrict__ offs,
    int64_t n, uint8_t *__restrict__ out) {
    const int64_t i = blockIdx.x;
    if (i >= n) return;
    const TagFetchRec r = recs[i];
    if (r.status != TF_VALUE) return;
    const uint8_t *src = ((r.src & TAG_SIDECAR_BIT) ? sidecar : payload) +
                         (r.src & ~TAG_SIDECAR_BIT);
    uint8_t *dst = out + offs[i];
    for (uint32_t k = threadIdx.x; k < r.len; k += WAVE) dst[k] = src[k];
}

// ===================== host session =====================

struct bydb_session {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    std::string err;
    // part residency
    uint8_t *d_payload = nullptr;
    uint64_t payload_cap = 0, payload_len = 0;
    int64_t part_ts_min = INT64_MAX, part_ts_max = INT64_MIN;
    bydb_block_desc *d_blocks = nullptr;
    int64_t blocks_cap = 0, n_blocks = 0;
    // aggregation config
    int field_vtype = BYDB_VT_INT64;
    uint32_t func_mask = 0;
    uint32_t n_groups = 0;
    int mode = BYDB_MODE_ALL;
    bydb_partial *d_partials = nullptr;   // owned buffer
    bydb_partial *d_acc = nullptr;        // active accumulation target
    uint64_t partials_cap = 0;
    DevErr *d_err = nullptr;
    PredBlock *d_preds = nullptr;
    int64_t preds_cap = 0;
    // per-row group-by on dictionary tags (composite keys over <=3 slots)
    int n_gslots = 0;                  // 0 = group by block group_code
    int gslots[3] = {-1, -1, -1};
    int64_t gmul[3] = {1, 1, 1};
    GroupBlock *d_groups = nullptr;    // [slot][block]
    uint16_t *d_gmap = nullptr;        // [slot][block][256]
    int64_t groups_cap = 0;
    bool groups_built = false;
    // plain-tag group-by: (gid,count) run pairs per normalized plain
    // stream on a grouped slot (k_resolve_plain_groups)
    uint16_t *d_gruns = nullptr;
    uint64_t gruns_cap_streams = 0;
    uint32_t *d_grun_ctr = nullptr;
    uint8_t *d_dom_blob[3] = {};
    uint64_t *d_dom_offs[3] = {};
    uint64_t *d_dom_hashes[3] = {};
    uint32_t *d_dom_gids[3] = {};
    uint32_t dom_table_size[3] = {};
    uint32_t dom_n[3] = {};
    // tag conditions: literals + IN-set tables of the last consume, and
    // the host staging copy they upload from
    uint8_t *d_filter = nullptr;
    uint64_t filter_cap = 0;
    std::vector<uint8_t> filter_stage;
    // plain (non-dictionary) tag columns: host-normalized sidecar arena +
    // per-row match bitmaps filled by k_resolve_plain_filter
    uint8_t *d_sidecar = nullptr;
    uint64_t sidecar_len = 0, sidecar_cap = 0;
    uint64_t n_plain_host = 0;  // (block,slot) plain streams normalized
    uint32_t *d_plain_ctr = nullptr;
    uint64_t *d_pred_bm = nullptr;
    uint64_t pred_bm_cap = 0;  // words
    uint8_t *d_pred_flags = nullptr;
    int64_t pred_flags_cap = 0;
    uint32_t *d_walk_count = nullptr;
    // criteria trees: per-class block counts of the last tree consume
    // (k_resolve_tree), read back once on the OR path
    uint32_t *d_tree_stats = nullptr;
    uint64_t tree_stats[4] = {0, 0, 0, 0};
    uint64_t *d_first_seen = nullptr;
    uint64_t first_seen_cap = 0;
    float last_ms = 0.0f;
    bool consumed = false;
    int16_t float_exp = 0;  // shared decimal exponent for float64 restore
    int stream_policy = BYDB_STREAM_AUTO;  // dense-stream load policy
    // cross-part version dedup (bydb_set_row_dedup): derived state over
    // the resident part, built on the first consume with dedup on
    int row_dedup = 0;
    bool dedup_built = false;
    uint64_t dedup_stats[4] = {0, 0, 0, 0};
    int64_t dd_n_inv = 0, dd_n_partial = 0, dd_n_full = 0;
    DedupInfo *d_dd_infos = nullptr;
    uint64_t *d_dd_peer_offs = nullptr;
    uint32_t *d_dd_peers = nullptr;
    int64_t *d_dd_arena = nullptr;
    uint64_t *d_dd_surv = nullptr;
    uint32_t *d_dd_plist = nullptr, *d_dd_flist = nullptr;
    unsigned long long *d_dd_ctr = nullptr;
    uint64_t dd_bm_base = 0;   // first pred_bm word of the merged bitmaps
    // nibble-packed dense field streams (bydb_set_field_pack): derived
    // state over the resident part, built on the first consume that reads
    // it.  d_pack: the slot table (n_blocks x u32) followed by the slots;
    // null when the build packed nothing.
    int field_pack = BYDB_PACK_AUTO;
    bool pack_built = false;
    uint8_t *d_pack = nullptr;
    unsigned long long *d_pack_ctr = nullptr;
    uint64_t pack_stats[4] = {0, 0, 0, 0};
    // BatchTop over raw rows (bydb_top_configure): the session selects rows
    // instead of folding them.  Everything below is scratch of one consume;
    // the row grid is sized once from top_n.
    bool top_on = false;
    int64_t top_n = 0;
    int top_asc = 0;
    uint64_t *d_top_bkeys = nullptr;    // [n_blocks] best-value keys
    uint8_t *d_top_bvalid = nullptr;
    int64_t top_blocks_cap = 0;
    uint64_t *d_top_grid = nullptr;     // [top_n][8192] row keys
    uint8_t *d_top_rvalid = nullptr;
    uint32_t *d_top_chosen = nullptr;   // [top_n] block indices
    uint32_t *d_top_winners = nullptr;  // [top_n] grid indices
    uint32_t *d_top_range = nullptr;    // [top_n] clamped rows per chosen block
    TopRec *d_top_recs = nullptr;       // [top_n]
    int64_t top_grid_cap = 0;           // in blocks (= top_n it was sized for)
    uint32_t *d_top_cnt = nullptr;      // selector chunk counters, 2 arrays
    uint64_t top_cnt_cap = 0;           // chunks per array
    TopSelState *d_top_st = nullptr;    // [2]: block select, row select
    // Scan -> Limit over raw rows (bydb_rows_configure): the session returns
    // rows [offset, offset + limit) of the time-ordered selection.  It
    // shares the top session's scratch; its own are the second key word per
    // block and the selector states of the two-word selects.
    bool rows_on = false;
    int64_t rows_offset = 0, rows_limit = 0;
    int rows_desc = 0;
    uint64_t *d_rows_blo = nullptr;     // [n_blocks] ~series_id
    int64_t rows_blocks_cap = 0;
    TopSelState *d_rows_st = nullptr;   // [4]: blocks hi, lo; rows hi, lo
    // Tag projection (bydb_rows_fetch_tags): the request / record / offsets
    // scratch of one call, a fixed size (TfLayout), and the output arena,
    // which grows on demand.  Nothing here grows with the part.
    uint8_t *d_tf = nullptr;
    uint8_t *d_tf_out = nullptr;
    uint64_t tf_out_cap = 0;
};

// What a read-once pass has to exceed before its loads bypass the caches:
// the MI355X Infinity Cache (256 MiB).  A smaller resident part is served
// from that cache pass after pass, and non-temporal loads would turn those
// hits into HBM reads.
static const uint64_t STREAM_CACHE_BYTES = 256ull << 20;

extern "C" int bydb_stream_policy_pick(int policy, uint64_t payload_bytes) {
    if (policy == BYDB_STREAM_CACHED) return BYDB_STREAM_CACHED;
    if (policy == BYDB_STREAM_STREAMING) return BYDB_STREAM_STREAMING;
    if (policy != BYDB_STREAM_AUTO) return BYDB_ERR_BAD_ARG;
    return payload_bytes > STREAM_CACHE_BYTES ? BYDB_STREAM_STREAMING
                                              : BYDB_STREAM_CACHED;
}

extern "C" int bydb_set_stream_policy(bydb_session *s, int policy) {
    if (policy != BYDB_STREAM_AUTO && policy != BYDB_STREAM_CACHED &&
        policy != BYDB_STREAM_STREAMING) {
        s->err = "unknown stream policy";
        return BYDB_ERR_BAD_ARG;
    }
    s->stream_policy = policy;
    return BYDB_OK;
}

// Grid caps of the per-block kernels (host side only; the kernels go round a
// grid-stride loop past them).  tests/test_loop_trips_cpu.py reads these two
// lines: its parts must stay larger than both.
// k_scan_agg_t, k_top_bounds, k_rows_bounds: 256-thread workgroups, one wave
// per block
#define SCAN_MAX_WGS 8192
// the 64-thread kernels that take one block per workgroup
#define BLOCK_KERNEL_MAX_WGS 65535

#define HIP_TRY(s, call)                                                      \
    do {                                                                      \
        hipError_t _e = (call);                                               \
        if (_e != hipSuccess) {                                               \
            (s)->err = std::string(#call) + ": " + hipGetErrorString(_e);     \
            return BYDB_ERR_HIP;                                              \
        }                                                                     \
    } while (0)

static void dedup_free(bydb_session *s) {
    if (s->d_dd_infos) (void)hipFree(s->d_dd_infos);
    if (s->d_dd_peer_offs) (void)hipFree(s->d_dd_peer_offs);
    if (s->d_dd_peers) (void)hipFree(s->d_dd_peers);
    if (s->d_dd_arena) (void)hipFree(s->d_dd_arena);
    if (s->d_dd_surv) (void)hipFree(s->d_dd_surv);
    if (s->d_dd_plist) (void)hipFree(s->d_dd_plist);
    if (s->d_dd_flist) (void)hipFree(s->d_dd_flist);
    if (s->d_dd_ctr) (void)hipFree(s->d_dd_ctr);
    s->d_dd_infos = nullptr; s->d_dd_peer_offs = nullptr;
    s->d_dd_peers = nullptr; s->d_dd_arena = nullptr;
    s->d_dd_surv = nullptr; s->d_dd_plist = nullptr;
    s->d_dd_flist = nullptr; s->d_dd_ctr = nullptr;
}

static void pack_free(bydb_session *s) {
    if (s->d_pack) (void)hipFree(s->d_pack);
    s->d_pack = nullptr;
    for (int i = 0; i < 4; i++) s->pack_stats[i] = 0;
}

static void top_free(bydb_session *s) {
    void *ptrs[] = {s->d_top_bkeys, s->d_top_bvalid, s->d_top_grid,
                    s->d_top_rvalid, s->d_top_chosen, s->d_top_winners,
                    s->d_top_recs, s->d_top_cnt, s->d_top_st,
                    s->d_top_range, s->d_rows_blo, s->d_rows_st};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    s->d_top_bkeys = nullptr; s->d_top_bvalid = nullptr;
    s->d_top_grid = nullptr; s->d_top_rvalid = nullptr;
    s->d_top_chosen = nullptr; s->d_top_winners = nullptr;
    s->d_top_recs = nullptr; s->d_top_cnt = nullptr; s->d_top_st = nullptr;
    s->d_top_range = nullptr;
    s->d_rows_blo = nullptr; s->d_rows_st = nullptr;
    s->rows_blocks_cap = 0;
    s->top_blocks_cap = 0; s->top_grid_cap = 0; s->top_cnt_cap = 0;
}

extern "C" bydb_session *bydb_session_create(int device) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= device) {
        fprintf(stderr, "bydb_session_create: hipGetDeviceCount=%s n=%d dev=%d\n",
                hipGetErrorString(e), n, device);
        return nullptr;
    }
    if ((e = hipSetDevice(device)) != hipSuccess) {
        fprintf(stderr, "bydb_session_create: hipSetDevice=%s\n", hipGetErrorString(e));
        return nullptr;
    }
    bydb_session *s = new bydb_session();
    s->device = device;
    if ((e = hipStreamCreate(&s->stream)) != hipSuccess ||
        (e = hipEventCreate(&s->ev_start)) != hipSuccess ||
        (e = hipEventCreate(&s->ev_stop)) != hipSuccess ||
        (e = hipMalloc(&s->d_err, sizeof(DevErr))) != hipSuccess ||
        (e = hipMalloc(&s->d_plain_ctr, sizeof(uint32_t))) != hipSuccess) {
        fprintf(stderr, "bydb_session_create: init failed: %s\n", hipGetErrorString(e));
        delete s;
        return nullptr;
    }
    (void)hipMemset(s->d_err, 0, sizeof(DevErr));
    (void)hipMemset(s->d_plain_ctr, 0, sizeof(uint32_t));
    return s;
}

extern "C" void bydb_session_destroy(bydb_session *s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->d_payload) (void)hipFree(s->d_payload);
    if (s->d_blocks) (void)hipFree(s->d_blocks);
    if (s->d_partials) (void)hipFree(s->d_partials);
    if (s->d_preds) (void)hipFree(s->d_preds);
    if (s->d_filter) (void)hipFree(s->d_filter);
    if (s->d_groups) (void)hipFree(s->d_groups);
    if (s->d_gmap) (void)hipFree(s->d_gmap);
    if (s->d_gruns) (void)hipFree(s->d_gruns);
    if (s->d_grun_ctr) (void)hipFree(s->d_grun_ctr);
    for (int sl = 0; sl < 3; sl++) {
        if (s->d_dom_blob[sl]) (void)hipFree(s->d_dom_blob[sl]);
        if (s->d_dom_offs[sl]) (void)hipFree(s->d_dom_offs[sl]);
        if (s->d_dom_hashes[sl]) (void)hipFree(s->d_dom_hashes[sl]);
        if (s->d_dom_gids[sl]) (void)hipFree(s->d_dom_gids[sl]);
    }
    if (s->d_err) (void)hipFree(s->d_err);
    if (s->d_sidecar) (void)hipFree(s->d_sidecar);
    if (s->d_plain_ctr) (void)hipFree(s->d_plain_ctr);
    if (s->d_pred_bm) (void)hipFree(s->d_pred_bm);
    if (s->d_pred_flags) (void)hipFree(s->d_pred_flags);
    if (s->d_walk_count) (void)hipFree(s->d_walk_count);
    if (s->d_tree_stats) (void)hipFree(s->d_tree_stats);
    if (s->d_first_seen) (void)hipFree(s->d_first_seen);
    dedup_free(s);
    pack_free(s);
    top_free(s);
    if (s->d_tf) (void)hipFree(s->d_tf);
    if (s->d_tf_out) (void)hipFree(s->d_tf_out);
    if (s->d_pack_ctr) (void)hipFree(s->d_pack_ctr);
    if (s->ev_start) (void)hipEventDestroy(s->ev_start);
    if (s->ev_stop) (void)hipEventDestroy(s->ev_stop);
    if (s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
}

extern "C" const char *bydb_last_error(bydb_session *s) {
    return s ? s->err.c_str() : "null session";
}

extern "C" int bydb_part_reserve(bydb_session *s, uint64_t payload_bytes,
                                 int64_t n_blocks) {
    HIP_TRY(s, hipSetDevice(s->device));
    if (s->d_payload) { (void)hipFree(s->d_payload); s->d_payload = nullptr; }
    if (s->d_blocks) { (void)hipFree(s->d_blocks); s->d_blocks = nullptr; }
    // the packed copy of the old part goes before the new payload is
    // allocated: it is up to half the old payload again
    pack_free(s);
    // +4KiB slack: the 256-byte quad-window loop runs an 8-window-deep
    // load pipeline (2 KiB of lead) and may read past the last stream's
    // end
    HIP_TRY(s, hipMalloc(&s->d_payload, payload_bytes + 4096));
    HIP_TRY(s, hipMemset(s->d_payload + payload_bytes, 0, 4096));
    HIP_TRY(s, hipMalloc(&s->d_blocks, sizeof(bydb_block_desc) * (size_t)n_blocks));
    s->payload_cap = payload_bytes;
    s->blocks_cap = n_blocks;
    s->payload_len = 0;
    s->n_blocks = 0;
    s->part_ts_min = INT64_MAX;
    s->part_ts_max = INT64_MIN;
    s->sidecar_len = 0;
    s->n_plain_host = 0;
    s->groups_built = false;
    s->dedup_built = false;
    s->pack_built = false;
    return BYDB_OK;
}

extern "C" int bydb_part_append(bydb_session *s, const uint8_t *payload,
                                uint64_t len, const bydb_block_desc *blocks,
                                int64_t n_blocks) {
    HIP_TRY(s, hipSetDevice(s->device));
    s->groups_built = false;
    s->dedup_built = false;
    s->pack_built = false;
    if (s->payload_len + len > s->payload_cap ||
        s->n_blocks + n_blocks > s->blocks_cap) {
        s->err = "part_append exceeds reservation";
        return BYDB_ERR_BAD_ARG;
    }
    // Plain (non-dictionary) tag columns are zstd-compressed in the part;
    // normalize them here — where the reference decompresses at part open
    // (zstd.go:49) — into the sidecar arena, and repoint the stored
    // descriptor (TAG_SIDECAR_BIT).  The payload arena layout is untouched
    // so later chunks' absolute offsets stay valid.
    std::vector<bydb_block_desc> fixed;
    std::vector<uint8_t> extra;
    const uint64_t part_end = s->payload_len + len;
    for (int64_t i = 0; i < n_blocks; i++) {
        const bydb_block_desc *bd = &blocks[i];
        if (bd->ts_min < s->part_ts_min) s->part_ts_min = bd->ts_min;
        if (bd->ts_max > s->part_ts_max) s->part_ts_max = bd->ts_max;
        // loud host-side validation: every stream the descriptor names
        // must lie inside the part appended so far (catches builders whose
        // offset base drifted from this session's arena)
        if (bd->ts_off + bd->ts_len > part_end ||
            bd->field_off + bd->field_len > part_end ||
            (bd->tag_len && bd->tag_off + bd->tag_len > part_end) ||
            (bd->tag2_len && bd->tag2_off + bd->tag2_len > part_end) ||
            (bd->tag3_len && bd->tag3_off + bd->tag3_len > part_end)) {
            s->err = "descriptor stream offsets exceed appended payload";
            return BYDB_ERR_BAD_ARG;
        }
        for (int sl = 0; sl < 3; sl++) {
            uint64_t toff = sl == 0 ? bd->tag_off
                                    : sl == 1 ? bd->tag2_off : bd->tag3_off;
            uint64_t tlen = sl == 0 ? bd->tag_len
                                    : sl == 1 ? bd->tag2_len : bd->tag3_len;
            if (tlen == 0 || (toff & TAG_SIDECAR_BIT)) continue;
            if (toff < s->payload_len || toff + tlen > s->payload_len + len)
                continue;  // stream not in this chunk: leave as-is
            const uint8_t *src = payload + (toff - s->payload_len);
            std::vector<uint8_t> norm;
            if (src[0] == BYDB_ENC_PLAIN) {
                if (!bydb_normalize_plain_tag(src, tlen, bd->count, norm)) {
                    s->err = "plain tag column normalization failed";
                    return BYDB_ERR_BAD_DATA;
                }
                s->n_plain_host++;
            } else if (src[0] == BYDB_ENC_DICTIONARY) {
                // dictionaries whose compress_block sections are zstd'd
                // (>=128 B) get the same host decompress; small plain
                // dictionaries parse on device untouched
                bool needed = false;
                if (!bydb_normalize_dict_tag(src, tlen, &needed, norm)) {
                    if (needed) {
                        s->err = "dictionary tag normalization failed";
                        return BYDB_ERR_BAD_DATA;
                    }
                    continue;
                }
                if (!needed) continue;
            } else {
                continue;
            }
            if (fixed.empty()) fixed.assign(blocks, blocks + n_blocks);
            uint64_t noff = TAG_SIDECAR_BIT | (s->sidecar_len + extra.size());
            bydb_block_desc &fd = fixed[(size_t)i];
            if (sl == 0) { fd.tag_off = noff; fd.tag_len = norm.size(); }
            else if (sl == 1) { fd.tag2_off = noff; fd.tag2_len = norm.size(); }
            else { fd.tag3_off = noff; fd.tag3_len = norm.size(); }
            extra.insert(extra.end(), norm.begin(), norm.end());
        }
        // null-bearing Plain FIELD columns (8-B sign-flip cell blocks):
        // normalize into the sidecar as bitmap + fixed cells so the fold
        // can skip nulls per row (aggregation.go:310 null check)
        if (bd->field_enc == BYDB_ENC_PLAIN &&
            !(bd->field_off & TAG_SIDECAR_BIT)) {
            const uint8_t *fsrc = payload + (bd->field_off - s->payload_len);
            std::vector<uint8_t> norm;
            if (!bydb_normalize_plain_field(fsrc, bd->field_len, bd->count,
                                            norm)) {
                s->err = "plain field column normalization failed";
                return BYDB_ERR_BAD_DATA;
            }
            if (fixed.empty()) fixed.assign(blocks, blocks + n_blocks);
            while ((s->sidecar_len + extra.size()) & 7) extra.push_back(0);
            bydb_block_desc &fd = fixed[(size_t)i];
            fd.field_off = TAG_SIDECAR_BIT | (s->sidecar_len + extra.size());
            fd.field_len = norm.size();
            extra.insert(extra.end(), norm.begin(), norm.end());
        }
    }
    if (!extra.empty()) {
        uint64_t need = s->sidecar_len + extra.size() + 64;
        if (need > s->sidecar_cap) {
            uint64_t ncap = s->sidecar_cap ? s->sidecar_cap : 4096;
            while (ncap < need) ncap *= 2;
            uint8_t *nb = nullptr;
            HIP_TRY(s, hipMalloc(&nb, ncap));
            if (s->sidecar_len)
                HIP_TRY(s, hipMemcpy(nb, s->d_sidecar, s->sidecar_len,
                                     hipMemcpyDeviceToDevice));
            if (s->d_sidecar) (void)hipFree(s->d_sidecar);
            s->d_sidecar = nb;
            s->sidecar_cap = ncap;
        }
        HIP_TRY(s, hipMemcpy(s->d_sidecar + s->sidecar_len, extra.data(),
                             extra.size(), hipMemcpyHostToDevice));
        s->sidecar_len += extra.size();
    }
    HIP_TRY(s, hipMemcpy(s->d_payload + s->payload_len, payload, len,
                         hipMemcpyHostToDevice));
    HIP_TRY(s, hipMemcpy(s->d_blocks + s->n_blocks,
                         fixed.empty() ? blocks : fixed.data(),
                         sizeof(bydb_block_desc) * (size_t)n_blocks,
                         hipMemcpyHostToDevice));
    s->payload_len += len;
    s->n_blocks += n_blocks;
    return BYDB_OK;
}

// The derived state (groups, dedup survivors, packed copy) is not
// invalidated here: with n_blocks == 0 no scan reads any of it, and the
// append that makes the part non-empty again invalidates all three.
extern "C" int bydb_part_clear(bydb_session *s) {
    s->payload_len = 0;
    s->n_blocks = 0;
    s->part_ts_min = INT64_MAX;
    s->part_ts_max = INT64_MIN;
    s->sidecar_len = 0;
    s->n_plain_host = 0;
    return BYDB_OK;
}

extern "C" int bydb_agg_configure(bydb_session *s, int field_vtype,
                                  uint32_t func_mask, uint32_t n_groups,
                                  int mode) {
    HIP_TRY(s, hipSetDevice(s->device));
    if (n_groups < 1) { s->err = "n_groups < 1"; return BYDB_ERR_BAD_ARG; }
    s->top_on = false;   // a BatchAggregation operator again
    s->rows_on = false;
    s->field_vtype = field_vtype;
    s->func_mask = func_mask;
    s->n_groups = n_groups;
    s->mode = mode;
    if (s->partials_cap < n_groups) {
        if (s->d_partials) (void)hipFree(s->d_partials);
        HIP_TRY(s, hipMalloc(&s->d_partials, sizeof(bydb_partial) * n_groups));
        s->partials_cap = n_groups;
    }
    if (s->first_seen_cap < n_groups) {
        if (s->d_first_seen) (void)hipFree(s->d_first_seen);
        HIP_TRY(s, hipMalloc(&s->d_first_seen, sizeof(uint64_t) * n_groups));
        s->first_seen_cap = n_groups;
    }
    s->d_acc = s->d_partials;
    s->n_gslots = 0;
    return bydb_reset(s);
}

// Load one slot's group domain onto the device (open-addressing table,
// equality by bytes).
static int load_domain(bydb_session *s, int pos, const uint8_t *dom_blob,
                       const uint64_t *dom_offs, uint32_t n_values) {
    uint32_t tsize = 4;
    while (tsize < n_values * 4) tsize <<= 1;
    std::vector<uint64_t> hashes(tsize, 0);
    std::vector<uint32_t> gids(tsize, GID_NONE);
    for (uint32_t g = 0; g < n_values; g++) {
        const uint8_t *v = dom_blob + dom_offs[g];
        uint64_t len = dom_offs[g + 1] - dom_offs[g];
        uint64_t h = fnv1a(v, len);
        uint32_t sl = (uint32_t)h & (tsize - 1);
        while (gids[sl] != GID_NONE) sl = (sl + 1) & (tsize - 1);
        hashes[sl] = h;
        gids[sl] = g;
    }
    uint64_t blob_len = dom_offs[n_values];
    if (s->d_dom_blob[pos]) { (void)hipFree(s->d_dom_blob[pos]); s->d_dom_blob[pos] = nullptr; }
    if (s->d_dom_offs[pos]) { (void)hipFree(s->d_dom_offs[pos]); s->d_dom_offs[pos] = nullptr; }
    if (s->d_dom_hashes[pos]) { (void)hipFree(s->d_dom_hashes[pos]); s->d_dom_hashes[pos] = nullptr; }
    if (s->d_dom_gids[pos]) { (void)hipFree(s->d_dom_gids[pos]); s->d_dom_gids[pos] = nullptr; }
    HIP_TRY(s, hipMalloc(&s->d_dom_blob[pos], blob_len ? blob_len : 1));
    HIP_TRY(s, hipMalloc(&s->d_dom_offs[pos], sizeof(uint64_t) * (n_values + 1)));
    HIP_TRY(s, hipMalloc(&s->d_dom_hashes[pos], sizeof(uint64_t) * tsize));
    HIP_TRY(s, hipMalloc(&s->d_dom_gids[pos], sizeof(uint32_t) * tsize));
    HIP_TRY(s, hipMemcpy(s->d_dom_blob[pos], dom_blob, blob_len, hipMemcpyHostToDevice));
    HIP_TRY(s, hipMemcpy(s->d_dom_offs[pos], dom_offs,
                         sizeof(uint64_t) * (n_values + 1), hipMemcpyHostToDevice));
    HIP_TRY(s, hipMemcpy(s->d_dom_hashes[pos], hashes.data(),
                         sizeof(uint64_t) * tsize, hipMemcpyHostToDevice));
    HIP_TRY(s, hipMemcpy(s->d_dom_gids[pos], gids.data(),
                         sizeof(uint32_t) * tsize, hipMemcpyHostToDevice));
    s->dom_table_size[pos] = tsize;
    s->dom_n[pos] = n_values;
    return BYDB_OK;
}

// Group rows by up to 3 dictionary tags (composite key, computeKey
// semantics): gid = g0 + n0*g1 + n0*n1*g2; per-slot domains concatenated
// in blobs/offs (offs holds, per slot, n_i+1 cumulative offsets).
extern "C" int bydb_agg_configure_by_tags(bydb_session *s, int field_vtype,
                                          uint32_t func_mask, const int *slots,
                                          int n_slots,
                                          const uint8_t *const *dom_blobs,
                                          const uint64_t *const *dom_offs,
                                          const uint32_t *n_values, int mode) {
    if (n_slots < 1 || n_slots > 3) { s->err = "n_slots 1..3"; return BYDB_ERR_BAD_ARG; }
    uint64_t total = 1;
    for (int i = 0; i < n_slots; i++) {
        if (slots[i] < 0 || slots[i] > 2 || n_values[i] < 1) {
            s->err = "bad slot/domain";
            return BYDB_ERR_BAD_ARG;
        }
        total *= n_values[i];
    }
    if (total > 65000) { s->err = "composite group space too large"; return BYDB_ERR_BAD_ARG; }
    int rc = bydb_agg_configure(s, field_vtype, func_mask, (uint32_t)total, mode);
    if (rc != BYDB_OK) return rc;
    s->n_gslots = n_slots;
    s->groups_built = false;
    int64_t mul = 1;
    for (int i = 0; i < n_slots; i++) {
        s->gslots[i] = slots[i];
        s->gmul[i] = mul;
        mul *= n_values[i];
        rc = load_domain(s, i, dom_blobs[i], dom_offs[i], n_values[i]);
        if (rc != BYDB_OK) return rc;
    }
    return BYDB_OK;
}

extern "C" int bydb_agg_configure_by_tag(bydb_session *s, int field_vtype,
                                         uint32_t func_mask, int tag_slot,
                                         const uint8_t *dom_blob,
                                         const uint64_t *dom_offs,
                                         uint32_t n_values, int mode) {
    const int slots[1] = {tag_slot};
    const uint8_t *blobs[1] = {dom_blob};
    const uint64_t *offs[1] = {dom_offs};
    const uint32_t nv[1] = {n_values};
    return bydb_agg_configure_by_tags(s, field_vtype, func_mask, slots, 1,
                                      blobs, offs, nv, mode);
}

extern "C" int bydb_set_partials_buffer(bydb_session *s, void *dev_ptr,
                                        uint64_t len) {
    if (dev_ptr == nullptr) {
        s->d_acc = s->d_partials;
        return BYDB_OK;
    }
    if (len < sizeof(bydb_partial) * s->n_groups) {
        s->err = "partials buffer too small";
        return BYDB_ERR_BAD_ARG;
    }
    s->d_acc = (bydb_partial *)dev_ptr;
    return bydb_reset(s);
}

extern "C" int bydb_reset(bydb_session *s) {
    HIP_TRY(s, hipSetDevice(s->device));
    if (!s->d_acc) { s->err = "configure first"; return BYDB_ERR_STATE; }
    int threads = 256;
    int blocks = (int)((s->n_groups + threads - 1) / threads);
    hipLaunchKernelGGL(k_reset_partials, dim3(blocks), dim3(threads), 0,
                       s->stream, s->d_acc, (int64_t)s->n_groups);
    HIP_TRY(s, hipGetLastError());
    if (s->d_first_seen)
        HIP_TRY(s, hipMemsetAsync(s->d_first_seen, 0xFF,
                                  sizeof(uint64_t) * s->n_groups, s->stream));
    HIP_TRY(s, hipMemsetAsync(s->d_err, 0, sizeof(DevErr), s->stream));
    s->consumed = false;
    return BYDB_OK;
}

// PredBlock / flag-byte / walk-census buffers for the resolve prepasses
static int ensure_pred_buffers(bydb_session *s) {
    if (s->preds_cap < s->n_blocks * 3) {
        if (s->d_preds) (void)hipFree(s->d_preds);
        HIP_TRY(s, hipMalloc(&s->d_preds,
                             sizeof(PredBlock) * (size_t)s->n_blocks * 3));
        s->preds_cap = s->n_blocks * 3;
    }
    if (s->pred_flags_cap < s->n_blocks) {
        if (s->d_pred_flags) (void)hipFree(s->d_pred_flags);
        HIP_TRY(s, hipMalloc(&s->d_pred_flags, (size_t)s->n_blocks));
        s->pred_flags_cap = s->n_blocks;
    }
    if (!s->d_walk_count)
        HIP_TRY(s, hipMalloc(&s->d_walk_count, sizeof(uint32_t)));
    HIP_TRY(s, hipMemsetAsync(s->d_walk_count, 0, sizeof(uint32_t),
                              s->stream));
    return BYDB_OK;
}

// ---- nibble-packed dense field streams: planner, build ----
// (kernel: k_pack_fields; fold: dense_region_packed)

// The slot planner.  Every candidate gets ceil((count-1)/2) bytes rounded
// up to a 128-byte multiple, slots laid end to end from offset 0 in block
// order: 128-byte aligned, pairwise disjoint, no memory line shared.
static uint64_t plan_pack(const bydb_block_desc *blocks, int64_t n,
                          uint64_t *slot_off, uint32_t *slot_len,
                          uint64_t *n_cand) {
    uint64_t at = 0, cand = 0;
    for (int64_t i = 0; i < n; i++) {
        const bool c = pack_candidate(&blocks[i]);
        const uint32_t len = c ? pack_slot_bytes(blocks[i].count) : 0;
        if (slot_off) slot_off[i] = c ? at : 0;
        if (slot_len) slot_len[i] = len;
        at += len;
        cand += c;
    }
    if (n_cand) *n_cand = cand;
    return at;
}

extern "C" int bydb_field_pack_plan(const bydb_block_desc *blocks,
                                    int64_t n_blocks, uint64_t *slot_off,
                                    uint32_t *slot_len,
                                    uint64_t *arena_bytes) {
    if (n_blocks < 0 || (n_blocks > 0 && blocks == nullptr) ||
        (n_blocks > 0 && (slot_off == nullptr || slot_len == nullptr)) ||
        arena_bytes == nullptr)
        return BYDB_ERR_BAD_ARG;
    *arena_bytes = plan_pack(blocks, n_blocks, slot_off, slot_len, nullptr);
    return BYDB_OK;
}

extern "C" int bydb_set_field_pack(bydb_session *s, int mode) {
    if (mode != BYDB_PACK_AUTO && mode != BYDB_PACK_OFF &&
        mode != BYDB_PACK_ON) {
        s->err = "unknown field pack mode";
        return BYDB_ERR_BAD_ARG;
    }
    // a change of mode drops the copy: what the new mode does not read must
    // not stay resident, and what it reads is built again by its first
    // consume (also after a build that fell back to the byte streams)
    if (mode != s->field_pack) {
        HIP_TRY(s, hipSetDevice(s->device));
        pack_free(s);
        s->pack_built = false;
    }
    s->field_pack = mode;
    return BYDB_OK;
}

// The closed-form scan would read packed data under the session's current
// mode and stream-load policy.
static bool pack_wanted(const bydb_session *s) {
    return s->field_pack == BYDB_PACK_ON ||
           (s->field_pack == BYDB_PACK_AUTO &&
            bydb_stream_policy_pick(s->stream_policy, s->payload_len) ==
                BYDB_STREAM_STREAMING);
}

extern "C" int bydb_field_pack_stats(bydb_session *s, uint64_t out[4]) {
    const bool live = s->pack_built && pack_wanted(s);
    for (int i = 0; i < 4; i++) out[i] = live ? s->pack_stats[i] : 0;
    return BYDB_OK;
}

// Once per resident part, on the first closed-form streaming consume with
// packing on: read the descriptors back, plan the slots, pack on the
// device, and read the two counters back — the build's single host wait.
// A part without candidates allocates nothing.  An allocation failure
// leaves the part unpacked: silently under AUTO, as BYDB_ERR_OOM under ON.
static int pack_build(bydb_session *s) {
    if (s->pack_built) return BYDB_OK;
    pack_free(s);
    const int64_t nb = s->n_blocks;
    // slot offsets are table entries in 128-byte units
    if (nb < 1 || nb > (int64_t)UINT32_MAX) {
        s->pack_built = true;
        return BYDB_OK;
    }
    std::vector<bydb_block_desc> hb((size_t)nb);
    HIP_TRY(s, hipMemcpy(hb.data(), s->d_blocks,
                         sizeof(bydb_block_desc) * (size_t)nb,
                         hipMemcpyDeviceToHost));
    std::vector<uint64_t> off((size_t)nb);
    std::vector<uint32_t> len((size_t)nb);
    uint64_t n_cand = 0;
    const uint64_t arena = plan_pack(hb.data(), nb, off.data(), len.data(),
                                     &n_cand);
    s->pack_stats[0] = n_cand;
    const uint64_t table_bytes =
        ((uint64_t)nb * sizeof(uint32_t) + PACK_SLOT_ALIGN - 1) &
        ~(uint64_t)(PACK_SLOT_ALIGN - 1);
    const uint64_t bytes = table_bytes + arena;
    if (n_cand == 0 || bytes / PACK_SLOT_ALIGN > (uint64_t)UINT32_MAX) {
        s->pack_built = true;
        return BYDB_OK;
    }
    if (hipMalloc(&s->d_pack, bytes) != hipSuccess) {
        (void)hipGetLastError();
        s->d_pack = nullptr;
        s->pack_built = true;   // unpacked until the part or the mode changes
        if (s->field_pack != BYDB_PACK_ON) return BYDB_OK;
        char buf[160];
        snprintf(buf, sizeof buf,
                 "field pack: cannot allocate %llu bytes for the packed "
                 "arena; the part stays unpacked",
                 (unsigned long long)bytes);
        s->err = buf;
        return BYDB_ERR_OOM;
    }
    if (!s->d_pack_ctr)
        HIP_TRY(s, hipMalloc(&s->d_pack_ctr, 2 * sizeof(unsigned long long)));
    std::vector<uint32_t> table((size_t)(table_bytes / sizeof(uint32_t)), 0);
    for (int64_t i = 0; i < nb; i++)
        if (len[(size_t)i])
            table[(size_t)i] =
                (uint32_t)((table_bytes + off[(size_t)i]) / PACK_SLOT_ALIGN);
    HIP_TRY(s, hipMemcpyAsync(s->d_pack, table.data(), table_bytes,
                              hipMemcpyHostToDevice, s->stream));
    HIP_TRY(s, hipMemsetAsync(s->d_pack_ctr, 0, 2 * sizeof(unsigned long long),
                              s->stream));
    const int grid =
        (int)(nb < BLOCK_KERNEL_MAX_WGS ? nb : BLOCK_KERNEL_MAX_WGS);
    hipLaunchKernelGGL(k_pack_fields, dim3(grid), dim3(WAVE), 0, s->stream,
                       s->d_payload, s->d_blocks, nb, s->d_pack, s->d_pack_ctr);
    HIP_TRY(s, hipGetLastError());
    unsigned long long h_ctr[2] = {0, 0};
    HIP_TRY(s, hipMemcpyAsync(h_ctr, s->d_pack_ctr, sizeof h_ctr,
                              hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(s, hipStreamSynchronize(s->stream));
    s->pack_stats[1] = h_ctr[PACK_CTR_BLOCKS];
    s->pack_stats[2] = h_ctr[PACK_CTR_BYTES];
    s->pack_stats[3] = arena;
    if (h_ctr[PACK_CTR_BLOCKS] == 0) {
        // nothing qualified: the scan gets no table
        (void)hipFree(s->d_pack);
        s->d_pack = nullptr;
        s->pack_stats[3] = 0;
    }
    s->pack_built = true;
    return BYDB_OK;
}

// The scan launch shared by every consume entry point: group resolve (once
// per part), kernel selection, light + heavy pass.
static int launch_scan(bydb_session *s, int64_t min_ts, int64_t max_ts,
                       PredBlock *preds, int n_preds) {
    int flags = 0;
    if (s->func_mask & ((1u << BYDB_AGG_MIN) | (1u << BYDB_AGG_MAX)))
        flags |= KF_NEED_VALUES;
    if (s->field_vtype == BYDB_VT_FLOAT64)
        flags |= KF_FLOAT | ((int)(uint16_t)s->float_exp << 16);
    const int threads = 256;                       // 4 waves per workgroup
    GroupBlock *groups = nullptr;
    if (s->n_gslots > 0) {
        if (s->groups_cap < s->n_blocks) {
            if (s->d_groups) (void)hipFree(s->d_groups);
            if (s->d_gmap) (void)hipFree(s->d_gmap);
            HIP_TRY(s, hipMalloc(&s->d_groups,
                                 sizeof(GroupBlock) * 3 * (size_t)s->n_blocks));
            HIP_TRY(s, hipMalloc(&s->d_gmap,
                                 sizeof(uint16_t) * 256 * 3 * (size_t)s->n_blocks));
            s->groups_cap = s->n_blocks;
            s->groups_built = false;
        }
        if (!s->groups_built) {
            int rthreads = 256;
            int rblocks = (int)((s->n_blocks + rthreads - 1) / rthreads);
            // plain (>256-distinct) tag columns on grouped slots resolve
            // into (gid,count) run pairs; size the arena by the count of
            // normalized plain streams (an upper bound)
            if (s->n_plain_host > 0) {
                uint64_t want = s->n_plain_host;
                uint64_t bytes =
                    want * GRUN_ENTRIES_PER_STREAM * sizeof(uint16_t);
                if (bytes > (4ull << 30)) {
                    s->err = "plain-tag group-by run arena exceeds 4 GiB";
                    return BYDB_ERR_OOM;
                }
                if (want > s->gruns_cap_streams) {
                    if (s->d_gruns) (void)hipFree(s->d_gruns);
                    HIP_TRY(s, hipMalloc(&s->d_gruns, bytes));
                    s->gruns_cap_streams = want;
                }
                if (!s->d_grun_ctr)
                    HIP_TRY(s, hipMalloc(&s->d_grun_ctr, sizeof(uint32_t)));
                HIP_TRY(s, hipMemsetAsync(s->d_grun_ctr, 0, sizeof(uint32_t),
                                          s->stream));
            }
            for (int i = 0; i < s->n_gslots; i++) {
                GroupDomain dom;
                dom.blob = s->d_dom_blob[i];
                dom.offs = s->d_dom_offs[i];
                dom.hashes = s->d_dom_hashes[i];
                dom.gids = s->d_dom_gids[i];
                dom.table_size = s->dom_table_size[i];
                dom.n = s->dom_n[i];
                hipLaunchKernelGGL(
                    k_resolve_groups, dim3(rblocks), dim3(rthreads), 0,
                    s->stream, s->d_payload, s->d_sidecar, s->d_blocks,
                    s->n_blocks, s->gslots[i], dom,
                    s->d_groups + (int64_t)i * s->n_blocks,
                    s->d_gmap, (uint32_t)((int64_t)i * 256 * s->n_blocks));
                HIP_TRY(s, hipGetLastError());
                if (s->n_plain_host > 0) {
                    int pgrid = (int)(s->n_blocks < BLOCK_KERNEL_MAX_WGS
                                          ? s->n_blocks
                                          : BLOCK_KERNEL_MAX_WGS);
                    hipLaunchKernelGGL(
                        k_resolve_plain_groups, dim3(pgrid), dim3(WAVE), 0,
                        s->stream, s->d_payload, s->d_sidecar, s->d_blocks,
                        s->n_blocks, s->gslots[i], dom,
                        s->d_groups + (int64_t)i * s->n_blocks, s->d_gruns,
                        s->gruns_cap_streams, s->d_grun_ctr);
                    HIP_TRY(s, hipGetLastError());
                }
            }
            s->groups_built = true;
        }
        groups = s->d_groups;
    }
    int64_t wgs = (s->n_blocks + 3) / 4;            // one wave per block
    int grid = (int)(wgs < SCAN_MAX_WGS ? wgs : SCAN_MAX_WGS);  // stride beyond
    if (grid < 1) grid = 1;
    const bool en_values = (flags & KF_NEED_VALUES) != 0;
    const bool en_preds = n_preds > 0;
    const bool en_groups = groups != nullptr;
    // the closed-form scan of a part too large for the last-level cache
    // (or a forced policy) reads its dense streams past the caches, and
    // the nibble-packed copy where a block has one (BYDB_PACK_ON takes the
    // streaming kernels for any size: only they read packed data).  The
    // copy is built here, ahead of ev_start, so the timing brackets the
    // scan only.
    const bool streaming =
        !en_values && !en_preds && !en_groups &&
        (s->field_pack == BYDB_PACK_ON ||
         bydb_stream_policy_pick(s->stream_policy, s->payload_len) ==
             BYDB_STREAM_STREAMING);
    const uint8_t *pack = nullptr;
    if (streaming && pack_wanted(s)) {
        int rc = pack_build(s);
        if (rc != BYDB_OK) return rc;
        pack = s->d_pack;
    }
    HIP_TRY(s, hipEventRecord(s->ev_start, s->stream));
    using ScanFn = decltype(&k_scan_agg_t<false, false, false, false, false>);
    ScanFn kfn, kfn_walk = nullptr;
    // the clamp-free instantiations run when the query range covers the
    // whole resident part (the common analytic scan; per-block FindRange
    // is then an identity)
    const bool en_clamp = !(s->n_blocks > 0 && min_ts <= s->part_ts_min &&
                            max_ts >= s->part_ts_max);
#define BYDB_KSEL(C)                                                         \
    if (en_values) {                                                         \
        if (en_preds) {                                                      \
            kfn = en_groups ? k_scan_agg_t<true, true, true, false, C>       \
                            : k_scan_agg_t<true, true, false, false, C>;     \
            kfn_walk = en_groups ? k_scan_agg_t<true, true, true, true, C>   \
                                 : k_scan_agg_t<true, true, false, true, C>; \
        } else {                                                             \
            kfn = en_groups ? k_scan_agg_t<true, false, true, false, C>      \
                            : k_scan_agg_t<true, false, false, false, C>;    \
        }                                                                    \
    } else {                                                                 \
        if (en_preds) {                                                      \
            kfn = en_groups ? k_scan_agg_t<false, true, true, false, C>      \
                            : k_scan_agg_t<false, true, false, false, C>;    \
            kfn_walk = en_groups ? k_scan_agg_t<false, true, true, true, C>  \
                                 : k_scan_agg_t<false, true, false, true, C>;\
        } else {                                                             \
            kfn = en_groups ? k_scan_agg_t<false, false, true, false, C>     \
                            : k_scan_agg_t<false, false, false, false, C>;   \
        }                                                                    \
    }
    if (en_clamp) {
        BYDB_KSEL(true)
    } else {
        BYDB_KSEL(false)
    }
#undef BYDB_KSEL
    if (streaming)
        kfn = en_clamp
                  ? k_scan_agg_t<false, false, false, false, true, true>
                  : k_scan_agg_t<false, false, false, false, false, true>;
    auto launch = [&](ScanFn fn, int pass_flags, const uint32_t *walk_count) {
        hipLaunchKernelGGL(fn, dim3(grid), dim3(threads), 0, s->stream,
                           s->d_payload, s->d_sidecar, s->d_blocks,
                           s->n_blocks, min_ts, max_ts, pass_flags, preds,
                           n_preds, s->d_pred_bm, s->d_pred_flags,
                           groups, s->d_gmap, s->d_gruns, s->n_gslots,
                           s->gmul[0], s->gmul[1], s->gmul[2],
                           (int64_t)s->n_groups, s->d_acc, s->d_err,
                           walk_count, s->d_first_seen, pack);
        return hipGetLastError();
    };
    // light pass: every block whose predicate verdict is uniform (no
    // walker state, no scratch spills in the scan loop)
    HIP_TRY(s, launch(kfn, flags, nullptr));
    // heavy pass: only the PF_WALK blocks (row-varying predicates).  When
    // none exist this is a flag-byte sweep (~tens of us)
    if (kfn_walk != nullptr)
        HIP_TRY(s, launch(kfn_walk, flags | KF_WALK_ONLY, s->d_walk_count));
    HIP_TRY(s, hipEventRecord(s->ev_stop, s->stream));
    s->consumed = true;
    return BYDB_OK;
}

// ---- cross-part version dedup: planner, build, per-consume apply ----
// (header: "cross-part version dedup"; kernels: k_dedup_decode / _mark /
// _apply)

// The overlap planner.  Block indices sorted by (series_id, ts_min); inside
// one series a block's peers among the later ones are exactly those whose
// ts_min does not exceed its ts_max, so the sweep stops at the first that
// does.  Output: symmetric CSR, each list ascending by block index.
static void plan_peers(const bydb_block_desc *blocks, int64_t n,
                       std::vector<uint64_t> &offs,
                       std::vector<uint32_t> &peers) {
    std::vector<uint32_t> ord((size_t)n);
    for (int64_t i = 0; i < n; i++) ord[(size_t)i] = (uint32_t)i;
    std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) {
        if (blocks[a].series_id != blocks[b].series_id)
            return blocks[a].series_id < blocks[b].series_id;
        if (blocks[a].ts_min != blocks[b].ts_min)
            return blocks[a].ts_min < blocks[b].ts_min;
        return a < b;
    });
    offs.assign((size_t)n + 1, 0);
    for (int pass = 0; pass < 2; pass++) {
        std::vector<uint64_t> fill;
        if (pass == 1) {
            for (int64_t i = 0; i < n; i++) offs[(size_t)i + 1] += offs[(size_t)i];
            peers.assign((size_t)offs[(size_t)n], 0);
            fill.assign(offs.begin(), offs.end() - 1);
        }
        for (int64_t i = 0; i < n; i++) {
            const bydb_block_desc &a = blocks[ord[(size_t)i]];
            for (int64_t j = i + 1; j < n; j++) {
                const bydb_block_desc &b = blocks[ord[(size_t)j]];
                if (b.series_id != a.series_id || b.ts_min > a.ts_max) break;
                if (pass == 0) {
                    offs[(size_t)ord[(size_t)i] + 1]++;
                    offs[(size_t)ord[(size_t)j] + 1]++;
                } else {
                    peers[(size_t)fill[ord[(size_t)i]]++] = ord[(size_t)j];
                    peers[(size_t)fill[ord[(size_t)j]]++] = ord[(size_t)i];
                }
            }
        }
    }
    for (int64_t i = 0; i < n; i++)
        std::sort(peers.begin() + (ptrdiff_t)offs[(size_t)i],
                  peers.begin() + (ptrdiff_t)offs[(size_t)i + 1]);
}

extern "C" int bydb_row_dedup_peers(const bydb_block_desc *blocks,
                                    int64_t n_blocks, uint64_t *peer_offs,
                                    uint32_t *peers, uint64_t peers_cap,
                                    uint64_t *n_peers) {
    if (n_blocks < 0 || n_blocks > (int64_t)UINT32_MAX ||
        (n_blocks > 0 && blocks == nullptr) || peer_offs == nullptr ||
        n_peers == nullptr)
        return BYDB_ERR_BAD_ARG;
    std::vector<uint64_t> offs;
    std::vector<uint32_t> pl;
    plan_peers(blocks, n_blocks, offs, pl);
    *n_peers = pl.size();
    memcpy(peer_offs, offs.data(), sizeof(uint64_t) * offs.size());
    if (pl.size() > peers_cap || (!pl.empty() && peers == nullptr))
        return BYDB_ERR_OOM;
    if (!pl.empty()) memcpy(peers, pl.data(), sizeof(uint32_t) * pl.size());
    return BYDB_OK;
}

extern "C" int bydb_set_row_dedup(bydb_session *s, int on) {
    if (on != 0 && on != 1) {
        s->err = "row dedup must be 0 or 1";
        return BYDB_ERR_BAD_ARG;
    }
    s->row_dedup = on;
    return BYDB_OK;
}

extern "C" int bydb_row_dedup_stats(bydb_session *s, uint64_t out[4]) {
    const bool live = s->row_dedup && s->dedup_built;
    for (int i = 0; i < 4; i++) out[i] = live ? s->dedup_stats[i] : 0;
    return BYDB_OK;
}

// Device allocation of the dedup build: a failure is BYDB_ERR_OOM with the
// size in the message, and turns dedup off so the session stays usable.
template <typename T>
static int dedup_alloc(bydb_session *s, T **p, uint64_t count,
                       const char *what) {
    const uint64_t bytes = (count ? count : 1) * sizeof(T);
    if (hipMalloc(p, bytes) != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        char buf[160];
        snprintf(buf, sizeof buf,
                 "row dedup: cannot allocate %llu bytes for the %s; "
                 "row dedup is now off",
                 (unsigned long long)bytes, what);
        s->err = buf;
        dedup_free(s);
        s->row_dedup = 0;
        return BYDB_ERR_OOM;
    }
    return BYDB_OK;
}

// Once per resident part, on the first consume with dedup on: read the
// descriptors back, plan the peers, decode and mark on the device, and
// read the four counters back — the build's single host wait.  A part
// without overlapping blocks allocates nothing.
static int dedup_build(bydb_session *s) {
    if (!s->row_dedup || s->dedup_built) return BYDB_OK;
    dedup_free(s);
    for (int i = 0; i < 4; i++) s->dedup_stats[i] = 0;
    s->dd_n_inv = s->dd_n_partial = s->dd_n_full = 0;
    const int64_t nb = s->n_blocks;
    std::vector<bydb_block_desc> hb((size_t)nb);
    HIP_TRY(s, hipMemcpy(hb.data(), s->d_blocks,
                         sizeof(bydb_block_desc) * (size_t)nb,
                         hipMemcpyDeviceToHost));
    std::vector<uint64_t> offs;
    std::vector<uint32_t> pl;
    plan_peers(hb.data(), nb, offs, pl);
    if (pl.empty()) {
        s->dedup_built = true;
        return BYDB_OK;
    }
    // involved blocks, their arena rows, and the CSR over involved indices
    std::vector<uint32_t> inv_of((size_t)nb, 0);
    std::vector<DedupInfo> infos;
    std::vector<uint64_t> ioffs(1, 0);
    uint64_t arena_rows = 0;
    for (int64_t bi = 0; bi < nb; bi++) {
        if (offs[(size_t)bi] == offs[(size_t)bi + 1]) continue;
        const bydb_block_desc &bd = hb[(size_t)bi];
        const uint8_t tenc = bd.ts_enc_with_version;
        const uint8_t tc = tenc >= BYDB_ENC_CONST_WV ? tenc - 4 : tenc;
        if (tc < BYDB_ENC_CONST || tc > BYDB_ENC_DELTA_OF_DELTA ||
            bd.version_enc < BYDB_ENC_CONST ||
            bd.version_enc > BYDB_ENC_DELTA_OF_DELTA || bd.count < 1 ||
            bd.count > PLAIN_BM_WORDS * 64) {
            char buf[128];
            snprintf(buf, sizeof buf,
                     "row dedup: block %lld has an unsupported timestamp / "
                     "version encoding or row count", (long long)bi);
            s->err = buf;
            return BYDB_ERR_BAD_DATA;
        }
        DedupInfo in;
        memset(&in, 0, sizeof in);
        in.block = (uint32_t)bi;
        in.count = bd.count;
        in.ts_min = bd.ts_min;
        in.ts_max = bd.ts_max;
        in.ver_first = bd.version_first;
        in.ts_kind = tc == BYDB_ENC_CONST ? DD_TS_CONST
                     : tc == BYDB_ENC_DELTA_CONST ? DD_TS_ARITH : DD_TS_ARENA;
        in.ts_arena = DD_NO_ARENA;
        in.ver_arena = DD_NO_ARENA;
        if (in.ts_kind == DD_TS_ARENA) {
            in.ts_arena = arena_rows;
            arena_rows += bd.count;
        }
        if (bd.version_enc != BYDB_ENC_CONST) {
            in.ver_arena = arena_rows;
            arena_rows += bd.count;
        }
        inv_of[(size_t)bi] = (uint32_t)infos.size();
        infos.push_back(in);
        ioffs.push_back(offs[(size_t)bi + 1]);
    }
    // ioffs holds each involved block's END in the block-indexed list; the
    // lists of uninvolved blocks are empty, so these are also the offsets
    // of the compacted list
    for (size_t k = 0; k < pl.size(); k++) pl[k] = inv_of[pl[k]];
    const int64_t n_inv = (int64_t)infos.size();
    int rc;
    if ((rc = dedup_alloc(s, &s->d_dd_infos, (uint64_t)n_inv, "block table")) ||
        (rc = dedup_alloc(s, &s->d_dd_peer_offs, (uint64_t)n_inv + 1,
                          "peer offsets")) ||
        (rc = dedup_alloc(s, &s->d_dd_peers, pl.size(), "peer list")) ||
        (rc = dedup_alloc(s, &s->d_dd_arena, arena_rows,
                          "timestamp / version arena")) ||
        (rc = dedup_alloc(s, &s->d_dd_surv,
                          (uint64_t)n_inv * PLAIN_BM_WORDS,
                          "survivor bitmaps")) ||
        (rc = dedup_alloc(s, &s->d_dd_plist, (uint64_t)n_inv, "block lists")) ||
        (rc = dedup_alloc(s, &s->d_dd_flist, (uint64_t)n_inv, "block lists")) ||
        (rc = dedup_alloc(s, &s->d_dd_ctr, 4, "counters")))
        return rc;
    HIP_TRY(s, hipMemcpyAsync(s->d_dd_infos, infos.data(),
                              sizeof(DedupInfo) * infos.size(),
                              hipMemcpyHostToDevice, s->stream));
    HIP_TRY(s, hipMemcpyAsync(s->d_dd_peer_offs, ioffs.data(),
                              sizeof(uint64_t) * ioffs.size(),
                              hipMemcpyHostToDevice, s->stream));
    HIP_TRY(s, hipMemcpyAsync(s->d_dd_peers, pl.data(),
                              sizeof(uint32_t) * pl.size(),
                              hipMemcpyHostToDevice, s->stream));
    HIP_TRY(s, hipMemsetAsync(s->d_dd_ctr, 0, 4 * sizeof(unsigned long long),
                              s->stream));
    const int grid =
        (int)(n_inv < BLOCK_KERNEL_MAX_WGS ? n_inv : BLOCK_KERNEL_MAX_WGS);
    hipLaunchKernelGGL(k_dedup_decode, dim3(grid), dim3(WAVE), 0, s->stream,
                       s->d_payload, s->payload_cap + 4096, s->d_blocks,
                       s->d_dd_infos, n_inv, s->d_dd_arena, s->d_err);
    HIP_TRY(s, hipGetLastError());
    hipLaunchKernelGGL(k_dedup_mark, dim3(grid), dim3(WAVE), 0, s->stream,
                       s->d_dd_infos, n_inv, s->d_dd_peer_offs, s->d_dd_peers,
                       s->d_dd_arena, s->d_dd_surv, s->d_dd_plist,
                       s->d_dd_flist, s->d_dd_ctr);
    HIP_TRY(s, hipGetLastError());
    unsigned long long h_ctr[4] = {0, 0, 0, 0};
    DevErr de;
    HIP_TRY(s, hipMemcpyAsync(h_ctr, s->d_dd_ctr, sizeof h_ctr,
                              hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(s, hipMemcpyAsync(&de, s->d_err, sizeof de, hipMemcpyDeviceToHost,
                              s->stream));
    HIP_TRY(s, hipStreamSynchronize(s->stream));
    s->dd_n_inv = n_inv;
    s->dd_n_partial = (int64_t)h_ctr[DD_CTR_PARTIAL];
    s->dd_n_full = (int64_t)h_ctr[DD_CTR_FULL];
    s->dedup_stats[0] = (uint64_t)n_inv;
    s->dedup_stats[1] = h_ctr[DD_CTR_PARTIAL];
    s->dedup_stats[2] = h_ctr[DD_CTR_FULL];
    s->dedup_stats[3] = h_ctr[DD_CTR_ROWS];
    // a device error (descending or unparseable stream) stays in d_err for
    // finalize to report; the build is then repeated by the next consume,
    // so a reset does not turn it into a silently unmerged scan
    s->dedup_built = de.code == DERR_NONE;
    return BYDB_OK;
}

// the part holds superseded rows and the session wants them dropped
static bool dedup_active(const bydb_session *s) {
    return s->row_dedup && s->dedup_built && s->dedup_stats[3] > 0;
}

// pred_bm words the merged bitmaps of this consume add to the demand
static uint64_t dedup_bm_words(const bydb_session *s) {
    return dedup_active(s) ? (uint64_t)s->dd_n_partial * PLAIN_BM_WORDS : 0;
}

// Grow the one pred_bm arena the scan receives to `words` (contents are
// not kept: every consume fills it again before the scan reads it).
static int ensure_pred_bm(bydb_session *s, uint64_t words) {
    if (words <= s->pred_bm_cap) return BYDB_OK;
    if (s->d_pred_bm) { (void)hipFree(s->d_pred_bm); s->d_pred_bm = nullptr; }
    s->pred_bm_cap = 0;
    HIP_TRY(s, hipMalloc(&s->d_pred_bm, words * sizeof(uint64_t)));
    s->pred_bm_cap = words;
    return BYDB_OK;
}

// ---- BatchTop over raw rows: the pipeline of one consume ----
// (header: "top-N data points by field value"; kernels: k_top_bounds,
// k_sel_*, k_top_row_keys, k_top_resolve*)

template <typename T>
static int top_alloc(bydb_session *s, T **p, uint64_t count) {
    if (*p) { (void)hipFree(*p); *p = nullptr; }
    HIP_TRY(s, hipMalloc(p, sizeof(T) * (size_t)(count ? count : 1)));
    return BYDB_OK;
}

// top_select(keys, valid, n, want) -> out[], count in st->n_out.  Nothing
// comes back to the host.
static int top_select(bydb_session *s, const uint64_t *keys,
                      const uint8_t *valid, uint64_t n, uint32_t want,
                      TopSelState *st, uint32_t *out) {
    const uint64_t chunks = (n + TOP_CHUNK - 1) / TOP_CHUNK;
    uint32_t *cnt_gt = s->d_top_cnt, *cnt_eq = s->d_top_cnt + s->top_cnt_cap;
    const int hgrid = (int)(chunks < 2048 ? chunks : 2048);
    HIP_TRY(s, hipMemsetAsync(st, 0, sizeof(TopSelState), s->stream));
    for (int pass = 0; pass < 8; pass++) {
        hipLaunchKernelGGL(k_sel_hist, dim3(hgrid), dim3(256), 0, s->stream,
                           keys, valid, n, st, pass);
        hipLaunchKernelGGL(k_sel_pick, dim3(1), dim3(256), 0, s->stream, st,
                           pass, want);
    }
    hipLaunchKernelGGL(k_sel_count, dim3((unsigned)chunks), dim3(256), 0,
                       s->stream, keys, valid, n, st, cnt_gt, cnt_eq);
    hipLaunchKernelGGL(k_sel_scan, dim3(1), dim3(1024), 0, s->stream, st,
                       cnt_gt, cnt_eq, (uint32_t)chunks);
    hipLaunchKernelGGL(k_sel_emit, dim3((unsigned)chunks), dim3(256), 0,
                       s->stream, keys, valid, n, st, cnt_gt, cnt_eq, out,
                       want);
    HIP_TRY(s, hipGetLastError());
    return BYDB_OK;
}

static int launch_top(bydb_session *s, int64_t min_ts, int64_t max_ts,
                      PredBlock *preds, int n_preds) {
    if (s->consumed) {
        s->err = "top session: one consume per epoch (finalize or reset first)";
        return BYDB_ERR_STATE;
    }
    int flags = KF_NEED_VALUES;
    if (s->field_vtype == BYDB_VT_FLOAT64) {
        if (s->float_exp == BYDB_FLOAT_RAW_EXP) {
            s->err = "top session: raw-float exponent is not supported";
            return BYDB_ERR_BAD_ARG;
        }
        flags |= KF_FLOAT | ((int)(uint16_t)s->float_exp << 16);
    }
    s->consumed = true;
    if (s->top_n == 0) return BYDB_OK;   // the reference's no-op
    const uint32_t N = (uint32_t)s->top_n;
    const int64_t nb = s->n_blocks;
    const uint64_t n_rows = (uint64_t)N * TOP_BLOCK_ROWS;
    int rc;
    if (s->top_blocks_cap < nb) {
        if ((rc = top_alloc(s, &s->d_top_bkeys, (uint64_t)nb)) ||
            (rc = top_alloc(s, &s->d_top_bvalid, (uint64_t)nb)))
            return rc;
        s->top_blocks_cap = nb;
    }
    if (s->top_grid_cap != (int64_t)N) {
        s->top_grid_cap = 0;
        if ((rc = top_alloc(s, &s->d_top_grid, n_rows)) ||
            (rc = top_alloc(s, &s->d_top_rvalid, n_rows)) ||
            (rc = top_alloc(s, &s->d_top_chosen, (uint64_t)N)) ||
            (rc = top_alloc(s, &s->d_top_winners, (uint64_t)N)) ||
            (rc = top_alloc(s, &s->d_top_range, (uint64_t)N)) ||
            (rc = top_alloc(s, &s->d_top_recs, (uint64_t)N)))
            return rc;
        s->top_grid_cap = (int64_t)N;
    }
    const uint64_t most = (uint64_t)nb > n_rows ? (uint64_t)nb : n_rows;
    const uint64_t chunks = (most + TOP_CHUNK - 1) / TOP_CHUNK;
    if (s->top_cnt_cap < chunks) {
        if ((rc = top_alloc(s, &s->d_top_cnt, 2 * chunks))) return rc;
        s->top_cnt_cap = chunks;
    }
    if (!s->d_top_st && (rc = top_alloc(s, &s->d_top_st, 2))) return rc;
    const uint64_t limit = s->payload_cap + 4096;
    HIP_TRY(s, hipEventRecord(s->ev_start, s->stream));
    HIP_TRY(s, hipMemsetAsync(s->d_top_bvalid, 0, (size_t)nb, s->stream));
    HIP_TRY(s, hipMemsetAsync(s->d_top_rvalid, 0, (size_t)n_rows, s->stream));
    int64_t wgs = (nb + 3) / 4;                    // one wave per block
    int grid = (int)(wgs < SCAN_MAX_WGS ? wgs : SCAN_MAX_WGS);  // stride beyond
    hipLaunchKernelGGL(k_top_bounds, dim3(grid), dim3(256), 0, s->stream,
                       s->d_payload, s->d_sidecar, s->d_blocks, nb, min_ts,
                       max_ts, flags, s->top_asc, preds, n_preds, s->d_pred_bm,
                       s->d_pred_flags, s->d_top_bkeys, s->d_top_bvalid,
                       s->d_err);
    HIP_TRY(s, hipGetLastError());
    if ((rc = top_select(s, s->d_top_bkeys, s->d_top_bvalid, (uint64_t)nb, N,
                         &s->d_top_st[0], s->d_top_chosen)))
        return rc;
    hipLaunchKernelGGL(k_top_row_range, dim3((N + 3) / 4), dim3(256), 0,
                       s->stream, s->d_payload, s->d_blocks, nb, min_ts,
                       max_ts, flags, &s->d_top_st[0], s->d_top_chosen,
                       s->d_top_range, N, s->d_err);
    hipLaunchKernelGGL(k_top_row_keys, dim3(N), dim3(WAVE), 0, s->stream,
                       s->d_payload, s->d_sidecar, limit, s->d_blocks, nb,
                       flags, s->top_asc, preds, n_preds, s->d_pred_bm,
                       s->d_pred_flags, &s->d_top_st[0], s->d_top_chosen,
                       s->d_top_range, s->d_top_grid, s->d_top_rvalid,
                       s->d_err);
    HIP_TRY(s, hipGetLastError());
    if ((rc = top_select(s, s->d_top_grid, s->d_top_rvalid, n_rows, N,
                         &s->d_top_st[1], s->d_top_winners)))
        return rc;
    hipLaunchKernelGGL(k_top_resolve_keys, dim3((N + 255) / 256), dim3(256), 0,
                       s->stream, s->d_blocks, nb, flags, s->top_asc,
                       &s->d_top_st[1], s->d_top_chosen, s->d_top_winners,
                       s->d_top_grid, s->d_top_recs, N);
    hipLaunchKernelGGL(k_top_resolve, dim3(N), dim3(WAVE), 0, s->stream,
                       s->d_payload, limit, s->d_blocks, nb, &s->d_top_st[1],
                       s->d_top_grid, s->d_top_recs, s->d_err);
    HIP_TRY(s, hipGetLastError());
    HIP_TRY(s, hipEventRecord(s->ev_stop, s->stream));
    return BYDB_OK;
}

// ---- Scan -> Limit over raw rows: the pipeline of one consume ----
// (header: "time-ordered rows with offset and limit"; kernels:
// k_rows_bounds*, k_sel2_*, k_rows_row_keys, k_rows_resolve*)

// rows_select(hi, lo, valid, n, want) -> out[], count in st->n_out.
static int rows_select(bydb_session *s, const uint64_t *hi, const uint64_t *lo,
                       const uint32_t *lo_map, const uint8_t *valid,
                       uint64_t n, uint32_t want, TopSelState *st_hi,
                       TopSelState *st, uint32_t *out) {
    const uint64_t chunks = (n + TOP_CHUNK - 1) / TOP_CHUNK;
    uint32_t *cnt_gt = s->d_top_cnt, *cnt_eq = s->d_top_cnt + s->top_cnt_cap;
    const int hgrid = (int)(chunks < 2048 ? chunks : 2048);
    HIP_TRY(s, hipMemsetAsync(st_hi, 0, sizeof(TopSelState), s->stream));
    HIP_TRY(s, hipMemsetAsync(st, 0, sizeof(TopSelState), s->stream));
    for (int pass = 0; pass < 8; pass++) {
        hipLaunchKernelGGL(k_sel_hist, dim3(hgrid), dim3(256), 0, s->stream,
                           hi, valid, n, st_hi, pass);
        hipLaunchKernelGGL(k_sel_pick, dim3(1), dim3(256), 0, s->stream, st_hi,
                           pass, want);
    }
    for (int pass = 0; pass < 8; pass++) {
        hipLaunchKernelGGL(k_sel2_hist, dim3(hgrid), dim3(256), 0, s->stream,
                           hi, lo, lo_map, valid, n, st_hi, st, pass);
        hipLaunchKernelGGL(k_sel2_pick, dim3(1), dim3(256), 0, s->stream,
                           st_hi, st, pass);
    }
    hipLaunchKernelGGL(k_sel2_count, dim3((unsigned)chunks), dim3(256), 0,
                       s->stream, hi, lo, lo_map, valid, n, st_hi, st, cnt_gt,
                       cnt_eq);
    hipLaunchKernelGGL(k_sel_scan, dim3(1), dim3(1024), 0, s->stream, st,
                       cnt_gt, cnt_eq, (uint32_t)chunks);
    hipLaunchKernelGGL(k_sel2_emit, dim3((unsigned)chunks), dim3(256), 0,
                       s->stream, hi, lo, lo_map, valid, n, st_hi, st, cnt_gt,
                       cnt_eq, out, want);
    HIP_TRY(s, hipGetLastError());
    return BYDB_OK;
}

// the fewest grid slots a row scan keeps: k_rows_bounds_ts decodes one
// deferred block per slot at a time, whatever N is
#define ROWS_MIN_SLOTS 256

static int launch_rows(bydb_session *s, int64_t min_ts, int64_t max_ts,
                       PredBlock *preds, int n_preds) {
    if (s->consumed) {
        s->err = "row scan: one consume per epoch (finalize or reset first)";
        return BYDB_ERR_STATE;
    }
    int flags = KF_NEED_VALUES;
    if (s->field_vtype == BYDB_VT_FLOAT64) {
        if (s->float_exp == BYDB_FLOAT_RAW_EXP) {
            s->err = "row scan: raw-float exponent is not supported";
            return BYDB_ERR_BAD_ARG;
        }
        flags |= KF_FLOAT | ((int)(uint16_t)s->float_exp << 16);
    }
    s->consumed = true;
    if (s->rows_limit == 0) return BYDB_OK;   // BatchLimit with nothing to keep
    const uint32_t N = (uint32_t)(s->rows_offset + s->rows_limit);
    const uint32_t slots = N < ROWS_MIN_SLOTS ? ROWS_MIN_SLOTS : N;
    const int64_t nb = s->n_blocks;
    const uint64_t n_rows = (uint64_t)N * TOP_BLOCK_ROWS;
    const uint64_t n_slot_rows = (uint64_t)slots * TOP_BLOCK_ROWS;
    int rc;
    if (s->top_blocks_cap < nb) {
        if ((rc = top_alloc(s, &s->d_top_bkeys, (uint64_t)nb)) ||
            (rc = top_alloc(s, &s->d_top_bvalid, (uint64_t)nb)))
            return rc;
        s->top_blocks_cap = nb;
    }
    if (s->rows_blocks_cap < nb) {
        if ((rc = top_alloc(s, &s->d_rows_blo, (uint64_t)nb))) return rc;
        s->rows_blocks_cap = nb;
    }
    if (s->top_grid_cap != (int64_t)slots) {
        s->top_grid_cap = 0;
        if ((rc = top_alloc(s, &s->d_top_grid, n_slot_rows)) ||
            (rc = top_alloc(s, &s->d_top_rvalid, n_slot_rows)) ||
            (rc = top_alloc(s, &s->d_top_chosen, (uint64_t)slots)) ||
            (rc = top_alloc(s, &s->d_top_winners, (uint64_t)slots)) ||
            (rc = top_alloc(s, &s->d_top_range, (uint64_t)slots)) ||
            (rc = top_alloc(s, &s->d_top_recs, (uint64_t)slots)))
            return rc;
        s->top_grid_cap = (int64_t)slots;
    }
    const uint64_t most = (uint64_t)nb > n_rows ? (uint64_t)nb : n_rows;
    const uint64_t chunks = (most + TOP_CHUNK - 1) / TOP_CHUNK;
    if (s->top_cnt_cap < chunks) {
        if ((rc = top_alloc(s, &s->d_top_cnt, 2 * chunks))) return rc;
        s->top_cnt_cap = chunks;
    }
    if (!s->d_rows_st && (rc = top_alloc(s, &s->d_rows_st, 4))) return rc;
    TopSelState *st_blocks = &s->d_rows_st[1], *st_rows = &s->d_rows_st[3];
    const uint64_t limit = s->payload_cap + 4096;
    HIP_TRY(s, hipEventRecord(s->ev_start, s->stream));
    HIP_TRY(s, hipMemsetAsync(s->d_top_bvalid, 0, (size_t)nb, s->stream));
    HIP_TRY(s, hipMemsetAsync(s->d_top_rvalid, 0, (size_t)n_rows, s->stream));
    int64_t wgs = (nb + 3) / 4;                    // one wave per block
    int grid = (int)(wgs < SCAN_MAX_WGS ? wgs : SCAN_MAX_WGS);  // stride beyond
    hipLaunchKernelGGL(k_rows_bounds, dim3(grid), dim3(256), 0, s->stream,
                       s->d_payload, s->d_sidecar, limit, s->d_blocks, nb,
                       min_ts, max_ts, flags, s->rows_desc, preds, n_preds,
                       s->d_pred_bm, s->d_pred_flags, s->d_top_bkeys,
                       s->d_rows_blo, s->d_top_bvalid, s->d_err);
    const int64_t ts_wgs = (nb + WAVE - 1) / WAVE;   // 64 blocks per step
    hipLaunchKernelGGL(k_rows_bounds_ts,
                       dim3((unsigned)((int64_t)slots < ts_wgs ? slots : ts_wgs)),
                       dim3(WAVE), 0, s->stream, s->d_payload, limit,
                       s->d_blocks, nb, s->rows_desc, s->d_top_bkeys,
                       s->d_top_bvalid, s->d_top_grid, s->d_err);
    HIP_TRY(s, hipGetLastError());
    if ((rc = rows_select(s, s->d_top_bkeys, s->d_rows_blo, nullptr,
                          s->d_top_bvalid, (uint64_t)nb, N, &s->d_rows_st[0],
                          st_blocks, s->d_top_chosen)))
        return rc;
    hipLaunchKernelGGL(k_top_row_range, dim3((N + 3) / 4), dim3(256), 0,
                       s->stream, s->d_payload, s->d_blocks, nb, min_ts,
                       max_ts, flags, st_blocks, s->d_top_chosen,
                       s->d_top_range, N, s->d_err);
    hipLaunchKernelGGL(k_rows_row_keys, dim3(N), dim3(WAVE), 0, s->stream,
                       s->d_payload, s->d_sidecar, limit, s->d_blocks, nb,
                       s->rows_desc, preds, n_preds, s->d_pred_bm,
                       s->d_pred_flags, st_blocks, s->d_top_chosen,
                       s->d_top_range, s->d_top_grid, s->d_top_rvalid,
                       s->d_err);
    HIP_TRY(s, hipGetLastError());
    if ((rc = rows_select(s, s->d_top_grid, s->d_rows_blo, s->d_top_chosen,
                          s->d_top_rvalid, n_rows, N, &s->d_rows_st[2],
                          st_rows, s->d_top_winners)))
        return rc;
    hipLaunchKernelGGL(k_rows_resolve_keys, dim3((N + 255) / 256), dim3(256),
                       0, s->stream, s->d_blocks, nb, st_rows,
                       s->d_top_chosen, s->d_top_winners, s->d_top_grid,
                       s->d_top_recs, N);
    hipLaunchKernelGGL(k_top_resolve, dim3(N), dim3(WAVE), 0, s->stream,
                       s->d_payload, limit, s->d_blocks, nb, st_rows,
                       s->d_top_grid, s->d_top_recs, s->d_err);
    hipLaunchKernelGGL(k_rows_resolve_field, dim3(N), dim3(WAVE), 0,
                       s->stream, s->d_payload, limit, s->d_blocks, nb,
                       st_rows, s->d_top_grid, s->d_top_recs, s->d_err);
    HIP_TRY(s, hipGetLastError());
    HIP_TRY(s, hipEventRecord(s->ev_stop, s->stream));
    return BYDB_OK;
}

// a top or row-scan session branches to its own pipeline here, and nowhere
// else
static int scan_or_top(bydb_session *s, int64_t min_ts, int64_t max_ts,
                       PredBlock *preds, int n_preds) {
    return s->rows_on  ? launch_rows(s, min_ts, max_ts, preds, n_preds)
           : s->top_on ? launch_top(s, min_ts, max_ts, preds, n_preds)
                       : launch_scan(s, min_ts, max_ts, preds, n_preds);
}

// The single point where every consume entry point reaches launch_scan.
// n_slots is what the resolve stage resolved (0: unfiltered).  Without
// superseded rows this is launch_scan itself — the same instantiations,
// the same arguments, no extra launch.  With them, k_dedup_apply rewrites
// the resolve output first (an unfiltered consume gets an all-CLEAR flag
// table to rewrite) and the scan runs with at least one predicate slot.
static int scan_deduped(bydb_session *s, int64_t min_ts, int64_t max_ts,
                        PredBlock *preds, int n_slots) {
    if (!dedup_active(s)) return scan_or_top(s, min_ts, max_ts, preds, n_slots);
    if (n_slots == 0) {
        int rc = ensure_pred_buffers(s);
        if (rc != BYDB_OK) return rc;
        HIP_TRY(s, hipMemsetAsync(s->d_pred_flags, PF_CLEAR,
                                  (size_t)s->n_blocks, s->stream));
        rc = ensure_pred_bm(s, dedup_bm_words(s));
        if (rc != BYDB_OK) return rc;
        s->dd_bm_base = 0;
    }
    int64_t route_wgs = (s->dd_n_full + WAVE - 1) / WAVE;
    int64_t want = s->dd_n_partial > route_wgs ? s->dd_n_partial : route_wgs;
    int grid = (int)(want < 1 ? 1
                     : want < BLOCK_KERNEL_MAX_WGS ? want
                                                   : BLOCK_KERNEL_MAX_WGS);
    hipLaunchKernelGGL(k_dedup_apply, dim3(grid), dim3(WAVE), 0, s->stream,
                       s->d_payload, s->d_sidecar, s->d_blocks, s->n_blocks,
                       s->d_dd_plist, s->dd_n_partial, s->d_dd_flist,
                       s->dd_n_full, s->d_dd_surv, s->d_preds, n_slots,
                       s->d_pred_flags, s->d_pred_bm, s->dd_bm_base,
                       s->d_walk_count);
    HIP_TRY(s, hipGetLastError());
    return scan_or_top(s, min_ts, max_ts, s->d_preds,
                       n_slots > 1 ? n_slots : 1);
}

extern "C" int bydb_consume(bydb_session *s, int64_t min_ts, int64_t max_ts,
                            const uint8_t *pred, uint64_t pred_len) {
    if (pred_len == 0) {
        return bydb_consume_multi(s, min_ts, max_ts, nullptr, nullptr, 0);
    }
    const uint8_t *preds[1] = {pred};
    uint64_t lens[1] = {pred_len};
    return bydb_consume_multi(s, min_ts, max_ts, preds, lens, 1);
}

static int consume_conds(bydb_session *s, int64_t min_ts, int64_t max_ts,
                         const bydb_tag_cond *conds, int n_conds);

// The argument rules every condition-taking entry point shares (header:
// "tag filter operators").
static int validate_conds(bydb_session *s, const bydb_tag_cond *conds,
                          int n_conds) {
    if (n_conds < 0 || n_conds > BYDB_FILTER_MAX_CONDS ||
        (n_conds > 0 && conds == nullptr)) {
        s->err = "n_conds must be 0..8";
        return BYDB_ERR_BAD_ARG;
    }
    uint64_t total_values = 0;
    for (int i = 0; i < n_conds; i++) {
        const bydb_tag_cond *c = &conds[i];
        const bool is_set = c->op == BYDB_OP_IN || c->op == BYDB_OP_NOT_IN;
        const bool is_range = c->op == BYDB_OP_LT || c->op == BYDB_OP_GT ||
                              c->op == BYDB_OP_LE || c->op == BYDB_OP_GE;
        if (c->slot < 0 || c->slot > 2) {
            s->err = "filter condition slot must be 0..2";
            return BYDB_ERR_BAD_ARG;
        }
        if (!is_set && !is_range && c->op != BYDB_OP_EQ &&
            c->op != BYDB_OP_NE) {
            s->err = "unknown filter operator";
            return BYDB_ERR_BAD_ARG;
        }
        if (c->tag_type != BYDB_TAG_STRING && c->tag_type != BYDB_TAG_INT) {
            s->err = "unknown filter tag type";
            return BYDB_ERR_BAD_ARG;
        }
        if (is_set ? c->n_values < 1 : c->n_values != 1) {
            s->err = is_set ? "IN / NOT_IN need at least one value"
                            : "operator takes exactly one value";
            return BYDB_ERR_BAD_ARG;
        }
        total_values += c->n_values;
        if (total_values > BYDB_FILTER_MAX_VALUES) {
            s->err = "more than 4096 filter values in one call";
            return BYDB_ERR_BAD_ARG;
        }
        if (c->value_offs == nullptr ||
            (c->values == nullptr &&
             c->value_offs[c->n_values] != c->value_offs[0])) {
            s->err = "filter condition values missing";
            return BYDB_ERR_BAD_ARG;
        }
        for (uint32_t v = 0; v < c->n_values; v++)
            if (c->value_offs[v + 1] < c->value_offs[v]) {
                s->err = "filter value offsets must ascend";
                return BYDB_ERR_BAD_ARG;
            }
        if (is_range && c->tag_type == BYDB_TAG_INT &&
            c->value_offs[1] - c->value_offs[0] != 8) {
            s->err = "int range literal must be an 8-byte cell";
            return BYDB_ERR_BAD_ARG;
        }
    }
    return BYDB_OK;
}

// Scan under ANDed tag conditions (header: "tag filter operators"): the
// public entry point validates, consume_conds does the work.
extern "C" int bydb_consume_filter(bydb_session *s, int64_t min_ts,
                                   int64_t max_ts, const bydb_tag_cond *conds,
                                   int n_conds) {
    HIP_TRY(s, hipSetDevice(s->device));
    if (!s->d_acc) { s->err = "configure first"; return BYDB_ERR_STATE; }
    if (s->n_blocks == 0) { s->err = "no part resident"; return BYDB_ERR_STATE; }
    int rc = validate_conds(s, conds, n_conds);
    if (rc != BYDB_OK) return rc;
    return consume_conds(s, min_ts, max_ts, conds, n_conds);
}

// The device form of validated conditions (n_conds >= 1).  The host sorts
// the conditions by slot — order[k] is the caller's index of FilterSet
// condition k — and uploads one arena — u64 section (set value offsets,
// set hashes), u32 section (set slots), byte section (literals and set
// values) — in a single copy.  IN / NOT_IN lists become the
// open-addressing table the group-by domain uses, so the device probes
// once per value instead of comparing n_values times.
static int build_filter_set(bydb_session *s, const bydb_tag_cond *conds,
                            int n_conds, FilterSet *fs_out,
                            int order[BYDB_FILTER_MAX_CONDS]) {
    // conditions sorted by slot (stable), arena sections built on the host
    int n_ord = 0;
    FilterSet &fs = *fs_out;
    memset(&fs, 0, sizeof(fs));
    for (int sl = 0; sl < 3; sl++) {
        fs.first[sl] = n_ord;
        fs.all_neg[sl] = 1;
        for (int i = 0; i < n_conds; i++)
            if (conds[i].slot == sl) {
                order[n_ord++] = i;
                if (conds[i].op != BYDB_OP_NE && conds[i].op != BYDB_OP_NOT_IN)
                    fs.all_neg[sl] = 0;
                fs.n_slots = sl + 1;
            }
    }
    fs.first[3] = n_ord;
    std::vector<uint64_t> a64;
    std::vector<uint32_t> a32;
    std::vector<uint8_t> a8;
    struct SetPos { uint64_t hashes, offs, gids; uint32_t tsize; };
    SetPos pos[BYDB_FILTER_MAX_CONDS];
    uint64_t lit_pos[BYDB_FILTER_MAX_CONDS];
    for (int k = 0; k < n_ord; k++) {
        const bydb_tag_cond *c = &conds[order[k]];
        const uint64_t v0 = c->value_offs[0];
        const uint64_t blob_len = c->value_offs[c->n_values] - v0;
        lit_pos[k] = a8.size();
        if (blob_len)
            a8.insert(a8.end(), c->values + v0, c->values + v0 + blob_len);
        pos[k].tsize = 0;
        if (c->op != BYDB_OP_IN && c->op != BYDB_OP_NOT_IN) continue;
        uint32_t tsize = 4;
        while (tsize < c->n_values * 4) tsize <<= 1;
        pos[k].tsize = tsize;
        pos[k].offs = a64.size();
        for (uint32_t v = 0; v <= c->n_values; v++)
            a64.push_back(lit_pos[k] + (c->value_offs[v] - v0));
        pos[k].hashes = a64.size();
        a64.resize(a64.size() + tsize, 0);
        pos[k].gids = a32.size();
        a32.resize(a32.size() + tsize, GID_NONE);
        for (uint32_t v = 0; v < c->n_values; v++) {
            uint64_t h = fnv1a(c->values + c->value_offs[v],
                               c->value_offs[v + 1] - c->value_offs[v]);
            uint32_t sl = (uint32_t)h & (tsize - 1);
            while (a32[pos[k].gids + sl] != GID_NONE) sl = (sl + 1) & (tsize - 1);
            a64[pos[k].hashes + sl] = h;
            a32[pos[k].gids + sl] = v;
        }
    }
    const uint64_t off32 = a64.size() * sizeof(uint64_t);
    const uint64_t off8 = off32 + a32.size() * sizeof(uint32_t);
    const uint64_t arena_len = off8 + a8.size();
    s->filter_stage.resize(arena_len ? arena_len : 1);
    if (!a64.empty()) memcpy(s->filter_stage.data(), a64.data(), off32);
    if (!a32.empty())
        memcpy(s->filter_stage.data() + off32, a32.data(), off8 - off32);
    if (!a8.empty()) memcpy(s->filter_stage.data() + off8, a8.data(), a8.size());
    if (s->filter_cap < s->filter_stage.size()) {
        if (s->d_filter) { (void)hipFree(s->d_filter); s->d_filter = nullptr; }
        uint64_t ncap = 4096;
        while (ncap < s->filter_stage.size()) ncap *= 2;
        HIP_TRY(s, hipMalloc(&s->d_filter, ncap));
        s->filter_cap = ncap;
    }
    HIP_TRY(s, hipMemcpyAsync(s->d_filter, s->filter_stage.data(),
                              s->filter_stage.size(), hipMemcpyHostToDevice,
                              s->stream));
    const uint64_t *d64 = (const uint64_t *)s->d_filter;
    const uint32_t *d32 = (const uint32_t *)(s->d_filter + off32);
    const uint8_t *d8 = s->d_filter + off8;
    for (int k = 0; k < n_ord; k++) {
        const bydb_tag_cond *c = &conds[order[k]];
        FilterCond *fc = &fs.c[k];
        fc->op = (uint8_t)c->op;
        fc->is_int = c->tag_type == BYDB_TAG_INT;
        if (pos[k].tsize) {
            fc->set.blob = d8;
            fc->set.offs = d64 + pos[k].offs;
            fc->set.hashes = d64 + pos[k].hashes;
            fc->set.gids = d32 + pos[k].gids;
            fc->set.table_size = pos[k].tsize;
            fc->set.n = c->n_values;
        } else {
            fc->lit = d8 + lit_pos[k];
            fc->lit_len = c->value_offs[1] - c->value_offs[0];
            if (fc->is_int && fc->lit_len == 8) {
                uint64_t u = 0;
                for (int b = 0; b < 8; b++)
                    u = (u << 8) | c->values[c->value_offs[0] + b];
                fc->lit_i = (int64_t)(u ^ (1ull << 63));
            }
        }
    }
    return BYDB_OK;
}

// The one resolve stage behind every conjunctive consume entry point, over
// conditions already validated: the two resolves feed the scan launch.
static int consume_conds(bydb_session *s, int64_t min_ts, int64_t max_ts,
                         const bydb_tag_cond *conds, int n_conds) {
    int rc = dedup_build(s);
    if (rc != BYDB_OK) return rc;
    if (n_conds == 0) return scan_deduped(s, min_ts, max_ts, nullptr, 0);
    FilterSet fs;
    int order[BYDB_FILTER_MAX_CONDS];
    rc = build_filter_set(s, conds, n_conds, &fs, order);
    if (rc != BYDB_OK) return rc;
    rc = ensure_pred_buffers(s);
    if (rc != BYDB_OK) return rc;
    const int rthreads = 256;
    const int rblocks = (int)((s->n_blocks + rthreads - 1) / rthreads);
    hipLaunchKernelGGL(k_resolve_filter, dim3(rblocks), dim3(rthreads), 0,
                       s->stream, s->d_payload, s->d_sidecar, s->d_blocks,
                       s->n_blocks, fs, s->d_preds, s->d_pred_flags,
                       s->d_walk_count);
    HIP_TRY(s, hipGetLastError());
    // plain columns: one bitmap per normalized (block,slot) stream at most,
    // counted at part_append — the arena is sized without a round-trip;
    // the dedup-merged bitmaps (count known from the build) follow them
    s->dd_bm_base = s->n_plain_host * PLAIN_BM_WORDS;
    rc = ensure_pred_bm(s, s->dd_bm_base + dedup_bm_words(s));
    if (rc != BYDB_OK) return rc;
    if (s->n_plain_host > 0) {
        HIP_TRY(s, hipMemsetAsync(s->d_plain_ctr, 0, sizeof(uint32_t),
                                  s->stream));
        int pgrid = (int)(s->n_blocks < BLOCK_KERNEL_MAX_WGS
                              ? s->n_blocks
                              : BLOCK_KERNEL_MAX_WGS);
        for (int sl = 0; sl < fs.n_slots; sl++) {
            if (fs.first[sl] == fs.first[sl + 1]) continue;
            hipLaunchKernelGGL(k_resolve_plain_filter, dim3(pgrid), dim3(WAVE),
                               0, s->stream, s->d_payload, s->d_sidecar,
                               s->d_blocks, s->n_blocks, fs, sl,
                               s->d_preds + (int64_t)sl * s->n_blocks,
                               s->d_pred_bm, s->d_plain_ctr, s->n_plain_host);
            HIP_TRY(s, hipGetLastError());
        }
    }
    return scan_deduped(s, min_ts, max_ts, s->d_preds, fs.n_slots);
}

// ---- criteria trees (header: "AND / OR criteria trees") ----
// Validate a post-order tree and evaluate it for every assignment of its
// leaves at once: a node's value is a 256-bit vector over signatures, a
// leaf's is "bit c of the signature", AND / OR are bitwise.  Pure host.
static int tree_table(const bydb_filter_node *nodes, int n_nodes, int n_conds,
                      uint64_t table[4], bool *has_or, const char **why) {
    struct Bits { uint64_t w[4]; };
    static const uint64_t kLeaf[6] = {
        0xAAAAAAAAAAAAAAAAull, 0xCCCCCCCCCCCCCCCCull, 0xF0F0F0F0F0F0F0F0ull,
        0xFF00FF00FF00FF00ull, 0xFFFF0000FFFF0000ull, 0xFFFFFFFF00000000ull};
    *has_or = false;
    if (n_conds < 1 || n_conds > BYDB_FILTER_MAX_CONDS) {
        *why = "a filter tree takes 1..8 conditions";
        return BYDB_ERR_BAD_ARG;
    }
    if (n_nodes != 2 * n_conds - 1 || nodes == nullptr || table == nullptr) {
        *why = "filter tree needs n_nodes == 2 * n_conds - 1";
        return BYDB_ERR_BAD_ARG;
    }
    Bits val[2 * BYDB_FILTER_MAX_CONDS - 1];
    bool cond_used[BYDB_FILTER_MAX_CONDS] = {};
    bool has_parent[2 * BYDB_FILTER_MAX_CONDS - 1] = {};
    // signatures that exist: the low 2^n_conds bits
    Bits live;
    for (int w = 0; w < 4; w++) {
        int64_t bits = ((int64_t)1 << n_conds) - 64 * w;
        live.w[w] = bits >= 64 ? ~0ull : bits <= 0 ? 0 : (1ull << bits) - 1;
    }
    for (int i = 0; i < n_nodes; i++) {
        const bydb_filter_node &nd = nodes[i];
        if (nd.op == BYDB_NODE_LEAF) {
            if (nd.left < 0 || nd.left >= n_conds) {
                *why = "filter tree leaf names no condition";
                return BYDB_ERR_BAD_ARG;
            }
            if (cond_used[nd.left]) {
                *why = "filter tree references a condition twice";
                return BYDB_ERR_BAD_ARG;
            }
            cond_used[nd.left] = true;
            for (int w = 0; w < 4; w++) {
                uint64_t v = nd.left < 6 ? kLeaf[nd.left]
                             : nd.left == 6 ? ((w & 1) ? ~0ull : 0)
                                            : ((w & 2) ? ~0ull : 0);
                val[i].w[w] = v & live.w[w];
            }
        } else if (nd.op == BYDB_NODE_AND || nd.op == BYDB_NODE_OR) {
            if (nd.left < 0 || nd.left >= i || nd.right < 0 || nd.right >= i) {
                *why = "filter tree child index must be below its parent's";
                return BYDB_ERR_BAD_ARG;
            }
            if (nd.left == nd.right || has_parent[nd.left] ||
                has_parent[nd.right]) {
                *why = "filter tree node has two parents";
                return BYDB_ERR_BAD_ARG;
            }
            has_parent[nd.left] = has_parent[nd.right] = true;
            if (nd.op == BYDB_NODE_OR) *has_or = true;
            for (int w = 0; w < 4; w++)
                val[i].w[w] = nd.op == BYDB_NODE_AND
                                  ? val[nd.left].w[w] & val[nd.right].w[w]
                                  : val[nd.left].w[w] | val[nd.right].w[w];
        } else {
            *why = "unknown filter tree node op";
            return BYDB_ERR_BAD_ARG;
        }
    }
    for (int c = 0; c < n_conds; c++)
        if (!cond_used[c]) {
            *why = "filter tree never references a condition";
            return BYDB_ERR_BAD_ARG;
        }
    for (int i = 0; i + 1 < n_nodes; i++)
        if (!has_parent[i]) {
            *why = "filter tree node has no parent";
            return BYDB_ERR_BAD_ARG;
        }
    for (int w = 0; w < 4; w++) table[w] = val[n_nodes - 1].w[w];
    return BYDB_OK;
}

extern "C" int bydb_filter_tree_table(const bydb_filter_node *nodes,
                                      int n_nodes, int n_conds,
                                      uint64_t table[4]) {
    bool has_or;
    const char *why;
    return tree_table(nodes, n_nodes, n_conds, table, &has_or, &why);
}

extern "C" int bydb_filter_tree_stats(bydb_session *s, uint64_t out[4]) {
    for (int i = 0; i < 4; i++) out[i] = s->tree_stats[i];
    return BYDB_OK;
}

// Scan under a criteria tree.  A tree without an OR node is the
// conjunction consume_conds already resolves.  Otherwise k_resolve_tree
// classifies every block; its row-bitmap census is read back — the one
// host wait of this path — to size the bitmap arena, k_resolve_tree_rows
// fills the bitmaps, and the unchanged scan launch consumes the result.
extern "C" int bydb_consume_filter_tree(bydb_session *s, int64_t min_ts,
                                        int64_t max_ts,
                                        const bydb_tag_cond *conds, int n_conds,
                                        const bydb_filter_node *nodes,
                                        int n_nodes) {
    HIP_TRY(s, hipSetDevice(s->device));
    if (!s->d_acc) { s->err = "configure first"; return BYDB_ERR_STATE; }
    if (s->n_blocks == 0) { s->err = "no part resident"; return BYDB_ERR_STATE; }
    for (int i = 0; i < 4; i++) s->tree_stats[i] = 0;
    if (n_conds == 0 && n_nodes == 0)
        return consume_conds(s, min_ts, max_ts, nullptr, 0);
    int rc = validate_conds(s, conds, n_conds);
    if (rc != BYDB_OK) return rc;
    TreeSpec ts;
    memset(&ts, 0, sizeof(ts));
    bool has_or = false;
    const char *why = "";
    rc = tree_table(nodes, n_nodes, n_conds, ts.tt, &has_or, &why);
    if (rc != BYDB_OK) { s->err = why; return rc; }
    if (!has_or) return consume_conds(s, min_ts, max_ts, conds, n_conds);
    rc = dedup_build(s);
    if (rc != BYDB_OK) return rc;

    FilterSet fs;
    int order[BYDB_FILTER_MAX_CONDS];
    rc = build_filter_set(s, conds, n_conds, &fs, order);
    if (rc != BYDB_OK) return rc;
    for (int k = 0; k < n_conds; k++) ts.bits |= (uint32_t)order[k] << (4 * k);
    rc = ensure_pred_buffers(s);
    if (rc != BYDB_OK) return rc;
    if (!s->d_tree_stats)
        HIP_TRY(s, hipMalloc(&s->d_tree_stats, 4 * sizeof(uint32_t)));
    HIP_TRY(s, hipMemsetAsync(s->d_tree_stats, 0, 4 * sizeof(uint32_t),
                              s->stream));
    const int rthreads = 256;
    const int rblocks = (int)((s->n_blocks + rthreads - 1) / rthreads);
    hipLaunchKernelGGL(k_resolve_tree, dim3(rblocks), dim3(rthreads), 0,
                       s->stream, s->d_payload, s->d_sidecar, s->d_blocks,
                       s->n_blocks, fs, ts, s->d_preds, s->d_pred_flags,
                       s->d_walk_count, s->d_tree_stats);
    HIP_TRY(s, hipGetLastError());
    uint32_t h_stats[4] = {0, 0, 0, 0};
    HIP_TRY(s, hipMemcpyAsync(h_stats, s->d_tree_stats, sizeof(h_stats),
                              hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(s, hipStreamSynchronize(s->stream));
    for (int i = 0; i < 4; i++) s->tree_stats[i] = h_stats[i];
    const uint64_t n_row_blocks = h_stats[3];
    // one bitmap per row-bitmap block, then the dedup-merged bitmaps; the
    // arena only grows and is shared with the plain-column bitmaps of
    // consume_conds
    s->dd_bm_base = n_row_blocks * PLAIN_BM_WORDS;
    rc = ensure_pred_bm(s, s->dd_bm_base + dedup_bm_words(s));
    if (rc != BYDB_OK) return rc;
    if (n_row_blocks > 0) {
        HIP_TRY(s, hipMemsetAsync(s->d_plain_ctr, 0, sizeof(uint32_t),
                                  s->stream));
        int pgrid = (int)(s->n_blocks < BLOCK_KERNEL_MAX_WGS
                              ? s->n_blocks
                              : BLOCK_KERNEL_MAX_WGS);
        hipLaunchKernelGGL(k_resolve_tree_rows, dim3(pgrid), dim3(WAVE), 0,
                           s->stream, s->d_payload, s->d_sidecar, s->d_blocks,
                           s->n_blocks, fs, ts, s->d_preds, s->d_pred_flags,
                           s->d_pred_bm, s->d_plain_ctr,
                           s->pred_bm_cap / PLAIN_BM_WORDS);
        HIP_TRY(s, hipGetLastError());
    }
    return scan_deduped(s, min_ts, max_ts, s->d_preds, fs.n_slots);
}

// Equality predicates: one BYDB_OP_EQ string condition per non-empty slot.
extern "C" int bydb_consume_multi(bydb_session *s, int64_t min_ts,
                                  int64_t max_ts, const uint8_t *const *preds_in,
                                  const uint64_t *pred_lens, int n_preds) {
    HIP_TRY(s, hipSetDevice(s->device));
    if (!s->d_acc) { s->err = "configure first"; return BYDB_ERR_STATE; }
    if (s->n_blocks == 0) { s->err = "no part resident"; return BYDB_ERR_STATE; }
    if (n_preds < 0 || n_preds > 3) { s->err = "n_preds must be 0..3"; return BYDB_ERR_BAD_ARG; }
    // drop trailing disabled slots; interior empty slots mean "no
    // constraint on that tag" and may pass a NULL pointer
    while (n_preds > 0 && pred_lens[n_preds - 1] == 0) n_preds--;
    bydb_tag_cond conds[3];
    uint64_t offs[3][2];
    int n_conds = 0;
    for (int i = 0; i < n_preds; i++) {
        if (pred_lens[i] == 0) continue;
        offs[n_conds][0] = 0;
        offs[n_conds][1] = pred_lens[i];
        bydb_tag_cond *c = &conds[n_conds];
        c->slot = i;
        c->op = BYDB_OP_EQ;
        c->tag_type = BYDB_TAG_STRING;
        c->n_values = 1;
        c->values = preds_in[i];
        c->value_offs = offs[n_conds];
        n_conds++;
    }
    return consume_conds(s, min_ts, max_ts, conds, n_conds);
}

extern "C" double bydb_last_consume_ms(bydb_session *s) { return s->last_ms; }

static int finalize_common(bydb_session *s, bydb_partial *host_parts,
                           int64_t n_groups) {
    HIP_TRY(s, hipSetDevice(s->device));
    if ((uint32_t)n_groups != s->n_groups) {
        s->err = "n_groups mismatch";
        return BYDB_ERR_BAD_ARG;
    }
    HIP_TRY(s, hipStreamSynchronize(s->stream));
    if (s->consumed) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, s->ev_start, s->ev_stop) == hipSuccess)
            s->last_ms = ms;
    }
    DevErr de;
    HIP_TRY(s, hipMemcpy(&de, s->d_err, sizeof de, hipMemcpyDeviceToHost));
    if (de.code != DERR_NONE) {
        char buf[128];
        snprintf(buf, sizeof buf, "device decode error %u at block %u", de.code,
                 de.block_lo);
        s->err = buf;
        return BYDB_ERR_BAD_DATA;
    }
    HIP_TRY(s, hipMemcpy(host_parts, s->d_acc,
                         sizeof(bydb_partial) * (size_t)n_groups,
                         hipMemcpyDeviceToHost));
    return BYDB_OK;
}

// Go math.Pow10 restated (decode-side float restore must reproduce its
// table-multiply rounding — float.go:77-102).
static const double h_pow10tab[32] = {
    1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12,
    1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22, 1e23,
    1e24, 1e25, 1e26, 1e27, 1e28, 1e29, 1e30, 1e31};
static const double h_pow10postab32[10] = {
    1e0, 1e32, 1e64, 1e96, 1e128, 1e160, 1e192, 1e224, 1e256, 1e288};
static double go_pow10(int nn) {
    if (0 <= nn && nn <= 308)
        return h_pow10postab32[(unsigned)nn / 32] * h_pow10tab[(unsigned)nn % 32];
    return 0.0;  // callers only use 0..308
}

static double restore_f64(int64_t v, int16_t exp) {
    if (exp >= 0) return (double)v * go_pow10(exp);
    double r = (double)v;
    int neg = -(int)exp;
    while (neg > 0) {
        int step = neg < 308 ? neg : 308;
        r /= go_pow10(step);
        neg -= step;
    }
    return r;
}

static double restore_f64_from_double(double v, int16_t exp) {
    if (exp >= 0) return v * go_pow10(exp);
    double r = v;
    int neg = -(int)exp;
    while (neg > 0) {
        int step = neg < 308 ? neg : 308;
        r /= go_pow10(step);
        neg -= step;
    }
    return r;
}

// The float64 restore at finalize needs the column's decimal exponent
// (column payload header, column.go:253-263).  One query aggregates one
// field column, whose blocks share the exponent at the benchmark configs;
// the host sets it per session before finalize.
extern "C" int bydb_set_float_exp(bydb_session *s, int16_t exp) {
    s->float_exp = exp;
    return BYDB_OK;
}

extern "C" int bydb_finalize_partials(bydb_session *s, bydb_partial *out,
                                      int64_t n_groups) {
    return finalize_common(s, out, n_groups);
}

/* Per-group first-seen keys ((item << 13) | row in storage order; ~0 =
 * group never entered).  Sorting group ids by these keys reproduces the
 * reference's first-seen group materialisation order (computeKey
 * creates groups in row-iteration order, aggregation.go:523), so a Go
 * twin can emit NextBatch rows in reference order from the host-domain
 * buffers.  Caveats (documented in DESIGN.md): a group whose only rows
 * fail a BITMAP-mode (plain-tag) predicate inside a row-varying merge
 * may still record the run-entry key; within one (item,row) tie the
 * order is exact. */
extern "C" int bydb_group_first_seen(bydb_session *s, uint64_t *out,
                                     int64_t n_groups) {
    HIP_TRY(s, hipSetDevice(s->device));
    if ((uint32_t)n_groups != s->n_groups || !s->d_first_seen) {
        s->err = "n_groups mismatch or not configured";
        return BYDB_ERR_BAD_ARG;
    }
    HIP_TRY(s, hipStreamSynchronize(s->stream));
    HIP_TRY(s, hipMemcpy(out, s->d_first_seen,
                         sizeof(uint64_t) * (size_t)n_groups,
                         hipMemcpyDeviceToHost));
    return BYDB_OK;
}

static void partial_to_result(const bydb_partial *p, int field_vtype,
                              int16_t float_exp, bydb_result *r) {
    r->sum_i = p->sum_i;
    r->count = p->count;
    r->min_i = p->min_i;
    r->max_i = p->max_i;
    if (field_vtype == BYDB_VT_FLOAT64 && float_exp == INT16_MIN) {
        // raw IEEE-754 domain (nullable float columns): min/max carried
        // as order-preserving bit keys (convert/number.go:148-157), sum
        // carried directly as a double
        auto key_to_f64 = [](int64_t k) {
            uint64_t bits = k >= 0 ? (uint64_t)k
                                   : ~((uint64_t)k ^ 0x8000000000000000ull);
            double d;
            memcpy(&d, &bits, 8);
            return d;
        };
        r->min_f = p->count ? key_to_f64(p->min_i) : 1.7976931348623157e308;
        r->max_f = p->count ? key_to_f64(p->max_i) : -1.7976931348623157e308;
        r->sum_f = p->sum_f;
        double c = (double)p->count;
        r->mean_f = c == 0 ? 0 : (r->sum_f / c < 1 ? 1 : r->sum_f / c);
        r->mean_i = 0;
    } else if (field_vtype == BYDB_VT_FLOAT64) {
        // decimal-int domain -> float64 (monotone restore; float.go:69-102)
        r->min_f = p->count ? restore_f64(p->min_i, float_exp) : 1.7976931348623157e308;
        r->max_f = p->count ? restore_f64(p->max_i, float_exp) : -1.7976931348623157e308;
        r->sum_f = restore_f64_from_double(p->sum_f, float_exp);
        double c = (double)p->count;
        r->mean_f = c == 0 ? 0 : (r->sum_f / c < 1 ? 1 : r->sum_f / c);
        r->mean_i = 0;
    } else {
        r->sum_f = 0;
        r->min_f = 0;
        r->max_f = 0;
        r->mean_f = 0;
        // meanFunc.Val (function.go:30-45)
        r->mean_i = p->count == 0 ? 0
                    : (p->sum_i / p->count < 1 ? 1 : p->sum_i / p->count);
    }
}

extern "C" int bydb_finalize(bydb_session *s, bydb_result *out,
                             int64_t n_groups) {
    std::vector<bydb_partial> parts((size_t)n_groups);
    int rc = finalize_common(s, parts.data(), n_groups);
    if (rc != BYDB_OK) return rc;
    for (int64_t g = 0; g < n_groups; g++)
        partial_to_result(&parts[(size_t)g], s->field_vtype, s->float_exp, &out[(size_t)g]);
    return BYDB_OK;
}

// ---- BatchTop over raw rows: configure, finalize, shard merge ----

extern "C" int bydb_top_configure(bydb_session *s, int field_vtype, int64_t n,
                                  int asc) {
    if (n < 0 || n > BYDB_TOP_ROWS_MAX) {
        s->err = "top n outside 0..BYDB_TOP_ROWS_MAX";
        return BYDB_ERR_BAD_ARG;
    }
    if (field_vtype != BYDB_VT_INT64 && field_vtype != BYDB_VT_FLOAT64) {
        s->err = "top field_vtype must be int64 or float64";
        return BYDB_ERR_BAD_ARG;
    }
    if (field_vtype == BYDB_VT_FLOAT64 && s->float_exp == BYDB_FLOAT_RAW_EXP) {
        s->err = "top over a raw-float session is not supported";
        return BYDB_ERR_BAD_ARG;
    }
    // the consume entry points and bydb_reset want a configured session:
    // a one-group, no-function aggregate that no kernel ever touches
    int rc = bydb_agg_configure(s, field_vtype, 0, 1, BYDB_MODE_ALL);
    if (rc != BYDB_OK) return rc;
    s->top_on = true;
    s->top_n = n;
    s->top_asc = asc ? 1 : 0;
    return BYDB_OK;
}

extern "C" int bydb_top_finalize(bydb_session *s, bydb_top_row *out,
                                 int64_t cap, int64_t *out_n) {
    HIP_TRY(s, hipSetDevice(s->device));
    if (!s->top_on) { s->err = "not a top session"; return BYDB_ERR_STATE; }
    if (!out_n) { s->err = "null out_n"; return BYDB_ERR_BAD_ARG; }
    *out_n = 0;
    HIP_TRY(s, hipStreamSynchronize(s->stream));
    if (!s->consumed || s->top_n == 0) {
        s->consumed = false;
        return BYDB_OK;
    }
    float ms = 0;
    if (hipEventElapsedTime(&ms, s->ev_start, s->ev_stop) == hipSuccess)
        s->last_ms = ms;
    DevErr de;
    HIP_TRY(s, hipMemcpy(&de, s->d_err, sizeof de, hipMemcpyDeviceToHost));
    if (de.code != DERR_NONE) {
        char buf[128];
        snprintf(buf, sizeof buf, "device decode error %u at block %u%s",
                 de.code, de.block_lo,
                 de.code == DERR_TOP_NULL
                     ? " (top selected a row of a null-bearing block)" : "");
        s->err = buf;
        return BYDB_ERR_BAD_DATA;
    }
    TopSelState st;
    HIP_TRY(s, hipMemcpy(&st, &s->d_top_st[1], sizeof st,
                         hipMemcpyDeviceToHost));
    const int64_t got = (int64_t)st.n_out;
    if (got > s->top_n) { s->err = "top selector overran"; return BYDB_ERR; }
    *out_n = got;
    if (cap < got || (got > 0 && !out)) {
        s->err = "top_finalize: out holds fewer rows than selected";
        return BYDB_ERR_OOM;   // the epoch stays open: call again
    }
    std::vector<TopRec> recs((size_t)got);
    if (got > 0)
        HIP_TRY(s, hipMemcpy(recs.data(), s->d_top_recs,
                             sizeof(TopRec) * (size_t)got,
                             hipMemcpyDeviceToHost));
    // the device hands winners over in seq order: a stable sort by key
    // leaves equal values in input order (top.go:66-82, 190-199)
    std::stable_sort(recs.begin(), recs.end(),
                     [](const TopRec &a, const TopRec &b) {
                         return a.key > b.key;
                     });
    const bool is_f = s->field_vtype == BYDB_VT_FLOAT64;
    for (int64_t i = 0; i < got; i++) {
        const TopRec &r = recs[(size_t)i];
        bydb_top_row *o = &out[i];
        o->series_id = r.series_id;
        o->ts = r.ts;
        o->version = r.version;
        o->value_i = r.value;
        o->value_f = is_f ? restore_f64(r.value, (int16_t)r.exp) : 0.0;
        o->seq = r.seq;
    }
    s->consumed = false;
    return BYDB_OK;
}

extern "C" int bydb_top_rows_merge_src(const bydb_top_row *const *lists,
                                       const int64_t *lens, int n_lists,
                                       int field_vtype, int64_t n, int asc,
                                       bydb_top_row *out, int32_t *out_list,
                                       int64_t *out_index, int64_t *out_n) {
    if (!out_n || n_lists < 0 || n < 0 || (n_lists > 0 && (!lists || !lens)) ||
        (field_vtype != BYDB_VT_INT64 && field_vtype != BYDB_VT_FLOAT64))
        return BYDB_ERR_BAD_ARG;
    struct Ent { const bydb_top_row *r; int list; };
    std::vector<Ent> all;
    for (int l = 0; l < n_lists; l++) {
        if (lens[l] < 0 || (lens[l] > 0 && !lists[l])) return BYDB_ERR_BAD_ARG;
        for (int64_t i = 0; i < lens[l]; i++) all.push_back({&lists[l][i], l});
    }
    const bool is_f = field_vtype == BYDB_VT_FLOAT64;
    // better value first; equal values: the earlier list, then the smaller
    // seq.  Shards restore in their own exponents, so float64 rows compare
    // as the reference compares them: by value_f.
    std::stable_sort(all.begin(), all.end(), [&](const Ent &a, const Ent &b) {
        if (is_f) {
            if (a.r->value_f != b.r->value_f)
                return asc ? a.r->value_f < b.r->value_f
                           : a.r->value_f > b.r->value_f;
        } else if (a.r->value_i != b.r->value_i) {
            return asc ? a.r->value_i < b.r->value_i
                       : a.r->value_i > b.r->value_i;
        }
        if (a.list != b.list) return a.list < b.list;
        return a.r->seq < b.r->seq;
    });
    const int64_t take = (int64_t)all.size() < n ? (int64_t)all.size() : n;
    *out_n = take;
    if (take > 0 && !out) return BYDB_ERR_BAD_ARG;
    for (int64_t i = 0; i < take; i++) {
        const Ent &e = all[(size_t)i];
        out[i] = *e.r;
        // where the row came from: the shard to ask for its tags
        if (out_list) out_list[i] = e.list;
        if (out_index) out_index[i] = (int64_t)(e.r - lists[e.list]);
    }
    return BYDB_OK;
}

extern "C" int bydb_top_rows_merge(const bydb_top_row *const *lists,
                                   const int64_t *lens, int n_lists,
                                   int field_vtype, int64_t n, int asc,
                                   bydb_top_row *out, int64_t *out_n) {
    return bydb_top_rows_merge_src(lists, lens, n_lists, field_vtype, n, asc,
                                   out, nullptr, nullptr, out_n);
}

// ---- Scan -> Limit over raw rows: configure, finalize, shard merge ----

static bool rows_window_ok(int64_t offset, int64_t limit) {
    return offset >= 0 && limit >= 0 && offset <= BYDB_TOP_ROWS_MAX &&
           limit <= BYDB_TOP_ROWS_MAX - offset;
}

// queryResult.Less (query.go:913-943) plus this engine's seq tiebreak
static bool rows_before(int order, int64_t ts_a, uint64_t sid_a, int64_t ts_b,
                        uint64_t sid_b, bool *tie) {
    *tie = false;
    if (ts_a != ts_b)
        return order == BYDB_ORDER_TS_DESC ? ts_a > ts_b : ts_a < ts_b;
    if (sid_a != sid_b) return sid_a < sid_b;
    *tie = true;
    return false;
}

extern "C" int bydb_rows_configure(bydb_session *s, int field_vtype,
                                   int64_t offset, int64_t limit, int order) {
    if (!rows_window_ok(offset, limit)) {
        s->err = "row scan window outside 0..BYDB_TOP_ROWS_MAX";
        return BYDB_ERR_BAD_ARG;
    }
    if (order != BYDB_ORDER_TS_ASC && order != BYDB_ORDER_TS_DESC) {
        s->err = "row scan order must be BYDB_ORDER_TS_ASC or _DESC";
        return BYDB_ERR_BAD_ARG;
    }
    if (field_vtype != BYDB_VT_INT64 && field_vtype != BYDB_VT_FLOAT64) {
        s->err = "row scan field_vtype must be int64 or float64";
        return BYDB_ERR_BAD_ARG;
    }
    if (field_vtype == BYDB_VT_FLOAT64 && s->float_exp == BYDB_FLOAT_RAW_EXP) {
        s->err = "row scan over a raw-float session is not supported";
        return BYDB_ERR_BAD_ARG;
    }
    // as bydb_top_configure: a one-group, no-function aggregate that no
    // kernel ever touches keeps the consume entry points and bydb_reset happy
    int rc = bydb_agg_configure(s, field_vtype, 0, 1, BYDB_MODE_ALL);
    if (rc != BYDB_OK) return rc;
    s->rows_on = true;
    s->rows_offset = offset;
    s->rows_limit = limit;
    s->rows_desc = order == BYDB_ORDER_TS_DESC ? 1 : 0;
    return BYDB_OK;
}

extern "C" int bydb_rows_finalize(bydb_session *s, bydb_top_row *out,
                                  int64_t cap, int64_t *out_n) {
    HIP_TRY(s, hipSetDevice(s->device));
    if (!s->rows_on) { s->err = "not a row-scan session"; return BYDB_ERR_STATE; }
    if (!out_n) { s->err = "null out_n"; return BYDB_ERR_BAD_ARG; }
    *out_n = 0;
    HIP_TRY(s, hipStreamSynchronize(s->stream));
    if (!s->consumed || s->rows_limit == 0) {
        s->consumed = false;
        return BYDB_OK;
    }
    float ms = 0;
    if (hipEventElapsedTime(&ms, s->ev_start, s->ev_stop) == hipSuccess)
        s->last_ms = ms;
    DevErr de;
    HIP_TRY(s, hipMemcpy(&de, s->d_err, sizeof de, hipMemcpyDeviceToHost));
    if (de.code != DERR_NONE) {
        char buf[128];
        snprintf(buf, sizeof buf, "device decode error %u at block %u%s",
                 de.code, de.block_lo,
                 de.code == DERR_TOP_NULL
                     ? " (row scan selected a row of a null-bearing block)"
                     : "");
        s->err = buf;
        return BYDB_ERR_BAD_DATA;
    }
    TopSelState st;
    HIP_TRY(s, hipMemcpy(&st, &s->d_rows_st[3], sizeof st,
                         hipMemcpyDeviceToHost));
    const int64_t sel = (int64_t)st.n_out;
    if (sel > s->rows_offset + s->rows_limit) {
        s->err = "row selector overran";
        return BYDB_ERR;
    }
    const int64_t got = sel > s->rows_offset ? sel - s->rows_offset : 0;
    *out_n = got;
    if (cap < got || (got > 0 && !out)) {
        s->err = "rows_finalize: out holds fewer rows than the window";
        return BYDB_ERR_OOM;   // the epoch stays open: call again
    }
    std::vector<TopRec> recs((size_t)sel);
    if (sel > 0)
        HIP_TRY(s, hipMemcpy(recs.data(), s->d_top_recs,
                             sizeof(TopRec) * (size_t)sel,
                             hipMemcpyDeviceToHost));
    const int order = s->rows_desc ? BYDB_ORDER_TS_DESC : BYDB_ORDER_TS_ASC;
    std::sort(recs.begin(), recs.end(),
              [order](const TopRec &a, const TopRec &b) {
                  bool tie;
                  bool lt = rows_before(order, a.ts, a.series_id, b.ts,
                                        b.series_id, &tie);
                  return tie ? a.seq < b.seq : lt;
              });
    const bool is_f = s->field_vtype == BYDB_VT_FLOAT64;
    for (int64_t i = 0; i < got; i++) {
        const TopRec &r = recs[(size_t)(s->rows_offset + i)];
        bydb_top_row *o = &out[i];
        o->series_id = r.series_id;
        o->ts = r.ts;
        o->version = r.version;
        o->value_i = r.value;
        o->value_f = is_f ? restore_f64(r.value, (int16_t)r.exp) : 0.0;
        o->seq = r.seq;
    }
    s->consumed = false;
    return BYDB_OK;
}

extern "C" int bydb_rows_merge_src(const bydb_top_row *const *lists,
                                   const int64_t *lens, int n_lists,
                                   int64_t offset, int64_t limit, int order,
                                   bydb_top_row *out, int32_t *out_list,
                                   int64_t *out_index, int64_t *out_n) {
    if (!out_n || n_lists < 0 || !rows_window_ok(offset, limit) ||
        (n_lists > 0 && (!lists || !lens)) ||
        (order != BYDB_ORDER_TS_ASC && order != BYDB_ORDER_TS_DESC))
        return BYDB_ERR_BAD_ARG;
    *out_n = 0;
    struct Ent { const bydb_top_row *r; int list; };
    std::vector<Ent> all;
    for (int l = 0; l < n_lists; l++) {
        if (lens[l] < 0 || (lens[l] > 0 && !lists[l])) return BYDB_ERR_BAD_ARG;
        for (int64_t i = 0; i < lens[l]; i++) all.push_back({&lists[l][i], l});
    }
    std::stable_sort(all.begin(), all.end(), [&](const Ent &a, const Ent &b) {
        bool tie;
        bool lt = rows_before(order, a.r->ts, a.r->series_id, b.r->ts,
                              b.r->series_id, &tie);
        if (!tie) return lt;
        if (a.list != b.list) return a.list < b.list;
        return a.r->seq < b.r->seq;
    });
    const int64_t total = (int64_t)all.size();
    int64_t take = total > offset ? total - offset : 0;
    if (take > limit) take = limit;
    *out_n = take;
    if (take > 0 && !out) return BYDB_ERR_BAD_ARG;
    for (int64_t i = 0; i < take; i++) {
        const Ent &e = all[(size_t)(offset + i)];
        out[i] = *e.r;
        if (out_list) out_list[i] = e.list;
        if (out_index) out_index[i] = (int64_t)(e.r - lists[e.list]);
    }
    return BYDB_OK;
}

extern "C" int bydb_rows_merge(const bydb_top_row *const *lists,
                               const int64_t *lens, int n_lists,
                               int64_t offset, int64_t limit, int order,
                               bydb_top_row *out, int64_t *out_n) {
    return bydb_rows_merge_src(lists, lens, n_lists, offset, limit, order, out,
                               nullptr, nullptr, out_n);
}

// ---- tag projection for row results ----

// d_tf: what the host uploads, what the kernels keep, and — contiguous, one
// download — what the host reads back
struct TfLayout {
    uint64_t seqs[BYDB_TAG_FETCH_MAX];
    TagFetchRec recs[BYDB_TAG_FETCH_MAX];
    struct Back {
        TagFetchResult res;
        uint64_t offs[BYDB_TAG_FETCH_MAX + 1];
        uint8_t nil[BYDB_TAG_FETCH_MAX];
    } back;
};

extern "C" int bydb_rows_fetch_tags(bydb_session *s, const uint64_t *seqs,
                                    int64_t n, int slot, uint8_t *data,
                                    uint64_t data_cap, uint64_t *offs,
                                    uint8_t *nil, uint64_t *data_len) {
    if (n < 0 || n > BYDB_TAG_FETCH_MAX) {
        s->err = "fetch_tags: n outside 0..BYDB_TAG_FETCH_MAX";
        return BYDB_ERR_BAD_ARG;
    }
    if (slot < 0 || slot > 2) {
        s->err = "fetch_tags: slot outside 0..2";
        return BYDB_ERR_BAD_ARG;
    }
    if (n == 0) {
        if (offs) offs[0] = 0;
        if (data_len) *data_len = 0;
        return BYDB_OK;
    }
    if (!seqs || !offs || !nil || !data_len) {
        s->err = "fetch_tags: null seqs / offs / nil / data_len";
        return BYDB_ERR_BAD_ARG;
    }
    if (s->n_blocks == 0) {
        s->err = "fetch_tags: no part is resident";
        return BYDB_ERR_STATE;
    }
    HIP_TRY(s, hipSetDevice(s->device));
    if (!s->d_tf) {
        if (hipMalloc(&s->d_tf, sizeof(TfLayout)) != hipSuccess) {
            (void)hipGetLastError();
            s->d_tf = nullptr;
            s->err = "fetch_tags: request scratch allocation failed (" +
                     std::to_string(sizeof(TfLayout)) + " bytes)";
            return BYDB_ERR_OOM;
        }
    }
    TfLayout *tf = (TfLayout *)s->d_tf;
    HIP_TRY(s, hipMemcpyAsync(tf->seqs, seqs, sizeof(uint64_t) * (size_t)n,
                              hipMemcpyHostToDevice, s->stream));
    hipLaunchKernelGGL(k_tag_fetch_locate, dim3((unsigned)n), dim3(WAVE), 0,
                       s->stream, s->d_payload, s->d_sidecar, s->d_blocks,
                       s->n_blocks, tf->seqs, n, slot, tf->recs);
    hipLaunchKernelGGL(k_tag_fetch_offsets, dim3(1), dim3(BYDB_TAG_FETCH_MAX),
                       0, s->stream, tf->recs, n, tf->back.offs, tf->back.nil,
                       &tf->back.res);
    HIP_TRY(s, hipGetLastError());
    // the call's first host wait; it is synchronous by contract
    static_assert(offsetof(TfLayout::Back, nil) ==
                      sizeof(TagFetchResult) +
                          sizeof(uint64_t) * (BYDB_TAG_FETCH_MAX + 1),
                  "TfLayout::Back is read back as one range");
    TfLayout::Back back;
    HIP_TRY(s, hipMemcpyAsync(&back, &tf->back,
                              offsetof(TfLayout::Back, nil) + (size_t)n,
                              hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(s, hipStreamSynchronize(s->stream));
    if (back.res.bad_seq != TF_NONE) {
        const uint32_t i = back.res.bad_seq;
        char buf[160];
        snprintf(buf, sizeof buf,
                 "fetch_tags: seqs[%u] names block %llu row %u outside the "
                 "resident part (%lld blocks)",
                 i, (unsigned long long)(seqs[i] >> 13),
                 (unsigned)(seqs[i] & 8191), (long long)s->n_blocks);
        s->err = buf;
        return BYDB_ERR_BAD_ARG;
    }
    if (back.res.bad_stream != TF_NONE) {
        const uint32_t i = back.res.bad_stream;
        char buf[160];
        snprintf(buf, sizeof buf,
                 "fetch_tags: tag stream of block %llu on slot %d cannot be "
                 "parsed (seqs[%u])",
                 (unsigned long long)(seqs[i] >> 13), slot, i);
        s->err = buf;
        return BYDB_ERR_BAD_DATA;
    }
    const uint64_t total = back.res.total;
    *data_len = total;
    memcpy(offs, back.offs, sizeof(uint64_t) * (size_t)(n + 1));
    memcpy(nil, back.nil, (size_t)n);
    if (data_cap < total || (total > 0 && !data)) {
        s->err = "fetch_tags: data holds fewer bytes than the values (" +
                 std::to_string(total) + ")";
        return BYDB_ERR_OOM;
    }
    if (total == 0) return BYDB_OK;
    if (s->tf_out_cap < total) {
        if (s->d_tf_out) (void)hipFree(s->d_tf_out);
        s->d_tf_out = nullptr;
        s->tf_out_cap = 0;
        uint64_t ncap = 64 << 10;
        while (ncap < total) ncap *= 2;
        if (hipMalloc(&s->d_tf_out, ncap) != hipSuccess) {
            (void)hipGetLastError();
            s->d_tf_out = nullptr;
            s->err = "fetch_tags: output arena allocation failed (" +
                     std::to_string(ncap) + " bytes)";
            return BYDB_ERR_OOM;
        }
        s->tf_out_cap = ncap;
    }
    hipLaunchKernelGGL(k_tag_fetch_copy, dim3((unsigned)n), dim3(WAVE), 0,
                       s->stream, s->d_payload, s->d_sidecar, tf->recs,
                       tf->back.offs, n, s->d_tf_out);
    HIP_TRY(s, hipGetLastError());
    HIP_TRY(s, hipMemcpyAsync(data, s->d_tf_out, total, hipMemcpyDeviceToHost,
                              s->stream));
    HIP_TRY(s, hipStreamSynchronize(s->stream));
    return BYDB_OK;
}

extern "C" int bydb_reduce_partials2(const bydb_partial *parts,
                                     int64_t n_parts_per_group, int64_t n_groups,
                                     int field_vtype, int16_t float_exp,
                                     bydb_result *out) {
    for (int64_t g = 0; g < n_groups; g++) {
        bydb_partial acc;
        acc.sum_i = 0;
        acc.count = 0;
        acc.min_i = INT64_MAX;
        acc.max_i = INT64_MIN;
        acc.sum_f = 0;
        // Combine — aggregation_reduce.go:120-138 / function.go Reduce
        for (int64_t k = 0; k < n_parts_per_group; k++) {
            const bydb_partial *p = &parts[k * n_groups + g];
            acc.sum_i = (int64_t)((uint64_t)acc.sum_i + (uint64_t)p->sum_i);
            acc.count += p->count;
            if (p->min_i < acc.min_i) acc.min_i = p->min_i;
            if (p->max_i > acc.max_i) acc.max_i = p->max_i;
            acc.sum_f += p->sum_f;
        }
        partial_to_result(&acc, field_vtype, float_exp, &out[g]);
    }
    return BYDB_OK;
}
