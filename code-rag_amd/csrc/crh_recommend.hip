// crh_recommend.hip -- recommend by example ("more like these, not like those") selected on the device.
//
// The reference's planner has a find_similar intent ("Other functions like X") and can only embed a snippet for it; Qdrant's
// counterpart is RecommendQuery(positive, negative, strategy) -- known by description only.  The definitions below are THIS
// repository's (tests/recommend_cases.py restates both kernels on the CPU and tests/test_recommend_gpu.py
// compares bit for bit).  A logical query is P positive and N negative EXAMPLES, each a stored row as crh_index_gather_vectors
// returns it; the slots of one query are [P positives | N negatives], of which the first n_pos / n_neg of each part are live.
//
// crh_recommend_query ("average"): q[i] = (ap + ap) - an, ap = sp / (float)n_pos, an = sn / (float)n_neg, sp / sn = +0.0f plus
// the live examples' elements in ascending slot order; with n_neg = 0, q[i] = ap.  Every operation rounded to f32 separately.
//
// crh_recommend_select ("best"): per logical query P lists of c entries (the exact top-c of each positive), the candidates'
// stored vectors and the raw examples.  s(e, x) is what crh_search scores row x with for the raw query e: cosine_preprocess(e)
// in k_prep_queries' sequential arithmetic (rounded to bf16 for a bf16 store), then the canonical dot (orc_dot).  Per distinct
// row (the first flat entry represents it): p = max over the live positives (best = the lowest slot that attains it), n = max
// over the live negatives (-inf without one); KEPT iff the row is no example row and ord(p) > ord(n).  Output: the first k kept
// rows by descending p, ties to the lower row.  T = the largest last score over the lists whose c entries are all real; the
// kept rows with ord(p) > ord(T) are SETTLED (all of them when no list is full): they are a prefix of the exact answer.
// Method AVERAGE takes ONE list per query (the search for the average query): it drops the example rows and keeps the list's
// own order, nothing else.
//
// One workgroup per logical query, one thread per flat entry (the block is the entry count rounded up to whole waves).  One LDS
// object: the prepared examples (at most 16 x (1536 + 4) f32: the 4 floats of padding put the rows of 16 lanes on different
// banks while one lane per example runs the ordered chain of its squared length), the staged rows (8 KB) and keys (4 KB).
// Sweep 1 finds every row's representative; the representatives read their stored row ONCE, 32 floats at a time, and carry up to
// 16 independent canonical chains in registers against 16-byte LDS reads whose address is the same in every lane; sweep 2 counts
// the kept representatives that precede each one (its output slot), as k_fuse_select does.  No global atomics, no scratch.
#include <cmath>

#include "crh_common.h"

namespace crh {
namespace {

constexpr int kRecMaxThreads = CRH_MAX_K;                  // 1024: one thread per entry
constexpr int kRecMaxEx = CRH_MAX_POS + CRH_MAX_NEG;       // 16
constexpr int kRecMaxDim = 1536;
constexpr int kRecPad = 4;                                 // floats between two examples in LDS
constexpr int kRecChunk = 64;                              // logical queries per launch: their live counts travel in the arguments
static_assert(kRecMaxThreads == 1024 && kRecMaxEx == 16, "k_recommend_select sizes its LDS and its chains for 1024 entries and 16 examples");

struct RecCounts {                                         // by value in the kernel arguments: byte q = n_pos | n_neg << 4
    uint32_t w[kRecChunk / 4];
};

struct __attribute__((aligned(16))) RecStage {
    float ex[kRecMaxEx * (kRecMaxDim + kRecPad)];          // the live examples, prepared: positives first, then the negatives
    int64_t row[kRecMaxThreads];                           // sweep 1: row of a real entry, -1 otherwise; sweep 2: -1 for a non-representative
    uint32_t key[kRecMaxThreads];                          // sweep 2: ord(p) of a kept representative, 0 otherwise
    float dv[kRecMaxEx];                                   // cosine_divisor of every example
};

__device__ __forceinline__ uint32_t rec_ord(float f)       // monotone f32 -> u32 (as ord_f32 of crh_kernels.hpp)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ uint32_t rec_unord_bits(uint32_t o) { return (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o; }

__device__ __forceinline__ float rec_bf16_round(float x)   // f32_to_bf16_bits / bf16_bits_f32 of crh_kernels.hpp
{
    uint32_t u = __float_as_uint(x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return __uint_as_float(((u | 0x00400000u) >> 16) << 16);
    return __uint_as_float(((u + 0x7fffu + ((u >> 16) & 1u)) >> 16) << 16);
}

__device__ __forceinline__ float rec_cosine_divisor(float len2)   // cosine_divisor of crh_kernels.hpp: 0 = leave the vector as it is
{
    if (len2 < 1.1920928955078125e-07f || fabsf(len2 - 1.0f) <= 1.0e-6f) return 0.0f;
    return __fsqrt_rn(len2);
}

// the counts byte of query q of the chunk without indexing the argument block dynamically (a dynamic index would move it to scratch)
__device__ __forceinline__ uint32_t rec_counts(const RecCounts &ct, int q)
{
    uint32_t w = ct.w[0];
#pragma unroll
    for (int i = 1; i < kRecChunk / 4; ++i) w = (q >> 2) == i ? ct.w[i] : w;
    return (w >> ((q & 3) * 8)) & 0xffu;
}

// ------------------------------------------------------------------ the average query
__global__ __launch_bounds__(256) void k_recommend_query(int P, int N, int dim, RecCounts ct, const float *__restrict__ examples,
                                                         float *__restrict__ out)
{
    const int q = blockIdx.x;
    const uint32_t cb = rec_counts(ct, q);
    const int np = (int)(cb & 15u), nn = (int)(cb >> 4);
    const float *ex = examples + (size_t)q * (P + N) * dim;
    const float fp = (float)np, fn = (float)nn;
    for (int i = threadIdx.x; i < dim; i += 256) {
        float sp = 0.0f, sn = 0.0f;
        for (int j = 0; j < np; ++j) sp = sp + ex[(size_t)j * dim + i];
        for (int j = 0; j < nn; ++j) sn = sn + ex[(size_t)(P + j) * dim + i];
        const float ap = __fdiv_rn(sp, fp);
        float v = ap;
        if (nn > 0) {
            const float an = __fdiv_rn(sn, fn);
            const float twice = ap + ap;
            v = twice - an;
        }
        out[(size_t)q * dim + i] = v;
    }
}

// ------------------------------------------------------------------ the selection
__global__ __launch_bounds__(kRecMaxThreads) void k_recommend_select(int P, int N, int c, int k, int dim, int method, int round_bf16, RecCounts ct,
                                                                     const uint32_t *__restrict__ score_bits, const int64_t *__restrict__ rows,
                                                                     const float *__restrict__ cand_vecs, const float *__restrict__ examples,
                                                                     const int64_t *__restrict__ example_rows, int64_t *__restrict__ out_rows,
                                                                     uint32_t *__restrict__ out_score_bits, uint32_t *__restrict__ out_neg_bits,
                                                                     int32_t *__restrict__ out_best, int32_t *__restrict__ out_info)
{
    __shared__ RecStage st;
    const int q = blockIdx.x, tid = threadIdx.x, npad = blockDim.x;   // npad >= m * c is a multiple of 64
    const bool best_method = method == CRH_RECOMMEND_BEST;
    const int m = best_method ? P : 1, n = m * c, E = P + N;
    const uint32_t cb = rec_counts(ct, q);
    const int np = (int)(cb & 15u), nn = (int)(cb >> 4), ne = np + nn;
    const size_t base = (size_t)q * n, obase = (size_t)q * k;
    const int stride = dim + kRecPad;

    int64_t row = -1;
    uint32_t sbits = 0xff800000u;            // -inf
    if (tid < n) {
        row = rows[base + tid];
        if (row >= 0) sbits = score_bits[base + tid];
        else row = -1;
    }
    const bool real = row >= 0;
    st.row[tid] = row;
    if (best_method) {
        // the live examples, raw: LDS slot j < np is positive j, slot np + j is negative j
        const float *ex = examples + (size_t)q * E * dim;
        const int d4 = dim >> 2;
        for (int t = tid; t < ne * d4; t += npad) {
            const int j = t / d4, i4 = t - j * d4;
            const int slot = j < np ? j : P + (j - np);
            *reinterpret_cast<float4 *>(&st.ex[j * stride + 4 * i4]) = reinterpret_cast<const float4 *>(ex + (size_t)slot * dim)[i4];
        }
    }
    __syncthreads();
    if (best_method && tid < ne) {
        float acc = 0.0f;                    // index order, product and sum rounded separately (oracle: orc_cosine_preprocess)
        const float4 *e4 = reinterpret_cast<const float4 *>(&st.ex[tid * stride]);
#pragma unroll 4
        for (int i = 0; i < (dim >> 2); ++i) {
            const float4 v = e4[i];
            float p;
            p = v.x * v.x;
            acc = acc + p;
            p = v.y * v.y;
            acc = acc + p;
            p = v.z * v.z;
            acc = acc + p;
            p = v.w * v.w;
            acc = acc + p;
        }
        st.dv[tid] = rec_cosine_divisor(acc);
    }

    // sweep 1: the first entry that names this thread's row represents it
    int first = npad;
    bool is_example = false;
    {
        const longlong2 *r2 = reinterpret_cast<const longlong2 *>(st.row);
        for (int u2 = 0; u2 < npad / 2; ++u2) {
            const longlong2 r = r2[u2];
            first = real && r.x == row && 2 * u2 < first ? 2 * u2 : first;
            first = real && r.y == row && 2 * u2 + 1 < first ? 2 * u2 + 1 : first;
        }
        const int64_t *er = example_rows + (size_t)q * E;
        for (int j = 0; j < E; ++j) is_example = is_example || (real && er[j] == row);
    }
    const bool rep = real && first == tid;
    __syncthreads();                         // the divisors are there; every thread is done reading the rows of sweep 1
    if (best_method) {
        for (int t = tid; t < ne * dim; t += npad) {
            const int j = t / dim, i = t - j * dim;
            const float dv = st.dv[j];
            float x = st.ex[j * stride + i];
            if (dv != 0.0f) x = __fdiv_rn(x, dv);
            st.ex[j * stride + i] = round_bf16 ? rec_bf16_round(x) : x;
        }
    }
    if (!rep) st.row[tid] = -1;
    __syncthreads();

    // T: the largest last score over the full lists (0 = no list is full: everything kept is settled)
    uint32_t t_ord = 0u;
    if (best_method) {
        for (int j = 0; j < m; ++j) {
            const size_t last = base + (size_t)j * c + (c - 1);
            if (rows[last] >= 0) {
                const uint32_t o = rec_ord(__uint_as_float(score_bits[last]));
                t_ord = o > t_ord ? o : t_ord;
            }
        }
    }

    // the canonical chains of a representative against every live example: acc_j = acc_j + e_j[i] * x[i], i ascending
    uint32_t p_ord = 0u, n_ord = rec_ord(-INFINITY);
    int best = -1;
    if (best_method && rep) {
        float acc[kRecMaxEx];
#pragma unroll
        for (int j = 0; j < kRecMaxEx; ++j) acc[j] = 0.0f;
        const float4 *xr = reinterpret_cast<const float4 *>(cand_vecs + (base + tid) * (size_t)dim);
        for (int c0 = 0; c0 < (dim >> 2); c0 += 8) {
            float4 v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = xr[c0 + i];
#pragma unroll
            for (int j = 0; j < kRecMaxEx; ++j) {
                if (j < ne) {                // (the same in every lane)
                    const float4 *e4 = reinterpret_cast<const float4 *>(&st.ex[j * stride]) + c0;
                    float a = acc[j];
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const float4 e = e4[i];
                        float p;
                        p = e.x * v[i].x;
                        a = a + p;
                        p = e.y * v[i].y;
                        a = a + p;
                        p = e.z * v[i].z;
                        a = a + p;
                        p = e.w * v[i].w;
                        a = a + p;
                    }
                    acc[j] = a;
                }
            }
        }
        p_ord = 0u;
#pragma unroll
        for (int j = 0; j < kRecMaxEx; ++j) {
            // (a NaN score is no score, DESIGN.md 3.25 -- the example holds a NaN or an infinity; the candidates come out of a
            // search and hold none: that example counts as -inf, it neither wins a row nor vetoes one)
            const uint32_t o = rec_ord(acc[j] == acc[j] ? acc[j] : -INFINITY);
            if (j < np) {
                if (o > p_ord) {
                    p_ord = o;
                    best = j;
                }
            } else if (j < ne) {
                n_ord = o > n_ord ? o : n_ord;
            }
        }
    }
    // AVERAGE keeps the list's own order (the search's: -0.0 and +0.0 are one value to it): the key is the position
    const bool kept = rep && !is_example && (!best_method || p_ord > n_ord);
    const uint32_t skey = best_method ? p_ord : 0xffffffffu - (uint32_t)tid;
    st.key[tid] = kept ? skey : 0u;          // (a kept row's image is above that of -inf, a position's key above 0: never 0)
    __syncthreads();

    // sweep 2: the kept representatives that precede this one in the output order
    int rank = 0, distinct = 0, nkept = 0, settled = 0;
    {
        const longlong2 *r2 = reinterpret_cast<const longlong2 *>(st.row);
        const uint4 *k4 = reinterpret_cast<const uint4 *>(st.key);
        for (int u4 = 0; u4 < npad / 4; ++u4) {
            const longlong2 ra = r2[2 * u4], rb = r2[2 * u4 + 1];
            const uint4 kv = k4[u4];
            const int64_t er[4] = {ra.x, ra.y, rb.x, rb.y};
            const uint32_t ek[4] = {kv.x, kv.y, kv.z, kv.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool other = ek[e] != 0u;
                distinct += (int)(er[e] >= 0);
                nkept += (int)other;
                settled += (int)(other && ek[e] > t_ord);
                rank += (int)(other && (ek[e] > skey || (ek[e] == skey && er[e] < row)));
            }
        }
    }
    if (kept && rank < k) {
        out_rows[obase + rank] = row;
        out_score_bits[obase + rank] = best_method ? rec_unord_bits(p_ord) : sbits;
        out_neg_bits[obase + rank] = rec_unord_bits(n_ord);
        out_best[obase + rank] = best;
    }
    // the slots behind the kept rows: the padding record -- every output slot is written, no caller clears the outputs
    for (int s = (nkept < k ? nkept : k) + tid; s < k; s += npad) {
        out_rows[obase + s] = -1;
        out_score_bits[obase + s] = 0xff800000u;   // -inf
        out_neg_bits[obase + s] = 0xff800000u;
        out_best[obase + s] = -1;
    }
    if (tid == 0) {
        int32_t *info = out_info + 4 * (size_t)q;
        info[0] = nkept;
        info[1] = settled;
        info[2] = distinct;
        info[3] = distinct - nkept;
    }
}

// checked live counts of a chunk of queries, packed for the kernel arguments
int pack_counts(const char *who, int q0, int nchunk, int P, int N, const int32_t *n_pos_host, const int32_t *n_neg_host, RecCounts *ct)
{
    for (int i = 0; i < kRecChunk / 4; ++i) ct->w[i] = 0u;
    for (int i = 0; i < nchunk; ++i) {
        const int np = n_pos_host ? n_pos_host[q0 + i] : P, nn = n_neg_host ? n_neg_host[q0 + i] : N;
        if (np < 1 || np > P || nn < 0 || nn > N)
            return fail(CRH_E_INVALID, "%s: query %d has n_pos=%d n_neg=%d (1 <= n_pos <= P = %d, 0 <= n_neg <= N = %d)", who, q0 + i, np, nn, P, N);
        ct->w[i >> 2] |= (uint32_t)(np | (nn << 4)) << ((i & 3) * 8);
    }
    return CRH_OK;
}

int check_shape(const char *who, int nq, int P, int N, int dim)
{
    if (nq < 0 || P < 1 || P > CRH_MAX_POS || N < 0 || N > CRH_MAX_NEG)
        return fail(CRH_E_INVALID, "%s: nq=%d P=%d N=%d (nq >= 0, 1 <= P <= %d, 0 <= N <= %d)", who, nq, P, N, CRH_MAX_POS, CRH_MAX_NEG);
    if (dim != 384 && dim != 768 && dim != 1024 && dim != 1536) return fail(CRH_E_INVALID, "%s: dim %d is not one of 384 / 768 / 1024 / 1536", who, dim);
    return CRH_OK;
}

}  // namespace
}  // namespace crh

using namespace crh;

extern "C" {

int crh_recommend_query(int nq, int P, int N, int dim, const float *examples_dev, const int32_t *n_pos_host, const int32_t *n_neg_host,
                        float *out_queries_dev, void *stream)
{
    CRH_TRY(check_shape("recommend_query", nq, P, N, dim));
    RecCounts ct;
    for (int q0 = 0; q0 < nq; q0 += kRecChunk)   // every count is checked before anything is launched
        CRH_TRY(pack_counts("recommend_query", q0, nq - q0 < kRecChunk ? nq - q0 : kRecChunk, P, N, n_pos_host, n_neg_host, &ct));
    if (nq == 0) return CRH_OK;
    if (!examples_dev || !out_queries_dev) return fail(CRH_E_INVALID, "recommend_query: NULL pointer");
    for (int q0 = 0; q0 < nq; q0 += kRecChunk) {
        const int nchunk = nq - q0 < kRecChunk ? nq - q0 : kRecChunk;
        CRH_TRY(pack_counts("recommend_query", q0, nchunk, P, N, n_pos_host, n_neg_host, &ct));
        hipLaunchKernelGGL(k_recommend_query, dim3((unsigned)nchunk), dim3(256), 0, static_cast<hipStream_t>(stream), P, N, dim, ct,
                           examples_dev + (size_t)q0 * (P + N) * dim, out_queries_dev + (size_t)q0 * dim);
        CRH_HIP(hipGetLastError());
    }
    return CRH_OK;
}

int crh_recommend_select(int nq, int P, int N, int c, int k, int dim, int method, int round_bf16, const float *scores_dev,
                         const int64_t *rows_dev, const float *cand_vecs_dev, const float *examples_dev, const int64_t *example_rows_dev,
                         const int32_t *n_pos_host, const int32_t *n_neg_host, int64_t *out_rows_dev, float *out_score_dev,
                         float *out_neg_dev, int32_t *out_best_dev, int32_t *out_info_dev, void *stream)
{
    CRH_TRY(check_shape("recommend_select", nq, P, N, dim));
    if (method != CRH_RECOMMEND_AVERAGE && method != CRH_RECOMMEND_BEST)
        return fail(CRH_E_INVALID, "recommend_select: method=%d is neither AVERAGE (0) nor BEST (1)", method);
    const int m = method == CRH_RECOMMEND_BEST ? P : 1;
    if (c < 1 || c > CRH_MAX_K || m * c > CRH_MAX_K || k < 1 || k > m * c)
        return fail(CRH_E_INVALID, "recommend_select: lists=%d c=%d k=%d (c >= 1, lists * c <= %d, 1 <= k <= lists * c)", m, c, k, CRH_MAX_K);
    if (round_bf16 != 0 && round_bf16 != 1) return fail(CRH_E_INVALID, "recommend_select: round_bf16=%d is neither 0 nor 1", round_bf16);
    RecCounts ct;
    for (int q0 = 0; q0 < nq; q0 += kRecChunk)   // every count is checked before anything is launched
        CRH_TRY(pack_counts("recommend_select", q0, nq - q0 < kRecChunk ? nq - q0 : kRecChunk, P, N, n_pos_host, n_neg_host, &ct));
    if (nq == 0) return CRH_OK;
    if (!scores_dev || !rows_dev || !example_rows_dev || !out_rows_dev || !out_score_dev || !out_neg_dev || !out_best_dev || !out_info_dev)
        return fail(CRH_E_INVALID, "recommend_select: NULL pointer");
    if (method == CRH_RECOMMEND_BEST) {
        if (!cand_vecs_dev || !examples_dev) return fail(CRH_E_INVALID, "recommend_select: NULL pointer");
        if (((reinterpret_cast<uintptr_t>(cand_vecs_dev) | reinterpret_cast<uintptr_t>(examples_dev)) & 15u) != 0)
            return fail(CRH_E_INVALID, "recommend_select: the vectors must be 16-byte aligned");
    }
    const int n = m * c, threads = (n + 63) / 64 * 64, E = P + N;
    for (int q0 = 0; q0 < nq; q0 += kRecChunk) {
        const int nchunk = nq - q0 < kRecChunk ? nq - q0 : kRecChunk;
        CRH_TRY(pack_counts("recommend_select", q0, nchunk, P, N, n_pos_host, n_neg_host, &ct));
        hipLaunchKernelGGL(k_recommend_select, dim3((unsigned)nchunk), dim3((unsigned)threads), 0, static_cast<hipStream_t>(stream), P, N, c, k, dim,
                           method, round_bf16, ct, reinterpret_cast<const uint32_t *>(scores_dev) + (size_t)q0 * n, rows_dev + (size_t)q0 * n,
                           cand_vecs_dev ? cand_vecs_dev + (size_t)q0 * n * dim : nullptr, examples_dev ? examples_dev + (size_t)q0 * E * dim : nullptr,
                           example_rows_dev + (size_t)q0 * E, out_rows_dev + (size_t)q0 * k, reinterpret_cast<uint32_t *>(out_score_dev) + (size_t)q0 * k,
                           reinterpret_cast<uint32_t *>(out_neg_dev) + (size_t)q0 * k, out_best_dev + (size_t)q0 * k, out_info_dev + (size_t)q0 * 4);
        CRH_HIP(hipGetLastError());
    }
    return CRH_OK;
}

}  // extern "C"
