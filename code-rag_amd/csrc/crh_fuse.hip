// crh_fuse.hip -- multi-query fusion (reciprocal-rank fusion / best match) over candidate lists left on the device.
//
// The reference's planner writes reformulations of a question (QueryPlan.sub_queries[].query_text, query/query_planner.py:66-91)
// and its engine searches the original text only (query/engine.py:315-346): with Qdrant every sub-query is one more RPC.  Here one
// corpus pass serves 64 queries, so the m lists of one question are there; what Qdrant offers for the step after them is
// prefetch=[...] + FusionQuery(RRF).  The definition below is THIS repository's (tests/fuse_cases.py restates it
// on the CPU and tests/test_fused_gpu.py compares bit for bit).
//
// Per logical query: m lists of c entries (score f32, row i64) as crh_search / crh_merge_topk* return them (padding rows < 0 at
// the end of a list); entry (j, p) has flat index u = j * c + p.  Its CONTRIBUTION is w_j / (float)(rrf_k + p + 1) (RRF: one
// correctly rounded f32 division) or its score (MAX).  A row's FUSED score is (RRF) +0.0f plus the contributions of its entries
// in ascending u, every addition rounded to f32, or (MAX) the largest contribution; with it go cos (its largest score), lists
// (bit j: list j holds it) and first (its smallest u).  "Largest" and the output order compare the order-preserving integer
// image of f32 (-0.0 < +0.0); the output is the first k distinct rows by descending fused score, ties to the lower row.
//
// One workgroup per logical query, one thread per entry (the block is m * c rounded up to whole waves).  Rows (8 KB),
// contributions (4 KB) and a third array (4 KB: the scores during sweep 1, the representatives' fused keys during sweep 2) are
// one LDS object; padding and the slots beyond m * c are stored as row -1.  Sweep 1: every thread walks ALL staged entries with
// 16-byte LDS reads whose address is the same in every lane (broadcast reads, no bank conflict; the list index of the walk is
// a scalar) and accumulates the fused score, cos and lists of its own row in ascending u; the thread that meets itself first is
// the row's REPRESENTATIVE.  Sweep 2: the representatives stage their fused keys, the others clear their row, and every
// representative counts the representatives that precede it in the output order: that count is its output slot.  No global
// atomics, no scratch, every store an ordinary vector store.
#include <cmath>

#include "crh_common.h"

namespace crh {
namespace {

constexpr int kFuseMaxThreads = CRH_MAX_K;   // 1024: one thread per entry
static_assert(kFuseMaxThreads == 1024, "k_fuse_select sizes its LDS for 1024 entries");

struct FuseWeights {                         // by value in the kernel arguments
    float w[CRH_MAX_LISTS];
};

struct __attribute__((aligned(16))) FuseStage {
    int64_t row[kFuseMaxThreads];            // row of a real entry, -1 for padding / beyond m * c; sweep 2: -1 for a non-representative
    float con[kFuseMaxThreads];              // RRF contribution (0 under MAX, whose fused score is cos)
    uint32_t aux[kFuseMaxThreads];           // sweep 1: score bits; sweep 2: ord image of the representative's fused score
};

__device__ __forceinline__ uint32_t fuse_ord(float f)   // monotone f32 -> u32 (as ord_f32 of crh_kernels.hpp)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the weight of list j without indexing the argument block dynamically (a dynamic index would move it to scratch)
__device__ __forceinline__ float fuse_weight(const FuseWeights &wt, int j)
{
    float w = wt.w[0];
#pragma unroll
    for (int i = 1; i < CRH_MAX_LISTS; ++i) w = j == i ? wt.w[i] : w;
    return w;
}

__global__ __launch_bounds__(kFuseMaxThreads) void k_fuse_select(int m, int c, int k, int method, int rrf_k, FuseWeights wt,
                                                                 const uint32_t *__restrict__ score_bits, const int64_t *__restrict__ rows,
                                                                 int64_t *__restrict__ out_rows, uint32_t *__restrict__ out_fused_bits,
                                                                 uint32_t *__restrict__ out_cos_bits, int32_t *__restrict__ out_lists,
                                                                 int32_t *__restrict__ out_first, int32_t *__restrict__ out_info)
{
    __shared__ FuseStage st;
    const int q = blockIdx.x, tid = threadIdx.x, n = m * c, npad = blockDim.x;   // npad >= n is a multiple of 64
    const size_t base = (size_t)q * n, obase = (size_t)q * k;
    int64_t row = -1;
    uint32_t sbits = 0xff800000u;            // -inf
    float con = 0.0f;
    if (tid < n) {
        row = rows[base + tid];
        if (row >= 0) {
            sbits = score_bits[base + tid];
            const int j = tid / c, p = tid - j * c;
            if (method == CRH_FUSE_RRF) con = fuse_weight(wt, j) / (float)((long long)rrf_k + p + 1);   // (MAX: the score itself, staged below; con stays 0)
        } else {
            row = -1;
        }
    }
    const bool real = row >= 0;
    st.row[tid] = row;
    st.con[tid] = con;
    st.aux[tid] = sbits;
    __syncthreads();

    // sweep 1: this thread's row against every staged entry, ascending u, four entries per step
    float fused = 0.0f;
    uint32_t cos_ord = 0u;                   // below the image of every float
    int lists = 0, first = npad, nreal = 0;
    {
        const longlong2 *r2 = reinterpret_cast<const longlong2 *>(st.row);
        const float4 *c4 = reinterpret_cast<const float4 *>(st.con);
        const uint4 *s4 = reinterpret_cast<const uint4 *>(st.aux);
        int j = 0, p = 0;                    // list and position of entry u (the same in every lane)
        for (int u4 = 0; u4 < npad / 4; ++u4) {
            const longlong2 ra = r2[2 * u4], rb = r2[2 * u4 + 1];
            const float4 cv = c4[u4];
            const uint4 sv = s4[u4];
            const int64_t er[4] = {ra.x, ra.y, rb.x, rb.y};
            const float ec[4] = {cv.x, cv.y, cv.z, cv.w};
            const uint32_t es[4] = {sv.x, sv.y, sv.z, sv.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int u = 4 * u4 + e;
                nreal += (int)(er[e] >= 0);
                const bool hit = real && er[e] == row;
                fused = hit ? fused + ec[e] : fused;
                const uint32_t so = fuse_ord(__uint_as_float(es[e]));
                cos_ord = hit && so > cos_ord ? so : cos_ord;
                lists |= hit ? 1 << (j & 15) : 0;
                first = hit && u < first ? u : first;
                if (++p == c) {
                    p = 0;
                    ++j;                     // (beyond m * c nothing hits: j is not used there)
                }
            }
        }
    }
    const bool rep = real && first == tid;
    const uint32_t cos_bits = (cos_ord & 0x80000000u) ? (cos_ord & 0x7fffffffu) : ~cos_ord;
    const uint32_t fused_bits = method == CRH_FUSE_RRF ? __float_as_uint(fused) : cos_bits;
    const uint32_t key = method == CRH_FUSE_RRF ? fuse_ord(fused) : cos_ord;
    __syncthreads();                         // every thread is done reading the scores and the rows of sweep 1
    st.aux[tid] = key;
    if (!rep) st.row[tid] = -1;
    __syncthreads();

    // sweep 2: the representatives that precede this one in the output order
    int rank = 0, distinct = 0;
    {
        const longlong2 *r2 = reinterpret_cast<const longlong2 *>(st.row);
        const uint4 *k4 = reinterpret_cast<const uint4 *>(st.aux);
        for (int u4 = 0; u4 < npad / 4; ++u4) {
            const longlong2 ra = r2[2 * u4], rb = r2[2 * u4 + 1];
            const uint4 kv = k4[u4];
            const int64_t er[4] = {ra.x, ra.y, rb.x, rb.y};
            const uint32_t ek[4] = {kv.x, kv.y, kv.z, kv.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool other = er[e] >= 0;
                distinct += (int)other;
                rank += (int)(other && (ek[e] > key || (ek[e] == key && er[e] < row)));
            }
        }
    }
    if (rep && rank < k) {
        out_rows[obase + rank] = row;
        out_fused_bits[obase + rank] = fused_bits;
        out_cos_bits[obase + rank] = cos_bits;
        out_lists[obase + rank] = lists;
        out_first[obase + rank] = first;
    }
    // the slots behind the distinct rows: the padding record -- every output slot is written, no caller clears the outputs
    for (int s = (distinct < k ? distinct : k) + tid; s < k; s += npad) {
        out_rows[obase + s] = -1;
        out_fused_bits[obase + s] = 0xff800000u;   // -inf
        out_cos_bits[obase + s] = 0xff800000u;
        out_lists[obase + s] = 0;
        out_first[obase + s] = -1;
    }
    if (tid == 0) {
        out_info[2 * (size_t)q] = distinct;
        out_info[2 * (size_t)q + 1] = nreal;
    }
}

}  // namespace
}  // namespace crh

using namespace crh;

extern "C" {

int crh_fuse_select(int nq, int m, int c, int k, int method, int rrf_k, const float *weights_host, const float *scores_dev,
                    const int64_t *rows_dev, int64_t *out_rows_dev, float *out_fused_dev, float *out_cos_dev, int32_t *out_lists_dev,
                    int32_t *out_first_dev, int32_t *out_info_dev, void *stream)
{
    if (nq < 0 || m < 1 || m > CRH_MAX_LISTS || c < 1 || c > CRH_MAX_K || m * c > CRH_MAX_K || k < 1 || k > m * c)
        return fail(CRH_E_INVALID, "fuse_select: nq=%d m=%d c=%d k=%d (1 <= m <= %d, c >= 1, m * c <= %d, 1 <= k <= m * c)", nq, m, c, k,
                    CRH_MAX_LISTS, CRH_MAX_K);
    if (method != CRH_FUSE_RRF && method != CRH_FUSE_MAX) return fail(CRH_E_INVALID, "fuse_select: method=%d is neither RRF (0) nor MAX (1)", method);
    if (rrf_k < 0) return fail(CRH_E_INVALID, "fuse_select: rrf_k=%d must be >= 0", rrf_k);
    if (weights_host && method == CRH_FUSE_MAX) return fail(CRH_E_INVALID, "fuse_select: weights are meaningless with method MAX");
    FuseWeights wt;
    for (int j = 0; j < CRH_MAX_LISTS; ++j) {
        wt.w[j] = weights_host && j < m ? weights_host[j] : 1.0f;
        if (!std::isfinite(wt.w[j]) || wt.w[j] < 0.0f) return fail(CRH_E_INVALID, "fuse_select: weights[%d] must be finite and >= 0", j);
    }
    if (nq == 0) return CRH_OK;
    if (!scores_dev || !rows_dev || !out_rows_dev || !out_fused_dev || !out_cos_dev || !out_lists_dev || !out_first_dev || !out_info_dev)
        return fail(CRH_E_INVALID, "fuse_select: NULL pointer");
    const int threads = (m * c + 63) / 64 * 64;
    hipLaunchKernelGGL(k_fuse_select, dim3((unsigned)nq), dim3((unsigned)threads), 0, static_cast<hipStream_t>(stream), m, c, k, method, rrf_k, wt,
                       reinterpret_cast<const uint32_t *>(scores_dev), rows_dev, out_rows_dev, reinterpret_cast<uint32_t *>(out_fused_dev),
                       reinterpret_cast<uint32_t *>(out_cos_dev), out_lists_dev, out_first_dev, out_info_dev);
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

}  // extern "C"
