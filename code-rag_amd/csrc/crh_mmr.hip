// crh_mmr.hip -- diversity-aware top-k (maximal marginal relevance) selected on the device.
//
// Nothing in the reference does this: it only ever sends query_points(query, limit, filter) (embeddings/client.py:142-148) and
// takes the cosine order as it comes.  Qdrant's query API offers Mmr(diversity, candidates_limit) and the RAG frameworks'
// Qdrant adaptors offer max_marginal_relevance_search -- by description only, not checkable offline: the arithmetic and the
// tie rule below are THIS repository's definition ("Diversity-aware top-k"; tests/mmr_cases.py restates it on
// the CPU with the C oracle's sequential dot, and tests/test_mmr_gpu.py compares bit for bit).
//
// Per query: a candidate list of c entries as crh_search / crh_merge_topk return it, the stored vector of every candidate
// (crh_index_gather_vectors), k <= c picks.
//   rel[i]   = the candidate's score;  sim(i, s) = the canonical dot of the two rows (acc = acc + x_i[e] * x_s[e], e ascending,
//              product and sum rounded separately: orc_dot of oracle/search_oracle.c; this file is compiled with -ffp-contract=off)
//   pick 1   = position 0;  pick t > 1 = the real, not yet picked candidate with the largest
//              obj = (1 - diversity) * rel - diversity * max over picked s of sim(., s)      (three separately rounded f32 operations)
//              ties to the lower position.
// This first version runs the canonical chain for every (candidate, pick) pair: one workgroup per query, the row of the last
// pick in LDS, a thread per candidate walks its own row against it -- c dots per pick, k * c in all (not the c^2 / 2 of a Gram
// matrix).  The nominate-then-decide form (a fast dot in any order, the canonical chain only for objectives within the margin
// of the best) is the follow-up DESIGN.md names.
#include <cmath>

#include "crh_common.h"

namespace crh {
namespace {

constexpr int kMmrThreads = 256;
constexpr int kMmrMaxDim = 1536;

__device__ __forceinline__ uint32_t mmr_ord(float f)   // monotone f32 -> u32 (as ord_f32 of crh_kernels.hpp)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// sequential f32 dot of one candidate row (global, row-major f32) with the picked row in LDS; dim % 32 == 0
__device__ __forceinline__ float mmr_canonical_dot(const float *__restrict__ x, const float *sv, int dim)
{
    const float4 *xr = reinterpret_cast<const float4 *>(x);
    const float4 *sr = reinterpret_cast<const float4 *>(sv);
    float acc = 0.0f;
    for (int c0 = 0; c0 < (dim >> 2); c0 += 8) {
        float4 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = xr[c0 + j];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float4 s = sr[c0 + j];
            float p;
            p = v[j].x * s.x;
            acc = acc + p;
            p = v[j].y * s.y;
            acc = acc + p;
            p = v[j].z * s.z;
            acc = acc + p;
            p = v[j].w * s.w;
            acc = acc + p;
        }
    }
    return acc;
}

// one workgroup per query
__global__ __launch_bounds__(kMmrThreads) void k_mmr_select(int c, int k, int dim, const float *__restrict__ scores, const int64_t *__restrict__ rows,
                                                            const float *__restrict__ vecs, float diversity, int32_t *__restrict__ out_pos,
                                                            int64_t *__restrict__ out_rows, float *__restrict__ out_scores, float *__restrict__ out_obj)
{
    __shared__ __attribute__((aligned(16))) float sv[kMmrMaxDim];   // the row of the last pick
    __shared__ float rel[CRH_MAX_K], pen[CRH_MAX_K], objv[CRH_MAX_K];
    __shared__ uint8_t avail[CRH_MAX_K];                            // real and not yet picked
    __shared__ unsigned long long wbest[kMmrThreads / 64];
    const int q = blockIdx.x, tid = threadIdx.x;
    const size_t base = (size_t)q * c, obase = (size_t)q * k;
    for (int i = tid; i < c; i += kMmrThreads) {
        rel[i] = scores[base + i];
        pen[i] = -INFINITY;
        avail[i] = rows[base + i] >= 0;
    }
    __syncthreads();
    const float lam = 1.0f - diversity;
    // pick 1 is position 0 (a list whose first entry is padding is an empty list: padding sits at the end)
    int pick = avail[0] ? 0 : -1;
    float pobj = lam * rel[0];
    int t = 0;
    while (pick >= 0) {
        if (tid == 0) {
            out_pos[obase + t] = pick;
            out_rows[obase + t] = rows[base + pick];
            out_scores[obase + t] = rel[pick];
            out_obj[obase + t] = pobj;
            avail[pick] = 0;
        }
        if (++t == k) break;
        const float4 *src = reinterpret_cast<const float4 *>(vecs + (base + pick) * (size_t)dim);
        for (int e = tid; e < (dim >> 2); e += kMmrThreads) reinterpret_cast<float4 *>(sv)[e] = src[e];
        __syncthreads();
        unsigned long long best = 0ull;   // (no candidate's key is 0: its low word is 0xffffffff - position > 0)
        for (int i = tid; i < c; i += kMmrThreads) {
            if (!avail[i]) continue;
            const float sim = mmr_canonical_dot(vecs + (base + i) * (size_t)dim, sv, dim);
            const float p = sim > pen[i] ? sim : pen[i];
            pen[i] = p;
            const float a = lam * rel[i];
            const float b = diversity * p;
            const float o = a - b;
            objv[i] = o;
            // larger objective first, then the lower position; -0 and +0 are one value, as they are to a comparison of floats
            const unsigned long long key = ((unsigned long long)mmr_ord(o == 0.0f ? 0.0f : o) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)i);
            best = key > best ? key : best;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long other = __shfl_xor(best, off, 64);
            best = other > best ? other : best;
        }
        if ((tid & 63) == 0) wbest[tid >> 6] = best;
        __syncthreads();
        best = wbest[0];
#pragma unroll
        for (int w = 1; w < kMmrThreads / 64; ++w) best = wbest[w] > best ? wbest[w] : best;
        pick = best == 0ull ? -1 : (int)(0xffffffffu - (uint32_t)(best & 0xffffffffull));
        pobj = pick >= 0 ? objv[pick] : 0.0f;
        __syncthreads();   // (sv, wbest and avail[pick] are rewritten by the next round)
    }
    // the slots behind the picks: the padding record -- every output slot is written, no caller clears the outputs
    for (int s = t + tid; s < k; s += kMmrThreads) {
        out_pos[obase + s] = -1;
        out_rows[obase + s] = -1;
        out_scores[obase + s] = -INFINITY;
        out_obj[obase + s] = -INFINITY;
    }
}

}  // namespace
}  // namespace crh

using namespace crh;

extern "C" {

int crh_mmr_select(int nq, int c, int k, int dim, const float *scores_dev, const int64_t *rows_dev, const float *vecs_dev, float diversity,
                   int32_t *out_pos_dev, int64_t *out_rows_dev, float *out_scores_dev, float *out_obj_dev, void *stream)
{
    if (nq < 0 || k < 1 || k > c || c > CRH_MAX_K) return fail(CRH_E_INVALID, "mmr: nq=%d c=%d k=%d (1 <= k <= c <= %d)", nq, c, k, CRH_MAX_K);
    if (dim != 384 && dim != 768 && dim != 1024 && dim != 1536) return fail(CRH_E_INVALID, "mmr: dim %d is not one of 384 / 768 / 1024 / 1536", dim);
    if (!(diversity >= 0.0f && diversity <= 1.0f)) return fail(CRH_E_INVALID, "mmr: diversity %g outside [0, 1]", (double)diversity);
    if (nq == 0) return CRH_OK;
    if (!scores_dev || !rows_dev || !vecs_dev || !out_pos_dev || !out_rows_dev || !out_scores_dev || !out_obj_dev)
        return fail(CRH_E_INVALID, "mmr: NULL pointer");
    if ((reinterpret_cast<uintptr_t>(vecs_dev) & 15u) != 0) return fail(CRH_E_INVALID, "mmr: the vectors must be 16-byte aligned");
    hipLaunchKernelGGL(k_mmr_select, dim3((unsigned)nq), dim3(kMmrThreads), 0, static_cast<hipStream_t>(stream), c, k, dim, scores_dev, rows_dev,
                       vecs_dev, diversity, out_pos_dev, out_rows_dev, out_scores_dev, out_obj_dev);
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

}  // extern "C"
