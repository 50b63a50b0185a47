// crh_group.hip -- exact per-group cap (group_by / group_size) over candidate lists left on the device.
//
// The reference caps results per file after the fetch (ResultReranker.deduplicate(max_per_file=3), query/reranker.py:122-145) and
// comes back short when one file owns the list; Qdrant's query_points_groups is "best effort".  The definition below is THIS
// repository's ("Per-group cap"; tests/group_cases.py restates it on the CPU and tests/test_grouped_gpu.py compares
// bit for bit).
//
// Per query: a candidate list of c entries as crh_search / crh_merge_topk* return it (padding rows < 0 at the end) and the code
// of every candidate in the group_by column (crh_index_gather_codes).  A candidate's rank in its group = the number of EARLIER
// real candidates with the same code; it is kept iff it is real and (code < 0 or rank < group_size).  The kept candidates are
// written in list order, the first k of them.
//
// One workgroup per query, one thread per candidate (the block is c rounded up to whole waves).  The codes are staged in LDS
// with validity folded in (padding is stored as -1, which never counts): 4 KB at most.  Every thread counts the earlier equal
// codes of its own candidate with 16-byte LDS reads whose address is the same in every lane (broadcast reads, no bank
// conflict); the bound of that loop is the wave's last position, so wave w reads 64 * (w + 1) codes.  The keep flags are
// compacted in list order with one ballot + mbcnt per wave and the waves' totals in LDS.  No global atomics, no scratch, every
// store an ordinary vector store.
#include <cmath>

#include "crh_common.h"

namespace crh {
namespace {

constexpr int kGroupMaxThreads = CRH_MAX_K;   // 1024: one thread per candidate
static_assert(kGroupMaxThreads == 1024, "k_group_select sizes its LDS and its wave totals for 1024 candidates");

__global__ __launch_bounds__(kGroupMaxThreads) void k_group_select(int c, int k, int group_size, const uint32_t *__restrict__ score_bits,
                                                                   const int64_t *__restrict__ rows, const int32_t *__restrict__ codes,
                                                                   int32_t *__restrict__ out_pos, int64_t *__restrict__ out_rows,
                                                                   uint32_t *__restrict__ out_score_bits, int32_t *__restrict__ out_codes,
                                                                   int32_t *__restrict__ out_info)
{
    __shared__ __attribute__((aligned(16))) int32_t lcode[kGroupMaxThreads];   // code of a real candidate, -1 for padding / beyond c
    __shared__ int wkept[kGroupMaxThreads / 64], wreal[kGroupMaxThreads / 64];
    const int q = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, nwaves = blockDim.x >> 6;
    const size_t base = (size_t)q * c, obase = (size_t)q * k;
    int64_t row = -1;
    int32_t code = -1;
    if (tid < c) {
        row = rows[base + tid];
        if (row >= 0) code = codes[base + tid];
    }
    const bool real = row >= 0;
    lcode[tid] = code;                 // (blockDim.x >= c is a multiple of 64: every slot a wave reads below is written)
    __syncthreads();
    int rank = 0;
    const int4 *l4 = reinterpret_cast<const int4 *>(lcode);
    for (int j4 = 0; j4 < (wave + 1) * 16; ++j4) {      // positions 0 .. 64 * (wave + 1) - 1, four per read; same address in every lane
        const int4 v = l4[j4];
        const int j = j4 * 4;
        rank += (int)(v.x == code && j < tid) + (int)(v.y == code && j + 1 < tid) + (int)(v.z == code && j + 2 < tid) + (int)(v.w == code && j + 3 < tid);
    }
    const bool keep = real && (code < 0 || rank < group_size);
    const unsigned long long km = __ballot(keep), rm = __ballot(real);
    const int pre = (int)__builtin_amdgcn_mbcnt_hi((unsigned int)(km >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)km, 0u));
    if ((tid & 63) == 0) {
        wkept[wave] = __popcll(km);
        wreal[wave] = __popcll(rm);
    }
    __syncthreads();
    int before = 0, kept = 0, nreal = 0;
    for (int w = 0; w < nwaves; ++w) {
        const int n = wkept[w];
        before += w < wave ? n : 0;
        kept += n;
        nreal += wreal[w];
    }
    const int at = before + pre;
    if (keep && at < k) {
        out_pos[obase + at] = tid;
        out_rows[obase + at] = row;
        out_score_bits[obase + at] = score_bits[base + tid];
        out_codes[obase + at] = code;
    }
    // the slots behind the kept candidates: the padding record -- every output slot is written, no caller clears the outputs
    for (int s = (kept < k ? kept : k) + tid; s < k; s += blockDim.x) {
        out_pos[obase + s] = -1;
        out_rows[obase + s] = -1;
        out_score_bits[obase + s] = 0xff800000u;   // -inf
        out_codes[obase + s] = -1;
    }
    if (tid == 0) {
        out_info[2 * (size_t)q] = kept;
        out_info[2 * (size_t)q + 1] = nreal;
    }
}

}  // namespace
}  // namespace crh

using namespace crh;

extern "C" {

int crh_group_select(int nq, int c, int k, int group_size, const float *scores_dev, const int64_t *rows_dev, const int32_t *codes_dev,
                     int32_t *out_pos_dev, int64_t *out_rows_dev, float *out_scores_dev, int32_t *out_codes_dev, int32_t *out_info_dev, void *stream)
{
    if (nq < 0 || k < 1 || k > c || c > CRH_MAX_K) return fail(CRH_E_INVALID, "group_select: nq=%d c=%d k=%d (1 <= k <= c <= %d)", nq, c, k, CRH_MAX_K);
    if (group_size < 1) return fail(CRH_E_INVALID, "group_select: group_size=%d must be >= 1", group_size);
    if (nq == 0) return CRH_OK;
    if (!scores_dev || !rows_dev || !codes_dev || !out_pos_dev || !out_rows_dev || !out_scores_dev || !out_codes_dev || !out_info_dev)
        return fail(CRH_E_INVALID, "group_select: NULL pointer");
    const int threads = (c + 63) / 64 * 64;
    hipLaunchKernelGGL(k_group_select, dim3((unsigned)nq), dim3((unsigned)threads), 0, static_cast<hipStream_t>(stream), c, k, group_size,
                       reinterpret_cast<const uint32_t *>(scores_dev), rows_dev, codes_dev, out_pos_dev, out_rows_dev,
                       reinterpret_cast<uint32_t *>(out_scores_dev), out_codes_dev, out_info_dev);
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

}  // extern "C"
