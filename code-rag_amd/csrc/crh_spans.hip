// crh_spans.hip -- overlap-free hit lists: the walk that drops a candidate whose lines a better hit already covers.
//
// The chunker emits an entity for a class and one for each of its methods, and splits long entities into parts that share
// trailing lines, so a good query returns the same lines two or three times.  The reference has no answer to that, and a cap
// per file (crh_group.hip) cannot tell a nested chunk from an unrelated one.  The definition below is THIS repository's
// (tests/span_cases.py restates it on the CPU and tests/test_spans_gpu.py compares bit for bit).
//
// Per query: a candidate list of c entries as crh_search / crh_merge_topk* return it (padding rows < 0 at the end) and, per
// candidate, the code of its file and its first and last line (crh_index_gather_codes over buffers pre-filled with -1).  A real
// candidate HAS A SPAN iff file >= 0, lo >= 0 and hi >= lo.  In list order: padding is skipped; a candidate without a span is
// kept; a candidate i with a span is dropped iff an earlier KEPT candidate j with a span and the same file shares ov > 0 lines
// with it and ov * 1000 > permille * min(len_i, len_j) -- 64-bit integers, nothing rounded.  The first k kept are written.
//
// One workgroup of ONE wave per query: the walk is sequential in the candidate (whether i is kept depends on which earlier
// ones were), so more waves would only add a barrier per candidate.  The list is read 64 candidates at a time, one per lane;
// the candidates without a span are settled by a ballot, the others taken one after the other: their (file, lo, hi) are read
// from the owning lane (v_readlane) and tested against the kept spans in LDS (3 x 4 KB at c = 1024), entry t by lane t % 64, the
// verdicts joined by a ballot after every 64 entries.  A kept span is appended to LDS by one lane; the workgroup barrier that
// orders that write before the next candidate's reads is a single-wave one.  The chunk's keep flags are a wave-uniform 64-bit
// mask: every lane counts the flags below its own and writes its candidate's record with ordinary vector stores.  No atomics,
// no scratch, no dependence on the order lanes arrive in.
#include "crh_common.h"

namespace crh {
namespace {

constexpr int kSpanMax = CRH_MAX_K;   // kept spans of one list
static_assert(kSpanMax == 1024, "k_span_select sizes its LDS for 1024 candidates");

__global__ __launch_bounds__(64) void k_span_select(int c, int k, int permille, const uint32_t *__restrict__ score_bits,
                                                    const int64_t *__restrict__ rows, const int32_t *__restrict__ files,
                                                    const int32_t *__restrict__ los, const int32_t *__restrict__ his,
                                                    int32_t *__restrict__ out_pos, int64_t *__restrict__ out_rows,
                                                    uint32_t *__restrict__ out_score_bits, int32_t *__restrict__ out_file,
                                                    int32_t *__restrict__ out_lo, int32_t *__restrict__ out_hi, int32_t *__restrict__ out_info)
{
    __shared__ int32_t kfile[kSpanMax], klo[kSpanMax], khi[kSpanMax];   // the kept candidates that have a span, in list order
    const int q = blockIdx.x, lane = threadIdx.x;
    const size_t base = (size_t)q * c, obase = (size_t)q * k;
    const unsigned long long below = (1ull << lane) - 1ull;
    int nspan = 0, nkept = 0, nreal = 0;                                 // wave-uniform
    for (int c0 = 0; c0 < c; c0 += 64) {
        const int i = c0 + lane;
        int64_t row = -1;
        int32_t file = -1, lo = -1, hi = -1;
        uint32_t sb = 0;
        if (i < c) {
            row = rows[base + i];
            if (row >= 0) {
                file = files[base + i];
                lo = los[base + i];
                hi = his[base + i];
                sb = score_bits[base + i];
            }
        }
        const bool real = row >= 0, span = real && file >= 0 && lo >= 0 && hi >= lo;
        const unsigned long long realmask = __ballot(real), spanmask = __ballot(span);
        unsigned long long keepmask = realmask & ~spanmask;              // no span: kept as it is
        for (unsigned long long m = spanmask; m; m &= m - 1) {
            const int j = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
            const int32_t fj = __builtin_amdgcn_readlane(file, j), lj = __builtin_amdgcn_readlane(lo, j), hj = __builtin_amdgcn_readlane(hi, j);
            const int64_t lenj = (int64_t)hj - lj + 1;
            bool redundant = false;
            for (int t0 = 0; t0 < nspan && !redundant; t0 += 64) {
                const int t = t0 + lane;
                bool hit = false;
                if (t < nspan && kfile[t] == fj) {
                    const int32_t l = klo[t], h = khi[t];
                    const int64_t ov = (int64_t)(h < hj ? h : hj) - (int64_t)(l > lj ? l : lj) + 1;
                    const int64_t len = (int64_t)h - l + 1;
                    hit = ov > 0 && ov * 1000 > (int64_t)permille * (len < lenj ? len : lenj);
                }
                redundant = __ballot(hit) != 0ull;
            }
            if (!redundant) {                                           // (uniform: nspan < kSpanMax since at most c <= 1024 are ever kept)
                if (lane == 0) {
                    kfile[nspan] = fj;
                    klo[nspan] = lj;
                    khi[nspan] = hj;
                }
                ++nspan;
                keepmask |= 1ull << j;
                __syncthreads();                                        // one wave: orders the append before the next candidate's reads
            }
        }
        const int at = nkept + __popcll(keepmask & below);
        if (((keepmask >> lane) & 1ull) && at < k) {
            out_pos[obase + at] = i;
            out_rows[obase + at] = row;
            out_score_bits[obase + at] = sb;
            out_file[obase + at] = file;
            out_lo[obase + at] = lo;
            out_hi[obase + at] = hi;
        }
        nkept += __popcll(keepmask);
        nreal += __popcll(realmask);
    }
    // the slots behind the kept candidates: the padding record -- every output slot is written, no caller clears the outputs
    for (int s = (nkept < k ? nkept : k) + lane; s < k; s += 64) {
        out_pos[obase + s] = -1;
        out_rows[obase + s] = -1;
        out_score_bits[obase + s] = 0xff800000u;   // -inf
        out_file[obase + s] = -1;
        out_lo[obase + s] = -1;
        out_hi[obase + s] = -1;
    }
    if (lane == 0) {
        out_info[2 * (size_t)q] = nkept;
        out_info[2 * (size_t)q + 1] = nreal;
    }
}

}  // namespace
}  // namespace crh

using namespace crh;

extern "C" {

int crh_span_select(int nq, int c, int k, int max_overlap_permille, const float *scores_dev, const int64_t *rows_dev,
                    const int32_t *file_codes_dev, const int32_t *lo_dev, const int32_t *hi_dev, int32_t *out_pos_dev, int64_t *out_rows_dev,
                    float *out_scores_dev, int32_t *out_file_dev, int32_t *out_lo_dev, int32_t *out_hi_dev, int32_t *out_info_dev, void *stream)
{
    if (nq < 0 || k < 1 || k > c || c > CRH_MAX_K) return fail(CRH_E_INVALID, "span_select: nq=%d c=%d k=%d (1 <= k <= c <= %d)", nq, c, k, CRH_MAX_K);
    if (max_overlap_permille < 0 || max_overlap_permille > 1000)
        return fail(CRH_E_INVALID, "span_select: max_overlap_permille=%d outside 0..1000", max_overlap_permille);
    if (nq == 0) return CRH_OK;
    if (!scores_dev || !rows_dev || !file_codes_dev || !lo_dev || !hi_dev || !out_pos_dev || !out_rows_dev || !out_scores_dev || !out_file_dev ||
        !out_lo_dev || !out_hi_dev || !out_info_dev)
        return fail(CRH_E_INVALID, "span_select: NULL pointer");
    hipLaunchKernelGGL(k_span_select, dim3((unsigned)nq), dim3(64), 0, static_cast<hipStream_t>(stream), c, k, max_overlap_permille,
                       reinterpret_cast<const uint32_t *>(scores_dev), rows_dev, file_codes_dev, lo_dev, hi_dev, out_pos_dev, out_rows_dev,
                       reinterpret_cast<uint32_t *>(out_scores_dev), out_file_dev, out_lo_dev, out_hi_dev, out_info_dev);
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

}  // extern "C"
