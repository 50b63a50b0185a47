// crh_facet.hip -- the facet list: the exact top-k of a histogram left on the device (crh_facet_select).
//
// Per list: n_bins int64 counts >= 0, bin = dictionary code (crh_index_facet / crh_search_range_facet, summed over shards and
// ranks by the caller).  The FACET LIST is the bins with count > 0 ordered by count descending, ties to the LOWER CODE (the
// value stored first -- Qdrant breaks ties by the value itself), cut at k; the tail is (-1, 0).
//
// One workgroup of 1024 threads per list, three phases:
//   1. t = the k-th largest count, by radix select over 8-bit digits from the highest non-zero byte of the list's maximum down
//      (a max reduction first: counts below 2^16 take two passes, not eight).  Each pass keeps a 256-bin LDS histogram of the
//      next digit among the counts that share the digits chosen so far, and walks it from 255 down.  Exact for any
//      non-negative int64.  The passes also give n_above, the number of counts > t.
//   2. ordered compaction in code order: every bin with count > t, and the first k - n_above bins with count == t (none when
//      t is 0: a zero count is never returned).  Chunks of 1024 bins, positions from a workgroup prefix sum (ballot + mbcnt
//      per wave, the waves' totals in LDS).  The equal bins all hold the smallest count and arrive in code order, so they go
//      straight behind the n_above larger ones.
//   3. a bitonic sort of the (<= k) survivors in LDS by (count descending, code ascending).
// No global atomics, no scratch, every store an ordinary vector store; deterministic.
#include "crh_common.h"

namespace crh {
namespace {

constexpr int kSelThreads = 1024;
static_assert(CRH_MAX_K <= kSelThreads, "k_facet_select keeps one survivor per thread");

__device__ inline bool facet_before(unsigned long long ca, int32_t a, unsigned long long cb, int32_t b)
{
    return ca > cb || (ca == cb && a < b);   // count descending, code ascending; the padding (0, INT32_MAX) goes last
}

__global__ __launch_bounds__(kSelThreads) void k_facet_select(int n_bins, int k, const unsigned long long *__restrict__ bins_all,
                                                              int32_t *__restrict__ out_codes, int64_t *__restrict__ out_counts,
                                                              int64_t *__restrict__ out_info)
{
    constexpr int NT = kSelThreads, NW = NT / 64;
    __shared__ unsigned long long scnt[NT];
    __shared__ int32_t scode[NT];
    __shared__ unsigned int hist[256];
    __shared__ unsigned long long wred[NW], wsum[NW];
    __shared__ unsigned int wnz[NW], wgt[NW], weq[NW];
    __shared__ unsigned long long s_prefix;
    __shared__ unsigned int s_kk, s_above;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long *bins = bins_all + (size_t)q * n_bins;

    // maximum, sum and the number of non-zero bins
    unsigned long long vmax = 0ull, vsum = 0ull;
    unsigned int nz = 0u;
    for (int b = tid; b < n_bins; b += NT) {
        const unsigned long long v = bins[b];
        vmax = v > vmax ? v : vmax;
        vsum += v;
        nz += v ? 1u : 0u;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(vmax, d);
        vmax = o > vmax ? o : vmax;
        vsum += __shfl_xor(vsum, d);
        nz += __shfl_xor(nz, d);
    }
    if (lane == 0) {
        wred[wave] = vmax;
        wsum[wave] = vsum;
        wnz[wave] = nz;
    }
    __syncthreads();
    vmax = 0ull;
    vsum = 0ull;
    nz = 0u;
    for (int w = 0; w < NW; ++w) {
        vmax = wred[w] > vmax ? wred[w] : vmax;
        vsum += wsum[w];
        nz += wnz[w];
    }
    if (tid == 0) {
        out_info[2 * (size_t)q] = (int64_t)nz;
        out_info[2 * (size_t)q + 1] = (int64_t)vsum;
    }

    // 1. the kk-th largest count, kk = min(k, n_bins) (zeros take part: t = 0 when fewer than kk bins are non-zero)
    unsigned long long prefix = 0ull, pmask = 0ull;
    unsigned int kk = (unsigned int)(k < n_bins ? k : n_bins), n_above = 0u;
    int top = 0;
    while (top < 7 && (vmax >> (8 * (top + 1))) != 0ull) ++top;   // the highest non-zero byte of the maximum (workgroup-uniform)
    for (int byte = top; byte >= 0; --byte) {
        if (tid < 256) hist[tid] = 0u;
        __syncthreads();
        for (int b0 = 0; b0 < n_bins; b0 += NT) {   // (workgroup-uniform trip count)
            const int b = b0 + tid;
            bool in = false;
            unsigned int digit = 0u;
            if (b < n_bins) {
                const unsigned long long v = bins[b];
                in = (v & pmask) == prefix;
                digit = (unsigned int)(v >> (8 * byte)) & 255u;
            }
            // a wave whose counts share one digit (the common case: many small counts) adds once
            const unsigned long long im = __ballot(in);
            if (im != 0ull) {
                const unsigned int d0 = (unsigned int)__shfl((int)digit, __builtin_ctzll(im));
                const unsigned long long sm = __ballot(in && digit == d0);
                if (sm == im) {
                    if (lane == __builtin_ctzll(im)) atomicAdd(&hist[d0], (unsigned int)__popcll(im));
                } else if (in)
                    atomicAdd(&hist[digit], 1u);
            }
        }
        __syncthreads();
        if (tid == 0) {
            unsigned int cum = 0u;
            int d = 255;
            for (; d > 0; --d) {
                if (cum + hist[d] >= kk) break;
                cum += hist[d];
            }
            s_prefix = prefix | ((unsigned long long)d << (8 * byte));
            s_kk = kk - cum;
            s_above = n_above + cum;
        }
        __syncthreads();
        prefix = s_prefix;
        kk = s_kk;
        n_above = s_above;
        pmask |= 255ull << (8 * byte);
        __syncthreads();
    }
    const unsigned long long t = prefix;   // (the bytes above `top` are zero in every count)
    const unsigned int eq_quota = t == 0ull ? 0u : (unsigned int)k - n_above;   // (n_above < k: the k-th largest is not above itself)

    // 2. ordered compaction
    scnt[tid] = 0ull;
    scode[tid] = 0x7fffffff;
    __syncthreads();
    unsigned int run_gt = 0u, run_eq = 0u;
    for (int b0 = 0; b0 < n_bins; b0 += NT) {
        const int b = b0 + tid;
        unsigned long long v = 0ull;
        if (b < n_bins) v = bins[b];
        const bool gt = v > t, eq = v == t && eq_quota != 0u && b < n_bins;
        const unsigned long long gm = __ballot(gt), em = __ballot(eq);
        if (lane == 0) {
            wgt[wave] = (unsigned int)__popcll(gm);
            weq[wave] = (unsigned int)__popcll(em);
        }
        __syncthreads();
        unsigned int gbefore = 0u, ebefore = 0u, gtot = 0u, etot = 0u;
        for (int w = 0; w < NW; ++w) {
            gbefore += w < wave ? wgt[w] : 0u;
            ebefore += w < wave ? weq[w] : 0u;
            gtot += wgt[w];
            etot += weq[w];
        }
        const unsigned int gpre = __builtin_amdgcn_mbcnt_hi((unsigned int)(gm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)gm, 0u));
        const unsigned int epre = __builtin_amdgcn_mbcnt_hi((unsigned int)(em >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)em, 0u));
        if (gt) {
            const unsigned int at = run_gt + gbefore + gpre;   // < n_above <= k - 1
            if (at < (unsigned int)NT) {
                scnt[at] = v;
                scode[at] = b;
            }
        }
        if (eq) {
            const unsigned int e = run_eq + ebefore + epre;
            if (e < eq_quota && n_above + e < (unsigned int)NT) {
                scnt[n_above + e] = v;                          // n_above + e < k
                scode[n_above + e] = b;
            }
        }
        run_gt += gtot;
        run_eq += etot;
        __syncthreads();
    }

    // 3. the survivors sorted: count descending, code ascending (padding: count 0, code INT32_MAX)
    int P = 64;
    while (P < k) P <<= 1;
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride >= 1; stride >>= 1) {
            __syncthreads();
            const int other = tid ^ stride;
            if (tid < P && other > tid) {
                const unsigned long long ca = scnt[tid], cb = scnt[other];
                const int32_t a = scode[tid], b = scode[other];
                const bool asc = (tid & size) == 0;
                const bool swap = asc ? facet_before(cb, b, ca, a) : facet_before(ca, a, cb, b);
                if (swap) {
                    scnt[tid] = cb;
                    scode[tid] = b;
                    scnt[other] = ca;
                    scode[other] = a;
                }
            }
        }
    __syncthreads();
    if (tid < k) {
        const unsigned long long c = scnt[tid];
        out_codes[(size_t)q * k + tid] = c ? scode[tid] : -1;
        out_counts[(size_t)q * k + tid] = (int64_t)c;
    }
}

}  // namespace
}  // namespace crh

using namespace crh;

extern "C" {

int crh_facet_select(int nq, int n_bins, int k, const int64_t *bins_dev, int32_t *out_codes_dev, int64_t *out_counts_dev, int64_t *out_info_dev,
                     void *stream)
{
    if (nq < 0 || n_bins < 1 || k < 1 || k > CRH_MAX_K)
        return fail(CRH_E_INVALID, "facet_select: nq=%d n_bins=%d k=%d (nq >= 0, n_bins >= 1, 1 <= k <= %d)", nq, n_bins, k, CRH_MAX_K);
    if (nq == 0) return CRH_OK;
    if (!bins_dev || !out_codes_dev || !out_counts_dev || !out_info_dev) return fail(CRH_E_INVALID, "facet_select: NULL pointer");
    hipLaunchKernelGGL(k_facet_select, dim3((unsigned)nq), dim3(kSelThreads), 0, static_cast<hipStream_t>(stream), n_bins, k,
                       reinterpret_cast<const unsigned long long *>(bins_dev), out_codes_dev, out_counts_dev, out_info_dev);
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

}  // extern "C"
