// crh_facet.hpp -- exact per-value counts of one dictionary column (crh_index_facet, crh_search_range_facet).
//
// A row COUNTS iff it is alive and passes the conditions -- and, in the semantic form, its canonical f32 score reaches the
// query's threshold (the in-range rule of crh_range.hpp, inclusive).  For the column's code c of a counting row:
//   0 <= c < n_bins   bins[c] += 1
//   c < 0             missing += 1       (-1: the row does not have the key)
//   c >= n_bins       out_of_range += 1  (never written anywhere; the store passes the dictionary's size, so this stays 0)
// info = (counted, missing, out_of_range) with counted = sum(bins) + missing + out_of_range.
//
// All sums are 64-bit INTEGER atomics: integer additions commute, so the result does not depend on the order in which
// workgroups, waves or lanes arrive -- every call gives the same bins, a re-run of a batch the same as its first run.
//
// k_facet_count walks the effective mask words (alive AND filter, one u32 per 32-row tile) one thread per row, grid-stride.
// A lane reads its row's code only when its mask bit is set: a tile whose word is 0 costs one broadcast word read and no code
// read (the text kernel's rule).  Global atomics are the scarce resource (every adder on one address, or 64 lanes on 64
// different rows, is more than ten times slower than a coalesced store -- measured for float atomics; integer ones are not
// measured), so neither route issues one per row:
//   LDS route  (n_bins <= kFacetLdsBins)  the workgroup counts into a 32-bit LDS histogram (a workgroup sees fewer than 2^32
//              rows) and flushes only its non-zero bins at the end, one 64-bit global atomic each;
//   RUN route  (larger n_bins: file_path, entity_name)  chunks of one file are stored next to each other, so each wave
//              run-length-aggregates equal ADJACENT codes among its passing lanes: a lane is a run's head iff the previous
//              passing lane holds another code (shuffle compare), the run's length is a popcount of the passing lanes up to
//              the next head, and the head issues one global atomic per run.  Any order of the codes gives the right sums;
//              an order without runs merely costs one atomic per row.
// The route is chosen by n_bins alone.
#pragma once

namespace crh {

constexpr int kFacetLdsBins = CRH_FACET_LDS_BINS;   // 32 KB of 32-bit LDS bins
constexpr int kFacetRounds = 4;                      // distinct codes a wave aggregates before its remaining lanes add alone

// where the faceting variant of k_range_count adds: the column, and the bins / info rows of the batch's first query
struct FacetOut {
    const int32_t *codes;        // the column: codes[row]
    int n_bins;
    unsigned long long *bins;    // [nq, n_bins]
    unsigned long long *info;    // [nq, 3]
};

__device__ inline unsigned long long *facet_slot(int32_t code, int n_bins, unsigned long long *bins, unsigned long long *info)
{
    return code < 0 ? info + 1 : code >= n_bins ? info + 2 : bins + code;
}

// Every lane of the wave calls this together (`on`: the lane has a counting row with this code; bins / info: one query's).
// Lanes with equal codes are aggregated: the first remaining lane's code is broadcast, its holders are counted by ballot and
// leave, for at most kFacetRounds distinct codes -- a ten-value column would otherwise serialise on ten addresses; what is
// left after that adds on its own.
__device__ inline void facet_add_wave(bool on, int32_t code, int n_bins, unsigned long long *bins, unsigned long long *info)
{
    const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    code = code < 0 ? -1 : code >= n_bins ? n_bins : code;     // one key per slot
    unsigned long long rem = __ballot(on);
    for (int r = 0; r < kFacetRounds && rem != 0ull; ++r) {    // (rem is wave-uniform)
        const int leader = __builtin_ctzll(rem);
        const int32_t c0 = __shfl(code, leader);
        const unsigned long long same = __ballot(on && code == c0);
        if (lane == leader) atomicAdd(facet_slot(c0, n_bins, bins, info), (unsigned long long)__popcll(same));
        if (code == c0) on = false;
        rem &= ~same;
    }
    if (on) atomicAdd(facet_slot(code, n_bins, bins, info), 1ull);
}

// Grid-stride over blocks of 256 rows; mask: ceil(rows / 32) validity words; codes: the column.  bins / info are zero when the
// kernel starts (the host clears them on the stream).
template <bool LDS>
__global__ __launch_bounds__(256) void k_facet_count(const uint32_t *__restrict__ mask, const int32_t *__restrict__ codes, int64_t rows, int n_bins,
                                                     unsigned long long *__restrict__ bins, unsigned long long *__restrict__ info)
{
    constexpr int NT = 256;
    __shared__ uint32_t hist[LDS ? kFacetLdsBins : 1];
    __shared__ unsigned int tot[3];
    const int tid = threadIdx.x, lane = tid & 63;
    if (LDS)
        for (int b = tid; b < n_bins; b += NT) hist[b] = 0u;
    if (tid < 3) tot[tid] = 0u;
    __syncthreads();
    unsigned int counted = 0u, missing = 0u, oor = 0u;
    for (int64_t r0 = (int64_t)blockIdx.x * NT; r0 < rows; r0 += (int64_t)gridDim.x * NT) {   // (workgroup-uniform trip count)
        const int64_t row = r0 + tid;
        bool pass = false;
        int32_t code = -1;
        if (row < rows) {
            const uint32_t w = mask[row >> 5];
            pass = (w >> (row & 31)) & 1u;
            if (pass) code = codes[row];
        }
        counted += pass ? 1u : 0u;
        missing += (pass && code < 0) ? 1u : 0u;
        oor += (pass && code >= n_bins) ? 1u : 0u;
        const bool binned = pass && code >= 0 && code < n_bins;
        if (LDS) {
            if (binned) atomicAdd(&hist[code], 1u);
        } else {
            const unsigned long long bm = __ballot(binned);
            if (bm != 0ull) {   // (wave-uniform)
                const unsigned long long below = bm & ((1ull << lane) - 1ull);
                const int prev = below ? 63 - __builtin_clzll(below) : lane;
                const int32_t pcode = __shfl(code, prev);
                const bool head = binned && (below == 0ull || pcode != code);
                const unsigned long long hm = __ballot(head);
                if (head) {
                    const unsigned long long above = lane == 63 ? 0ull : hm & (~0ull << (lane + 1));
                    const unsigned long long upto = above ? ((1ull << __builtin_ctzll(above)) - 1ull) : ~0ull;   // lanes before the next head
                    atomicAdd(&bins[code], (unsigned long long)__popcll(bm & upto & (~0ull << lane)));
                }
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        counted += __shfl_xor(counted, d);
        missing += __shfl_xor(missing, d);
        oor += __shfl_xor(oor, d);
    }
    if (lane == 0) {
        if (counted) atomicAdd(&tot[0], counted);
        if (missing) atomicAdd(&tot[1], missing);
        if (oor) atomicAdd(&tot[2], oor);
    }
    __syncthreads();
    if (tid < 3 && tot[tid]) atomicAdd(&info[tid], (unsigned long long)tot[tid]);
    if (LDS)
        for (int b = tid; b < n_bins; b += NT) {
            const uint32_t v = hist[b];
            if (v) atomicAdd(&bins[b], (unsigned long long)v);
        }
}

}  // namespace crh
