// crh_range.hpp -- score threshold and exact in-range counts (crh_search_range).
//
// For a raw query q let s(q, x) be the canonical f32 score crh_search gives row x, and thr a finite f32 threshold.  Row x is IN
// RANGE iff it is alive, passes the filter and s(q, x) >= thr as f32 values (inclusive).  The LIST is the exact top-k cut
// after its last in-range entry; the COUNT is the number of in-range rows, however many there are.
//
// The bf16 scan nominates every valid row whose MFMA score reaches tau[q], and |MFMA score - canonical score| <= eps with
// margin = margin_for(h) = 2 eps.  So with tau[q] = thr[q] - margin every in-range row is a candidate, and a
// candidate's approximate score a sorts it into one of three classes:
//   a >= thr + margin    canonical >= thr + margin - eps > thr: in range, counted from the score the scan produced;
//   a <  thr - margin    never nominated;
//   otherwise            the BAND: only these rows are given the ordered f32 chain, and count iff canonical >= thr.
// (thr -+ margin are rounded f32 sums: half an ulp of a value below 4, 2.4e-7, against the eps = margin / 2 >= 1.5e-4 of slack
// both comparisons keep.)
//
// A range batch is the three-launch bf16 form (enqueue_batch_range in crh_index.hip): k_prep_queries; [seed scan, k_tau;]
// k_range_tau; the MODE 1 scan -- k_scan over every tile or k_scan_list over a sparse mask's tile list; k_select; [k_range_count;]
// k_range_cut.  k_scan, k_scan_list, k_tau, k_select and k_prep_queries are used as they are.  Range batches do not use the
// int8 pass, the one-launch scan or the wide scan, whatever crh_index_set_nomination allows: the int8 intervals carry no
// per-query threshold argument, and the other two have no place between their phases where k_range_tau could run.
#pragma once

namespace crh {

// the thresholds of one batch, a kernel argument (as QueryClasses is): the library keeps no device copy whose lifetime a
// batch that is run again by crh_search_finish would depend on
struct RangeThr {
    float v[kMaxQ];
};

// One workgroup of `width` threads, thread = query slot.  List only: tau[q] = max(tau[q], thr[q] - margin) on top of k_tau's
// threshold -- a row that is in the canonical top-k AND in range has an approximate score of at least both.  With counts
// (counts != nullptr): tau[q] = thr[q] - margin, every in-range row becomes a candidate, and the query's total starts from 0.
// Slots >= nq keep +inf: they nominate nothing.
__global__ __launch_bounds__(64) void k_range_tau(RangeThr thr, float margin, int nq, float *__restrict__ tau, unsigned long long *__restrict__ counts)
{
    const int q = threadIdx.x;
    float t = INFINITY;
    if (q < nq) {
        const float lo = thr.v[q] - margin;
        t = counts ? lo : fmaxf(tau[q], lo);
        if (counts) counts[q] = 0ull;
    }
    tau[q] = t;
}

// Grid (nq, P): workgroup (q, p) takes every P-th block of 256 entries of query q's candidate list, so a band of many rows
// (hundreds of duplicates exactly at the threshold) is spread over P workgroups.  Candidates above the band are counted at
// once; band rows are collected in LDS (wave-aggregated append) and re-scored densely, one thread per row, with the same
// ordered chains k_select uses (canonical_dot_f32 on the master of an f32 store, canonical_dot_tiled on the tiles: 16 / 8
// 16-byte pieces in flight per thread).  The workgroup's total goes into counts[q] with one 64-bit integer atomic: integer
// additions commute, the result does not depend on the order of arrival.  A list that overflowed (qcount > qcap) gives a
// partial total here; k_select has flagged the overflow, the batch is run again and k_range_tau zeroes the total first.
// FACET (crh_search_range_facet; crh_facet.hpp): every row that is counted also adds 1 to its query's bin, `missing` or
// `out_of_range` by its code in fo.codes, wave-aggregated (facet_add_wave), and the workgroup's total goes into info[q][0] as
// well.  The host zeroes the batch's bins and info rows on the stream before the scan -- before a re-run too.
template <bool F32, bool FACET = false>
__global__ __launch_bounds__(256) void k_range_count(const u32x2 *__restrict__ qlist, const unsigned int *__restrict__ qcount, int qcap, RangeThr thr,
                                                     float margin, const float *__restrict__ qn, const u32x4 *__restrict__ xt,
                                                     const float *__restrict__ xf32, int dim, int ksteps, unsigned long long *__restrict__ counts,
                                                     FacetOut fo = FacetOut{})
{
    constexpr int NT = 256;
    constexpr int ROUNDS = 4;                 // blocks of NT candidates between two re-scoring rounds
    __shared__ float qv[2048];
    __shared__ uint32_t band[ROUNDS * NT];    // (a round appends at most NT rows)
    __shared__ unsigned int nband, total;
    const int q = blockIdx.x, tid = threadIdx.x;
    const unsigned int mtrue = qcount[q];
    const unsigned int M = mtrue < (unsigned int)qcap ? mtrue : (unsigned int)qcap;
    if ((unsigned int)blockIdx.y * NT >= M) return;   // (workgroup-uniform, before any barrier)
    for (int i = tid; i < dim; i += NT) qv[i] = qn[(size_t)q * dim + i];
    if (tid == 0) {
        nband = 0u;
        total = 0u;
    }
    __syncthreads();
    const float t = thr.v[q], hi = t + margin, lo = t - margin;
    const u32x2 *ql = qlist + (size_t)q * qcap;
    unsigned int cnt = 0u;
    unsigned long long *fbins = nullptr, *finfo = nullptr;
    if constexpr (FACET) {
        fbins = fo.bins + (size_t)q * fo.n_bins;
        finfo = fo.info + (size_t)q * 3;
    }
    // the rows collected so far: every thread reads nband behind a barrier, nobody appends before the next one
    auto rescore = [&]() {
        __syncthreads();
        const unsigned int n = nband;
        if constexpr (FACET) {
            for (unsigned int p0 = 0; p0 < n; p0 += NT) {   // (workgroup-uniform trip count: the waves aggregate together)
                const unsigned int p = p0 + tid;
                bool in = false;
                int32_t code = -1;
                if (p < n) {
                    const uint32_t row = band[p];
                    const float c = F32 ? canonical_dot_f32(xf32, dim, row, qv) : canonical_dot_tiled(xt, ksteps, row, qv);
                    in = c >= t;
                    if (in) code = fo.codes[row];
                }
                cnt += in ? 1u : 0u;
                facet_add_wave(in, code, fo.n_bins, fbins, finfo);
            }
        } else {
            for (unsigned int p = tid; p < n; p += NT) {
                const uint32_t row = band[p];
                const float c = F32 ? canonical_dot_f32(xf32, dim, row, qv) : canonical_dot_tiled(xt, ksteps, row, qv);
                cnt += (c >= t) ? 1u : 0u;
            }
        }
        __syncthreads();
        if (tid == 0) nband = 0u;
        __syncthreads();
    };
    int round = 0;
    for (unsigned int i0 = (unsigned int)blockIdx.y * NT; i0 < M; i0 += gridDim.y * NT) {   // (workgroup-uniform trip count)
        const unsigned int i = i0 + tid;
        bool inband = false, above = false;
        uint32_t row = 0u;
        if (i < M) {
            const u32x2 e = ql[i];
            const float a = bits_f32(e.x);
            if (a >= hi) {
                cnt += 1u;
                above = true;
                row = e.y;
            } else if (a >= lo) {
                inband = true;
                row = e.y;
            }
        }
        if constexpr (FACET) facet_add_wave(above, above ? fo.codes[row] : -1, fo.n_bins, fbins, finfo);
        const unsigned long long bm = __ballot(inband);   // one LDS atomic per wave, not one per band row
        unsigned int base = 0u;
        if ((tid & 63) == 0 && bm != 0ull) base = atomicAdd(&nband, (unsigned int)__popcll(bm));
        base = __shfl(base, 0);
        if (inband) band[base + __builtin_amdgcn_mbcnt_hi((unsigned int)(bm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)bm, 0u))] = row;
        if (++round == ROUNDS) {
            round = 0;
            rescore();
        }
    }
    rescore();
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d);
    if ((tid & 63) == 0 && cnt) atomicAdd(&total, cnt);
    __syncthreads();
    if (tid == 0 && total) {
        atomicAdd(&counts[q], (unsigned long long)total);
        if constexpr (FACET) atomicAdd(&finfo[0], (unsigned long long)total);
    }
}

// k_select's list is sorted: its entries below the threshold are a suffix, and become the padding (-inf, -1).
__global__ __launch_bounds__(256) void k_range_cut(RangeThr thr, int k, float *__restrict__ out_scores, int64_t *__restrict__ out_rows)
{
    const float t = thr.v[blockIdx.x];
    float *os = out_scores + (size_t)blockIdx.x * k;
    int64_t *orow = out_rows + (size_t)blockIdx.x * k;
    for (int i = threadIdx.x; i < k; i += 256) {
        if (!(os[i] >= t)) {
            os[i] = -INFINITY;
            orow[i] = -1;
        }
    }
}

}  // namespace crh
