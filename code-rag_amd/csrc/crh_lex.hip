// crh_lex.hip -- exact BM25 keyword search over a forward index in HBM (gfx950 / CDNA4 only).
//
// Replaces what Qdrant's sparse (BM25) vectors answer in query_points(prefetch=[dense, sparse], query=FusionQuery(RRF)): which
// stored chunks literally hold `parse_retry_after`.  The other half, the fusion, is crh_fuse_select.  The definition is THIS
// repository's (tests/lex_cases.py restates it on the CPU and tests/test_lexical_gpu.py compares bit for bit).
//
// A crh_lex handle is a FORWARD index whose rows are numbered like the rows of the crh_index beside it: row_off int64 [rows + 1],
// per entry a term id (u32, ascending and distinct inside a row) and its frequency (u8), per row its length dl (int32) -- 5 bytes
// per distinct term of a row.  A search streams all of it once per pass: brute force, exact, bound by HBM like the dense scan.
//
// The score of row r for a query, with c = (float)tf, len = (float)dl, every operation rounded to f32 on its own (the file is
// compiled -ffp-contract=off, the divisions are __fdiv_rn):
//     norm    = k1 * ((1.0f - b) + b * (len / avgdl))
//     contrib = idf_t * ((c * (k1 + 1.0f)) / (c + norm))
//     score   = +0.0f, then + contrib for each of the query's terms the row holds, in ASCENDING term id
// idf_t and avgdl are inputs (the host computes them from crh_lex_stats), so no logarithm is taken here.
//
// k_lex_walk, one wave per 32-row tile (the dense index's tile and mask word): a tile whose mask word is 0 is skipped without
// reading its entries; otherwise the wave streams the tile's contiguous entries, 64 ids per step and kLexSteps steps in flight,
// and every lane probes an open-addressing table in LDS of the pass's distinct query terms {id, base, 64-bit query
// membership}.  Hits are rare: a ballot takes them out and the wave handles them in ascending lane order, which is ascending
// (row, term) order.  The hit's row is counted from the 33 offsets the wave holds; LANE q IS QUERY q: it adds the contribution
// to its one accumulator when its membership bit is set, and when the row changes the lanes that touched the finished row hand
// it on.  That is the prescribed summation order with one accumulator and one flag per lane, no floating-point atomics, and no
// dependence on how tiles are spread over waves.
//
// Two passes of the same body.  Pass A files every finished (row, q, score) in a per-query histogram over the top 16 bits of the
// order-preserving integer image of the score (64 x 65536 u32, integer atomics); k_lex_cut finds per query the lowest bucket B_q
// whose suffix count reaches k and the exact number M_q of rows at or above it -- the histogram's total is out_count, exact and
// never clipped.  The candidate lists are then sized to the sum of M_q exactly: no overflow, no regrow path, no sampling
// assumption; 200 000 identical rows just make one list long.  Pass B scores again and appends the keys (ord(score) << 32) | ~row
// of the rows in buckets >= B_q; k_lex_select takes the k largest keys per query (radix select + bitonic sort: descending
// score, ties to the lower row).  The same walk with a table of bare terms counts document frequencies (crh_lex_stats).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "crh_common.h"

namespace crh {
namespace {

typedef __attribute__((ext_vector_type(4))) unsigned int lex_u32x4;

constexpr int kLexPassQ = 64;                    // queries per pass: lane q is query q
constexpr int kLexMaxKeys = kLexPassQ * CRH_LEX_MAX_QUERY_TERMS;   // 2048 distinct terms (and idf values) per pass at most
constexpr int kLexMaxSlots = 2 * kLexMaxKeys;    // 4096 slots of 16 bytes = 64 KiB of LDS at most; the table is sized to the pass
constexpr int kLexBuckets = 65536;               // histogram buckets per query: the top 16 bits of ord(score)
constexpr int kLexWaves = 4;                     // waves per k_lex_walk workgroup
constexpr int kLexSteps = 4;                     // 64-entry steps a wave has in flight
constexpr int kLexSelectThreads = 1024;

enum { LEX_HIST = 0, LEX_APPEND = 1, LEX_DF = 2 };

__device__ __forceinline__ uint32_t lex_ord(float f)       // monotone f32 -> u32 (as ord_f32 of crh_kernels.hpp)
{
    const uint32_t u = __builtin_bit_cast(uint32_t, f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float lex_unord(uint32_t o)
{
    return __builtin_bit_cast(float, (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}
__host__ __device__ __forceinline__ uint32_t lex_slot(uint32_t id, int log2_slots) { return (id * 2654435761u) >> (32 - log2_slots); }

struct LexWalk {
    const int64_t *row_off;
    const uint32_t *terms;
    const uint8_t *tf;
    const int32_t *dl;
    int64_t rows;
    const uint32_t *mask;        // one word per tile, or nullptr: every row
    const lex_u32x4 *table;      // 1 << log2_slots slots {id, base, membership lo, hi}; membership 0 = empty slot
    const float *idf;            // n_idf values: query q's idf of a slot's term is idf[base + (member queries below q)]
    int log2_slots, n_idf;
    float k1, b, avgdl;
    unsigned int *hist;          // LEX_HIST: [64][65536] bucket counts; LEX_DF: one count per table key (at `base`)
    const unsigned int *cut;     // LEX_APPEND: B_q
    const unsigned long long *list_base;   // LEX_APPEND: where query q's list starts in cand
    unsigned int *fill;          // LEX_APPEND: entries appended to query q's list so far
    unsigned long long *cand;
};

template <int MODE>
__global__ __launch_bounds__(kLexWaves * 64) void k_lex_walk(const LexWalk a)
{
    extern __shared__ lex_u32x4 lex_lds[];
    const int slots = 1 << a.log2_slots;
    float *lidf = reinterpret_cast<float *>(lex_lds + slots);
    for (int i = threadIdx.x; i < slots; i += kLexWaves * 64) lex_lds[i] = a.table[i];
    for (int i = threadIdx.x; i < a.n_idf; i += kLexWaves * 64) lidf[i] = a.idf[i];
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t ntiles = (a.rows + 31) / 32;
    const uint32_t smask = (uint32_t)slots - 1u;
    const unsigned long long below = (1ull << lane) - 1ull;
    const float k1p = a.k1 + 1.0f, one_minus_b = 1.0f - a.b;

    for (int64_t t = (int64_t)blockIdx.x * kLexWaves + wave; t < ntiles; t += (int64_t)gridDim.x * kLexWaves) {
        const int64_t r0 = t * 32;
        const int nrow = (int)(a.rows - r0 < 32 ? a.rows - r0 : 32);
        uint32_t m = a.mask ? a.mask[t] : 0xffffffffu;
        if (nrow < 32) m &= (1u << nrow) - 1u;
        if (m == 0u) continue;                                            // (wave-uniform) nothing of the tile is read
        const int64_t myoff = a.row_off[r0 + (lane < nrow ? lane : nrow)];   // lanes 0..nrow: the tile's offsets; the rest repeat the end
        const int64_t begin = __shfl(myoff, 0), end = __shfl(myoff, nrow);
        const uint32_t rel = (uint32_t)(myoff - begin), total = (uint32_t)(end - begin);
        const int mydl = lane < nrow ? a.dl[r0 + lane] : 0;
        const uint32_t *tp = a.terms + begin;
        const uint8_t *fp = a.tf + begin;

        int cur = -1;                 // the row being summed (wave-uniform)
        float acc = 0.0f;             // lane q: query q's score of row `cur` so far
        bool touched = false;         // lane q: row `cur` holds one of query q's terms
        auto hand_on = [&]() {
            if (MODE != LEX_DF && touched) {
                const uint32_t o = lex_ord(acc);
                if (MODE == LEX_HIST) {
                    atomicAdd(&a.hist[(size_t)lane * kLexBuckets + (o >> 16)], 1u);
                } else if ((o >> 16) >= a.cut[lane]) {
                    const unsigned int at = atomicAdd(&a.fill[lane], 1u);
                    a.cand[a.list_base[lane] + at] = ((unsigned long long)o << 32) | (unsigned long long)(~(uint32_t)(r0 + cur));
                }
            }
            acc = 0.0f;
            touched = false;
        };

        for (uint32_t s0 = 0; s0 < total; s0 += 64u * kLexSteps) {
            uint32_t id[kLexSteps];
#pragma unroll
            for (int u = 0; u < kLexSteps; ++u) {
                const uint32_t e = s0 + 64u * u + lane;
                id[u] = e < total ? tp[e] : 0u;
            }
#pragma unroll
            for (int u = 0; u < kLexSteps; ++u) {
                const uint32_t e0 = s0 + 64u * u, e = e0 + lane;
                if (e0 >= total) break;
                bool hit = false;
                uint32_t slot = lex_slot(id[u], a.log2_slots);
                if (e < total) {
                    for (;;) {                                           // (the table is at most half full: the probe ends)
                        const lex_u32x4 s = lex_lds[slot];
                        if ((s.z | s.w) == 0u) break;
                        if (s.x == id[u]) {
                            hit = true;
                            break;
                        }
                        slot = (slot + 1u) & smask;
                    }
                }
                unsigned long long hm = __ballot(hit);
                if (hm == 0ull) continue;
                const int c8 = hit ? (int)fp[e] : 0;
                while (hm) {                                             // ascending lane = ascending (row, term)
                    const int j = __ffsll((long long)hm) - 1;
                    hm &= hm - 1ull;
                    const int r = __popcll(__ballot(rel <= e0 + (uint32_t)j)) - 1;   // the last row whose entries start at or before the hit
                    if (!((m >> r) & 1u)) continue;
                    const lex_u32x4 s = lex_lds[__shfl(slot, j)];
                    if (MODE == LEX_DF) {
                        if (lane == 0) atomicAdd(&a.hist[s.y], 1u);
                        continue;
                    }
                    if (r != cur) {
                        hand_on();
                        cur = r;
                    }
                    const unsigned long long member = ((unsigned long long)s.w << 32) | s.z;
                    const float c = (float)__shfl(c8, j), len = (float)__shfl(mydl, r);   // (every lane takes part: read before the branch)
                    if ((member >> lane) & 1ull) {
                        const float w = lidf[s.y + __popcll(member & below)];
                        const float norm = a.k1 * (one_minus_b + a.b * __fdiv_rn(len, a.avgdl));
                        acc = acc + w * __fdiv_rn(c * k1p, c + norm);
                        touched = true;
                    }
                }
            }
        }
        hand_on();
    }
}

// Per query: the lowest bucket B whose suffix count reaches k (0 when fewer than k rows qualify), the rows M at or above it,
// and the histogram's total = the number of qualifying rows.  One workgroup of 256 threads per query, 256 buckets per thread.
__global__ __launch_bounds__(256) void k_lex_cut(const unsigned int *__restrict__ hist, int k, unsigned int *__restrict__ cut,
                                                 unsigned int *__restrict__ m_out, int64_t *__restrict__ out_count)
{
    __shared__ unsigned int part[256];
    const int q = blockIdx.x, tid = threadIdx.x;
    const unsigned int *h = hist + (size_t)q * kLexBuckets + (size_t)tid * 256;
    unsigned int mine = 0u;
    for (int i = 0; i < 256; ++i) mine += h[i];
    part[tid] = mine;
    __syncthreads();
    unsigned int above = 0u, all = 0u;
    for (int i = 0; i < 256; ++i) {
        const unsigned int p = part[i];
        all += p;
        above += i > tid ? p : 0u;
    }
    if (tid == 0) out_count[q] = (int64_t)all;
    if (all < (unsigned int)k) {
        if (tid == 0) {
            cut[q] = 0u;
            m_out[q] = all;
        }
    } else if (above < (unsigned int)k && (unsigned int)k <= above + mine) {   // exactly one thread: its chunk holds the k-th row
        unsigned int run = above;
        for (int i = 255; i >= 0; --i) {
            run += h[i];
            if (run >= (unsigned int)k) {
                cut[q] = (unsigned int)(tid * 256 + i);
                m_out[q] = run;
                break;
            }
        }
    }
}

// The k largest of query q's n unique keys, descending, written with row_base added; tail (-inf, -1).  One workgroup per
// query.  k-th largest by MSB-first 8-bit radix passes, then a bitonic sort of the keys at or above it.  (The workgroup
// helpers of crh_kernels.hpp do the same for the dense index; that header defines the dense kernels and belongs to one
// translation unit, so this file has its own small copies, like lex_ord.)
__global__ __launch_bounds__(kLexSelectThreads) void k_lex_select(const unsigned long long *__restrict__ cand,
                                                                  const unsigned long long *__restrict__ list_base,
                                                                  const unsigned int *__restrict__ m_in, int k, int64_t row_base,
                                                                  float *__restrict__ out_scores, int64_t *__restrict__ out_rows)
{
    constexpr int NT = kLexSelectThreads;
    __shared__ unsigned long long sortbuf[CRH_MAX_K];
    __shared__ unsigned int hist[256], bcast[2], scount;
    const int q = blockIdx.x, tid = threadIdx.x;
    const unsigned int n = m_in[q];
    const unsigned long long *keys = cand + list_base[q];
    float *os = out_scores + (size_t)q * k;
    int64_t *orow = out_rows + (size_t)q * k;
    const unsigned int k2 = (unsigned int)k < n ? (unsigned int)k : n;
    if (k2 > 0u) {                                                       // (uniform)
        unsigned long long prefix = 0ull;
        unsigned int kk = k2;
        for (int shift = 56; shift >= 0; shift -= 8) {
            if (tid < 256) hist[tid] = 0u;
            __syncthreads();
            for (unsigned int i = tid; i < n; i += NT) {
                const unsigned long long key = keys[i];
                if (shift == 56 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[(unsigned int)(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                unsigned int run = 0u;
                for (int d = 255; d >= 0; --d) {
                    const unsigned int c = hist[d];
                    if (run + c >= kk) {
                        bcast[0] = (unsigned int)d;
                        bcast[1] = kk - run;
                        break;
                    }
                    run += c;
                }
            }
            __syncthreads();
            prefix = (prefix << 8) | (unsigned long long)bcast[0];
            kk = bcast[1];
            __syncthreads();
        }
        int P = 1;
        while (P < (int)k2) P <<= 1;
        for (int i = tid; i < P; i += NT) sortbuf[i] = 0ull;
        if (tid == 0) scount = 0u;
        __syncthreads();
        for (unsigned int i = tid; i < n; i += NT) {
            const unsigned long long key = keys[i];
            if (key >= prefix) {                                         // keys are unique: exactly k2 of them
                const unsigned int o = atomicAdd(&scount, 1u);
                if (o < (unsigned int)CRH_MAX_K) sortbuf[o] = key;
            }
        }
        for (int size = 2; size <= P; size <<= 1) {
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                __syncthreads();
                for (int t = tid; t < (P >> 1); t += NT) {
                    const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                    const bool desc = (lo & size) == 0;
                    const unsigned long long x = sortbuf[lo], y = sortbuf[hi];
                    if ((x < y) == desc) {
                        sortbuf[lo] = y;
                        sortbuf[hi] = x;
                    }
                }
            }
        }
        __syncthreads();
    }
    for (int i = tid; i < k; i += NT) {
        if (i < (int)k2) {
            const unsigned long long key = sortbuf[i];
            os[i] = lex_unord((uint32_t)(key >> 32));
            orow[i] = row_base + (int64_t)(uint32_t)(~(uint32_t)key);
        } else {
            os[i] = -INFINITY;
            orow[i] = -1;
        }
    }
}

// every slot of nq lists is padding and every count 0: an empty index, or a pass none of whose queries has a term
__global__ __launch_bounds__(256) void k_lex_pad(int nq, int k, float *__restrict__ out_scores, int64_t *__restrict__ out_rows,
                                                 int64_t *__restrict__ out_count)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (int64_t)nq * k) {
        out_scores[i] = -INFINITY;
        out_rows[i] = -1;
    }
    if (i < nq) out_count[i] = 0;
}

// rows and sum of dl over the rows whose mask bit is set: out[0] += rows, out[1] += dl
__global__ __launch_bounds__(256) void k_lex_rowstats(const int32_t *__restrict__ dl, int64_t rows, const uint32_t *__restrict__ mask,
                                                      unsigned long long *__restrict__ out)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool on = r < rows && (!mask || ((mask[r >> 5] >> (r & 31)) & 1u));
    unsigned long long len = on ? (unsigned long long)dl[r] : 0ull;
    const unsigned long long n = (unsigned long long)__popcll(__ballot(on));
    for (int d = 32; d > 0; d >>= 1) len += __shfl_xor(len, d);
    if ((threadIdx.x & 63) == 0 && n) {
        atomicAdd(&out[0], n);
        atomicAdd(&out[1], len);
    }
}

template <typename T>
int lex_alloc(T **p, int64_t n)
{
    void *v = nullptr;
    hipError_t e = hipMalloc(&v, (size_t)std::max<int64_t>(n, 1) * sizeof(T));
    if (e != hipSuccess) return fail(CRH_E_CAPACITY, "hipMalloc of %lld bytes failed: %s", (long long)(n * (int64_t)sizeof(T)), hipGetErrorString(e));
    *p = static_cast<T *>(v);
    return CRH_OK;
}

// capacity for `need` elements of which the first `used` are kept: doubling, the old buffer copied and released
template <typename T>
int lex_grow(T **p, int64_t *cap, int64_t used, int64_t need)
{
    if (need <= *cap) return CRH_OK;
    int64_t c = std::max<int64_t>(*cap, 1024);
    while (c < need) c *= 2;
    T *np = nullptr;
    CRH_TRY(lex_alloc(&np, c));
    if (used > 0) CRH_HIP(hipMemcpy(np, *p, (size_t)used * sizeof(T), hipMemcpyDeviceToDevice));
    if (*p) CRH_HIP(hipFree(*p));
    *p = np;
    *cap = c;
    return CRH_OK;
}

// the open-addressing table of a pass, built on the host: key i sits at the first free slot from lex_slot(id)
struct LexTable {
    int log2_slots = 6;
    std::vector<lex_u32x4> slots;
    void build(const std::vector<uint32_t> &ids, const std::vector<uint32_t> &base, const std::vector<unsigned long long> &member)
    {
        log2_slots = 6;
        while ((size_t)(1 << log2_slots) < 2 * ids.size()) ++log2_slots;
        slots.assign((size_t)1 << log2_slots, lex_u32x4{0u, 0u, 0u, 0u});
        const uint32_t smask = (1u << log2_slots) - 1u;
        for (size_t i = 0; i < ids.size(); ++i) {
            uint32_t s = lex_slot(ids[i], log2_slots);
            while ((slots[s].z | slots[s].w) != 0u) s = (s + 1u) & smask;
            slots[s] = lex_u32x4{ids[i], base[i], (uint32_t)member[i], (uint32_t)(member[i] >> 32)};
        }
    }
};

}  // namespace
}  // namespace crh

struct crh_lex {
    int device = 0;
    int64_t rows = 0, entries = 0;
    int64_t cap_off = 0, cap_entries = 0, cap_tf = 0, cap_dl = 0;
    int64_t *row_off = nullptr;      // [rows + 1]
    uint32_t *terms = nullptr;
    uint8_t *tf = nullptr;
    int32_t *dl = nullptr;
    // workspace of the search and stats calls: allocated on first use, grown by doubling, released by crh_lex_destroy only
    unsigned int *hist = nullptr;            // [64][65536]; the head doubles as the df counters of crh_lex_stats
    crh::lex_u32x4 *table = nullptr;         // kLexMaxSlots slots, then kLexMaxKeys idf values
    unsigned int *ctl = nullptr;             // cut[64], m[64], fill[64]
    unsigned long long *list_base = nullptr; // [64], then the two sums of k_lex_rowstats
    unsigned long long *cand = nullptr;
    int64_t cand_cap = 0;
};

using namespace crh;

namespace {

int lex_workspace(crh_lex *l)
{
    if (l->hist) return CRH_OK;
    CRH_TRY(lex_alloc(&l->table, kLexMaxSlots + kLexMaxKeys / 4));
    CRH_TRY(lex_alloc(&l->ctl, 3 * kLexPassQ));
    CRH_TRY(lex_alloc(&l->list_base, kLexPassQ + 2));
    CRH_TRY(lex_alloc(&l->hist, (int64_t)kLexPassQ * kLexBuckets));
    return CRH_OK;
}

template <int MODE>
int lex_launch_walk(crh_lex *l, const LexTable &tab, int n_idf, const uint32_t *mask, float k1, float b, float avgdl, hipStream_t st)
{
    LexWalk a{};
    a.row_off = l->row_off;
    a.terms = l->terms;
    a.tf = l->tf;
    a.dl = l->dl;
    a.rows = l->rows;
    a.mask = mask;
    a.table = l->table;
    a.idf = reinterpret_cast<const float *>(l->table + kLexMaxSlots);
    a.log2_slots = tab.log2_slots;
    a.n_idf = n_idf;
    a.k1 = k1;
    a.b = b;
    a.avgdl = avgdl;
    a.hist = l->hist;
    a.cut = l->ctl;
    a.fill = l->ctl + 2 * kLexPassQ;
    a.list_base = l->list_base;
    a.cand = l->cand;
    const size_t lds = ((size_t)1 << tab.log2_slots) * 16 + (size_t)n_idf * 4;
    static OncePerDevice once;   // (per instantiation) the largest table + idf image is 72 KiB: above what a launch gets by default
    if (once.need())
        CRH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_lex_walk<MODE>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    kLexMaxSlots * 16 + kLexMaxKeys * 4));
    const int64_t ntiles = ceil_div(l->rows, 32);
    const unsigned blocks = (unsigned)std::min<int64_t>(ceil_div(ntiles, kLexWaves), (int64_t)current_device_cus() * 8);
    hipLaunchKernelGGL(k_lex_walk<MODE>, dim3(blocks), dim3(kLexWaves * 64), lds, st, a);
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

int lex_upload_table(crh_lex *l, const LexTable &tab, const std::vector<float> &idf, hipStream_t st)
{
    CRH_HIP(hipMemcpyAsync(l->table, tab.slots.data(), tab.slots.size() * 16, hipMemcpyHostToDevice, st));
    if (!idf.empty()) CRH_HIP(hipMemcpyAsync(l->table + kLexMaxSlots, idf.data(), idf.size() * 4, hipMemcpyHostToDevice, st));
    return CRH_OK;
}

}  // namespace

extern "C" {

int crh_lex_create(int device, int64_t capacity_rows, crh_lex **out)
{
    if (!out) return fail(CRH_E_INVALID, "out is NULL");
    *out = nullptr;
    if (capacity_rows < 0 || capacity_rows >= (1LL << 31)) return fail(CRH_E_INVALID, "capacity_rows=%lld outside 0..2^31-1", (long long)capacity_rows);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(CRH_E_NODEVICE, "no usable device %d", device);
    DeviceGuard g(device);
    if (!g.ok) return fail(CRH_E_NODEVICE, "hipSetDevice(%d) failed", device);
    crh_lex *l = new crh_lex();
    l->device = device;
    const int64_t zero = 0;
    int rc = lex_grow(&l->row_off, &l->cap_off, 0, capacity_rows + 1);
    if (rc == CRH_OK) rc = lex_grow(&l->dl, &l->cap_dl, 0, capacity_rows);
    if (rc == CRH_OK && hipMemcpy(l->row_off, &zero, 8, hipMemcpyHostToDevice) != hipSuccess) rc = fail(CRH_E_HIP, "hipMemcpy failed");
    if (rc != CRH_OK) {
        crh_lex_destroy(l);
        return rc;
    }
    *out = l;
    return CRH_OK;
}

int crh_lex_destroy(crh_lex *l)
{
    if (!l) return CRH_OK;
    DeviceGuard g(l->device);
    (void)hipDeviceSynchronize();
    void *bufs[] = {l->row_off, l->terms, l->tf, l->dl, l->hist, l->table, l->ctl, l->list_base, l->cand};
    for (void *p : bufs)
        if (p) (void)hipFree(p);
    delete l;
    return CRH_OK;
}

int crh_lex_clear(crh_lex *l)
{
    if (!l) return fail(CRH_E_INVALID, "lex handle is NULL");
    l->rows = 0;
    l->entries = 0;
    return CRH_OK;
}

int crh_lex_count(crh_lex *l, int64_t *rows_out, int64_t *entries_out)
{
    if (!l) return fail(CRH_E_INVALID, "lex handle is NULL");
    if (rows_out) *rows_out = l->rows;
    if (entries_out) *entries_out = l->entries;
    return CRH_OK;
}

int crh_lex_append(crh_lex *l, int64_t n, const int64_t *row_off_host, const uint32_t *terms_host, const uint8_t *tf_host, const int32_t *dl_host)
{
    if (!l) return fail(CRH_E_INVALID, "lex handle is NULL");
    if (n < 0) return fail(CRH_E_INVALID, "n=%lld is negative", (long long)n);
    if (n == 0) return CRH_OK;
    if (!row_off_host || !dl_host) return fail(CRH_E_INVALID, "NULL pointer");
    if (row_off_host[0] != 0) return fail(CRH_E_INVALID, "lex_append: row_off[0]=%lld, not 0", (long long)row_off_host[0]);
    for (int64_t i = 0; i < n; ++i)
        if (row_off_host[i + 1] < row_off_host[i]) return fail(CRH_E_INVALID, "lex_append: row_off decreases at row %lld", (long long)i);
    const int64_t ne = row_off_host[n];
    if (ne > 0 && (!terms_host || !tf_host)) return fail(CRH_E_INVALID, "NULL pointer");
    if (l->rows + n >= (1LL << 31)) return fail(CRH_E_CAPACITY, "lex_append: more than 2^31-1 rows");
    for (int64_t i = 0; i < n; ++i) {
        int64_t sum = 0;
        for (int64_t e = row_off_host[i]; e < row_off_host[i + 1]; ++e) {
            if (e > row_off_host[i] && terms_host[e] <= terms_host[e - 1])
                return fail(CRH_E_INVALID, "lex_append: the term ids of row %lld are not strictly ascending", (long long)i);
            if (tf_host[e] == 0) return fail(CRH_E_INVALID, "lex_append: row %lld holds a term with tf 0", (long long)i);
            sum += tf_host[e];
        }
        if ((int64_t)dl_host[i] < sum) return fail(CRH_E_INVALID, "lex_append: dl=%d of row %lld is below the sum of its tf (%lld)", dl_host[i], (long long)i, (long long)sum);
    }
    DeviceGuard g(l->device);
    CRH_HIP(hipDeviceSynchronize());   // (searches in flight on other streams read the buffers a growth releases)
    CRH_TRY(lex_grow(&l->row_off, &l->cap_off, l->rows + 1, l->rows + n + 1));
    CRH_TRY(lex_grow(&l->dl, &l->cap_dl, l->rows, l->rows + n));
    CRH_TRY(lex_grow(&l->terms, &l->cap_entries, l->entries, l->entries + ne));
    CRH_TRY(lex_grow(&l->tf, &l->cap_tf, l->entries, l->entries + ne));
    std::vector<int64_t> off((size_t)n);
    for (int64_t i = 0; i < n; ++i) off[(size_t)i] = l->entries + row_off_host[i + 1];
    CRH_HIP(hipMemcpy(l->row_off + l->rows + 1, off.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    CRH_HIP(hipMemcpy(l->dl + l->rows, dl_host, (size_t)n * 4, hipMemcpyHostToDevice));
    if (ne > 0) {
        CRH_HIP(hipMemcpy(l->terms + l->entries, terms_host, (size_t)ne * 4, hipMemcpyHostToDevice));
        CRH_HIP(hipMemcpy(l->tf + l->entries, tf_host, (size_t)ne, hipMemcpyHostToDevice));
    }
    l->rows += n;
    l->entries += ne;
    return CRH_OK;
}

int crh_lex_stats(crh_lex *l, const uint32_t *mask_dev, int64_t nt, const uint32_t *terms_host, int64_t *df_out_host, int64_t *rows_out,
                  int64_t *sum_dl_out)
{
    if (!l) return fail(CRH_E_INVALID, "lex handle is NULL");
    if (nt < 0 || (nt > 0 && (!terms_host || !df_out_host))) return fail(CRH_E_INVALID, "lex_stats: nt=%lld or a NULL pointer", (long long)nt);
    for (int64_t i = 0; i < nt; ++i) df_out_host[i] = 0;
    if (rows_out) *rows_out = 0;
    if (sum_dl_out) *sum_dl_out = 0;
    if (l->rows == 0) return CRH_OK;
    DeviceGuard g(l->device);
    CRH_TRY(lex_workspace(l));
    unsigned long long *sums = l->list_base + kLexPassQ;
    CRH_HIP(hipMemsetAsync(sums, 0, 16, nullptr));
    hipLaunchKernelGGL(k_lex_rowstats, dim3((unsigned)ceil_div(l->rows, 256)), dim3(256), 0, nullptr, l->dl, l->rows, mask_dev, sums);
    CRH_HIP(hipGetLastError());
    unsigned long long hs[2] = {0, 0};
    CRH_HIP(hipMemcpy(hs, sums, 16, hipMemcpyDeviceToHost));
    if (rows_out) *rows_out = (int64_t)hs[0];
    if (sum_dl_out) *sum_dl_out = (int64_t)hs[1];
    // the distinct terms, kLexMaxKeys per walk; a repeated term reads its first occurrence's count
    std::unordered_map<uint32_t, int64_t> first;
    std::vector<uint32_t> ids;
    std::vector<int64_t> where;
    for (int64_t i = 0; i < nt; ++i)
        if (first.emplace(terms_host[i], (int64_t)ids.size()).second) ids.push_back(terms_host[i]);
    std::vector<unsigned int> counts(ids.size());
    LexTable tab;
    for (size_t c0 = 0; c0 < ids.size(); c0 += kLexMaxKeys) {
        const size_t nk = std::min<size_t>(kLexMaxKeys, ids.size() - c0);
        std::vector<uint32_t> part(ids.begin() + c0, ids.begin() + c0 + nk), base(nk);
        std::vector<unsigned long long> member(nk, 1ull);
        for (size_t i = 0; i < nk; ++i) base[i] = (uint32_t)i;
        tab.build(part, base, member);
        CRH_TRY(lex_upload_table(l, tab, {}, nullptr));
        CRH_HIP(hipMemsetAsync(l->hist, 0, nk * 4, nullptr));
        CRH_TRY(lex_launch_walk<LEX_DF>(l, tab, 0, mask_dev, 0.0f, 0.0f, 1.0f, nullptr));
        CRH_HIP(hipMemcpy(counts.data() + c0, l->hist, nk * 4, hipMemcpyDeviceToHost));
    }
    for (int64_t i = 0; i < nt; ++i) df_out_host[i] = (int64_t)counts[(size_t)first[terms_host[i]]];
    return CRH_OK;
}

int crh_lex_search(crh_lex *l, int nq, const int64_t *q_off_host, const uint32_t *q_terms_host, const float *q_idf_host, float k1, float b,
                   float avgdl, int k, const uint32_t *mask_dev, int64_t row_base, float *out_scores_dev, int64_t *out_rows_dev,
                   int64_t *out_count_dev, void *stream)
{
    if (!l) return fail(CRH_E_INVALID, "lex handle is NULL");
    if (nq < 0 || k < 1 || k > CRH_MAX_K) return fail(CRH_E_INVALID, "lex_search: nq=%d k=%d (nq >= 0, 1 <= k <= %d)", nq, k, CRH_MAX_K);
    if (nq == 0) return CRH_OK;
    if (!q_off_host || !out_scores_dev || !out_rows_dev || !out_count_dev) return fail(CRH_E_INVALID, "lex_search: NULL pointer");
    if (!(avgdl > 0.0f) || !std::isfinite(avgdl) || !std::isfinite(k1) || !std::isfinite(b))
        return fail(CRH_E_INVALID, "lex_search: k1=%g b=%g avgdl=%g (finite, avgdl > 0)", (double)k1, (double)b, (double)avgdl);
    if (q_off_host[0] != 0) return fail(CRH_E_INVALID, "lex_search: q_off[0]=%lld, not 0", (long long)q_off_host[0]);
    for (int q = 0; q < nq; ++q) {
        const int64_t a = q_off_host[q], e = q_off_host[q + 1];
        if (e < a || e - a > CRH_LEX_MAX_QUERY_TERMS)
            return fail(CRH_E_INVALID, "lex_search: query %d has %lld terms (0..%d)", q, (long long)(e - a), CRH_LEX_MAX_QUERY_TERMS);
        if (e > a && (!q_terms_host || !q_idf_host)) return fail(CRH_E_INVALID, "lex_search: NULL pointer");
        for (int64_t i = a + 1; i < e; ++i)
            if (q_terms_host[i] <= q_terms_host[i - 1]) return fail(CRH_E_INVALID, "lex_search: the term ids of query %d are not strictly ascending", q);
    }
    DeviceGuard g(l->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    CRH_TRY(lex_workspace(l));
    LexTable tab;
    for (int p0 = 0; p0 < nq; p0 += kLexPassQ) {
        const int np = std::min(kLexPassQ, nq - p0);
        float *os = out_scores_dev + (size_t)p0 * k;
        int64_t *orow = out_rows_dev + (size_t)p0 * k;
        int64_t *oc = out_count_dev + p0;
        // the pass's distinct terms with their member queries; a term's idf values lie in ascending query order from `base`
        std::unordered_map<uint32_t, size_t> at;
        std::vector<uint32_t> ids;
        std::vector<unsigned long long> member;
        for (int q = 0; q < np; ++q)
            for (int64_t i = q_off_host[p0 + q]; i < q_off_host[p0 + q + 1]; ++i) {
                auto it = at.emplace(q_terms_host[i], ids.size());
                if (it.second) {
                    ids.push_back(q_terms_host[i]);
                    member.push_back(0ull);
                }
                member[it.first->second] |= 1ull << q;
            }
        if (ids.empty() || l->rows == 0) {
            hipLaunchKernelGGL(k_lex_pad, dim3((unsigned)ceil_div((int64_t)np * k, 256)), dim3(256), 0, st, np, k, os, orow, oc);
            CRH_HIP(hipGetLastError());
            continue;
        }
        std::vector<uint32_t> base(ids.size());
        uint32_t n_idf = 0;
        for (size_t i = 0; i < ids.size(); ++i) {
            base[i] = n_idf;
            n_idf += (uint32_t)__builtin_popcountll(member[i]);
        }
        std::vector<float> idf(n_idf);
        for (int q = 0; q < np; ++q)
            for (int64_t i = q_off_host[p0 + q]; i < q_off_host[p0 + q + 1]; ++i) {
                const size_t s = at[q_terms_host[i]];
                idf[base[s] + (uint32_t)__builtin_popcountll(member[s] & ((1ull << q) - 1ull))] = q_idf_host[i];
            }
        tab.build(ids, base, member);
        CRH_TRY(lex_upload_table(l, tab, idf, st));
        CRH_HIP(hipMemsetAsync(l->hist, 0, (size_t)np * kLexBuckets * 4, st));
        CRH_HIP(hipMemsetAsync(l->ctl, 0, 3 * kLexPassQ * 4, st));
        CRH_TRY(lex_launch_walk<LEX_HIST>(l, tab, (int)n_idf, mask_dev, k1, b, avgdl, st));
        hipLaunchKernelGGL(k_lex_cut, dim3((unsigned)np), dim3(256), 0, st, l->hist, k, l->ctl, l->ctl + kLexPassQ, oc);
        CRH_HIP(hipGetLastError());
        unsigned int m[kLexPassQ] = {};
        CRH_HIP(hipMemcpyAsync(m, l->ctl + kLexPassQ, (size_t)np * 4, hipMemcpyDeviceToHost, st));
        CRH_HIP(hipStreamSynchronize(st));   // the lists are sized to what pass A counted
        unsigned long long lb[kLexPassQ] = {}, total = 0ull;
        for (int q = 0; q < np; ++q) {
            lb[q] = total;
            total += m[q];
        }
        if ((int64_t)total > l->cand_cap) CRH_TRY(lex_grow(&l->cand, &l->cand_cap, 0, (int64_t)total));
        CRH_HIP(hipMemcpyAsync(l->list_base, lb, sizeof lb, hipMemcpyHostToDevice, st));
        if (total > 0ull) CRH_TRY(lex_launch_walk<LEX_APPEND>(l, tab, (int)n_idf, mask_dev, k1, b, avgdl, st));
        hipLaunchKernelGGL(k_lex_select, dim3((unsigned)np), dim3(kLexSelectThreads), 0, st, l->cand, l->list_base, l->ctl + kLexPassQ, k, row_base,
                           os, orow);
        CRH_HIP(hipGetLastError());
        CRH_HIP(hipStreamSynchronize(st));   // (lb and the table leave this frame; the next pass reuses the workspace)
    }
    return CRH_OK;
}

}  // extern "C"
