// crh_graph.hip -- the call graph beside the index: batched, bit-parallel, level-synchronous BFS over CSRs in
// device memory, the listing of what it reached, the reached nodes as a row bitmap, and one shortest path.  gfx950 only.
//
// Bit q of a 64-bit word per node belongs to source set ("query") q, so one pass over the graph advances up to 64 searches:
// the "lane q = query q" idiom of crh_lex.hip with the lanes inside a word.  Every result is a set or a minimum depth, and OR
// does not depend on order: the outputs are exact and the same from run to run.
//
//   k_graph_sources   level 0 from the source lists (atomicOr: several queries may name one node)
//   k_graph_level     one launch per level, PULL form: next[u] = (OR of front[v] over u's neighbours v in the CSR opposite to
//                     the direction of travel) & ~seen[u].  next[u] and seen[u] have one writer, the lane that owns u; front is
//                     the level the previous launch finished.  Nothing inside a launch waits for another workgroup.  A
//                     workgroup ORs its new words together and makes one device-scope atomicOr into active[d]; the next
//                     launch reads active[d - 1] first and leaves when it is 0, so the levels enqueued behind a dead frontier
//                     cost a launch each and nothing else, and the host never waits between levels.
//   k_graph_unself    without include_self: the source bits leave `seen` (they stay in level 0)
//   k_graph_list      one workgroup per query: the nodes of levels first_level .. max_hops in (depth, node id) order, compacted
//                     by ballots and a scan over the workgroup's waves; the exact count
//   k_graph_row_words row -> node -> bit q of seen, as the validity words crh_index_row_mask writes
//   k_graph_path      one wave walks back from the target's level, taking the smallest neighbour that lies in the level before
//
// One lane per node; list_reduce is the one walk of an adjacency list: a list of CRH_GRAPH_WAVE_DEGREE entries or more is walked
// by its whole wave (64 entries per step, reduced over the lanes), the shorter ones by their own lane.  The four sweeps below
// (minimum, through list_min) and the narrow k_sigma_level (saturating sum) go through it; k_graph_level has the same walk
// written out with OR (it measured slower through the helper).
//
// Personalised PageRank over the same CSRs stands behind the BFS kernels: k_ppr_inv, k_ppr_seed, k_ppr_step (one
// launch per step, pull form, sums in list order: its own loops, never list_reduce), k_ppr_bins / k_ppr_bins_exclude, k_ppr_order.
//
// Components and layers are monotone sweeps to a fixed point, one launch per sweep, all in the one frame
// sweep_nodes: k_scc_trim, k_scc_colour, k_scc_mark, k_graph_layer; beside them k_scc_colour_init, k_scc_roots, k_scc_members,
// k_scc_count, k_scc_bins_count / k_scc_bins_keep, k_graph_layer_max, k_graph_node_words.
//
// Chains in full read the levels of a BFS: k_sigma_init / k_sigma_level (the number of shortest chains per node
// and query, saturating u64, one launch per level), k_graph_chains (one wave unranks one chain), k_between_meet / k_between_out
// (the nodes on a way from one set to another); k_graph_sources<true> / k_graph_level<true> are the BFS with an avoided node
// per query.
#include <algorithm>
#include <cstring>
#include <vector>

#include "crh_common.h"

namespace crh {
namespace {

using u64 = unsigned long long;

constexpr int kGraphThreads = 256;
constexpr int kGraphWaves = kGraphThreads / 64;
constexpr int kGraphListPerLane = 4;           // nodes a lane of k_graph_list looks at per step (1024 per workgroup)

__device__ __forceinline__ u64 shfl64(u64 v, int src)
{
    const unsigned lo = __shfl((unsigned)v, src), hi = __shfl((unsigned)(v >> 32), src);
    return ((u64)hi << 32) | lo;
}

__device__ __forceinline__ u64 wave_or(u64 v)
{
    unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        lo |= __shfl_xor(lo, o);
        hi |= __shfl_xor(hi, o);
    }
    return ((u64)hi << 32) | lo;
}

__device__ __forceinline__ int wave_min(int v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}

// The bits of the queries there are.
__host__ __device__ __forceinline__ u64 query_mask(int nq)
{
    return nq == 64 ? ~0ull : (1ull << nq) - 1ull;
}

// The one walk of an adjacency list: combine(...) of f(adj[i], key) over the list [b, e) of the lane's node, `identity` for an
// empty one.  The lane walks a list of fewer than CRH_GRAPH_WAVE_DEGREE entries itself; the longer ones are handed round by
// ballot, each walked by the whole wave 64 entries per step and reduced by wave_combine, and the result goes to the lane that
// owns the list.  `key` is what f needs to know about the node that owns the list (the lanes that help with another lane's list
// get that lane's).  EVERY lane of the wave calls it, with b == e when it has nothing to walk: the ballot and the shuffles
// inside are the whole wave's.  The terms are combined in whatever order the split gives, so the reduction must not depend on
// order: OR, a minimum, a saturating sum of terms >= 0.  k_ppr_step does NOT come here: its f32 sums are in list order by design
// (bit-equal to the CPU restatement).
template <class T, class F, class C, class W>
__device__ __forceinline__ T list_reduce(const int32_t *adj, int64_t b, int64_t e, int lane, int key, T identity, F f, C combine, W wave_combine)
{
    T acc = identity;
    const bool wide = e - b >= CRH_GRAPH_WAVE_DEGREE;
    if (!wide)
        for (int64_t i = b; i < e; ++i) acc = combine(acc, f(adj[i], key));
    u64 m = __ballot(wide);
    while (m) {
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        const int64_t bb = (int64_t)shfl64((u64)b, src), ee = (int64_t)shfl64((u64)e, src);
        const int owner = __shfl(key, src);
        T part = identity;
        for (int64_t i = bb + lane; i < ee; i += 64) part = combine(part, f(adj[i], owner));
        part = wave_combine(part);
        if (lane == src) acc = part;
    }
    return acc;
}

struct SourceArgs {
    int64_t off[CRH_GRAPH_MAX_QUERIES + 1];   // by value: at most 65 offsets
    const int32_t *nodes;
    int nq;
    int64_t n_nodes;
    u64 *level0;
    u64 *active0;
    const u64 *avoid;                         // AVOID only: bit q at v = query q never enters v
};

template <bool AVOID>
__global__ __launch_bounds__(kGraphThreads) void k_graph_sources(const SourceArgs a)
{
    const int64_t total = a.off[a.nq];
    for (int64_t i = (int64_t)blockIdx.x * kGraphThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kGraphThreads) {
        const int64_t v = a.nodes[i];
        if (v < 0 || v >= a.n_nodes) continue;                       // (-1: padding; a device list may hold anything)
        int q = 0;
        while (q + 1 < a.nq && a.off[q + 1] <= i) ++q;
        if (AVOID && ((a.avoid[v] >> q) & 1ull)) continue;           // (an avoided source is no source)
        atomicOr(a.level0 + v, 1ull << q);
        atomicOr(a.active0, 1ull << q);
    }
}

struct LevelArgs {
    const int64_t *off[2];
    const int32_t *adj[2];
    int ncsr;
    const u64 *front;
    u64 *next;
    u64 *seen;
    const u64 *active_prev;
    u64 *active_cur;
    int64_t n;
    u64 qmask;
    const u64 *avoid;                         // AVOID only
};

template <bool AVOID>
__global__ __launch_bounds__(kGraphThreads) void k_graph_level(const LevelArgs a)
{
    if (*a.active_prev == 0ull) return;                              // (written by the launch before this one: the frontier died)
    __shared__ u64 s_or[kGraphWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 mine = 0ull;
    for (int64_t base = ((int64_t)blockIdx.x * kGraphWaves + wave) * 64; base < a.n; base += (int64_t)gridDim.x * kGraphThreads) {
        const int64_t u = base + lane;                               // (base is the wave's: its lanes stay together)
        const bool in = u < a.n;
        const u64 sn = in ? (AVOID ? a.seen[u] | a.avoid[u] : a.seen[u]) : ~0ull;   // (a query that avoids u counts as having seen it)
        const bool want = (~sn & a.qmask) != 0ull;                   // (a node every query has seen already reads no list)
        u64 acc = 0ull;
        for (int c = 0; c < a.ncsr; ++c) {
            int64_t b = 0, e = 0;
            if (want) {
                b = a.off[c][u];
                e = a.off[c][u + 1];
            }
            // list_reduce written out with OR, every list ORed straight into the node's word: through the helper the kernel
            // took two registers more and the avoiding BFS of a small graph measured slower (profiles/graph_refactor.md).
            // The same contract holds: every lane reaches the ballot, with b == e when it has nothing to walk.
            const bool wide = e - b >= CRH_GRAPH_WAVE_DEGREE;
            if (!wide)
                for (int64_t i = b; i < e; ++i) acc |= a.front[a.adj[c][i]];
            u64 m = __ballot(wide);
            while (m) {
                const int src = __ffsll((long long)m) - 1;
                m &= m - 1;
                const int64_t bb = (int64_t)shfl64((u64)b, src), ee = (int64_t)shfl64((u64)e, src);
                u64 part = 0ull;
                for (int64_t i = bb + lane; i < ee; i += 64) part |= a.front[a.adj[c][i]];
                part = wave_or(part);
                if (lane == src) acc |= part;
            }
        }
        const u64 nw = acc & ~sn;
        if (nw) {                                                    // (the level was zeroed before the first launch)
            a.next[u] = nw;
            a.seen[u] = AVOID ? a.seen[u] | nw : sn | nw;
        }
        mine |= nw;
    }
    mine = wave_or(mine);
    if (lane == 0) s_or[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 all = 0ull;
        for (int w = 0; w < kGraphWaves; ++w) all |= s_or[w];
        if (all) atomicOr(a.active_cur, all);
    }
}

__global__ __launch_bounds__(kGraphThreads) void k_graph_unself(const u64 *level0, u64 *seen, int64_t n)
{
    for (int64_t v = (int64_t)blockIdx.x * kGraphThreads + threadIdx.x; v < n; v += (int64_t)gridDim.x * kGraphThreads) {
        const u64 s = level0[v];
        if (s) seen[v] &= ~s;
    }
}

__global__ __launch_bounds__(kGraphThreads) void k_graph_list(const u64 *levels, int64_t n, int first_level, int max_hops, int limit,
                                                              int32_t *out_nodes, int32_t *out_depth, int64_t *out_count)
{
    __shared__ int s_cnt[kGraphWaves];
    const int q = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int64_t kStep = (int64_t)kGraphThreads * kGraphListPerLane;
    int64_t total = 0;                                               // (the same in every thread)
    for (int d = first_level; d <= max_hops; ++d) {
        const u64 *lv = levels + (int64_t)d * n;
        for (int64_t base = 0; base < n; base += kStep) {
            // wave w takes the nodes base + w * 256 .. + 256, its pass j the 64 of them from j * 64: ascending node ids
            const int64_t first = base + (int64_t)wave * 64 * kGraphListPerLane;
            bool hit[kGraphListPerLane];
            int before[kGraphListPerLane];
            int wcount = 0;
#pragma unroll
            for (int j = 0; j < kGraphListPerLane; ++j) {
                const int64_t v = first + j * 64 + lane;
                hit[j] = v < n && ((lv[v] >> q) & 1ull);
                const u64 bal = __ballot(hit[j]);
                before[j] = wcount + __popcll(bal & ((1ull << lane) - 1ull));
                wcount += __popcll(bal);
            }
            if (lane == 0) s_cnt[wave] = wcount;
            __syncthreads();
            int pre = 0, all = 0;
#pragma unroll
            for (int w = 0; w < kGraphWaves; ++w) {
                if (w < wave) pre += s_cnt[w];
                all += s_cnt[w];
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < kGraphListPerLane; ++j) {
                const int64_t pos = total + pre + before[j];
                if (hit[j] && pos < limit) {
                    out_nodes[(int64_t)q * limit + pos] = (int32_t)(first + j * 64 + lane);
                    out_depth[(int64_t)q * limit + pos] = d;
                }
            }
            total += all;
        }
    }
    for (int64_t p = total + threadIdx.x; p < limit; p += kGraphThreads) {
        out_nodes[(int64_t)q * limit + p] = -1;
        out_depth[(int64_t)q * limit + p] = -1;
    }
    if (threadIdx.x == 0) out_count[q] = total;
}

__global__ __launch_bounds__(kGraphThreads) void k_graph_row_words(const int32_t *row_node, int64_t n_rows, const u64 *seen, int64_t n_nodes,
                                                                   int q, uint32_t *out, int64_t n_words)
{
    const int lane = threadIdx.x & 63;
    const int64_t pairs = (n_words + 1) / 2;                         // a wave writes two words
    for (int64_t p = (int64_t)blockIdx.x * kGraphWaves + (threadIdx.x >> 6); p < pairs; p += (int64_t)gridDim.x * kGraphWaves) {
        const int64_t r = p * 64 + lane;
        bool bit = false;
        if (r < n_rows) {
            const int64_t v = row_node[r];
            bit = v >= 0 && v < n_nodes && ((seen[v] >> q) & 1ull);
        }
        const u64 bal = __ballot(bit);
        if (lane == 0) out[2 * p] = (uint32_t)bal;
        if (lane == 32 && 2 * p + 1 < n_words) out[2 * p + 1] = (uint32_t)(bal >> 32);
    }
}

struct PathArgs {
    const int64_t *off[2];
    const int32_t *adj[2];
    int ncsr;
    const u64 *levels;
    int64_t n;
    int q;
    int64_t target;
    int max_hops;
    int32_t *out;        // [CRH_GRAPH_MAX_HOPS + 2]: the length, then the nodes from the source to the target
};

__global__ __launch_bounds__(64) void k_graph_path(const PathArgs a)
{
    const int lane = threadIdx.x;
    const bool at = lane <= a.max_hops && ((a.levels[(int64_t)lane * a.n + a.target] >> a.q) & 1ull);
    const u64 where = __ballot(at);
    if (!where) {
        if (lane == 0) a.out[0] = 0;
        return;
    }
    const int depth = __ffsll((long long)where) - 1;
    int64_t cur = a.target;
    if (lane == 0) {
        a.out[0] = depth + 1;
        a.out[1 + depth] = (int32_t)cur;
    }
    for (int d = depth; d >= 1; --d) {
        const u64 *prev = a.levels + (int64_t)(d - 1) * a.n;
        int best = 0x7fffffff;
        for (int c = 0; c < a.ncsr; ++c) {
            const int64_t b = a.off[c][cur], e = a.off[c][cur + 1];
            for (int64_t i = b + lane; i < e; i += 64) {
                const int p = a.adj[c][i];
                if ((prev[p] >> a.q) & 1ull) best = min(best, p);
            }
        }
        best = wave_min(best);
        if (best == 0x7fffffff) {                                    // (levels that are not this graph's BFS: no path, never a wild index)
            if (lane == 0) a.out[0] = 0;
            return;
        }
        cur = best;
        if (lane == 0) a.out[d] = best;
    }
}

// ---------------------------------------------------------------------------------------------------- personalised PageRank
// (DESIGN.md 3.30).  State is f32 [n_nodes, QS], QS the smallest power of two >= nq: lane l of a wave owns node base + l / QS and
// query l % QS.  Every sum has ONE writer and walks its pull list in list order, every operation is a separate f32 rounding
// (the library is built with -ffp-contract=off) and subnormals are kept: the result is the same bits as the CPU restatement.

__global__ __launch_bounds__(kGraphThreads) void k_ppr_inv(const int64_t *off0, const int64_t *off1, int64_t n, float *inv)
{
    for (int64_t v = (int64_t)blockIdx.x * kGraphThreads + threadIdx.x; v < n; v += (int64_t)gridDim.x * kGraphThreads) {
        int64_t out = off0[v + 1] - off0[v];
        if (off1) out += off1[v + 1] - off1[v];
        inv[v] = out > 0 ? 1.0f / (float)out : 0.0f;                 // (correctly rounded: v_div_scale / _fmas / _fixup)
    }
}

// One workgroup per query.  p0 and contrib0 were zeroed on the stream; the FIRST entry of a node takes the ordered sum of the
// weights of all its entries, found by comparing against the earlier entries as the group select does.
__global__ __launch_bounds__(kGraphThreads) void k_ppr_seed(const int32_t *nodes, const float *weights, int c, int64_t n, int shift,
                                                            const float *inv, float *p0, float *contrib)
{
    __shared__ int32_t s_node[CRH_MAX_K];
    __shared__ float s_w[CRH_MAX_K];
    __shared__ float s_sum;
    const int q = blockIdx.x;
    for (int i = threadIdx.x; i < c; i += kGraphThreads) {
        const int64_t v = nodes[(int64_t)q * c + i];
        const float w = weights ? weights[(int64_t)q * c + i] : 1.0f;
        const bool real = v >= 0 && v < n && w > 0.0f && w < __builtin_inff();   // (a negative, NaN or infinite weight counts as +0)
        s_node[i] = real ? (int32_t)v : -1;
        s_w[i] = real ? w : 0.0f;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float sum = 0.0f;
        for (int i = 0; i < c; ++i) sum += s_w[i];                  // (list order; padding adds +0, which changes no bits)
        s_sum = sum;
    }
    __syncthreads();
    const float sum = s_sum;
    const bool live = sum > 0.0f && sum < __builtin_inff();
    for (int i = threadIdx.x; i < c; i += kGraphThreads) {
        const int32_t v = s_node[i];
        if (v < 0) continue;
        bool first = true;
        for (int j = 0; j < i && first; ++j) first = s_node[j] != v;
        if (!first) continue;
        float w = 0.0f;
        for (int j = i; j < c; ++j)
            if (s_node[j] == v) w += s_w[j];
        const float p = live ? w / sum : 0.0f;
        const int64_t at = ((int64_t)v << shift) | q;
        p0[at] = p;
        contrib[at] = p * inv[v];
    }
}

struct PprStepArgs {
    const int64_t *off[2];
    const int32_t *adj[2];
    int ncsr;
    const float *p0, *inv, *contrib;   // contrib: what the launch before this one finished
    float *next, *p;                   // contrib_{t+1}, p_{t+1}
    int64_t n;
    int shift;
    float restart, a;
};

// One launch per step; a lane owns (node, query) and is the only writer of both outputs.  No list walk is skipped.  WIDE (QS =
// 64): the wave owns one node, loads 64 adjacency entries at a time and reads one 256-byte row of contrib per neighbour.
template <bool WIDE>
__global__ __launch_bounds__(kGraphThreads) void k_ppr_step(const PprStepArgs a)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int q = lane & ((1 << a.shift) - 1);
    const int per = 64 >> a.shift;                                   // nodes of a wave
    const int64_t groups = (a.n + per - 1) / per;
    for (int64_t w = (int64_t)blockIdx.x * kGraphWaves + wave; w < groups; w += (int64_t)gridDim.x * kGraphWaves) {
        const int64_t u = WIDE ? w : w * per + (lane >> a.shift);
        const bool in = u < a.n;
        float acc = 0.0f;
        for (int c = 0; c < a.ncsr; ++c) {
            const int32_t *adj = a.adj[c];
            if (WIDE) {
                const int64_t b = a.off[c][u], e = a.off[c][u + 1];
                for (int64_t i = b; i < e; i += 64) {
                    const int cnt = (int)(e - i < 64 ? e - i : 64);
                    const int mine = lane < cnt ? adj[i + lane] : 0;
                    int j = 0;
                    for (; j + 16 <= cnt; j += 16) {                 // sixteen rows in flight; the additions keep the list's order
                        float row[16];
#pragma unroll
                        for (int t = 0; t < 16; ++t) {
                            const int64_t v = __shfl(mine, j + t);
                            row[t] = a.contrib[(v << 6) | lane];
                        }
#pragma unroll
                        for (int t = 0; t < 16; ++t) acc += row[t];
                    }
                    for (; j + 4 <= cnt; j += 4) {
                        const int64_t v0 = __shfl(mine, j), v1 = __shfl(mine, j + 1), v2 = __shfl(mine, j + 2), v3 = __shfl(mine, j + 3);
                        const float c0 = a.contrib[(v0 << 6) | lane], c1 = a.contrib[(v1 << 6) | lane];
                        const float c2 = a.contrib[(v2 << 6) | lane], c3 = a.contrib[(v3 << 6) | lane];
                        acc += c0;
                        acc += c1;
                        acc += c2;
                        acc += c3;
                    }
                    for (; j < cnt; ++j) {
                        const int64_t v = __shfl(mine, j);
                        acc += a.contrib[(v << 6) | lane];
                    }
                }
            } else if (in) {
                const int64_t b = a.off[c][u], e = a.off[c][u + 1];
                int64_t i = b;
                for (; i + 8 <= e; i += 8) {                         // eight entries in flight, added in list order
                    float part[8];
#pragma unroll
                    for (int t = 0; t < 8; ++t) part[t] = a.contrib[((int64_t)adj[i + t] << a.shift) | q];
#pragma unroll
                    for (int t = 0; t < 8; ++t) acc += part[t];
                }
                for (; i < e; ++i) acc += a.contrib[((int64_t)adj[i] << a.shift) | q];
            }
        }
        if (in) {
            const int64_t at = (u << a.shift) | q;
            const float pn = (a.restart * a.p0[at]) + (a.a * acc);
            a.p[at] = pn;
            a.next[at] = pn * a.inv[u];
        }
    }
}

// bins[q, v] = the bit pattern of p[v, q] (order-preserving for >= +0): a 64-node tile is turned in LDS.
__global__ __launch_bounds__(kGraphThreads) void k_ppr_bins(const float *p, int64_t n, int shift, int nq, int64_t *bins)
{
    __shared__ uint32_t s_bits[64][65];
    const int qs = 1 << shift;
    for (int64_t base = (int64_t)blockIdx.x * 64; base < n; base += (int64_t)gridDim.x * 64) {
        const int nodes = (int)(n - base < 64 ? n - base : 64);
        for (int e = threadIdx.x; e < nodes * qs; e += kGraphThreads) s_bits[e >> shift][e & (qs - 1)] = __float_as_uint(p[base * qs + e]);
        __syncthreads();
        for (int e = threadIdx.x; e < nq * 64; e += kGraphThreads) {
            const int q = e >> 6, v = e & 63;
            if (v < nodes) bins[(int64_t)q * n + base + v] = (int64_t)s_bits[v][q];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kGraphThreads) void k_ppr_bins_exclude(const int32_t *exclude, int nq, int c, int64_t n, int64_t *bins)
{
    const int64_t total = (int64_t)nq * c;
    for (int64_t i = (int64_t)blockIdx.x * kGraphThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kGraphThreads) {
        const int64_t v = exclude[i];
        if (v >= 0 && v < n) bins[(i / c) * n + v] = 0;              // (several entries may name one node: they all write 0)
    }
}

// One workgroup per query: list 0 of the fuse table is the candidates as they stand, list 1 the candidates with graph_score > 0
// by descending graph_score, ties to the earlier position (rank by counting), padded with (-1, -inf).
__global__ __launch_bounds__(kGraphThreads) void k_ppr_order(const float *p, int64_t n, int shift, int c, const int64_t *rows, const float *cosine,
                                                             const int32_t *nodes, float *out_scores, int64_t *out_rows, float *out_gs)
{
    __shared__ uint32_t s_key[CRH_MAX_K];
    const int q = blockIdx.x;
    const int64_t in = (int64_t)q * c, out0 = (int64_t)q * 2 * c, out1 = out0 + c;
    for (int i = threadIdx.x; i < c; i += kGraphThreads) {
        const int64_t r = rows[in + i], v = nodes[in + i];
        const float g = (r >= 0 && v >= 0 && v < n) ? p[(v << shift) | q] : 0.0f;
        const uint32_t key = g > 0.0f ? __float_as_uint(g) : 0u;
        s_key[i] = key;
        out_gs[in + i] = __uint_as_float(key);
        out_scores[out0 + i] = cosine[in + i];
        out_rows[out0 + i] = r;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < c; i += kGraphThreads) {
        const uint32_t key = s_key[i];
        int before = 0, zeros = 0, zeros_before = 0;
        for (int j = 0; j < c; ++j) {
            const uint32_t o = s_key[j];
            before += (o > key || (o == key && j < i)) ? 1 : 0;
            zeros += o == 0u ? 1 : 0;
            zeros_before += (o == 0u && j < i) ? 1 : 0;
        }
        if (key) {
            out_scores[out1 + before] = __uint_as_float(key);
            out_rows[out1 + before] = rows[in + i];
        } else {
            out_scores[out1 + (c - zeros) + zeros_before] = -__builtin_inff();
            out_rows[out1 + (c - zeros) + zeros_before] = -1;
        }
    }
}

// ------------------------------------------------------------------------------- components and layers
// Integer sweeps over the same CSRs, one lane per node, one launch per sweep.  Every sweep is MONOTONE (a label is set once, a
// colour only falls, a layer only rises) towards a fixed point that does not depend on the order of the updates, so a sweep
// works in place: a value another lane wrote earlier in the same launch is as good as last launch's.  A sweep ORs its flags
// (bit 0: something changed, bit 1: an unassigned node is left) into ONE word with one atomicOr per workgroup; the next launch
// reads that word first and leaves when bit 0 is clear, so the host enqueues kSweepBatch sweeps per read-back.

constexpr int kSweepBatch = 16;                // sweeps enqueued per read-back of the flag words
constexpr int kSccCounters = 24;               // the extra words of the work arrays: flags [kSweepBatch + 1] from 0, four counters from here
constexpr int kNoColour = 0x7fffffff;

// The minimum of f(adj[i], key) over the list [b, e) of the lane's node, kNoColour for an empty one: list_reduce, under its contract.
template <class F>
__device__ __forceinline__ int list_min(const int32_t *adj, int64_t b, int64_t e, int lane, int key, F f)
{
    return list_reduce(adj, b, e, lane, key, kNoColour, f, [](int x, int y) { return min(x, y); }, [](int x) { return wave_min(x); });
}

// One atomicOr per workgroup: the OR of the lanes' flag bits 0 and 1.
__device__ __forceinline__ void sweep_flags(unsigned mine, unsigned *flag)
{
    __shared__ unsigned s_flag[kGraphWaves];
    const unsigned w = (__ballot(mine & 1u) ? 1u : 0u) | (__ballot(mine & 2u) ? 2u : 0u);
    if ((threadIdx.x & 63) == 0) s_flag[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned all = 0u;
        for (int i = 0; i < kGraphWaves; ++i) all |= s_flag[i];
        if (all) atomicOr(flag, all);
    }
}

// The frame of a sweep: it leaves at once when the sweep before it changed nothing, gives every node to one lane, and ORs the
// flag bits that body(u, in, lane) returns (`in`: u is a node) into *cur.  The nodes are handed out by the wave, and a lane
// past the last node still calls body: what body does with a list (list_min) is the whole wave's.
template <class B>
__device__ __forceinline__ void sweep_nodes(int64_t n, const unsigned *prev, unsigned *cur, B body)
{
    if ((*prev & 1u) == 0u) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned mine = 0u;
    for (int64_t base = ((int64_t)blockIdx.x * kGraphWaves + wave) * 64; base < n; base += (int64_t)gridDim.x * kGraphThreads) {
        const int64_t u = base + lane;                               // (base is the wave's: its lanes stay together)
        mine |= body(u, u < n, lane);
    }
    sweep_flags(mine, cur);
}

struct SccArgs {
    const int64_t *off_out, *off_in;           // the forward CSR (a node's targets) and the reverse one (its sources)
    const int32_t *adj_out, *adj_in;
    int32_t *comp;                             // -1: unassigned
    int32_t *colour;
    int64_t n;
    const unsigned *prev;
    unsigned *cur;
};

// Trim: an unassigned node without an unassigned in-neighbour, or without an unassigned out-neighbour, is a component by itself.
__global__ __launch_bounds__(kGraphThreads) void k_scc_trim(const SccArgs a)
{
    sweep_nodes(a.n, a.prev, a.cur, [&a](int64_t u, bool in, int lane) {
        const bool open = in && a.comp[u] < 0;
        const int32_t *comp = a.comp;
        const int self = (int)u;
        auto open_other = [comp](int v, int owner) { return v != owner && comp[v] < 0 ? 0 : 1; };
        const int no_in = list_min(a.adj_in, open ? a.off_in[u] : 0, open ? a.off_in[u + 1] : 0, lane, self, open_other);   // 0: there is one
        const int no_out = list_min(a.adj_out, open ? a.off_out[u] : 0, open ? a.off_out[u + 1] : 0, lane, self, open_other);
        if (!open) return 0u;
        if (no_in == 0 && no_out == 0) return 2u;
        a.comp[u] = self;
        return 1u;
    });
}

__global__ __launch_bounds__(kGraphThreads) void k_scc_colour_init(const int32_t *comp, int32_t *colour, int64_t n)
{
    for (int64_t v = (int64_t)blockIdx.x * kGraphThreads + threadIdx.x; v < n; v += (int64_t)gridDim.x * kGraphThreads)
        colour[v] = comp[v] < 0 ? (int32_t)v : kNoColour;           // (an assigned node never lowers a neighbour's colour)
}

// Colour: the smallest id among the unassigned nodes that reach the node.
__global__ __launch_bounds__(kGraphThreads) void k_scc_colour(const SccArgs a)
{
    sweep_nodes(a.n, a.prev, a.cur, [&a](int64_t u, bool in, int lane) {
        const bool open = in && a.comp[u] < 0;
        const int32_t *colour = a.colour;
        const int least = list_min(a.adj_in, open ? a.off_in[u] : 0, open ? a.off_in[u + 1] : 0, lane, 0, [colour](int v, int) { return (int)colour[v]; });
        if (!open || least >= a.colour[u]) return 0u;
        a.colour[u] = least;
        return 1u;
    });
}

__global__ __launch_bounds__(kGraphThreads) void k_scc_roots(int32_t *comp, const int32_t *colour, int64_t n)
{
    for (int64_t v = (int64_t)blockIdx.x * kGraphThreads + threadIdx.x; v < n; v += (int64_t)gridDim.x * kGraphThreads)
        if (comp[v] < 0 && colour[v] == (int32_t)v) comp[v] = (int32_t)v;
}

// Back-mark: an unassigned node of colour c joins component c once one of its out-neighbours has.
__global__ __launch_bounds__(kGraphThreads) void k_scc_mark(const SccArgs a)
{
    sweep_nodes(a.n, a.prev, a.cur, [&a](int64_t u, bool in, int lane) {
        const bool open = in && a.comp[u] < 0;
        const int32_t *comp = a.comp;
        const int c = open ? (int)a.colour[u] : -2;
        const int hit = list_min(a.adj_out, open ? a.off_out[u] : 0, open ? a.off_out[u + 1] : 0, lane, c,
                                 [comp](int v, int mine_c) { return comp[v] == mine_c ? 0 : 1; });
        if (!open || hit != 0) return 0u;
        a.comp[u] = c;
        return 1u;
    });
}

// counters: [0] components, [1] components of two nodes or more, [2] nodes that are not their component's label.  `big` was zeroed.
__global__ __launch_bounds__(kGraphThreads) void k_scc_members(const int32_t *comp, int32_t *big, int64_t n, unsigned *counters)
{
    unsigned mine = 0u;
    for (int64_t v = (int64_t)blockIdx.x * kGraphThreads + threadIdx.x; v < n; v += (int64_t)gridDim.x * kGraphThreads) {
        const int64_t c = comp[v];
        if (c != v && c >= 0 && c < n) {
            big[c] = 1;                                              // (every member writes the same value)
            ++mine;
        }
    }
    for (int o = 32; o >= 1; o >>= 1) mine += __shfl_xor(mine, o);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(counters + 2, mine);
}

__global__ __launch_bounds__(kGraphThreads) void k_scc_count(const int32_t *comp, const int32_t *big, int64_t n, unsigned *counters)
{
    unsigned roots = 0u, bigs = 0u;
    for (int64_t v = (int64_t)blockIdx.x * kGraphThreads + threadIdx.x; v < n; v += (int64_t)gridDim.x * kGraphThreads)
        if (comp[v] == (int32_t)v) {
            ++roots;
            bigs += big[v] ? 1u : 0u;
        }
    for (int o = 32; o >= 1; o >>= 1) {
        roots += __shfl_xor(roots, o);
        bigs += __shfl_xor(bigs, o);
    }
    if ((threadIdx.x & 63) == 0) {
        if (roots) atomicAdd(counters + 0, roots);
        if (bigs) atomicAdd(counters + 1, bigs);
    }
}

__global__ __launch_bounds__(kGraphThreads) void k_scc_bins_count(const int32_t *comp, int64_t n, u64 *bins)
{
    for (int64_t v = (int64_t)blockIdx.x * kGraphThreads + threadIdx.x; v < n; v += (int64_t)gridDim.x * kGraphThreads) {
        const int64_t c = comp[v];
        if (c >= 0 && c < n) atomicAdd(bins + c, 1ull);              // (a label that is no node counts nowhere)
    }
}

__global__ __launch_bounds__(kGraphThreads) void k_scc_bins_keep(const int32_t *self_nodes, int64_t n_self, int64_t n, u64 *bins)
{
    for (int64_t c = (int64_t)blockIdx.x * kGraphThreads + threadIdx.x; c < n; c += (int64_t)gridDim.x * kGraphThreads) {
        const u64 size = bins[c];
        if (size != 1ull) continue;                                  // (0 stays 0; two nodes or more are a cycle)
        int64_t lo = 0, hi = n_self;                                 // the one member is c itself: is it in the sorted list?
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (self_nodes[mid] < c) lo = mid + 1; else hi = mid;
        }
        if (!(lo < n_self && self_nodes[lo] == c)) bins[c] = 0ull;
    }
}

struct LayerArgs {
    const int64_t *off;                        // the pull CSR: ALONG the reverse one, AGAINST the forward one
    const int32_t *adj;
    const int32_t *comp;
    int32_t *layer;
    int64_t n;
    const unsigned *prev;
    unsigned *cur;
};

// layer[u] = max over the pull list of layer[v] + (comp[v] != comp[u]), from zeros: the longest path of the condensation.
__global__ __launch_bounds__(kGraphThreads) void k_graph_layer(const LayerArgs a)
{
    sweep_nodes(a.n, a.prev, a.cur, [&a](int64_t u, bool in, int lane) {
        const int32_t *comp = a.comp, *layer = a.layer;
        const int cu = in ? (int)comp[u] : 0;
        const int best = -list_min(a.adj, in ? a.off[u] : 0, in ? a.off[u + 1] : 0, lane, cu,
                                   [comp, layer](int v, int own) { return -((int)layer[v] + (comp[v] != own ? 1 : 0)); });
        if (!in || best == -kNoColour || best <= a.layer[u]) return 0u;
        a.layer[u] = best;
        return 1u;
    });
}

__global__ __launch_bounds__(kGraphThreads) void k_graph_layer_max(const int32_t *layer, int64_t n, int *out)
{
    int best = 0;
    for (int64_t v = (int64_t)blockIdx.x * kGraphThreads + threadIdx.x; v < n; v += (int64_t)gridDim.x * kGraphThreads) best = max(best, (int)layer[v]);
    best = -wave_min(-best);
    if ((threadIdx.x & 63) == 0 && best > 0) atomicMax(out, best);
}

__global__ __launch_bounds__(kGraphThreads) void k_graph_node_words(int64_t n, int mode, const int32_t *values, const int64_t *bins, int64_t lo, int64_t hi,
                                                                    int q, u64 *out)
{
    for (int64_t v = (int64_t)blockIdx.x * kGraphThreads + threadIdx.x; v < n; v += (int64_t)gridDim.x * kGraphThreads) {
        const int64_t x = values[v];
        bool hit;
        if (mode == CRH_GRAPH_WORDS_IN_CYCLE)
            hit = x >= 0 && x < n && bins[x] > 0;
        else if (mode == CRH_GRAPH_WORDS_SAME_COMPONENT)
            hit = x == lo;
        else
            hit = lo <= x && x <= hi;
        out[v] = hit ? 1ull << q : 0ull;
    }
}

// ------------------------------------------------------------------- chains in full: counts, the K first, between
// Exact integers over the levels of a BFS.  sigma is u64 [n_nodes, QS] in the layout of the PageRank state: lane l of a wave owns
// node base + l / QS and query l % QS.  Sums SATURATE at 2^64 - 1; every term is >= 0, so min(true sum, 2^64 - 1) is the same in
// whatever order the terms are added, and a long list may be split over the wave.

__device__ __forceinline__ u64 sat_add(u64 a, u64 b)
{
    const u64 s = a + b;
    return s < a ? ~0ull : s;
}

__device__ __forceinline__ u64 wave_sat_sum(u64 v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = sat_add(v, shfl64(v, (int)(threadIdx.x & 63) ^ o));
    return v;
}

// Level 0, and every other word zeroed: sigma[v][q] = bit q of levels[0][v] for q < nq.
__global__ __launch_bounds__(kGraphThreads) void k_sigma_init(const u64 *level0, int64_t n, int shift, u64 qmask, u64 *sigma)
{
    const int64_t total = n << shift;
    for (int64_t i = (int64_t)blockIdx.x * kGraphThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kGraphThreads)
        sigma[i] = ((level0[i >> shift] & qmask) >> (i & ((1 << shift) - 1))) & 1ull;
}

struct SigmaArgs {
    const int64_t *off;                        // the pull CSR
    const int32_t *adj;
    const u64 *cur, *prev;                     // levels[d], levels[d - 1]
    const u64 *active;                         // &active[d]
    u64 *sigma;
    int64_t n;
    int shift;
    u64 qmask;                                 // the queries there are: a column from nq on stays 0
};

// One launch per level d >= 1; a lane owns (node, query) and is the only writer of its entry.  It writes entries of level d
// and reads entries of level d - 1 only, so one buffer serves.  WIDE (QS = 64): the wave owns one node, loads 64 adjacency
// entries and their level words at a time and reads one 512-byte row of sigma per neighbour that any wanted query passed
// through.  Otherwise a lane walks its own list by list_reduce, which has the whole wave walk a list of CRH_GRAPH_WAVE_DEGREE
// entries or more for that lane's query (the key).
template <bool WIDE>
__global__ __launch_bounds__(kGraphThreads) void k_sigma_level(const SigmaArgs a)
{
    if (*a.active == 0ull) return;                                   // (nothing lies at this depth)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int q = lane & ((1 << a.shift) - 1);
    const int per = 64 >> a.shift;                                   // nodes of a wave
    const int64_t groups = (a.n + per - 1) / per;
    for (int64_t w = (int64_t)blockIdx.x * kGraphWaves + wave; w < groups; w += (int64_t)gridDim.x * kGraphWaves) {
        if (WIDE) {
            const int64_t u = w;                                     // (w < groups = n)
            const u64 uw = a.cur[u] & a.qmask;
            if (uw == 0ull) continue;                                // (the wave's: all lanes leave together)
            const int64_t b = a.off[u], e = a.off[u + 1];
            u64 acc = 0ull;
            for (int64_t i = b; i < e; i += 64) {
                const bool have = i + lane < e;
                const int mine = have ? a.adj[i + lane] : 0;
                const u64 pw = have ? a.prev[mine] & uw : 0ull;
                u64 m = __ballot(pw != 0ull);
                while (m) {
                    const int j = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    const int64_t v = __shfl(mine, j);
                    const u64 pv = shfl64(pw, j);
                    if ((pv >> lane) & 1ull) acc = sat_add(acc, a.sigma[(v << 6) | lane]);
                }
            }
            if ((uw >> lane) & 1ull) a.sigma[(u << 6) | lane] = acc;
        } else {
            const int64_t u = w * per + (lane >> a.shift);
            const bool mineq = u < a.n && (((a.cur[u] & a.qmask) >> q) & 1ull);
            int64_t b = 0, e = 0;
            if (mineq) {
                b = a.off[u];
                e = a.off[u + 1];
            }
            const u64 *prev = a.prev, *sigma = a.sigma;
            const int shift = a.shift;
            const u64 acc = list_reduce(a.adj, b, e, lane, q, 0ull,
                                        [prev, sigma, shift](int64_t v, int qq) { return (prev[v] >> qq) & 1ull ? sigma[(v << shift) | qq] : 0ull; },
                                        [](u64 x, u64 y) { return sat_add(x, y); }, [](u64 x) { return wave_sat_sum(x); });
            if (mineq) a.sigma[(u << a.shift) | q] = acc;
        }
    }
}

struct ChainArgs {
    const int64_t *off;                        // the pull CSR
    const int32_t *adj;
    const u64 *levels, *sigma;
    int64_t n;
    int shift, nq, max_hops, K;
    int32_t host_targets[CRH_GRAPH_MAX_QUERIES];   // by value, as the source offsets of the BFS
    const int32_t *dev_targets;                // or NULL: host_targets
    int32_t *out_nodes;                        // [nq][K][max_hops + 1]
    int32_t *out_len;                          // [nq]
    u64 *out_count;                            // [nq]
};

// One wave per (query, rank): unranks chain `rank` in the order of the node sequences read backwards from the target.  A step
// reads 64 entries of the pull list; an inclusive saturating scan of the qualifying entries' sigma finds the first entry whose
// running sum exceeds what is left of the rank (rank < K <= 64, so a saturated sum compares as the true one would).
__global__ __launch_bounds__(kGraphThreads) void k_graph_chains(const ChainArgs a)
{
    const int lane = threadIdx.x & 63;
    const int64_t slot = (int64_t)blockIdx.x * kGraphWaves + (threadIdx.x >> 6);
    if (slot >= (int64_t)a.nq * a.K) return;
    const int q = (int)(slot / a.K), rank = (int)(slot % a.K);
    const int64_t t = a.dev_targets ? a.dev_targets[q] : a.host_targets[q];
    const bool node = t >= 0 && t < a.n;
    const bool at = node && lane <= a.max_hops && ((a.levels[(int64_t)lane * a.n + t] >> q) & 1ull);
    const u64 where = __ballot(at);
    const int depth = where ? __ffsll((long long)where) - 1 : -1;
    const u64 count = where ? a.sigma[(t << a.shift) | q] : 0ull;
    if (rank == 0 && lane == 0) {
        a.out_count[q] = count;
        a.out_len[q] = depth + 1;
    }
    int mine = -1;                                                   // lane l holds the chain's node l, -1 beyond it
    bool ok = (u64)rank < count;
    if (ok) {
        if (lane == depth) mine = (int)t;
        u64 rem = (u64)rank;
        int64_t u = t;
        for (int d = depth; d >= 1 && ok; --d) {
            const u64 *prev = a.levels + (int64_t)(d - 1) * a.n;
            const int64_t b = a.off[u], e = a.off[u + 1];
            int next = -1;
            for (int64_t i = b; i < e && next < 0; i += 64) {
                const bool have = i + lane < e;
                const int v = have ? a.adj[i + lane] : 0;
                const bool qual = have && ((prev[v] >> q) & 1ull);
                const u64 s = qual ? a.sigma[((int64_t)v << a.shift) | q] : 0ull;
                u64 incl = s;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const u64 up = shfl64(incl, lane >= o ? lane - o : lane);
                    if (lane >= o) incl = sat_add(incl, up);
                }
                const u64 hit = __ballot(qual && rem < incl);
                if (hit) {
                    const int j = __ffsll((long long)hit) - 1;
                    const u64 before = j ? shfl64(incl, j - 1) : 0ull;   // (<= rem: exact, never saturated)
                    rem -= before;
                    next = __shfl(v, j);
                } else {
                    rem -= shfl64(incl, 63);                         // (<= rem likewise)
                }
            }
            if (next < 0) {                                          // (levels and sigma that are not this graph's: no chain, never a wild index)
                ok = false;
                break;
            }
            if (lane == d - 1) mine = next;
            u = next;
        }
    }
    if (lane <= a.max_hops) a.out_nodes[slot * (a.max_hops + 1) + lane] = ok ? mine : -1;
}

struct BetweenArgs {
    const u64 *fwd, *back;                     // levels of the two searches, [max_hops + 1][n]
    int64_t n;
    int max_hops, mode, nq;
    u64 *meet;                                 // [max_hops + 1]
    u64 *out;                                  // [n]
    int32_t *dist;                             // [nq] or NULL
};

constexpr int kLevels = CRH_GRAPH_MAX_HOPS + 1;

// meet[d] = OR over v and i + j = d of F[i][v] & B[j][v], d <= max_hops: one atomicOr per workgroup and distance.  meet was zeroed.
__global__ __launch_bounds__(kGraphThreads) void k_between_meet(const BetweenArgs a)
{
    __shared__ u64 s_meet[kGraphWaves][kLevels];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 m[kLevels];
#pragma unroll
    for (int d = 0; d < kLevels; ++d) m[d] = 0ull;
    for (int64_t v = (int64_t)blockIdx.x * kGraphThreads + threadIdx.x; v < a.n; v += (int64_t)gridDim.x * kGraphThreads) {
        u64 f[kLevels], bk[kLevels], anyf = 0ull, anyb = 0ull;
#pragma unroll
        for (int i = 0; i < kLevels; ++i) {
            f[i] = i <= a.max_hops ? a.fwd[(int64_t)i * a.n + v] : 0ull;
            bk[i] = i <= a.max_hops ? a.back[(int64_t)i * a.n + v] : 0ull;
            anyf |= f[i];
            anyb |= bk[i];
        }
        if ((anyf & anyb) == 0ull) continue;
#pragma unroll
        for (int i = 0; i < kLevels; ++i)
#pragma unroll
            for (int j = 0; j < kLevels - i; ++j) m[i + j] |= f[i] & bk[j];
    }
#pragma unroll
    for (int d = 0; d < kLevels; ++d) {
        const u64 w = wave_or(m[d]);
        if (lane == 0) s_meet[wave][d] = w;
    }
    __syncthreads();
    if (threadIdx.x <= a.max_hops) {
        u64 all = 0ull;
        for (int w = 0; w < kGraphWaves; ++w) all |= s_meet[w][threadIdx.x];
        if (all) atomicOr(a.meet + threadIdx.x, all);
    }
}

// out[v] = OR over i + j <= max_hops of F[i][v] & B[j][v] & M[i + j]; M[d] = every query (mode 0) or the queries whose sets
// first meet at distance d (mode 1).  dist[q] = that distance, -1 when the sets never meet within max_hops.
__global__ __launch_bounds__(kGraphThreads) void k_between_out(const BetweenArgs a)
{
    u64 mask[kLevels], earlier = 0ull;
    const u64 qmask = query_mask(a.nq);
#pragma unroll
    for (int d = 0; d < kLevels; ++d) {
        const u64 md = d <= a.max_hops ? a.meet[d] : 0ull;
        mask[d] = d > a.max_hops ? 0ull : a.mode == 0 ? qmask : md & ~earlier;
        earlier |= md;
    }
    if (a.dist && blockIdx.x == 0 && (int)threadIdx.x < a.nq) {
        int dq = -1;
        for (int d = a.max_hops; d >= 0; --d)
            if ((a.meet[d] >> threadIdx.x) & 1ull) dq = d;
        a.dist[threadIdx.x] = dq;
    }
    for (int64_t v = (int64_t)blockIdx.x * kGraphThreads + threadIdx.x; v < a.n; v += (int64_t)gridDim.x * kGraphThreads) {
        u64 f[kLevels], bk[kLevels];
#pragma unroll
        for (int i = 0; i < kLevels; ++i) {
            f[i] = i <= a.max_hops ? a.fwd[(int64_t)i * a.n + v] : 0ull;
            bk[i] = i <= a.max_hops ? a.back[(int64_t)i * a.n + v] : 0ull;
        }
        u64 acc = 0ull;
#pragma unroll
        for (int i = 0; i < kLevels; ++i)
#pragma unroll
            for (int j = 0; j < kLevels - i; ++j) acc |= f[i] & bk[j] & mask[i + j];
        a.out[v] = acc;
    }
}

int graph_alloc(void **p, int64_t bytes)
{
    *p = nullptr;
    CRH_HIP(hipMalloc(p, (size_t)std::max<int64_t>(bytes, 8)));
    return CRH_OK;
}

int check_csr(const char *what, int64_t n_nodes, int64_t n_edges, const int64_t *off, const int32_t *adj)
{
    if (!off || (n_edges > 0 && !adj)) return fail(CRH_E_INVALID, "graph_set_relation: %s: NULL pointer", what);
    if (off[0] != 0 || off[n_nodes] != n_edges)
        return fail(CRH_E_INVALID, "graph_set_relation: %s offsets run from %lld to %lld, not 0 to %lld", what, (long long)off[0], (long long)off[n_nodes], (long long)n_edges);
    for (int64_t v = 0; v < n_nodes; ++v)
        if (off[v + 1] < off[v]) return fail(CRH_E_INVALID, "graph_set_relation: %s offsets decrease at node %lld", what, (long long)v);
    for (int64_t i = 0; i < n_edges; ++i)
        if (adj[i] < 0 || adj[i] >= n_nodes) return fail(CRH_E_INVALID, "graph_set_relation: %s entry %lld names node %d of %lld", what, (long long)i, adj[i], (long long)n_nodes);
    return CRH_OK;
}

unsigned graph_blocks(int64_t items, int64_t per_block)
{
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(items, per_block), (int64_t)current_device_cus() * 8));
}

// The range of an argument that several entry points take, refused in the name of the one that was called.
int check_nq(const char *who, int nq)
{
    if (nq < 1 || nq > CRH_GRAPH_MAX_QUERIES) return fail(CRH_E_INVALID, "%s: nq=%d outside 1..%d", who, nq, CRH_GRAPH_MAX_QUERIES);
    return CRH_OK;
}

int check_hops(const char *who, int max_hops)
{
    if (max_hops < 1 || max_hops > CRH_GRAPH_MAX_HOPS) return fail(CRH_E_INVALID, "%s: max_hops=%d outside 1..%d", who, max_hops, CRH_GRAPH_MAX_HOPS);
    return CRH_OK;
}

int check_n_nodes(const char *who, int64_t n_nodes)
{
    if (n_nodes < 0 || n_nodes >= (1LL << 31)) return fail(CRH_E_INVALID, "%s: n_nodes=%lld outside 0..2^31-1", who, (long long)n_nodes);
    return CRH_OK;
}

int check_q(const char *who, int q)
{
    if (q < 0 || q >= CRH_GRAPH_MAX_QUERIES) return fail(CRH_E_INVALID, "%s: q=%d outside 0..%d", who, q, CRH_GRAPH_MAX_QUERIES - 1);
    return CRH_OK;
}

}  // namespace
}  // namespace crh

struct crh_graph_relation {
    bool set = false;
    int64_t n_edges = 0;
    int64_t *off[2] = {nullptr, nullptr};    // 0: along the edges (a node's targets), 1: against them (its sources)
    int32_t *adj[2] = {nullptr, nullptr};
};

struct crh_graph {
    int device = 0;
    int64_t n_nodes = 0;
    crh_graph_relation rel[CRH_GRAPH_MAX_RELATIONS];
    int32_t *path = nullptr;                 // CRH_GRAPH_MAX_HOPS + 2 ints
    void *sources = nullptr;                 // the upload of a host source list (graph_stage)
    int64_t cap_sources = 0;                 // bytes
    float *inv[CRH_GRAPH_MAX_RELATIONS][3] = {};   // personalised PageRank: 1 / out(v) per (relation, direction), built on first use
    void *seeds = nullptr;                   // the upload of a host seed list: nodes, then weights
    int64_t cap_seeds = 0;                   // bytes
};

using namespace crh;

namespace {

void graph_free_relation(crh_graph_relation &r)
{
    for (int c = 0; c < 2; ++c) {
        if (r.off[c]) (void)hipFree(r.off[c]);
        if (r.adj[c]) (void)hipFree(r.adj[c]);
        r.off[c] = nullptr;
        r.adj[c] = nullptr;
    }
    r.set = false;
    r.n_edges = 0;
}

void graph_drop_inv(crh_graph *g, int rel)
{
    for (float *&p : g->inv[rel]) {
        if (p) (void)hipFree(p);
        p = nullptr;
    }
}

// The shift of the (node, query) layout that the PageRank state and sigma share: entry (v << shift) | q, 1 << shift = QS, the
// smallest power of two >= nq.
int layout_shift(int nq)
{
    int shift = 0;
    while ((1 << shift) < nq) ++shift;
    return shift;
}

// The upload of host lists of `bytes` each, one behind the other (NULL: its place stays as it is), into a buffer of the handle's
// that grows on demand to at least `min_cap` bytes.  Returns when the copies are done.
int graph_stage(void **buf, int64_t *cap, int64_t bytes, int64_t min_cap, hipStream_t st, std::initializer_list<const void *> lists)
{
    const int64_t need = bytes * (int64_t)lists.size();
    if (*cap < need) {
        CRH_HIP(hipStreamSynchronize(st));   // (a call in flight on this stream still reads the old upload)
        if (*buf) (void)hipFree(*buf);
        *buf = nullptr;
        *cap = 0;
        CRH_TRY(graph_alloc(buf, std::max(need, min_cap)));
        *cap = std::max(need, min_cap);
    }
    char *at = static_cast<char *>(*buf);
    for (const void *list : lists) {
        if (list) CRH_HIP(hipMemcpyAsync(at, list, (size_t)bytes, hipMemcpyHostToDevice, st));
        at += bytes;
    }
    CRH_HIP(hipStreamSynchronize(st));       // (the caller may free its lists on return; pageable memory is staged anyway)
    return CRH_OK;
}

// The CSRs a traversal in `direction` PULLS through: travelling along the edges, a node looks at its sources (the reverse CSR).
int graph_pull(const crh_graph *g, int rel, int direction, const int64_t **off, const int32_t **adj)
{
    const crh_graph_relation &r = g->rel[rel];
    int n = 0;
    if (direction == CRH_GRAPH_ALONG || direction == CRH_GRAPH_BOTH) {
        off[n] = r.off[1];
        adj[n++] = r.adj[1];
    }
    if (direction == CRH_GRAPH_AGAINST || direction == CRH_GRAPH_BOTH) {
        off[n] = r.off[0];
        adj[n++] = r.adj[0];
    }
    return n;
}

// The one pull CSR of ALONG or AGAINST, for the callers that have refused CRH_GRAPH_BOTH.
void graph_pull_one(const crh_graph *g, int rel, int direction, const int64_t **off, const int32_t **adj)
{
    const int c = direction == CRH_GRAPH_ALONG ? 1 : 0;              // ALONG pulls through a node's sources
    *off = g->rel[rel].off[c];
    *adj = g->rel[rel].adj[c];
}

int graph_check_rel(const crh_graph *g, int rel, int direction, const char *who)
{
    if (!g) return fail(CRH_E_INVALID, "graph handle is NULL");
    if (rel < 0 || rel >= CRH_GRAPH_MAX_RELATIONS || !g->rel[rel].set) return fail(CRH_E_INVALID, "%s: relation %d is not set", who, rel);
    if (direction != CRH_GRAPH_ALONG && direction != CRH_GRAPH_AGAINST && direction != CRH_GRAPH_BOTH)
        return fail(CRH_E_INVALID, "%s: direction=%d is none of CRH_GRAPH_ALONG / _AGAINST / _BOTH", who, direction);
    return CRH_OK;
}

}  // namespace

extern "C" {

int crh_graph_create(int device, int64_t n_nodes, crh_graph **out)
{
    if (!out) return fail(CRH_E_INVALID, "out is NULL");
    *out = nullptr;
    if (n_nodes < 0 || n_nodes >= (1LL << 31)) return fail(CRH_E_INVALID, "n_nodes=%lld outside 0..2^31-1", (long long)n_nodes);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(CRH_E_NODEVICE, "no usable device %d", device);
    DeviceGuard g(device);
    if (!g.ok) return fail(CRH_E_NODEVICE, "hipSetDevice(%d) failed", device);
    crh_graph *h = new crh_graph();
    h->device = device;
    h->n_nodes = n_nodes;
    void *p = nullptr;
    const int rc = graph_alloc(&p, 4 * (CRH_GRAPH_MAX_HOPS + 2));
    h->path = static_cast<int32_t *>(p);
    if (rc != CRH_OK) {
        crh_graph_destroy(h);
        return rc;
    }
    *out = h;
    return CRH_OK;
}

int crh_graph_destroy(crh_graph *g)
{
    if (!g) return CRH_OK;
    DeviceGuard guard(g->device);
    (void)hipDeviceSynchronize();
    for (auto &r : g->rel) graph_free_relation(r);
    for (int r = 0; r < CRH_GRAPH_MAX_RELATIONS; ++r) graph_drop_inv(g, r);
    if (g->seeds) (void)hipFree(g->seeds);
    if (g->path) (void)hipFree(g->path);
    if (g->sources) (void)hipFree(g->sources);
    delete g;
    return CRH_OK;
}

int crh_graph_count(crh_graph *g, int rel, int64_t *nodes_out, int64_t *edges_out)
{
    if (!g) return fail(CRH_E_INVALID, "graph handle is NULL");
    if (rel < 0 || rel >= CRH_GRAPH_MAX_RELATIONS) return fail(CRH_E_INVALID, "graph_count: relation %d outside 0..%d", rel, CRH_GRAPH_MAX_RELATIONS - 1);
    if (nodes_out) *nodes_out = g->n_nodes;
    if (edges_out) *edges_out = g->rel[rel].set ? g->rel[rel].n_edges : -1;
    return CRH_OK;
}

int crh_graph_set_relation(crh_graph *g, int rel, int64_t n_edges, const int64_t *off_fwd_host, const int32_t *adj_fwd_host,
                           const int64_t *off_rev_host, const int32_t *adj_rev_host)
{
    if (!g) return fail(CRH_E_INVALID, "graph handle is NULL");
    if (rel < 0 || rel >= CRH_GRAPH_MAX_RELATIONS) return fail(CRH_E_INVALID, "graph_set_relation: relation %d outside 0..%d", rel, CRH_GRAPH_MAX_RELATIONS - 1);
    if (n_edges < 0) return fail(CRH_E_INVALID, "graph_set_relation: n_edges=%lld is negative", (long long)n_edges);
    CRH_TRY(check_csr("forward", g->n_nodes, n_edges, off_fwd_host, adj_fwd_host));
    CRH_TRY(check_csr("reverse", g->n_nodes, n_edges, off_rev_host, adj_rev_host));
    DeviceGuard guard(g->device);
    CRH_HIP(hipDeviceSynchronize());       // (a traversal in flight reads the arrays this call releases)
    crh_graph_relation fresh;
    const int64_t *offs[2] = {off_fwd_host, off_rev_host};
    const int32_t *adjs[2] = {adj_fwd_host, adj_rev_host};
    int rc = CRH_OK;
    for (int c = 0; c < 2 && rc == CRH_OK; ++c) {
        void *po = nullptr, *pa = nullptr;
        rc = graph_alloc(&po, (g->n_nodes + 1) * 8);
        fresh.off[c] = static_cast<int64_t *>(po);
        if (rc == CRH_OK) rc = graph_alloc(&pa, n_edges * 4);
        fresh.adj[c] = static_cast<int32_t *>(pa);
        if (rc == CRH_OK && hipMemcpy(fresh.off[c], offs[c], (size_t)(g->n_nodes + 1) * 8, hipMemcpyHostToDevice) != hipSuccess)
            rc = fail(CRH_E_HIP, "graph_set_relation: the upload of the offsets failed");
        if (rc == CRH_OK && n_edges > 0 && hipMemcpy(fresh.adj[c], adjs[c], (size_t)n_edges * 4, hipMemcpyHostToDevice) != hipSuccess)
            rc = fail(CRH_E_HIP, "graph_set_relation: the upload of the adjacency failed");
    }
    if (rc != CRH_OK) {
        graph_free_relation(fresh);
        return rc;                          // (the relation as it was stays)
    }
    graph_free_relation(g->rel[rel]);
    graph_drop_inv(g, rel);                 // (1 / out(v) of the edges that leave)
    fresh.set = true;
    fresh.n_edges = n_edges;
    g->rel[rel] = fresh;
    return CRH_OK;
}

}  // extern "C"

namespace {

// crh_graph_bfs and crh_graph_bfs_avoiding: `avoid` NULL launches the kernels without the avoided-node test.
int graph_bfs_run(const char *who, crh_graph *g, int rel, int direction, int nq, const int64_t *src_off_host, const int32_t *src_nodes, int sources_on_device,
                  int max_hops, int include_self, const uint64_t *avoid_dev, uint64_t *levels_dev, uint64_t *seen_dev, uint64_t *active_dev, void *stream)
{
    CRH_TRY(graph_check_rel(g, rel, direction, who));
    CRH_TRY(check_nq(who, nq));
    CRH_TRY(check_hops(who, max_hops));
    if (!src_off_host) return fail(CRH_E_INVALID, "%s: NULL pointer", who);
    if (src_off_host[0] != 0) return fail(CRH_E_INVALID, "%s: src_off[0]=%lld, not 0", who, (long long)src_off_host[0]);
    for (int q = 0; q < nq; ++q)
        if (src_off_host[q + 1] < src_off_host[q]) return fail(CRH_E_INVALID, "%s: src_off decreases at query %d", who, q);
    const int64_t total = src_off_host[nq];
    if (total > 0 && !src_nodes) return fail(CRH_E_INVALID, "%s: NULL pointer", who);
    if (!sources_on_device)
        for (int64_t i = 0; i < total; ++i)
            if (src_nodes[i] < -1 || src_nodes[i] >= g->n_nodes)
                return fail(CRH_E_INVALID, "%s: source %lld names node %d of %lld", who, (long long)i, src_nodes[i], (long long)g->n_nodes);
    const int64_t n = g->n_nodes;
    if (n == 0) return CRH_OK;
    if (!levels_dev || !seen_dev || !active_dev) return fail(CRH_E_INVALID, "%s: NULL pointer", who);
    DeviceGuard guard(g->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    u64 *levels = reinterpret_cast<u64 *>(levels_dev), *seen = reinterpret_cast<u64 *>(seen_dev), *active = reinterpret_cast<u64 *>(active_dev);
    const int32_t *nodes_dev = src_nodes;
    if (!sources_on_device && total > 0) {
        CRH_TRY(graph_stage(&g->sources, &g->cap_sources, total * 4, 1024 * 4, st, {src_nodes}));
        nodes_dev = static_cast<const int32_t *>(g->sources);
    }
    CRH_HIP(hipMemsetAsync(levels, 0, (size_t)(max_hops + 1) * (size_t)n * 8, st));
    CRH_HIP(hipMemsetAsync(active, 0, (size_t)(max_hops + 1) * 8, st));
    if (total > 0) {
        SourceArgs sa{};
        for (int q = 0; q <= nq; ++q) sa.off[q] = src_off_host[q];
        sa.nodes = nodes_dev;
        sa.nq = nq;
        sa.n_nodes = n;
        sa.level0 = levels;
        sa.active0 = active;
        sa.avoid = reinterpret_cast<const u64 *>(avoid_dev);
        if (avoid_dev)
            hipLaunchKernelGGL(k_graph_sources<true>, dim3(graph_blocks(total, kGraphThreads)), dim3(kGraphThreads), 0, st, sa);
        else
            hipLaunchKernelGGL(k_graph_sources<false>, dim3(graph_blocks(total, kGraphThreads)), dim3(kGraphThreads), 0, st, sa);
    }
    CRH_HIP(hipMemcpyAsync(seen, levels, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
    LevelArgs la{};
    la.ncsr = graph_pull(g, rel, direction, la.off, la.adj);
    la.seen = seen;
    la.n = n;
    la.qmask = query_mask(nq);
    la.avoid = reinterpret_cast<const u64 *>(avoid_dev);
    const unsigned blocks = graph_blocks(n, kGraphThreads);
    for (int d = 1; d <= max_hops; ++d) {
        la.front = levels + (int64_t)(d - 1) * n;
        la.next = levels + (int64_t)d * n;
        la.active_prev = active + (d - 1);
        la.active_cur = active + d;
        if (avoid_dev)
            hipLaunchKernelGGL(k_graph_level<true>, dim3(blocks), dim3(kGraphThreads), 0, st, la);
        else
            hipLaunchKernelGGL(k_graph_level<false>, dim3(blocks), dim3(kGraphThreads), 0, st, la);
    }
    if (!include_self) hipLaunchKernelGGL(k_graph_unself, dim3(blocks), dim3(kGraphThreads), 0, st, levels, seen, n);
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

}  // namespace

extern "C" {

int crh_graph_bfs(crh_graph *g, int rel, int direction, int nq, const int64_t *src_off_host, const int32_t *src_nodes, int sources_on_device,
                  int max_hops, int include_self, uint64_t *levels_dev, uint64_t *seen_dev, uint64_t *active_dev, void *stream)
{
    return graph_bfs_run("graph_bfs", g, rel, direction, nq, src_off_host, src_nodes, sources_on_device, max_hops, include_self, nullptr, levels_dev, seen_dev,
                         active_dev, stream);
}

int crh_graph_bfs_avoiding(crh_graph *g, int rel, int direction, int nq, const int64_t *src_off_host, const int32_t *src_nodes, int sources_on_device,
                           int max_hops, int include_self, const uint64_t *avoid_dev, uint64_t *levels_dev, uint64_t *seen_dev, uint64_t *active_dev,
                           void *stream)
{
    if (g && g->n_nodes > 0 && !avoid_dev) return fail(CRH_E_INVALID, "graph_bfs_avoiding: NULL pointer");
    return graph_bfs_run("graph_bfs_avoiding", g, rel, direction, nq, src_off_host, src_nodes, sources_on_device, max_hops, include_self, avoid_dev, levels_dev,
                         seen_dev, active_dev, stream);
}

int crh_graph_list(crh_graph *g, int nq, const uint64_t *levels_dev, int max_hops, int first_level, int limit, int32_t *out_nodes_dev,
                   int32_t *out_depth_dev, int64_t *out_count_dev, void *stream)
{
    if (!g) return fail(CRH_E_INVALID, "graph handle is NULL");
    CRH_TRY(check_nq("graph_list", nq));
    CRH_TRY(check_hops("graph_list", max_hops));
    if (first_level < 0 || first_level > max_hops) return fail(CRH_E_INVALID, "graph_list: first_level=%d outside 0..%d", first_level, max_hops);
    if (limit < 0 || limit > CRH_GRAPH_MAX_LIMIT) return fail(CRH_E_INVALID, "graph_list: limit=%d outside 0..%d", limit, CRH_GRAPH_MAX_LIMIT);
    if (!out_count_dev || (limit > 0 && (!out_nodes_dev || !out_depth_dev)) || (g->n_nodes > 0 && !levels_dev))
        return fail(CRH_E_INVALID, "graph_list: NULL pointer");
    DeviceGuard guard(g->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_graph_list, dim3((unsigned)nq), dim3(kGraphThreads), 0, st, reinterpret_cast<const u64 *>(levels_dev), g->n_nodes, first_level,
                       max_hops, limit, out_nodes_dev, out_depth_dev, out_count_dev);
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

int crh_graph_row_words(const int32_t *row_node_dev, int64_t n_rows, const uint64_t *seen_dev, int64_t n_nodes, int q, uint32_t *out_words_dev,
                        int64_t n_words, void *stream)
{
    if (n_rows < 0 || n_rows >= (1LL << 31) || n_nodes < 0) return fail(CRH_E_INVALID, "graph_row_words: n_rows=%lld, n_nodes=%lld", (long long)n_rows, (long long)n_nodes);
    CRH_TRY(check_q("graph_row_words", q));
    if (n_words < ceil_div(n_rows, 32)) return fail(CRH_E_INVALID, "graph_row_words: %lld words for %lld rows", (long long)n_words, (long long)n_rows);
    if (n_words == 0) return CRH_OK;
    if (!out_words_dev || (n_rows > 0 && (!row_node_dev || (n_nodes > 0 && !seen_dev)))) return fail(CRH_E_INVALID, "graph_row_words: NULL pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_graph_row_words, dim3(graph_blocks((n_words + 1) / 2, kGraphWaves)), dim3(kGraphThreads), 0, st, row_node_dev, n_rows,
                       reinterpret_cast<const u64 *>(seen_dev), n_nodes, q, out_words_dev, n_words);
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

int crh_graph_path(crh_graph *g, int rel, int direction, const uint64_t *levels_dev, int q, int64_t target, int max_hops, int32_t *out_nodes_host,
                   int *out_len, void *stream)
{
    CRH_TRY(graph_check_rel(g, rel, direction, "graph_path"));
    if (!out_len || !out_nodes_host) return fail(CRH_E_INVALID, "graph_path: NULL pointer");
    *out_len = 0;
    CRH_TRY(check_q("graph_path", q));
    CRH_TRY(check_hops("graph_path", max_hops));
    if (target < 0 || target >= g->n_nodes) return fail(CRH_E_INVALID, "graph_path: target=%lld is no node of %lld", (long long)target, (long long)g->n_nodes);
    if (!levels_dev) return fail(CRH_E_INVALID, "graph_path: NULL pointer");
    DeviceGuard guard(g->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    PathArgs a{};
    a.ncsr = graph_pull(g, rel, direction, a.off, a.adj);
    a.levels = reinterpret_cast<const u64 *>(levels_dev);
    a.n = g->n_nodes;
    a.q = q;
    a.target = target;
    a.max_hops = max_hops;
    a.out = g->path;
    hipLaunchKernelGGL(k_graph_path, dim3(1), dim3(64), 0, st, a);
    CRH_HIP(hipGetLastError());
    int32_t got[CRH_GRAPH_MAX_HOPS + 2] = {};
    CRH_HIP(hipMemcpyAsync(got, g->path, sizeof got, hipMemcpyDeviceToHost, st));
    CRH_HIP(hipStreamSynchronize(st));
    const int len = got[0];
    if (len < 0 || len > max_hops + 1) return fail(CRH_E_INTERNAL, "graph_path: a path of %d nodes", len);
    for (int i = 0; i < len; ++i) out_nodes_host[i] = got[1 + i];
    *out_len = len;
    return CRH_OK;
}

int crh_graph_ppr(crh_graph *g, int rel, int direction, int nq, int c, const int32_t *seed_nodes, const float *seed_weights, int seeds_on_device,
                  float restart, int steps, float *work_dev, float *out_dev, void *stream)
{
    CRH_TRY(graph_check_rel(g, rel, direction, "graph_ppr"));
    CRH_TRY(check_nq("graph_ppr", nq));
    if (c < 1 || c > CRH_MAX_K) return fail(CRH_E_INVALID, "graph_ppr: c=%d outside 1..%d", c, CRH_MAX_K);
    if (steps < 1 || steps > CRH_GRAPH_PPR_MAX_STEPS) return fail(CRH_E_INVALID, "graph_ppr: steps=%d outside 1..%d", steps, CRH_GRAPH_PPR_MAX_STEPS);
    if (!(restart > 0.0f && restart < 1.0f)) return fail(CRH_E_INVALID, "graph_ppr: restart=%g is not inside (0, 1)", (double)restart);
    if (!seed_nodes) return fail(CRH_E_INVALID, "graph_ppr: NULL pointer");
    const int64_t n = g->n_nodes, total = (int64_t)nq * c;
    if (!seeds_on_device)
        for (int64_t i = 0; i < total; ++i) {
            if (seed_nodes[i] < -1 || seed_nodes[i] >= n)
                return fail(CRH_E_INVALID, "graph_ppr: seed %lld names node %d of %lld", (long long)i, seed_nodes[i], (long long)n);
            if (seed_weights && !(seed_weights[i] >= 0.0f && seed_weights[i] < __builtin_inff()))
                return fail(CRH_E_INVALID, "graph_ppr: weight %lld is %g, not a finite value >= 0", (long long)i, (double)seed_weights[i]);
        }
    if (n == 0) return CRH_OK;
    if (!work_dev || !out_dev) return fail(CRH_E_INVALID, "graph_ppr: NULL pointer");
    DeviceGuard guard(g->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int shift = layout_shift(nq);
    const int64_t plane = n << shift;
    float *&inv = g->inv[rel][direction];
    if (!inv) {                              // built once per (relation, direction); crh_graph_set_relation drops it
        void *p = nullptr;
        CRH_TRY(graph_alloc(&p, n * 4));
        const crh_graph_relation &r = g->rel[rel];
        const int64_t *o0 = direction == CRH_GRAPH_AGAINST ? r.off[1] : r.off[0];            // out(v): the OPPOSITE list or lists
        const int64_t *o1 = direction == CRH_GRAPH_BOTH ? r.off[1] : nullptr;
        hipLaunchKernelGGL(k_ppr_inv, dim3(graph_blocks(n, kGraphThreads)), dim3(kGraphThreads), 0, st, o0, o1, n, static_cast<float *>(p));
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {     // (another stream may use it next)
            (void)hipFree(p);
            return fail(CRH_E_HIP, "graph_ppr: building 1 / out(v) failed");
        }
        inv = static_cast<float *>(p);
    }
    const int32_t *nodes_dev = seed_nodes;
    const float *weights_dev = seed_weights;
    if (!seeds_on_device) {
        CRH_TRY(graph_stage(&g->seeds, &g->cap_seeds, total * 4, 4096 * 8, st, {seed_nodes, seed_weights}));
        nodes_dev = static_cast<const int32_t *>(g->seeds);
        weights_dev = seed_weights ? reinterpret_cast<const float *>(nodes_dev + total) : nullptr;
    }
    float *p0 = work_dev, *ping = work_dev + plane, *pong = work_dev + 2 * plane;
    CRH_HIP(hipMemsetAsync(p0, 0, (size_t)plane * 2 * 4, st));       // p0 and contrib_0: +0 wherever no seed lands
    hipLaunchKernelGGL(k_ppr_seed, dim3((unsigned)nq), dim3(kGraphThreads), 0, st, nodes_dev, weights_dev, c, n, shift, inv, p0, ping);
    PprStepArgs sa{};
    sa.ncsr = graph_pull(g, rel, direction, sa.off, sa.adj);
    sa.p0 = p0;
    sa.inv = inv;
    sa.p = out_dev;
    sa.n = n;
    sa.shift = shift;
    sa.restart = restart;
    sa.a = 1.0f - restart;
    const unsigned blocks = graph_blocks(ceil_div(n, 64 >> shift), kGraphWaves);
    for (int t = 0; t < steps; ++t) {
        sa.contrib = (t & 1) ? pong : ping;
        sa.next = (t & 1) ? ping : pong;
        if (shift == 6)
            hipLaunchKernelGGL(k_ppr_step<true>, dim3(blocks), dim3(kGraphThreads), 0, st, sa);
        else
            hipLaunchKernelGGL(k_ppr_step<false>, dim3(blocks), dim3(kGraphThreads), 0, st, sa);
    }
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

int crh_graph_ppr_bins(int64_t n_nodes, int nq, const float *scores_dev, int c, const int32_t *exclude_dev, int64_t *out_bins_dev, void *stream)
{
    CRH_TRY(check_n_nodes("graph_ppr_bins", n_nodes));
    CRH_TRY(check_nq("graph_ppr_bins", nq));
    if (c < 0 || c > CRH_MAX_K || (c > 0 && !exclude_dev)) return fail(CRH_E_INVALID, "graph_ppr_bins: %d exclusions per query (0..%d) at %p", c, CRH_MAX_K, (const void *)exclude_dev);
    if (n_nodes == 0) return CRH_OK;
    if (!scores_dev || !out_bins_dev) return fail(CRH_E_INVALID, "graph_ppr_bins: NULL pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_ppr_bins, dim3(graph_blocks(n_nodes, 64)), dim3(kGraphThreads), 0, st, scores_dev, n_nodes, layout_shift(nq), nq, out_bins_dev);
    if (c > 0)
        hipLaunchKernelGGL(k_ppr_bins_exclude, dim3(graph_blocks((int64_t)nq * c, kGraphThreads)), dim3(kGraphThreads), 0, st, exclude_dev, nq, c, n_nodes,
                           out_bins_dev);
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

int crh_graph_ppr_order(int64_t n_nodes, int nq, int c, const float *scores_dev, const int64_t *rows_dev, const float *cosine_dev,
                        const int32_t *nodes_dev, float *out_fuse_scores_dev, int64_t *out_fuse_rows_dev, float *out_graph_score_dev, void *stream)
{
    CRH_TRY(check_n_nodes("graph_ppr_order", n_nodes));
    CRH_TRY(check_nq("graph_ppr_order", nq));
    if (c < 1 || c > CRH_MAX_K) return fail(CRH_E_INVALID, "graph_ppr_order: c=%d outside 1..%d", c, CRH_MAX_K);
    if (!rows_dev || !cosine_dev || !nodes_dev || !out_fuse_scores_dev || !out_fuse_rows_dev || !out_graph_score_dev || (n_nodes > 0 && !scores_dev))
        return fail(CRH_E_INVALID, "graph_ppr_order: NULL pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_ppr_order, dim3((unsigned)nq), dim3(kGraphThreads), 0, st, scores_dev, n_nodes, layout_shift(nq), c, rows_dev, cosine_dev, nodes_dev,
                       out_fuse_scores_dev, out_fuse_rows_dev, out_graph_score_dev);
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

}  // extern "C"

namespace {

// Enqueues sweeps, kSweepBatch per read-back of their flag words, until one changes nothing.  `launch(prev, cur)` enqueues one
// sweep that leaves at once when bit 0 of *prev is clear and ORs its own flags into *cur.  `ran` counts the sweeps that did
// run, `launched` all of them; the loop never goes past `cap` sweeps that ran (CRH_E_INTERNAL).  *last = the flags of the sweep
// that changed nothing.
template <class L>
int sweep_to_fixed_point(L launch, unsigned *flags, hipStream_t st, int64_t cap, int64_t &ran, int64_t &launched, unsigned *last, const char *who)
{
    unsigned host[kSweepBatch + 1];
    while (ran < cap) {                                              // (every pass adds at least one to `ran`)
        const int batch = (int)std::min<int64_t>(kSweepBatch, cap - ran);
        CRH_HIP(hipMemsetAsync(flags, 0, sizeof host, st));
        CRH_HIP(hipMemsetAsync(flags, 1, 4, st));                    // flags[0] != 0: the first sweep of a batch always runs
        for (int i = 0; i < batch; ++i) launch(flags + i, flags + i + 1);
        launched += batch;
        CRH_HIP(hipGetLastError());
        CRH_HIP(hipMemcpyAsync(host, flags, sizeof host, hipMemcpyDeviceToHost, st));
        CRH_HIP(hipStreamSynchronize(st));
        for (int i = 1; i <= batch; ++i) {
            ++ran;
            if ((host[i] & 1u) == 0u) {
                *last = host[i];
                return CRH_OK;
            }
        }
    }
    return fail(CRH_E_INTERNAL, "%s: no fixed point within %lld sweeps", who, (long long)cap);
}

}  // namespace

extern "C" {

int crh_graph_scc(crh_graph *g, int rel, int32_t *comp_out_dev, int32_t *work_dev, int64_t *info_host, void *stream)
{
    CRH_TRY(graph_check_rel(g, rel, CRH_GRAPH_ALONG, "graph_scc"));
    if (!info_host) return fail(CRH_E_INVALID, "graph_scc: NULL pointer");
    info_host[0] = info_host[1] = info_host[2] = info_host[3] = 0;
    const int64_t n = g->n_nodes;
    if (n == 0) return CRH_OK;
    if (!comp_out_dev || !work_dev) return fail(CRH_E_INVALID, "graph_scc: NULL pointer");
    DeviceGuard guard(g->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const crh_graph_relation &r = g->rel[rel];
    SccArgs a{};
    a.off_out = r.off[0];
    a.adj_out = r.adj[0];
    a.off_in = r.off[1];
    a.adj_in = r.adj[1];
    a.comp = comp_out_dev;
    a.colour = work_dev;
    a.n = n;
    unsigned *flags = reinterpret_cast<unsigned *>(work_dev + n);
    unsigned *counters = reinterpret_cast<unsigned *>(work_dev + n) + kSccCounters;
    const unsigned blocks = graph_blocks(n, kGraphThreads);
    const int64_t cap = CRH_GRAPH_SCC_MAX_SWEEPS(n);
    int64_t ran = 0, launched = 0;
    auto sweep = [&](void (*kernel)(const SccArgs)) {
        return [&, kernel](const unsigned *prev, unsigned *cur) {
            a.prev = prev;
            a.cur = cur;
            hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kGraphThreads), 0, st, a);
        };
    };
    CRH_HIP(hipMemsetAsync(comp_out_dev, 0xff, (size_t)n * 4, st));  // -1: unassigned
    bool done = false;
    for (int64_t round = 0; round <= n && !done; ++round) {          // (a round that finds a node left assigns its colour's root at least)
        unsigned last = 0u;
        CRH_TRY(sweep_to_fixed_point(sweep(k_scc_trim), flags, st, cap, ran, launched, &last, "graph_scc"));
        if ((last & 2u) == 0u) {
            done = true;
            break;
        }
        hipLaunchKernelGGL(k_scc_colour_init, dim3(blocks), dim3(kGraphThreads), 0, st, comp_out_dev, work_dev, n);
        CRH_TRY(sweep_to_fixed_point(sweep(k_scc_colour), flags, st, cap, ran, launched, &last, "graph_scc"));
        hipLaunchKernelGGL(k_scc_roots, dim3(blocks), dim3(kGraphThreads), 0, st, comp_out_dev, work_dev, n);
        CRH_TRY(sweep_to_fixed_point(sweep(k_scc_mark), flags, st, cap, ran, launched, &last, "graph_scc"));
    }
    if (!done) return fail(CRH_E_INTERNAL, "graph_scc: nodes left after %lld rounds", (long long)n + 1);
    CRH_HIP(hipMemsetAsync(work_dev, 0, (size_t)n * 4, st));         // the colours are spent: which labels have a second member
    CRH_HIP(hipMemsetAsync(counters, 0, 16, st));
    hipLaunchKernelGGL(k_scc_members, dim3(blocks), dim3(kGraphThreads), 0, st, comp_out_dev, work_dev, n, counters);
    hipLaunchKernelGGL(k_scc_count, dim3(blocks), dim3(kGraphThreads), 0, st, comp_out_dev, work_dev, n, counters);
    CRH_HIP(hipGetLastError());
    unsigned got[4] = {};
    CRH_HIP(hipMemcpyAsync(got, counters, sizeof got, hipMemcpyDeviceToHost, st));
    CRH_HIP(hipStreamSynchronize(st));
    info_host[0] = got[0];
    info_host[1] = got[1];
    info_host[2] = (int64_t)got[1] + got[2];                         // a component of two or more: its label and the others
    info_host[3] = launched;
    return CRH_OK;
}

int crh_graph_scc_bins(int64_t n_nodes, const int32_t *comp_dev, const int32_t *self_nodes_dev, int64_t n_self, int64_t *out_bins_dev, void *stream)
{
    CRH_TRY(check_n_nodes("graph_scc_bins", n_nodes));
    if (n_self < 0 || n_self > n_nodes || (n_self > 0 && !self_nodes_dev))
        return fail(CRH_E_INVALID, "graph_scc_bins: %lld self-loop nodes (0..%lld) at %p", (long long)n_self, (long long)n_nodes, (const void *)self_nodes_dev);
    if (n_nodes == 0) return CRH_OK;
    if (!comp_dev || !out_bins_dev) return fail(CRH_E_INVALID, "graph_scc_bins: NULL pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    u64 *bins = reinterpret_cast<u64 *>(out_bins_dev);
    CRH_HIP(hipMemsetAsync(bins, 0, (size_t)n_nodes * 8, st));
    const unsigned blocks = graph_blocks(n_nodes, kGraphThreads);
    hipLaunchKernelGGL(k_scc_bins_count, dim3(blocks), dim3(kGraphThreads), 0, st, comp_dev, n_nodes, bins);
    hipLaunchKernelGGL(k_scc_bins_keep, dim3(blocks), dim3(kGraphThreads), 0, st, self_nodes_dev, n_self, n_nodes, bins);
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

int crh_graph_layers(crh_graph *g, int rel, int direction, const int32_t *comp_dev, int32_t *out_dev, int32_t *work_dev, int64_t *info_host, void *stream)
{
    CRH_TRY(graph_check_rel(g, rel, direction, "graph_layers"));
    if (direction == CRH_GRAPH_BOTH) return fail(CRH_E_INVALID, "graph_layers: direction is CRH_GRAPH_ALONG or CRH_GRAPH_AGAINST (taken both ways every edge lies on a cycle)");
    if (!info_host) return fail(CRH_E_INVALID, "graph_layers: NULL pointer");
    info_host[0] = info_host[1] = 0;
    const int64_t n = g->n_nodes;
    if (n == 0) return CRH_OK;
    if (!comp_dev || !out_dev || !work_dev) return fail(CRH_E_INVALID, "graph_layers: NULL pointer");
    DeviceGuard guard(g->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    LayerArgs a{};
    graph_pull_one(g, rel, direction, &a.off, &a.adj);
    a.comp = comp_dev;
    a.layer = out_dev;
    a.n = n;
    unsigned *flags = reinterpret_cast<unsigned *>(work_dev);
    int *most = reinterpret_cast<int *>(work_dev) + kSccCounters;
    const unsigned blocks = graph_blocks(n, kGraphThreads);
    int64_t ran = 0, launched = 0;
    unsigned last = 0u;
    CRH_HIP(hipMemsetAsync(out_dev, 0, (size_t)n * 4, st));
    CRH_TRY(sweep_to_fixed_point(
        [&](const unsigned *prev, unsigned *cur) {
            a.prev = prev;
            a.cur = cur;
            hipLaunchKernelGGL(k_graph_layer, dim3(blocks), dim3(kGraphThreads), 0, st, a);
        },
        flags, st, CRH_GRAPH_LAYERS_MAX_SWEEPS(n), ran, launched, &last, "graph_layers"));
    CRH_HIP(hipMemsetAsync(most, 0, 4, st));
    hipLaunchKernelGGL(k_graph_layer_max, dim3(blocks), dim3(kGraphThreads), 0, st, out_dev, n, most);
    CRH_HIP(hipGetLastError());
    int got = 0;
    CRH_HIP(hipMemcpyAsync(&got, most, 4, hipMemcpyDeviceToHost, st));
    CRH_HIP(hipStreamSynchronize(st));
    info_host[0] = (int64_t)got + 1;
    info_host[1] = launched;
    return CRH_OK;
}

int crh_graph_node_words(int64_t n_nodes, int mode, const int32_t *values_dev, const int64_t *bins_dev, int64_t lo, int64_t hi, int q,
                         uint64_t *out_words_dev, void *stream)
{
    CRH_TRY(check_n_nodes("graph_node_words", n_nodes));
    if (mode != CRH_GRAPH_WORDS_IN_CYCLE && mode != CRH_GRAPH_WORDS_SAME_COMPONENT && mode != CRH_GRAPH_WORDS_RANGE)
        return fail(CRH_E_INVALID, "graph_node_words: mode=%d is none of CRH_GRAPH_WORDS_*", mode);
    CRH_TRY(check_q("graph_node_words", q));
    if (n_nodes == 0) return CRH_OK;
    if (!values_dev || !out_words_dev || (mode == CRH_GRAPH_WORDS_IN_CYCLE && !bins_dev)) return fail(CRH_E_INVALID, "graph_node_words: NULL pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_graph_node_words, dim3(graph_blocks(n_nodes, kGraphThreads)), dim3(kGraphThreads), 0, st, n_nodes, mode, values_dev, bins_dev, lo, hi, q,
                       reinterpret_cast<u64 *>(out_words_dev));
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

}  // extern "C"

// ---- chains in full

namespace {

// What the chain calls share: a set relation, ALONG or AGAINST, 1..64 queries, 1..16 hops.
int chains_check(const char *who, crh_graph *g, int rel, int direction, int nq, int max_hops)
{
    CRH_TRY(graph_check_rel(g, rel, direction, who));
    if (direction == CRH_GRAPH_BOTH)
        return fail(CRH_E_INVALID, "%s: direction is CRH_GRAPH_ALONG or CRH_GRAPH_AGAINST (taken both ways a chain may turn back on itself)", who);
    CRH_TRY(check_nq(who, nq));
    return check_hops(who, max_hops);
}

}  // namespace

extern "C" {

int crh_graph_sigma(crh_graph *g, int rel, int direction, int nq, const uint64_t *levels_dev, const uint64_t *active_dev, int max_hops,
                    uint64_t *sigma_out_dev, void *stream)
{
    CRH_TRY(chains_check("graph_sigma", g, rel, direction, nq, max_hops));
    const int64_t n = g->n_nodes;
    if (n == 0) return CRH_OK;
    if (!levels_dev || !active_dev || !sigma_out_dev) return fail(CRH_E_INVALID, "graph_sigma: NULL pointer");
    DeviceGuard guard(g->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const u64 *levels = reinterpret_cast<const u64 *>(levels_dev);
    SigmaArgs a{};
    graph_pull_one(g, rel, direction, &a.off, &a.adj);
    a.sigma = reinterpret_cast<u64 *>(sigma_out_dev);
    a.n = n;
    a.shift = layout_shift(nq);
    a.qmask = query_mask(nq);
    hipLaunchKernelGGL(k_sigma_init, dim3(graph_blocks(n << a.shift, kGraphThreads)), dim3(kGraphThreads), 0, st, levels, n, a.shift, a.qmask, a.sigma);
    const unsigned blocks = graph_blocks(ceil_div(n, 64 >> a.shift), kGraphWaves);
    for (int d = 1; d <= max_hops; ++d) {
        a.cur = levels + (int64_t)d * n;
        a.prev = levels + (int64_t)(d - 1) * n;
        a.active = reinterpret_cast<const u64 *>(active_dev) + d;
        if (a.shift == 6)
            hipLaunchKernelGGL(k_sigma_level<true>, dim3(blocks), dim3(kGraphThreads), 0, st, a);
        else
            hipLaunchKernelGGL(k_sigma_level<false>, dim3(blocks), dim3(kGraphThreads), 0, st, a);
    }
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

int crh_graph_chains(crh_graph *g, int rel, int direction, int nq, const uint64_t *levels_dev, const uint64_t *sigma_dev, int max_hops,
                     const int32_t *targets, int targets_on_device, int K, int32_t *out_nodes_dev, int32_t *out_len_dev, uint64_t *out_count_dev,
                     void *stream)
{
    CRH_TRY(chains_check("graph_chains", g, rel, direction, nq, max_hops));
    if (K < 1 || K > CRH_GRAPH_MAX_CHAINS) return fail(CRH_E_INVALID, "graph_chains: K=%d outside 1..%d", K, CRH_GRAPH_MAX_CHAINS);
    if (!targets) return fail(CRH_E_INVALID, "graph_chains: NULL pointer");
    const int64_t n = g->n_nodes;
    if (!targets_on_device)
        for (int q = 0; q < nq; ++q)
            if (targets[q] < -1 || targets[q] >= n) return fail(CRH_E_INVALID, "graph_chains: target %d names node %d of %lld", q, targets[q], (long long)n);
    if (n == 0) return CRH_OK;
    if (!levels_dev || !sigma_dev || !out_nodes_dev || !out_len_dev || !out_count_dev) return fail(CRH_E_INVALID, "graph_chains: NULL pointer");
    DeviceGuard guard(g->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    ChainArgs a{};
    graph_pull_one(g, rel, direction, &a.off, &a.adj);
    a.levels = reinterpret_cast<const u64 *>(levels_dev);
    a.sigma = reinterpret_cast<const u64 *>(sigma_dev);
    a.n = n;
    a.shift = layout_shift(nq);
    a.nq = nq;
    a.max_hops = max_hops;
    a.K = K;
    if (targets_on_device)
        a.dev_targets = targets;
    else
        for (int q = 0; q < nq; ++q) a.host_targets[q] = targets[q];
    a.out_nodes = out_nodes_dev;
    a.out_len = out_len_dev;
    a.out_count = reinterpret_cast<u64 *>(out_count_dev);
    hipLaunchKernelGGL(k_graph_chains, dim3((unsigned)ceil_div((int64_t)nq * K, kGraphWaves)), dim3(kGraphThreads), 0, st, a);
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

int crh_graph_between(int64_t n_nodes, int nq, const uint64_t *levels_fwd_dev, const uint64_t *levels_back_dev, int max_hops, int mode, uint64_t *meet_dev,
                      uint64_t *out_words_dev, int32_t *out_dist_dev, void *stream)
{
    CRH_TRY(check_n_nodes("graph_between", n_nodes));
    CRH_TRY(check_nq("graph_between", nq));
    CRH_TRY(check_hops("graph_between", max_hops));
    if (mode != CRH_GRAPH_BETWEEN_ANY && mode != CRH_GRAPH_BETWEEN_SHORTEST) return fail(CRH_E_INVALID, "graph_between: mode=%d is none of CRH_GRAPH_BETWEEN_*", mode);
    if (n_nodes == 0) return CRH_OK;
    if (!levels_fwd_dev || !levels_back_dev || !meet_dev || !out_words_dev) return fail(CRH_E_INVALID, "graph_between: NULL pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    BetweenArgs a{};
    a.fwd = reinterpret_cast<const u64 *>(levels_fwd_dev);
    a.back = reinterpret_cast<const u64 *>(levels_back_dev);
    a.n = n_nodes;
    a.max_hops = max_hops;
    a.mode = mode;
    a.nq = nq;
    a.meet = reinterpret_cast<u64 *>(meet_dev);
    a.out = reinterpret_cast<u64 *>(out_words_dev);
    a.dist = out_dist_dev;
    CRH_HIP(hipMemsetAsync(a.meet, 0, (size_t)(max_hops + 1) * 8, st));
    const unsigned blocks = graph_blocks(n_nodes, kGraphThreads);
    hipLaunchKernelGGL(k_between_meet, dim3(blocks), dim3(kGraphThreads), 0, st, a);
    hipLaunchKernelGGL(k_between_out, dim3(blocks), dim3(kGraphThreads), 0, st, a);
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

}  // extern "C"
