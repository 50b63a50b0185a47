// crh_rerank_hybrid.hip -- the hybrid re-rank with BOTH branches on the device: graph results and vector hits in one list.
//
// crh_rerank.hip restates HybridRanker.rank_results for candidate lists that hold vector hits only.  The reference never ranks
// that way: QueryEngine.search (src/lattice/query/engine.py:222-260) gathers a graph context and the vector hits side by side,
// and rank_results (query/ranking/ranker.py:24-54) scores the graph nodes role by role (scorer.py:9-77), the vector hits after
// them (scorer.py:80-126), lets the first entry of a file:entity:start_line key absorb the later ones (ranker.py:171-202), sorts
// (:46-48) and caps (:204-229).  With the call graph in device memory (crh_graph.hip) the graph branch can be built there too:
//
//   crh_graph_node_rows    node -> its lowest alive row (the row whose payload stands for the node in a result)
//   crh_graph_candidates   BFS lists (crh_graph_list) + a host-made segment table -> per query [G] node / row / role / depth
//   crh_rerank_hybrid      G graph entries followed by k vector entries per query -> the ranked survivors
//
// Every float expression is evaluated in f64 with the reference's operand order (-ffp-contract=off), so the scores equal the
// Python result to the last bit; code-rag_amd/ranking/hybrid.py is the host restatement, pinned by the reference's own outputs.
#include "crh_common.h"

namespace crh {
namespace {

__device__ __forceinline__ bool hy_bytes_equal(const uint8_t *a, const uint8_t *b, int n)
{
    for (int i = 0; i < n; ++i)
        if (a[i] != b[i]) return false;
    return true;
}

// `needle in hay` of Python str on UTF-8 bytes, as in crh_rerank.hip (quirk Q8: an empty needle is in every name)
__device__ bool hy_contains(const uint8_t *hay, int hn, const uint8_t *needle, int nn)
{
    if (nn == 0) return true;
    for (int s = 0; s + nn <= hn; ++s)
        if (hy_bytes_equal(hay + s, needle, nn)) return true;
    return false;
}

// one lane per row: out[node] = min(out[node], row_base + local) over the alive rows of this shard.  The array is pre-filled
// with -1, the maximum of the unsigned view, and a minimum does not depend on the order of the lanes or of the shards.
__global__ void k_graph_node_rows(int64_t n_rows, const int32_t *__restrict__ row_node, const uint32_t *__restrict__ alive, int64_t row_base,
                                  int64_t n_nodes, unsigned long long *__restrict__ out)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    if (alive && !((alive[r >> 5] >> (r & 31)) & 1u)) return;
    const int64_t v = row_node[r];
    if (v < 0 || v >= n_nodes) return;
    atomicMin(&out[v], (unsigned long long)(row_base + r));
}

struct CandArgs {
    const crh_graph_segment *segs;   // device copy, sorted by query
    const int32_t *seg_off;          // [nq + 1]
    const int32_t *list_nodes, *list_depth;   // [n_lists][limit]
    const int64_t *node_rows;        // [n_nodes]
    int64_t n_nodes;
    int limit, G;
    int32_t *out_node, *out_role, *out_depth;
    int64_t *out_row;
};

// one WAVE per query: the segments one after the other, 64 entries of a segment at a time, kept entries packed with a ballot
// (order preserved); no LDS, no barrier
__global__ __launch_bounds__(64) void k_graph_candidates(CandArgs a)
{
    const int q = blockIdx.x, lane = threadIdx.x;
    const size_t base = (size_t)q * a.G;
    int filled = 0;
    for (int s = a.seg_off[q]; s < a.seg_off[q + 1]; ++s) {
        const crh_graph_segment sg = a.segs[s];
        const int n = sg.node >= 0 ? 1 : (sg.take < a.limit ? sg.take : a.limit);
        for (int e0 = 0; e0 < n; e0 += 64) {
            const int e = e0 + lane;
            int32_t node = -1, depth = 0;
            if (e < n) {
                if (sg.node >= 0) {
                    node = sg.node;
                } else {
                    node = a.list_nodes[(size_t)sg.list_row * a.limit + e];
                    depth = a.list_depth[(size_t)sg.list_row * a.limit + e];
                }
            }
            int64_t row = -1;
            if (node >= 0 && node < a.n_nodes) row = a.node_rows[node];
            const bool keep = row >= 0;
            const unsigned long long m = __ballot(keep);
            const int slot = filled + __popcll(m & ((1ull << lane) - 1ull));
            if (keep && slot < a.G) {
                a.out_node[base + slot] = node;
                a.out_row[base + slot] = row;
                a.out_role[base + slot] = sg.role;
                a.out_depth[base + slot] = depth;
            }
            filled += __popcll(m);
        }
    }
    for (int slot = (filled < a.G ? filled : a.G) + lane; slot < a.G; slot += 64) {
        a.out_node[base + slot] = -1;
        a.out_row[base + slot] = -1;
        a.out_role[base + slot] = -1;
        a.out_depth[base + slot] = -1;
    }
}

constexpr int NSIG = CRH_RR_HYBRID_SIGNALS;
constexpr int TAB = CRH_RR_HYBRID_TABLE;
// the signals an entry of each source carries (scorer.py:60-74 / :87-92), as bits of the order in the header
constexpr int32_t MASK_GRAPH = 0x1f, MASK_VECTOR = 0x6a;

struct HybridArgs {
    int G, k;
    const int64_t *g_rows;
    const int32_t *g_role, *g_depth, *g_rich;
    crh_rerank_columns g_cols;
    const float *scores;
    const int64_t *rows;
    crh_rerank_columns cols;
    const crh_rerank_hybrid_query *queries;   // device copy
    double bonus;
    int max_per_file, max_total, primary_top, centrality_top, centrality_limit;
    int32_t *out_index;
    double *out_score, *out_signals;
    int32_t *out_mask, *out_count, *out_flags;
};

// one workgroup per query; n = G + k <= CRH_RR_MAX_HYBRID candidates, the graph entries first.  Dynamic LDS per candidate: f64
// final + 7 f64 signals, i32 pos / file / key / signal mask, u8 alive / valid / hybrid / keep: 84 bytes, 42 KB at n = 512.
__global__ __launch_bounds__(256) void k_rerank_hybrid(HybridArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int G = a.G, k = a.k, n = G + k, q = blockIdx.x, tid = threadIdx.x;
    double *fin = reinterpret_cast<double *>(lds);
    double *sig = fin + n;                                   // [NSIG][n]
    int32_t *pos = reinterpret_cast<int32_t *>(sig + NSIG * n);
    int32_t *filec = pos + n;
    int32_t *keyc = filec + n;
    int32_t *maskc = keyc + n;
    uint8_t *alive = reinterpret_cast<uint8_t *>(maskc + n);
    uint8_t *valid = alive + n;                              // a real entry (stays set when the entry is absorbed)
    uint8_t *hybrid = valid + n;
    uint8_t *keepf = hybrid + n;
    __shared__ int32_t tab_node[TAB], tab_deg[TAB];
    __shared__ int tab_n, need_host, total;

    const crh_rerank_hybrid_query &Q = a.queries[q];
    const size_t gb = (size_t)q * G, vb = (size_t)q * k;
    if (tid == 0) {
        // centrality table as engine.py:348-377 builds it (insertion order, engine_helpers.centrality_candidates): the keys of the
        // first primary_top PRIMARY graph entries, then of the first centrality_top named vector hits, one entry per key, cut at
        // centrality_limit names.  A name the graph has no degree for (< 0) takes its place in the cut and answers no lookup.
        int t = 0, overflow = 0, taken = 0;
        for (int i = 0; i < G && taken < a.primary_top && t < a.centrality_limit && !overflow; ++i) {
            if (a.g_rows[gb + i] < 0 || a.g_role[gb + i] != CRH_ROLE_PRIMARY) continue;
            ++taken;
            const int node = a.g_cols.node_code[gb + i];
            bool seen = false;
            for (int u = 0; u < t; ++u) seen = seen || tab_node[u] == node;
            if (seen) continue;
            if (t >= TAB) {
                overflow = 1;
                break;
            }
            tab_node[t] = node;
            tab_deg[t] = a.g_cols.degree[gb + i];
            ++t;
        }
        for (int i = 0; i < k && i < a.centrality_top && t < a.centrality_limit && !overflow; ++i) {
            if (a.rows[vb + i] < 0 || a.cols.name_len[vb + i] <= 0) continue;
            const int node = a.cols.node_code[vb + i];
            bool seen = false;
            for (int u = 0; u < t; ++u) seen = seen || tab_node[u] == node;
            if (seen) continue;
            if (t >= TAB) {
                overflow = 1;
                break;
            }
            tab_node[t] = node;
            tab_deg[t] = a.cols.degree[vb + i];
            ++t;
        }
        tab_n = t;
        need_host = (overflow || Q.base.n_entities < 0 || Q.base.n_entities > CRH_RR_MAX_ENTITIES) ? 1 : 0;
        total = 0;
    }
    __syncthreads();

    for (int i = tid; i < n; i += blockDim.x) {
        const bool graph = i < G;
        const size_t c = graph ? gb + i : vb + (i - G);
        const crh_rerank_columns &cols = graph ? a.g_cols : a.cols;
        const bool ok = (graph ? a.g_rows[c] : a.rows[c]) >= 0;
        alive[i] = ok;
        valid[i] = ok;
        hybrid[i] = 0;
        keepf[i] = 0;
        pos[i] = -1;
        filec[i] = ok ? cols.file_code[c] : 0;
        keyc[i] = ok ? cols.key_code[c] : 0;
        maskc[i] = graph ? MASK_GRAPH : MASK_VECTOR;
        double s[NSIG] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        double f = 0.0;
        if (ok) {
            const int nl = cols.name_len[c];
            const uint8_t *nm = cols.name + c * CRH_RR_NAME_BYTES;
            if (nl > CRH_RR_NAME_BYTES) atomicExch(&need_host, 1);   // only a prefix is here: the host must decide this query
            const int hn = nl < CRH_RR_NAME_BYTES ? nl : CRH_RR_NAME_BYTES;
            bool exact = false, sub = false;
            for (int e = 0; e < Q.base.n_entities && e < CRH_RR_MAX_ENTITIES; ++e) {
                const int el = Q.base.entity_len[e];
                if (el == nl && hy_bytes_equal(nm, Q.base.entity[e], el)) exact = true;
                if (hy_contains(nm, hn, Q.base.entity[e], el)) sub = true;
            }
            s[1] = exact ? 1.0 : sub ? 0.5 : 0.0;                    // scorer.py:31-35, :92-96
            const int node = cols.node_code[c];
            for (int t = 0; t < tab_n; ++t)
                if (tab_node[t] == node) {                            // one entry per key
                    if (tab_deg[t] >= 0) {
                        const double d = (double)tab_deg[t] / 50.0;
                        s[3] = d < 1.0 ? d : 1.0;                     // min(1.0, total_degree / 50), scorer.py:48-54
                    }
                    break;
                }
        }
        if (ok && graph) {
            const int role = a.g_role[c];
            double base = 1.0;
            if (role == CRH_ROLE_CALLER || role == CRH_ROLE_CALLEE) {   // scorer.py:22-27: depth_from_query or 1
                int depth = a.g_depth[c];
                if (depth == 0) depth = 1;
                const double d = 1.0 - (double)(depth - 1) * 0.2;
                base = 0.3 > d ? 0.3 : d;                              // max(0.3, d): the first argument wins a tie
            }
            s[0] = base;
            s[2] = role == CRH_ROLE_PRIMARY ? 1.0 : role == CRH_ROLE_CALLER ? 0.8 : role == CRH_ROLE_CALLEE ? 0.7 : 0.5;
            const int bits = a.g_rich[c];
            double rich = 0.0;                                        // scorer.py:56-66; a graph node carries no content
            if (bits & 1) rich = rich + 0.3;
            if (bits & 2) rich = rich + 0.2;
            if (bits & 4) rich = rich + 0.2;
            s[4] = rich;
            // scorer.py:68-74, the five products summed left to right
            f = s[0] * Q.graph_weight;
            f = f + s[1] * a.bonus;
            f = f + s[2] * Q.relationship_bonus;
            f = f + s[3] * Q.base.centrality_weight;
            f = f + s[4] * Q.context_weight;
        } else if (!graph) {
            // (a padding slot keeps its score in the signal, as k_rerank_vector does; it is never alive)
            const double vs = (double)a.scores[c];
            s[5] = vs;
            if (ok) {
                const int cl = cols.content_len[c];
                s[6] = cl <= 0 ? 0.0 : (cl > 100 && cl < 2000) ? 0.8 : (cl > 50 && cl < 3000) ? 0.5 : 0.3;   // scorer.py:105-114
            }
            // scorer.py:119-124
            f = vs * Q.base.vector_weight;
            f = f + s[1] * a.bonus;
            f = f + s[3] * Q.base.centrality_weight;
            f = f + s[6] * 0.1;
        }
        fin[i] = f;
        for (int j = 0; j < NSIG; ++j) sig[j * n + i] = s[j];
    }
    __syncthreads();

    // merge entries sharing file:entity:start_line (ranker.py:171-202): the first one absorbs the later ones in list order, graph
    // entries before vector hits; the signals are a union, the larger value where both carry one
    for (int i = tid; i < n; i += blockDim.x) {
        if (!valid[i]) continue;
        bool first = true;
        for (int j = 0; j < i; ++j)
            if (valid[j] && keyc[j] == keyc[i]) {
                first = false;
                break;
            }
        if (!first) {
            pos[i] = -2;       // absorbed; alive[] is cleared after the barrier (other owners read valid[] and keyc[] only)
            continue;
        }
        double f = fin[i];
        double s[NSIG];
        for (int t = 0; t < NSIG; ++t) s[t] = sig[t * n + i];
        int mask = maskc[i];
        bool merged = false;
        for (int j = i + 1; j < n; ++j) {
            if (!valid[j] || keyc[j] != keyc[i]) continue;
            double c = (f + fin[j]) / 2;
            c = c * 1.1;
            f = c;
            const int mj = maskc[j];
            for (int t = 0; t < NSIG; ++t) {
                if (!((mj >> t) & 1)) continue;
                const double v = sig[t * n + j];
                if (!((mask >> t) & 1) || v > s[t]) s[t] = v;         // max(held, value): held unless value is larger
            }
            mask |= mj;
            merged = true;
        }
        if (merged) {
            // groups are disjoint: entry i is written by its owner only and read by no other owner
            fin[i] = f;
            for (int t = 0; t < NSIG; ++t) sig[t * n + i] = s[t];
            maskc[i] = mask;
            hybrid[i] = 1;
        }
    }
    __syncthreads();
    for (int i = tid; i < n; i += blockDim.x)
        if (pos[i] == -2) alive[i] = 0;
    __syncthreads();

    // stable descending sort by score (ranker.py:46-48)
    for (int i = tid; i < n; i += blockDim.x) {
        int p = -1;
        if (alive[i]) {
            p = 0;
            const double fi = fin[i];
            for (int j = 0; j < n; ++j)
                if (alive[j] && (fin[j] > fi || (fin[j] == fi && j < i))) ++p;
        }
        pos[i] = p;
    }
    __syncthreads();
    // caps (ranker.py:204-229): at most max_per_file per file in sorted order, then the first max_total of those
    for (int i = tid; i < n; i += blockDim.x) {
        uint8_t keep = 0;
        if (alive[i]) {
            int occ = 0;
            for (int j = 0; j < n; ++j)
                if (alive[j] && pos[j] < pos[i] && filec[j] == filec[i]) ++occ;
            keep = occ < a.max_per_file;
        }
        keepf[i] = keep;
    }
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < n; i += blockDim.x) {
        if (!keepf[i]) continue;
        int slot = 0;
        for (int j = 0; j < n; ++j)
            if (keepf[j] && pos[j] < pos[i]) ++slot;
        if (slot >= a.max_total) continue;
        const size_t o = (size_t)q * a.max_total + slot;
        a.out_index[o] = i;
        a.out_score[o] = fin[i];
        for (int t = 0; t < NSIG; ++t) a.out_signals[o * NSIG + t] = sig[t * n + i];
        a.out_mask[o] = maskc[i];
        a.out_flags[o] = (hybrid[i] ? 1 : 0) | (i < G ? 2 : 0);
        ++mine;
    }
    if (mine) atomicAdd(&total, mine);
    __syncthreads();
    if (tid == 0) a.out_count[q] = need_host ? -1 : total;
    // the slots behind the survivors are written too: no caller has to clear the outputs before a call
    for (int slot = total + tid; slot < a.max_total; slot += blockDim.x) {
        const size_t o = (size_t)q * a.max_total + slot;
        a.out_index[o] = -1;
        a.out_score[o] = 0.0;
        for (int t = 0; t < NSIG; ++t) a.out_signals[o * NSIG + t] = 0.0;
        a.out_mask[o] = 0;
        a.out_flags[o] = 0;
    }
}

bool columns_complete(const crh_rerank_columns *c)
{
    return c && c->content_len && c->degree && c->file_code && c->key_code && c->node_code && c->name_len && c->name;
}

}  // namespace
}  // namespace crh

using namespace crh;

extern "C" {

int crh_graph_node_rows(int64_t n_rows, const int32_t *row_node_dev, const uint32_t *alive_words_dev, int64_t row_base, int64_t n_nodes,
                        int64_t *node_rows_dev, void *stream)
{
    if (n_rows < 0 || n_nodes < 0 || row_base < 0) return fail(CRH_E_INVALID, "node rows: negative size");
    if (n_rows == 0 || n_nodes == 0) return CRH_OK;
    if (!row_node_dev || !node_rows_dev) return fail(CRH_E_INVALID, "node rows: NULL pointer");
    hipLaunchKernelGGL(k_graph_node_rows, dim3((unsigned)ceil_div(n_rows, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), n_rows,
                       row_node_dev, alive_words_dev, row_base, n_nodes, reinterpret_cast<unsigned long long *>(node_rows_dev));
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

int crh_graph_candidates(int nq, int G, int n_segments, const crh_graph_segment *segments_host, const int32_t *list_nodes_dev,
                         const int32_t *list_depth_dev, int n_lists, int limit, const int64_t *node_rows_dev, int64_t n_nodes,
                         crh_graph_segment *segments_dev, int32_t *seg_off_dev, int32_t *out_node_dev, int64_t *out_row_dev,
                         int32_t *out_role_dev, int32_t *out_depth_dev, void *stream)
{
    if (nq < 0 || nq > CRH_GRAPH_CAND_MAX_QUERIES || G < 0 || n_segments < 0 || n_segments > CRH_GRAPH_CAND_MAX_SEGMENTS || n_lists < 0 ||
        limit < 0 || n_nodes < 0)
        return fail(CRH_E_INVALID, "graph candidates: nq=%d G=%d segments=%d lists=%d limit=%d", nq, G, n_segments, n_lists, limit);
    if (nq == 0 || G == 0) return CRH_OK;
    if (!out_node_dev || !out_row_dev || !out_role_dev || !out_depth_dev || !seg_off_dev || (n_segments > 0 && (!segments_host || !segments_dev)))
        return fail(CRH_E_INVALID, "graph candidates: NULL pointer");
    if (n_nodes > 0 && !node_rows_dev) return fail(CRH_E_INVALID, "graph candidates: NULL node rows");
    // every index a lane will form is checked here, before anything is launched
    int32_t off[CRH_GRAPH_CAND_MAX_QUERIES + 1];
    int prev = 0;
    for (int q = 0; q <= nq; ++q) off[q] = 0;
    for (int s = 0; s < n_segments; ++s) {
        const crh_graph_segment &sg = segments_host[s];
        if (sg.query < prev || sg.query >= nq) return fail(CRH_E_INVALID, "graph candidates: segment %d: query %d out of order or range", s, sg.query);
        prev = sg.query;
        if (sg.role < CRH_ROLE_PRIMARY || sg.role > CRH_ROLE_CHILD) return fail(CRH_E_INVALID, "graph candidates: segment %d: role %d", s, sg.role);
        if (sg.node >= 0) {
            if (sg.node >= n_nodes) return fail(CRH_E_INVALID, "graph candidates: segment %d: node %d of %lld", s, sg.node, (long long)n_nodes);
        } else {
            if (sg.list_row < 0 || sg.list_row >= n_lists || sg.take < 0)
                return fail(CRH_E_INVALID, "graph candidates: segment %d: list row %d of %d, take %d", s, sg.list_row, n_lists, sg.take);
            if (sg.take > 0 && limit > 0 && (!list_nodes_dev || !list_depth_dev)) return fail(CRH_E_INVALID, "graph candidates: NULL list");
        }
        ++off[sg.query + 1];
    }
    for (int q = 0; q < nq; ++q) off[q + 1] += off[q];
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_segments > 0) CRH_HIP(hipMemcpyAsync(segments_dev, segments_host, sizeof(crh_graph_segment) * (size_t)n_segments, hipMemcpyHostToDevice, st));
    CRH_HIP(hipMemcpyAsync(seg_off_dev, off, sizeof(int32_t) * (size_t)(nq + 1), hipMemcpyHostToDevice, st));
    CRH_HIP(hipStreamSynchronize(st));   // (as crh_graph_bfs: `off` leaves scope and the caller may free its table on return)
    CandArgs a;
    a.segs = segments_dev;
    a.seg_off = seg_off_dev;
    a.list_nodes = list_nodes_dev;
    a.list_depth = list_depth_dev;
    a.node_rows = node_rows_dev;
    a.n_nodes = n_nodes;
    a.limit = limit;
    a.G = G;
    a.out_node = out_node_dev;
    a.out_row = out_row_dev;
    a.out_role = out_role_dev;
    a.out_depth = out_depth_dev;
    hipLaunchKernelGGL(k_graph_candidates, dim3(nq), dim3(64), 0, st, a);
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

int crh_rerank_hybrid(int nq, int G, int k, const int64_t *g_rows_dev, const int32_t *g_role_dev, const int32_t *g_depth_dev,
                      const crh_rerank_columns *g_cols, const int32_t *g_rich_dev, const float *scores_dev, const int64_t *rows_dev,
                      const crh_rerank_columns *cols, const crh_rerank_hybrid_query *queries_dev, double entity_match_bonus,
                      int max_per_file, int max_total, int primary_top, int centrality_top, int centrality_limit, int32_t *out_index_dev,
                      double *out_score_dev, double *out_signals_dev, int32_t *out_mask_dev, int32_t *out_count_dev, int32_t *out_flags_dev,
                      void *stream)
{
    if (nq < 0 || G < 0 || k < 0 || G + k < 1 || G > CRH_RR_MAX_HYBRID || k > CRH_RR_MAX_HYBRID || G + k > CRH_RR_MAX_HYBRID)
        return fail(CRH_E_INVALID, "hybrid rerank: nq=%d G=%d k=%d (1 <= G + k <= %d)", nq, G, k, CRH_RR_MAX_HYBRID);
    if (max_per_file <= 0 || max_total <= 0 || primary_top < 0 || centrality_top < 0 || centrality_limit < 0)
        return fail(CRH_E_INVALID, "hybrid rerank: bad caps");
    if (nq == 0) return CRH_OK;
    if (!queries_dev || !out_index_dev || !out_score_dev || !out_signals_dev || !out_mask_dev || !out_count_dev || !out_flags_dev)
        return fail(CRH_E_INVALID, "hybrid rerank: NULL pointer");
    if (G > 0 && (!g_rows_dev || !g_role_dev || !g_depth_dev || !g_rich_dev || !columns_complete(g_cols)))
        return fail(CRH_E_INVALID, "hybrid rerank: NULL graph table");
    if (k > 0 && (!scores_dev || !rows_dev || !columns_complete(cols))) return fail(CRH_E_INVALID, "hybrid rerank: NULL vector table");
    HybridArgs a = {};
    a.G = G;
    a.k = k;
    a.g_rows = g_rows_dev;
    a.g_role = g_role_dev;
    a.g_depth = g_depth_dev;
    a.g_rich = g_rich_dev;
    if (G > 0) a.g_cols = *g_cols;
    a.scores = scores_dev;
    a.rows = rows_dev;
    if (k > 0) a.cols = *cols;
    a.queries = queries_dev;
    a.bonus = entity_match_bonus;
    a.max_per_file = max_per_file;
    a.max_total = max_total;
    a.primary_top = primary_top;
    a.centrality_top = centrality_top;
    a.centrality_limit = centrality_limit;
    a.out_index = out_index_dev;
    a.out_score = out_score_dev;
    a.out_signals = out_signals_dev;
    a.out_mask = out_mask_dev;
    a.out_count = out_count_dev;
    a.out_flags = out_flags_dev;
    const size_t lds = (size_t)(G + k) * (8 * (1 + NSIG) + 4 * 4 + 4);
    hipLaunchKernelGGL(k_rerank_hybrid, dim3(nq), dim3(256), lds, static_cast<hipStream_t>(stream), a);
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

}  // extern "C"
