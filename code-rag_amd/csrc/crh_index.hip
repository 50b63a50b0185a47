// crh_index.hip -- host side of the HBM-resident cosine index behind include/coderag_hip.h.
//
// Replaces the Qdrant collection the reference talks to through
// src/lattice/embeddings/client.py (QdrantManager): create / upsert / search / delete.
// One handle = one collection shard on one GPU.  gfx950 only; no fallback path exists:
// if HIP or the device is missing every entry point fails with CRH_E_HIP / CRH_E_NODEVICE.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "crh_common.h"
#include "crh_kernels.hpp"
#include "crh_i8.hpp"
#include "crh_facet.hpp"
#include "crh_range.hpp"

namespace crh {
std::string &last_error_ref()
{
    thread_local std::string s;
    return s;
}
}  // namespace crh

using namespace crh;

namespace {

constexpr int kWaves = 16;      // waves per scan workgroup (one workgroup per CU)
constexpr int kRing = 8;        // 1-KiB loads in flight per wave
constexpr int kWideWaves = 8;   // waves per k_scan_wide workgroup: each sees every tile of its workgroup for 32 queries, so the
                                // workgroup's share of the candidate workspace is cut into 8 lists of 2 x wave_cap entries
constexpr int kI8Waves = 8;     // k_scan_i8: waves per workgroup, 1-KiB loads in flight per wave (crh_i8.hpp)
#ifndef CRH_I8_RING
#define CRH_I8_RING 8
#endif
constexpr int kI8Ring = CRH_I8_RING;
constexpr int kI8SelectParts = 4;   // workgroups per query in k_select behind the int8 scan (64 queries x 4 = the chip)
constexpr int kStatusSlots = 1024;
constexpr int64_t kWorkspaceBudget = 48LL << 30;
constexpr int kRangeParts = 8;  // workgroups per query in k_range_count (crh_range.hpp)
constexpr int kSparseDen = 4;   // the sparse route is taken from 1 populated tile in this many down (profiles/sparse_crossover.md)

// A filter in the form the index keeps, compares and uploads: [n conditions, then per condition: column, mode (0 in, 1 not in,
// 2 between, 3 not between, 4 words, 5 not words), set size, the set's codes ascending without repeats -- for a range: 2, lo, hi;
// for a row bitmap the "column" is the caller's tag and the set is 4 values: the device pointer's low and high half, n's low and
// high half].  crh_filter lists and crh_condition lists both become one of these.
using FilterKey = std::vector<int32_t>;

// what build_mask hands a search: the row mask, and -- while the sparse route is enabled -- the ascending list of the tiles
// whose mask word is not 0 (nlist < 0: no list was made)
struct MaskRef {
    const uint32_t *mask = nullptr;
    const uint32_t *list = nullptr;
    int64_t nlist = -1;
};

// A kept mask: what it was built from and on, and the device copy of its key.  The mask words themselves are in the workspace.
struct MaskCache {
    uint64_t built_at = 0;          // crh_index::mutations when it was built (0: never, or its buffers were reallocated)
    hipStream_t stream = nullptr;   // (the stream the kept mask was built on: another stream rebuilds it -- nothing orders the two)
    bool valid = false;
    FilterKey key;                  // (also the host source of the sets' upload)
    int32_t *sets = nullptr;        // device copy of key: the sets k_filter_mask / k_filter_mask_classes search
    int64_t sets_cap = 0;
    int64_t nlist = -1;             // length of the list of populated tiles made with the mask (< 0: none was made)
};

struct Pending {
    int nq, k;
    FilterKey key;
    int64_t row_base;
    const float *q_dev;
    float *out_s;
    int64_t *out_r;
    int slot;
    hipStream_t stream;   // the stream the batch was enqueued on: what a finish waits for, and where the batch is run again
    bool multi;     // a mixed-filter batch (crh_search_multi): key is the classes' keys behind their number, cls the queries' classes
    QueryClasses cls;
    bool range;     // a range batch (crh_search_range): thr the queries' thresholds, counts their in-range totals (device; nullptr: list only)
    RangeThr thr;
    unsigned long long *counts;
    // a faceting range batch (crh_search_range_facet): the column, and this batch's bins [nq, n_bins] / info [nq, 3] rows (device;
    // fbins == nullptr: none).  enqueue_batch_range zeroes both before the scan, so a batch that is run again starts from 0.
    int fcol, n_bins;
    unsigned long long *fbins, *finfo;
    int path;       // how enqueue_batch nominated the batch's rows: CRH_NOMINATE_INT8 / _BF16 (one launch) / _BF16_3 (three launches, wide scan)
};

}  // namespace

struct crh_index {
    int dim = 0, ksteps = 0, dtype = 0, ncols = 0, device = 0, cu_count = 0;
    int batch_q = 64;  // queries per k_scan pass: 64, or 32 when the 64-query image would not fit LDS (dim 1536)
    bool wide_ok = false;  // k_scan_wide (up to 256 queries per corpus pass, query fragments in registers) exists for this dim
    bool fused_scan = true;   // <= batch_q queries: seed scan + threshold + main scan in one launch (CODERAG_HIP_FUSED_SCAN=0: three)
    // After a grid-wide wait timed out (another stream's kernels held CUs) the index runs the three-launch form for a WINDOW OF
    // TIME, not a number of batches: 0.2 s, doubled by every further time-out up to 5 s, back to 0.2 s once a one-launch batch
    // has gone through (round 3 rested 1024 batches: 2.5 s of queries at the bf16 rate for what is usually a transient cause).
    std::chrono::steady_clock::time_point fused_rest_until{};
    double fused_rest_s = 0.2;
    bool fused_resting() const { return std::chrono::steady_clock::now() < fused_rest_until; }
    // int8 nomination copy (crh_i8.hpp): derived from xt, brought up to date before a scan (i8_sync); tiles >= i8_dirty_from are stale
    bool i8 = false;          // <= batch_q queries are nominated from the copy (dim 384 / 768 / 1536; CODERAG_HIP_I8=0: never)
    u32x4 *x8 = nullptr;
    float *srow = nullptr;
    u32x4 *xrow = nullptr;    // row-major bf16 rows beside the copy (bf16 stores; crh_i8.hpp, ROW-MAJOR ROWS): what k_select's single-row reads use
    bool want_xrow = true;    // (CODERAG_HIP_ROWMAJOR=0: never -- the single-row reads then go to the tiles, as in round 3)
    unsigned int *i8stat = nullptr;
    int64_t x8_cap_tiles = 0, i8_dirty_from = 0;
    int i8_strikes = 0;       // consecutive int8-nominated batches whose candidate buffers overflowed (3: the copy is left unused ...
    int i8_cooldown = 0;      // ... for this many batches; then it gets ONE more try, and the next overflow rests it again)
    bool i8_suppress = false; // (while such a batch is run again on the bf16 scan)
    int nominate_max = CRH_NOMINATE_INT8;   // crh_index_set_nomination: the most advanced mode the caller allows
    bool i8_sample_record = true;           // the sample launch records its tiles' upper ends, the pass does not read those tiles again (CODERAG_HIP_I8_SAMPLE_RECORD=0: it does)
    bool i8_sample_auto = true;             // (CODERAG_HIP_I8_SAMPLE set: that many tiles at every size)
    int i8_sample = kI8SampleTiles;         // sample tiles behind the int8 scan's thresholds: 8192 halves the candidates of 4096 for 100 MB more
                                            // sample reads (-22 us per batch on one index, tools/sample_ab.py); CODERAG_HIP_I8_SAMPLE
    int64_t i8_min_rows = 1000000;          // below this the pass is too short for the copy to pay on every kind of data: Gaussian rows gain
                                            // from 100 k rows up (0.134 against 0.147 ms per batch; 0.285 / 0.360 at 1M), rows around one shared
                                            // mean with isotropic noise -- the widest candidate sets -- only from ~1.5M (1M: 0.397 against 0.358;
                                            // 2M: 0.554 / 0.597; profiles/r04_i8_crossover.txt); CODERAG_HIP_I8_MIN_ROWS
    int64_t cap_rows = 0, cap_tiles = 0, count = 0, alive_count = 0;
    // The validity mask of the last filter is kept while nothing it was built from has changed (rows, alive bits, codes: every
    // mutation bumps `mutations`): the reference's searchers send the same equality filter with query after query (project_name,
    // language: query/vector_search.py:83-93), and rebuilding the mask is a pass over the code columns per batch (~20 us at 10M rows).
    uint64_t mutations = 1;
    MaskCache mask;
    // The sparse route: a filtered batch of <= batch_q queries whose mask leaves at most 1 tile in
    // sparse_den populated walks the list of those tiles with k_scan_list instead of streaming every tile.  The list is made
    // with the mask and kept with it.  crh_index_set_sparse_route / CODERAG_HIP_SPARSE=0, CODERAG_HIP_SPARSE_DEN.
    bool sparse_on = true;
    int sparse_den = kSparseDen;
    // The class masks of a mixed-filter call (crh_search_multi) are kept the same way, under their own key -- the classes' keys
    // one after the other behind their number -- and in their own buffers, so a mixed call and the single-filter calls around
    // it each find their masks as they left them.
    MaskCache cmask;
    FilterClasses *cmask_classes = nullptr;   // device copy of the classes' descriptions (k_filter_mask_classes)
    u32x4 *xt = nullptr;
    float *xf32 = nullptr;
    uint32_t *alive = nullptr;
    int32_t *codes = nullptr;
    unsigned int *scratch_u32 = nullptr;

    // tuning
    int seed_tiles = 4096, wave_cap = 2048, qcap = 65536, force_fallback = 0;

    // search workspace (lazily sized): everything a batch writes between its query preparation and its final selection
    struct Workspace {
        int ws_blocks = 0, ws_wave_cap = 0, ws_qcap = 0, ws_seed = 0;
        int64_t ws_mask_tiles = 0;
        float *qn = nullptr, *gmax = nullptr, *tau = nullptr, *qpar = nullptr, *qlo = nullptr;
        u32x4 *qfrag = nullptr, *qfrag8 = nullptr, *wave_lists = nullptr, *shi = nullptr;
        uint32_t *effmask = nullptr;
        int64_t ws_cmask_tiles = 0;
        uint32_t *cmask = nullptr;      // [cap_tiles][8] the class words of a mixed-filter batch, interleaved per tile
        uint32_t *cunion = nullptr;     // [cap_tiles] their OR: the row mask of the union
        uint32_t *clist = nullptr;      // the union's populated tiles, laid out like tilelist
        uint32_t *tilelist = nullptr;   // [cap_tiles] the populated tiles of effmask, [ceil(cap_tiles / 256)] workgroup counts, [1] the list's length
        u32x2 *qlist = nullptr;
        unsigned long long *skeys = nullptr, *skeys2 = nullptr;
    };
    Workspace ws;
    SearchStatus *status = nullptr;
    float *stage_q = nullptr;
    int64_t stage_q_elems = 0;
    float *stage_os = nullptr;
    int64_t *stage_or = nullptr;
    int64_t stage_out_elems = 0;
    unsigned long long *stage_cnt = nullptr;   // the in-range counts of a crh_search_range call with host outputs
    int64_t stage_cnt_elems = 0;
    void *stage_in = nullptr;
    int64_t stage_in_bytes = 0;

    std::vector<Pending> pending;
    int next_slot = 0;
    crh_search_stats stats{};
    bool stats_carry = false;       // a mutation completed pending batches: their stats stay until the caller's own finish
    hipEvent_t order_ev = nullptr;  // puts a call behind the pending batches of ANOTHER stream (they share the workspace); made on first use

    // optional HIP-event timing of the dominant kernel (bench.py's roofline figure)
    bool profiling = false;
    bool profile_whole_scan = false;   // (crh_index_set_profiling(h, 2): the events bracket the int8 scan's three launches, not the pass alone)
    std::vector<hipEvent_t> ev;  // 2 per status slot: before / after the main scan launch
    double prof_scan_ms = 0.0;
    int64_t prof_scan_launches = 0;
};

namespace {

template <typename T>
int dev_alloc(T **p, int64_t elems)
{
    *p = nullptr;
    if (elems <= 0) return CRH_OK;
    CRH_HIP(hipMalloc(reinterpret_cast<void **>(p), (size_t)elems * sizeof(T)));
    return CRH_OK;
}
template <typename T>
void dev_free(T *&p)
{
    if (p) (void)hipFree(p);
    p = nullptr;
}

float margin_for(const crh_index *h)
{
    // bound on |MFMA bf16 score - canonical score| for unit vectors, times 2 ("margin"):
    //  bf16 store: both sums run over the same exact products; f32 accumulation error <= 768*2^-24 each
    //  f32 store : + rounding q and x to bf16 for the scan.  bf16 keeps 8 significant bits: round to nearest moves a value by up
    //              to u = 2^-8 of itself (half an ulp at the bottom of a binade; NOT 2^-9), a product of two rounded operands by
    //              up to 2u + u^2 of itself, and sum |q_i x_i| <= |q| |x| <= 1 by Cauchy-Schwarz: <= 2*2^-8 + 2^-16 = 7.83e-3.
    //              tests/margin_cases.py builds unit vectors that reach 5.08e-3 per row (1.0e-2 between two rows).
    //  (wider rows sum more terms: the bound scales with dim; 1.5e-4 = 1.6 x (2 * 768 * 2^-24) is kept up to dim 768)
    const float acc = 1.5e-4f * (h->dim > 768 ? (float)h->dim / 768.f : 1.f);
    return h->dtype == CRH_DTYPE_BF16 ? 2.f * acc : 2.f * (acc + 7.83e-3f);
}

int ensure_stage_in(crh_index *h, int64_t bytes)
{
    if (h->stage_in_bytes >= bytes) return CRH_OK;
    if (h->stage_in) (void)hipFree(h->stage_in);
    h->stage_in = nullptr;
    h->stage_in_bytes = 0;   // (sizes are cleared before every reallocation below too: a failed hipMalloc must not leave a
                             // recorded size next to a NULL pointer for the next call to trust)
    CRH_HIP(hipMalloc(&h->stage_in, (size_t)bytes));
    h->stage_in_bytes = bytes;
    return CRH_OK;
}

int scan_blocks(const crh_index *h, int64_t nitems)
{
    int64_t b = ceil_div(nitems, kWaves);
    if (b > h->cu_count) b = h->cu_count;
    if (b < 1) b = 1;
    return (int)b;
}

// (re)allocate the search workspace for the given candidate capacities
int ensure_workspace(crh_index *h, crh_index::Workspace &w, int wave_cap, int qcap)
{
    const int blocks = h->cu_count;
    if (!w.qn) CRH_TRY(dev_alloc(&w.qn, (int64_t)kWideQ * h->dim));
    if (!w.qfrag) CRH_TRY(dev_alloc(&w.qfrag, (int64_t)(kWideQ / 32) * h->ksteps * 64));
    if (!w.tau) CRH_TRY(dev_alloc(&w.tau, kWideQ));
    if (h->i8 && !w.qfrag8) CRH_TRY(dev_alloc(&w.qfrag8, (int64_t)(kMaxQ / 32) * 2 * (h->dim / 32) * 64));
    if (h->i8 && !w.qpar) CRH_TRY(dev_alloc(&w.qpar, kMaxQ * 4));
    // the sample launch's record of upper ends (crh_i8.hpp, `shi`) is an optimisation: no memory for it -> the pass reads every tile
    if (h->i8 && !w.shi && hipMalloc(reinterpret_cast<void **>(&w.shi), (size_t)kI8SampleTiles * 64 * 4 * sizeof(u32x4)) != hipSuccess) {
        (void)hipGetLastError();
        w.shi = nullptr;
        h->i8_sample_record = false;
    }
    if (!h->status) {
        CRH_TRY(dev_alloc(&h->status, kStatusSlots));
        CRH_HIP(hipMemset(h->status, 0, sizeof(SearchStatus) * kStatusSlots));
    }
    if (w.ws_seed < h->seed_tiles) {
        dev_free(w.gmax);
        w.ws_seed = 0;
        CRH_TRY(dev_alloc(&w.gmax, (int64_t)h->seed_tiles * kWideQ));
        w.ws_seed = h->seed_tiles;
    }
    if (w.ws_mask_tiles < h->cap_tiles) {
        dev_free(w.effmask);
        dev_free(w.tilelist);
        w.ws_mask_tiles = 0;
        h->mask.built_at = 0;
        CRH_TRY(dev_alloc(&w.effmask, h->cap_tiles));
        CRH_TRY(dev_alloc(&w.tilelist, h->cap_tiles + ceil_div(h->cap_tiles, 256) + 1));
        w.ws_mask_tiles = h->cap_tiles;
    }
    if (w.ws_blocks != blocks || w.ws_wave_cap != wave_cap) {
        const int64_t bytes = (int64_t)blocks * kWaves * wave_cap * 16;
        if (bytes > kWorkspaceBudget) return fail(CRH_E_CAPACITY, "candidate workspace of %lld bytes exceeds the budget", (long long)bytes);
        dev_free(w.wave_lists);
        w.ws_blocks = w.ws_wave_cap = 0;
        CRH_TRY(dev_alloc(&w.wave_lists, (int64_t)blocks * kWaves * wave_cap));
        w.ws_blocks = blocks;
        w.ws_wave_cap = wave_cap;
    }
    if (w.ws_qcap != qcap) {
        const int64_t bytes = (int64_t)kWideQ * qcap * 16;
        if (bytes > kWorkspaceBudget) return fail(CRH_E_CAPACITY, "per-query candidate lists of %lld bytes exceed the budget", (long long)bytes);
        dev_free(w.qlist);
        dev_free(w.skeys);
        dev_free(w.qlo);
        dev_free(w.skeys2);
        w.ws_qcap = 0;
        CRH_TRY(dev_alloc(&w.qlist, (int64_t)kWideQ * qcap));
        CRH_TRY(dev_alloc(&w.skeys, (int64_t)kWideQ * qcap));
        if (h->i8) CRH_TRY(dev_alloc(&w.qlo, (int64_t)kMaxQ * qcap));
        if (h->i8) CRH_TRY(dev_alloc(&w.skeys2, (int64_t)kMaxQ * qcap));
        w.ws_qcap = qcap;
    }
    return CRH_OK;
}
// the workspace at the current tuning: what the entry points outside crh_search work in
int ensure_workspace0(crh_index *h)
{
    crh_index::Workspace &w = h->ws;
    return ensure_workspace(h, w, std::max(h->wave_cap, w.ws_wave_cap), std::max(h->qcap, w.ws_qcap));
}

__global__ void k_fill_pad(float *s, int64_t *r, int64_t n)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        s[i] = -INFINITY;
        r[i] = -1;
    }
}

// crh_filter list -> key: one-element "in" sets (the code is taken as it is: an equality, -1 included)
void key_from_filters(const crh_filter *filters, int nfilt, FilterKey &key)
{
    key.assign(1, nfilt);
    for (int f = 0; f < nfilt; ++f) {
        const int32_t c[4] = {filters[f].col, 0, 1, filters[f].code};
        key.insert(key.end(), c, c + 4);
    }
}

// crh_condition list -> key: arguments checked, every set sorted, repeats and negative codes dropped (no row's code is a
// negative member: -1 means "key absent", which is in no set)
int key_from_conditions(const crh_index *h, const crh_condition *conds, int n_conds, bool need_one, FilterKey &key, bool words_ok = false)
{
    if (n_conds < (need_one ? 1 : 0) || n_conds > CRH_MAX_FILTERS)
        return fail(CRH_E_INVALID, "n_conds=%d outside %d..%d%s", n_conds, need_one ? 1 : 0, CRH_MAX_FILTERS, need_one ? " (a delete needs a filter)" : "");
    if (n_conds > 0 && !conds) return fail(CRH_E_INVALID, "conds is NULL");
    key.assign(1, n_conds);
    int64_t total = 0;
    for (int f = 0; f < n_conds; ++f) {
        const crh_condition &c = conds[f];
        if (c.negate == CRH_COND_WORDS || c.negate == CRH_COND_NOT_WORDS) {   // a row bitmap: the pointer and n as they are, col is a tag
            if (!words_ok) return fail(CRH_E_INVALID, "condition %d: a row-bitmap condition (mode %d) is not taken by this entry point", f, c.negate);
            if (c.n < ceil_div(h->count, kTileRows))
                return fail(CRH_E_INVALID, "condition %d: a row bitmap of n=%lld words, the index has %lld tiles", f, (long long)c.n,
                            (long long)ceil_div(h->count, kTileRows));
            if (!c.codes && h->count > 0) return fail(CRH_E_INVALID, "condition %d: the row bitmap is NULL", f);
            const uint64_t ptr = (uint64_t)reinterpret_cast<uintptr_t>(c.codes), n = (uint64_t)c.n;
            const int32_t r[7] = {c.col, c.negate, 4, (int32_t)(uint32_t)ptr, (int32_t)(uint32_t)(ptr >> 32), (int32_t)(uint32_t)n, (int32_t)(uint32_t)(n >> 32)};
            key.insert(key.end(), r, r + 7);
            continue;
        }
        if (c.col < 0 || c.col >= h->ncols) return fail(CRH_E_INVALID, "condition %d: column %d out of range (index has %d code columns)", f, c.col, h->ncols);
        if (c.n < 0) return fail(CRH_E_INVALID, "condition %d: set size %lld is negative", f, (long long)c.n);
        if (c.n > 0 && !c.codes) return fail(CRH_E_INVALID, "condition %d: codes is NULL with n=%lld", f, (long long)c.n);
        total += c.n;
        if (total > (1LL << 28)) return fail(CRH_E_CAPACITY, "the sets of one filter hold more than 2^28 codes");
        if (c.negate == CRH_COND_BETWEEN || c.negate == CRH_COND_NOT_BETWEEN) {   // a range: the two bounds as they are (lo > hi: empty)
            if (c.n != 2) return fail(CRH_E_INVALID, "condition %d: a range condition takes n = 2 bounds, got n=%lld", f, (long long)c.n);
            const int32_t r[5] = {c.col, c.negate, 2, c.codes[0], c.codes[1]};
            key.insert(key.end(), r, r + 5);
            continue;
        }
        std::vector<int32_t> v;
        v.reserve((size_t)c.n);
        for (int64_t i = 0; i < c.n; ++i)
            if (c.codes[i] >= 0) v.push_back(c.codes[i]);
        std::sort(v.begin(), v.end());
        v.erase(std::unique(v.begin(), v.end()), v.end());
        const int32_t head[3] = {c.col, c.negate ? 1 : 0, (int32_t)v.size()};
        key.insert(key.end(), head, head + 3);
        key.insert(key.end(), v.begin(), v.end());
    }
    return CRH_OK;
}

// one filter of a key, starting at key[at], as k_filter_mask takes it (set offsets are positions in the key); returns the
// position behind it, or 0 -- and the column in *bad_col -- for a column the index does not have
size_t filterset_from_key(const crh_index *h, const FilterKey &key, size_t at, FilterSet &fs, bool *sets, int *bad_col)
{
    const int nfilt = key[at++];
    fs.n = nfilt;
    for (int f = 0; f < nfilt; ++f) {
        const bool words = (key[at + 1] & 4) != 0;                 // a row bitmap: no column, [pointer lo, hi, n lo, hi] behind the head
        if (!words && (key[at] < 0 || key[at] >= h->ncols)) {
            *bad_col = key[at];
            return 0;
        }
        fs.col[f] = key[at];
        fs.neg[f] = key[at + 1];
        fs.cnt[f] = key[at + 2];
        fs.off[f] = (int)at + 3;
        const bool range = (fs.neg[f] & 2) != 0;                  // [lo, hi] behind the head; nothing to upload
        fs.one[f] = fs.cnt[f] == 1 || range || words ? key[at + 3] : 0;
        fs.hi[f] = range || words ? key[at + 4] : 0;
        *sets = *sets || (fs.cnt[f] > 1 && !range && !words);
        at += 3 + (size_t)fs.cnt[f];
    }
    return at;
}

// is the kept mask the one of this key, built on this stream from the index as it is now, with a tile list iff the sparse route is on?
bool mask_is_current(const MaskCache &c, const crh_index *h, const FilterKey &key, hipStream_t st)
{
    return c.valid && c.built_at == h->mutations && c.stream == st && c.key == key && (c.nlist >= 0) == h->sparse_on;
}

// the device copy of the cache's key: FilterSet::off are positions in it
int upload_sets(MaskCache &c, hipStream_t st)
{
    const int64_t n = (int64_t)c.key.size();
    if (c.sets_cap < n) {
        dev_free(c.sets);
        c.sets_cap = 0;
        CRH_TRY(dev_alloc(&c.sets, n));
        c.sets_cap = n;
    }
    CRH_HIP(hipMemcpyAsync(c.sets, c.key.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    return CRH_OK;
}

// the two launches of a tile list: one workgroup per 256 mask words in both (blockcnt: one word per workgroup)
void launch_tile_list(const uint32_t *words, int64_t ntiles, uint32_t *blockcnt, uint32_t *list, uint32_t *len, hipStream_t st)
{
    const unsigned nb = (unsigned)ceil_div(ntiles, 256);
    hipLaunchKernelGGL(k_tilelist_count, dim3(nb), dim3(256), 0, st, words, ntiles, blockcnt);
    hipLaunchKernelGGL(k_tilelist_fill, dim3(nb), dim3(256), 0, st, words, ntiles, blockcnt, list, len);
}

#ifdef CRH_ENABLE_DEBUG   // helpers of the crh_debug_* selection entry points below
template <typename T>
struct DebugBuf {   // a device array of a debug entry point, released when the call returns
    T *p = nullptr;
    ~DebugBuf() { dev_free(p); }
};

template <int NT, int NB, typename KeyT>
void launch_debug_kth(const void *keys, unsigned nsets, unsigned n, const unsigned *ks, unsigned floor_key, unsigned nblocks,
                      unsigned long long *kmin, unsigned long long *kmax)
{
    hipLaunchKernelGGL((k_debug_kth<NT, NB, KeyT>), dim3(nblocks), dim3(NT), 0, nullptr, static_cast<const KeyT *>(keys), nsets, n, ks,
                       (uint32_t)floor_key, kmin, kmax);
}
#endif

// the populated tiles of a row mask, in order, into list_buf (laid out like Workspace::tilelist); their number decides the
// route, so the host waits for it -- once per mask, not per batch
int make_tile_list(crh_index *h, const uint32_t *words, uint32_t *list_buf, hipStream_t st, int64_t *nlist)
{
    const int64_t ntiles = ceil_div(h->count, kTileRows);
    uint32_t *blockcnt = list_buf + h->cap_tiles, *len = blockcnt + ceil_div(h->cap_tiles, 256);
    launch_tile_list(words, ntiles, blockcnt, list_buf, len, st);
    CRH_HIP(hipGetLastError());
    uint32_t n = 0;
    CRH_HIP(hipMemcpyAsync(&n, len, 4, hipMemcpyDeviceToHost, st));
    CRH_HIP(hipStreamSynchronize(st));
    *nlist = n;
    return CRH_OK;
}

int build_mask(crh_index *h, crh_index::Workspace &w, const FilterKey &key, MaskRef *out, hipStream_t st)
{
    *out = MaskRef{};
    const int nfilt = key.empty() ? 0 : key[0];
    if (nfilt == 0 || h->count == 0) {   // (an empty index: nothing to mask, and a zero-block launch is an error)
        out->mask = h->alive;
        return CRH_OK;
    }
    FilterSet fs;
    bool sets = false;
    int bad_col = 0;
    if (filterset_from_key(h, key, 0, fs, &sets, &bad_col) == 0)
        return fail(CRH_E_INVALID, "filter column %d out of range (index has %d code columns)", bad_col, h->ncols);
    MaskCache &c = h->mask;
    if (!mask_is_current(c, h, key, st)) {
        c.valid = false;
        c.key = key;
        if (sets) CRH_TRY(upload_sets(c, st));
        const int64_t rows = (h->count + 63) & ~63LL;
        hipLaunchKernelGGL(k_filter_mask, dim3((unsigned)ceil_div(rows, 256)), dim3(256), 0, st, h->alive, h->codes, h->cap_rows,
                           h->count, fs, c.sets, w.effmask);
        CRH_HIP(hipGetLastError());
        c.nlist = -1;
        if (h->sparse_on) CRH_TRY(make_tile_list(h, w.effmask, w.tilelist, st, &c.nlist));
        c.built_at = h->mutations;
        c.stream = st;
        c.valid = true;
    }
    out->mask = w.effmask;
    out->list = w.tilelist;
    out->nlist = c.nlist;
    return CRH_OK;
}

// does a batch of nq queries under this mask take the sparse route?
bool sparse_use(const crh_index *h, const MaskRef &m, int nq)
{
    return h->sparse_on && m.nlist >= 0 && nq <= h->batch_q && m.nlist * h->sparse_den <= ceil_div(h->count, kTileRows);
}

// The masks of a mixed-filter batch: ckey = [number of classes, then every class's key].  out->mask is the union's row mask,
// *cmask_out the interleaved class words; the union's tile list is made while the sparse route is enabled.  Kept like the
// single mask (key, mutations, stream), in buffers of their own.
int build_class_masks(crh_index *h, crh_index::Workspace &w, const FilterKey &ckey, MaskRef *out, const uint32_t **cmask_out, hipStream_t st)
{
    *out = MaskRef{};
    *cmask_out = nullptr;
    if (h->count == 0) return CRH_OK;   // (an empty index: every batch is padding, no mask is read)
    MaskCache &c = h->cmask;
    if (w.ws_cmask_tiles < h->cap_tiles) {
        dev_free(w.cmask);
        dev_free(w.cunion);
        dev_free(w.clist);
        w.ws_cmask_tiles = 0;
        c.valid = false;
        CRH_TRY(dev_alloc(&w.cmask, h->cap_tiles * CRH_MAX_CLASSES));
        CRH_TRY(dev_alloc(&w.cunion, h->cap_tiles));
        CRH_TRY(dev_alloc(&w.clist, h->cap_tiles + ceil_div(h->cap_tiles, 256) + 1));
        w.ws_cmask_tiles = h->cap_tiles;
    }
    if (!mask_is_current(c, h, ckey, st)) {
        c.valid = false;
        c.key = ckey;
        FilterClasses fc{};
        fc.n = ckey[0];
        bool sets = false;
        int bad_col = 0;
        size_t at = 1;
        for (int cl = 0; cl < fc.n; ++cl) {
            at = filterset_from_key(h, ckey, at, fc.c[cl], &sets, &bad_col);
            if (at == 0) return fail(CRH_E_INVALID, "class %d: filter column out of range (index has %d code columns)", cl, h->ncols);
        }
        if (!h->cmask_classes) CRH_TRY(dev_alloc(&h->cmask_classes, 1));
        // (the source is on this frame: a copy from pageable memory has left it when the call returns)
        CRH_HIP(hipMemcpyAsync(h->cmask_classes, &fc, sizeof(fc), hipMemcpyHostToDevice, st));
        if (sets) CRH_TRY(upload_sets(c, st));
        CRH_HIP(hipStreamSynchronize(st));
        const int64_t rows = (h->count + 63) & ~63LL;
        hipLaunchKernelGGL(k_filter_mask_classes, dim3((unsigned)ceil_div(rows, 256)), dim3(256), 0, st, h->alive, h->codes, h->cap_rows,
                           h->count, h->cmask_classes, c.sets, w.cmask, w.cunion);
        CRH_HIP(hipGetLastError());
        c.nlist = -1;
        if (h->sparse_on) CRH_TRY(make_tile_list(h, w.cunion, w.clist, st, &c.nlist));
        c.built_at = h->mutations;
        c.stream = st;
        c.valid = true;
    }
    out->mask = w.cunion;
    out->list = w.clist;
    out->nlist = c.nlist;
    *cmask_out = w.cmask;
    return CRH_OK;
}

// scan kernel instantiations: k-steps = dim / 16; 64 queries per pass except for dim 1536 (32: LDS)
template <int MODE>
int launch_scan(crh_index *h, crh_index::Workspace &w, int blocks, hipStream_t st, const uint32_t *mask, int nitems, int stride, int wave_cap, int qcap,
                SearchStatus *stt)
{
#define CRH_SCAN(KS, QB)                                                                                                       \
    hipLaunchKernelGGL((k_scan<KS, MODE, kWaves, kRing, QB>), dim3(blocks), dim3(kWaves * 64), 0, st, h->xt, w.qfrag, w.tau, \
                       mask, nitems, stride, w.gmax, w.wave_lists, wave_cap, stt->qcount, w.qlist, qcap, stt)
    switch (h->ksteps) {
    case 24: CRH_SCAN(24, 2); break;
    case 48: CRH_SCAN(48, 2); break;
    case 64: CRH_SCAN(64, 2); break;
    case 96: CRH_SCAN(96, 1); break;
    default: return fail(CRH_E_INTERNAL, "no scan kernel for %d k-steps", h->ksteps);
    }
#undef CRH_SCAN
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

// the same walk over a list of tiles (the sparse route): every dim the index supports
template <int MODE>
int launch_scan_list(crh_index *h, crh_index::Workspace &w, int blocks, hipStream_t st, const MaskRef &m, int nitems, int stride, int wave_cap, int qcap,
                     SearchStatus *stt)
{
#define CRH_SCAN_LIST(KS, QB)                                                                                                       \
    hipLaunchKernelGGL((k_scan_list<KS, MODE, kWaves, kRing, QB>), dim3(blocks), dim3(kWaves * 64), 0, st, h->xt, w.qfrag, w.tau, \
                       m.mask, m.list, nitems, stride, w.gmax, w.wave_lists, wave_cap, stt->qcount, w.qlist, qcap, stt)
    switch (h->ksteps) {
    case 24: CRH_SCAN_LIST(24, 2); break;
    case 48: CRH_SCAN_LIST(48, 2); break;
    case 64: CRH_SCAN_LIST(64, 2); break;
    case 96: CRH_SCAN_LIST(96, 1); break;
    default: return fail(CRH_E_INTERNAL, "no list scan kernel for %d k-steps", h->ksteps);
    }
#undef CRH_SCAN_LIST
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

// the classed scans of a mixed-filter batch: dense (list == false) or over the union's tile list
// (dim 1024, dense: with the ring of 8 the two picked words cost two spilled VGPRs, and a scratch access inside the tile loop
// breaks the counted waits -- that one instantiation runs a ring of 4; the others hold 128 VGPRs without a spill)
constexpr int kClsRing64 = 4;
template <int MODE>
int launch_scan_cls(crh_index *h, crh_index::Workspace &w, int blocks, hipStream_t st, const MaskRef &m, const uint32_t *cmask, const QueryClasses &cls,
                    bool list, int nitems, int stride, int wave_cap, int qcap, SearchStatus *stt)
{
    const u32x8 *cm = reinterpret_cast<const u32x8 *>(cmask);
#define CRH_SCAN_CLS(KS, QB)                                                                                                          \
    if (list)                                                                                                                         \
        hipLaunchKernelGGL((k_scan_list_cls<KS, MODE, kWaves, kRing, QB>), dim3(blocks), dim3(kWaves * 64), 0, st, h->xt, w.qfrag, w.tau, \
                           cm, cls, m.list, nitems, stride, w.gmax, w.wave_lists, wave_cap, stt->qcount, w.qlist, qcap, stt); \
    else                                                                                                                              \
        hipLaunchKernelGGL((k_scan_cls<KS, MODE, kWaves, KS == 64 ? kClsRing64 : kRing, QB>), dim3(blocks), dim3(kWaves * 64), 0, st, h->xt, w.qfrag, w.tau,  \
                           cm, cls, nitems, stride, w.gmax, w.wave_lists, wave_cap, stt->qcount, w.qlist, qcap, stt)
    switch (h->ksteps) {
    case 24: CRH_SCAN_CLS(24, 2); break;
    case 48: CRH_SCAN_CLS(48, 2); break;
    case 64: CRH_SCAN_CLS(64, 2); break;
    case 96: CRH_SCAN_CLS(96, 1); break;
    default: return fail(CRH_E_INTERNAL, "no classed scan kernel for %d k-steps", h->ksteps);
    }
#undef CRH_SCAN_CLS
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

// What a one-launch scan may spend in ONE grid-wide wait, in 100 MHz ticks: eight times the time its pass over `bytes` should take
// (priced at 4 TB/s, two thirds of what the scans reach), at least 2 ms.  A wait ends when every workgroup has become resident and
// done its share of the phase before it; on an otherwise idle device that is microseconds, beside another stream's kernels it is
// that kernel's remaining time -- and beyond this bound the three-launch form, which needs nobody resident, is the better answer.
unsigned int wait_ticks_for(double bytes)
{
    const double ticks = 8.0 * bytes / 4.0e12 * 1.0e8;
    return (unsigned int)std::min(4.0e9, std::max(2.0e5, ticks));
}

// seed scan + threshold + main scan in one launch (k_scan_fused): <= batch_q queries, the default sample size
int launch_scan_fused(crh_index *h, crh_index::Workspace &w, int blocks, hipStream_t st, const uint32_t *mask, int ntiles, int G, int S, int k, float margin,
                      int nq, int wave_cap, int qcap, SearchStatus *stt)
{
#define CRH_FUSED(KS, QB)                                                                                                          \
    hipLaunchKernelGGL((k_scan_fused<KS, kWaves, kRing, QB>), dim3(blocks), dim3(kWaves * 64), 0, st, h->xt, w.qfrag, mask, ntiles, G, S, \
                       w.gmax, w.tau, k, margin, nq, w.wave_lists, wave_cap, stt->qcount, w.qlist, qcap, stt, h->force_fallback == 2 ? 1 : 0, \
                       wait_ticks_for((double)ntiles * h->ksteps * 1024.0))
    switch (h->ksteps) {
    case 24: CRH_FUSED(24, 2); break;
    case 48: CRH_FUSED(48, 2); break;
    case 96: CRH_FUSED(96, 1); break;
    default: return fail(CRH_E_INTERNAL, "no fused scan kernel for %d k-steps", h->ksteps);   // (dim 1024: its 128 KB query image leaves no LDS for the threshold step)
    }
#undef CRH_FUSED
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

// ---- int8 nomination (crh_i8.hpp)
constexpr int kI8MaxK = 256;   // beyond this k the threshold sits so low that the int8 intervals nominate several 100 k rows per query
bool i8_use(const crh_index *h, int nq, int k)
{
    // (three launches, no grid-wide wait: an index resting from a time-out of the one-launch bf16 scan still nominates from the copy)
    return k <= kI8MaxK && h->i8 && h->nominate_max >= CRH_NOMINATE_INT8 && !h->i8_suppress && h->i8_cooldown == 0 && nq <= h->batch_q && h->fused_scan &&
           (h->seed_tiles == 4096 || h->seed_tiles == kI8SampleTiles) && h->count >= h->i8_min_rows;
}

// the copy covers the index: (re)allocate with the capacity, requantise the tiles touched since the last scan.  Running out of
// memory for the copy is not an error: the index goes on with the bf16 scan.
int i8_alloc(crh_index *h)
{
    if (!h->i8 || h->x8_cap_tiles >= h->cap_tiles) return CRH_OK;
    const int ks8 = h->dim / 32;
    dev_free(h->x8);
    dev_free(h->srow);
    dev_free(h->xrow);
    h->x8_cap_tiles = 0;
    bool ok = hipMalloc(reinterpret_cast<void **>(&h->x8), (size_t)h->cap_tiles * ks8 * 1024) == hipSuccess &&
              hipMalloc(reinterpret_cast<void **>(&h->srow), (size_t)h->cap_tiles * 32 * sizeof(float)) == hipSuccess;
    if (ok && !h->i8stat)
        ok = hipMalloc(reinterpret_cast<void **>(&h->i8stat), 16) == hipSuccess && hipMemset(h->i8stat, 0, 16) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        dev_free(h->x8);
        dev_free(h->srow);
        h->i8 = false;
        return CRH_OK;
    }
    // the row-major rows are an accelerator of the selection step only: no memory for them -> the tiles are read instead
    if (h->want_xrow && h->dtype == CRH_DTYPE_BF16 &&
        hipMalloc(reinterpret_cast<void **>(&h->xrow), (size_t)h->cap_tiles * 32 * h->dim * 2) != hipSuccess) {
        (void)hipGetLastError();
        h->xrow = nullptr;
    }
    h->x8_cap_tiles = h->cap_tiles;
    h->i8_dirty_from = 0;
    return CRH_OK;
}

int i8_sync(crh_index *h, hipStream_t st)
{
    if (!h->i8) return CRH_OK;
    const int64_t ntiles = ceil_div(h->count, kTileRows);
    CRH_TRY(i8_alloc(h));
    if (!h->i8) return CRH_OK;
    if (h->i8_dirty_from < ntiles) {
        if (h->dtype == CRH_DTYPE_F32)
            hipLaunchKernelGGL(k_requant_i8<true>, dim3((unsigned)(ntiles - h->i8_dirty_from)), dim3(64), 0, st, h->xt, h->xf32, h->x8, h->srow,
                               h->i8stat, h->i8_dirty_from, h->ksteps, h->count, (u32x4 *)nullptr);
        else
            hipLaunchKernelGGL(k_requant_i8<false>, dim3((unsigned)(ntiles - h->i8_dirty_from)), dim3(64), 0, st, h->xt, h->xf32, h->x8, h->srow,
                               h->i8stat, h->i8_dirty_from, h->ksteps, h->count, h->xrow);
        CRH_HIP(hipGetLastError());
        h->i8_dirty_from = ntiles;
    }
    return CRH_OK;
}

// what separates a row's canonical score from the exact dot of the QUANTISED-FROM rows and the canonical query: the two f32
// summation orders only -- the copy of an f32 store is quantised from its f32 master, not from the bf16 tiles
float i8_c_abs(const crh_index *h) { return 1.5e-4f * (h->dim > 768 ? (float)h->dim / 768.f : 1.f) + 1e-5f; }

// The sample behind the thresholds: G tiles, every S-th one.  It is read twice (its own launch, then the pass) and buys the
// thresholds: its cost grows with G, the candidates it leaves with 1 / G -- the best G goes with the square root of the corpus.
// 8192 tiles were tuned at 10M rows (2.6 % of them); the same 8192 are 26 % of a 1M-row corpus (profiles/r04_i8_crossover.txt).
// An explicit sample size is kept.
void i8_sample_plan(const crh_index *h, int64_t ntiles, int *G, int *S)
{
    int64_t g_auto = h->i8_sample;
    if (h->seed_tiles == 4096 && h->i8_sample_auto)
        g_auto = std::max<int64_t>(1024, std::min<int64_t>(h->i8_sample, (int64_t)(h->i8_sample * std::sqrt((double)ntiles / 312500.0))));
    *G = (int)std::min<int64_t>(h->seed_tiles == 4096 ? g_auto : h->seed_tiles, ntiles);
    *S = (int)std::max<int64_t>(1, ntiles / *G);
}

// PART 1: the sample tiles, 2: the thresholds (one workgroup per query), 3: the pass -- three launches, stream order between them
template <int PART>
int launch_scan_i8(crh_index *h, crh_index::Workspace &w, int blocks, hipStream_t st, const uint32_t *mask, int ntiles, int G, int S, int k, float c_abs,
                   int nq, int wave_cap, int qcap, SearchStatus *stt, u32x4 *shi)
{
#define CRH_I8(KS8, RING, QB)                                                                                                          \
    hipLaunchKernelGGL((k_scan_i8<KS8, kI8Waves, RING, QB, PART>), dim3(PART == 2 ? QB * 32 : blocks), dim3(kI8Waves * 64), 0, st, h->x8, h->srow, \
                       h->i8stat, w.qfrag8, w.qpar, mask, ntiles, G, S, reinterpret_cast<uint32_t *>(w.gmax), w.tau, k, c_abs, sqrtf((float)h->dim), \
                       nq, w.wave_lists, wave_cap, stt->qcount, w.qlist, w.qlo, qcap, stt, h->xt,                                               \
                       h->dtype == CRH_DTYPE_F32 ? h->xf32 : (const float *)nullptr, w.qn, h->xrow, PART == 2 ? (u32x4 *)nullptr : shi)
    switch (h->dim) {
    case 384: CRH_I8(12, 12, 2); break;
    case 768: CRH_I8(24, kI8Ring, 2); break;
    case 1024: CRH_I8(32, kI8Ring, 2); break;   // (128 KB of query image: fits since the threshold step is a launch of its own)
    case 1536: CRH_I8(48, kI8Ring, 1); break;
    default: return fail(CRH_E_INTERNAL, "no int8 scan kernel for dim %d", h->dim);
    }
#undef CRH_I8
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

// the wide scan: dim 384 / 768 (the query block of a wave must fit its registers)
template <int MODE>
int launch_scan_wide(crh_index *h, crh_index::Workspace &w, hipStream_t st, const uint32_t *mask, int nitems, int stride, int nblk, int wave_cap, int qcap,
                     SearchStatus *stt)
{
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(nitems, h->cu_count));
#define CRH_WIDE(KS)                                                                                                              \
    hipLaunchKernelGGL((k_scan_wide<KS, MODE>), dim3(blocks), dim3(512), 0, st, h->xt, w.qfrag, w.tau, mask, nitems, stride, nblk, \
                       w.gmax, kWideQ, w.wave_lists, kWideWaves, wave_cap * (kWaves / kWideWaves), stt->qcount, w.qlist, qcap, stt)
    switch (h->ksteps) {
    case 24: CRH_WIDE(24); break;
    case 48: CRH_WIDE(48); break;
    default: return fail(CRH_E_INTERNAL, "no wide scan kernel for %d k-steps", h->ksteps);
    }
#undef CRH_WIDE
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

// the queries of a batch as the scans take them: the bf16 image and the canonical queries, with_i8: the integer images too
// (width query slots are prepared: slots >= nq are zero queries, tau = +inf)
int launch_prep(crh_index *h, crh_index::Workspace &w, hipStream_t st, const float *q_dev, int nq, int width, SearchStatus *stt, bool with_i8)
{
#define CRH_PREP(BF16, I8)                                                                                                     \
    hipLaunchKernelGGL((k_prep_queries<BF16, I8>), dim3(width), dim3(64), 0, st, q_dev, nq, h->dim, h->ksteps, w.qn, w.qfrag, stt, \
                       I8 ? w.qfrag8 : (u32x4 *)nullptr, I8 ? w.qpar : (float *)nullptr)
    if (h->dtype == CRH_DTYPE_BF16) {
        if (with_i8) CRH_PREP(true, true); else CRH_PREP(true, false);
    } else {
        if (with_i8) CRH_PREP(false, true); else CRH_PREP(false, false);
    }
#undef CRH_PREP
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

// the selection behind every bf16 scan: canonical scores of the nominated rows, the k best of each query
int launch_select_bf16(crh_index *h, crh_index::Workspace &w, hipStream_t st, int nq, int k, float margin, int64_t row_base, float *out_s, int64_t *out_r,
                       SearchStatus *stt)
{
    if (h->dtype == CRH_DTYPE_F32)
        hipLaunchKernelGGL(k_select<true>, dim3(nq), dim3(1024), 0, st, w.qlist, (const float *)nullptr, stt->qcount, w.ws_qcap, w.skeys, (unsigned long long *)nullptr, w.qn, h->xt,
                           h->xf32, h->dim, h->ksteps, k, margin, row_base, out_s, out_r, stt);
    else
        hipLaunchKernelGGL(k_select<false>, dim3(nq), dim3(1024), 0, st, w.qlist, (const float *)nullptr, stt->qcount, w.ws_qcap, w.skeys, (unsigned long long *)nullptr, w.qn, h->xt,
                           h->xf32, h->dim, h->ksteps, k, margin, row_base, out_s, out_r, stt);
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

// a batch no row can match (an empty index, an empty tile list): the padding the scans would arrive at
int pad_batch(crh_index *h, int slot, int nq, int k, float *out_s, int64_t *out_r, hipStream_t st, bool sparse)
{
    if (sparse) {
        h->stats.batches += 1;
        if (h->profiling) {   // (finish_pending reads the pair of every batch)
            CRH_HIP(hipEventRecord(h->ev[2 * slot], st));
            CRH_HIP(hipEventRecord(h->ev[2 * slot + 1], st));
        }
    }
    CRH_HIP(hipMemsetAsync(h->status + slot, 0, sizeof(SearchStatus), st));
    const int64_t n = (int64_t)nq * k;
    hipLaunchKernelGGL(k_fill_pad, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, out_s, out_r, n);
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

void count_batch(crh_index *h, int64_t rows, int64_t tiles, int64_t seed)
{
    h->stats.rows += rows;
    h->stats.tiles += tiles;
    h->stats.seed_tiles += seed;
    h->stats.batches += 1;
}

// The three-launch bf16 form of a batch: prepare the queries, seed scan over a sample of the items (tiles, or positions of a
// tile list), thresholds (k_tau), main scan over all of them, selection.  scan(mode, n, stride) launches the scan kernel in
// mode 0 (seed) / 1 (main), the mode as a std::integral_constant; rows is what the batch counts as read, width the query
// slots prepared, qstride the row pitch of the seed maxima.
template <typename Scan>
int enqueue_three(crh_index *h, crh_index::Workspace &w, const float *q_dev, int nq, int k, int64_t items, int64_t rows, int width, int qstride,
                  int64_t row_base, float *out_s, int64_t *out_r, int slot, hipStream_t st, Scan scan)
{
    const float margin = margin_for(h);
    SearchStatus *stt = h->status + slot;
    CRH_TRY(launch_prep(h, w, st, q_dev, nq, width, stt, false));
    const int G = (int)std::min<int64_t>(h->seed_tiles, items);
    const int stride = (int)(items / G);   // (G * stride <= items: every sample position is inside them)
    CRH_TRY(scan(std::integral_constant<int, 0>{}, G, stride));
    hipLaunchKernelGGL(k_tau, dim3(width), dim3(256), (size_t)G * 4, st, w.gmax, G, k, margin, nq, w.tau, qstride);
    CRH_HIP(hipGetLastError());
    if (h->profiling) CRH_HIP(hipEventRecord(h->ev[2 * slot], st));
    CRH_TRY(scan(std::integral_constant<int, 1>{}, (int)items, 1));
    if (h->profiling) CRH_HIP(hipEventRecord(h->ev[2 * slot + 1], st));
    CRH_TRY(launch_select_bf16(h, w, st, nq, k, margin, row_base, out_s, out_r, stt));
    count_batch(h, rows, items, G);
    return CRH_OK;
}

// one batch (<= batch_q queries through k_scan, or up to kWideQ through k_scan_wide), everything enqueued on `st`
int enqueue_batch(crh_index *h, crh_index::Workspace &w, const float *q_dev, int nq, int k, const MaskRef &mref, int64_t row_base, float *out_s,
                  int64_t *out_r, int slot, hipStream_t st, int *path_out)
{
    *path_out = CRH_NOMINATE_BF16_3;
    const uint32_t *mask = mref.mask;
    const int64_t ntiles = ceil_div(h->count, kTileRows);
    const bool sparse = ntiles > 0 && sparse_use(h, mref, nq);
    if (ntiles == 0 || (sparse && mref.nlist == 0)) return pad_batch(h, slot, nq, k, out_s, out_r, st, sparse);
    const int wave_cap = w.ws_wave_cap, qcap = w.ws_qcap;
    const float margin = margin_for(h);
    SearchStatus *stt = h->status + slot;
    const bool wide = nq > h->batch_q;
    if (wide && (!h->wide_ok || nq > kWideQ)) return fail(CRH_E_INTERNAL, "batch of %d queries has no scan kernel", nq);
    const int nblk = (nq + 31) / 32;                       // 32-query blocks in use (wide scan)
    const int width = wide ? nblk * 32 : h->batch_q;       // query slots prepared (slots >= nq are zero queries, tau = +inf)
    const int qstride = wide ? kWideQ : 64;                // row pitch of the seed maxima

    // The sparse route: the mask leaves few tiles populated -- the three-launch bf16 scan over the LIST of those tiles
    // (k_scan_list), thresholds seeded from listed tiles only; k_select as behind every bf16 scan, so ids and score bits are
    // what the dense route gives.  It reads nlist tiles instead of ntiles; the int8 copy is not needed at that size.
    if (sparse)
        return enqueue_three(h, w, q_dev, nq, k, mref.nlist, std::min<int64_t>(h->count, mref.nlist * kTileRows), width, qstride, row_base, out_s, out_r, slot, st,
                             [&](auto mode, int n, int stride) {
                                 return launch_scan_list<decltype(mode)::value>(h, w, scan_blocks(h, n), st, mref, n, stride, wave_cap, qcap, stt);
                             });

    // <= batch_q queries, nominated from the int8 copy (crh_i8.hpp): half the bytes of the pass, same results
    if (i8_use(h, nq, k)) {
        CRH_TRY(i8_sync(h, st));
    }
    if (i8_use(h, nq, k)) {   // (asked again: i8_sync may have given the copy up for lack of memory)
        CRH_TRY(launch_prep(h, w, st, q_dev, nq, width, stt, true));   // one launch prepares the bf16 image, the canonical queries and the integer images
        const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(ntiles, kI8Waves), h->cu_count));
        int G8, S8;
        i8_sample_plan(h, ntiles, &G8, &S8);
        const float c_abs = i8_c_abs(h);
        if (h->profiling && h->profile_whole_scan) CRH_HIP(hipEventRecord(h->ev[2 * slot], st));   // (all three launches of the scan)
        // the sample launch records the upper ends of its tiles' rows and the pass takes those tiles' candidates from the record
        // instead of reading and multiplying the tiles again (crh_i8.hpp, `shi`; CODERAG_HIP_I8_SAMPLE_RECORD=0: the pass reads every tile)
        u32x4 *shi = h->i8_sample_record ? w.shi : nullptr;
        CRH_TRY(launch_scan_i8<1>(h, w, blocks, st, mask, (int)ntiles, G8, S8, k, c_abs, nq, wave_cap * (kWaves / kI8Waves), qcap, stt, shi));
        CRH_TRY(launch_scan_i8<2>(h, w, blocks, st, mask, (int)ntiles, G8, S8, k, c_abs, nq, wave_cap * (kWaves / kI8Waves), qcap, stt, shi));
        if (h->profiling && !h->profile_whole_scan) CRH_HIP(hipEventRecord(h->ev[2 * slot], st));   // (the dominant kernel: the pass)
        CRH_TRY(launch_scan_i8<3>(h, w, blocks, st, mask, (int)ntiles, G8, S8, k, c_abs, nq, wave_cap * (kWaves / kI8Waves), qcap, stt, shi));
        if (h->profiling) CRH_HIP(hipEventRecord(h->ev[2 * slot + 1], st));
        // (k_select's margin behind this scan: twice what separates a row's score summed in any order from its canonical score)
        if (h->dtype == CRH_DTYPE_F32)
            hipLaunchKernelGGL((k_select<true, true>), dim3(nq, kI8SelectParts), dim3(1024), 0, st, w.qlist, w.qlo, stt->qcount, qcap, w.skeys, w.skeys2, w.qn, h->xt,
                               h->xf32, h->dim, h->ksteps, k, 2.f * c_abs, row_base, out_s, out_r, stt, (const u32x4 *)nullptr);
        else
            hipLaunchKernelGGL((k_select<false, true>), dim3(nq, kI8SelectParts), dim3(1024), 0, st, w.qlist, w.qlo, stt->qcount, qcap, w.skeys, w.skeys2, w.qn, h->xt,
                               h->xf32, h->dim, h->ksteps, k, 2.f * c_abs, row_base, out_s, out_r, stt, h->xrow);
        CRH_HIP(hipGetLastError());
        // the canonical chains of the few rows the fast scores leave, and the ranking (the kernel boundary is where a query's workgroups meet)
        if (h->dtype == CRH_DTYPE_F32)
            hipLaunchKernelGGL(k_select_final<true>, dim3(nq, kI8SelectParts), dim3(256), 0, st, w.skeys2, w.skeys, qcap, w.qn, h->xt, h->xf32, (const u32x4 *)nullptr,
                               h->dim, h->ksteps, k, 2.f * c_abs, row_base, out_s, out_r, stt);
        else
            hipLaunchKernelGGL(k_select_final<false>, dim3(nq, kI8SelectParts), dim3(256), 0, st, w.skeys2, w.skeys, qcap, w.qn, h->xt, h->xf32, h->xrow,
                               h->dim, h->ksteps, k, 2.f * c_abs, row_base, out_s, out_r, stt);
        CRH_HIP(hipGetLastError());
        count_batch(h, h->count, ntiles, G8);
        *path_out = CRH_NOMINATE_INT8;
        return CRH_OK;
    }

    // <= batch_q queries at the default sample size: seed scan, threshold and main scan are ONE launch (k_scan_fused: every wave's
    // first tile is its sample tile, two grid-wide waits, the corpus read once).  The whole grid must be resident for those
    // waits: it is never larger than the CU count and a workgroup's LDS footprint leaves room for one per CU.
    if (!wide && h->fused_scan && !h->fused_resting() && h->nominate_max >= CRH_NOMINATE_BF16 && h->seed_tiles == 4096 && h->ksteps != 64) {
        if (h->i8_cooldown > 0 && !h->i8_suppress) h->i8_cooldown -= 1;
        CRH_TRY(launch_prep(h, w, st, q_dev, nq, width, stt, false));
        const int blocks = scan_blocks(h, ntiles);
        const int waves = blocks * kWaves;
        const int Gf = (int)std::min<int64_t>(std::min(waves, 4096), ntiles);
        const int Sf = Gf == waves ? (int)std::max<int64_t>(1, ntiles / Gf) : 1;
        if (h->profiling) CRH_HIP(hipEventRecord(h->ev[2 * slot], st));
        CRH_TRY(launch_scan_fused(h, w, blocks, st, mask, (int)ntiles, Gf, Sf, k, margin, nq, wave_cap, qcap, stt));
        if (h->profiling) CRH_HIP(hipEventRecord(h->ev[2 * slot + 1], st));
        CRH_TRY(launch_select_bf16(h, w, st, nq, k, margin, row_base, out_s, out_r, stt));
        count_batch(h, h->count, ntiles, Gf);
        *path_out = CRH_NOMINATE_BF16;
        return CRH_OK;
    }
    if (!wide && h->i8_cooldown > 0 && !h->i8_suppress) h->i8_cooldown -= 1;
    return enqueue_three(h, w, q_dev, nq, k, ntiles, h->count, width, qstride, row_base, out_s, out_r, slot, st, [&](auto mode, int n, int stride) {
        return wide ? launch_scan_wide<decltype(mode)::value>(h, w, st, mask, n, stride, nblk, wave_cap, qcap, stt)
                    : launch_scan<decltype(mode)::value>(h, w, scan_blocks(h, n), st, mask, n, stride, wave_cap, qcap, stt);
    });
}

// One mixed-filter batch (<= batch_q queries, <= CRH_MAX_CLASSES classes): always the three-launch bf16 form, through the
// classed scans -- over every tile, or over the union's tile list when the union is sparse enough.  k_tau and k_select as
// behind every bf16 scan.
int enqueue_batch_multi(crh_index *h, crh_index::Workspace &w, const float *q_dev, int nq, int k, const MaskRef &mref, const uint32_t *cmask,
                        const QueryClasses &cls, int64_t row_base, float *out_s, int64_t *out_r, int slot, hipStream_t st)
{
    const int64_t ntiles = ceil_div(h->count, kTileRows);
    const bool sparse = ntiles > 0 && sparse_use(h, mref, nq);
    if (ntiles == 0 || (sparse && mref.nlist == 0)) return pad_batch(h, slot, nq, k, out_s, out_r, st, sparse);
    const int64_t items = sparse ? mref.nlist : ntiles;   // list positions or tiles
    return enqueue_three(h, w, q_dev, nq, k, items, sparse ? std::min<int64_t>(h->count, items * kTileRows) : h->count, h->batch_q, 64, row_base, out_s, out_r,
                         slot, st, [&](auto mode, int n, int stride) {
                             return launch_scan_cls<decltype(mode)::value>(h, w, scan_blocks(h, n), st, mref, cmask, cls, sparse, n, stride, w.ws_wave_cap, w.ws_qcap,
                                                                           h->status + slot);
                         });
}

// the bins and info rows of one faceting batch, cleared in stream order
int facet_zero(unsigned long long *bins, unsigned long long *info, int nq, int n_bins, hipStream_t st)
{
    CRH_HIP(hipMemsetAsync(bins, 0, sizeof(unsigned long long) * (size_t)nq * (size_t)n_bins, st));
    CRH_HIP(hipMemsetAsync(info, 0, sizeof(unsigned long long) * (size_t)nq * 3, st));
    return CRH_OK;
}

// One range batch (<= batch_q queries; crh_range.hpp): always the three-launch bf16 form -- over every tile, or over the
// mask's tile list when it is sparse enough -- with k_range_tau between the thresholds and the main scan, and the count and
// the cut behind k_select.  List only: the seed scan and k_tau run as in enqueue_three and the threshold can only raise tau.
// With counts: tau is the threshold's lower band edge alone, so there is nothing to seed.
int enqueue_batch_range(crh_index *h, crh_index::Workspace &w, const Pending &p, const MaskRef &mref, int slot, hipStream_t st)
{
    const int64_t ntiles = ceil_div(h->count, kTileRows);
    const bool sparse = ntiles > 0 && sparse_use(h, mref, p.nq);
    if (ntiles == 0 || (sparse && mref.nlist == 0)) {
        if (p.counts) CRH_HIP(hipMemsetAsync(p.counts, 0, sizeof(unsigned long long) * (size_t)p.nq, st));
        if (p.fbins) CRH_TRY(facet_zero(p.fbins, p.finfo, p.nq, p.n_bins, st));
        return pad_batch(h, slot, p.nq, p.k, p.out_s, p.out_r, st, sparse);
    }
    const int64_t items = sparse ? mref.nlist : ntiles;   // list positions or tiles
    const int wave_cap = w.ws_wave_cap, qcap = w.ws_qcap, width = h->batch_q;
    const float margin = margin_for(h);
    SearchStatus *stt = h->status + slot;
    auto scan = [&](auto mode, int n, int stride) {
        return sparse ? launch_scan_list<decltype(mode)::value>(h, w, scan_blocks(h, n), st, mref, n, stride, wave_cap, qcap, stt)
                      : launch_scan<decltype(mode)::value>(h, w, scan_blocks(h, n), st, mref.mask, n, stride, wave_cap, qcap, stt);
    };
    CRH_TRY(launch_prep(h, w, st, p.q_dev, p.nq, width, stt, false));   // (zeroes the slot's SearchStatus)
    if (p.fbins) CRH_TRY(facet_zero(p.fbins, p.finfo, p.nq, p.n_bins, st));   // (as k_range_tau zeroes counts: a re-run adds to nothing)
    int G = 0;
    if (!p.counts) {
        G = (int)std::min<int64_t>(h->seed_tiles, items);
        CRH_TRY(scan(std::integral_constant<int, 0>{}, G, (int)(items / G)));
        hipLaunchKernelGGL(k_tau, dim3(width), dim3(256), (size_t)G * 4, st, w.gmax, G, p.k, margin, p.nq, w.tau, 64);
        CRH_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_range_tau, dim3(1), dim3(width), 0, st, p.thr, margin, p.nq, w.tau, p.counts);
    CRH_HIP(hipGetLastError());
    if (h->profiling) CRH_HIP(hipEventRecord(h->ev[2 * slot], st));
    CRH_TRY(scan(std::integral_constant<int, 1>{}, (int)items, 1));
    if (h->profiling) CRH_HIP(hipEventRecord(h->ev[2 * slot + 1], st));
    CRH_TRY(launch_select_bf16(h, w, st, p.nq, p.k, margin, p.row_base, p.out_s, p.out_r, stt));
    if (p.counts && p.fbins) {
        const FacetOut fo{h->codes + (int64_t)p.fcol * h->cap_rows, p.n_bins, p.fbins, p.finfo};
        if (h->dtype == CRH_DTYPE_F32)
            hipLaunchKernelGGL((k_range_count<true, true>), dim3(p.nq, kRangeParts), dim3(256), 0, st, w.qlist, stt->qcount, qcap, p.thr, margin, w.qn, h->xt,
                               h->xf32, h->dim, h->ksteps, p.counts, fo);
        else
            hipLaunchKernelGGL((k_range_count<false, true>), dim3(p.nq, kRangeParts), dim3(256), 0, st, w.qlist, stt->qcount, qcap, p.thr, margin, w.qn, h->xt,
                               h->xf32, h->dim, h->ksteps, p.counts, fo);
        CRH_HIP(hipGetLastError());
    } else if (p.counts) {
        if (h->dtype == CRH_DTYPE_F32)
            hipLaunchKernelGGL(k_range_count<true>, dim3(p.nq, kRangeParts), dim3(256), 0, st, w.qlist, stt->qcount, qcap, p.thr, margin, w.qn, h->xt, h->xf32,
                               h->dim, h->ksteps, p.counts);
        else
            hipLaunchKernelGGL(k_range_count<false>, dim3(p.nq, kRangeParts), dim3(256), 0, st, w.qlist, stt->qcount, qcap, p.thr, margin, w.qn, h->xt, h->xf32,
                               h->dim, h->ksteps, p.counts);
        CRH_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_range_cut, dim3(p.nq), dim3(256), 0, st, p.thr, p.k, p.out_s, p.out_r);
    CRH_HIP(hipGetLastError());
    count_batch(h, sparse ? std::min<int64_t>(h->count, items * kTileRows) : h->count, items, G);
    return CRH_OK;
}

int next_pow2(int64_t v)
{
    int64_t p = 1;
    while (p < v) p <<= 1;
    return (int)std::min<int64_t>(p, 1LL << 30);
}

// One batch of a search, enqueued on `st` under status slot `slot`: the mask(s) of its filter -- found as the last batch left
// them, or built -- and the pipeline of its kind.  The driver runs every batch through here, finish_pending the ones it runs again.
int enqueue_pending(crh_index *h, crh_index::Workspace &w, const Pending &p, int slot, hipStream_t st, int *path_out)
{
    MaskRef mask;
    // (the masks live in the workspace: stream order puts their rebuild behind the previous batch's scan)
    if (p.multi) {
        const uint32_t *cmask = nullptr;
        CRH_TRY(build_class_masks(h, w, p.key, &mask, &cmask, st));
        *path_out = CRH_NOMINATE_BF16_3;
        return enqueue_batch_multi(h, w, p.q_dev, p.nq, p.k, mask, cmask, p.cls, p.row_base, p.out_s, p.out_r, slot, st);
    }
    CRH_TRY(build_mask(h, w, p.key, &mask, st));
    if (p.range) {
        *path_out = CRH_NOMINATE_BF16_3;
        return enqueue_batch_range(h, w, p, mask, slot, st);
    }
    return enqueue_batch(h, w, p.q_dev, p.nq, p.k, mask, p.row_base, p.out_s, p.out_r, slot, st, path_out);
}

// Completes every pending batch.  A batch is final only once its status slot has been read: the wait is for every stream a
// pending batch was enqueued on -- not for the caller's, which may be another one -- and a batch whose candidate buffers
// overflowed or whose one-launch scan timed out is run again on ITS stream.  Every entry point that changes what such a
// re-run would read (rows, alive words, code columns, capacity) comes through here first, so a re-run always answers for
// the index the batch was enqueued on.
int finish_pending(crh_index *h)
{
    if (h->pending.empty()) return CRH_OK;
    std::vector<hipStream_t> streams;
    for (const Pending &p : h->pending)
        if (std::find(streams.begin(), streams.end(), p.stream) == streams.end()) streams.push_back(p.stream);
    for (hipStream_t s : streams) CRH_HIP(hipStreamSynchronize(s));
    hipStream_t cst = streams.back();
    const int used = std::max(1, std::min(h->next_slot, kStatusSlots));   // slots are handed out in order from 0
    std::vector<SearchStatus> host((size_t)used);
    // (copies of the search path go through a stream of the batches, not through hipMemcpy: that one runs on the NULL stream and would wait for everything
    // another thread has queued there -- an encoder forward under way on torch's default stream held every answer back ~13 ms)
    CRH_HIP(hipMemcpyAsync(host.data(), h->status, sizeof(SearchStatus) * (size_t)used, hipMemcpyDeviceToHost, cst));
    CRH_HIP(hipStreamSynchronize(cst));
    std::vector<Pending> todo;
    todo.swap(h->pending);
    h->next_slot = 0;
    crh_index::Workspace &w = h->ws;   // (everything is idle: a batch that overflowed is re-run alone on its stream)
    for (const Pending &p : todo) {
        hipStream_t st = p.stream;
        SearchStatus s = host[p.slot];
        if (h->profiling && h->count > 0) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, h->ev[2 * p.slot], h->ev[2 * p.slot + 1]) == hipSuccess) {
                h->prof_scan_ms += ms;
                h->prof_scan_launches += 1;
            }
        }
        int attempts = 0;
        int path = p.path;
        bool i8_regrown = false, no_i8 = false;   // no_i8: this batch has been sent to the bf16 scan -- for ALL its remaining attempts
        if (!(s.bar_timeout || s.wave_overflow || s.q_overflow)) {
            if (path == CRH_NOMINATE_INT8) h->i8_strikes = 0;
            if (path != CRH_NOMINATE_BF16_3) h->fused_rest_s = 0.2;   // a one-launch batch went through: the next time-out rests the short window again
        }
        while (s.bar_timeout || s.wave_overflow || s.q_overflow) {
            if (++attempts > 6) return fail(CRH_E_INTERNAL, "candidate buffers still overflow after %d regrowths", attempts - 1);
            int wc = w.ws_wave_cap, qc = w.ws_qcap;
            if (s.bar_timeout) {
                // A grid-wide wait of the one-launch scan gave up: some workgroup was not resident within the launch's bound (other
                // streams' kernels holding CUs).  The batch's results are void and its counts mean nothing (the thresholds were never
                // agreed on): the buffers stay as they are, the batch is run again in the three-launch form, which needs no
                // co-residency, and the index stays on that form for a window of time (crh_index::fused_rest_until).
                h->fused_rest_until = std::chrono::steady_clock::now() + std::chrono::duration_cast<std::chrono::steady_clock::duration>(
                                                                            std::chrono::duration<double>(h->fused_rest_s));
                h->fused_rest_s = std::min(5.0, h->fused_rest_s * 2.0);
                h->stats.fallback_used |= 2;
            } else if (path == CRH_NOMINATE_INT8) {
                // The int8 intervals of this data / this k nominated more rows than the buffers hold.  The true counts are known:
                // when they are moderate (at most 2 % of the rows per query: beyond that the selection behind the scan costs more
                // than the half pass it saves) the buffers grow to them ONCE and the batch runs again from the copy; otherwise,
                // or when that was not enough, the batch goes to the bf16 scan (whose buffers regrow if they must), and three such
                // batches in a row rest the copy for 4096 batches.
                const int64_t need_q = next_pow2((int64_t)s.max_qcount), need_w = next_pow2((int64_t)s.max_wave_cnt) / (kWaves / kI8Waves);   // (an int8 wave's list is kWaves / kI8Waves x wave_cap entries)
                const bool moderate = h->force_fallback != 3 && (int64_t)s.max_qcount <= std::max<int64_t>(h->count / 50, 4096) &&
                                      (int64_t)kWideQ * need_q * 16 * 2 <= kWorkspaceBudget / 4;
                if (!i8_regrown && moderate) {
                    i8_regrown = true;
                    h->stats.fallback_used |= 1;
                    wc = std::max(wc, (int)std::min<int64_t>(need_w, 1 << 20));
                    qc = std::max(qc, (int)need_q);
                    h->qcap = std::max(h->qcap, qc);          // (the data will not change its mind: later batches start from here)
                    h->wave_cap = std::max(h->wave_cap, wc);
                } else {
                    h->i8_strikes += 1;
                    if (h->i8_strikes >= 3) {
                        h->i8_strikes = 2;
                        h->i8_cooldown = 4096;
                    }
                    no_i8 = true;
                    h->stats.fallback_used |= 4;
                }
            } else {
                h->stats.fallback_used |= 1;
                wc = std::max(wc, next_pow2((int64_t)s.max_wave_cnt));
                qc = std::max(qc, next_pow2((int64_t)s.max_qcount));
            }
            // A range batch lists every row at or above its threshold's band: a threshold so low that the lists would not fit
            // the budget is refused here, by the true count -- never answered with a clipped one.
            if (p.range && ((int64_t)kWideQ * qc * 16 > kWorkspaceBudget || (int64_t)h->cu_count * kWaves * wc * 16 > kWorkspaceBudget))
                return fail(CRH_E_CAPACITY, "range search: a query has %u candidate rows at or above its threshold's band (a wave of the scan: %u), "
                            "more than the candidate workspace may hold -- raise the threshold or narrow the filter", s.max_qcount, s.max_wave_cnt);
            CRH_TRY(ensure_workspace(h, w, wc, qc));
            if (!p.multi) h->i8_suppress = no_i8;
            const int rc = enqueue_pending(h, w, p, 0, st, &path);
            h->i8_suppress = false;
            CRH_TRY(rc);
            CRH_HIP(hipMemcpyAsync(&s, h->status, sizeof(SearchStatus), hipMemcpyDeviceToHost, st));
            CRH_HIP(hipStreamSynchronize(st));
        }
        h->stats.candidates += (int64_t)s.candidates;
        h->stats.max_query_cands = std::max<int64_t>(h->stats.max_query_cands, s.max_qcount);
    }
    return CRH_OK;
}

// What every entry point that changes rows, alive words, code columns or capacity does first: the pending batches are
// completed against the index they were enqueued on (one wait for their streams; nothing pending: this test alone).  Their
// stats stay readable until the caller's own crh_search_finish.
int complete_pending(crh_index *h)
{
    if (h->pending.empty()) return CRH_OK;
    DeviceGuard g(h->device);
    CRH_TRY(finish_pending(h));
    h->stats_carry = true;
    return CRH_OK;
}

// the device staging of a call's lists: host outputs are copied from it, crh_search_range_facet leaves its k = 1 lists in it
int ensure_stage_out(crh_index *h, int64_t elems)
{
    if (h->stage_out_elems >= elems) return CRH_OK;
    dev_free(h->stage_os);
    dev_free(h->stage_or);
    h->stage_out_elems = 0;
    CRH_TRY(dev_alloc(&h->stage_os, elems));
    CRH_TRY(dev_alloc(&h->stage_or, elems));
    h->stage_out_elems = elems;
    return CRH_OK;
}

// The search driver: every batch of a call enqueued on the stream, and -- unless queries and outputs are the caller's device
// buffers -- finished and copied back.  What differs between the entry points is passed in: i8_presize (the call may nominate
// from the int8 copy: its candidate buffers are sized beforehand) and plan(p, q0, left, st), which sets the size of the batch
// that starts at query q0 with `left` queries to go (p.nq) and, for a mixed-filter call, p.multi and p.cls.
template <typename Plan>
int search_batches(crh_index *h, int nq, const float *queries, int queries_on_device, int k, const FilterKey &key, bool i8_presize, int64_t row_base,
                   float *out_scores, int64_t *out_rows, int out_on_device, void *stream, Plan plan)
{
    DeviceGuard g(h->device);
    hipStream_t st = static_cast<hipStream_t>(stream);

    // force_fallback (testing): 1 = start from absurdly small candidate buffers so the regrow-and-rerun path runs (behind the int8
    // scan: its one regrowth); 3 = the same, and the int8 scan may NOT regrow (its batches go to the bf16 scan: the strike path);
    // 2 = the one-launch scan's first grid-wide wait expects an arrival too many, so its time-out path runs
    const bool tiny = h->force_fallback == 1 || h->force_fallback == 3;
    int wc = tiny ? 4 : std::max(h->wave_cap, h->ws.ws_wave_cap);
    int qc = tiny ? 8 : std::max(h->qcap, h->ws.ws_qcap);
    if (i8_presize && !tiny && i8_use(h, 1, k)) {
        // the int8 intervals nominate a fixed FRACTION of the rows (the thresholds come from a fixed number of sample tiles):
        // ~21 k per query and ~660 per wave of the int8 scan at 10M rows.  The defaults hold that twice over up to 10M rows; beyond,
        // the buffers grow with the index (the int8 scan cannot regrow them after the fact: an overflow sends the batch to bf16)
        const int64_t scale = next_pow2(ceil_div(h->count, 10000000));
        wc = (int)std::max<int64_t>(wc, std::min<int64_t>(2048 * scale, 1 << 18));
        qc = (int)std::max<int64_t>(qc, std::min<int64_t>(131072 * scale, 1 << 24));
    }
    CRH_TRY(ensure_workspace(h, h->ws, wc, qc));

    const float *q_dev = queries;
    if (!queries_on_device) {
        const int64_t elems = (int64_t)nq * h->dim;
        if (h->stage_q_elems < elems) {
            dev_free(h->stage_q);
            h->stage_q_elems = 0;
            CRH_TRY(dev_alloc(&h->stage_q, elems));
            h->stage_q_elems = elems;
        }
        CRH_HIP(hipMemcpyAsync(h->stage_q, queries, (size_t)elems * 4, hipMemcpyHostToDevice, st));
        q_dev = h->stage_q;
    }
    float *os = out_scores;
    int64_t *orow = out_rows;
    if (!out_on_device) {
        CRH_TRY(ensure_stage_out(h, (int64_t)nq * k));
        os = h->stage_os;
        orow = h->stage_or;
    }
    if (h->pending.empty() && !h->stats_carry) h->stats = crh_search_stats{};
    // Batches pending on ANOTHER stream use the same workspace (query images, thresholds, candidate lists): this call's work
    // goes behind them.  One stream -- every caller in this repository -- never gets here.
    if (!h->pending.empty() && h->pending.back().stream != st) {
        if (!h->order_ev) CRH_HIP(hipEventCreateWithFlags(&h->order_ev, hipEventDisableTiming));
        CRH_HIP(hipEventRecord(h->order_ev, h->pending.back().stream));
        CRH_HIP(hipStreamWaitEvent(st, h->order_ev, 0));
    }

    for (int q0 = 0; q0 < nq;) {
        if (h->next_slot >= kStatusSlots) CRH_TRY(complete_pending(h));   // (every stream's batches: the slots are the index's)
        Pending p{};
        CRH_TRY(plan(p, q0, nq - q0, st));
        p.k = k;
        p.key = key;
        p.row_base = row_base;
        p.q_dev = q_dev + (int64_t)q0 * h->dim;
        p.out_s = os + (int64_t)q0 * k;
        p.out_r = orow + (int64_t)q0 * k;
        p.slot = h->next_slot++;
        p.stream = st;
        CRH_TRY(enqueue_pending(h, h->ws, p, p.slot, st, &p.path));
        h->pending.push_back(p);
        q0 += p.nq;
    }
    if (!out_on_device || !queries_on_device) {
        CRH_TRY(finish_pending(h));
        h->stats_carry = false;
        if (!out_on_device) {
            CRH_HIP(hipMemcpyAsync(out_scores, h->stage_os, (size_t)nq * k * 4, hipMemcpyDeviceToHost, st));
            CRH_HIP(hipMemcpyAsync(out_rows, h->stage_or, (size_t)nq * k * 8, hipMemcpyDeviceToHost, st));
            CRH_HIP(hipStreamSynchronize(st));
        }
    }
    return CRH_OK;
}

// The single-filter search.  More than one k_scan pass worth of queries: up to kWideQ of them share ONE corpus pass through k_scan_wide
int search_key(crh_index *h, int nq, const float *queries, int queries_on_device, int k, const FilterKey &key, int64_t row_base,
               float *out_scores, int64_t *out_rows, int out_on_device, void *stream)
{
    return search_batches(h, nq, queries, queries_on_device, k, key, true, row_base, out_scores, out_rows, out_on_device, stream,
                          [&](Pending &p, int, int left, hipStream_t st) {
                              MaskRef mask;   // (the sparse rule asks the mask; enqueue_pending then finds it kept)
                              CRH_TRY(build_mask(h, h->ws, key, &mask, st));
                              int b = (h->wide_ok && left > h->batch_q) ? std::min(kWideQ, left) : std::min(h->batch_q, left);
                              // up to two passes over the int8 copy (2 x ~1.55 ms at 10M rows) beat one wide pass over the bf16 tiles (~4.2 ms)
                              if (left > h->batch_q && left <= 2 * h->batch_q && h->count > 0 && i8_use(h, h->batch_q, k)) b = h->batch_q;
                              // a mask sparse enough for the list scan: batch_q queries per pass over the few listed tiles, however many there are
                              if (h->count > 0 && sparse_use(h, mask, h->batch_q)) b = std::min(h->batch_q, left);
                              p.nq = b;
                              return (int)CRH_OK;
                          });
}

// The mixed-filter search: as search_key, with the classes' masks and the classed batches (<= batch_q queries each, in caller order)
int search_multi_key(crh_index *h, int nq, const float *queries, int queries_on_device, int k, const FilterKey &ckey, const int32_t *query_class,
                     int64_t row_base, float *out_scores, int64_t *out_rows, int out_on_device, void *stream)
{
    return search_batches(h, nq, queries, queries_on_device, k, ckey, false, row_base, out_scores, out_rows, out_on_device, stream,
                          [&](Pending &p, int q0, int left, hipStream_t) {
                              p.nq = std::min(h->batch_q, left);
                              p.multi = true;
                              for (int i = 0; i < p.nq; ++i) p.cls.w[i >> 3] |= (uint32_t)query_class[q0 + i] << ((i & 7) * 4);
                              return (int)CRH_OK;
                          });
}

// The range search (crh_range.hpp): the same filter for every query, <= batch_q queries per batch in caller order, each batch
// with its own thresholds; counts_dev: the totals' device buffer, or nullptr for the list alone
int search_range_key(crh_index *h, int nq, const float *queries, int queries_on_device, int k, const float *thresholds, const FilterKey &key,
                     int64_t row_base, float *out_scores, int64_t *out_rows, unsigned long long *counts_dev, int out_on_device, void *stream,
                     int fcol = -1, int n_bins = 0, unsigned long long *fbins = nullptr, unsigned long long *finfo = nullptr)
{
    return search_batches(h, nq, queries, queries_on_device, k, key, false, row_base, out_scores, out_rows, out_on_device, stream,
                          [&](Pending &p, int q0, int left, hipStream_t) {
                              p.nq = std::min(h->batch_q, left);
                              p.range = true;
                              for (int i = 0; i < p.nq; ++i) p.thr.v[i] = thresholds[q0 + i];
                              p.counts = counts_dev ? counts_dev + q0 : nullptr;
                              p.fcol = fcol;
                              p.n_bins = n_bins;
                              p.fbins = fbins ? fbins + (size_t)q0 * (size_t)n_bins : nullptr;
                              p.finfo = fbins ? finfo + (size_t)q0 * 3 : nullptr;
                              return (int)CRH_OK;
                          });
}

}  // namespace

extern "C" {

int crh_abi_version(void) { return CRH_ABI_VERSION; }
const char *crh_last_error(void) { return last_error_ref().c_str(); }

int crh_device_count(int *count)
{
    if (!count) return fail(CRH_E_INVALID, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail(CRH_E_NODEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *count = n;
    return CRH_OK;
}

int crh_device_info(int device, char *name_out, int name_cap, char *arch_out, int arch_cap, int64_t *hbm_bytes_out,
                    int *cu_count_out)
{
    hipDeviceProp_t prop;
    CRH_HIP(hipGetDeviceProperties(&prop, device));
    if (name_out && name_cap > 0) snprintf(name_out, (size_t)name_cap, "%s", prop.name);
    if (arch_out && arch_cap > 0) snprintf(arch_out, (size_t)arch_cap, "%s", prop.gcnArchName);
    if (hbm_bytes_out) *hbm_bytes_out = (int64_t)prop.totalGlobalMem;
    if (cu_count_out) *cu_count_out = prop.multiProcessorCount;
    return CRH_OK;
}

int crh_index_create(int dim, int dtype, int64_t capacity_rows, int n_code_cols, int device, crh_index **out)
{
    if (!out) return fail(CRH_E_INVALID, "out is NULL");
    *out = nullptr;
    if (dim != 384 && dim != 768 && dim != 1024 && dim != 1536)
        return fail(CRH_E_INVALID, "dim %d not supported: scan kernels are instantiated for 384, 768 (UniXcoder, the tuned case), 1024 and 1536", dim);
    if (dtype != CRH_DTYPE_F32 && dtype != CRH_DTYPE_BF16) return fail(CRH_E_INVALID, "unknown dtype %d", dtype);
    if (capacity_rows <= 0 || capacity_rows > (1LL << 31)) return fail(CRH_E_INVALID, "capacity_rows %lld out of range", (long long)capacity_rows);
    if (n_code_cols < 0 || n_code_cols > 64) return fail(CRH_E_INVALID, "n_code_cols %d out of range", n_code_cols);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(CRH_E_NODEVICE, "no HIP device visible");
    if (device < 0 || device >= ndev) return fail(CRH_E_INVALID, "device %d out of range (%d visible)", device, ndev);
    hipDeviceProp_t prop;
    CRH_HIP(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(CRH_E_NODEVICE, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
    DeviceGuard g(device);
    if (!g.ok) return fail(CRH_E_HIP, "hipSetDevice(%d) failed", device);

    crh_index *h = new crh_index();
    h->dim = dim;
    h->ksteps = dim / 16;
    h->batch_q = dim > 1024 ? 32 : 64;   // (k_scan's 64-query image does not fit LDS at dim 1536)
    h->wide_ok = dim <= 768 && getenv("CODERAG_HIP_NO_WIDE_SCAN") == nullptr;   // (the env switch exists for A/B timing only)
    {
        const char *e = getenv("CODERAG_HIP_FUSED_SCAN");
        h->fused_scan = !(e && e[0] == '0');
        const char *e8 = getenv("CODERAG_HIP_I8");
        h->i8 = h->fused_scan && !(e8 && e8[0] == '0');
        if (h->i8) h->qcap = 131072;   // ~21 k candidates per query and 10M Gaussian rows behind the int8 scan (37 k with 4096 sample tiles)
        if (const char *em = getenv("CODERAG_HIP_I8_MIN_ROWS")) h->i8_min_rows = atoll(em);
        if (const char *er = getenv("CODERAG_HIP_I8_SAMPLE_RECORD")) h->i8_sample_record = !(er[0] == '0');
        if (const char *es = getenv("CODERAG_HIP_I8_SAMPLE")) {
            h->i8_sample = std::max(1024, std::min(kI8SampleTiles, atoi(es)));
            h->i8_sample_auto = false;
        }
        if (const char *er = getenv("CODERAG_HIP_ROWMAJOR")) h->want_xrow = er[0] != '0';
        if (const char *ep = getenv("CODERAG_HIP_SPARSE")) h->sparse_on = ep[0] != '0';
        if (const char *ed = getenv("CODERAG_HIP_SPARSE_DEN")) h->sparse_den = std::max(1, atoi(ed));
    }
    h->dtype = dtype;
    h->ncols = n_code_cols;
    h->device = device;
    h->cu_count = prop.multiProcessorCount;
    h->cap_rows = (capacity_rows + 31) & ~31LL;
    h->cap_tiles = h->cap_rows / 32;
    int rc = dev_alloc(&h->xt, h->cap_tiles * h->ksteps * 64);
    if (rc == CRH_OK && dtype == CRH_DTYPE_F32) rc = dev_alloc(&h->xf32, h->cap_rows * dim);
    if (rc == CRH_OK) rc = dev_alloc(&h->alive, h->cap_tiles);
    if (rc == CRH_OK && n_code_cols) rc = dev_alloc(&h->codes, h->cap_rows * n_code_cols);
    if (rc == CRH_OK) rc = dev_alloc(&h->scratch_u32, 4);
    if (rc == CRH_OK && hipMemset(h->xt, 0, (size_t)h->cap_tiles * h->ksteps * 1024) != hipSuccess) rc = fail(CRH_E_HIP, "hipMemset(xt) failed");
    if (rc == CRH_OK && hipMemset(h->alive, 0, (size_t)h->cap_tiles * 4) != hipSuccess) rc = fail(CRH_E_HIP, "hipMemset(alive) failed");
    if (rc == CRH_OK && h->codes && hipMemset(h->codes, 0xff, (size_t)h->cap_rows * n_code_cols * 4) != hipSuccess)
        rc = fail(CRH_E_HIP, "hipMemset(codes) failed");
    // an index created for >= i8_min_rows rows takes the memory of its int8 copy now, next to the rows (one large, early
    // allocation: the pass over a copy allocated late, between a framework's cached blocks, measured ~5 % slower in some runs)
    if (rc == CRH_OK && h->i8 && h->cap_rows >= h->i8_min_rows) rc = i8_alloc(h);
    if (rc != CRH_OK) {
        crh_index_destroy(h);
        return rc;
    }
    *out = h;
    return CRH_OK;
}

int crh_index_destroy(crh_index *h)
{
    if (!h) return CRH_OK;
    DeviceGuard g(h->device);
    (void)hipDeviceSynchronize();
    dev_free(h->xt);
    dev_free(h->xf32);
    dev_free(h->alive);
    dev_free(h->codes);
    dev_free(h->scratch_u32);
    dev_free(h->mask.sets);
    dev_free(h->cmask.sets);
    dev_free(h->cmask_classes);
    {
        crh_index::Workspace &w = h->ws;
        dev_free(w.qn);
        dev_free(w.gmax);
        dev_free(w.tau);
        dev_free(w.qfrag);
        dev_free(w.wave_lists);
        dev_free(w.effmask);
        dev_free(w.tilelist);
        dev_free(w.cmask);
        dev_free(w.cunion);
        dev_free(w.clist);
        dev_free(w.qlist);
        dev_free(w.skeys);
        dev_free(w.qfrag8);
        dev_free(w.shi);
        dev_free(w.qpar);
        dev_free(w.qlo);
        dev_free(w.skeys2);
    }
    dev_free(h->x8);
    dev_free(h->srow);
    dev_free(h->xrow);
    dev_free(h->i8stat);
    dev_free(h->status);
    dev_free(h->stage_q);
    dev_free(h->stage_os);
    dev_free(h->stage_or);
    dev_free(h->stage_cnt);
    if (h->stage_in) (void)hipFree(h->stage_in);
    for (auto &e : h->ev) (void)hipEventDestroy(e);
    if (h->order_ev) (void)hipEventDestroy(h->order_ev);
    delete h;
    return CRH_OK;
}

static int append_impl(crh_index *h, int64_t n, const float *vecs, int on_device, const int32_t *codes, int64_t *first_row_out,
                       void *stream, int preprocessed);

int crh_index_append(crh_index *h, int64_t n, const float *vecs, int on_device, const int32_t *codes, int64_t *first_row_out,
                     void *stream)
{
    return append_impl(h, n, vecs, on_device, codes, first_row_out, stream, 0);
}

int crh_index_append_preprocessed(crh_index *h, int64_t n, const float *vecs, int on_device, const int32_t *codes,
                                  int64_t *first_row_out, void *stream)
{
    return append_impl(h, n, vecs, on_device, codes, first_row_out, stream, 1);
}

static int append_impl(crh_index *h, int64_t n, const float *vecs, int on_device, const int32_t *codes, int64_t *first_row_out,
                       void *stream, int preprocessed)
{
    if (!h) return fail(CRH_E_INVALID, "index is NULL");
    if (n < 0) return fail(CRH_E_INVALID, "n < 0");
    if (first_row_out) *first_row_out = h->count;
    if (n == 0) return CRH_OK;
    if (!vecs) return fail(CRH_E_INVALID, "vecs is NULL");
    if (h->ncols > 0 && !codes) return fail(CRH_E_INVALID, "index has %d code columns but codes is NULL", h->ncols);
    if (h->count + n > h->cap_rows)
        return fail(CRH_E_CAPACITY, "append of %lld rows exceeds capacity (%lld of %lld used)", (long long)n, (long long)h->count,
                    (long long)h->cap_rows);
    CRH_TRY(complete_pending(h));   // (a pending batch that is run again must not see these rows)
    DeviceGuard g(h->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t chunk = 65536;
    for (int64_t off = 0; off < n; off += chunk) {
        const int64_t m = std::min(chunk, n - off);
        const float *src = vecs + off * h->dim;
        const int32_t *csrc = codes ? codes + off * h->ncols : nullptr;
        if (!on_device) {
            const int64_t vb = m * h->dim * 4, cb = m * h->ncols * 4;
            CRH_TRY(ensure_stage_in(h, vb + cb));
            CRH_HIP(hipMemcpyAsync(h->stage_in, src, (size_t)vb, hipMemcpyHostToDevice, st));
            src = static_cast<const float *>(h->stage_in);
            if (csrc) {
                void *cd = static_cast<char *>(h->stage_in) + vb;
                CRH_HIP(hipMemcpyAsync(cd, csrc, (size_t)cb, hipMemcpyHostToDevice, st));
                csrc = static_cast<const int32_t *>(cd);
            }
        }
        const int64_t first = h->count + off;
        const unsigned blocks = (unsigned)ceil_div(m, 32);
        if (h->dtype == CRH_DTYPE_F32)
            hipLaunchKernelGGL(k_append<true>, dim3(blocks), dim3(256), 0, st, src, m, first, h->dim, h->ksteps, h->xt, h->xf32, preprocessed);
        else
            hipLaunchKernelGGL(k_append<false>, dim3(blocks), dim3(256), 0, st, src, m, first, h->dim, h->ksteps, h->xt, h->xf32, preprocessed);
        CRH_HIP(hipGetLastError());
        if (csrc) {
            hipLaunchKernelGGL(k_store_codes, dim3((unsigned)ceil_div(m * h->ncols, 256)), dim3(256), 0, st, csrc, m, h->ncols, first,
                               h->cap_rows, h->codes);
            CRH_HIP(hipGetLastError());
        }
        const int64_t ntl = ((first + m - 1) >> 5) - (first >> 5) + 1;
        hipLaunchKernelGGL(k_set_alive, dim3((unsigned)ceil_div(ntl, 256)), dim3(256), 0, st, h->alive, first, m);
        CRH_HIP(hipGetLastError());
        if (!on_device) CRH_HIP(hipStreamSynchronize(st));  // the staging buffer is reused by the next chunk
    }
    h->i8_dirty_from = std::min<int64_t>(h->i8_dirty_from, h->count / kTileRows);   // (the last tile may have been partly filled)
    h->count += n;
    h->alive_count += n;
    h->mutations += 1;
    return CRH_OK;
}

int crh_index_tombstone(crh_index *h, int64_t n, const int64_t *rows)
{
    if (!h) return fail(CRH_E_INVALID, "index is NULL");
    if (n <= 0) return CRH_OK;
    if (!rows) return fail(CRH_E_INVALID, "rows is NULL");
    CRH_TRY(complete_pending(h));   // (a pending batch that is run again must still see these rows)
    DeviceGuard g(h->device);
    CRH_TRY(ensure_stage_in(h, n * 8));
    CRH_HIP(hipMemcpy(h->stage_in, rows, (size_t)n * 8, hipMemcpyHostToDevice));
    CRH_HIP(hipMemset(h->scratch_u32, 0, 4));
    hipLaunchKernelGGL(k_tombstone, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, 0, h->alive,
                       static_cast<const int64_t *>(h->stage_in), n, h->count, h->scratch_u32);
    CRH_HIP(hipGetLastError());
    unsigned int cleared = 0;
    CRH_HIP(hipMemcpy(&cleared, h->scratch_u32, 4, hipMemcpyDeviceToHost));
    h->alive_count -= cleared;
    h->mutations += 1;
    return CRH_OK;
}

static int tombstone_key(crh_index *h, const FilterKey &key, int64_t *n_cleared_out)
{
    if (h->count == 0) return CRH_OK;
    CRH_TRY(complete_pending(h));
    DeviceGuard g(h->device);
    CRH_HIP(hipDeviceSynchronize());   // searches in flight on other streams read `alive` / the shared mask buffer
    CRH_TRY(ensure_workspace0(h));
    MaskRef m;
    CRH_TRY(build_mask(h, h->ws, key, &m, nullptr));
    const int64_t ntiles = ceil_div(h->count, 32);
    CRH_HIP(hipMemset(h->scratch_u32, 0, 4));
    hipLaunchKernelGGL(k_tombstone_mask, dim3((unsigned)ceil_div(ntiles, 256)), dim3(256), 0, 0, h->alive, m.mask, ntiles, h->scratch_u32);
    CRH_HIP(hipGetLastError());
    unsigned int cleared = 0;
    CRH_HIP(hipMemcpy(&cleared, h->scratch_u32, 4, hipMemcpyDeviceToHost));
    h->alive_count -= cleared;
    h->mutations += 1;
    if (n_cleared_out) *n_cleared_out = cleared;
    return CRH_OK;
}

int crh_index_tombstone_filter(crh_index *h, const crh_filter *filters, int n_filters, int64_t *n_cleared_out)
{
    if (!h) return fail(CRH_E_INVALID, "index is NULL");
    if (n_cleared_out) *n_cleared_out = 0;
    if (n_filters <= 0 || n_filters > CRH_MAX_FILTERS) return fail(CRH_E_INVALID, "n_filters=%d outside 1..%d (a delete needs a filter)", n_filters, CRH_MAX_FILTERS);
    if (!filters) return fail(CRH_E_INVALID, "filters is NULL");
    FilterKey key;
    key_from_filters(filters, n_filters, key);
    return tombstone_key(h, key, n_cleared_out);
}

int crh_index_tombstone_cond(crh_index *h, const crh_condition *conds, int n_conds, int64_t *n_cleared_out)
{
    if (!h) return fail(CRH_E_INVALID, "index is NULL");
    if (n_cleared_out) *n_cleared_out = 0;
    FilterKey key;
    CRH_TRY(key_from_conditions(h, conds, n_conds, true, key));
    return tombstone_key(h, key, n_cleared_out);
}

int crh_index_compact(crh_index *h, int64_t *old_to_new_host, int64_t *rows_after)
{
    if (!h) return fail(CRH_E_INVALID, "index is NULL");
    if (rows_after) *rows_after = h->alive_count;
    DeviceGuard g(h->device);
    CRH_HIP(hipDeviceSynchronize());   // searches in flight on any stream read what is about to move
    if (!h->pending.empty()) return fail(CRH_E_INVALID, "compact: searches with device outputs are pending (call crh_search_finish first)");
    const int64_t count = h->count, ntiles = ceil_div(count, 32);
    if (count == 0) return CRH_OK;
    if (h->alive_count == count) {   // nothing to reclaim: the identity map
        if (old_to_new_host)
            for (int64_t r = 0; r < count; ++r) old_to_new_host[r] = r;
        return CRH_OK;
    }
    // per-tile prefix of the alive counts (host: ntiles words, 1.25 MB per 10M rows)
    std::vector<uint32_t> words((size_t)ntiles);
    CRH_HIP(hipMemcpy(words.data(), h->alive, (size_t)ntiles * 4, hipMemcpyDeviceToHost));
    std::vector<int64_t> prefix((size_t)ntiles);
    int64_t new_count = 0;
    for (int64_t t = 0; t < ntiles; ++t) {
        prefix[(size_t)t] = new_count;
        new_count += __builtin_popcount(words[(size_t)t]);
    }
    if (new_count != h->alive_count) return fail(CRH_E_INTERNAL, "compact: %lld alive bits, %lld alive rows on record", (long long)new_count, (long long)h->alive_count);
    const int64_t new_tiles = ceil_div(new_count, 32);
    // The rows only ever move DOWN (new <= old), so the image is compacted in place, chunk by chunk through a bounce buffer:
    // the new tiles [c, c + C) are gathered from old rows >= 32 c -- which no earlier chunk has overwritten -- and then copied
    // over the old tiles [c, c + C), which no later chunk reads.  The chunk bounds the extra memory (1M rows: 1.5 GB of tiles).
    const int64_t chunk_tiles = std::min<int64_t>(std::max<int64_t>(new_tiles, 1), 1 << 15);
    const int64_t chunk_rows = chunk_tiles * 32;
    const size_t per_row = std::max<size_t>((size_t)h->dim * 2, h->xf32 ? (size_t)h->dim * 4 : 0);
    int64_t *d_prefix = nullptr, *d_o2n = nullptr;
    int32_t *d_n2o = nullptr;
    void *bounce = nullptr;
    auto cleanup = [&]() {
        if (d_prefix) (void)hipFree(d_prefix);
        if (d_o2n) (void)hipFree(d_o2n);
        if (d_n2o) (void)hipFree(d_n2o);
        if (bounce) (void)hipFree(bounce);
    };
#define CRH_CPT(expr)                                                                                                        \
    do {                                                                                                                     \
        hipError_t e_ = (expr);                                                                                              \
        if (e_ != hipSuccess) {                                                                                              \
            cleanup();                                                                                                       \
            return fail(CRH_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);               \
        }                                                                                                                    \
    } while (0)
    CRH_CPT(hipMalloc(reinterpret_cast<void **>(&d_prefix), (size_t)ntiles * 8));
    CRH_CPT(hipMalloc(reinterpret_cast<void **>(&d_o2n), (size_t)count * 8));
    CRH_CPT(hipMalloc(reinterpret_cast<void **>(&d_n2o), (size_t)std::max<int64_t>(new_count, 1) * 4));
    CRH_CPT(hipMalloc(&bounce, (size_t)chunk_rows * per_row));
    CRH_CPT(hipMemcpy(d_prefix, prefix.data(), (size_t)ntiles * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_compact_map, dim3((unsigned)ceil_div(count, 256)), dim3(256), 0, 0, h->alive, d_prefix, count, d_o2n, d_n2o);
    CRH_CPT(hipGetLastError());
    const size_t tile_bytes = (size_t)h->ksteps * 1024;
    const int row16 = h->dim / 4;   // 16-byte pieces of an f32 row
    for (int64_t t0 = 0; t0 < new_tiles; t0 += chunk_tiles) {
        const int64_t nt = std::min(chunk_tiles, new_tiles - t0), r0 = t0 * 32, nr = nt * 32;
        hipLaunchKernelGGL(k_compact_tiles, dim3((unsigned)nt), dim3(256), 0, 0, h->xt, h->ksteps, d_n2o, new_count, t0, static_cast<u32x4 *>(bounce));
        CRH_CPT(hipGetLastError());
        CRH_CPT(hipMemcpyAsync(reinterpret_cast<char *>(h->xt) + (size_t)t0 * tile_bytes, bounce, (size_t)nt * tile_bytes, hipMemcpyDeviceToDevice, 0));
        if (h->xf32) {
            hipLaunchKernelGGL(k_compact_rows16, dim3((unsigned)ceil_div(nr * row16, 256)), dim3(256), 0, 0, reinterpret_cast<const u32x4 *>(h->xf32), row16,
                               d_n2o, new_count, r0, nr, static_cast<u32x4 *>(bounce));
            CRH_CPT(hipGetLastError());
            CRH_CPT(hipMemcpyAsync(h->xf32 + r0 * h->dim, bounce, (size_t)nr * h->dim * 4, hipMemcpyDeviceToDevice, 0));
        }
        for (int c = 0; c < h->ncols; ++c) {
            int32_t *col = h->codes + (int64_t)c * h->cap_rows;
            hipLaunchKernelGGL(k_compact_i32, dim3((unsigned)ceil_div(nr, 256)), dim3(256), 0, 0, col, d_n2o, new_count, r0, nr, (int32_t)-1,
                               static_cast<int32_t *>(bounce));
            CRH_CPT(hipGetLastError());
            CRH_CPT(hipMemcpyAsync(col + r0, bounce, (size_t)nr * 4, hipMemcpyDeviceToDevice, 0));
        }
    }
    // what lies beyond the new end goes back to the state crh_index_create leaves: zero tiles, no alive bits, codes -1
    if (ntiles > new_tiles) {
        CRH_CPT(hipMemsetAsync(reinterpret_cast<char *>(h->xt) + (size_t)new_tiles * tile_bytes, 0, (size_t)(ntiles - new_tiles) * tile_bytes, 0));
        for (int c = 0; c < h->ncols; ++c)
            CRH_CPT(hipMemsetAsync(h->codes + (int64_t)c * h->cap_rows + new_tiles * 32, 0xff, (size_t)(ntiles - new_tiles) * 32 * 4, 0));
    }
    hipLaunchKernelGGL(k_compact_alive, dim3((unsigned)ceil_div(ntiles, 256)), dim3(256), 0, 0, h->alive, new_count, ntiles);
    CRH_CPT(hipGetLastError());
    if (old_to_new_host) CRH_CPT(hipMemcpy(old_to_new_host, d_o2n, (size_t)count * 8, hipMemcpyDeviceToHost));
    CRH_CPT(hipDeviceSynchronize());
#undef CRH_CPT
    cleanup();
    h->count = new_count;
    h->mutations += 1;
    h->i8_dirty_from = 0;
    h->alive_count = new_count;
    if (rows_after) *rows_after = new_count;
    return CRH_OK;
}

int crh_index_export(crh_index *h, int64_t first_tile, int64_t n_tiles, void *tiles_host, float *master_host, uint32_t *alive_host,
                     int32_t *codes_host)
{
    if (!h) return fail(CRH_E_INVALID, "index is NULL");
    const int64_t used_tiles = ceil_div(h->count, 32);
    if (first_tile < 0 || n_tiles < 0 || first_tile + n_tiles > used_tiles)
        return fail(CRH_E_INVALID, "tile range [%lld,+%lld) outside the %lld tiles in use", (long long)first_tile, (long long)n_tiles, (long long)used_tiles);
    if (n_tiles == 0) return CRH_OK;
    DeviceGuard g(h->device);
    CRH_HIP(hipDeviceSynchronize());
    const size_t tile_bytes = (size_t)h->ksteps * 1024;
    if (tiles_host) CRH_HIP(hipMemcpy(tiles_host, reinterpret_cast<const char *>(h->xt) + (size_t)first_tile * tile_bytes, (size_t)n_tiles * tile_bytes, hipMemcpyDeviceToHost));
    const int64_t r0 = first_tile * 32, nr = std::min(n_tiles * 32, h->cap_rows - r0);
    if (master_host) {
        if (!h->xf32) return fail(CRH_E_INVALID, "export: this index keeps no f32 master copy (dtype bf16)");
        CRH_HIP(hipMemcpy(master_host, h->xf32 + r0 * h->dim, (size_t)nr * h->dim * 4, hipMemcpyDeviceToHost));
        if (r0 + nr > h->count)   // slots of the last tile past the row count were never written: the file gets zeros there
            memset(master_host + (h->count - r0) * h->dim, 0, (size_t)(r0 + nr - h->count) * h->dim * 4);
    }
    if (alive_host) CRH_HIP(hipMemcpy(alive_host, h->alive + first_tile, (size_t)n_tiles * 4, hipMemcpyDeviceToHost));
    if (codes_host)
        for (int c = 0; c < h->ncols; ++c)
            CRH_HIP(hipMemcpy(codes_host + (int64_t)c * n_tiles * 32, h->codes + (int64_t)c * h->cap_rows + r0, (size_t)nr * 4, hipMemcpyDeviceToHost));
    return CRH_OK;
}

int crh_index_import(crh_index *h, int64_t first_tile, int64_t n_tiles, int64_t rows_after, const void *tiles_host,
                     const float *master_host, const uint32_t *alive_host, const int32_t *codes_host)
{
    if (!h) return fail(CRH_E_INVALID, "index is NULL");
    if (first_tile < 0 || n_tiles <= 0 || first_tile + n_tiles > h->cap_tiles)
        return fail(CRH_E_CAPACITY, "import of tiles [%lld,+%lld) exceeds the capacity of %lld tiles (reserve first)", (long long)first_tile,
                    (long long)n_tiles, (long long)h->cap_tiles);
    if (first_tile * 32 != ((h->count + 31) & ~31LL))
        return fail(CRH_E_INVALID, "import must continue at the end of the index (tile %lld, got %lld)", (long long)(((h->count + 31) & ~31LL) / 32), (long long)first_tile);
    if (rows_after <= first_tile * 32 || rows_after > (first_tile + n_tiles) * 32 || rows_after <= (first_tile + n_tiles - 1) * 32)
        return fail(CRH_E_INVALID, "rows_after=%lld does not end inside the last imported tile", (long long)rows_after);
    if (!tiles_host || !alive_host) return fail(CRH_E_INVALID, "import: tiles and alive words are required");
    if ((h->xf32 != nullptr) != (master_host != nullptr)) return fail(CRH_E_INVALID, "import: the f32 master copy goes with dtype f32, and only with it");
    if ((h->ncols > 0) != (codes_host != nullptr)) return fail(CRH_E_INVALID, "import: index has %d code columns", h->ncols);
    CRH_TRY(complete_pending(h));
    DeviceGuard g(h->device);
    CRH_HIP(hipDeviceSynchronize());
    const size_t tile_bytes = (size_t)h->ksteps * 1024;
    const int64_t r0 = first_tile * 32, nr = n_tiles * 32;
    CRH_HIP(hipMemcpy(reinterpret_cast<char *>(h->xt) + (size_t)first_tile * tile_bytes, tiles_host, (size_t)n_tiles * tile_bytes, hipMemcpyHostToDevice));
    if (master_host) CRH_HIP(hipMemcpy(h->xf32 + r0 * h->dim, master_host, (size_t)nr * h->dim * 4, hipMemcpyHostToDevice));
    // rows past rows_after in the last tile are not rows of the index: their alive bits must stay clear
    std::vector<uint32_t> al(alive_host, alive_host + n_tiles);
    const int tail = (int)(rows_after - (first_tile + n_tiles - 1) * 32);
    if (tail < 32) al[(size_t)n_tiles - 1] &= (1u << tail) - 1u;
    int64_t alive_rows = 0;
    for (uint32_t w : al) alive_rows += __builtin_popcount(w);
    CRH_HIP(hipMemcpy(h->alive + first_tile, al.data(), (size_t)n_tiles * 4, hipMemcpyHostToDevice));
    for (int c = 0; c < h->ncols; ++c)
        CRH_HIP(hipMemcpy(h->codes + (int64_t)c * h->cap_rows + r0, codes_host + (int64_t)c * nr, (size_t)nr * 4, hipMemcpyHostToDevice));
    h->count = rows_after;
    h->mutations += 1;
    h->i8_dirty_from = std::min<int64_t>(h->i8_dirty_from, first_tile);
    h->alive_count += alive_rows;
    return CRH_OK;
}

int crh_index_count(crh_index *h, int64_t *rows_out, int64_t *alive_out)
{
    if (!h) return fail(CRH_E_INVALID, "index is NULL");
    if (rows_out) *rows_out = h->count;
    if (alive_out) *alive_out = h->alive_count;
    return CRH_OK;
}

int crh_index_clear(crh_index *h)
{
    if (!h) return fail(CRH_E_INVALID, "index is NULL");
    CRH_TRY(complete_pending(h));   // (the pending batches answer for the rows that are about to go)
    DeviceGuard g(h->device);
    CRH_HIP(hipDeviceSynchronize());
    const int64_t used_tiles = ceil_div(h->count, 32);
    if (used_tiles) {
        CRH_HIP(hipMemset(h->xt, 0, (size_t)used_tiles * h->ksteps * 1024));
        CRH_HIP(hipMemset(h->alive, 0, (size_t)used_tiles * 4));
    }
    h->count = 0;
    h->mutations += 1;
    h->i8_dirty_from = 0;
    h->alive_count = 0;
    return CRH_OK;
}

int crh_index_reserve(crh_index *h, int64_t capacity_rows)
{
    if (!h) return fail(CRH_E_INVALID, "index is NULL");
    if (capacity_rows <= h->cap_rows) return CRH_OK;
    if (capacity_rows > (1LL << 31)) return fail(CRH_E_INVALID, "capacity_rows %lld out of range", (long long)capacity_rows);
    CRH_TRY(complete_pending(h));   // (rows and code columns move to new buffers, the kept masks are void)
    DeviceGuard g(h->device);
    CRH_HIP(hipDeviceSynchronize());
    const int64_t new_rows = (capacity_rows + 31) & ~31LL, new_tiles = new_rows / 32;
    const int64_t used_tiles = ceil_div(h->count, 32);
    u32x4 *nxt = nullptr;
    float *nf32 = nullptr;
    uint32_t *nalive = nullptr;
    int32_t *ncodes = nullptr;
    int rc = dev_alloc(&nxt, new_tiles * h->ksteps * 64);
    if (rc == CRH_OK && h->xf32) rc = dev_alloc(&nf32, new_rows * h->dim);
    if (rc == CRH_OK) rc = dev_alloc(&nalive, new_tiles);
    if (rc == CRH_OK && h->ncols) rc = dev_alloc(&ncodes, new_rows * h->ncols);
    hipError_t e = hipSuccess;
    if (rc == CRH_OK) {
        const size_t used_b = (size_t)used_tiles * h->ksteps * 1024;
        if (e == hipSuccess) e = hipMemset(reinterpret_cast<char *>(nxt) + used_b, 0, (size_t)new_tiles * h->ksteps * 1024 - used_b);
        if (e == hipSuccess && used_b) e = hipMemcpy(nxt, h->xt, used_b, hipMemcpyDeviceToDevice);
        if (e == hipSuccess) e = hipMemset(nalive, 0, (size_t)new_tiles * 4);
        if (e == hipSuccess && used_tiles) e = hipMemcpy(nalive, h->alive, (size_t)used_tiles * 4, hipMemcpyDeviceToDevice);
        if (e == hipSuccess && nf32 && h->count) e = hipMemcpy(nf32, h->xf32, (size_t)h->count * h->dim * 4, hipMemcpyDeviceToDevice);
        if (e == hipSuccess && ncodes) e = hipMemset(ncodes, 0xff, (size_t)new_rows * h->ncols * 4);
        for (int c = 0; c < h->ncols && e == hipSuccess && h->count; ++c)
            e = hipMemcpy(ncodes + (int64_t)c * new_rows, h->codes + (int64_t)c * h->cap_rows, (size_t)h->count * 4, hipMemcpyDeviceToDevice);
        if (e != hipSuccess) rc = fail(CRH_E_HIP, "reserve copy failed: %s", hipGetErrorString(e));
    }
    if (rc != CRH_OK) {
        dev_free(nxt);
        dev_free(nf32);
        dev_free(nalive);
        dev_free(ncodes);
        return rc;
    }
    dev_free(h->xt);
    dev_free(h->xf32);
    dev_free(h->alive);
    dev_free(h->codes);
    h->xt = nxt;
    h->xf32 = nf32;
    h->alive = nalive;
    h->codes = ncodes;
    h->cap_rows = new_rows;
    h->mutations += 1;   // (the code columns moved to their new pitch)
    h->cap_tiles = new_tiles;
    return CRH_OK;
}

int crh_index_read_rows(crh_index *h, int64_t first, int64_t n, float *out_host)
{
    if (!h) return fail(CRH_E_INVALID, "index is NULL");
    if (first < 0 || n < 0 || first + n > h->count) return fail(CRH_E_INVALID, "row range [%lld,+%lld) outside the index", (long long)first, (long long)n);
    if (n == 0) return CRH_OK;
    if (!out_host) return fail(CRH_E_INVALID, "out_host is NULL");
    DeviceGuard g(h->device);
    if (h->dtype == CRH_DTYPE_F32) {
        CRH_HIP(hipMemcpy(out_host, h->xf32 + first * h->dim, (size_t)n * h->dim * 4, hipMemcpyDeviceToHost));
        return CRH_OK;
    }
    const int64_t chunk = 65536;
    CRH_TRY(ensure_stage_in(h, std::min(chunk, n) * h->dim * 4));
    for (int64_t off = 0; off < n; off += chunk) {
        const int64_t m = std::min(chunk, n - off);
        hipLaunchKernelGGL(k_untile_rows, dim3((unsigned)ceil_div(m * (h->dim / 8), 256)), dim3(256), 0, 0, h->xt, h->ksteps,
                           first + off, m, h->dim, static_cast<float *>(h->stage_in));
        CRH_HIP(hipGetLastError());
        CRH_HIP(hipMemcpy(out_host + off * h->dim, h->stage_in, (size_t)m * h->dim * 4, hipMemcpyDeviceToHost));
    }
    return CRH_OK;
}

int crh_index_gather_vectors(crh_index *h, int64_t n, const int64_t *rows_dev, int64_t row_base, float *out_dev, void *stream)
{
    if (!h) return fail(CRH_E_INVALID, "index is NULL");
    if (n < 0 || n > (1LL << 40) / h->dim) return fail(CRH_E_INVALID, "gather_vectors: n=%lld out of range", (long long)n);
    if (n == 0) return CRH_OK;
    if (!rows_dev || !out_dev) return fail(CRH_E_INVALID, "gather_vectors: NULL pointer");
    DeviceGuard g(h->device);
    if (!g.ok) return fail(CRH_E_HIP, "hipSetDevice(%d) failed", h->device);
    // the row-major bf16 rows hold the tiles the last int8 synchronisation wrote (tiles >= i8_dirty_from are stale or absent)
    const bool rows_live = h->dtype == CRH_DTYPE_BF16 && h->xrow != nullptr && h->x8_cap_tiles >= h->cap_tiles;
    hipLaunchKernelGGL(k_gather_vectors, dim3((unsigned)ceil_div(n * (h->dim / 8), 256)), dim3(256), 0, static_cast<hipStream_t>(stream), n, rows_dev,
                       row_base, h->count, h->dim, h->ksteps, h->dtype == CRH_DTYPE_F32 ? h->xf32 : (const float *)nullptr,
                       rows_live ? h->xrow : (const u32x4 *)nullptr, rows_live ? h->i8_dirty_from : (int64_t)0, h->xt, out_dev);
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

int crh_index_gather_codes(crh_index *h, int col, int64_t n, const int64_t *rows_dev, int64_t row_base, int32_t *out_codes_dev, void *stream)
{
    if (!h) return fail(CRH_E_INVALID, "index is NULL");
    if (col < 0 || col >= h->ncols) return fail(CRH_E_INVALID, "gather_codes: column %d outside 0..%d", col, h->ncols - 1);
    if (n < 0 || n > (1LL << 38)) return fail(CRH_E_INVALID, "gather_codes: n=%lld out of range", (long long)n);
    if (n == 0) return CRH_OK;
    if (!rows_dev || !out_codes_dev) return fail(CRH_E_INVALID, "gather_codes: NULL pointer");
    DeviceGuard g(h->device);
    if (!g.ok) return fail(CRH_E_HIP, "hipSetDevice(%d) failed", h->device);
    hipLaunchKernelGGL(k_gather_codes, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), n, rows_dev, row_base,
                       h->count, h->codes + (int64_t)col * h->cap_rows, out_codes_dev);
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

#ifdef CRH_ENABLE_DEBUG   // libcoderag_hip_debug.so only
int crh_debug_read_ceiling(crh_index *h, void *stream)
{
    if (!h) return fail(CRH_E_INVALID, "index is NULL");
    DeviceGuard g(h->device);
    const int64_t ntiles = ceil_div(h->count, kTileRows);
    if (ntiles == 0) return CRH_OK;
    CRH_TRY(ensure_workspace0(h));
    crh_index::Workspace &w = h->ws;
    return launch_scan<2>(h, w, scan_blocks(h, ntiles), static_cast<hipStream_t>(stream), h->alive, (int)ntiles, 1, w.ws_wave_cap, w.ws_qcap, h->status);
}

// Moves the int8 copy to a fresh allocation (the new one is taken BEFORE the old one is released, so it lands elsewhere): the
// speed of a pass depends on where the copy sits (tools/alloc_modes.py), this lets one index try several places.
int crh_debug_i8_move(crh_index *h)
{
    if (!h || !h->i8 || !h->x8) return fail(CRH_E_INVALID, "no int8 copy to move");
    DeviceGuard g(h->device);
    CRH_HIP(hipDeviceSynchronize());
    const int ks8 = h->dim / 32;
    u32x4 *nx = nullptr;
    float *ns = nullptr;
    CRH_HIP(hipMalloc(reinterpret_cast<void **>(&nx), (size_t)h->x8_cap_tiles * ks8 * 1024));
    CRH_HIP(hipMalloc(reinterpret_cast<void **>(&ns), (size_t)h->x8_cap_tiles * 32 * sizeof(float)));
    dev_free(h->x8);
    dev_free(h->srow);
    h->x8 = nx;
    h->srow = ns;
    h->i8_dirty_from = 0;
    return CRH_OK;
}

// What the int8 scan computes before it nominates: the interval of every (query, row), the quantisation parameters and the
// thresholds, all from the product's own launches (k_requant_i8, launch_prep with the integer images, k_scan_i8 PART 1 and PART 2).  Nothing
// here restates the arithmetic: the upper ends come from the `shi` record of a sample launch over EVERY tile (G = tiles, S = 1),
// both ends as f32 from the store that launch makes in this build only (crh_i8.hpp, g_i8_debug_ends), the thresholds from a
// second sample launch with the sample enqueue_batch would take, followed by the threshold launch.  Queries go through in
// batches of batch_q like a search's.  Host pointers throughout; the index must have no search pending.
int crh_debug_i8_intervals(crh_index *h, int nq, const float *queries, int k, const crh_filter *filters, int n_filters, float *hi_rec_out,
                           float *hi_out, float *lo_out, float *srow_out, float *qpar_out, float *dn_out, float *c_abs_out, float *tau_out)
{
    if (!h) return fail(CRH_E_INVALID, "index is NULL");
    if (nq < 1 || nq > kMaxQ || !queries) return fail(CRH_E_INVALID, "nq=%d outside 1..%d or no queries", nq, kMaxQ);
    if (!hi_rec_out || !hi_out || !lo_out || !srow_out || !qpar_out || !dn_out || !c_abs_out || !tau_out) return fail(CRH_E_INVALID, "NULL output pointer");
    if (n_filters < 0 || n_filters > CRH_MAX_FILTERS || (n_filters > 0 && !filters)) return fail(CRH_E_INVALID, "n_filters=%d outside 0..%d", n_filters, CRH_MAX_FILTERS);
    if (!h->pending.empty()) return fail(CRH_E_INVALID, "a search is pending: crh_search_finish first");
    const int64_t ntiles = ceil_div(h->count, kTileRows);
    if (ntiles < 1 || ntiles > kI8SampleTiles) return fail(CRH_E_INVALID, "%lld tiles outside 1..%d (the record of upper ends holds that many)", (long long)ntiles, kI8SampleTiles);
    if (!i8_use(h, 1, k)) return fail(CRH_E_INVALID, "this index does not nominate from an int8 copy at k=%d", k);
    DeviceGuard g(h->device);
    if (!g.ok) return fail(CRH_E_HIP, "hipSetDevice(%d) failed", h->device);
    hipStream_t st = nullptr;
    CRH_TRY(ensure_workspace0(h));
    crh_index::Workspace &w = h->ws;
    if ((int64_t)w.ws_seed * kWideQ < (int64_t)kMaxQ * ntiles) return fail(CRH_E_INVALID, "the sample keys of %lld tiles do not fit the workspace", (long long)ntiles);
    if (!w.shi) return fail(CRH_E_INVALID, "no memory for the record of upper ends");
    struct Tmp {
        float *p = nullptr;
        ~Tmp() { dev_free(p); }
    } q_dev, ends;
    const int64_t pitch = ntiles * 32, count = h->count;
    CRH_TRY(dev_alloc(&q_dev.p, (int64_t)nq * h->dim));
    CRH_TRY(dev_alloc(&ends.p, 2 * kMaxQ * pitch));
    CRH_HIP(hipMemcpy(q_dev.p, queries, (size_t)nq * h->dim * 4, hipMemcpyHostToDevice));
    FilterKey key;
    key_from_filters(filters, n_filters, key);
    const int QB = h->batch_q / 32;
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(ntiles, kI8Waves), h->cu_count));
    const int wave_cap = w.ws_wave_cap * (kWaves / kI8Waves), qcap = w.ws_qcap;
    const float c_abs = i8_c_abs(h);
    SearchStatus *stt = h->status;
    std::vector<uint32_t> rec((size_t)ntiles * QB * 2 * 64 * 4);
    for (int q0 = 0; q0 < nq; q0 += h->batch_q) {
        const int b = std::min(h->batch_q, nq - q0);
        MaskRef mask;
        CRH_TRY(build_mask(h, w, key, &mask, st));
        CRH_TRY(i8_sync(h, st));
        if (!i8_use(h, b, k)) return fail(CRH_E_INVALID, "no memory for the int8 copy");
        CRH_TRY(launch_prep(h, w, st, q_dev.p + (int64_t)q0 * h->dim, b, h->batch_q, stt, true));
        // every tile as a sample tile: the record of upper ends, and both ends as f32
        I8DebugEnds on{ends.p, ends.p + kMaxQ * pitch, pitch}, off{nullptr, nullptr, 0};
        CRH_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_i8_debug_ends), &on, sizeof(on)));
        const int rc = launch_scan_i8<1>(h, w, blocks, st, mask.mask, (int)ntiles, (int)ntiles, 1, k, c_abs, b, wave_cap, qcap, stt, w.shi);
        CRH_HIP(hipDeviceSynchronize());
        CRH_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_i8_debug_ends), &off, sizeof(off)));
        CRH_TRY(rc);
        CRH_HIP(hipMemcpy(rec.data(), w.shi, rec.size() * 4, hipMemcpyDeviceToHost));
        for (int q = 0; q < b; ++q) {
            CRH_HIP(hipMemcpy(hi_out + (int64_t)(q0 + q) * count, on.hi + (int64_t)q * pitch, (size_t)count * 4, hipMemcpyDeviceToHost));
            CRH_HIP(hipMemcpy(lo_out + (int64_t)(q0 + q) * count, on.lo + (int64_t)q * pitch, (size_t)count * 4, hipMemcpyDeviceToHost));
        }
        // the record's layout (crh_i8.hpp, `shi`): [tile][block][v][lane] of four words, two bf16 each; value 8 v + 2 e (+ 1) of a
        // lane is row (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of the tile for query 32 block + (lane & 31)
        for (int64_t t = 0; t < ntiles; ++t)
            for (int blk = 0; blk < QB; ++blk)
                for (int v = 0; v < 2; ++v)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int e = 0; e < 8; ++e) {
                            const uint32_t word = rec[((((size_t)t * QB + blk) * 2 + v) * 64 + lane) * 4 + (e >> 1)];
                            const uint32_t bits = (e & 1) ? (word & 0xffff0000u) : (word << 16);
                            const int r = 8 * v + e, q = blk * 32 + (lane & 31);
                            const int64_t row = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                            if (q < b && row < count) memcpy(hi_rec_out + (int64_t)(q0 + q) * count + row, &bits, 4);
                        }
        // the thresholds: the sample a search takes, then the threshold launch
        int G8, S8;
        i8_sample_plan(h, ntiles, &G8, &S8);
        u32x4 *shi = h->i8_sample_record ? w.shi : nullptr;
        CRH_TRY(launch_scan_i8<1>(h, w, blocks, st, mask.mask, (int)ntiles, G8, S8, k, c_abs, b, wave_cap, qcap, stt, shi));
        CRH_TRY(launch_scan_i8<2>(h, w, blocks, st, mask.mask, (int)ntiles, G8, S8, k, c_abs, b, wave_cap, qcap, stt, shi));
        CRH_HIP(hipDeviceSynchronize());
        CRH_HIP(hipMemcpy(tau_out + q0, w.tau, (size_t)b * 4, hipMemcpyDeviceToHost));
        CRH_HIP(hipMemcpy(qpar_out + (int64_t)q0 * 4, w.qpar, (size_t)b * 16, hipMemcpyDeviceToHost));
    }
    for (int64_t i = (int64_t)nq * 4; i < (int64_t)kMaxQ * 4; ++i) qpar_out[i] = 0.f;
    CRH_HIP(hipMemcpy(srow_out, h->srow, (size_t)count * 4, hipMemcpyDeviceToHost));
    CRH_HIP(hipMemcpy(dn_out, h->i8stat, 4, hipMemcpyDeviceToHost));
    *c_abs_out = c_abs;
    return CRH_OK;
}

// The product's instantiations of wg_kth_largest_fast / wg_kth_largest on the caller's key sets (k_debug_kth, crh_kernels.hpp).
int crh_debug_kth_largest(int variant, const void *keys, unsigned nsets, unsigned n, const unsigned *k, unsigned floor_key, unsigned nblocks,
                          unsigned long long *key_out)
{
    const bool u64 = (variant & CRH_DEBUG_SEL_U64) != 0;
    const int shape = variant & ~CRH_DEBUG_SEL_U64;
    if (variant < 0 || shape > CRH_DEBUG_SEL_RADIX_256) return fail(CRH_E_INVALID, "debug_kth_largest: unknown variant %d", variant);
    if (u64 && shape <= CRH_DEBUG_SEL_FAST_256) return fail(CRH_E_INVALID, "debug_kth_largest: wg_kth_largest_fast takes u32 keys (variant %d)", variant);
    if (u64 && shape == CRH_DEBUG_SEL_RADIX_512) return fail(CRH_E_INVALID, "debug_kth_largest: the product has no u64 radix select of 512 threads");
    if (!keys || !k || !key_out) return fail(CRH_E_INVALID, "debug_kth_largest: NULL pointer");
    if (nsets < 1 || nsets > 65535u || n < 1 || (uint64_t)nsets * n > (1ull << 28)) return fail(CRH_E_INVALID, "debug_kth_largest: nsets=%u, n=%u out of range", nsets, n);
    if (nblocks < 1 || nblocks > 65535u) return fail(CRH_E_INVALID, "debug_kth_largest: nblocks=%u outside 1..65535", nblocks);
    for (unsigned s = 0; s < nsets; ++s)
        if (k[s] < 1 || k[s] > n) return fail(CRH_E_INVALID, "debug_kth_largest: k[%u]=%u outside 1..n=%u", s, k[s], n);
    const size_t kbytes = (size_t)nsets * n * (u64 ? 8 : 4);
    DebugBuf<unsigned char> kd;
    DebugBuf<unsigned> ksd;
    DebugBuf<unsigned long long> mm;   // [2][nsets]: the smallest and the largest key any thread of a set's workgroup returned
    CRH_TRY(dev_alloc(&kd.p, (int64_t)kbytes));
    CRH_TRY(dev_alloc(&ksd.p, nsets));
    CRH_TRY(dev_alloc(&mm.p, 2 * (int64_t)nsets));
    CRH_HIP(hipMemcpy(kd.p, keys, kbytes, hipMemcpyHostToDevice));
    CRH_HIP(hipMemcpy(ksd.p, k, (size_t)nsets * 4, hipMemcpyHostToDevice));
    CRH_HIP(hipMemset(mm.p, 0xff, (size_t)nsets * 8));
    CRH_HIP(hipMemset(mm.p + nsets, 0, (size_t)nsets * 8));
    unsigned long long *kmin = mm.p, *kmax = mm.p + nsets;
    switch (variant) {
    case CRH_DEBUG_SEL_FAST_1024: launch_debug_kth<1024, 1024, uint32_t>(kd.p, nsets, n, ksd.p, floor_key, nblocks, kmin, kmax); break;
    case CRH_DEBUG_SEL_FAST_512: launch_debug_kth<512, 512, uint32_t>(kd.p, nsets, n, ksd.p, floor_key, nblocks, kmin, kmax); break;
    case CRH_DEBUG_SEL_FAST_256: launch_debug_kth<256, 256, uint32_t>(kd.p, nsets, n, ksd.p, floor_key, nblocks, kmin, kmax); break;
    case CRH_DEBUG_SEL_RADIX_1024: launch_debug_kth<1024, 0, uint32_t>(kd.p, nsets, n, ksd.p, floor_key, nblocks, kmin, kmax); break;
    case CRH_DEBUG_SEL_RADIX_512: launch_debug_kth<512, 0, uint32_t>(kd.p, nsets, n, ksd.p, floor_key, nblocks, kmin, kmax); break;
    case CRH_DEBUG_SEL_RADIX_256: launch_debug_kth<256, 0, uint32_t>(kd.p, nsets, n, ksd.p, floor_key, nblocks, kmin, kmax); break;
    case CRH_DEBUG_SEL_RADIX_1024 | CRH_DEBUG_SEL_U64: launch_debug_kth<1024, 0, unsigned long long>(kd.p, nsets, n, ksd.p, floor_key, nblocks, kmin, kmax); break;
    default: launch_debug_kth<256, 0, unsigned long long>(kd.p, nsets, n, ksd.p, floor_key, nblocks, kmin, kmax); break;
    }
    CRH_HIP(hipGetLastError());
    CRH_HIP(hipDeviceSynchronize());
    std::vector<unsigned long long> got(2 * (size_t)nsets);
    CRH_HIP(hipMemcpy(got.data(), mm.p, got.size() * 8, hipMemcpyDeviceToHost));
    for (unsigned s = 0; s < nsets; ++s) {
        if (got[s] != got[nsets + s])
            return fail(CRH_E_INTERNAL, "debug_kth_largest: the threads of set %u returned different keys (%llx .. %llx)", s, got[s], got[nsets + s]);
        key_out[s] = got[s];
    }
    return CRH_OK;
}

// select_tail<1024> (k_select's) or select_tail<256> (k_select_final's) on the caller's keys (k_debug_select_tail).
int crh_debug_select_tail(int variant, const unsigned long long *keys, unsigned Ms, int k, int64_t row_base, float *scores_out, int64_t *rows_out)
{
    if (variant != CRH_DEBUG_TAIL_1024 && variant != CRH_DEBUG_TAIL_256) return fail(CRH_E_INVALID, "debug_select_tail: unknown variant %d", variant);
    if (!keys || !scores_out || !rows_out) return fail(CRH_E_INVALID, "debug_select_tail: NULL pointer");
    if (Ms < 1 || Ms > (1u << 24)) return fail(CRH_E_INVALID, "debug_select_tail: Ms=%u outside 1..2^24", Ms);
    if (k < 1 || k > CRH_MAX_K) return fail(CRH_E_INVALID, "debug_select_tail: k=%d outside 1..%d", k, CRH_MAX_K);
    DebugBuf<unsigned long long> kd;
    DebugBuf<float> os;
    DebugBuf<int64_t> orow;
    CRH_TRY(dev_alloc(&kd.p, Ms));
    CRH_TRY(dev_alloc(&os.p, k));
    CRH_TRY(dev_alloc(&orow.p, k));
    CRH_HIP(hipMemcpy(kd.p, keys, (size_t)Ms * 8, hipMemcpyHostToDevice));
    CRH_HIP(hipMemset(os.p, 0x55, (size_t)k * 4));      // (an entry the helper leaves unwritten comes back as neither a score nor padding)
    CRH_HIP(hipMemset(orow.p, 0x55, (size_t)k * 8));
    if (variant == CRH_DEBUG_TAIL_1024)
        hipLaunchKernelGGL(k_debug_select_tail<1024>, dim3(1), dim3(1024), 0, nullptr, kd.p, Ms, k, row_base, os.p, orow.p);
    else
        hipLaunchKernelGGL(k_debug_select_tail<256>, dim3(1), dim3(256), 0, nullptr, kd.p, Ms, k, row_base, os.p, orow.p);
    CRH_HIP(hipGetLastError());
    CRH_HIP(hipDeviceSynchronize());
    CRH_HIP(hipMemcpy(scores_out, os.p, (size_t)k * 4, hipMemcpyDeviceToHost));
    CRH_HIP(hipMemcpy(rows_out, orow.p, (size_t)k * 8, hipMemcpyDeviceToHost));
    return CRH_OK;
}

// make_tile_list's two launches (launch_tile_list) on the caller's mask words.  list_out [ntiles] goes IN as well: what the
// caller put there is what the list buffer holds before the launches, so the entries past *len_out show what was left alone.
int crh_debug_tile_list(const uint32_t *mask_words, int64_t ntiles, uint32_t *list_out, uint32_t *len_out)
{
    if (!mask_words || !list_out || !len_out) return fail(CRH_E_INVALID, "debug_tile_list: NULL pointer");
    if (ntiles < 1 || ntiles > (1LL << 26)) return fail(CRH_E_INVALID, "debug_tile_list: ntiles=%lld outside 1..2^26", (long long)ntiles);
    DebugBuf<uint32_t> words, list;   // list: [ntiles] the list, then one count per workgroup, then the length (Workspace::tilelist)
    const int64_t nb = ceil_div(ntiles, 256);
    CRH_TRY(dev_alloc(&words.p, ntiles));
    CRH_TRY(dev_alloc(&list.p, ntiles + nb + 1));
    CRH_HIP(hipMemcpy(words.p, mask_words, (size_t)ntiles * 4, hipMemcpyHostToDevice));
    CRH_HIP(hipMemcpy(list.p, list_out, (size_t)ntiles * 4, hipMemcpyHostToDevice));
    CRH_HIP(hipMemset(list.p + ntiles, 0xff, (size_t)(nb + 1) * 4));
    launch_tile_list(words.p, ntiles, list.p + ntiles, list.p, list.p + ntiles + nb, nullptr);
    CRH_HIP(hipGetLastError());
    CRH_HIP(hipDeviceSynchronize());
    CRH_HIP(hipMemcpy(list_out, list.p, (size_t)ntiles * 4, hipMemcpyDeviceToHost));
    CRH_HIP(hipMemcpy(len_out, list.p + ntiles + nb, 4, hipMemcpyDeviceToHost));
    return CRH_OK;
}
#endif  // CRH_ENABLE_DEBUG

#ifdef CRH_FUSED_STAMPS   // a measurement build only (tools/fused_stamps.py): per-workgroup phase clocks of the last k_scan_fused
int crh_debug_fused_stamps(unsigned long long *out)
{
    CRH_HIP(hipDeviceSynchronize());
    CRH_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fused_stamps), sizeof(unsigned long long) * 256 * 24));
    return CRH_OK;
}
int crh_debug_select_stamps(unsigned long long *out)
{
    CRH_HIP(hipDeviceSynchronize());
    CRH_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_select_stamps), sizeof(unsigned long long) * 64 * 16));
    return CRH_OK;
}
#endif

int crh_index_set_nomination(crh_index *h, int mode)
{
    if (!h) return fail(CRH_E_INVALID, "index is NULL");
    if (mode < CRH_NOMINATE_BF16_3 || mode > CRH_NOMINATE_INT8) return fail(CRH_E_INVALID, "unknown nomination mode %d", mode);
    h->nominate_max = mode;
    if (mode == CRH_NOMINATE_INT8) h->i8_strikes = h->i8_cooldown = 0;   // asking for it again gives the copy another chance at once
    return CRH_OK;
}

int crh_index_get_nomination(crh_index *h, int *mode_out)
{
    if (!h || !mode_out) return fail(CRH_E_INVALID, "NULL argument");
    const bool one_launch = h->fused_scan && !h->fused_resting() && h->nominate_max >= CRH_NOMINATE_BF16 && h->seed_tiles == 4096 && h->ksteps != 64;
    *mode_out = i8_use(h, 1, 100) ? CRH_NOMINATE_INT8 : (one_launch ? CRH_NOMINATE_BF16 : CRH_NOMINATE_BF16_3);
    return CRH_OK;
}

int crh_index_set_tuning(crh_index *h, int seed_tiles, int wave_cand_cap, int query_cand_cap, int force_fallback)
{
    if (!h) return fail(CRH_E_INVALID, "index is NULL");
    if (seed_tiles > 0) h->seed_tiles = seed_tiles > 12288 ? 12288 : seed_tiles;  // k_tau keeps the sample column in LDS
    if (wave_cand_cap > 0) h->wave_cap = wave_cand_cap;
    if (query_cand_cap > 0) h->qcap = query_cand_cap;
    if (force_fallback >= 0) h->force_fallback = force_fallback;
    return CRH_OK;
}

static int search_args(crh_index *h, int nq, const float *queries, int k, float *out_scores, int64_t *out_rows)
{
    if (!h) return fail(CRH_E_INVALID, "index is NULL");
    if (nq < 0) return fail(CRH_E_INVALID, "nq < 0");
    if (nq == 0) return CRH_OK;
    if (!queries || !out_scores || !out_rows) return fail(CRH_E_INVALID, "NULL query or output pointer");
    if (k <= 0 || k > CRH_MAX_K) return fail(CRH_E_CAPACITY, "k=%d outside 1..%d", k, CRH_MAX_K);
    return CRH_OK;
}

int crh_search(crh_index *h, int nq, const float *queries, int queries_on_device, int k, const crh_filter *filters, int n_filters,
               int64_t row_base, float *out_scores, int64_t *out_rows, int out_on_device, void *stream)
{
    CRH_TRY(search_args(h, nq, queries, k, out_scores, out_rows));
    if (nq == 0) return CRH_OK;
    if (n_filters < 0 || n_filters > CRH_MAX_FILTERS) return fail(CRH_E_INVALID, "n_filters=%d outside 0..%d", n_filters, CRH_MAX_FILTERS);
    if (n_filters > 0 && !filters) return fail(CRH_E_INVALID, "filters is NULL");
    FilterKey key;
    key_from_filters(filters, n_filters, key);
    return search_key(h, nq, queries, queries_on_device, k, key, row_base, out_scores, out_rows, out_on_device, stream);
}

int crh_search_cond(crh_index *h, int nq, const float *queries, int queries_on_device, int k, const crh_condition *conds, int n_conds,
                    int64_t row_base, float *out_scores, int64_t *out_rows, int out_on_device, void *stream)
{
    CRH_TRY(search_args(h, nq, queries, k, out_scores, out_rows));
    if (nq == 0) return CRH_OK;
    FilterKey key;
    CRH_TRY(key_from_conditions(h, conds, n_conds, false, key, true));
    return search_key(h, nq, queries, queries_on_device, k, key, row_base, out_scores, out_rows, out_on_device, stream);
}

int crh_search_multi(crh_index *h, int nq, const float *queries, int queries_on_device, int k, const crh_condition *conds,
                     const int32_t *class_off, int n_classes, const int32_t *query_class, int64_t row_base, float *out_scores,
                     int64_t *out_rows, int out_on_device, void *stream)
{
    CRH_TRY(search_args(h, nq, queries, k, out_scores, out_rows));
    if (n_classes < 1 || n_classes > CRH_MAX_CLASSES) return fail(CRH_E_INVALID, "n_classes=%d outside 1..%d", n_classes, CRH_MAX_CLASSES);
    if (!class_off) return fail(CRH_E_INVALID, "class_off is NULL");
    if (class_off[0] < 0) return fail(CRH_E_INVALID, "class_off[0]=%d is negative", class_off[0]);
    FilterKey ckey(1, n_classes), key;
    for (int c = 0; c < n_classes; ++c) {
        const int n = class_off[c + 1] - class_off[c];
        if (n < 0) return fail(CRH_E_INVALID, "class_off is not ascending at class %d", c);
        CRH_TRY(key_from_conditions(h, n > 0 ? conds + class_off[c] : nullptr, n, false, key));
        ckey.insert(ckey.end(), key.begin(), key.end());
    }
    if (nq == 0) return CRH_OK;
    if (!query_class) return fail(CRH_E_INVALID, "query_class is NULL");
    for (int i = 0; i < nq; ++i)
        if (query_class[i] < 0 || query_class[i] >= n_classes)
            return fail(CRH_E_INVALID, "query_class[%d]=%d outside 0..%d", i, query_class[i], n_classes - 1);
    return search_multi_key(h, nq, queries, queries_on_device, k, ckey, query_class, row_base, out_scores, out_rows, out_on_device, stream);
}

int crh_search_range(crh_index *h, int nq, const float *queries, int queries_on_device, int k, const float *thresholds_host,
                     const crh_condition *conds, int n_conds, int64_t row_base, float *out_scores, int64_t *out_rows, int64_t *out_counts,
                     int out_on_device, void *stream)
{
    if (!h) return fail(CRH_E_INVALID, "index is NULL");
    if (nq < 0) return fail(CRH_E_INVALID, "nq < 0");
    if (k <= 0 || k > CRH_MAX_K) return fail(CRH_E_INVALID, "k=%d outside 1..%d", k, CRH_MAX_K);
    FilterKey key;
    CRH_TRY(key_from_conditions(h, conds, n_conds, false, key, true));
    if (nq == 0) return CRH_OK;
    if (!queries || !out_scores || !out_rows) return fail(CRH_E_INVALID, "NULL query or output pointer");
    if (!thresholds_host) return fail(CRH_E_INVALID, "thresholds_host is NULL");
    for (int i = 0; i < nq; ++i)
        if (!std::isfinite(thresholds_host[i])) return fail(CRH_E_INVALID, "thresholds_host[%d]=%g is not a finite number", i, (double)thresholds_host[i]);
    unsigned long long *cnt = reinterpret_cast<unsigned long long *>(out_counts);
    if (out_counts && !out_on_device) {
        DeviceGuard g(h->device);
        if (h->stage_cnt_elems < nq) {
            dev_free(h->stage_cnt);
            h->stage_cnt_elems = 0;
            CRH_TRY(dev_alloc(&h->stage_cnt, nq));
            h->stage_cnt_elems = nq;
        }
        cnt = h->stage_cnt;
    }
    CRH_TRY(search_range_key(h, nq, queries, queries_on_device, k, thresholds_host, key, row_base, out_scores, out_rows, cnt, out_on_device, stream));
    if (out_counts && !out_on_device) {   // (host outputs: the batches are finished, the totals final)
        DeviceGuard g(h->device);
        hipStream_t st = static_cast<hipStream_t>(stream);
        CRH_HIP(hipMemcpyAsync(out_counts, h->stage_cnt, sizeof(int64_t) * (size_t)nq, hipMemcpyDeviceToHost, st));
        CRH_HIP(hipStreamSynchronize(st));
    }
    return CRH_OK;
}

int crh_index_set_sparse_route(crh_index *h, int enable, int max_fraction_den)
{
    if (!h) return fail(CRH_E_INVALID, "index is NULL");
    if (enable >= 0) h->sparse_on = enable != 0;
    if (max_fraction_den > 0) h->sparse_den = max_fraction_den;
    return CRH_OK;
}

int crh_search_finish(crh_index *h, void *stream)
{
    if (!h) return fail(CRH_E_INVALID, "index is NULL");
    DeviceGuard g(h->device);
    (void)stream;   // (the batches know their streams; kept for the ABI and for callers that name the stream they work on)
    const int rc = finish_pending(h);
    h->stats_carry = false;
    return rc;
}

int crh_index_set_profiling(crh_index *h, int enable)
{
    if (!h) return fail(CRH_E_INVALID, "index is NULL");
    DeviceGuard g(h->device);
    if (enable && h->ev.empty()) {
        h->ev.resize(2 * kStatusSlots);
        for (auto &e : h->ev) CRH_HIP(hipEventCreate(&e));
    }
    h->profiling = enable != 0;
    h->profile_whole_scan = enable == 2;
    h->prof_scan_ms = 0.0;
    h->prof_scan_launches = 0;
    return CRH_OK;
}

int crh_index_get_profile(crh_index *h, double *scan_ms_total, int64_t *scan_launches)
{
    if (!h) return fail(CRH_E_INVALID, "index is NULL");
    if (scan_ms_total) *scan_ms_total = h->prof_scan_ms;
    if (scan_launches) *scan_launches = h->prof_scan_launches;
    return CRH_OK;
}

int crh_search_get_stats(crh_index *h, crh_search_stats *out)
{
    if (!h || !out) return fail(CRH_E_INVALID, "NULL argument");
    *out = h->stats;
    return CRH_OK;
}

int crh_merge_topk(int nlists, int nq, int k, const float *scores_dev, const int64_t *rows_dev, float *out_scores_dev,
                   int64_t *out_rows_dev, void *stream)
{
    return crh_merge_topk_strided(nlists, nq, k, scores_dev, rows_dev, (int64_t)nq * k, (int64_t)nq * k, out_scores_dev, out_rows_dev, stream);
}

int crh_merge_topk_strided(int nlists, int nq, int k, const float *scores_dev, const int64_t *rows_dev, int64_t score_list_stride,
                           int64_t row_list_stride, float *out_scores_dev, int64_t *out_rows_dev, void *stream)
{
    if (nlists <= 0 || nq < 0 || k <= 0) return fail(CRH_E_INVALID, "bad merge shape nlists=%d nq=%d k=%d", nlists, nq, k);
    if (score_list_stride < (int64_t)nq * k || row_list_stride < (int64_t)nq * k)
        return fail(CRH_E_INVALID, "merge list strides %lld / %lld are shorter than a list of %d x %d", (long long)score_list_stride,
                    (long long)row_list_stride, nq, k);
    if (nq == 0) return CRH_OK;
    if (!scores_dev || !rows_dev || !out_scores_dev || !out_rows_dev) return fail(CRH_E_INVALID, "NULL pointer");
    const int total = nlists * k;
    if (total > 8192) return fail(CRH_E_CAPACITY, "nlists*k=%d exceeds 8192", total);
    int P = 1;
    while (P < total) P <<= 1;
    const size_t lds = (size_t)P * 4 + 8 + (size_t)P * 8;   // 96 KiB at P = 8192: above the 64 KiB a launch gets by default
    static OncePerDevice once;
    if (once.need()) CRH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_merge_topk), hipFuncAttributeMaxDynamicSharedMemorySize, 8192 * 12 + 8));
    hipLaunchKernelGGL(k_merge_topk, dim3(nq), dim3(1024), lds, static_cast<hipStream_t>(stream), nlists, nq, k, scores_dev, rows_dev,
                       score_list_stride, row_list_stride, out_scores_dev, out_rows_dev);
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

static int match_key(crh_index *h, const FilterKey &key, int64_t limit, int64_t *rows_out_host, int64_t *n_out)
{
    DeviceGuard g(h->device);
    CRH_TRY(ensure_workspace0(h));
    MaskRef m;
    CRH_TRY(build_mask(h, h->ws, key, &m, nullptr));
    const int64_t ntiles = ceil_div(h->count, 32);
    std::vector<uint32_t> hm((size_t)ntiles);
    CRH_HIP(hipMemcpy(hm.data(), m.mask, (size_t)ntiles * 4, hipMemcpyDeviceToHost));
    int64_t found = 0;
    for (int64_t t = 0; t < ntiles && found < limit; ++t) {
        uint32_t m = hm[(size_t)t];
        while (m && found < limit) {
            const int b = __builtin_ctz(m);
            m &= m - 1;
            if (rows_out_host) rows_out_host[found] = t * 32 + b;
            ++found;
        }
    }
    *n_out = found;
    return CRH_OK;
}

int crh_index_match_rows(crh_index *h, const crh_filter *filters, int n_filters, int64_t limit, int64_t *rows_out_host, int64_t *n_out)
{
    if (!h || !n_out) return fail(CRH_E_INVALID, "NULL argument");
    *n_out = 0;
    if (limit <= 0 || h->count == 0) return CRH_OK;   // (rows_out_host == NULL: count only, up to `limit`)
    if (n_filters < 0 || n_filters > CRH_MAX_FILTERS) return fail(CRH_E_INVALID, "n_filters=%d outside 0..%d", n_filters, CRH_MAX_FILTERS);
    if (n_filters > 0 && !filters) return fail(CRH_E_INVALID, "filters is NULL");
    FilterKey key;
    key_from_filters(filters, n_filters, key);
    return match_key(h, key, limit, rows_out_host, n_out);
}

int crh_index_match_rows_cond(crh_index *h, const crh_condition *conds, int n_conds, int64_t limit, int64_t *rows_out_host, int64_t *n_out)
{
    if (!h || !n_out) return fail(CRH_E_INVALID, "NULL argument");
    *n_out = 0;
    FilterKey key;
    CRH_TRY(key_from_conditions(h, conds, n_conds, false, key, true));
    if (limit <= 0 || h->count == 0) return CRH_OK;   // (rows_out_host == NULL: count only, up to `limit`)
    return match_key(h, key, limit, rows_out_host, n_out);
}

// The validity words of a search under these conditions, for a structure beside the index (crh_lex): the mask build_mask
// hands a search -- the alive words without a condition -- copied out in stream order.
int crh_index_row_mask(crh_index *h, const crh_condition *conds, int n_conds, uint32_t *out_mask_dev, int64_t n_words, void *stream)
{
    if (!h) return fail(CRH_E_INVALID, "index is NULL");
    FilterKey key;
    CRH_TRY(key_from_conditions(h, conds, n_conds, false, key, true));
    const int64_t ntiles = ceil_div(h->count, kTileRows);
    if (n_words < ntiles) return fail(CRH_E_INVALID, "row_mask: n_words=%lld, the index has %lld tiles", (long long)n_words, (long long)ntiles);
    if (ntiles == 0) return CRH_OK;
    if (!out_mask_dev) return fail(CRH_E_INVALID, "out_mask_dev is NULL");
    DeviceGuard g(h->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    CRH_TRY(ensure_workspace0(h));
    MaskRef m;
    CRH_TRY(build_mask(h, h->ws, key, &m, st));
    CRH_HIP(hipMemcpyAsync(out_mask_dev, m.mask, (size_t)ntiles * 4, hipMemcpyDeviceToDevice, st));
    return CRH_OK;
}

static int facet_args(crh_index *h, int col, int n_bins, const char *what)
{
    if (!h) return fail(CRH_E_INVALID, "index is NULL");
    if (col < 0 || col >= h->ncols) return fail(CRH_E_INVALID, "%s: column %d outside 0..%d", what, col, h->ncols - 1);
    if (n_bins < 1) return fail(CRH_E_INVALID, "%s: n_bins=%d must be >= 1", what, n_bins);
    return CRH_OK;
}

// The histogram of one code column over the rows a search under these conditions would see (crh_facet.hpp): the mask is the
// one build_mask hands a search, found in its cache or built; the outputs are cleared and counted into in stream order.
int crh_index_facet(crh_index *h, int col, const crh_condition *conds, int n_conds, int n_bins, int64_t *out_bins_dev, int64_t *out_info_dev,
                    void *stream)
{
    CRH_TRY(facet_args(h, col, n_bins, "facet"));
    FilterKey key;
    CRH_TRY(key_from_conditions(h, conds, n_conds, false, key, true));
    if (!out_bins_dev || !out_info_dev) return fail(CRH_E_INVALID, "facet: NULL output pointer");
    DeviceGuard g(h->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned long long *bins = reinterpret_cast<unsigned long long *>(out_bins_dev), *info = reinterpret_cast<unsigned long long *>(out_info_dev);
    CRH_TRY(facet_zero(bins, info, 1, n_bins, st));
    if (h->count == 0) return CRH_OK;
    CRH_TRY(ensure_workspace0(h));
    MaskRef m;
    CRH_TRY(build_mask(h, h->ws, key, &m, st));
    const int32_t *column = h->codes + (int64_t)col * h->cap_rows;
    const unsigned blocks = (unsigned)std::min<int64_t>(ceil_div(h->count, 256), (int64_t)h->cu_count * 8);
    if (n_bins <= kFacetLdsBins)
        hipLaunchKernelGGL(k_facet_count<true>, dim3(blocks), dim3(256), 0, st, m.mask, column, h->count, n_bins, bins, info);
    else
        hipLaunchKernelGGL(k_facet_count<false>, dim3(blocks), dim3(256), 0, st, m.mask, column, h->count, n_bins, bins, info);
    CRH_HIP(hipGetLastError());
    return CRH_OK;
}

// The semantic form: a range batch with counts whose k_range_count also adds every counted row to its query's bins.  The
// lists (k = 1) stay in the index's staging.  The batches are finished before the call returns -- a batch whose candidate
// lists overflowed has to be run again, and the staging must not outlive the call -- so the outputs are final in stream order.
int crh_search_range_facet(crh_index *h, int nq, const float *queries, int queries_on_device, const float *thresholds_host,
                           const crh_condition *conds, int n_conds, int col, int n_bins, int64_t *out_bins_dev, int64_t *out_info_dev, void *stream)
{
    CRH_TRY(facet_args(h, col, n_bins, "range facet"));
    if (nq < 0) return fail(CRH_E_INVALID, "nq < 0");
    FilterKey key;
    CRH_TRY(key_from_conditions(h, conds, n_conds, false, key, true));
    if (nq == 0) return CRH_OK;
    if (!queries || !out_bins_dev || !out_info_dev) return fail(CRH_E_INVALID, "NULL query or output pointer");
    if (!thresholds_host) return fail(CRH_E_INVALID, "thresholds_host is NULL");
    for (int i = 0; i < nq; ++i)
        if (!std::isfinite(thresholds_host[i])) return fail(CRH_E_INVALID, "thresholds_host[%d]=%g is not a finite number", i, (double)thresholds_host[i]);
    {
        DeviceGuard g(h->device);
        CRH_TRY(ensure_stage_out(h, nq));
        if (h->stage_cnt_elems < nq) {
            dev_free(h->stage_cnt);
            h->stage_cnt_elems = 0;
            CRH_TRY(dev_alloc(&h->stage_cnt, nq));
            h->stage_cnt_elems = nq;
        }
    }
    CRH_TRY(search_range_key(h, nq, queries, queries_on_device, 1, thresholds_host, key, 0, h->stage_os, h->stage_or, h->stage_cnt, 1, stream, col,
                             n_bins, reinterpret_cast<unsigned long long *>(out_bins_dev), reinterpret_cast<unsigned long long *>(out_info_dev)));
    DeviceGuard g(h->device);
    const int rc = finish_pending(h);
    h->stats_carry = false;
    return rc;
}

}  // extern "C"
