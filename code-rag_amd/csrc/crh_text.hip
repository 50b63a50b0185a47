// crh_text.hip -- literal substring match (k_text_match), regular-expression match by byte DFA (k_text_regex) and approximate
// substring match within a bounded edit distance (k_text_fuzzy; both described where they stand) over the chunks' text in HBM
// (gfx950 / CDNA4 only).
//
// Replaces what Qdrant answers for FieldCondition(key, match=MatchText(text)) on a field WITHOUT a full-text index: an exact
// substring match ("chunks that contain `retry_after=`").  The definition is THIS repository's (tests/text_cases.py
// restates it with bytes.find and tests/test_text_gpu.py compares word for word).
//
// A crh_text handle is an ARENA whose rows are numbered like the rows of the crh_index beside it: row_off int64 [rows + 1] and the
// rows' bytes one behind the other.  kTextSlack zeroed bytes follow the last byte, also after a growth: the kernel's loads are
// 16-byte aligned and start below `end`, its look-ahead dword is 4-byte aligned and starts below `end`, so neither leaves them.
//
// k_text_match, one wave per 32-row tile (the dense index's tile and mask word): a tile whose mask word is 0 writes 0 and reads no
// byte.  Otherwise the tile's bytes -- one contiguous range, taken from the 16-byte boundary at or below its first byte -- are
// streamed kTextLane bytes per lane per step, kTextSteps steps in flight.  A lane tests its 16 start positions: the 4 bytes at
// position j are v_alignbyte of two neighbouring dwords, the fifth dword is the first dword of the next lane (of lane 0 of the next
// step for lane 63; one look-ahead dword behind the window for its last step).  Each is compared under a mask with every
// pattern's first min(4, len) bytes; the minimum over positions and patterns is 0 iff some position survives.  Survivors are rare:
// a ballot finds them, and only then are the per-pattern position masks made.  A survivor's row is counted from the 33 offsets
// the wave holds in its lanes; it matches iff the whole pattern lies inside the row and -- beyond 4 bytes -- a byte-per-lane
// compare agrees.  A row that is settled (matched, masked out, or too short from here on) drops its remaining survivors at once.
// Row bits per pattern are wave-uniform registers; at the end of the tile they are combined, ANDed with the mask word and stored
// by lane 0: one plain store per tile, no atomic on the result path, no dependence on which wave took which tile.  The count is
// one integer atomic per wave.
//
// Patterns travel as kernel arguments: their first words and masks stay in SGPRs, their bytes are copied to LDS once per
// workgroup.  The pattern list is padded to 1, 2, 4 or 8 entries by repeating its first pattern (ALL and ANY are both idempotent),
// so the inner loops unroll over a compile-time count and no register array is indexed at run time.
#include <algorithm>
#include <cstring>
#include <vector>

#include "crh_common.h"

namespace crh {
namespace {

typedef __attribute__((ext_vector_type(4))) unsigned int text_u32x4;

constexpr int kTextWaves = 4;                           // waves per workgroup
constexpr int kTextLane = 16;                           // bytes a lane loads per step
constexpr int kTextStep = 64 * kTextLane;               // bytes a wave covers per step (1024)
constexpr int kTextSteps = 4;                           // steps a wave has in flight
constexpr int kTextWindow = kTextSteps * kTextStep;     // 4096
constexpr int64_t kTextSlack = 64;                      // zeroed bytes kept behind the arena's last byte

struct TextArgs {
    const int64_t *row_off;
    const uint8_t *bytes;
    int64_t rows;
    const uint32_t *mask;        // one word per tile, or nullptr: every row
    uint32_t *out;               // one word per tile
    unsigned long long *count;   // += set bits
    int combine;
    int len[CRH_TEXT_MAX_PATTERNS];
    uint32_t fw[CRH_TEXT_MAX_PATTERNS];      // first min(4, len) bytes, little endian (folded when the match folds)
    uint32_t fm[CRH_TEXT_MAX_PATTERNS];      // their byte mask
    uint32_t pat[CRH_TEXT_MAX_PATTERNS * CRH_TEXT_MAX_PATTERN_BYTES / 4];   // the patterns' bytes, 64 per pattern
};

// ASCII 'A'..'Z' -> 'a'..'z' in each byte of x; every other byte (0x80.. included) as it is
__host__ __device__ __forceinline__ uint32_t text_fold4(uint32_t x)
{
    const uint32_t y = x & 0x7f7f7f7fu;
    const uint32_t ge_a = y + 0x3f3f3f3fu;   // bit 7 of a byte: y >= 0x41
    const uint32_t gt_z = y + 0x25252525u;   // bit 7 of a byte: y >= 0x5b
    return x | ((ge_a & ~gt_z & ~x & 0x80808080u) >> 2);
}

// the 4 bytes at byte offset j (0..15) of the 20 bytes d[0..4]
template <int J>
__device__ __forceinline__ uint32_t text_word(const uint32_t (&d)[5])
{
    if (J % 4 == 0) return d[J / 4];
    return __builtin_amdgcn_alignbyte(d[J / 4 + 1], d[J / 4], (uint32_t)(J % 4));
}

template <int J, int NP>
__device__ __forceinline__ void text_min(const uint32_t (&d)[5], const TextArgs &a, uint32_t &mn)
{
    const uint32_t w = text_word<J>(d);
#pragma unroll
    for (int p = 0; p < NP; ++p) mn = min(mn, (w ^ a.fw[p]) & a.fm[p]);
    if constexpr (J + 1 < kTextLane) text_min<J + 1, NP>(d, a, mn);
}

template <int J>
__device__ __forceinline__ uint32_t text_hits(const uint32_t (&d)[5], uint32_t fw, uint32_t fm)
{
    const uint32_t h = (((text_word<J>(d) ^ fw) & fm) == 0u ? 1u : 0u) << J;
    if constexpr (J + 1 < kTextLane) return h | text_hits<J + 1>(d, fw, fm);
    return h;
}

template <int NP, bool FOLD>
__global__ __launch_bounds__(kTextWaves * 64) void k_text_match(const TextArgs a)
{
    __shared__ uint32_t lpat32[NP * CRH_TEXT_MAX_PATTERN_BYTES / 4];
    for (int i = threadIdx.x; i < NP * CRH_TEXT_MAX_PATTERN_BYTES / 4; i += kTextWaves * 64) lpat32[i] = a.pat[i];
    __syncthreads();
    const uint8_t *lpat = reinterpret_cast<const uint8_t *>(lpat32);

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t ntiles = (a.rows + 31) / 32;
    unsigned int found = 0u;   // set bits this wave has written (wave-uniform)

    for (int64_t t = (int64_t)blockIdx.x * kTextWaves + wave; t < ntiles; t += (int64_t)gridDim.x * kTextWaves) {
        const int64_t r0 = t * 32;
        const int nrow = (int)(a.rows - r0 < 32 ? a.rows - r0 : 32);
        uint32_t m = a.mask ? a.mask[t] : 0xffffffffu;
        if (nrow < 32) m &= (1u << nrow) - 1u;
        m = __builtin_amdgcn_readfirstlane(m);
        if (m == 0u) {                                                    // (wave-uniform) nothing of the tile is read
            if (lane == 0) a.out[t] = 0u;
            continue;
        }
        const int64_t myoff = a.row_off[r0 + (lane < nrow ? lane : nrow)];   // lanes 0..nrow: the tile's offsets; the rest repeat the end
        const int64_t begin = __shfl(myoff, 0), end = __shfl(myoff, nrow);
        uint32_t rb[NP];                                                  // per pattern: the rows that hold it (wave-uniform)
#pragma unroll
        for (int p = 0; p < NP; ++p) rb[p] = 0u;

        for (int64_t s0 = begin & ~(int64_t)(kTextLane - 1); s0 < end; s0 += kTextWindow) {
            text_u32x4 w[kTextSteps];
#pragma unroll
            for (int u = 0; u < kTextSteps; ++u) {
                const int64_t at = s0 + (int64_t)u * kTextStep + lane * kTextLane;
                w[u] = at < end ? *reinterpret_cast<const text_u32x4 *>(a.bytes + at) : text_u32x4{0u, 0u, 0u, 0u};
            }
            uint32_t ahead = s0 + kTextWindow < end ? *reinterpret_cast<const uint32_t *>(a.bytes + s0 + kTextWindow) : 0u;
            if (FOLD) {
#pragma unroll
                for (int u = 0; u < kTextSteps; ++u) {
                    w[u].x = text_fold4(w[u].x);
                    w[u].y = text_fold4(w[u].y);
                    w[u].z = text_fold4(w[u].z);
                    w[u].w = text_fold4(w[u].w);
                }
                ahead = text_fold4(ahead);
            }
#pragma unroll
            for (int u = 0; u < kTextSteps; ++u) {
                const int64_t e0 = s0 + (int64_t)u * kTextStep;
                if (e0 >= end) break;
                const int64_t lb = e0 + lane * kTextLane;                 // the lane's first position
                const uint32_t next0 = u + 1 < kTextSteps ? __shfl(w[u + 1].x, 0) : ahead;
                uint32_t d4 = __shfl_down(w[u].x, 1);
                if (lane == 63) d4 = next0;
                const uint32_t d[5] = {w[u].x, w[u].y, w[u].z, w[u].w, d4};
                uint32_t mn = 0xffffffffu;
                text_min<0, NP>(d, a, mn);
                if (__ballot(mn == 0u && lb < end && lb + kTextLane > begin) == 0ull) continue;
                // positions of the lane inside the tile's bytes: [max(begin - lb, 0), min(end - lb, 16))
                const int64_t vlo = begin - lb, vhi = end - lb;
                uint32_t valid = vhi >= kTextLane ? 0xffffu : vhi <= 0 ? 0u : (1u << (int)vhi) - 1u;
                if (vlo > 0) valid &= vlo >= kTextLane ? 0u : ~((1u << (int)vlo) - 1u);
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    const int len = a.len[p];
                    uint32_t hits = mn == 0u ? text_hits<0>(d, a.fw[p], a.fm[p]) & valid : 0u;
                    unsigned long long hm;
                    while ((hm = __ballot(hits != 0u)) != 0ull) {
                        const int L = __ffsll((long long)hm) - 1;
                        const uint32_t hl = __builtin_amdgcn_readlane(hits, L);
                        const int j = __ffs((int)hl) - 1;
                        const int64_t pos = e0 + (int64_t)L * kTextLane + j;
                        const int r = __popcll(__ballot(myoff <= pos)) - 1;   // the last row that starts at or before pos: the row pos lies in
                        const int64_t rend = __shfl(myoff, r + 1);
                        bool settled = !((m >> r) & 1u) || ((rb[p] >> r) & 1u) || pos + len > rend;
                        if (!settled) {
                            bool same = true;
                            if (len > 4) {                                // (the first 4 bytes are the masked compare above)
                                uint32_t tb = 0u, pb = 0u;
                                if (lane < len) {
                                    tb = a.bytes[pos + lane];
                                    if (FOLD && tb >= 'A' && tb <= 'Z') tb |= 0x20u;
                                    pb = lpat[p * CRH_TEXT_MAX_PATTERN_BYTES + lane];
                                }
                                same = __ballot(tb != pb) == 0ull;
                            }
                            if (same) {
                                rb[p] |= 1u << r;
                                settled = true;
                            }
                        }
                        if (settled) {                                    // nothing more to learn from this row: drop its positions
                            const int64_t dr = rend - lb;
                            if (dr > 0) hits &= dr >= kTextLane ? 0u : ~((1u << (int)dr) - 1u);
                        } else if (lane == L) {
                            hits &= hits - 1u;
                        }
                    }
                }
            }
        }
        uint32_t res = rb[0];
#pragma unroll
        for (int p = 1; p < NP; ++p) res = a.combine == CRH_TEXT_ANY ? (res | rb[p]) : (res & rb[p]);
        res = __builtin_amdgcn_readfirstlane(res & m);
        if (lane == 0) a.out[t] = res;
        found += (unsigned int)__popc(res);
    }
    if (lane == 0 && found) atomicAdd(a.count, (unsigned long long)found);
}

// ---- k_text_regex: a byte DFA walked over every row
//
// One wave per PAIR of 32-row tiles, one lane per row; pairs are strided over the waves of the grid as the tiles are above.  A pair
// whose two mask words are 0 stores zeros and reads no byte.  The DFA's image -- the class map (256 bytes) and the table with one
// more column than the caller's, the SKIP column whose entry is the state itself -- is copied from the handle's buffer to dynamic
// LDS once per workgroup; the LDS request is the size of THIS DFA, so a small one keeps full occupancy.  A lane streams its own
// row with 16-byte aligned loads from `off[r] & ~15` to below `off[r + 1]` (so at most 15 bytes behind the row's end are read: the
// arena's last row stays inside kTextSlack), the next load issued before the current 16 bytes are walked.  A byte outside
// [begin, end) takes the SKIP class, so the walk has no branch and the predicate is off the dependent chain: per byte the chain is
// one multiply-add and one LDS byte read.  The wave loops while any lane has bytes left and is not in the (absorbing) accept
// state; then every lane feeds END.  A wave takes as long as its longest row; one very long row is a serial walk.  The two result
// words are the halves of one ballot, ANDed with the mask words, stored by lane 0 -- the second only if that tile exists; the
// count is one integer atomic per wave.
constexpr int kRegexClassMap = 256;                     // bytes of the class map in front of the table in the image
constexpr int kRegexImageMax = kRegexClassMap + CRH_REGEX_MAX_TABLE_BYTES + CRH_REGEX_MAX_STATES;   // (the SKIP column: one byte per state)

struct RegexArgs {
    const int64_t *row_off;
    const uint8_t *bytes;
    int64_t rows;
    const uint32_t *mask;        // one word per tile, or nullptr: every row
    uint32_t *out;               // one word per tile
    unsigned long long *count;   // += set bits
    const uint32_t *image;       // image_words dwords: class map, then table [n_states][ncols]
    int image_words;
    int ncols;                   // the caller's n_classes + 1: column ncols - 1 is SKIP
    int end_class;
    int accept;
};

template <int J>
__device__ __forceinline__ void regex_classes(const text_u32x4 &w, int lo, int hi, uint32_t skip, const uint8_t *lds, uint32_t (&c)[kTextLane])
{
    const uint32_t d = J / 4 == 0 ? w.x : J / 4 == 1 ? w.y : J / 4 == 2 ? w.z : w.w;
    const uint32_t cls = lds[(d >> (8 * (J % 4))) & 0xffu];
    c[J] = (J >= lo && J < hi) ? cls : skip;
    if constexpr (J + 1 < kTextLane) regex_classes<J + 1>(w, lo, hi, skip, lds, c);
}

__global__ __launch_bounds__(kTextWaves * 64) void k_text_regex(const RegexArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t regex_lds[];
    for (int i = threadIdx.x; i < a.image_words; i += kTextWaves * 64) regex_lds[i] = a.image[i];
    __syncthreads();
    const uint8_t *lmap = reinterpret_cast<const uint8_t *>(regex_lds);
    const uint8_t *ltab = lmap + kRegexClassMap;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t ntiles = (a.rows + 31) / 32, npairs = (ntiles + 1) / 2;
    const uint32_t ncols = (uint32_t)a.ncols, skip = ncols - 1u, accept = (uint32_t)a.accept;
    unsigned int found = 0u;   // set bits this wave has written (wave-uniform)

    for (int64_t pr = (int64_t)blockIdx.x * kTextWaves + wave; pr < npairs; pr += (int64_t)gridDim.x * kTextWaves) {
        const int64_t t0 = pr * 2, r0 = pr * 64;
        const bool second = t0 + 1 < ntiles;                              // (wave-uniform) does the pair's second tile exist?
        uint32_t m0 = a.mask ? a.mask[t0] : 0xffffffffu;
        uint32_t m1 = second ? (a.mask ? a.mask[t0 + 1] : 0xffffffffu) : 0u;
        const int64_t left = a.rows - r0;                                 // >= 1
        if (left < 32) m0 &= (1u << (int)left) - 1u;
        if (left < 64) m1 &= left <= 32 ? 0u : (1u << (int)(left - 32)) - 1u;
        m0 = __builtin_amdgcn_readfirstlane(m0);
        m1 = __builtin_amdgcn_readfirstlane(m1);
        if ((m0 | m1) == 0u) {                                            // (wave-uniform) nothing of the pair is read
            if (lane == 0) {
                a.out[t0] = 0u;
                if (second) a.out[t0 + 1] = 0u;
            }
            continue;
        }
        const bool active = (((lane < 32 ? m0 : m1) >> (lane & 31)) & 1u) != 0u;   // (a set bit is a row below `rows`)
        int64_t begin = 0, end = 0;
        if (active) {
            begin = a.row_off[r0 + lane];
            end = a.row_off[r0 + lane + 1];
        }
        int64_t p = begin < end ? begin & ~(int64_t)(kTextLane - 1) : end;
        uint32_t s = 0u;
        text_u32x4 cur = p < end ? *reinterpret_cast<const text_u32x4 *>(a.bytes + p) : text_u32x4{0u, 0u, 0u, 0u};
        while (__ballot(p < end && s != accept) != 0ull) {
            const int64_t pn = p + kTextLane;
            // (unconditional, so that nothing waits for it before the walk: a lane without a next chunk reloads the arena's first)
            const text_u32x4 nxt = *reinterpret_cast<const text_u32x4 *>(a.bytes + (pn < end ? pn : 0));
            // the lane's bytes of this chunk that lie inside its row: [lo, hi) of 0..16 (none once p >= end)
            const int64_t dlo = begin - p, dhi = end - p;
            const int lo = dlo > 0 ? (int)dlo : 0;
            const int hi = dhi >= kTextLane ? kTextLane : dhi > 0 ? (int)dhi : 0;
            uint32_t c[kTextLane];
            regex_classes<0>(cur, lo, hi, skip, lmap, c);                 // (independent of the state: off the chain)
#pragma unroll
            for (int j = 0; j < kTextLane; ++j) s = ltab[__umul24(s, ncols) + c[j]];   // (s < 256, ncols <= 258)
            p = pn;
            cur = nxt;
        }
        s = ltab[__umul24(s, ncols) + (uint32_t)a.end_class];
        const unsigned long long hit = __ballot(active && s == accept);
        const uint32_t w0 = (uint32_t)hit & m0, w1 = (uint32_t)(hit >> 32) & m1;
        if (lane == 0) {
            a.out[t0] = w0;
            if (second) a.out[t0 + 1] = w1;
        }
        found += (unsigned int)(__popc(w0) + __popc(w1));
    }
    if (lane == 0 && found) atomicAdd(a.count, (unsigned long long)found);
}

// ---- k_text_fuzzy: approximate substring match, at most CRH_FUZZY_MAX_EDITS byte edits
//
// A row's DISTANCE is min over its substrings S of Levenshtein(P, S) = min_j D[m][j] of Sellers' table (D[0][j] = 0, D[i][0] = i);
// level d of the output holds the rows whose distance is <= d.  The lane and tile shape is k_text_regex's: one wave per pair of
// tiles, one lane per row, the same 16-byte aligned loads (so the same bound: at most 15 bytes behind a row's end, inside
// kTextSlack), a pair whose mask words are 0 stores zeros in every level and reads no byte.  A lane keeps one column of the table
// as Myers' two difference vectors (Pv: D[i][j] - D[i-1][j] = +1, Mv: = -1; bit i - 1 is row i) in a W = 32- or 64-bit word and
// D[m][j] as a running score; the best score is the row's distance, exact for every level at once.  Bits at and above m hold
// garbage that never comes down: the column step carries and shifts upwards only.  The equality table Peq[byte] (bit i: P[i]
// equals the byte; with fold_case the ASCII letters of both sides folded, so the text itself is never folded) is made in LDS
// once per workgroup, thread b making entry b from the pattern in the kernel's arguments; its lookup depends on the text byte
// alone and the 16 of a chunk are issued before the chunk's first column step.  A byte outside the lane's [begin, end) is walked
// like any other and its step discarded by selects, so the walk has no divergent branch.  A lane whose best score is 0 is
// settled; the wave loops while any lane has bytes left and is not.  Each level is one ballot ANDed with the mask words and stored
// by lane 0; each level's count is one integer atomic per wave.
struct FuzzyArgs {
    const int64_t *row_off;
    const uint8_t *bytes;
    int64_t rows;
    const uint32_t *mask;        // one word per tile, or nullptr: every row
    uint32_t *out;               // [k + 1][ntiles]
    unsigned long long *count;   // [k + 1], += set bits
    int m, k, fold;
    uint32_t pat[CRH_TEXT_MAX_PATTERN_BYTES / 4];   // the pattern's bytes (folded when the match folds), zeros behind
};

template <typename W, int J>
__device__ __forceinline__ void fuzzy_eqs(const text_u32x4 &w, const W *peq, W (&eq)[kTextLane])
{
    const uint32_t d = J / 4 == 0 ? w.x : J / 4 == 1 ? w.y : J / 4 == 2 ? w.z : w.w;
    eq[J] = peq[(d >> (8 * (J % 4))) & 0xffu];
    if constexpr (J + 1 < kTextLane) fuzzy_eqs<W, J + 1>(w, peq, eq);
}

template <typename W>
__global__ __launch_bounds__(kTextWaves * 64) void k_text_fuzzy(const FuzzyArgs a)
{
    static_assert(kTextWaves * 64 == 256, "one thread per entry of the equality table");
    __shared__ W peq[256];
    {
        uint32_t b = threadIdx.x;                                         // (kTextWaves * 64 == 256: one entry per thread)
        if (a.fold && b >= 'A' && b <= 'Z') b |= 0x20u;
        W e = 0;
#pragma unroll
        for (int i = 0; i < (int)sizeof(W) * 8; ++i)
            if (i < a.m && ((a.pat[i / 4] >> (8 * (i % 4))) & 0xffu) == b) e |= (W)1 << i;
        peq[threadIdx.x] = e;
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t ntiles = (a.rows + 31) / 32, npairs = (ntiles + 1) / 2;
    const int m = a.m, k = a.k;
    const W top = (W)1 << (m - 1);
    unsigned int found[CRH_FUZZY_MAX_EDITS + 1] = {0u, 0u, 0u, 0u};      // per level: set bits this wave has written (wave-uniform)

    for (int64_t pr = (int64_t)blockIdx.x * kTextWaves + wave; pr < npairs; pr += (int64_t)gridDim.x * kTextWaves) {
        const int64_t t0 = pr * 2, r0 = pr * 64;
        const bool second = t0 + 1 < ntiles;                              // (wave-uniform) does the pair's second tile exist?
        uint32_t m0 = a.mask ? a.mask[t0] : 0xffffffffu;
        uint32_t m1 = second ? (a.mask ? a.mask[t0 + 1] : 0xffffffffu) : 0u;
        const int64_t left = a.rows - r0;                                 // >= 1
        if (left < 32) m0 &= (1u << (int)left) - 1u;
        if (left < 64) m1 &= left <= 32 ? 0u : (1u << (int)(left - 32)) - 1u;
        m0 = __builtin_amdgcn_readfirstlane(m0);
        m1 = __builtin_amdgcn_readfirstlane(m1);
        if ((m0 | m1) == 0u) {                                            // (wave-uniform) nothing of the pair is read
            if (lane == 0) {
#pragma unroll
                for (int d = 0; d <= CRH_FUZZY_MAX_EDITS; ++d) {
                    if (d > k) break;
                    a.out[d * ntiles + t0] = 0u;
                    if (second) a.out[d * ntiles + t0 + 1] = 0u;
                }
            }
            continue;
        }
        const bool active = (((lane < 32 ? m0 : m1) >> (lane & 31)) & 1u) != 0u;   // (a set bit is a row below `rows`)
        int64_t begin = 0, end = 0;
        if (active) {
            begin = a.row_off[r0 + lane];
            end = a.row_off[r0 + lane + 1];
        }
        int64_t p = begin < end ? begin & ~(int64_t)(kTextLane - 1) : end;
        W pv = ~(W)0, mv = 0;
        int score = m, best = m;                                          // (D[m][0] = m: the empty row's distance)
        text_u32x4 cur = p < end ? *reinterpret_cast<const text_u32x4 *>(a.bytes + p) : text_u32x4{0u, 0u, 0u, 0u};
        while (__ballot(p < end && best != 0) != 0ull) {
            const int64_t pn = p + kTextLane;
            // (unconditional, so that nothing waits for it before the walk: a lane without a next chunk reloads the arena's first)
            const text_u32x4 nxt = *reinterpret_cast<const text_u32x4 *>(a.bytes + (pn < end ? pn : 0));
            // the lane's bytes of this chunk that lie inside its row: [lo, hi) of 0..16 (none once p >= end)
            const int64_t dlo = begin - p, dhi = end - p;
            const int lo = dlo > 0 ? (int)dlo : 0;
            const int hi = dhi >= kTextLane ? kTextLane : dhi > 0 ? (int)dhi : 0;
            W eq[kTextLane];
            fuzzy_eqs<W, 0>(cur, peq, eq);                                // (independent of the state: off the chain)
#pragma unroll
            for (int j = 0; j < kTextLane; ++j) {
                const bool in = j >= lo && j < hi;
                const W e = eq[j];
                const W xv = e | mv;
                const W xh = (((e & pv) + pv) ^ pv) | e;
                W ph = mv | ~(xh | pv);
                W mh = pv & xh;
                const int ns = score + ((ph & top) != 0 ? 1 : 0) - ((mh & top) != 0 ? 1 : 0);
                ph <<= 1;                                                 // (no carry in: D[0][j] - D[0][j-1] = 0, a match may start anywhere)
                mh <<= 1;
                const W npv = mh | ~(xv | ph), nmv = ph & xv;
                pv = in ? npv : pv;
                mv = in ? nmv : mv;
                score = in ? ns : score;
                best = min(best, score);
            }
            p = pn;
            cur = nxt;
        }
#pragma unroll
        for (int d = 0; d <= CRH_FUZZY_MAX_EDITS; ++d) {
            if (d > k) break;
            const unsigned long long hit = __ballot(active && best <= d);
            const uint32_t w0 = (uint32_t)hit & m0, w1 = (uint32_t)(hit >> 32) & m1;
            if (lane == 0) {
                a.out[d * ntiles + t0] = w0;
                if (second) a.out[d * ntiles + t0 + 1] = w1;
            }
            found[d] += (unsigned int)(__popc(w0) + __popc(w1));
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int d = 0; d <= CRH_FUZZY_MAX_EDITS; ++d)
            if (d <= k && found[d]) atomicAdd(a.count + d, (unsigned long long)found[d]);
    }
}

int text_alloc(void **p, int64_t bytes)
{
    hipError_t e = hipMalloc(p, (size_t)std::max<int64_t>(bytes, 1));
    if (e != hipSuccess) return fail(CRH_E_CAPACITY, "hipMalloc of %lld bytes failed: %s", (long long)bytes, hipGetErrorString(e));
    return CRH_OK;
}

// capacity for `need` bytes (+ `slack` zeroed ones behind) of which the first `used` are kept: doubling, the new buffer zeroed
// whole, the old one copied and released
int text_grow(uint8_t **p, int64_t *cap, int64_t used, int64_t need, int64_t slack)
{
    if (*p && need <= *cap) return CRH_OK;
    int64_t c = std::max<int64_t>(*cap, 4096);
    while (c < need) c *= 2;
    void *np = nullptr;
    CRH_TRY(text_alloc(&np, c + slack));
    CRH_HIP(hipMemset(np, 0, (size_t)(c + slack)));
    if (used > 0) CRH_HIP(hipMemcpy(np, *p, (size_t)used, hipMemcpyDeviceToDevice));
    if (*p) CRH_HIP(hipFree(*p));
    *p = static_cast<uint8_t *>(np);
    *cap = c;
    return CRH_OK;
}

template <int NP>
void text_launch(const TextArgs &a, bool fold, unsigned blocks, hipStream_t st)
{
    if (fold) hipLaunchKernelGGL((k_text_match<NP, true>), dim3(blocks), dim3(kTextWaves * 64), 0, st, a);
    else hipLaunchKernelGGL((k_text_match<NP, false>), dim3(blocks), dim3(kTextWaves * 64), 0, st, a);
}

}  // namespace
}  // namespace crh

struct crh_text {
    int device = 0;
    int64_t rows = 0, nbytes = 0;
    int64_t cap_off = 0, cap_bytes = 0;   // in bytes: of row_off (8 per entry), of bytes (without the slack)
    uint8_t *row_off = nullptr;           // int64 [rows + 1]
    uint8_t *bytes = nullptr;             // nbytes, then kTextSlack zeros
    unsigned long long *count = nullptr;  // CRH_FUZZY_MAX_EDITS + 1 counters: the match's / the regex's is the first, the fuzzy match's one per level
    uint8_t *regex_image = nullptr;       // kRegexImageMax bytes, allocated by the first crh_text_regex
    std::vector<uint8_t> regex_host;      // the image the last crh_text_regex uploaded (the copy's source outlives the call)
};

using namespace crh;

extern "C" {

int crh_text_create(int device, int64_t capacity_rows, int64_t capacity_bytes, crh_text **out)
{
    if (!out) return fail(CRH_E_INVALID, "out is NULL");
    *out = nullptr;
    if (capacity_rows < 0 || capacity_rows >= (1LL << 31)) return fail(CRH_E_INVALID, "capacity_rows=%lld outside 0..2^31-1", (long long)capacity_rows);
    if (capacity_bytes < 0) return fail(CRH_E_INVALID, "capacity_bytes=%lld is negative", (long long)capacity_bytes);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(CRH_E_NODEVICE, "no usable device %d", device);
    DeviceGuard g(device);
    if (!g.ok) return fail(CRH_E_NODEVICE, "hipSetDevice(%d) failed", device);
    crh_text *t = new crh_text();
    t->device = device;
    void *cnt = nullptr;
    int rc = text_grow(&t->row_off, &t->cap_off, 0, (capacity_rows + 1) * 8, 0);   // (zeroed: row_off[0] = 0)
    if (rc == CRH_OK) rc = text_grow(&t->bytes, &t->cap_bytes, 0, capacity_bytes, kTextSlack);
    if (rc == CRH_OK) rc = text_alloc(&cnt, 8 * (CRH_FUZZY_MAX_EDITS + 1));
    t->count = static_cast<unsigned long long *>(cnt);
    if (rc != CRH_OK) {
        crh_text_destroy(t);
        return rc;
    }
    *out = t;
    return CRH_OK;
}

int crh_text_destroy(crh_text *t)
{
    if (!t) return CRH_OK;
    DeviceGuard g(t->device);
    (void)hipDeviceSynchronize();
    void *bufs[] = {t->row_off, t->bytes, t->count, t->regex_image};
    for (void *p : bufs)
        if (p) (void)hipFree(p);
    delete t;
    return CRH_OK;
}

int crh_text_clear(crh_text *t)
{
    if (!t) return fail(CRH_E_INVALID, "text handle is NULL");
    t->rows = 0;
    t->nbytes = 0;
    return CRH_OK;
}

int crh_text_count(crh_text *t, int64_t *rows_out, int64_t *bytes_out)
{
    if (!t) return fail(CRH_E_INVALID, "text handle is NULL");
    if (rows_out) *rows_out = t->rows;
    if (bytes_out) *bytes_out = t->nbytes;
    return CRH_OK;
}

int crh_text_append(crh_text *t, int64_t n, const int64_t *row_off_host, const uint8_t *bytes_host)
{
    if (!t) return fail(CRH_E_INVALID, "text handle is NULL");
    if (n < 0) return fail(CRH_E_INVALID, "n=%lld is negative", (long long)n);
    if (n == 0) return CRH_OK;
    if (!row_off_host) return fail(CRH_E_INVALID, "NULL pointer");
    if (row_off_host[0] != 0) return fail(CRH_E_INVALID, "text_append: row_off[0]=%lld, not 0", (long long)row_off_host[0]);
    for (int64_t i = 0; i < n; ++i)
        if (row_off_host[i + 1] < row_off_host[i]) return fail(CRH_E_INVALID, "text_append: row_off decreases at row %lld", (long long)i);
    const int64_t nb = row_off_host[n];
    if (nb > 0 && !bytes_host) return fail(CRH_E_INVALID, "NULL pointer");
    if (t->rows + n >= (1LL << 31)) return fail(CRH_E_CAPACITY, "text_append: more than 2^31-1 rows");
    DeviceGuard g(t->device);
    CRH_HIP(hipDeviceSynchronize());   // (matches in flight on other streams read the buffers a growth releases)
    CRH_TRY(text_grow(&t->row_off, &t->cap_off, (t->rows + 1) * 8, (t->rows + n + 1) * 8, 0));
    CRH_TRY(text_grow(&t->bytes, &t->cap_bytes, t->nbytes, t->nbytes + nb, kTextSlack));
    std::vector<int64_t> off((size_t)n);
    for (int64_t i = 0; i < n; ++i) off[(size_t)i] = t->nbytes + row_off_host[i + 1];
    const int64_t zero = 0;
    if (t->rows == 0) CRH_HIP(hipMemcpy(t->row_off, &zero, 8, hipMemcpyHostToDevice));
    CRH_HIP(hipMemcpy(t->row_off + (t->rows + 1) * 8, off.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    if (nb > 0) CRH_HIP(hipMemcpy(t->bytes + t->nbytes, bytes_host, (size_t)nb, hipMemcpyHostToDevice));
    CRH_HIP(hipMemset(t->bytes + t->nbytes + nb, 0, (size_t)kTextSlack));   // (a cleared arena still holds its old bytes here)
    t->rows += n;
    t->nbytes += nb;
    return CRH_OK;
}

int crh_text_match(crh_text *t, int n_pat, const int64_t *pat_off_host, const uint8_t *pat_bytes_host, int fold_case, int combine,
                   const uint32_t *mask_dev, uint32_t *out_words_dev, int64_t *out_count_host, void *stream)
{
    if (!t) return fail(CRH_E_INVALID, "text handle is NULL");
    if (out_count_host) *out_count_host = 0;
    if (n_pat < 1 || n_pat > CRH_TEXT_MAX_PATTERNS) return fail(CRH_E_INVALID, "text_match: n_pat=%d outside 1..%d", n_pat, CRH_TEXT_MAX_PATTERNS);
    if (!pat_off_host || !pat_bytes_host) return fail(CRH_E_INVALID, "text_match: NULL pointer");
    if (combine != CRH_TEXT_ALL && combine != CRH_TEXT_ANY) return fail(CRH_E_INVALID, "text_match: combine=%d is neither CRH_TEXT_ALL nor CRH_TEXT_ANY", combine);
    if (pat_off_host[0] != 0) return fail(CRH_E_INVALID, "text_match: pat_off[0]=%lld, not 0", (long long)pat_off_host[0]);
    for (int p = 0; p < n_pat; ++p) {
        const int64_t len = pat_off_host[p + 1] - pat_off_host[p];
        if (len < 1 || len > CRH_TEXT_MAX_PATTERN_BYTES)
            return fail(CRH_E_INVALID, "text_match: pattern %d has %lld bytes (1..%d)", p, (long long)len, CRH_TEXT_MAX_PATTERN_BYTES);
    }
    if (t->rows == 0) return CRH_OK;
    if (!out_words_dev) return fail(CRH_E_INVALID, "text_match: out_words_dev is NULL");
    TextArgs a{};
    a.row_off = reinterpret_cast<const int64_t *>(t->row_off);
    a.bytes = t->bytes;
    a.rows = t->rows;
    a.mask = mask_dev;
    a.out = out_words_dev;
    a.count = t->count;
    a.combine = combine;
    int np = 1;
    while (np < n_pat) np *= 2;
    uint8_t *pb = reinterpret_cast<uint8_t *>(a.pat);
    for (int p = 0; p < np; ++p) {
        const int src = p < n_pat ? p : 0;                                // (padding repeats pattern 0: ALL and ANY are idempotent)
        const int64_t o = pat_off_host[src];
        const int len = (int)(pat_off_host[src + 1] - o);
        a.len[p] = len;
        for (int i = 0; i < len; ++i) {
            uint8_t c = pat_bytes_host[o + i];
            if (fold_case && c >= 'A' && c <= 'Z') c = (uint8_t)(c | 0x20);
            pb[p * CRH_TEXT_MAX_PATTERN_BYTES + i] = c;
        }
        uint32_t fw = 0;
        std::memcpy(&fw, pb + p * CRH_TEXT_MAX_PATTERN_BYTES, (size_t)std::min(len, 4));   // (gfx950 hosts are little endian, as the device)
        a.fw[p] = fw;
        a.fm[p] = len >= 4 ? 0xffffffffu : (1u << (8 * len)) - 1u;
    }
    DeviceGuard g(t->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    CRH_HIP(hipMemsetAsync(t->count, 0, 8, st));
    const int64_t ntiles = ceil_div(t->rows, 32);
    const unsigned blocks = (unsigned)std::min<int64_t>(ceil_div(ntiles, kTextWaves), (int64_t)current_device_cus() * 8);
    const bool fold = fold_case != 0;
    switch (np) {
    case 1: text_launch<1>(a, fold, blocks, st); break;
    case 2: text_launch<2>(a, fold, blocks, st); break;
    case 4: text_launch<4>(a, fold, blocks, st); break;
    default: text_launch<8>(a, fold, blocks, st); break;
    }
    CRH_HIP(hipGetLastError());
    if (out_count_host) {
        unsigned long long c = 0ull;
        CRH_HIP(hipMemcpyAsync(&c, t->count, 8, hipMemcpyDeviceToHost, st));
        CRH_HIP(hipStreamSynchronize(st));
        *out_count_host = (int64_t)c;
    }
    return CRH_OK;
}

int crh_text_regex(crh_text *t, int n_states, int n_classes, const uint8_t *class_of_host, int end_class, const uint8_t *trans_host,
                   int accept_state, const uint32_t *mask_dev, uint32_t *out_words_dev, int64_t *out_count_host, void *stream)
{
    if (!t) return fail(CRH_E_INVALID, "text handle is NULL");
    if (out_count_host) *out_count_host = 0;
    if (n_states < 1 || n_states > CRH_REGEX_MAX_STATES) return fail(CRH_E_INVALID, "text_regex: n_states=%d outside 1..%d", n_states, CRH_REGEX_MAX_STATES);
    if (n_classes < 2 || n_classes > 257) return fail(CRH_E_INVALID, "text_regex: n_classes=%d outside 2..257", n_classes);
    if ((int64_t)n_states * n_classes > CRH_REGEX_MAX_TABLE_BYTES)
        return fail(CRH_E_INVALID, "text_regex: a table of %d x %d bytes (at most %d)", n_states, n_classes, CRH_REGEX_MAX_TABLE_BYTES);
    if (!class_of_host || !trans_host) return fail(CRH_E_INVALID, "text_regex: NULL pointer");
    if (end_class < 0 || end_class >= n_classes) return fail(CRH_E_INVALID, "text_regex: end_class=%d outside 0..%d", end_class, n_classes - 1);
    if (accept_state < 0 || accept_state >= n_states) return fail(CRH_E_INVALID, "text_regex: accept_state=%d outside 0..%d", accept_state, n_states - 1);
    for (int b = 0; b < 256; ++b)
        if (class_of_host[b] >= n_classes) return fail(CRH_E_INVALID, "text_regex: class_of[%d]=%d is no class (%d classes)", b, (int)class_of_host[b], n_classes);
    for (int i = 0; i < n_states * n_classes; ++i)
        if (trans_host[i] >= n_states)
            return fail(CRH_E_INVALID, "text_regex: trans[%d][%d]=%d is no state (%d states)", i / n_classes, i % n_classes, (int)trans_host[i], n_states);
    for (int c = 0; c < n_classes; ++c)
        if (trans_host[accept_state * n_classes + c] != accept_state)
            return fail(CRH_E_INVALID, "text_regex: the accept state %d is not absorbing (class %d leaves it)", accept_state, c);
    if (t->rows == 0) return CRH_OK;
    if (!out_words_dev) return fail(CRH_E_INVALID, "text_regex: out_words_dev is NULL");
    DeviceGuard g(t->device);
    if (!t->regex_image) {
        void *img = nullptr;
        CRH_TRY(text_alloc(&img, kRegexImageMax));
        t->regex_image = static_cast<uint8_t *>(img);
    }
    // the image the kernel copies to LDS: the class map, then the table with the SKIP column (a state's entry: itself) behind
    // the caller's columns, padded with zeros to whole 16 bytes
    const int ncols = n_classes + 1;
    const size_t image_bytes = ((size_t)kRegexClassMap + (size_t)n_states * ncols + 15) / 16 * 16;
    t->regex_host.assign(image_bytes, 0);
    std::memcpy(t->regex_host.data(), class_of_host, 256);
    for (int s = 0; s < n_states; ++s) {
        uint8_t *row = t->regex_host.data() + kRegexClassMap + (size_t)s * ncols;
        std::memcpy(row, trans_host + (size_t)s * n_classes, (size_t)n_classes);
        row[n_classes] = (uint8_t)s;
    }
    RegexArgs a{};
    a.row_off = reinterpret_cast<const int64_t *>(t->row_off);
    a.bytes = t->bytes;
    a.rows = t->rows;
    a.mask = mask_dev;
    a.out = out_words_dev;
    a.count = t->count;
    a.image = reinterpret_cast<const uint32_t *>(t->regex_image);
    a.image_words = (int)(image_bytes / 4);
    a.ncols = ncols;
    a.end_class = end_class;
    a.accept = accept_state;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // (regex_host is pageable: HIP has read it when this call returns, which is what lets the NEXT call on this handle rewrite it
    // while this one is only enqueued -- without out_count_host nothing else here waits)
    CRH_HIP(hipMemcpyAsync(t->regex_image, t->regex_host.data(), image_bytes, hipMemcpyHostToDevice, st));
    CRH_HIP(hipMemsetAsync(t->count, 0, 8, st));
    const int64_t npairs = ceil_div(ceil_div(t->rows, 32), 2);
    const unsigned blocks = (unsigned)std::min<int64_t>(ceil_div(npairs, kTextWaves), (int64_t)current_device_cus() * 8);
    hipLaunchKernelGGL(k_text_regex, dim3(blocks), dim3(kTextWaves * 64), image_bytes, st, a);
    CRH_HIP(hipGetLastError());
    if (out_count_host) {
        unsigned long long c = 0ull;
        CRH_HIP(hipMemcpyAsync(&c, t->count, 8, hipMemcpyDeviceToHost, st));
        CRH_HIP(hipStreamSynchronize(st));
        *out_count_host = (int64_t)c;
    }
    return CRH_OK;
}

int crh_text_fuzzy(crh_text *t, const uint8_t *pat_host, int len, int max_edits, int fold_case, const uint32_t *mask_dev,
                   uint32_t *out_words_dev, int64_t *out_counts_host, void *stream)
{
    // (the arguments first, the handle after them: a caller's mistake is named whatever it passes as the handle)
    if (len < 1 || len > CRH_TEXT_MAX_PATTERN_BYTES) return fail(CRH_E_INVALID, "text_fuzzy: len=%d outside 1..%d", len, CRH_TEXT_MAX_PATTERN_BYTES);
    if (max_edits < 0 || max_edits > CRH_FUZZY_MAX_EDITS) return fail(CRH_E_INVALID, "text_fuzzy: max_edits=%d outside 0..%d", max_edits, CRH_FUZZY_MAX_EDITS);
    if (len <= max_edits) return fail(CRH_E_INVALID, "text_fuzzy: len=%d is not above max_edits=%d (every row would match)", len, max_edits);
    if (!pat_host) return fail(CRH_E_INVALID, "text_fuzzy: pat_host is NULL");
    if (!t) return fail(CRH_E_INVALID, "text_fuzzy: the text handle is NULL");
    if (out_counts_host) std::fill(out_counts_host, out_counts_host + max_edits + 1, (int64_t)0);
    if (t->rows == 0) return CRH_OK;   // (before the output is looked at, as in crh_text_match / crh_text_regex: a buffer of 0 words may be NULL)
    if (!out_words_dev) return fail(CRH_E_INVALID, "text_fuzzy: out_words_dev is NULL");
    FuzzyArgs a{};
    a.row_off = reinterpret_cast<const int64_t *>(t->row_off);
    a.bytes = t->bytes;
    a.rows = t->rows;
    a.mask = mask_dev;
    a.out = out_words_dev;
    a.count = t->count;
    a.m = len;
    a.k = max_edits;
    a.fold = fold_case != 0;
    uint8_t *pb = reinterpret_cast<uint8_t *>(a.pat);
    for (int i = 0; i < len; ++i) {
        uint8_t c = pat_host[i];
        if (fold_case && c >= 'A' && c <= 'Z') c = (uint8_t)(c | 0x20);
        pb[i] = c;
    }
    DeviceGuard g(t->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    CRH_HIP(hipMemsetAsync(t->count, 0, 8 * (size_t)(max_edits + 1), st));
    const int64_t npairs = ceil_div(ceil_div(t->rows, 32), 2);
    const unsigned blocks = (unsigned)std::min<int64_t>(ceil_div(npairs, kTextWaves), (int64_t)current_device_cus() * 8);
    if (len <= 32) hipLaunchKernelGGL(k_text_fuzzy<uint32_t>, dim3(blocks), dim3(kTextWaves * 64), 0, st, a);
    else hipLaunchKernelGGL(k_text_fuzzy<unsigned long long>, dim3(blocks), dim3(kTextWaves * 64), 0, st, a);
    CRH_HIP(hipGetLastError());
    if (out_counts_host) {
        unsigned long long c[CRH_FUZZY_MAX_EDITS + 1] = {0ull, 0ull, 0ull, 0ull};
        CRH_HIP(hipMemcpyAsync(c, t->count, 8 * (size_t)(max_edits + 1), hipMemcpyDeviceToHost, st));
        CRH_HIP(hipStreamSynchronize(st));
        for (int d = 0; d <= max_edits; ++d) out_counts_host[d] = (int64_t)c[d];
    }
    return CRH_OK;
}

}  // extern "C"
