// crh_text.hip -- literal substring match over the chunks' text in HBM (gfx950 / CDNA4 only).
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
    unsigned long long *count = nullptr;  // the match's counter
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
    if (rc == CRH_OK) rc = text_alloc(&cnt, 8);
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
    void *bufs[] = {t->row_off, t->bytes, t->count};
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

}  // extern "C"
