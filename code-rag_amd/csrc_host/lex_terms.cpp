// lex_terms.cpp -- the term cutter of the keyword index (plain C++, no GPU code; part of lib/libcoderag_tok.so).
//
// The definition is this repository's own; tests/lex_cases.py restates it in Python and is its checker.
//   word      a maximal run of bytes that are ASCII letters, ASCII digits, '_' or >= 0x80 (those count as lower-case letters
//             and are never folded)
//   sub-words the word split at every '_' (empty pieces vanish), each piece split further at lower->upper (getUser), at
//             letter<->digit (sha256) and inside an upper-case run before its last capital when a lower-case letter follows
//             (HTTPServer -> HTTP, Server); ASCII-lower-cased
//   emitted   every sub-word; the whole word as well (lower-cased, underscores kept) when it gave more than one sub-word; a term
//             shorter than 2 or longer than 64 bytes is dropped.  No stop words, no stemming.
//   term id   32-bit FNV-1a of the term's bytes
//   per text  the distinct ids ascending, tf = occurrences saturated at 255, dl = emitted terms before de-duplication
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

namespace {

constexpr size_t kMinTerm = 2, kMaxTerm = 64;

inline bool is_upper(unsigned char c) { return c >= 'A' && c <= 'Z'; }
inline bool is_digit(unsigned char c) { return c >= '0' && c <= '9'; }
inline bool is_word(unsigned char c) { return c >= 0x80 || c == '_' || is_digit(c) || is_upper(c) || (c >= 'a' && c <= 'z'); }
inline int cls(unsigned char c) { return is_digit(c) ? 0 : is_upper(c) ? 1 : 2; }   // digit, upper, lower (and >= 0x80)

// FNV-1a of s[0..n) lower-cased (ASCII)
inline void emit(const unsigned char *s, size_t n, std::vector<uint32_t> &ids)
{
    if (n < kMinTerm || n > kMaxTerm) return;
    uint32_t h = 2166136261u;
    for (size_t i = 0; i < n; ++i) {
        const unsigned char c = is_upper(s[i]) ? (unsigned char)(s[i] + 32) : s[i];
        h = (h ^ c) * 16777619u;
    }
    ids.push_back(h);
}

struct Row {
    std::vector<uint32_t> ids;   // distinct, ascending
    std::vector<uint8_t> tf;
    int32_t dl = 0;
};

void cut(const unsigned char *d, size_t n, std::vector<uint32_t> &ids, Row &out)
{
    ids.clear();
    size_t i = 0;
    while (i < n) {
        if (!is_word(d[i])) {
            ++i;
            continue;
        }
        size_t j = i;
        while (j < n && is_word(d[j])) ++j;
        size_t subs = 0;
        for (size_t p = i; p < j;) {            // the pieces between underscores
            if (d[p] == '_') {
                ++p;
                continue;
            }
            size_t e = p;
            while (e < j && d[e] != '_') ++e;
            size_t start = p;
            for (size_t x = p + 1; x < e; ++x) {
                const int a = cls(d[x - 1]), b = cls(d[x]);
                bool cutb = (a == 2 && b == 1) || ((a == 0) != (b == 0));
                if (!cutb && a == 1 && b == 1 && x + 1 < e && cls(d[x + 1]) == 2) cutb = true;
                if (cutb) {
                    emit(d + start, x - start, ids);
                    ++subs;
                    start = x;
                }
            }
            emit(d + start, e - start, ids);
            ++subs;
            p = e;
        }
        if (subs > 1) emit(d + i, j - i, ids);
        i = j;
    }
    out.dl = (int32_t)std::min<size_t>(ids.size(), 0x7fffffffu);
    std::sort(ids.begin(), ids.end());
    out.ids.clear();
    out.tf.clear();
    for (size_t a = 0; a < ids.size();) {
        size_t b = a;
        while (b < ids.size() && ids[b] == ids[a]) ++b;
        out.ids.push_back(ids[a]);
        out.tf.push_back((uint8_t)std::min<size_t>(b - a, 255));
        a = b;
    }
}

struct Result {
    std::vector<Row> rows;
    int64_t entries = 0;
};

}  // namespace

extern "C" {

// Cut n texts (texts[i], lens[i] bytes; a NULL text is empty) on `threads` threads (<= 0: the machine's, at most 16).  Returns a
// result to read with crl_terms_entries / crl_terms_copy and to release with crl_terms_free.
void *crl_terms_batch(int64_t n, const char *const *texts, const int64_t *lens, int threads)
{
    Result *r = new Result();
    r->rows.resize((size_t)std::max<int64_t>(n, 0));
    if (n > 0) {
        int nt = threads > 0 ? threads : (int)std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency()));
        nt = (int)std::min<int64_t>(nt, n);
        std::atomic<int64_t> next(0);
        auto run = [&]() {
            std::vector<uint32_t> ids;
            for (;;) {
                const int64_t i = next.fetch_add(1);
                if (i >= n) break;
                const size_t len = texts[i] && lens[i] > 0 ? (size_t)lens[i] : 0;
                cut(reinterpret_cast<const unsigned char *>(texts[i]), len, ids, r->rows[(size_t)i]);
            }
        };
        if (nt <= 1) {
            run();
        } else {
            std::vector<std::thread> pool;
            for (int k = 0; k < nt; ++k) pool.emplace_back(run);
            for (auto &th : pool) th.join();
        }
    }
    for (const Row &row : r->rows) r->entries += (int64_t)row.ids.size();
    return r;
}

int64_t crl_terms_entries(const void *res) { return static_cast<const Result *>(res)->entries; }

// CSR of the result: row_off int64 [n + 1], terms u32 / tf u8 [entries], dl int32 [n]
void crl_terms_copy(const void *res, int64_t *row_off, uint32_t *terms, uint8_t *tf, int32_t *dl)
{
    const Result *r = static_cast<const Result *>(res);
    int64_t at = 0;
    row_off[0] = 0;
    for (size_t i = 0; i < r->rows.size(); ++i) {
        const Row &row = r->rows[i];
        if (!row.ids.empty()) {
            std::memcpy(terms + at, row.ids.data(), row.ids.size() * 4);
            std::memcpy(tf + at, row.tf.data(), row.tf.size());
        }
        at += (int64_t)row.ids.size();
        row_off[i + 1] = at;
        dl[i] = row.dl;
    }
}

void crl_terms_free(void *res) { delete static_cast<Result *>(res); }

}  // extern "C"
