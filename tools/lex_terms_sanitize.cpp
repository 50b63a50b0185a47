// Stand-alone driver of code-rag_amd/csrc_host/lex_terms.cpp for a sanitizer run on the host (no Python, no GPU):
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/lex_terms_sanitize.cpp code-rag_amd/csrc_host/lex_terms.cpp -o lex_terms_sanitize && ./lex_terms_sanitize
// Cuts the awkward strings of tests/test_lexical_host.py and a 1 MB text on 1 and 7 threads and checks the CSR it gets back.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

extern "C" {
void *crl_terms_batch(int64_t n, const char *const *texts, const int64_t *lens, int threads);
int64_t crl_terms_entries(const void *res);
void crl_terms_copy(const void *res, int64_t *row_off, uint32_t *terms, uint8_t *tf, int32_t *dl);
void crl_terms_free(void *res);
}

int main()
{
    std::vector<std::string> texts = {"", "!!! ... ;; --", "_", "__init__", "a_b", "getHTTPResponseCode2xx", "SHA256_digest", "HTTPServer",
                                      std::string(35, 'x') + std::string(35, 'Y'), std::string(70, 'q'), "",
                                      "gr\xc3\xb6\xc3\x9f" "e\xc3\x84nderung_na\xc3\xafveCaf\xc3\xa9 \xe5\xa4\x89\xe6\x95\xb0_9x",
                                      "a\xed\xb2\x80" "b foo\xed\xb2\x80" "Bar", "line_one\r\nlineTwo\r\n\r\nline3", "trailing_", "_", "Z", ""};
    for (int i = 0; i < 300; ++i) texts[10] += "word ";
    std::string big;
    while (big.size() < (1u << 20)) big += "def parse_retry_after(resp): return min(MAX_BACKOFF_MS, int(resp.headers['Retry-After']))  # HTTPServerError\n";
    big.resize(1u << 20);
    texts.push_back(big);
    std::vector<const char *> ptrs;
    std::vector<int64_t> lens;
    for (const std::string &t : texts) {
        ptrs.push_back(t.empty() ? nullptr : t.data());
        lens.push_back((int64_t)t.size());
    }
    int64_t first_entries = -1;
    for (int threads : {1, 7}) {
        void *res = crl_terms_batch((int64_t)texts.size(), ptrs.data(), lens.data(), threads);
        const int64_t ne = crl_terms_entries(res);
        std::vector<int64_t> off(texts.size() + 1);
        std::vector<uint32_t> terms((size_t)ne);
        std::vector<uint8_t> tf((size_t)ne);
        std::vector<int32_t> dl(texts.size());
        crl_terms_copy(res, off.data(), terms.data(), tf.data(), dl.data());
        crl_terms_free(res);
        if (off.back() != ne || dl[10] != 300 || off[11] - off[10] != 1 || tf[(size_t)off[10]] != 255 || dl[9] != 0 || dl[8] != 2) {
            std::printf("unexpected result on %d threads\n", threads);
            return 1;
        }
        for (size_t r = 0; r < texts.size(); ++r) {
            int64_t sum = 0;
            for (int64_t e = off[r]; e < off[r + 1]; ++e) {
                if ((e > off[r] && terms[(size_t)e] <= terms[(size_t)e - 1]) || tf[(size_t)e] == 0) return 2;
                sum += tf[(size_t)e];
            }
            if (dl[r] < sum) return 3;
        }
        if (first_entries >= 0 && first_entries != ne) return 4;
        first_entries = ne;
    }
    void *none = crl_terms_batch(0, nullptr, nullptr, 3);
    if (crl_terms_entries(none) != 0) return 5;
    crl_terms_free(none);
    std::printf("lex_terms: %lld entries from %zu texts, clean\n", (long long)first_entries, texts.size());
    return 0;
}
