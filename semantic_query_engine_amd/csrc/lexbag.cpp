// lexbag.cpp -- host-only bag code of the lexical index (include/sqe.h: sqe_lex_put, sqe_lex_search): what arrives through the
// ABI is checked here before anything reads it, and a document's bag is brought into its canonical form (distinct terms
// ascending, capped tf, dl); the same for an ordered document's sequence and for the clause tables of a phrase query (make
// lexseq_asan, tests/native/lexseq_sanitize_driver.cpp).  No HIP: builds with plain g++ (make lexbag_asan, tests/native/lexbag_sanitize_driver.cpp).
#include "lexbag.h"

#include <algorithm>

namespace sqe {

const char* lexbag_check(const int64_t* offsets, int64_t n, const int32_t* terms, int n_terms, int64_t max_len) {
    if (n < 0) return "negative count";
    if (!offsets) return "null offsets";
    if (offsets[0] != 0) return "offsets must start at 0";
    for (int64_t i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i]) return "offsets must not decrease";
        if (max_len > 0 && offsets[i + 1] - offsets[i] > max_len) return "more than 64 term occurrences in a query";
    }
    const int64_t total = offsets[n];
    if (total > 0 && !terms) return "null terms";
    for (int64_t p = 0; p < total; ++p)
        if (terms[p] < 0 || terms[p] >= n_terms) return "term out of range";
    return nullptr;
}

const char* lexbag_check_ids(const int64_t* ids, int64_t n) {
    if (n < 0) return "negative count";
    if (n > 0 && !ids) return "null ids";
    for (int64_t i = 0; i < n; ++i)
        if (ids[i] < 0) return "negative id";
    std::vector<int64_t> s(ids, ids + n);
    std::sort(s.begin(), s.end());
    if (std::adjacent_find(s.begin(), s.end()) != s.end()) return "duplicate id";
    return nullptr;
}

int64_t lexbag_canon(const int32_t* terms, int64_t len, std::vector<int32_t>& terms_out, std::vector<uint16_t>& tf_out) {
    terms_out.clear();
    tf_out.clear();
    if (len <= 0) return 0;
    std::vector<int32_t> s(terms, terms + len);
    std::sort(s.begin(), s.end());
    for (int64_t i = 0; i < len;) {
        int64_t j = i + 1;
        while (j < len && s[j] == s[i]) ++j;
        terms_out.push_back(s[i]);
        tf_out.push_back((uint16_t)std::min<int64_t>(j - i, LEX_TF_CAP));
        i = j;
    }
    return len;
}

int64_t lexseq_append(const int32_t* terms, int64_t len, std::vector<int32_t>& terms_out, std::vector<uint16_t>& tf_out,
                      std::vector<int32_t>& seq_log) {
    lexbag_canon(terms, len, terms_out, tf_out);
    const int64_t at = (int64_t)seq_log.size();
    if (len > 0) seq_log.insert(seq_log.end(), terms, terms + len);
    return at;
}

const char* lexclause_check(const int64_t* qoffsets, int64_t B, const int64_t* coffsets, const int32_t* terms, int n_terms, int64_t max_len) {
    if (B < 0) return "negative count";
    if (!qoffsets) return "null offsets";
    if (qoffsets[0] != 0) return "offsets must start at 0";
    for (int64_t b = 0; b < B; ++b)
        if (qoffsets[b + 1] < qoffsets[b]) return "offsets must not decrease";
    const int64_t C = qoffsets[B];
    if (!coffsets) return "null clause offsets";
    if (coffsets[0] != 0) return "clause offsets must start at 0";
    for (int64_t c = 0; c < C; ++c) {
        if (coffsets[c + 1] < coffsets[c]) return "clause offsets must not decrease";
        if (coffsets[c + 1] == coffsets[c]) return "an empty clause";
    }
    for (int64_t b = 0; b < B; ++b)
        if (coffsets[qoffsets[b + 1]] - coffsets[qoffsets[b]] > max_len) return "more than 64 term occurrences in a query";
    const int64_t total = coffsets[C];
    if (total > 0 && !terms) return "null terms";
    for (int64_t p = 0; p < total; ++p)
        if (terms[p] < 0 || terms[p] >= n_terms) return "term out of range";
    return nullptr;
}

}  // namespace sqe
