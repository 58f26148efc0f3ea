// lexbag.h -- host-only bag code of the lexical index (lexbag.cpp): the checks of a batch of term bags as they arrive through
// the C ABI and the canonical form of one bag.  Plain C++ (no HIP header), so it also builds with g++ under the sanitizers
// (make lexbag_asan).
#pragma once

#include <stdint.h>

#include <vector>

namespace sqe {

constexpr int LEX_MAX_TERMS = 131072;      // n_terms limit of sqe_lex_create
constexpr int LEX_MAX_QUERY = 64;          // term occurrences of one query
constexpr int LEX_TF_CAP = 65535;          // tf(t, d) is capped here; dl(d) is not

// offsets [n + 1] must start at 0 and not decrease; every term of terms[0 .. offsets[n]) must lie in [0, n_terms).  max_len > 0
// also bounds the length of each bag (queries).  Returns null when the batch is well formed, else a static text that names the
// fault; reads nothing past a fault (terms is not touched when the offsets are malformed).
const char* lexbag_check(const int64_t* offsets, int64_t n, const int32_t* terms, int n_terms, int64_t max_len);

// ids [n] must be >= 0 and distinct.  Returns null or a static text.
const char* lexbag_check_ids(const int64_t* ids, int64_t n);

// The canonical form of one bag: its distinct terms ascending, tf of each (capped at LEX_TF_CAP); returns dl = len.
int64_t lexbag_canon(const int32_t* terms, int64_t len, std::vector<int32_t>& terms_out, std::vector<uint16_t>& tf_out);

}  // namespace sqe
