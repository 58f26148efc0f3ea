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

// An ordered document (sqe_lex_put_ordered): the canonical bag of the sequence terms[0 .. len) as lexbag_canon makes it, and the
// sequence itself appended to seq_log.  Returns where in seq_log it starts; dl = len.
int64_t lexseq_append(const int32_t* terms, int64_t len, std::vector<int32_t>& terms_out, std::vector<uint16_t>& tf_out,
                      std::vector<int32_t>& seq_log);

// The tables of B clause queries (sqe_lex_search_phrase): query b owns the clauses qoffsets[b] .. qoffsets[b + 1], clause c the
// occurrences terms[coffsets[c] .. coffsets[c + 1]).  Both tables start at 0; qoffsets does not decrease, coffsets increases (no
// empty clause); a query holds at most max_len occurrences; every term lies in [0, n_terms).  Returns null or a static text;
// coffsets is read only once qoffsets is well formed, terms only once coffsets is.
const char* lexclause_check(const int64_t* qoffsets, int64_t B, const int64_t* coffsets, const int32_t* terms, int n_terms, int64_t max_len);

}  // namespace sqe
