// Sanitizer driver for the pair form of csrc/tokenizer.cpp, sqe_tokenize_pair_batch (test infrastructure, host-only: built by
// `make -C semantic_query_engine_amd/csrc tokenizer_pair_asan` with g++ -fsanitize=address,undefined, like
// tokenizer_sanitize_driver.cpp for the single-text form).
//
//   tokenizer_pair_asan <vocab file> <cases file> <out file>
// cases file: repeated { int32 max_len; int32 max_a; int64 a_bytes; int64 b_bytes; a; b }.  Every pair is tokenised alone
// and, in groups of 70 at one shape, through the threaded path; the driver checks the ABI's invariants and writes per case
// { len, ids[max_len], types[max_len] }, which the Python test compares with what the shipped libsqe.so returns.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "sqe.h"

namespace sqe {
static std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
}  // namespace sqe

static std::vector<char> slurp(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    std::vector<char> b;
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + n);
    fclose(f);
    return b;
}

#define REQUIRE(c)                                                        \
    do {                                                                  \
        if (!(c)) { fprintf(stderr, "REQUIRE failed: %s (line %d)\n", #c, __LINE__); exit(3); } \
    } while (0)

// an exact-size heap copy: a read one byte past the text is a heap-buffer-overflow ASan reports
static char* exact_copy(const char* src, int64_t n) {
    char* copy = (char*)malloc(n > 0 ? (size_t)n : 1);
    memcpy(copy, src, (size_t)n);
    return copy;
}

// the contract every row keeps, whatever the bytes were
static void check_row(const int32_t* ids, const int32_t* types, int len, int max_len, int max_a, int32_t cls, int32_t sep) {
    REQUIRE(len >= 3 && len <= max_len);
    REQUIRE(ids[0] == cls && ids[len - 1] == sep);
    int first_b = -1;
    for (int j = 1; j < len; ++j)
        if (types[j] == 1) { first_b = j; break; }
    REQUIRE(first_b >= 2 && first_b - 2 <= max_a && ids[first_b - 1] == sep);
    for (int j = 0; j < max_len; ++j) {
        REQUIRE(types[j] == (j >= first_b && j < len ? 1 : 0));
        if (j >= len) REQUIRE(ids[j] == 0);
    }
}

int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: %s vocab cases out\n", argv[0]); return 2; }
    const std::vector<char> vocab = slurp(argv[1]);
    const std::vector<char> cases = slurp(argv[2]);
    sqe_tokenizer* tok = nullptr;
    REQUIRE(sqe_tokenizer_create(vocab.data(), (int64_t)vocab.size(), &tok) == SQE_OK && tok);
    int32_t probe[2];
    int plen = 0;
    REQUIRE(sqe_tokenize(tok, nullptr, 0, 2, probe, &plen) == SQE_OK && plen == 2);
    const int32_t cls = probe[0], sep = probe[1];

    // argument checking of the ABI itself
    {
        const char* t[1] = {"x"};
        const int64_t n1[1] = {1}, neg[1] = {-1};
        const char* null_t[1] = {nullptr};
        int32_t ids[16], types[16], lens[1];
        REQUIRE(sqe_tokenize_pair_batch(tok, t, n1, t, n1, 1, 3, 1, ids, types, lens) == SQE_ERR_INVALID);    // max_len < 4
        REQUIRE(sqe_tokenize_pair_batch(tok, t, n1, t, n1, 1, 16, 0, ids, types, lens) == SQE_ERR_INVALID);   // max_a < 1
        REQUIRE(sqe_tokenize_pair_batch(tok, t, n1, t, n1, 1, 16, 14, ids, types, lens) == SQE_ERR_INVALID);  // max_a > max_len - 3
        REQUIRE(sqe_tokenize_pair_batch(tok, t, n1, t, n1, -1, 16, 4, ids, types, lens) == SQE_ERR_INVALID);
        REQUIRE(sqe_tokenize_pair_batch(nullptr, t, n1, t, n1, 1, 16, 4, ids, types, lens) == SQE_ERR_INVALID);
        REQUIRE(sqe_tokenize_pair_batch(tok, t, n1, t, n1, 1, 16, 4, ids, nullptr, lens) == SQE_ERR_INVALID);
        REQUIRE(sqe_tokenize_pair_batch(tok, t, neg, t, n1, 1, 16, 4, ids, types, lens) == SQE_ERR_INVALID);
        REQUIRE(sqe_tokenize_pair_batch(tok, t, n1, null_t, n1, 1, 16, 4, ids, types, lens) == SQE_ERR_INVALID);
        REQUIRE(sqe_tokenize_pair_batch(tok, nullptr, nullptr, nullptr, nullptr, 0, 16, 4, nullptr, nullptr, nullptr) == SQE_OK);
        const int64_t zero[1] = {0};
        REQUIRE(sqe_tokenize_pair_batch(tok, null_t, zero, null_t, zero, 1, 4, 1, ids, types, lens) == SQE_OK && lens[0] == 3);
    }

    FILE* out = fopen(argv[3], "wb");
    REQUIRE(out);
    std::vector<const char*> as, bs;
    std::vector<int64_t> an, bn;
    size_t pos = 0;
    while (pos + 24 <= cases.size()) {
        int32_t max_len, max_a;
        int64_t na, nb;
        memcpy(&max_len, cases.data() + pos, 4);
        memcpy(&max_a, cases.data() + pos + 4, 4);
        memcpy(&na, cases.data() + pos + 8, 8);
        memcpy(&nb, cases.data() + pos + 16, 8);
        pos += 24;
        REQUIRE(na >= 0 && nb >= 0 && pos + (size_t)na + (size_t)nb <= cases.size());
        const char* a = exact_copy(cases.data() + pos, na);
        const char* b = exact_copy(cases.data() + pos + na, nb);
        pos += (size_t)na + (size_t)nb;
        // exact-size outputs: a write past max_len ids is reported too
        std::vector<int32_t> ids((size_t)max_len, -7), types((size_t)max_len, -7);
        int32_t len = -1;
        REQUIRE(sqe_tokenize_pair_batch(tok, &a, &na, &b, &nb, 1, max_len, max_a, ids.data(), types.data(), &len) == SQE_OK);
        check_row(ids.data(), types.data(), len, max_len, max_a, cls, sep);
        fwrite(&len, 4, 1, out);
        fwrite(ids.data(), 4, (size_t)max_len, out);
        fwrite(types.data(), 4, (size_t)max_len, out);
        as.push_back(a); bs.push_back(b); an.push_back(na); bn.push_back(nb);
    }
    // the threaded path (64 pairs and more): the rows of the single calls
    const int ML = 48, MA = 12;
    for (size_t lo = 0; lo < as.size(); lo += 70) {
        const int n = (int)std::min<size_t>(70, as.size() - lo);
        std::vector<int32_t> ids((size_t)n * ML, -7), types((size_t)n * ML, -7), lens((size_t)n, -7);
        REQUIRE(sqe_tokenize_pair_batch(tok, as.data() + lo, an.data() + lo, bs.data() + lo, bn.data() + lo, n, ML, MA,
                                        ids.data(), types.data(), lens.data()) == SQE_OK);
        for (int i = 0; i < n; ++i) {
            int32_t rid[ML], rty[ML], rlen = -1;
            REQUIRE(sqe_tokenize_pair_batch(tok, &as[lo + i], &an[lo + i], &bs[lo + i], &bn[lo + i], 1, ML, MA, rid, rty, &rlen) == SQE_OK);
            REQUIRE(lens[i] == rlen);
            REQUIRE(memcmp(rid, ids.data() + (size_t)i * ML, sizeof rid) == 0 && memcmp(rty, types.data() + (size_t)i * ML, sizeof rty) == 0);
        }
    }
    fclose(out);
    for (const char* t : as) free((void*)t);
    for (const char* t : bs) free((void*)t);
    sqe_tokenizer_destroy(tok);
    printf("ok %zu cases\n", as.size());
    return 0;
}
