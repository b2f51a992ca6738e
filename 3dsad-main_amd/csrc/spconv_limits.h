// The limits of the sparse-convolution family (SPEC.md §21, §22), one definition each: spconv.hip, spconv_grad.hip and spconv_pool.hip
// refuse by these.  Host code; included inside each file's anonymous namespace, after common.h.
#pragma once

constexpr int SP_MAX_KVOL = 27;           // 3 x 3 x 3: a kernel offset is one bit of a 32-bit mask
constexpr int SP_MAX_C = 256;             // Cin and Cout

inline int sp_kvol_ok(const char *fn, int Kvol) {
    SAD_REQUIRE(Kvol >= 1, "%s: Kvol must be >= 1 (got %d)", fn, Kvol);
    if (Kvol > SP_MAX_KVOL) return sad::fail(SAD_EUNSUPPORTED, "%s: Kvol = %d (at most %d = 3 x 3 x 3)", fn, Kvol, SP_MAX_KVOL);
    return SAD_OK;
}

inline int sp_channels_ok(const char *fn, int Kvol, int Cin, int Cout) {
    SAD_REQUIRE(Cin >= 1 && Cout >= 1, "%s: Cin, Cout must be >= 1 (got %d, %d)", fn, Cin, Cout);
    if (int rc = sp_kvol_ok(fn, Kvol)) return rc;
    if (Cin > SP_MAX_C || Cout > SP_MAX_C) return sad::fail(SAD_EUNSUPPORTED, "%s: Cin = %d, Cout = %d (at most %d each)", fn, Cin, Cout, SP_MAX_C);
    return SAD_OK;
}

// an index array of `rows` x Kvol entries is addressed with 32-bit element numbers
inline int sp_rows_ok(const char *fn, const char *what, long long rows, int Kvol) {
    if (rows * Kvol >= (1LL << 31)) return sad::fail(SAD_EUNSUPPORTED, "%s: %s * Kvol = %lld must be below 2^31", fn, what, rows * Kvol);
    return SAD_OK;
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
