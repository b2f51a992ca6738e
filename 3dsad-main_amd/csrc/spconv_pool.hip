// Sparse max pool over a rulebook and its backward (SPEC.md §22.1, §22.2).  The upstream reference has no such operator; the semantics
// are SPEC.md's own.
//
// Both kernels are gathers bounded by memory traffic.  One form serves both: a workgroup (256 threads) owns a tile of R consecutive
// rows of the index array (nbr [No,Kvol] for the pool, nbrT [Nv,Kvol] for its backward), R a power of two in 16 .. 256 chosen on the
// host.  The tile's R x Kvol indices are one contiguous run of memory: they are read ONCE, coalesced, into LDS, and every channel of
// a row then takes its neighbour list from there (an LDS broadcast: the lanes of a row read one address), not from memory again.
// An item is (row, 4 consecutive channels) when C % 4 == 0 and the arrays are 16-byte aligned — 16-byte loads and stores, the lanes
// of a row side by side — and (row, channel) otherwise (a row of C % 4 != 0 floats does not begin on a 16-byte boundary).  Items go
// to the threads round robin, so a wave's stores are whole contiguous rows.
// The neighbour list is walked kk ascending in groups of four: the (up to) four row loads of a group are issued before the first is
// used, an entry outside [0, rows) costs no load (its lanes are masked off), and the walk keeps the order the definitions fix —
// "strictly greater replaces" for the pool (ties, -0.0f against +0.0f included, stay with the lowest kk), one rounding per addition
// in kk order for the backward.  No atomics, no scratch: two calls give the same bits.
// maxpool       out[o][c] = a bit copy of the winning feat element, arg[o][c] = its global input row; 0.0f / -1 for a row without
//               a valid entry.
// maxpool grad  grad_feat[i][c] = sum over kk ascending of g[o][c] for o = nbrT[i,kk] valid with arg[o][c] == i, from +0.0f.
#include "common.h"
#include <algorithm>

namespace {

#include "spconv_limits.h"
constexpr int SP_THREADS = 256, SP_GROUP = 4, SP_MIN_ROWS = 16, SP_MAX_ROWS = 256, SP_ITEMS = 1024;

// the tile's index rows -> LDS (entries of rows beyond `rows_total` are never read)
__device__ __forceinline__ int stage_rows(const int32_t *__restrict__ idx, long long row0, long long rows_total, int R, int Kvol, int32_t *s_idx) {
    const int nrows = (int)(rows_total - row0 < R ? rows_total - row0 : R);
    const int32_t *src = idx + (size_t)row0 * Kvol;
    for (int e = threadIdx.x; e < nrows * Kvol; e += SP_THREADS) s_idx[e] = src[e];
    __syncthreads();
    return nrows;
}

template <int V> struct Vec;
template <> struct Vec<1> { using F = float; using I = int32_t; };
template <> struct Vec<4> { using F = float4; using I = int4; };

// (selects, not branches: every loaded value is consumed on every path, so the loads of a group stay in flight together)
__device__ __forceinline__ void pool_take(float &cur, int32_t &arg, float v, int n, bool first) {
    const bool take = n >= 0 && (first || v > cur);
    cur = take ? v : cur;
    arg = take ? n : arg;
}
__device__ __forceinline__ void pool_take(float4 &cur, int4 &arg, const float4 &v, int n, bool first) {
    pool_take(cur.x, arg.x, v.x, n, first);
    pool_take(cur.y, arg.y, v.y, n, first);
    pool_take(cur.z, arg.z, v.z, n, first);
    pool_take(cur.w, arg.w, v.w, n, first);
}
__device__ __forceinline__ void grad_take(float &acc, int32_t a, float g, int i) {
    const float sum = acc + g;
    acc = a == i ? sum : acc;
}
__device__ __forceinline__ void grad_take(float4 &acc, const int4 &a, const float4 &g, int i) {
    grad_take(acc.x, a.x, g.x, i);
    grad_take(acc.y, a.y, g.y, i);
    grad_take(acc.z, a.z, g.z, i);
    grad_take(acc.w, a.w, g.w, i);
}
__device__ __forceinline__ void set_all(float &f, float v) { f = v; }
__device__ __forceinline__ void set_all(float4 &f, float v) { f = make_float4(v, v, v, v); }
__device__ __forceinline__ void set_all(int32_t &f, int v) { f = v; }
__device__ __forceinline__ void set_all(int4 &f, int v) { f = make_int4(v, v, v, v); }

// V = channels of an item (4: C % 4 == 0 and aligned arrays; 1 otherwise); CQ = items of a row (C / V)
template <int V>
__global__ __launch_bounds__(SP_THREADS) void spconv_max_pool_kernel(const float *__restrict__ feat, const int32_t *__restrict__ nbr, int Nv, int No,
                                                                     int Kvol, int CQ, int R, float *__restrict__ out, int32_t *__restrict__ arg) {
    using F = typename Vec<V>::F;
    using I = typename Vec<V>::I;
    extern __shared__ __attribute__((aligned(16))) int32_t sp_idx[];
    const long long row0 = (long long)blockIdx.x * R;
    const int nrows = stage_rows(nbr, row0, No, R, Kvol, sp_idx);
    const F *__restrict__ src = reinterpret_cast<const F *>(feat);
    for (int it = threadIdx.x; it < nrows * CQ; it += SP_THREADS) {
        const int r = it / CQ, q = it - r * CQ;
        const int32_t *list = sp_idx + r * Kvol;
        F cur;
        I win;
        set_all(cur, 0.0f);
        set_all(win, -1);
        bool first = true;
        for (int k0 = 0; k0 < Kvol; k0 += SP_GROUP) {
            int n[SP_GROUP];
            F v[SP_GROUP];
#pragma unroll
            for (int j = 0; j < SP_GROUP; ++j) {
                n[j] = k0 + j < Kvol ? list[k0 + j] : -1;
                if ((unsigned)n[j] >= (unsigned)Nv) n[j] = -1;   // (never read outside feat, whatever the caller passed)
            }
#pragma unroll
            for (int j = 0; j < SP_GROUP; ++j) {
                set_all(v[j], 0.0f);
                if (n[j] >= 0) v[j] = src[(size_t)n[j] * CQ + q];
            }
#pragma unroll
            for (int j = 0; j < SP_GROUP; ++j) {
                pool_take(cur, win, v[j], n[j], first);
                first = first && n[j] < 0;
            }
        }
        const size_t dst = (size_t)(row0 + r) * CQ + q;
        reinterpret_cast<F *>(out)[dst] = cur;
        reinterpret_cast<I *>(arg)[dst] = win;
    }
}

template <int V>
__global__ __launch_bounds__(SP_THREADS) void spconv_max_pool_grad_kernel(const float *__restrict__ g, const int32_t *__restrict__ arg,
                                                                          const int32_t *__restrict__ nbrT, int Nv, int No, int Kvol, int CQ, int R,
                                                                          float *__restrict__ grad_feat) {
    using F = typename Vec<V>::F;
    using I = typename Vec<V>::I;
    extern __shared__ __attribute__((aligned(16))) int32_t sp_idx[];
    const long long row0 = (long long)blockIdx.x * R;
    const int nrows = stage_rows(nbrT, row0, Nv, R, Kvol, sp_idx);
    const F *__restrict__ gsrc = reinterpret_cast<const F *>(g);
    const I *__restrict__ asrc = reinterpret_cast<const I *>(arg);
    for (int it = threadIdx.x; it < nrows * CQ; it += SP_THREADS) {
        const int r = it / CQ, q = it - r * CQ;
        const int i = (int)(row0 + r);
        const int32_t *list = sp_idx + r * Kvol;
        F acc;
        set_all(acc, 0.0f);
        for (int k0 = 0; k0 < Kvol; k0 += SP_GROUP) {
            int o[SP_GROUP];
            F gv[SP_GROUP];
            I av[SP_GROUP];
#pragma unroll
            for (int j = 0; j < SP_GROUP; ++j) {
                o[j] = k0 + j < Kvol ? list[k0 + j] : -1;
                if ((unsigned)o[j] >= (unsigned)No) o[j] = -1;   // (never read outside g and arg)
            }
#pragma unroll
            for (int j = 0; j < SP_GROUP; ++j) {
                set_all(av[j], -1);                              // (no row: i >= 0, so an entry without a load adds nothing)
                set_all(gv[j], 0.0f);
                if (o[j] >= 0) {
                    av[j] = asrc[(size_t)o[j] * CQ + q];
                    gv[j] = gsrc[(size_t)o[j] * CQ + q];
                }
            }
#pragma unroll
            for (int j = 0; j < SP_GROUP; ++j) grad_take(acc, av[j], gv[j], i);
        }
        reinterpret_cast<F *>(grad_feat)[(size_t)(row0 + r) * CQ + q] = acc;
    }
}

// rows of a tile: about SP_ITEMS items per workgroup, halved while the grid stays below two workgroups per compute unit
inline int tile_rows(long long rows, int CQ) {
    int R = SP_MAX_ROWS;
    while (R > SP_MIN_ROWS && (long long)(R / 2) * CQ >= SP_ITEMS) R /= 2;
    const long long want = 2LL * sad::device_cus();
    while (R > SP_MIN_ROWS && (rows + R - 1) / R < want) R /= 2;
    return R;
}

int pool_args_ok(const char *fn, int Nv, int No, int Kvol, int C) {
    SAD_REQUIRE(Nv >= 0 && No >= 0, "%s: Nv and No must be >= 0 (got %d, %d)", fn, Nv, No);
    SAD_REQUIRE(C >= 1, "%s: C must be >= 1 (got %d)", fn, C);
    if (int rc = sp_kvol_ok(fn, Kvol)) return rc;
    if ((long long)Nv * C >= (1LL << 31) || (long long)No * C >= (1LL << 31))
        return sad::fail(SAD_EUNSUPPORTED, "%s: Nv * C and No * C must be below 2^31 (got %d, %d rows of %d)", fn, Nv, No, C);
    return SAD_OK;
}

}  // namespace

SAD_API int sad_spconv_max_pool_f32(const float *feat, const int32_t *nbr, int Nv, int No, int Kvol, int C, float *out, int32_t *arg,
                                    sad_stream_t stream) {
    if (int rc = pool_args_ok("sad_spconv_max_pool_f32", Nv, No, Kvol, C)) return rc;
    SAD_REQUIRE((Nv == 0 || feat) && (No == 0 || (nbr && out && arg)), "sad_spconv_max_pool_f32: NULL pointer");
    if (No == 0) return SAD_OK;
    const hipStream_t st = (hipStream_t)stream;
    const bool vec = C % 4 == 0 && aligned16(feat) && aligned16(out) && aligned16(arg);
    const int CQ = vec ? C / 4 : C, R = tile_rows(No, CQ);
    const unsigned grid = (unsigned)(((long long)No + R - 1) / R);
    const size_t lds = (size_t)R * Kvol * sizeof(int32_t);
    if (vec)
        hipLaunchKernelGGL((spconv_max_pool_kernel<4>), dim3(grid), dim3(SP_THREADS), lds, st, feat, nbr, Nv, No, Kvol, CQ, R, out, arg);
    else
        hipLaunchKernelGGL((spconv_max_pool_kernel<1>), dim3(grid), dim3(SP_THREADS), lds, st, feat, nbr, Nv, No, Kvol, CQ, R, out, arg);
    return sad::check_launch("sad_spconv_max_pool_f32");
}

SAD_API int sad_spconv_max_pool_grad_f32(const float *g, const int32_t *arg, const int32_t *nbrT, int Nv, int No, int Kvol, int C,
                                         float *grad_feat, sad_stream_t stream) {
    if (int rc = pool_args_ok("sad_spconv_max_pool_grad_f32", Nv, No, Kvol, C)) return rc;
    SAD_REQUIRE((No == 0 || (g && arg)) && (Nv == 0 || (nbrT && grad_feat)), "sad_spconv_max_pool_grad_f32: NULL pointer");
    if (Nv == 0) return SAD_OK;
    const hipStream_t st = (hipStream_t)stream;
    const bool vec = C % 4 == 0 && aligned16(g) && aligned16(arg) && aligned16(grad_feat);
    const int CQ = vec ? C / 4 : C, R = tile_rows(Nv, CQ);
    const unsigned grid = (unsigned)(((long long)Nv + R - 1) / R);
    const size_t lds = (size_t)R * Kvol * sizeof(int32_t);
    if (vec)
        hipLaunchKernelGGL((spconv_max_pool_grad_kernel<4>), dim3(grid), dim3(SP_THREADS), lds, st, g, arg, nbrT, Nv, No, Kvol, CQ, R, grad_feat);
    else
        hipLaunchKernelGGL((spconv_max_pool_grad_kernel<1>), dim3(grid), dim3(SP_THREADS), lds, st, g, arg, nbrT, Nv, No, Kvol, CQ, R, grad_feat);
    return sad::check_launch("sad_spconv_max_pool_grad_f32");
}
