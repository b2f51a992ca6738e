// Feature propagation (SPEC.md §18): three_nn, three_interpolate and its backward — the operators a
// PointNet++-style FP layer imports next to fps / ball_query.
//
// three_nn: one LANE per unknown point (P of them per lane), the best three (d2, j) in registers.
// Every lane of a wave needs the same known point at the same time, so the known points are a
// wave-uniform stream.  Two forms deliver it (option "nn_variant"):
//   0 (default) LDS tiles of float4 records, read with a broadcast ds_read_b128 (4 LDS cycles per
//     wave-instruction), one unknown point per lane (40 VGPRs, 8 waves per SIMD);
//   2 the same with P = 2 unknown points per lane, one read serving both (74 VGPRs, 6 waves per SIMD);
//   1 scalar loads from a wave-uniform address (no LDS, no vector-memory issue).
// Measured at B = 32, n = 16384, m = 4096 (tools/fp_bench.py, two runs): 645-703 / 749-793 / 702-712 us for 0 / 2 / 1 —
// the LDS is not the limit at one point per lane, and the second point costs occupancy.
// The known points are scanned in ascending j, so a strict `<` against the current third best
// keeps the lowest index on ties with no extra compare, and the insertion is skipped with a
// wave-uniform ballot when no lane improves (the common case after the first tiles).
// The weights of §18 are written by the same kernel.
//
// three_interpolate: channel-major (lanes along the unknown points, CH channels per thread) and
// point-major (lanes along 16-byte channel chunks of a row, into a column slice of a wider row).
// three_interpolate_grad: point-major float atomics with the channel axis on the lanes (the
// group_grad_pm_kernel pattern of backward.hip); a channel-major gradient is transposed through LDS
// on the way in.
#include "common.h"

namespace {

constexpr int NN_THREADS = 256;
constexpr int NN_TILE = 1024;           // known points per LDS tile (16 KiB)
constexpr int NN_GROUP = 4;             // known points per ballot

struct Best3 {
    float d0, d1, d2;
    int i0, i1, i2;
};

__device__ __forceinline__ void best3_init(Best3 &s) {
    s.d0 = s.d1 = s.d2 = __builtin_inff();
    s.i0 = s.i1 = s.i2 = 0;
}

// (d, j) with j greater than every index seen so far: strict compares put it behind equal distances
__device__ __forceinline__ void best3_insert(Best3 &s, float d, int j) {
    if (!(d < s.d2)) return;
    const bool c1 = d < s.d1, c0 = d < s.d0;
    s.d2 = c1 ? s.d1 : d;
    s.i2 = c1 ? s.i1 : j;
    s.d1 = c0 ? s.d0 : (c1 ? d : s.d1);
    s.i1 = c0 ? s.i0 : (c1 ? j : s.i1);
    s.d0 = c0 ? d : s.d0;
    s.i0 = c0 ? j : s.i0;
}

__device__ __forceinline__ void nn_store(const Best3 &s, size_t o, float *__restrict__ dist2, int32_t *__restrict__ idx,
                                         float *__restrict__ w) {
    dist2[o + 0] = s.d0;
    dist2[o + 1] = s.d1;
    dist2[o + 2] = s.d2;
    idx[o + 0] = s.i0;
    idx[o + 1] = s.i1;
    idx[o + 2] = s.i2;
    if (w) {
        // r = 1 / (sqrt(d2) + 1e-8): correctly rounded sqrtf and division under hipcc defaults; d2 = +inf gives r = 0
        const float r0 = 1.0f / (sqrtf(s.d0) + 1e-8f);
        const float r1 = 1.0f / (sqrtf(s.d1) + 1e-8f);
        const float r2 = 1.0f / (sqrtf(s.d2) + 1e-8f);
        const float norm = (r0 + r1) + r2;
        w[o + 0] = r0 / norm;
        w[o + 1] = r1 / norm;
        w[o + 2] = r2 / norm;
    }
}

// LDS form: P unknown points per lane, one broadcast float4 read per known point serves all of them
template <int P>
__global__ __launch_bounds__(NN_THREADS) void three_nn_lds_kernel(const float *__restrict__ unknown, const float *__restrict__ known,
                                                                  int n, int m, float *__restrict__ dist2, int32_t *__restrict__ idx,
                                                                  float *__restrict__ w) {
    __shared__ float4 tile[NN_TILE];
    const int b = blockIdx.y;
    const int i0 = blockIdx.x * (NN_THREADS * P) + threadIdx.x;
    const float *kb = known + (size_t)b * m * 3;
    float ux[P], uy[P], uz[P];
    Best3 s[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int i = min(i0 + p * NN_THREADS, n - 1);     // tail lanes scan a copy of the last point and store nothing
        const float *u = unknown + ((size_t)b * n + i) * 3;
        ux[p] = u[0];
        uy[p] = u[1];
        uz[p] = u[2];
        best3_init(s[p]);
    }
    for (int base = 0; base < m; base += NN_TILE) {
        const int cnt = min(NN_TILE, m - base);
        __syncthreads();                                   // the previous tile is no longer read
        const int cnt4 = (cnt + NN_GROUP - 1) / NN_GROUP * NN_GROUP;
        for (int t = threadIdx.x; t < cnt4; t += NN_THREADS) {
            // padding records at +inf: their d2 is +inf, which the strict compare never inserts
            const float *q = kb + (size_t)(base + t) * 3;
            tile[t] = t < cnt ? make_float4(q[0], q[1], q[2], 0.f) : make_float4(__builtin_inff(), __builtin_inff(), __builtin_inff(), 0.f);
        }
        __syncthreads();
        for (int t = 0; t < cnt4; t += NN_GROUP) {       // one ballot per NN_GROUP known points
            float d[NN_GROUP][P];
            bool imp = false;
#pragma unroll
            for (int g = 0; g < NN_GROUP; ++g) {
                const float4 k = tile[t + g];
#pragma unroll
                for (int p = 0; p < P; ++p) {
                    d[g][p] = sad::d2f(k.x, k.y, k.z, ux[p], uy[p], uz[p]);
                    imp |= d[g][p] < s[p].d2;
                }
            }
            if (__ballot(imp)) {
#pragma unroll
                for (int g = 0; g < NN_GROUP; ++g)
#pragma unroll
                    for (int p = 0; p < P; ++p) best3_insert(s[p], d[g][p], base + t + g);
            }
        }
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int i = i0 + p * NN_THREADS;
        if (i < n) nn_store(s[p], ((size_t)b * n + i) * 3, dist2, idx, w);
    }
}

// Scalar form: the known point's address is the same in every lane (scalar loads through the constant cache)
__global__ __launch_bounds__(NN_THREADS) void three_nn_scalar_kernel(const float *__restrict__ unknown, const float *__restrict__ known,
                                                                     int n, int m, float *__restrict__ dist2, int32_t *__restrict__ idx,
                                                                     float *__restrict__ w) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * NN_THREADS + threadIdx.x;
    const float *u = unknown + ((size_t)b * n + min(i, n - 1)) * 3;
    const float ux = u[0], uy = u[1], uz = u[2];
    const float *kb = known + (size_t)b * m * 3;
    Best3 s;
    best3_init(s);
    const int m4 = m / NN_GROUP * NN_GROUP;
    for (int j = 0; j < m4; j += NN_GROUP) {
        float d[NN_GROUP];
        bool imp = false;
#pragma unroll
        for (int g = 0; g < NN_GROUP; ++g) {
            const float *q = kb + (j + g) * 3;
            d[g] = sad::d2f(q[0], q[1], q[2], ux, uy, uz);
            imp |= d[g] < s.d2;
        }
        if (__ballot(imp)) {
#pragma unroll
            for (int g = 0; g < NN_GROUP; ++g) best3_insert(s, d[g], j + g);
        }
    }
    for (int j = m4; j < m; ++j) best3_insert(s, sad::d2f(kb[j * 3 + 0], kb[j * 3 + 1], kb[j * 3 + 2], ux, uy, uz), j);
    if (i < n) nn_store(s, ((size_t)b * n + i) * 3, dist2, idx, w);
}

// ---- three_interpolate ----------------------------------------------------------------------
constexpr int CM_CH = 16;      // channels per thread of the channel-major form

__device__ __forceinline__ float interp1(float w0, float w1, float w2, float f0, float f1, float f2) {
    const float a = w0 * f0, bb = w1 * f1, c = w2 * f2;
    const float s = a + bb;
    return s + c;
}

__device__ __forceinline__ void load_iw(const int32_t *__restrict__ idx, const float *__restrict__ w, size_t o, int j[3], float ww[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        j[k] = idx[o + k];
        ww[k] = w[o + k];
    }
}

// feat [B,C,m] -> out [B,C,n]; an index outside [0,m) reads a zero feature (never memory outside the scene)
__global__ __launch_bounds__(256) void interp_cm_kernel(const float *__restrict__ feat, const int32_t *__restrict__ idx,
                                                        const float *__restrict__ w, int C, int m, int n, float *__restrict__ out) {
    const int b = blockIdx.z;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int j[3];
    float ww[3];
    load_iw(idx, w, ((size_t)b * n + i) * 3, j, ww);
    bool ok[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        ok[k] = (unsigned)j[k] < (unsigned)m;
        j[k] = ok[k] ? j[k] : 0;
    }
    const int c0 = blockIdx.y * CM_CH;
#pragma unroll 4
    for (int cc = 0; cc < CM_CH; ++cc) {
        const int c = c0 + cc;
        if (c >= C) break;
        const float *f = feat + ((size_t)b * C + c) * m;
        const float f0 = ok[0] ? f[j[0]] : 0.f, f1 = ok[1] ? f[j[1]] : 0.f, f2 = ok[2] ? f[j[2]] : 0.f;
        out[((size_t)b * C + c) * n + i] = interp1(ww[0], ww[1], ww[2], f0, f1, f2);
    }
}

// feat [B,m,C] -> out rows (b*n + i)*ld_out + col_off + [0, C); one thread per (point, chunk), VEC = 4: 16-byte chunks
template <int VEC>
__global__ __launch_bounds__(256) void interp_pm_kernel(const float *__restrict__ feat, const int32_t *__restrict__ idx,
                                                        const float *__restrict__ w, int C, int m, int n, long long rows,
                                                        float *__restrict__ out, int ld_out, int col_off) {
    const int cpr = C / VEC;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= rows * cpr) return;
    const long long r = e / cpr;                 // (b, i) row
    const int q = (int)(e - r * cpr);
    const long long b = r / n;
    int j[3];
    float ww[3];
    load_iw(idx, w, (size_t)r * 3, j, ww);
    const float *fb = feat + (size_t)b * m * C + (size_t)q * VEC;
    float *o = out + (size_t)r * ld_out + col_off + (size_t)q * VEC;
    if constexpr (VEC == 4) {
        float4 f[3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            f[k] = (unsigned)j[k] < (unsigned)m ? *(const float4 *)(fb + (size_t)j[k] * C) : make_float4(0.f, 0.f, 0.f, 0.f);
        float4 v;
        v.x = interp1(ww[0], ww[1], ww[2], f[0].x, f[1].x, f[2].x);
        v.y = interp1(ww[0], ww[1], ww[2], f[0].y, f[1].y, f[2].y);
        v.z = interp1(ww[0], ww[1], ww[2], f[0].z, f[1].z, f[2].z);
        v.w = interp1(ww[0], ww[1], ww[2], f[0].w, f[1].w, f[2].w);
        *(float4 *)o = v;
    } else {
        float f[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) f[k] = (unsigned)j[k] < (unsigned)m ? fb[(size_t)j[k] * C] : 0.f;
        *o = interp1(ww[0], ww[1], ww[2], f[0], f[1], f[2]);
    }
}

// ---- three_interpolate_grad -----------------------------------------------------------------
// grad_out point-major [B,n,C]: one thread per (point, channel), channels on the lanes
__global__ __launch_bounds__(256) void interp_grad_pm_kernel(const float *__restrict__ gout, const int32_t *__restrict__ idx,
                                                             const float *__restrict__ w, int C, int m, int n, long long rows,
                                                             float *__restrict__ gfeat_pm) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= rows * C) return;
    const long long r = e / C;
    const int c = (int)(e - r * C);
    const float g = gout[e];
    if (g == 0.f) return;
    const long long b = r / n;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int j = idx[(size_t)r * 3 + k];
        const float t = w[(size_t)r * 3 + k] * g;
        if ((unsigned)j < (unsigned)m && t != 0.f) atomicAdd(gfeat_pm + ((size_t)b * m + j) * C + c, t);
    }
}

// grad_out channel-major [B,C,n]: a 64-channel x 64-point tile read coalesced along the points, transposed through LDS,
// then each wave walks the points with the channels on the lanes
__global__ __launch_bounds__(256) void interp_grad_cm_kernel(const float *__restrict__ gout, const int32_t *__restrict__ idx,
                                                             const float *__restrict__ w, int C, int m, int n,
                                                             float *__restrict__ gfeat_pm) {
    __shared__ float tile[64][65];
    __shared__ int sidx[64][3];
    __shared__ float sw[64][3];
    const int b = blockIdx.z, c0 = blockIdx.y * 64, t0 = blockIdx.x * 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < 192) {
        const int t = threadIdx.x / 3, k = threadIdx.x - 3 * (threadIdx.x / 3);
        const bool in = t0 + t < n;
        sidx[t][k] = in ? idx[((size_t)b * n + t0 + t) * 3 + k] : -1;
        sw[t][k] = in ? w[((size_t)b * n + t0 + t) * 3 + k] : 0.f;
    }
    for (int cc = wave; cc < 64; cc += 4) {
        const int c = c0 + cc, t = t0 + lane;
        tile[cc][lane] = (c < C && t < n) ? gout[((size_t)b * C + c) * n + t] : 0.f;
    }
    __syncthreads();
    const int c = c0 + lane;
    if (c >= C) return;
    for (int tt = wave; tt < 64; tt += 4) {
        const float g = tile[lane][tt];
        if (g == 0.f) continue;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int j = sidx[tt][k];
            const float t = sw[tt][k] * g;
            if ((unsigned)j < (unsigned)m && t != 0.f) atomicAdd(gfeat_pm + ((size_t)b * m + j) * C + c, t);
        }
    }
}

}  // namespace

SAD_API int sad_three_nn_f32(const float *unknown, const float *known, int B, int n, int m, float *dist2, int32_t *idx, float *w,
                             sad_stream_t stream) {
    SAD_REQUIRE(unknown && known && dist2 && idx, "sad_three_nn_f32: NULL pointer");
    SAD_REQUIRE(B >= 1 && n >= 1, "sad_three_nn_f32: B and n must be >= 1");
    SAD_REQUIRE(m >= 1, "sad_three_nn_f32: m must be >= 1 (got %d)", m);
    SAD_REQUIRE(B <= 65535 && (long long)B * n * 3 < (1LL << 31) && (long long)m * 3 < (1LL << 31), "sad_three_nn_f32: sizes too large");
    const hipStream_t st = (hipStream_t)stream;
    if (sad::get_option(sad::OPT_NN_VARIANT) == 1) {
        hipLaunchKernelGGL(three_nn_scalar_kernel, dim3((n + NN_THREADS - 1) / NN_THREADS, B), dim3(NN_THREADS), 0, st, unknown, known,
                           n, m, dist2, idx, w);
    } else if (sad::get_option(sad::OPT_NN_VARIANT) == 2) {
        hipLaunchKernelGGL(three_nn_lds_kernel<2>, dim3((n + 2 * NN_THREADS - 1) / (2 * NN_THREADS), B), dim3(NN_THREADS), 0, st,
                           unknown, known, n, m, dist2, idx, w);
    } else {
        hipLaunchKernelGGL(three_nn_lds_kernel<1>, dim3((n + NN_THREADS - 1) / NN_THREADS, B), dim3(NN_THREADS), 0, st, unknown, known,
                           n, m, dist2, idx, w);
    }
    return sad::check_launch("sad_three_nn_f32");
}

SAD_API int sad_three_interpolate_f32(const float *feat, const int32_t *idx, const float *w, int B, int C, int m, int n, int point_major,
                                      float *out, int ld_out, int col_off, sad_stream_t stream) {
    SAD_REQUIRE(feat && idx && w && out, "sad_three_interpolate_f32: NULL pointer");
    SAD_REQUIRE(B >= 1 && C >= 1 && n >= 1, "sad_three_interpolate_f32: B, C and n must be >= 1");
    SAD_REQUIRE(m >= 1, "sad_three_interpolate_f32: m must be >= 1 (got %d)", m);
    SAD_REQUIRE(point_major == 0 || point_major == 1, "sad_three_interpolate_f32: layout must be 0 (channel-major) or 1 (point-major), got %d",
                point_major);
    const hipStream_t st = (hipStream_t)stream;
    if (!point_major) {
        SAD_REQUIRE(col_off == 0 && ld_out == n, "sad_three_interpolate_f32: channel-major output is [B,C,n]: col_off must be 0 and ld_out n");
        SAD_REQUIRE(B <= 65535 && (C + CM_CH - 1) / CM_CH <= 65535, "sad_three_interpolate_f32: B or C too large");
        dim3 grid((n + 255) / 256, (C + CM_CH - 1) / CM_CH, B);
        hipLaunchKernelGGL(interp_cm_kernel, grid, dim3(256), 0, st, feat, idx, w, C, m, n, out);
        return sad::check_launch("sad_three_interpolate_f32");
    }
    SAD_REQUIRE(col_off >= 0 && ld_out >= col_off + C, "sad_three_interpolate_f32: bad col_off %d / ld_out %d for C = %d", col_off, ld_out, C);
    const long long rows = (long long)B * n;
    const bool vec = C % 4 == 0 && ld_out % 4 == 0 && col_off % 4 == 0 && ((uintptr_t)feat & 15) == 0 && ((uintptr_t)out & 15) == 0;
    const long long threads = rows * (vec ? C / 4 : C);
    SAD_REQUIRE((threads + 255) / 256 < (1LL << 31), "sad_three_interpolate_f32: sizes too large");
    const dim3 grid((unsigned)((threads + 255) / 256));
    if (vec)
        hipLaunchKernelGGL(interp_pm_kernel<4>, grid, dim3(256), 0, st, feat, idx, w, C, m, n, rows, out, ld_out, col_off);
    else
        hipLaunchKernelGGL(interp_pm_kernel<1>, grid, dim3(256), 0, st, feat, idx, w, C, m, n, rows, out, ld_out, col_off);
    return sad::check_launch("sad_three_interpolate_f32");
}

SAD_API int sad_three_interpolate_grad_f32(const float *grad_out, const int32_t *idx, const float *w, int B, int C, int n, int m,
                                           int point_major, float *grad_feat_pm, sad_stream_t stream) {
    SAD_REQUIRE(grad_out && idx && w && grad_feat_pm, "sad_three_interpolate_grad_f32: NULL pointer");
    SAD_REQUIRE(B >= 1 && C >= 1 && n >= 1, "sad_three_interpolate_grad_f32: B, C and n must be >= 1");
    SAD_REQUIRE(m >= 1, "sad_three_interpolate_grad_f32: m must be >= 1 (got %d)", m);
    SAD_REQUIRE(point_major == 0 || point_major == 1,
                "sad_three_interpolate_grad_f32: layout must be 0 (channel-major) or 1 (point-major), got %d", point_major);
    const hipStream_t st = (hipStream_t)stream;
    if (!point_major) {
        SAD_REQUIRE(B <= 65535 && (C + 63) / 64 <= 65535, "sad_three_interpolate_grad_f32: B or C too large");
        dim3 grid((n + 63) / 64, (C + 63) / 64, B);
        hipLaunchKernelGGL(interp_grad_cm_kernel, grid, dim3(256), 0, st, grad_out, idx, w, C, m, n, grad_feat_pm);
        return sad::check_launch("sad_three_interpolate_grad_f32");
    }
    const long long rows = (long long)B * n;
    SAD_REQUIRE((rows * C + 255) / 256 < (1LL << 31), "sad_three_interpolate_grad_f32: sizes too large");
    hipLaunchKernelGGL(interp_grad_pm_kernel, dim3((unsigned)((rows * C + 255) / 256)), dim3(256), 0, st, grad_out, idx, w, C, m, n, rows,
                       grad_feat_pm);
    return sad::check_launch("sad_three_interpolate_grad_f32");
}
