// Ball query (fixed, multi-radius and per-centroid adaptive radius) and kNN for gfx950
// (SPEC.md §3, §4).  No reference source exists (/root/reference/README.md:1-2).
//
// ball_query: one wave64 owns CW centroids.  Lanes stride over the scene's points in index order
// (64 points per step, one per lane); for every (centroid, radius) pair the in-radius predicate is
// turned into a 64-bit ballot, each accepted lane's output slot is count_so_far + popcount of the
// lower accepted lanes, and the running count is a wave-uniform scalar — so the first `nsample`
// accepted indices land in ascending index order without sorting, exactly as the sequential scan
// of SPEC.md §3 produces them.  d2 is evaluated once per pair and shared by all radii.
#include "common.h"

namespace {

struct BQParams {
    float radii[SAD_MAX_RADII];
    int nsample[SAD_MAX_RADII];
    int32_t *idx[SAD_MAX_RADII];
    int32_t *cnt[SAD_MAX_RADII];   // optional: number of accepted points per centroid, capped at nsample
};

constexpr int BQ_WAVES = 8;
constexpr int BQ_CW = 2;             // centroids of a wave
constexpr int BQ_BLOCK = BQ_WAVES * BQ_CW;
constexpr int BQ_STAGE_MAX = 2048;   // staged form: three planes of ceil64(N) floats, at most 24 KB of LDS
constexpr int BQ_STAGE_LOADS = BQ_STAGE_MAX / (BQ_WAVES * 64);

// STAGED: the workgroup copies its scene into LDS once (planes x | y | z of Np = ceil64(N) floats, the tail holds
// NaN, which no radius accepts) and the scan reads LDS only; the next chunk's reads are issued before the current
// chunk's tests.  !STAGED (N > BQ_STAGE_MAX): the chunks come straight from global memory.
// Per centroid and chunk one ballot against the centroid's widest r^2 gates the per-radius blocks.
// Eight waves of two centroids: with the scene in LDS a chunk read is cheap, and the scan is a chain of ballots, scalar
// tests and branches that only more resident waves hide (DESIGN.md §3.2 has the shapes that were measured).
template <int NR, int CW, bool STAGED>
__global__ __launch_bounds__(BQ_WAVES * 64) void ball_query_kernel(
    const float *__restrict__ xyz, const float *__restrict__ new_xyz,
    const float *__restrict__ radius_pc, BQParams prm, int N, int M) {
    extern __shared__ float bq_lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y;
    const float *p = xyz + (size_t)b * N * 3;
    const int Np = (N + 63) & ~63;
    const float *sx = bq_lds, *sy = bq_lds + Np, *sz = bq_lds + 2 * Np;

    if (STAGED) {
        // point j by thread j mod 512: a wave reads 768 contiguous bytes per step; every load is issued before the first store
        float vx[BQ_STAGE_LOADS], vy[BQ_STAGE_LOADS], vz[BQ_STAGE_LOADS];
#pragma unroll
        for (int k = 0; k < BQ_STAGE_LOADS; ++k) {
            if (k * BQ_WAVES * 64 >= Np) break;          // workgroup-uniform
            const int j = k * BQ_WAVES * 64 + (int)threadIdx.x;
            const int jj = j < N ? j : N - 1;
            vx[k] = p[jj * 3 + 0];
            vy[k] = p[jj * 3 + 1];
            vz[k] = p[jj * 3 + 2];
        }
#pragma unroll
        for (int k = 0; k < BQ_STAGE_LOADS; ++k) {
            if (k * BQ_WAVES * 64 >= Np) break;
            const int j = k * BQ_WAVES * 64 + (int)threadIdx.x;
            if (j < Np) {
                const bool real = j < N;
                bq_lds[j] = real ? vx[k] : __builtin_nanf("");
                bq_lds[Np + j] = real ? vy[k] : __builtin_nanf("");
                bq_lds[2 * Np + j] = real ? vz[k] : __builtin_nanf("");
            }
        }
        __syncthreads();
    }

    const int m0 = (blockIdx.x * BQ_WAVES + wave) * CW;
    if (m0 >= M) return;      // wave-uniform; no barrier follows

    float cx[CW], cy[CW], cz[CW], r2[CW][NR], rw[CW];
    int cnt[CW][NR], first[CW][NR];
    bool active[CW];
    int ndone = 0;
#pragma unroll
    for (int c = 0; c < CW; ++c) {
        active[c] = (m0 + c) < M;
        const int m = active[c] ? m0 + c : M - 1;
        const float *q = new_xyz + ((size_t)b * M + m) * 3;
        cx[c] = q[0];
        cy[c] = q[1];
        cz[c] = q[2];
        rw[c] = -__builtin_inff();
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            float rad = prm.radii[r];
            if (radius_pc) rad = rad * radius_pc[(size_t)b * M + m];
            r2[c][r] = rad * rad;
            rw[c] = r2[c][r] > rw[c] ? r2[c][r] : rw[c];      // the widest r^2; a NaN one never wins and accepts nothing
            first[c][r] = 0;
            cnt[c][r] = active[c] ? 0 : prm.nsample[r];
            if (!active[c]) ++ndone;
        }
    }

    float px, py, pz;
    if (STAGED) {
        px = sx[lane];
        py = sy[lane];
        pz = sz[lane];
    }
    for (int base = 0; base < N && ndone < CW * NR; base += 64) {
        const int j = base + lane;
        const bool valid = STAGED || j < N;
        float qx, qy, qz;
        if (STAGED) {
            const int jn = base + 64 < Np ? j + 64 : j;      // the next chunk (the last one reads itself again)
            qx = sx[jn];
            qy = sy[jn];
            qz = sz[jn];
        } else {
            const int jj = valid ? j : N - 1;
            px = p[jj * 3 + 0];
            py = p[jj * 3 + 1];
            pz = p[jj * 3 + 2];
        }
#pragma unroll
        for (int c = 0; c < CW; ++c) {
            const float d = sad::d2f(px, py, pz, cx[c], cy[c], cz[c]);
            if (__ballot(valid && (d < rw[c])) == 0ull) continue;      // wave-uniform: no radius of this centroid accepts a point of the chunk
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                if (cnt[c][r] >= prm.nsample[r]) continue;      // wave-uniform: full
                const bool in = valid && (d < r2[c][r]);
                const unsigned long long mask = __ballot(in);
                if (mask != 0ull) {  // wave-uniform
                    const int slot = cnt[c][r] + __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
                    if (in && slot < prm.nsample[r])
                        prm.idx[r][((size_t)b * M + (m0 + c)) * prm.nsample[r] + slot] = j;
                    if (cnt[c][r] == 0) first[c][r] = base + __builtin_ctzll(mask);
                    cnt[c][r] += __builtin_popcountll(mask);
                    if (cnt[c][r] >= prm.nsample[r]) ++ndone;
                }
            }
        }
        if (STAGED) {
            px = qx;
            py = qy;
            pz = qz;
        }
    }
    // SPEC.md §3 padding: remaining slots repeat the first accepted index (0 if none).
#pragma unroll
    for (int c = 0; c < CW; ++c) {
        if (!active[c]) continue;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const int S = prm.nsample[r];
            const int n = cnt[c][r] < S ? cnt[c][r] : S;
            for (int s = n + lane; s < S; s += 64)
                prm.idx[r][((size_t)b * M + (m0 + c)) * S + s] = first[c][r];
            if (prm.cnt[r] && lane == 0) prm.cnt[r][(size_t)b * M + (m0 + c)] = n;
        }
    }
}

template <int NR>
void launch_bq(const float *xyz, const float *new_xyz, const float *radius_pc, const BQParams &prm,
               int B, int N, int M, hipStream_t st) {
    dim3 grid((M + BQ_BLOCK - 1) / BQ_BLOCK, B);
    const size_t lds = N <= BQ_STAGE_MAX ? (size_t)3 * ((N + 63) & ~63) * sizeof(float) : 0;
    auto kernel = N <= BQ_STAGE_MAX ? ball_query_kernel<NR, BQ_CW, true> : ball_query_kernel<NR, BQ_CW, false>;
    hipLaunchKernelGGL(kernel, grid, dim3(BQ_WAVES * 64), lds, st, xyz, new_xyz, radius_pc, prm, N, M);
}

// ---- kNN: one wave per centroid; lane i holds the i-th best (d2, j) so far -------------------
__global__ __launch_bounds__(256) void knn_kernel(const float *__restrict__ xyz,
                                                  const float *__restrict__ new_xyz, int N, int M,
                                                  int K, int32_t *__restrict__ idx) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y;
    const int m = blockIdx.x * 4 + wave;
    if (m >= M) return;
    const float *p = xyz + (size_t)b * N * 3;
    const float *q = new_xyz + ((size_t)b * M + m) * 3;
    const float cx = q[0], cy = q[1], cz = q[2];
    float ld = __builtin_inff();  // sorted list, ascending (d2, j); lanes >= K stay +inf
    int lj = 0;
    float worst = __builtin_inff();
    // entries of the list in use (wave-uniform).  A list that is not full takes any d2, +inf included: finite points whose
    // squared distance overflows are ordinary candidates (SPEC.md §4 orders them by index behind the finite ones), and
    // `d < worst` alone left index 0 in their place
    int filled = 0;
    for (int base = 0; base < N; base += 64) {
        const int j = base + lane;
        const bool valid = j < N;
        const int jj = valid ? j : N - 1;
        const float d = sad::d2f(p[jj * 3 + 0], p[jj * 3 + 1], p[jj * 3 + 2], cx, cy, cz);
        unsigned long long mask = __ballot(valid && (d < worst || filled < K));
        while (mask) {
            const int l = __builtin_ctzll(mask);
            mask &= mask - 1;
            const float xd = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, d), l));
            if (!(xd < worst) && filled >= K) continue;  // the list tightened since the ballot
            // equal d2 with a lower index is already in the list -> the new entry goes after it
            const int pos = __builtin_popcountll(__ballot(lane < filled && ld <= xd));
            const float ud = __shfl_up(ld, 1, 64);
            const int uj = __shfl_up(lj, 1, 64);
            if (lane > pos) {
                ld = ud;
                lj = uj;
            } else if (lane == pos) {
                ld = xd;
                lj = base + l;
            }
            if (lane >= K) ld = __builtin_inff();
            filled = filled < K ? filled + 1 : K;
            worst = filled < K ? __builtin_inff() : __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ld), K - 1));
        }
    }
    if (lane < K) idx[((size_t)b * M + m) * K + lane] = lj;
}

int check_common(const char *fn, const void *xyz, const void *new_xyz, int B, int N, int M) {
    if (!xyz || !new_xyz) return sad::fail(SAD_EINVAL, "%s: NULL pointer", fn);
    if (B < 1 || N < 1 || M < 1) return sad::fail(SAD_EINVAL, "%s: need B,N,M >= 1 (B=%d N=%d M=%d)", fn, B, N, M);
    if (B > 65535) return sad::fail(SAD_EUNSUPPORTED, "%s: B=%d > 65535", fn, B);
    if ((size_t)N * 3 >= (1u << 31)) return sad::fail(SAD_EUNSUPPORTED, "%s: N too large", fn);
    return SAD_OK;
}

}  // namespace

SAD_API int sad_ball_query_multi_f32(const float *xyz, const float *new_xyz, int n_radii,
                                     const float *radii, const float *radius_pc,
                                     const int *nsamples, int32_t *const *idx, int32_t *const *cnt,
                                     int B, int N, int M, sad_stream_t stream) {
    if (int e = check_common("sad_ball_query_multi_f32", xyz, new_xyz, B, N, M)) return e;
    SAD_REQUIRE(n_radii >= 1 && n_radii <= SAD_MAX_RADII, "sad_ball_query_multi_f32: n_radii=%d not in 1..%d", n_radii, SAD_MAX_RADII);
    SAD_REQUIRE(radii && nsamples && idx, "sad_ball_query_multi_f32: NULL parameter array");
    BQParams prm{};
    for (int r = 0; r < n_radii; ++r) {
        SAD_REQUIRE(nsamples[r] >= 1 && nsamples[r] <= 64, "sad_ball_query: nsample=%d not in 1..64", nsamples[r]);
        SAD_REQUIRE(idx[r], "sad_ball_query: NULL idx output");
        prm.radii[r] = radii[r];
        prm.nsample[r] = nsamples[r];
        prm.idx[r] = idx[r];
        prm.cnt[r] = cnt ? cnt[r] : nullptr;
    }
    hipStream_t st = (hipStream_t)stream;
    switch (n_radii) {
        case 1: launch_bq<1>(xyz, new_xyz, radius_pc, prm, B, N, M, st); break;
        case 2: launch_bq<2>(xyz, new_xyz, radius_pc, prm, B, N, M, st); break;
        case 3: launch_bq<3>(xyz, new_xyz, radius_pc, prm, B, N, M, st); break;
        default: launch_bq<4>(xyz, new_xyz, radius_pc, prm, B, N, M, st); break;
    }
    return sad::check_launch("sad_ball_query");
}

SAD_API int sad_ball_query_f32(const float *xyz, const float *new_xyz, float radius,
                               const float *radius_pc, int B, int N, int M, int S, int32_t *idx,
                               sad_stream_t stream) {
    const float radii[1] = {radius_pc ? 1.0f : radius};  // 1.0f * r == r exactly
    const int ns[1] = {S};
    int32_t *const outs[1] = {idx};
    return sad_ball_query_multi_f32(xyz, new_xyz, 1, radii, radius_pc, ns, outs, nullptr, B, N, M, stream);
}

SAD_API int sad_knn_f32(const float *xyz, const float *new_xyz, int B, int N, int M, int K,
                        int32_t *idx, sad_stream_t stream) {
    if (int e = check_common("sad_knn_f32", xyz, new_xyz, B, N, M)) return e;
    SAD_REQUIRE(idx, "sad_knn_f32: NULL idx");
    SAD_REQUIRE(K >= 1 && K <= 64 && K <= N, "sad_knn_f32: need 1 <= K <= min(64, N) (K=%d N=%d)", K, N);
    dim3 grid((M + 3) / 4, B);
    hipLaunchKernelGGL(knn_kernel, grid, dim3(256), 0, (hipStream_t)stream, xyz, new_xyz, N, M, K, idx);
    return sad::check_launch("sad_knn_f32");
}
