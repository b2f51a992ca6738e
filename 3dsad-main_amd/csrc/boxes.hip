// Box operators (SPEC.md §19): pairwise BEV / 3-D IoU, points_in_boxes and roipoint_pool3d — the box-level
// operators a detector's users reach for after NMS.  The geometry (corners, the clip, inside() and its constants) is
// box_geom.h's, shared with every other box kernel, so every decision is bit-identical to the CPU oracle.
//
// boxes_iou: a 2-D grid of IOU_TA x IOU_TB pair tiles per scene.  A workgroup computes the local corners, centres, areas and
// heights of its tile's boxes once into LDS, then each thread clips one pair with poly_clip_area<256> in
// thread-interleaved LDS scratch (the NMS mask kernel's layout).  One kernel, a mode argument (BEV / 3-D).
//
// points_in_boxes: one lane per point.  The per-box constants (cx,cy,cz, l/2, w/2, h/2, c, s) are computed by
// the workgroup into LDS tiles of PIB_TILE boxes, scanned in ascending k; the first hit is the answer, so a wave
// stops scanning once a ballot shows every lane has one, and the workgroup stops loading tiles once all do.
//
// roipoint_pool3d: one workgroup per RP_BPB boxes of a scene (fewer for large S), up to four boxes per wave.
// The scene's points stream through LDS tiles shared by all the workgroup's boxes; per 64 points and box the
// in-box predicate is a ballot, an accepted lane's slot is the running count plus the popcount of the lower
// accepted lanes (the ball-query scan of ball_query.hip), so the first S indices land in ascending order in
// LDS, and a box stops at S.  The cyclic fill is made in LDS, then the workgroup copies its boxes' rows
// [xyz || feat] (16-byte stores when the row width 3 + C is a multiple of 4, as in interp.hip's point-major form).
#include "box_geom.h"

namespace {

constexpr int IOU_TA = 8, IOU_TB = 32;     // a-boxes x b-boxes per workgroup (256 pairs): one pair per thread
constexpr int PIB_THREADS = 256;
constexpr int PIB_TILE = 256;              // boxes per LDS tile (8 KiB)
constexpr int RP_THREADS = 256;
constexpr int RP_TILE = 1024;              // points per LDS tile (12 KiB)
constexpr int RP_BPW = 4;                  // boxes per wave at most
constexpr int RP_SEL_INTS = 8192;          // LDS for the selected indices of a workgroup's boxes (32 KiB): S <= 8192

// ---- pairwise IoU -------------------------------------------------------------------------------------------
// grid (ceil(Kb / IOU_TB), ceil(Ka / IOU_TA), B); mode 0 = BEV (§13 iou_bev), 1 = 3-D (§19.3)
__global__ __launch_bounds__(256) void boxes_iou_kernel(const float *__restrict__ a, const float *__restrict__ b, int Ka,
                                                        int Kb, int Da, int Db, int mode, float *__restrict__ iou) {
    __shared__ float s_ax[IOU_TA][4], s_ay[IOU_TA][4], s_ac[IOU_TA][2], s_aarea[IOU_TA], s_az[IOU_TA], s_ah[IOU_TA], s_avol[IOU_TA];
    __shared__ float s_bx[IOU_TB][4], s_by[IOU_TB][4], s_bc[IOU_TB][2], s_barea[IOU_TB], s_bz[IOU_TB], s_bh[IOU_TB], s_bvol[IOU_TB];
    __shared__ float s_poly[4 * 10 * 256];     // per-thread clipping scratch, thread-interleaved
    const int tid = threadIdx.x, sc = blockIdx.z;
    const int i0 = blockIdx.y * IOU_TA, j0 = blockIdx.x * IOU_TB;
    if (tid < IOU_TA + IOU_TB) {
        const bool isa = tid < IOU_TA;
        const int t = isa ? tid : tid - IOU_TA;
        const int k = (isa ? i0 : j0) + t, K = isa ? Ka : Kb;
        if (k < K) {
            const float *bx = isa ? a + ((size_t)sc * Ka + k) * Da : b + ((size_t)sc * Kb + k) * Db;
            // box_footprint3d and, below, height_overlap and iou_of, written out
            float cx[4], cy[4];
            box_corners(bx, cx, cy);
            const float area = bx[3] * bx[4];
            const float vol = area * bx[5];
            float *px = isa ? s_ax[t] : s_bx[t], *py = isa ? s_ay[t] : s_by[t];
#pragma unroll
            for (int q = 0; q < 4; ++q) { px[q] = cx[q]; py[q] = cy[q]; }
            float *pc = isa ? s_ac[t] : s_bc[t];
            pc[0] = bx[0]; pc[1] = bx[1];
            (isa ? s_aarea : s_barea)[t] = area;
            (isa ? s_az : s_bz)[t] = bx[2];
            (isa ? s_ah : s_bh)[t] = bx[5];
            (isa ? s_avol : s_bvol)[t] = vol;
        }
    }
    __syncthreads();
    const int ti = tid / IOU_TB, tj = tid - ti * IOU_TB;
    const int i = i0 + ti, j = j0 + tj;
    if (i >= Ka || j >= Kb) return;
    const float inter = poly_clip_area<256>(s_ax[ti], s_ay[ti], s_ac[ti][0] - s_bc[tj][0], s_ac[ti][1] - s_bc[tj][1], s_bx[tj], s_by[tj], s_poly + tid);
    float r;
    if (mode == 0) {
        float den = s_aarea[ti] + s_barea[tj];
        den = den - inter;
        r = den > 0.0f ? inter / den : 0.0f;
    } else {
        const float ha = 0.5f * s_ah[ti], hb = 0.5f * s_bh[tj];
        const float za = s_az[ti], zb = s_bz[tj];
        const float top = fminf(za + ha, zb + hb), bot = fmaxf(za - ha, zb - hb);
        float oh = top - bot;
        oh = oh > 0.0f ? oh : 0.0f;
        const float i3 = inter * oh;
        float den = s_avol[ti] + s_bvol[tj];
        den = den - i3;
        r = den > 0.0f ? i3 / den : 0.0f;
    }
    iou[((size_t)sc * Ka + i) * Kb + j] = r;
}

// ---- points_in_boxes ----------------------------------------------------------------------------------------
// grid (ceil(N / PIB_THREADS), B)
__global__ __launch_bounds__(PIB_THREADS) void points_in_boxes_kernel(const float *__restrict__ xyz, const float *__restrict__ boxes,
                                                                      int N, int K, int D, int32_t *__restrict__ box_idx) {
    __shared__ float4 s_k0[PIB_TILE], s_k1[PIB_TILE];      // (cx, cy, cz, hl), (hw, hh, c, s)
    const int b = blockIdx.y;
    const int n = blockIdx.x * PIB_THREADS + threadIdx.x;
    const bool valid = n < N;
    const float *p = xyz + ((size_t)b * N + (valid ? n : N - 1)) * 3;
    const float px = p[0], py = p[1], pz = p[2];
    int hit = -1;
    bool done = !valid;                                     // tail lanes count as answered
    for (int base = 0; base < K; base += PIB_TILE) {
        const int cnt = min(PIB_TILE, K - base);
        if (threadIdx.x < cnt) {
            const BoxK k = box_consts(boxes + ((size_t)b * K + base + threadIdx.x) * D, 0.0f);
            s_k0[threadIdx.x] = make_float4(k.cx, k.cy, k.cz, k.hl);
            s_k1[threadIdx.x] = make_float4(k.hw, k.hh, k.c, k.s);
        }
        __syncthreads();
        if (__ballot(!done)) {                              // (wave-uniform)
            for (int t = 0; t < cnt; ++t) {
                const float4 k0 = s_k0[t], k1 = s_k1[t];
                if (!done && inside(px, py, pz, k0.x, k0.y, k0.z, k0.w, k1.x, k1.y, k1.z, k1.w)) {
                    hit = base + t;
                    done = true;
                }
                if ((t & 7) == 7 && !__ballot(!done)) break;   // every lane of the wave has its lowest box
            }
        }
        // every thread of the workgroup is answered: no further tile (also keeps the tile from being overwritten early)
        if (__syncthreads_and(done)) break;
    }
    if (valid) box_idx[(size_t)b * N + n] = hit;
}

// ---- roipoint_pool3d ----------------------------------------------------------------------------------------
// grid (ceil(K / bpb), B); dynamic LDS: bpb * S ints (the selected indices, cyclically filled)
template <int VEC>
__global__ __launch_bounds__(RP_THREADS) void roipoint_pool3d_kernel(const float *__restrict__ xyz, const float *__restrict__ feat,
                                                                     const float *__restrict__ boxes, int N, int K, int D, int C,
                                                                     float e, int S, int bpb, float *__restrict__ pooled,
                                                                     int32_t *__restrict__ empty, int32_t *__restrict__ idx) {
    __shared__ float s_pts[RP_TILE * 3];
    __shared__ int s_cnt[RP_THREADS / 64 * RP_BPW];
    extern __shared__ int s_sel[];                          // [bpb][S]
    const int b = blockIdx.y, k0 = blockIdx.x * bpb;
    const int nb = min(bpb, K - k0);                        // boxes of this workgroup
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // the wave's boxes: local indices wave * bpw + q, q < nbw
    const int bpw = (bpb + RP_THREADS / 64 - 1) / (RP_THREADS / 64);
    const int nbw = max(0, min(bpw, nb - wave * bpw));
    BoxK bk[RP_BPW];
    int cnt[RP_BPW];
#pragma unroll
    for (int q = 0; q < RP_BPW; ++q) {
        const int lb = q < nbw ? wave * bpw + q : 0;        // (a box of the workgroup: nb >= 1)
        bk[q] = box_consts(boxes + ((size_t)b * K + k0 + lb) * D, e);
        cnt[q] = q < nbw ? 0 : S;
    }
    const float *pb = xyz + (size_t)b * N * 3;
    for (int base = 0; base < N; base += RP_TILE) {
        const int np = min(RP_TILE, N - base);
        __syncthreads();                                    // the previous tile is no longer read
        for (int t = threadIdx.x; t < np * 3; t += RP_THREADS) s_pts[t] = pb[(size_t)base * 3 + t];
        __syncthreads();
        bool wdone = true;
#pragma unroll
        for (int q = 0; q < RP_BPW; ++q) wdone = wdone && cnt[q] >= S;
        for (int c0 = 0; c0 < np && !wdone; c0 += 64) {     // (wave-uniform)
            const int t = c0 + lane;
            const bool ok = t < np;
            const int tt = ok ? t : 0;
            const float px = s_pts[tt * 3 + 0], py = s_pts[tt * 3 + 1], pz = s_pts[tt * 3 + 2];
            wdone = true;
#pragma unroll
            for (int q = 0; q < RP_BPW; ++q) {
                if (cnt[q] < S) {                           // (wave-uniform)
                    const bool in = ok && inside(px, py, pz, bk[q].cx, bk[q].cy, bk[q].cz, bk[q].hl, bk[q].hw, bk[q].hh, bk[q].c, bk[q].s);
                    const unsigned long long m = __ballot(in);
                    const int slot = cnt[q] + __builtin_popcountll(m & ((1ull << lane) - 1ull));
                    if (in && slot < S) s_sel[(wave * bpw + q) * S + slot] = base + t;
                    cnt[q] += __builtin_popcountll(m);
                }
                wdone = wdone && cnt[q] >= S;
            }
        }
        if (__syncthreads_and(wdone)) break;                // every box of the workgroup holds S points
    }
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < RP_BPW; ++q)
            if (q < nbw) s_cnt[wave * bpw + q] = min(cnt[q], S);
    }
    __syncthreads();
    // cyclic fill of slots cnt .. S-1, the empty flags and the optional index output
    for (int r = threadIdx.x; r < nb * S; r += RP_THREADS) {
        const int lb = r / S, s = r - lb * S;
        const int c = s_cnt[lb];
        if (s >= c && c > 0) s_sel[r] = s_sel[lb * S + s % c];
    }
    if (threadIdx.x < nb) empty[(size_t)b * K + k0 + threadIdx.x] = s_cnt[threadIdx.x] == 0;
    __syncthreads();
    const size_t row0 = ((size_t)b * K + k0) * S;           // first output row of the workgroup
    if (idx) {
        for (int r = threadIdx.x; r < nb * S; r += RP_THREADS) idx[row0 + r] = s_cnt[r / S] > 0 ? s_sel[r] : 0;
    }
    // copy: element e = (row r, chunk q) of the workgroup's nb * S rows of W = 3 + C floats
    const int W = 3 + C;
    const int cpr = W / VEC;
    const float *fb = feat + (size_t)b * N * C;
    const int total = nb * S * cpr;
    for (int el = threadIdx.x; el < total; el += RP_THREADS) {
        const int r = el / cpr, q = el - r * cpr;
        const bool full = s_cnt[r / S] > 0;
        const int j = full ? s_sel[r] : 0;
        float v[VEC];
#pragma unroll
        for (int u = 0; u < VEC; ++u) {
            const int col = q * VEC + u;
            v[u] = !full ? 0.0f : (col < 3 ? pb[(size_t)j * 3 + col] : fb[(size_t)j * C + (col - 3)]);
        }
        float *o = pooled + (row0 + r) * W + (size_t)q * VEC;
        if constexpr (VEC == 4)
            *(float4 *)o = make_float4(v[0], v[1], v[2], v[3]);
        else
            *o = v[0];
    }
}

}  // namespace

SAD_API int sad_boxes_iou_f32(const float *a, const float *b, int B, int Ka, int Kb, int Da, int Db, int mode, float *iou,
                              sad_stream_t stream) {
    SAD_REQUIRE(a && b && iou, "sad_boxes_iou_f32: NULL pointer");
    SAD_REQUIRE(B >= 1 && Ka >= 1 && Kb >= 1, "sad_boxes_iou_f32: B, Ka and Kb must be >= 1");
    SAD_REQUIRE(Da >= 7 && Db >= 7, "sad_boxes_iou_f32: box rows need D >= 7 fields (got %d, %d)", Da, Db);
    SAD_REQUIRE(mode == SAD_IOU_BEV || mode == SAD_IOU_3D, "sad_boxes_iou_f32: mode must be 0 (BEV) or 1 (3-D), got %d", mode);
    SAD_REQUIRE(B <= 65535 && (Ka + IOU_TA - 1) / IOU_TA <= 65535, "sad_boxes_iou_f32: B or Ka too large");
    const dim3 grid((Kb + IOU_TB - 1) / IOU_TB, (Ka + IOU_TA - 1) / IOU_TA, B);
    hipLaunchKernelGGL(boxes_iou_kernel, grid, dim3(256), 0, (hipStream_t)stream, a, b, Ka, Kb, Da, Db, mode, iou);
    return sad::check_launch("sad_boxes_iou_f32");
}

SAD_API int sad_points_in_boxes_f32(const float *xyz, const float *boxes, int B, int N, int K, int D, int32_t *box_idx,
                                    sad_stream_t stream) {
    SAD_REQUIRE(xyz && boxes && box_idx, "sad_points_in_boxes_f32: NULL pointer");
    SAD_REQUIRE(B >= 1 && N >= 1 && K >= 1, "sad_points_in_boxes_f32: B, N and K must be >= 1");
    SAD_REQUIRE(D >= 7, "sad_points_in_boxes_f32: box rows need D >= 7 fields (got %d)", D);
    SAD_REQUIRE(B <= 65535, "sad_points_in_boxes_f32: B too large");
    const dim3 grid((N + PIB_THREADS - 1) / PIB_THREADS, B);
    hipLaunchKernelGGL(points_in_boxes_kernel, grid, dim3(PIB_THREADS), 0, (hipStream_t)stream, xyz, boxes, N, K, D, box_idx);
    return sad::check_launch("sad_points_in_boxes_f32");
}

SAD_API int sad_roipoint_pool3d_f32(const float *xyz, const float *feat, const float *boxes, int B, int N, int K, int D, int C,
                                    float extra_width, int S, float *pooled, int32_t *empty, int32_t *idx, sad_stream_t stream) {
    SAD_REQUIRE(xyz && boxes && pooled && empty, "sad_roipoint_pool3d_f32: NULL pointer");
    SAD_REQUIRE(C >= 0 && (C == 0 || feat), "sad_roipoint_pool3d_f32: C = %d needs a feature pointer (NULL only for C = 0)", C);
    SAD_REQUIRE(B >= 1 && N >= 1 && K >= 1, "sad_roipoint_pool3d_f32: B, N and K must be >= 1");
    SAD_REQUIRE(D >= 7, "sad_roipoint_pool3d_f32: box rows need D >= 7 fields (got %d)", D);
    SAD_REQUIRE(S >= 1, "sad_roipoint_pool3d_f32: S must be >= 1 (got %d)", S);
    if (S > RP_SEL_INTS) return sad::fail(SAD_EUNSUPPORTED, "sad_roipoint_pool3d_f32: S=%d > %d", S, RP_SEL_INTS);
    const int bpb = min(RP_THREADS / 64 * RP_BPW, RP_SEL_INTS / S);       // boxes per workgroup: 16 up to S = 512
    const int W = 3 + C;
    const bool vec = W % 4 == 0 && ((uintptr_t)pooled & 15) == 0;
    SAD_REQUIRE(B <= 65535 && (long long)bpb * S * (W / (vec ? 4 : 1)) < (1LL << 31) && (long long)N * C < (1LL << 31) &&
                    (long long)N * 3 < (1LL << 31),
                "sad_roipoint_pool3d_f32: sizes too large");
    const dim3 grid((K + bpb - 1) / bpb, B);
    const size_t lds = (size_t)bpb * S * sizeof(int);
    const hipStream_t st = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(roipoint_pool3d_kernel<4>, grid, dim3(RP_THREADS), lds, st, xyz, feat, boxes, N, K, D, C, extra_width, S,
                           bpb, pooled, empty, idx);
    else
        hipLaunchKernelGGL(roipoint_pool3d_kernel<1>, grid, dim3(RP_THREADS), lds, st, xyz, feat, boxes, N, K, D, C, extra_width, S,
                           bpb, pooled, empty, idx);
    return sad::check_launch("sad_roipoint_pool3d_f32");
}
