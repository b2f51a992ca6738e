// Rotated-box NMS in bird's-eye view for gfx950 (SPEC.md §13; SURVEY.md §8(f) row 1: the step right
// after the measured path).  No reference source exists (/root/reference/README.md:1-2).
//
// One workgroup per scene.  (1) rank the boxes by (score desc, index asc) with an O(K^2) counting
// rank (K <= 512, one box per thread); (2) thread p computes row p of the suppression matrix —
// bit q set iff IoU(rank p, rank q) > thr for q > p — with exact Sutherland-Hodgman clipping in
// binary32 (no contraction; sin/cos by the reproducible routine of SPEC §13, so the CPU oracle and
// this kernel make identical keep decisions); (3) one wave walks the ranking with 64-bit mask words.
// The ranking (rank_candidates), the pair test (pair_suppresses), the mask kernel, the decision chain of a chunk
// (chunk_decide) and the workspace view are nms_core.h's, shared with nms_select.hip.  Here: the LDS-resident matrix and
// walk of nms_bev_kernel, the corners of the ranked boxes, the nms_bev workspace law, and what the one-wave walk does
// with a chunk's kept mask.
#include "box_geom.h"

namespace {

#include "prims.h"       // u64, readlane_u64
#include "nms_core.h"

constexpr int NMS_MAXK = 512;
constexpr int NMS_WORDS = NMS_MAXK / 64;

template <int THREADS>
__global__ __launch_bounds__(THREADS) void nms_bev_kernel(const float *__restrict__ boxes, int K,
                                                          float iou_thr, float score_thr,
                                                          int32_t *__restrict__ keep,
                                                          int32_t *__restrict__ order,
                                                          int32_t *__restrict__ count) {
    __shared__ float s_cx[NMS_MAXK][4], s_cy[NMS_MAXK][4], s_ctr[NMS_MAXK][2], s_area[NMS_MAXK], s_score[NMS_MAXK];
    __shared__ int s_rank2idx[NMS_MAXK];
    __shared__ unsigned long long s_mask[NMS_MAXK][NMS_WORDS];
    __shared__ float s_poly[4 * 10 * THREADS];   // per-thread clipping scratch, thread-interleaved
    __shared__ int s_n;
    const int tid = threadIdx.x;
    const float *bx = boxes + (size_t)blockIdx.x * K * 9;
    int32_t *kp = keep + (size_t)blockIdx.x * K, *od = order + (size_t)blockIdx.x * K;

    // 1. rank among the candidates (score >= threshold): score descending, index ascending
    const int n = rank_candidates<THREADS>(bx, K, score_thr, kp, od, s_score, s_rank2idx, &s_n);
    // local corners, centres and areas in rank order (box_footprint, written out here and in nms_prep_kernel: DESIGN.md)
    for (int p = tid; p < n; p += THREADS) {
        const float *b = bx + (size_t)s_rank2idx[p] * 9;
        float cx[4], cy[4];
        box_corners(b, cx, cy);
#pragma unroll
        for (int k = 0; k < 4; ++k) { s_cx[p][k] = cx[k]; s_cy[p][k] = cy[k]; }
        s_ctr[p][0] = b[0]; s_ctr[p][1] = b[1];
        s_area[p] = b[3] * b[4];
    }
    __syncthreads();
    // 2. suppression matrix
    for (int p = tid; p < n; p += THREADS) {
        unsigned long long w[NMS_WORDS];
#pragma unroll
        for (int k = 0; k < NMS_WORDS; ++k) w[k] = 0ull;
        for (int q = p + 1; q < n; ++q) {
            if (pair_suppresses<THREADS>(s_cx[p], s_cy[p], s_ctr[p], s_area[p], s_cx[q], s_cy[q], s_ctr[q], s_area[q], iou_thr, s_poly + tid)) {
#pragma unroll
                for (int k = 0; k < NMS_WORDS; ++k)
                    if ((q >> 6) == k) w[k] |= 1ull << (q & 63);
            }
        }
#pragma unroll
        for (int k = 0; k < NMS_WORDS; ++k) s_mask[p][k] = w[k];
    }
    __syncthreads();
    // 3. walk the ranking (lanes 0..NMS_WORDS-1 of wave 0 hold one removed-word each)
    if (tid < 64) {
        unsigned long long removed = 0ull;
        int nk = 0;
        for (int p = 0; p < n; ++p) {
            const unsigned long long word = __shfl(removed, p >> 6, 64);
            if (!((word >> (p & 63)) & 1ull)) {            // wave-uniform
                if (tid == 0) {
                    const int i = s_rank2idx[p];
                    od[nk] = i;
                    kp[i] = 1;
                }
                ++nk;
                if (tid < NMS_WORDS) removed |= s_mask[p][tid];
            }
        }
        if (tid == 0) count[blockIdx.x] = nk;
    }
}

// ---- three-kernel variant (caller workspace): the K x K suppression matrix is spread over the chip --
// prep (one workgroup per scene): ranking, local corners, centres, areas -> workspace; mask (nms_core.h); walk (one
// wave per scene).  Same arithmetic as nms_bev_kernel, same keep decisions.
struct NmsBevLayout {     // per scene: [4] ints (n, pad), rank2idx [K], area [K], cx, cy [K][4], ctr [K][2], mask [K][NMS_WORDS]; no labels
    typedef NmsWs View;
    static constexpr bool LABELS = false;
    __host__ __device__ static size_t scene_bytes(int K) {
        return 16 + (size_t)K * 4 * 2 + (size_t)K * 16 * 2 + (size_t)K * 8 + (size_t)K * NMS_WORDS * 8;
    }
    __device__ __forceinline__ static View view(void *base, int scene, int K) {
        unsigned char *q = (unsigned char *)base + (size_t)scene * scene_bytes(K);
        View w;
        w.n = (int *)q; q += 16;
        w.rank2idx = (int *)q; q += (size_t)K * 4;
        w.area = (float *)q; q += (size_t)K * 4;
        w.cx = (float *)q; q += (size_t)K * 16;
        w.cy = (float *)q; q += (size_t)K * 16;
        w.ctr = (float *)q; q += (size_t)K * 8;
        w.mask = (u64 *)q;
        w.label = nullptr;
        w.W = NMS_WORDS;
        return w;
    }
};

__global__ __launch_bounds__(256) void nms_prep_kernel(const float *__restrict__ boxes, int K, float score_thr,
                                                       int32_t *__restrict__ keep, int32_t *__restrict__ order,
                                                       void *__restrict__ wsbase) {
    __shared__ float s_score[NMS_MAXK];
    __shared__ int s_rank2idx[NMS_MAXK];
    __shared__ int s_n;
    const int tid = threadIdx.x;
    const float *bx = boxes + (size_t)blockIdx.x * K * 9;
    int32_t *kp = keep + (size_t)blockIdx.x * K, *od = order + (size_t)blockIdx.x * K;
    const NmsWs w = NmsBevLayout::view(wsbase, blockIdx.x, K);
    const int n = rank_candidates<256>(bx, K, score_thr, kp, od, s_score, s_rank2idx, &s_n);
    if (tid == 0) w.n[0] = n;
    for (int p = tid; p < n; p += 256) {
        const int i = s_rank2idx[p];
        const float *b = bx + (size_t)i * 9;
        float cx[4], cy[4];
        box_corners(b, cx, cy);
#pragma unroll
        for (int k = 0; k < 4; ++k) { w.cx[p * 4 + k] = cx[k]; w.cy[p * 4 + k] = cy[k]; }
        w.ctr[p * 2] = b[0]; w.ctr[p * 2 + 1] = b[1];
        w.area[p] = b[3] * b[4];
        w.rank2idx[p] = i;
    }
}

// Greedy walk of the ranking, 64 ranks at a time (round 5; the first version took one dependent global load and one
// cross-lane read per kept box: 79 us for 32 scenes of 256 boxes).  Lane i of chunk c holds row p = 64c + i of the matrix.
// Inside a chunk the decision chain runs on a 64-bit scalar mask (who is still alive) and lane reads of the chunk's own
// word (chunk_decide, nms_core.h); what the chunk's kept boxes suppress in LATER chunks is or-ed into per-chunk words in LDS,
// each kept lane looping over its own row (at most NMS_WORDS - 1 words; nmsx_walk_kernel's four-wave form is for long rows).
// Same greedy rule: box p is kept iff no kept box of higher rank suppresses it.
__global__ __launch_bounds__(64) void nms_walk_kernel(int K, int32_t *__restrict__ keep, int32_t *__restrict__ order,
                                                      int32_t *__restrict__ count, void *__restrict__ wsbase) {
    __shared__ u64 s_rem[NMS_WORDS];
    const int lane = threadIdx.x;
    const NmsWs w = NmsBevLayout::view(wsbase, blockIdx.x, K);
    int32_t *kp = keep + (size_t)blockIdx.x * K, *od = order + (size_t)blockIdx.x * K;
    const int n = __builtin_amdgcn_readfirstlane(w.n[0]);          // (wave-uniform by construction: tell the compiler)
    const int nch = (n + 63) >> 6;
    if (lane < NMS_WORDS) s_rem[lane] = 0ull;
    __syncthreads();
    int nk = 0;
    for (int c = 0; c < nch; ++c) {                                  // (wave-uniform)
        const int p = 64 * c + lane;
        const bool have = p < n;
        const u64 own = have ? w.mask[(size_t)p * w.W + c] : 0ull;         // suppressed by p inside its chunk
        const int idx = have ? w.rank2idx[p] : 0;
        const u64 kept = chunk_decide(own, n, c, s_rem[c]);
        const bool mine = (kept >> lane) & 1ull;
        if (mine) {
            od[nk + __builtin_popcountll(kept & ((1ull << lane) - 1ull))] = idx;
            kp[idx] = 1;
            for (int k = c + 1; k < nch; ++k) {                      // later chunks: usually nothing
                const u64 wk = w.mask[(size_t)p * w.W + k];
                if (wk) atomicOr(&s_rem[k], wk);
            }
        }
        nk += __builtin_popcountll(kept);
        __syncthreads();                                             // (one wave: orders the LDS atomics before the next chunk's read)
    }
    if (lane == 0) count[blockIdx.x] = nk;
}

}  // namespace

SAD_API int sad_nms_bev_f32(const float *boxes, int B, int K, float iou_thr, float score_thr,
                            int32_t *keep, int32_t *order, int32_t *count, sad_stream_t stream) {
    SAD_REQUIRE(boxes && keep && order && count, "sad_nms_bev_f32: NULL pointer");
    SAD_REQUIRE(B >= 1 && K >= 1, "sad_nms_bev_f32: need B,K >= 1");
    if (K > NMS_MAXK) return sad::fail(SAD_EUNSUPPORTED, "sad_nms_bev_f32: K=%d > %d", K, NMS_MAXK);
    hipLaunchKernelGGL((nms_bev_kernel<256>), dim3(B), dim3(256), 0, (hipStream_t)stream, boxes, K, iou_thr,
                       score_thr, keep, order, count);
    return sad::check_launch("sad_nms_bev_f32");
}

SAD_API size_t sad_nms_bev_workspace_bytes(int B, int K) {
    if (B < 1 || K < 1 || K > NMS_MAXK) return 0;
    return (size_t)B * NmsBevLayout::scene_bytes(K);
}

SAD_API int sad_nms_bev_ws_f32(const float *boxes, int B, int K, float iou_thr, float score_thr,
                               int32_t *keep, int32_t *order, int32_t *count, void *workspace, sad_stream_t stream) {
    SAD_REQUIRE(boxes && keep && order && count && workspace, "sad_nms_bev_ws_f32: NULL pointer");
    SAD_REQUIRE(B >= 1 && B <= 65535 && K >= 1, "sad_nms_bev_ws_f32: need 1 <= B <= 65535, K >= 1");
    SAD_REQUIRE((uintptr_t)workspace % 16 == 0, "sad_nms_bev_ws_f32: workspace must be 16-byte aligned");
    if (K > NMS_MAXK) return sad::fail(SAD_EUNSUPPORTED, "sad_nms_bev_ws_f32: K=%d > %d", K, NMS_MAXK);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(nms_prep_kernel, dim3(B), dim3(256), 0, st, boxes, K, score_thr, keep, order, workspace);
    hipLaunchKernelGGL(nms_mask_kernel<NmsBevLayout>, dim3((K + NMS_ROWS_PER_WG - 1) / NMS_ROWS_PER_WG, B), dim3(256), 0, st, K, iou_thr, 0, workspace);
    hipLaunchKernelGGL(nms_walk_kernel, dim3(B), dim3(64), 0, st, K, keep, order, count, workspace);
    return sad::check_launch("sad_nms_bev_ws_f32");
}
