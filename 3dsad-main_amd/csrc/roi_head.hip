// RoI head targets and box codec (SPEC.md §28): the survivors of nms_boxes + padded ground truth -> the S sampled RoIs a
// second stage trains on, with their matched ground truth in the RoI's frame and the residual code; and the inverse of that
// code for inference.  The RoI-head counterpart of dense_head.hip (§25) + dense_target.hip (§26).
//
// roi_targets   two launches, no [R,G] matrix, nothing read back:
//   pass 1      grid (ceil(R / 16), B), 256 threads: 16 RoIs x 16 slices of the boxes.  The scene's boxes come through LDS in
//               chunks of GCH: local corners, centre, z, h, volume and label, 14 words per box, computed once per workgroup.  A thread clips
//               its RoI against the boxes of its slice that it is eligible for in ascending g with §19.3's helpers of box_geom.h
//               (poly_clip_area<256> in thread-interleaved LDS scratch): boxes_iou3d's value (tests/test_gpu_box_identities.py),
//               and keeps the maximum under a strict >; the 16 slices meet in LDS (largest m, lowest g among equals), so the
//               lowest g wins; (m, j) go to the workspace.
//   pass 2      one workgroup per scene.  Candidates r < n_b are classified (fg / hard / easy) by exact float compares and
//               compacted in ascending r by wave ballots + a scan over the four waves; the fg keys (h(b, r) << 32 | r) are
//               sorted by an LDS bitonic sort; then one thread per slot picks its candidate (all integer) and writes the
//               nine outputs.  A row beyond n_b is never read, in either pass.
// roi_decode    one elementwise launch, one thread per row.
#include "box_geom.h"
#include <math.h>

namespace {

#include "prims.h"

constexpr int ROI_MAXR = 4096, ROI_MAXS = 1024, ROI_MAXG = 1024;
constexpr int P1_ROIS = 16, P1_SLICES = 16; // pass 1: RoIs per workgroup x slices of the boxes
constexpr int P1_THREADS = P1_ROIS * P1_SLICES;
constexpr int GCH = P1_THREADS;            // pass 1: ground-truth boxes per LDS chunk (14 KB), one per thread
constexpr int P2_THREADS = 256;
constexpr unsigned DRAW_BASE = 0x80000000u;
constexpr float PI_F = 3.14159265358979323846f;
constexpr float TWO_PI_F = 6.283185307179586476925286766559f;
constexpr float HALF_PI_F = 1.57079632679489661923f;
constexpr float THREE_HALF_PI_F = 4.71238898038468985769f;

struct RoiP {
    const float *rois;
    const int32_t *roi_count, *roi_labels;
    const float *gt;
    const int32_t *gl;
    float *ws_m;            // [B,R] m(r)
    int32_t *ws_j;          // [B,R] j(r)
    int32_t *index, *match, *labels;
    float *iou, *cls_target;
    int32_t *reg_valid;
    float *rois_s, *gt_local, *reg_target;
    int R, D, G, Dg, S, fg_max, cls_mode;
    unsigned seed;
    float fg_thr, bg_lo, hard_ratio, reg_fg_thr, cls_fg_thr, cls_bg_thr;
};

// n_b: the candidates of scene b
__device__ __forceinline__ int roi_candidates(const RoiP &p, int b) {
    return p.roi_count ? min(max(p.roi_count[b], 0), p.R) : p.R;
}

// ---- pass 1 -------------------------------------------------------------------------------------------------------------
// A workgroup owns P1_ROIS RoIs x P1_SLICES slices of the boxes: thread = (RoI, slice), slice s takes the boxes t = s (mod P1_SLICES) of
// every chunk in ascending g, so a clip (a long serial chain through LDS) is one of ~G / 16 per thread and the pairs of a scene spread
// over ceil(R / 16) workgroups.  A thread steps from one box it is eligible for to the next, so the lanes of a wave clip together
// whatever their classes.  The slices' (m, j) meet in LDS: the largest m, the lowest j among equals, which is the lowest g overall.
__global__ __launch_bounds__(P1_THREADS) void roi_match_kernel(const RoiP p) {
    __shared__ float s_gx[GCH][4], s_gy[GCH][4], s_gc[GCH][2], s_gz[GCH], s_gh[GCH], s_gvol[GCH];
    __shared__ int s_glab[GCH];
    __shared__ float s_poly[4 * 10 * P1_THREADS];      // per-thread clipping scratch, thread-interleaved
    __shared__ float s_m[P1_THREADS];
    __shared__ int s_j[P1_THREADS];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int nb = roi_candidates(p, b);
    if ((int)blockIdx.x * P1_ROIS >= nb) return;       // (the whole workgroup: no candidate here)
    const int slice = tid / P1_ROIS;
    const int r = blockIdx.x * P1_ROIS + (tid - slice * P1_ROIS);
    const bool live = r < nb;
    float ax[4] = {0.f, 0.f, 0.f, 0.f}, ay[4] = {0.f, 0.f, 0.f, 0.f};
    float ac[2] = {0.f, 0.f}, az = 0.f, ah = 0.f, avol = 0.f;
    int alab = 0;
    if (live) {
        box_footprint3d(p.rois + ((size_t)b * p.R + r) * p.D, ax, ay, ac, az, ah, avol);
        if (p.roi_labels) alab = p.roi_labels[(size_t)b * p.R + r];
    }
    const bool any_class = p.roi_labels == nullptr;
    float m = 0.0f;
    int j = -1;
    for (int g0 = 0; g0 < p.G; g0 += GCH) {
        const int cnt = min(GCH, p.G - g0);
        __syncthreads();                                // the previous chunk is no longer read
        if (tid < cnt) {
            const int t = tid;
            const size_t row = (size_t)b * p.G + g0 + t;
            const int lab = p.gl[row];
            s_glab[t] = lab;
            if (lab >= 0) {                             // a padding row is never eligible: its fields are not read
                box_footprint3d(p.gt + row * p.Dg, s_gx[t], s_gy[t], s_gc[t], s_gz[t], s_gh[t], s_gvol[t]);
            }
        }
        __syncthreads();
        for (int t = live ? slice : cnt;; t += P1_SLICES) {
            for (; t < cnt; t += P1_SLICES) {           // on to the next box of the slice that this RoI is eligible for
                const int lab = s_glab[t];
                if (lab >= 0 && (any_class || lab == alab)) break;
            }
            if (t >= cnt) break;
            // §19.3, mode 3d, a = the RoI, b = the box
            const float inter = poly_clip_area<P1_THREADS>(ax, ay, ac[0] - s_gc[t][0], ac[1] - s_gc[t][1], s_gx[t], s_gy[t], s_poly + tid);
            const float oh = height_overlap(ah, s_gh[t], az, s_gz[t]);
            const float v = iou_of(inter * oh, avol, s_gvol[t]);
            if (j < 0 || v > m) { m = v; j = g0 + t; }  // strict: a tie stays with the lowest g of the slice
        }
    }
    s_m[tid] = m;
    s_j[tid] = j;
    __syncthreads();
    if (slice == 0 && live) {
#pragma unroll 1
        for (int q = 1; q < P1_SLICES; ++q) {
            const float mq = s_m[q * P1_ROIS + tid];
            const int jq = s_j[q * P1_ROIS + tid];
            if (jq >= 0 && (j < 0 || mq > m || (mq == m && jq < j))) { m = mq; j = jq; }
        }
        p.ws_m[(size_t)b * p.R + r] = m;
        p.ws_j[(size_t)b * p.R + r] = j;
    }
}

// ---- pass 2 -------------------------------------------------------------------------------------------------------------
// §28.1 heading of the box in the RoI's frame: into [-pi/2, pi/2], a box that faces backwards is flipped
__device__ __forceinline__ float local_heading(float gyaw, float rr) {
    const float dr = gyaw - rr;
    float o = dr - (floorf(dr / TWO_PI_F) * TWO_PI_F);
    if (o > HALF_PI_F && o < THREE_HALF_PI_F) {
        o = o + PI_F;
        o = o - (floorf(o / TWO_PI_F) * TWO_PI_F);
    }
    if (o > PI_F) o = o - TWO_PI_F;
    return fminf(fmaxf(o, -HALF_PI_F), HALF_PI_F);
}

__global__ __launch_bounds__(P2_THREADS) void roi_sample_kernel(const RoiP p) {
    __shared__ u64 keys[ROI_MAXR];                      // the fg keys, sorted (32 KB)
    __shared__ unsigned short fgl[ROI_MAXR];            // fg in ascending r
    __shared__ unsigned short bgl[ROI_MAXR];            // hard from the front, easy from the back, each in ascending r
    __shared__ int wcnt[3][P2_THREADS / 64];
    __shared__ int base[3];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nb_c = roi_candidates(p, b);
    const float *wm = p.ws_m + (size_t)b * p.R;
    const int32_t *wj = p.ws_j + (size_t)b * p.R;
    if (tid < 3) base[tid] = 0;
    __syncthreads();
    // classify and compact, P2_THREADS candidates at a time in ascending r
    for (int r0 = 0; r0 < nb_c; r0 += P2_THREADS) {
        const int r = r0 + tid;
        int c = -1;
        if (r < nb_c) {
            const float m = wm[r];
            c = m >= p.fg_thr ? 0 : (m >= p.bg_lo ? 1 : 2);
        }
        const u64 lower = (1ull << lane) - 1ull;
        u64 mine = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const u64 bal = __ballot(c == k);
            if (lane == 0) wcnt[k][wave] = __builtin_popcountll(bal);
            if (c == k) mine = bal;
        }
        __syncthreads();
        if (c >= 0) {
            int at = base[c] + __builtin_popcountll(mine & lower);
            for (int w = 0; w < wave; ++w) at += wcnt[c][w];
            if (c == 0) fgl[at] = (unsigned short)r;
            else if (c == 1) bgl[at] = (unsigned short)r;
            else bgl[ROI_MAXR - 1 - at] = (unsigned short)r;
        }
        __syncthreads();
        if (tid < 3) base[tid] += wcnt[tid][0] + wcnt[tid][1] + wcnt[tid][2] + wcnt[tid][3];
        __syncthreads();
    }
    const int n_fg = base[0], n_hard = base[1], n_easy = base[2], n_bg = n_hard + n_easy;
    const bool ranked = n_fg > 0 && n_bg > 0;
    int nf = n_fg == 0 ? 0 : p.S;
    if (ranked) {
        nf = min(min(p.fg_max, n_fg), p.S);
        // the (key(r), r) pairs of the fg class in ascending order: bitonic sort over the next power of two
        int P = 1;
        while (P < n_fg) P <<= 1;
        for (int t = tid; t < P; t += P2_THREADS) {
            const unsigned r = fgl[t < n_fg ? t : 0];
            keys[t] = t < n_fg ? ((u64)h17(p.seed, (unsigned)b, r) << 32) | r : ~0ull;
        }
        __syncthreads();
        for (int k = 2; k <= P; k <<= 1) {
            for (int jj = k >> 1; jj > 0; jj >>= 1) {
                for (int t = tid; t < P / 2; t += P2_THREADS) {
                    const int i = ((t & ~(jj - 1)) << 1) | (t & (jj - 1));
                    const u64 lo = keys[i], hi = keys[i + jj];
                    const bool asc = (i & k) == 0;
                    if ((lo > hi) == asc) { keys[i] = hi; keys[i + jj] = lo; }
                }
                __syncthreads();
            }
        }
    }
    const int nbg = p.S - nf;
    int nh = 0;                                         // bg slots that draw from hard
    if (n_hard > 0 && n_easy > 0) nh = min((int)floorf((float)nbg * p.hard_ratio), n_hard);
    else if (n_hard > 0) nh = nbg;
    const float d = p.cls_fg_thr - p.cls_bg_thr;
    for (int i = tid; i < p.S; i += P2_THREADS) {
        const size_t o = (size_t)b * p.S + i;
        float *rs = p.rois_s + o * 7, *gloc = p.gt_local + o * 7, *rt = p.reg_target + o * 7;
        if (nb_c == 0) {                                // an empty slot
            p.index[o] = -1; p.match[o] = -1; p.labels[o] = -1;
            p.iou[o] = 0.0f; p.cls_target[o] = -1.0f; p.reg_valid[o] = 0;
#pragma unroll
            for (int q = 0; q < 7; ++q) { rs[q] = 0.0f; gloc[q] = 0.0f; rt[q] = 0.0f; }
            continue;
        }
        const unsigned draw = h17(p.seed, (unsigned)b, DRAW_BASE + (unsigned)i);
        int r;
        if (i < nf) r = ranked ? (int)(unsigned)keys[i] : fgl[draw % (unsigned)n_fg];
        else if (i - nf < nh) r = bgl[draw % (unsigned)n_hard];
        else r = bgl[ROI_MAXR - 1 - (int)(draw % (unsigned)n_easy)];
        const float m = wm[r];
        const int j = wj[r];
        const float *roi = p.rois + ((size_t)b * p.R + r) * p.D;
        float rv[7];
#pragma unroll
        for (int q = 0; q < 7; ++q) rv[q] = roi[q];
        p.index[o] = r;
        p.match[o] = j;
        p.labels[o] = j >= 0 ? p.gl[(size_t)b * p.G + j] : -1;
        p.iou[o] = m;
        p.reg_valid[o] = (j >= 0 && m > p.reg_fg_thr) ? 1 : 0;
        float ct;
        if (m > p.cls_fg_thr) ct = 1.0f;
        else if (m < p.cls_bg_thr) ct = 0.0f;
        else ct = p.cls_mode == SAD_ROI_CLS_ROI_IOU ? (m - p.cls_bg_thr) / d : -1.0f;
        p.cls_target[o] = ct;
        float lv[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, tv[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (j >= 0) {
            const float *g = p.gt + ((size_t)b * p.G + j) * p.Dg;
            float s, c;
            sincos_r(rv[6], s, c);
            const float dx = g[0] - rv[0], dy = g[1] - rv[1], dz = g[2] - rv[2];
            to_frame(dx, dy, c, s, lv[0], lv[1]);
            lv[2] = dz; lv[3] = g[3]; lv[4] = g[4]; lv[5] = g[5];
            lv[6] = local_heading(g[6], rv[6]);
            roi_encode_local(lv, roi_anchor(rv), tv);
        }
#pragma unroll
        for (int q = 0; q < 7; ++q) { rs[q] = rv[q]; gloc[q] = lv[q]; rt[q] = tv[q]; }
    }
}

// ---- roi_decode -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void roi_decode_kernel(const float *__restrict__ rois, int D, const float *__restrict__ reg,
                                                         int rows, float *__restrict__ boxes) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    const float *roi = rois + (size_t)i * D, *t = reg + (size_t)i * 7;
    float *o = boxes + (size_t)i * 7;
    const RoiAnchor a = roi_anchor(roi);
    float s, c, d[6], x, y;
    sincos_r(roi[6], s, c);
    roi_decode_local(t, a, d);
    from_frame(d[0], d[1], c, s, x, y);
    o[0] = x + roi[0];
    o[1] = y + roi[1];
    o[2] = d[2] + roi[2];
    o[3] = d[3];
    o[4] = d[4];
    o[5] = d[5];
    o[6] = t[6] + roi[6];
}

}  // namespace

SAD_API size_t sad_roi_targets_workspace_bytes(int B, int R) {
    if (B < 1 || B > 65535 || R < 1 || R > ROI_MAXR) return 0;
    return (size_t)B * (size_t)R * 8;
}

SAD_API int sad_roi_targets_f32(const sad_roi_targets_args *a, sad_stream_t stream) {
    const char *fn = "sad_roi_targets_f32";
    if (int rc = args_ok(fn, a)) return rc;
    SAD_REQUIRE(a->rois && a->index && a->match && a->labels && a->iou && a->cls_target && a->reg_valid && a->rois_s && a->gt_local &&
                    a->reg_target, "%s: NULL pointer", fn);
    SAD_REQUIRE(a->B >= 1 && a->R >= 1 && a->S >= 1 && a->G >= 0, "%s: need B, R, S >= 1 and G >= 0 (got %d, %d, %d, %d)", fn, a->B, a->R,
                a->S, a->G);
    SAD_REQUIRE(a->D >= 7, "%s: rois rows have D = %d columns (need D >= 7)", fn, a->D);
    SAD_REQUIRE(a->G == 0 || a->Dg >= 7, "%s: gt_boxes rows have D = %d columns (need D >= 7)", fn, a->Dg);
    SAD_REQUIRE(a->G == 0 || (a->gt_boxes && a->gt_labels), "%s: NULL pointer (gt_boxes, gt_labels)", fn);
    SAD_REQUIRE(a->fg_max >= 0, "%s: need fg_max >= 0 (got %d)", fn, a->fg_max);
    SAD_REQUIRE(a->hard_ratio >= 0.0f && a->hard_ratio <= 1.0f, "%s: need 0 <= hard_ratio <= 1 (got %g)", fn, (double)a->hard_ratio);
    SAD_REQUIRE(a->bg_lo >= 0.0f && a->bg_lo <= a->fg_thr && a->fg_thr > 0.0f, "%s: need 0 <= bg_lo <= fg_thr and fg_thr > 0 (got %g, %g)", fn,
                (double)a->bg_lo, (double)a->fg_thr);
    SAD_REQUIRE(a->cls_bg_thr < a->cls_fg_thr, "%s: need cls_bg_thr < cls_fg_thr (got %g, %g)", fn, (double)a->cls_bg_thr, (double)a->cls_fg_thr);
    SAD_REQUIRE(a->reg_fg_thr == a->reg_fg_thr, "%s: reg_fg_thr is NaN", fn);
    SAD_REQUIRE(a->cls_mode == SAD_ROI_CLS_ROI_IOU || a->cls_mode == SAD_ROI_CLS_CLS, "%s: cls_mode must be SAD_ROI_CLS_ROI_IOU or SAD_ROI_CLS_CLS (got %d)",
                fn, a->cls_mode);
    if (a->B > 65535 || a->R > ROI_MAXR || a->S > ROI_MAXS || a->G > ROI_MAXG)
        return sad::fail(SAD_EUNSUPPORTED, "%s: B = %d, R = %d, S = %d, G = %d (B <= 65535, R <= 4096, S <= 1024, G <= 1024 supported)", fn, a->B,
                         a->R, a->S, a->G);
    SAD_REQUIRE(a->workspace, "%s: NULL workspace (sad_roi_targets_workspace_bytes(B, R) bytes)", fn);
    SAD_REQUIRE(((uintptr_t)a->workspace & 3) == 0, "%s: the workspace must be 4-byte aligned", fn);
    RoiP p = {};
    p.rois = a->rois; p.roi_count = a->roi_count; p.roi_labels = a->roi_labels; p.gt = a->gt_boxes; p.gl = a->gt_labels;
    p.ws_m = (float *)a->workspace;
    p.ws_j = (int32_t *)a->workspace + (size_t)a->B * a->R;
    p.index = a->index; p.match = a->match; p.labels = a->labels; p.iou = a->iou; p.cls_target = a->cls_target;
    p.reg_valid = a->reg_valid; p.rois_s = a->rois_s; p.gt_local = a->gt_local; p.reg_target = a->reg_target;
    p.R = a->R; p.D = a->D; p.G = a->G; p.Dg = a->Dg; p.S = a->S; p.fg_max = a->fg_max; p.cls_mode = a->cls_mode; p.seed = a->seed;
    p.fg_thr = a->fg_thr; p.bg_lo = a->bg_lo; p.hard_ratio = a->hard_ratio; p.reg_fg_thr = a->reg_fg_thr;
    p.cls_fg_thr = a->cls_fg_thr; p.cls_bg_thr = a->cls_bg_thr;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(roi_match_kernel, dim3((unsigned)((a->R + P1_ROIS - 1) / P1_ROIS), a->B), dim3(P1_THREADS), 0, st, p);
    if (int rc = sad::check_launch(fn)) return rc;
    hipLaunchKernelGGL(roi_sample_kernel, dim3(a->B), dim3(P2_THREADS), 0, st, p);
    return sad::check_launch(fn);
}

SAD_API int sad_roi_decode_f32(const float *rois, int D, const float *reg, int B, int S, float *boxes, sad_stream_t stream) {
    const char *fn = "sad_roi_decode_f32";
    SAD_REQUIRE(rois && reg && boxes, "%s: NULL pointer", fn);
    SAD_REQUIRE(B >= 1 && S >= 1, "%s: need B, S >= 1 (got %d, %d)", fn, B, S);
    SAD_REQUIRE(D >= 7, "%s: rois rows have D = %d columns (need D >= 7)", fn, D);
    if ((long long)B * S >= (1LL << 31)) return sad::fail(SAD_EUNSUPPORTED, "%s: B * S = %d * %d rows (B * S < 2^31 supported)", fn, B, S);
    const int rows = B * S;
    hipLaunchKernelGGL(roi_decode_kernel, dim3(sad::blocks_for((unsigned long long)rows, 256)), dim3(256), 0, (hipStream_t)stream, rois, D, reg,
                       rows, boxes);
    return sad::check_launch(fn);
}
