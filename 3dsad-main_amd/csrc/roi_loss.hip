// RoI head loss (SPEC.md §29): the two predictions of a second stage and the targets of roi_targets (§28.1), read where they are ->
// the per-scene losses (classification, regression, corner) and the gradient with respect to both predictions.  The RoI-head
// counterpart of dense_loss.hip (§27): same arithmetic rules, same normaliser, same sums, no float atomics.
//
// One launch, no workspace, no memset, no atomics on memory: grid B, one workgroup of 256 threads owns a scene; thread tid takes
// the slots tid, tid + 256, ... (at most four passes: S <= 1024).
//   counts      n_cls = #(cls_target >= 0), n_reg = #(reg_valid != 0): per thread, a wave count, the four wave counts through LDS.
//               The targets of the scene's slots stay in LDS for the passes.
//   a pass      the 7-column rows of 256 slots (rcnn_reg, reg_target, gt_local) are one contiguous run of the scene: they come
//               in through LDS in memory order, consecutive threads on consecutive words; the thread that owns a row reads it
//               at stride 7 (odd: no bank conflict), overwrites it with the row's gradients, and grad_reg, grad_corner and
//               per_roi leave the same way.  rcnn_cls / grad_cls are unit-stride and go direct; of a rois row only columns
//               3..5 are read, by the owner, at row stride D.
//   sums        per thread in ascending slot order, then block_sum (prims.h); thread 0 writes loss[b, :] and num[b, :].
// The corner loss is evaluated in the RoI's frame (corner distances do not change under the RoI's rotation and translation):
// no second decode, no sin / cos of the RoI; the eight corners are unrolled, the seven gradient sums stay in registers.
#include "box_geom.h"
#include <math.h>

namespace {

#include "prims.h"

constexpr int RL_THREADS = 256, RL_MAXS = 1024;

struct RoiL {
    const float *cls, *reg, *ct, *tgt, *rois, *gl;
    const int32_t *valid;
    float *loss;
    int32_t *num;
    float *gcls, *greg, *gcor, *per;
    int S, D, normalize;
    float beta, cw[7], scale[3];
};

// §29 regression of one row: r = predictions, t = targets -> the row's term and gradients
__device__ __forceinline__ float reg_row(const RoiL &p, const float *r, const float *t, float wq, float *g) {
    float l = 0.0f;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const float d = (r[j] - t[j]) * p.cw[j];
        float sg;
        const float lj = smooth_l1(d, p.beta, sg);
        g[j] = (sg * p.cw[j]) * wq;
        l = l + lj;
    }
    return l * wq;
}

// §29 corner loss of one row in the RoI's frame: t = residuals, an = the RoI's anchor, gt = gt_local -> the term and gradients
__device__ __forceinline__ float corner_row(const float *t, const RoiAnchor &an, const float *gt, float wq, float *g) {
    float d[6]; roi_decode_local(t, an, d);
    const float px = d[0], py = d[1], pz = d[2], pl = d[3], pw = d[4], ph = d[5];
    float sp, cp, sg, cg;
    sincos_r(t[6], sp, cp);
    sincos_r(gt[6], sg, cg);
    const float hl = 0.5f * pl, hw = 0.5f * pw, hh = 0.5f * ph;
    const float ghl = 0.5f * gt[3], ghw = 0.5f * gt[4], ghh = 0.5f * gt[5];
    constexpr float SX[8] = {1, 1, -1, -1, 1, 1, -1, -1}, SY[8] = {1, -1, -1, 1, 1, -1, -1, 1}, SZ[8] = {-1, -1, -1, -1, 1, 1, 1, 1};
    float sum = 0.0f, a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f, a4 = 0.0f, a5 = 0.0f, a6 = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float ox = SX[k] * hl, oy = SY[k] * hw, oz = SZ[k] * hh;
        float rx, ry, grx, gry;
        from_frame(ox, oy, cp, sp, rx, ry);
        const float X = rx + px, Y = ry + py, Z = oz + pz;
        const float gox = SX[k] * ghl, goy = SY[k] * ghw, goz = SZ[k] * ghh;
        from_frame(gox, goy, cg, sg, grx, gry);
        const float ex = X - (grx + gt[0]), ey = Y - (gry + gt[1]), ez = Z - (goz + gt[2]);
        const float fx = X - (gt[0] - grx), fy = Y - (gt[1] - gry);
        const float d0 = sqrtf(((ex * ex) + (ey * ey)) + (ez * ez));
        const float d1 = sqrtf(((fx * fx) + (fy * fy)) + (ez * ez));
        const bool flip = d1 < d0;                      // strict: a tie stays unflipped
        const float dist = flip ? d1 : d0, ux = flip ? fx : ex, uy = flip ? fy : ey;
        const bool quad = dist < 1.0f;
        sum = sum + (quad ? (0.5f * dist) * dist : dist - 0.5f);
        const float ax = quad ? ux : ux / dist, ay = quad ? uy : uy / dist, az = quad ? ez : ez / dist;
        a0 = a0 + (ax * an.dg);
        a1 = a1 + (ay * an.dg);
        a2 = a2 + (az * an.ha);
        a3 = a3 + (((ax * cp) + (ay * sp)) * ox);
        a4 = a4 + (((ay * cp) - (ax * sp)) * oy);
        a5 = a5 + (az * oz);
        a6 = a6 + ((ay * rx) - (ax * ry));
    }
    g[0] = (a0 * 0.125f) * wq; g[1] = (a1 * 0.125f) * wq; g[2] = (a2 * 0.125f) * wq; g[3] = (a3 * 0.125f) * wq;
    g[4] = (a4 * 0.125f) * wq; g[5] = (a5 * 0.125f) * wq; g[6] = (a6 * 0.125f) * wq;
    return (sum * 0.125f) * wq;
}

__global__ __launch_bounds__(RL_THREADS) void roi_loss_kernel(const RoiL p) {
    __shared__ float s_reg[RL_THREADS * 7];            // rcnn_reg rows in, grad_reg rows out
    __shared__ float s_tgt[RL_THREADS * 7];
    __shared__ float s_gl[RL_THREADS * 7];             // gt_local rows in, grad_corner rows out
    __shared__ float s_per[RL_THREADS * 3];
    __shared__ float s_ct[RL_MAXS];
    __shared__ int32_t s_valid[RL_MAXS];
    __shared__ int wsum[2][RL_THREADS / 64];
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const size_t row0 = (size_t)b * p.S;
    const bool corner = p.rois != nullptr;
    int nc = 0, nr = 0;
    for (int i = tid; i < p.S; i += RL_THREADS) {
        const float t = p.ct[row0 + i];
        const int32_t v = p.valid[row0 + i];
        s_ct[i] = t;
        s_valid[i] = v;
        nc += t >= 0.0f;
        nr += v != 0;
    }
    nc = wave_count(nc);
    nr = wave_count(nr);
    if ((tid & 63) == 0) { wsum[0][tid >> 6] = nc; wsum[1][tid >> 6] = nr; }
    __syncthreads();
    const int n_cls = wsum[0][0] + wsum[0][1] + wsum[0][2] + wsum[0][3], n_reg = wsum[1][0] + wsum[1][1] + wsum[1][2] + wsum[1][3];
    const float wq0 = norm_weight(p.scale[0], n_cls, p.normalize), wq1 = norm_weight(p.scale[1], n_reg, p.normalize),
                wq2 = norm_weight(p.scale[2], n_reg, p.normalize);
    float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f;
    for (int i0 = 0; i0 < p.S; i0 += RL_THREADS) {
        const int n = min(RL_THREADS, p.S - i0);
        const size_t w7 = (row0 + i0) * 7;
        __syncthreads();                                // the previous pass has left LDS
        for (int i = tid; i < n * 7; i += RL_THREADS) {
            s_reg[i] = p.reg[w7 + i];
            s_tgt[i] = p.tgt[w7 + i];
            if (corner) s_gl[i] = p.gl[w7 + i];
        }
        __syncthreads();
        if (tid < n) {
            const int slot = i0 + tid;
            // ---- classification
            const float x = p.cls[row0 + slot], t = s_ct[slot];
            float gx;
            const float l0 = bce_one(x, t, t >= 0.0f, wq0, gx);
            p.gcls[row0 + slot] = gx;
            // ---- regression and corners: valid rows only, results selected
            float l1 = 0.0f, l2 = 0.0f, g[7], gc[7];
#pragma unroll
            for (int j = 0; j < 7; ++j) { g[j] = 0.0f; gc[j] = 0.0f; }
            if (s_valid[slot] != 0) {
                float r[7], tg[7];
#pragma unroll
                for (int j = 0; j < 7; ++j) { r[j] = s_reg[tid * 7 + j]; tg[j] = s_tgt[tid * 7 + j]; }
                l1 = reg_row(p, r, tg, wq1, g);
                if (corner) {
                    float gt[7];
#pragma unroll
                    for (int j = 0; j < 7; ++j) gt[j] = s_gl[tid * 7 + j];
                    l2 = corner_row(r, roi_anchor(p.rois + (row0 + slot) * p.D), gt, wq2, gc);
                }
            }
#pragma unroll
            for (int j = 0; j < 7; ++j) { s_reg[tid * 7 + j] = g[j]; s_gl[tid * 7 + j] = gc[j]; }
            s_per[tid * 3] = l0; s_per[tid * 3 + 1] = l1; s_per[tid * 3 + 2] = l2;
            acc0 = acc0 + l0; acc1 = acc1 + l1; acc2 = acc2 + l2;
        }
        __syncthreads();
        for (int i = tid; i < n * 7; i += RL_THREADS) {
            p.greg[w7 + i] = s_reg[i];
            if (corner) p.gcor[w7 + i] = s_gl[i];
        }
        if (p.per)
            for (int i = tid; i < n * 3; i += RL_THREADS) p.per[(row0 + i0) * 3 + i] = s_per[i];
    }
    const float s0 = block_sum(acc0, red), s1 = block_sum(acc1, red), s2 = block_sum(acc2, red);
    if (tid == 0) {
        p.loss[(size_t)b * 3] = s0; p.loss[(size_t)b * 3 + 1] = s1; p.loss[(size_t)b * 3 + 2] = s2;
        p.num[(size_t)b * 2] = n_cls; p.num[(size_t)b * 2 + 1] = n_reg;
    }
}

}  // namespace

SAD_API int sad_roi_head_loss_f32(const sad_roi_head_loss_args *a, sad_stream_t stream) {
    const char *fn = "sad_roi_head_loss_f32";
    if (int rc = args_ok(fn, a)) return rc;
    SAD_REQUIRE(a->rcnn_cls && a->rcnn_reg && a->cls_target && a->reg_valid && a->reg_target && a->loss && a->num && a->grad_cls && a->grad_reg,
                "%s: NULL pointer", fn);
    SAD_REQUIRE(a->B >= 1 && a->S >= 1, "%s: need B, S >= 1 (got %d, %d)", fn, a->B, a->S);
    SAD_REQUIRE((a->rois == nullptr) == (a->gt_local == nullptr), "%s: rois and gt_local must be given together (the corner component)", fn);
    SAD_REQUIRE((a->rois == nullptr) == (a->grad_corner == nullptr), "%s: grad_corner must be given iff rois and gt_local are", fn);
    SAD_REQUIRE(a->rois == nullptr || a->D >= 7, "%s: rois rows have D = %d columns (need D >= 7)", fn, a->D);
    SAD_REQUIRE(a->beta > 0.0f, "%s: need beta > 0 (got %g)", fn, (double)a->beta);
    if (a->B > 65535 || a->S > RL_MAXS) return sad::fail(SAD_EUNSUPPORTED, "%s: B = %d, S = %d (B <= 65535, S <= 1024 supported)", fn, a->B, a->S);
    RoiL p = {};
    p.cls = a->rcnn_cls; p.reg = a->rcnn_reg; p.ct = a->cls_target; p.valid = a->reg_valid; p.tgt = a->reg_target;
    p.rois = a->rois; p.gl = a->gt_local;
    p.loss = a->loss; p.num = a->num; p.gcls = a->grad_cls; p.greg = a->grad_reg; p.gcor = a->grad_corner; p.per = a->per_roi;
    p.S = a->S; p.D = a->D; p.normalize = a->normalize != 0; p.beta = a->beta;
    for (int j = 0; j < 7; ++j) p.cw[j] = a->code_weights[j];
    for (int i = 0; i < 3; ++i) p.scale[i] = a->scale[i];
    hipLaunchKernelGGL(roi_loss_kernel, dim3(a->B), dim3(RL_THREADS), 0, (hipStream_t)stream, p);
    return sad::check_launch(fn);
}
