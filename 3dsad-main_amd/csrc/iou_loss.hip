// Rotated IoU losses (SPEC.md §34): the IoU of ALIGNED pairs (pred[i] against target[i]) in bird's-eye view or 3-D, the IoU / DIoU
// loss on it and the analytic gradient with respect to the pred's seven columns, in one launch.  The value is §19.3's, from
// box_geom.h's helpers: iou equals the diagonal of boxes_iou_* bit for bit.
//
// The gradient does not differentiate the clip.  The target is fixed, so the intersection I changes only where the boundary of
// P ∩ T lies on an edge of P: dI = ∮ (v·n) ds over those pieces, and the normal velocity of P's boundary is linear along an edge.
// The edge pass clips each of P's four edges against T's closed rectangle in T's frame (Liang-Barsky, four half-planes, fully
// unrolled, registers only) -> the length inside and its midpoint; five sums of those give dI, the quotient rule the rest.
//
// One launch, one lane per pair, workgroups of 256; no workspace, no memset, no atomics, no barrier.  Rows are read and written
// by their owner at row stride D (7 or more words; not staged through LDS: at N <= 1e5 the launch is latency-bound and the rows
// are a few hundred kilobytes).  Every result is selected, never multiplied by a mask: NaN in a row of weight 0 reaches neither
// loss nor grad.
#include "box_geom.h"
#include <math.h>

namespace {

constexpr int IL_THREADS = 256, IL_COR = 17;           // 16 corner words per lane at an odd stride: no bank conflict

struct IouL {
    const float *pred, *tgt, *wt, *rois;
    float *loss, *iou, *grad, *dec;
    int N, Dp, Dt, Dr, mode, diou, roi;
};

// §34 one half-plane of the Liang-Barsky clip: q >= 0 is inside at t = 0, p the rate at which q is used up
__device__ __forceinline__ void lb_half(float p, float q, float &t0, float &t1, bool &ok) {
    const bool par = p == 0.0f;
    ok = ok && !(par && !(q >= 0.0f));
    const float r = q / p;
    t0 = (!par && p < 0.0f && r > t0) ? r : t0;
    t1 = (!par && p > 0.0f && r < t1) ? r : t1;
}

// the segment (X0,Y0)-(X1,Y1) against |X| <= hl, |Y| <= hw, closed -> f: the fraction inside, tm: the parameter of its midpoint
__device__ __forceinline__ void clip_edge(float X0, float Y0, float X1, float Y1, float hl, float hw, float &f, float &tm) {
    const float dX = X1 - X0, dY = Y1 - Y0;
    float t0 = 0.0f, t1 = 1.0f;
    bool ok = true;
    lb_half(-dX, X0 + hl, t0, t1, ok);
    lb_half(dX, hl - X0, t0, t1, ok);
    lb_half(-dY, Y0 + hw, t0, t1, ok);
    lb_half(dY, hw - Y0, t0, t1, ok);
    const float d = t1 - t0;
    const bool live = ok && d > 0.0f;
    f = live ? d : 0.0f;
    tm = live ? 0.5f * (t0 + t1) : 0.0f;
}

// derivative of a corner's X (Y) in the target's frame with respect to (x, y, l, w, yaw); sx, sy: half the corner's signs, 0: the target's
struct D5 { float x, y, l, w, t; };
__device__ __forceinline__ D5 corner_dX(float sx, float sy, float l, float w, float ct, float st, float cd, float sd) {
    const bool own = sx != 0.0f;
    const float a = sx * l, b = sy * w;
    D5 d;
    d.x = own ? ct : 0.0f;
    d.y = own ? st : 0.0f;
    d.l = own ? sx * cd : 0.0f;
    d.w = own ? -(sy * sd) : 0.0f;
    d.t = own ? -((a * sd) + (b * cd)) : 0.0f;
    return d;
}
__device__ __forceinline__ D5 corner_dY(float sx, float sy, float l, float w, float ct, float st, float cd, float sd) {
    const bool own = sx != 0.0f;
    const float a = sx * l, b = sy * w;
    D5 d;
    d.x = own ? -st : 0.0f;
    d.y = own ? ct : 0.0f;
    d.l = own ? sx * sd : 0.0f;
    d.w = own ? sy * cd : 0.0f;
    d.t = own ? (a * cd) - (b * sd) : 0.0f;
    return d;
}

__global__ __launch_bounds__(IL_THREADS) void iou_loss_kernel(const IouL p) {
    __shared__ float s_poly[4 * 10 * IL_THREADS];      // per-thread clipping scratch, thread-interleaved
    __shared__ float s_cor[IL_THREADS * IL_COR];       // per-thread corners: target x, y, pred x, y
    const int tid = threadIdx.x;
    const size_t i = (size_t)blockIdx.x * IL_THREADS + tid;
    if (i >= (size_t)p.N) return;
    float P[7], T[7], jac[6] = {1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f};
    {
        const float *r = p.pred + i * p.Dp, *t = p.tgt + i * p.Dt;
#pragma unroll
        for (int j = 0; j < 7; ++j) { P[j] = r[j]; T[j] = t[j]; }
    }
    if (p.roi) {                                        // §34 code = roi: the box decoded in the RoI's frame, as §29's corner loss
        const RoiAnchor an = roi_anchor(p.rois + i * p.Dr);
        roi_decode_local(P, an, P);
        jac[0] = an.dg; jac[1] = an.dg; jac[2] = an.ha; jac[3] = P[3]; jac[4] = P[4]; jac[5] = P[5];
        if (p.dec) {
#pragma unroll
            for (int j = 0; j < 7; ++j) p.dec[i * 7 + j] = P[j];
        }
    }
    const float x = P[0], y = P[1], z = P[2], l = P[3], w = P[4], h = P[5];
    const float gz = T[2], gl = T[3], gw = T[4], gh = T[5];
    float sp, cp, st, ct;
    sincos_r(P[6], sp, cp);
    sincos_r(T[6], st, ct);
    const float hl = 0.5f * l, hw = 0.5f * w, ghl = 0.5f * gl, ghw = 0.5f * gw;
    const float ddx = x - T[0], ddy = y - T[1];
    float cx[4], cy[4], tx[4], ty[4], X[4], Y[4];
    box_corners(P, cx, cy);
    box_corners(T, tx, ty);
    float *cor = s_cor + tid * IL_COR;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        cor[k] = tx[k]; cor[4 + k] = ty[k]; cor[8 + k] = cx[k]; cor[12 + k] = cy[k];
        to_frame(ddx + cx[k], ddy + cy[k], ct, st, X[k], Y[k]);
    }
    const float inter = poly_clip_area<IL_THREADS>(cor + 8, cor + 12, ddx, ddy, cor, cor + 4, s_poly + tid);
    // ---- edge pass: the length of each pred edge inside the target and the parameter of its midpoint
    float ln[4], tm[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float f;
        clip_edge(X[k], Y[k], X[(k + 1) & 3], Y[(k + 1) & 3], ghl, ghw, f, tm[k]);
        ln[k] = f * ((k & 1) ? w : l);
    }
    const float ea = ln[3] - ln[1], eb = ln[0] - ln[2];
    const float dIx = (cp * ea) - (sp * eb), dIy = (cp * eb) + (sp * ea);
    const float dIl = 0.5f * (ln[1] + ln[3]), dIw = 0.5f * (ln[0] + ln[2]);
    const float u0 = hl - (tm[0] * l), v1 = hw - (tm[1] * w), u2 = (tm[2] * l) - hl, v3 = (tm[3] * w) - hw;
    const float dIt = ((ln[0] * u0) + (ln[1] * v1)) - ((ln[2] * u2) + (ln[3] * v3));
    // ---- the IoU of §19.3 and the quotient rule
    float iou, nx, ny, nz, nl, nw, nh, nt, S, den;
    bool live;
    float topP = 0.0f, topT = 0.0f, botP = 0.0f, botT = 0.0f;
    if (p.mode == SAD_IOU_BEV) {
        iou = iou_of(inter, l * w, gl * gw, S, den);
        live = inter > 0.0f && den > 0.0f;
        nx = dIx * S; ny = dIy * S; nz = 0.0f; nh = 0.0f; nt = dIt * S;
        nl = (dIl * S) - (inter * w);
        nw = (dIw * S) - (inter * l);
    } else {
        const float oh = height_overlap(h, gh, z, gz, topP, topT, botP, botT);
        const float i3 = inter * oh;
        iou = iou_of(i3, (l * w) * h, (gl * gw) * gh, S, den);
        live = inter > 0.0f && oh > 0.0f && den > 0.0f;
        const float tp = topP < topT ? 1.0f : 0.0f, bp = botP > botT ? 1.0f : 0.0f;      // a tie is the target's
        nx = (dIx * oh) * S; ny = (dIy * oh) * S; nt = (dIt * oh) * S;
        nz = (inter * (tp - bp)) * S;
        nl = ((dIl * oh) * S) - (i3 * (w * h));
        nw = ((dIw * oh) * S) - (i3 * (l * h));
        nh = ((inter * (0.5f * (tp + bp))) * S) - (i3 * (l * w));
    }
    const float den2 = den * den;
    float g[7];
    g[0] = live ? -(nx / den2) : 0.0f; g[1] = live ? -(ny / den2) : 0.0f; g[2] = live ? -(nz / den2) : 0.0f;
    g[3] = live ? -(nl / den2) : 0.0f; g[4] = live ? -(nw / den2) : 0.0f; g[5] = live ? -(nh / den2) : 0.0f;
    g[6] = live ? -(nt / den2) : 0.0f;
    float loss = 1.0f - iou;
    if (p.diou) {
        // ---- the box aligned with the target's axes around both footprints: a tie goes to the lowest corner, then to the target
        constexpr float SXH[4] = {0.5f, -0.5f, -0.5f, 0.5f}, SYH[4] = {0.5f, 0.5f, -0.5f, -0.5f};
        float rho2 = (ddx * ddx) + (ddy * ddy);
        float e0 = ghl, e1 = -ghl, e2 = ghw, e3 = -ghw;
        float sx0 = 0.0f, sy0 = 0.0f, sx1 = 0.0f, sy1 = 0.0f, sx2 = 0.0f, sy2 = 0.0f, sx3 = 0.0f, sy3 = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (X[k] > e0) { e0 = X[k]; sx0 = SXH[k]; sy0 = SYH[k]; }
            if (X[k] < e1) { e1 = X[k]; sx1 = SXH[k]; sy1 = SYH[k]; }
            if (Y[k] > e2) { e2 = Y[k]; sx2 = SXH[k]; sy2 = SYH[k]; }
            if (Y[k] < e3) { e3 = Y[k]; sx3 = SXH[k]; sy3 = SYH[k]; }
        }
        const float cw = e0 - e1, ch = e2 - e3;
        float c2 = (cw * cw) + (ch * ch);
        const float cd = (cp * ct) + (sp * st), sd = (sp * ct) - (cp * st);
        const D5 a1 = corner_dX(sx0, sy0, l, w, ct, st, cd, sd), a0 = corner_dX(sx1, sy1, l, w, ct, st, cd, sd);
        const D5 b1 = corner_dY(sx2, sy2, l, w, ct, st, cd, sd), b0 = corner_dY(sx3, sy3, l, w, ct, st, cd, sd);
        float dc[7], dr[7];
        dc[0] = 2.0f * ((cw * (a1.x - a0.x)) + (ch * (b1.x - b0.x)));
        dc[1] = 2.0f * ((cw * (a1.y - a0.y)) + (ch * (b1.y - b0.y)));
        dc[3] = 2.0f * ((cw * (a1.l - a0.l)) + (ch * (b1.l - b0.l)));
        dc[4] = 2.0f * ((cw * (a1.w - a0.w)) + (ch * (b1.w - b0.w)));
        dc[6] = 2.0f * ((cw * (a1.t - a0.t)) + (ch * (b1.t - b0.t)));
        dc[2] = 0.0f; dc[5] = 0.0f;
        dr[0] = 2.0f * ddx; dr[1] = 2.0f * ddy; dr[2] = 0.0f; dr[3] = 0.0f; dr[4] = 0.0f; dr[5] = 0.0f; dr[6] = 0.0f;
        if (p.mode != SAD_IOU_BEV) {
            const float ddz = z - gz;
            rho2 = rho2 + (ddz * ddz);
            const float cz = fmaxf(topP, topT) - fminf(botP, botT);
            c2 = c2 + (cz * cz);
            const float tpz = topP > topT ? 1.0f : 0.0f, bpz = botP < botT ? 1.0f : 0.0f;
            dc[2] = 2.0f * (cz * (tpz - bpz));
            dc[5] = 2.0f * (cz * (0.5f * (tpz + bpz)));
            dr[2] = 2.0f * ddz;
        }
        const bool okc = c2 > 0.0f;
        loss = loss + (okc ? rho2 / c2 : 0.0f);
        const float c4 = c2 * c2;
#pragma unroll
        for (int j = 0; j < 7; ++j) g[j] = g[j] + (okc ? ((dr[j] * c2) - (rho2 * dc[j])) / c4 : 0.0f);
    }
    // ---- weight, the decode's Jacobian, and the selection that keeps a row of weight 0 out of every result
    bool on = true;
    if (p.wt) {
        const float wv = p.wt[i];
        on = wv != 0.0f;
        loss = loss * wv;
#pragma unroll
        for (int j = 0; j < 7; ++j) g[j] = g[j] * wv;
    }
    if (p.roi) {
#pragma unroll
        for (int j = 0; j < 6; ++j) g[j] = g[j] * jac[j];
    }
    p.loss[i] = on ? loss : 0.0f;
    p.iou[i] = iou;
    if (p.grad) {
#pragma unroll
        for (int j = 0; j < 7; ++j) p.grad[i * 7 + j] = on ? g[j] : 0.0f;
    }
}

}  // namespace

SAD_API int sad_rotated_iou_loss_f32(const sad_rotated_iou_loss_args *a, sad_stream_t stream) {
    const char *fn = "sad_rotated_iou_loss_f32";
    if (int rc = args_ok(fn, a)) return rc;
    SAD_REQUIRE(a->pred && a->target && a->loss && a->iou, "%s: NULL pointer", fn);
    SAD_REQUIRE(a->N >= 1, "%s: need N >= 1 (got %d)", fn, a->N);
    SAD_REQUIRE(a->Dp >= 7 && a->Dt >= 7, "%s: box rows have D = %d, %d columns (need D >= 7)", fn, a->Dp, a->Dt);
    SAD_REQUIRE(a->mode == SAD_IOU_BEV || a->mode == SAD_IOU_3D, "%s: mode must be SAD_IOU_BEV or SAD_IOU_3D (got %d)", fn, a->mode);
    SAD_REQUIRE(a->kind == SAD_IOU_LOSS_IOU || a->kind == SAD_IOU_LOSS_DIOU, "%s: kind must be SAD_IOU_LOSS_IOU or SAD_IOU_LOSS_DIOU (got %d)", fn, a->kind);
    SAD_REQUIRE(a->code == SAD_IOU_CODE_BOX || a->code == SAD_IOU_CODE_ROI, "%s: code must be SAD_IOU_CODE_BOX or SAD_IOU_CODE_ROI (got %d)", fn, a->code);
    SAD_REQUIRE((a->rois != nullptr) == (a->code == SAD_IOU_CODE_ROI), "%s: rois must be given iff code is SAD_IOU_CODE_ROI", fn);
    SAD_REQUIRE(a->rois == nullptr || a->Dr >= 7, "%s: rois rows have D = %d columns (need D >= 7)", fn, a->Dr);
    SAD_REQUIRE(a->decoded == nullptr || a->code == SAD_IOU_CODE_ROI, "%s: decoded is an output of code SAD_IOU_CODE_ROI only", fn);
    SAD_REQUIRE((a->grad != nullptr) == (a->need_grad != 0), "%s: grad must be given iff need_grad is set", fn);
    IouL p = {};
    p.pred = a->pred; p.tgt = a->target; p.wt = a->weight; p.rois = a->rois;
    p.loss = a->loss; p.iou = a->iou; p.grad = a->grad; p.dec = a->decoded;
    p.N = a->N; p.Dp = a->Dp; p.Dt = a->Dt; p.Dr = a->Dr;
    p.mode = a->mode; p.diou = a->kind == SAD_IOU_LOSS_DIOU; p.roi = a->code == SAD_IOU_CODE_ROI;
    hipLaunchKernelGGL(iou_loss_kernel, dim3((unsigned)(((long long)a->N + IL_THREADS - 1) / IL_THREADS)), dim3(IL_THREADS), 0, (hipStream_t)stream, p);
    return sad::check_launch(fn);
}
