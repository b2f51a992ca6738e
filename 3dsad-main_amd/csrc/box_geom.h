// Rotated-box geometry of SPEC.md §13, §19.1, §19.3 and §28.1, ONE definition per formula, for every box kernel (DESIGN.md names the
// few sites that keep a written-out copy, and why).  Binary32, no contraction (-ffp-contract=off), one rounding per written
// operation: the CPU oracle and every kernel agree bit for bit.
#pragma once
#include "common.h"
#include <math.h>

namespace {

__device__ __forceinline__ void sincos_r(float th, float &s_out, float &c_out) {
    const float n = rintf(th * 0.63661975f);
    float r = th - n * 1.5703125f;
    r = r - n * 4.8375129699707031e-4f;
    r = r - n * 7.5497899548918861e-8f;
    const int q = ((int)n) & 3;
    const float r2 = r * r;
    float ps = -1.9515295891e-4f;
    ps = ps * r2; ps = ps + 8.3321608736e-3f;
    ps = ps * r2; ps = ps + -1.6666654611e-1f;
    float S = r * r2; S = S * ps; S = r + S;
    float pc = 2.443315711809948e-5f;
    pc = pc * r2; pc = pc + -1.388731625493765e-3f;
    pc = pc * r2; pc = pc + 4.166664568298827e-2f;
    float C = r2 * r2; C = C * pc;
    const float h = 0.5f * r2;
    const float one = 1.0f - h;
    C = one + C;
    s_out = q == 0 ? S : (q == 1 ? C : (q == 2 ? -S : -C));
    c_out = q == 0 ? C : (q == 1 ? -S : (q == 2 ? -C : S));
}

// §13 a world offset into a box's frame (c, s: cos and sin of its yaw), and back
__device__ __forceinline__ void to_frame(float dx, float dy, float c, float s, float &lx, float &ly) {
    lx = (dx * c) + (dy * s);
    ly = (dy * c) - (dx * s);
}
__device__ __forceinline__ void from_frame(float lx, float ly, float c, float s, float &x, float &y) {
    x = (lx * c) - (ly * s);
    y = (lx * s) + (ly * c);
}

// §13 local corners: the four corner offsets of a box from its own centre, counter-clockwise.  The centre is not added: a pair
// is clipped in the frame of its second box (poly_clip_area), so the IoU does not depend on where the scene lies.
__device__ __forceinline__ void box_corners(const float *bx, float *ox, float *oy) {
    float s, c;
    sincos_r(bx[6], s, c);
    const float hl = 0.5f * bx[3], hw = 0.5f * bx[4];
    const float dx[4] = {hl, -hl, -hl, hl}, dy[4] = {hw, hw, -hw, -hw};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float a = c * dx[k], b = s * dy[k];
        ox[k] = a - b;
        a = s * dx[k]; b = c * dy[k];
        oy[k] = a + b;
    }
}

// §13 a box for the pair test: local corners, centre (x, y) and area, written where the caller keeps them
__device__ __forceinline__ void box_footprint(const float *bx, float *cx, float *cy, float *ctr, float &area) {
    float ox[4], oy[4];
    box_corners(bx, ox, oy);
#pragma unroll
    for (int k = 0; k < 4; ++k) { cx[k] = ox[k]; cy[k] = oy[k]; }
    ctr[0] = bx[0]; ctr[1] = bx[1];
    area = bx[3] * bx[4];
}
// §19.3 ... and z, height, volume
__device__ __forceinline__ void box_footprint3d(const float *bx, float *cx, float *cy, float *ctr, float &z, float &h, float &vol) {
    float area;
    box_footprint(bx, cx, cy, ctr, area);
    z = bx[2]; h = bx[5];
    vol = area * bx[5];
}

// §13 IoU from the intersection and the areas (§19.3: inter * oh and the volumes), by reference: the caller decides when they are
// read (pair_suppresses); sum and den go out for iou_loss.hip's gradient
__device__ __forceinline__ float iou_of(float inter, const float &a, const float &b, float &sum, float &den) {
    sum = a + b; den = sum - inter;
    return den > 0.0f ? inter / den : 0.0f;
}
__device__ __forceinline__ float iou_of(float inter, const float &a, const float &b) { float s, d; return iou_of(inter, a, b, s, d); }
// §19.3 the z overlap of two boxes (heights, then centres), clamped at 0; the tops and bottoms go out as well
__device__ __forceinline__ float height_overlap(float ha, float hb, float za, float zb, float &topa, float &topb, float &bota,
                                                float &botb) {
    const float hha = 0.5f * ha, hhb = 0.5f * hb;
    topa = za + hha; topb = zb + hhb; bota = za - hha; botb = zb - hhb;
    const float oh = fminf(topa, topb) - fmaxf(bota, botb);
    return oh > 0.0f ? oh : 0.0f;
}
__device__ __forceinline__ float height_overlap(float ha, float hb, float za, float zb) {
    float t[4];
    return height_overlap(ha, hb, za, zb, t[0], t[1], t[2], t[3]);
}

// §19.1 per-box constants of inside(p, box, e): centre, half extents of the enlarged box, cos, sin
struct BoxK { float cx, cy, cz, hl, hw, hh, c, s; };
__device__ __forceinline__ BoxK box_consts(const float *bx, float e) {
    BoxK k;
    float s, c;
    sincos_r(bx[6], s, c);
    const float e2 = 2.0f * e;
    const float L = bx[3] + e2, W = bx[4] + e2, H = bx[5] + e2;
    k.cx = bx[0]; k.cy = bx[1]; k.cz = bx[2];
    k.hl = 0.5f * L; k.hw = 0.5f * W; k.hh = 0.5f * H;
    k.c = c; k.s = s;
    return k;
}
// a ground-truth row that counts (§31.1, §35): a class in [0, C) and three positive extents
__device__ __forceinline__ bool gt_row_valid(int cls, int C, const float *r) {
    return cls >= 0 && cls < C && r[3] > 0.0f && r[4] > 0.0f && r[5] > 0.0f;
}

// §19.1 inside(p, box, e) on the box's constants
__device__ __forceinline__ bool inside(float px, float py, float pz, float cx, float cy, float cz, float hl, float hw,
                                       float hh, float c, float s) {
    const float dx = px - cx, dy = py - cy, dz = pz - cz;
    float lx, ly;
    to_frame(dx, dy, c, s, lx, ly);
    return fabsf(dz) <= hh && fabsf(lx) < hl && fabsf(ly) < hw;
}

// §28.1 the local anchor of a RoI: clamped extents and the diagonal
struct RoiAnchor { float la, wa, ha, dg; };
__device__ __forceinline__ RoiAnchor roi_anchor(const float *roi) {
    RoiAnchor a;
    a.la = fmaxf(roi[3], 1e-5f); a.wa = fmaxf(roi[4], 1e-5f); a.ha = fmaxf(roi[5], 1e-5f);
    a.dg = sqrtf((a.la * a.la) + (a.wa * a.wa));
    return a;
}
// §28.1 the residual code in the RoI's frame: t -> o[0 .. 5], centre and extents (o may be t); lv, the box in that frame -> tv
__device__ __forceinline__ void roi_decode_local(const float *t, const RoiAnchor &a, float *o) {
    o[0] = t[0] * a.dg; o[1] = t[1] * a.dg; o[2] = t[2] * a.ha;
    o[3] = expf(t[3]) * a.la; o[4] = expf(t[4]) * a.wa; o[5] = expf(t[5]) * a.ha;
}
__device__ __forceinline__ void roi_encode_local(const float *lv, const RoiAnchor &a, float *tv) {
    tv[0] = lv[0] / a.dg; tv[1] = lv[1] / a.dg; tv[2] = lv[2] / a.ha;
    tv[3] = logf(fmaxf(lv[3], 1e-5f) / a.la); tv[4] = logf(fmaxf(lv[4], 1e-5f) / a.wa); tv[5] = logf(fmaxf(lv[5], 1e-5f) / a.ha);
    tv[6] = lv[6];
}

// area of (box a) ∩ (box b) in b's frame: a's vertices are (ddx, ddy) + its local corners, with (ddx, ddy) = a.centre - b.centre
// (one rounding each, by the caller), b's vertices are its local corners; counter-clockwise; vertex lists live in LDS
// scratch vertex lists: element v of list L lives at sc[(L*10 + v) * STRIDE] (thread-interleaved LDS)
template <int STRIDE>
__device__ float poly_clip_area(const float *ax, const float *ay, float ddx, float ddy, const float *bxs, const float *bys,
                                float *sc) {
    // two vertex lists, A = lists 0/1 (x/y), B = lists 2/3; a pass reads one and writes the other (round 5: the copy back
    // and the integer modulo of the neighbour index are gone — same floating-point operations, same order, same results)
#define vx(L, i) sc[((L) * 20 + (i)) * STRIDE]
#define vy(L, i) sc[((L) * 20 + 10 + (i)) * STRIDE]
    int n = 4;
    int cur = 0;
    for (int i = 0; i < 4; ++i) { vx(0, i) = ddx + ax[i]; vy(0, i) = ddy + ay[i]; }
    for (int e = 0; e < 4 && n > 0; ++e) {
        const float q0x = bxs[e], q0y = bys[e], q1x = bxs[(e + 1) & 3], q1y = bys[(e + 1) & 3];
        const float ex = q1x - q0x, ey = q1y - q0y;
        const int nxt = cur ^ 1;
        int m = 0;
        // the previous vertex of vertex 0 is vertex n - 1; afterwards it is the vertex just visited (kept in registers)
        float ppx = vx(cur, n - 1), ppy = vy(cur, n - 1);
        float cp;
        {
            const float a = ppy - q0y, b = ppx - q0x;
            const float t1 = ex * a, t2 = ey * b;
            cp = t1 - t2;
        }
        for (int i = 0; i < n; ++i) {
            const float cxi = vx(cur, i), cyi = vy(cur, i);
            const float a = cyi - q0y, b = cxi - q0x;
            const float t1 = ex * a, t2 = ey * b;
            const float cc = t1 - t2;
            const bool in_c = cc >= 0.0f, in_p = cp >= 0.0f;
            if (in_c != in_p) {
                const float den = cp - cc;
                const float t = cp / den;
                float d = cxi - ppx;
                d = t * d;
                vx(nxt, m) = ppx + d;
                d = cyi - ppy;
                d = t * d;
                vy(nxt, m) = ppy + d;
                ++m;
            }
            if (in_c) { vx(nxt, m) = cxi; vy(nxt, m) = cyi; ++m; }
            ppx = cxi; ppy = cyi; cp = cc;
        }
        n = m;
        cur = nxt;
    }
    if (n < 3) return 0.0f;
    float sum = 0.0f;
    const float x0 = vx(cur, 0), y0 = vy(cur, 0);
    float xi = x0, yi = y0;
    for (int i = 0; i < n; ++i) {
        const bool last = i + 1 == n;
        const float xj = last ? x0 : vx(cur, last ? 0 : i + 1), yj = last ? y0 : vy(cur, last ? 0 : i + 1);
        const float t1 = xi * yj, t2 = xj * yi;
        const float d = t1 - t2;
        sum = sum + d;
        xi = xj; yi = yj;
    }
    sum = sum < 0.0f ? -sum : sum;
    return 0.5f * sum;
#undef vx
#undef vy
}

}  // namespace
