// Rotated-box geometry of SPEC.md §13, shared by the NMS kernels (nms.hip), the box operators (boxes.hip) and the RoI head
// (roi_head.hip, roi_loss.hip): the reproducible sin/cos, the box corners, the Sutherland-Hodgman clipped area and the RoI's local anchor.  Binary32, no contraction
// (the library is built with -ffp-contract=off), so the CPU oracle and every kernel agree bit for bit.
#pragma once
#include "common.h"

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

// §19.1 inside(p, box, e) on the box's constants: centre, half extents of the enlarged box, cos, sin (boxes.hip, point_head.hip)
__device__ __forceinline__ bool inside(float px, float py, float pz, float cx, float cy, float cz, float hl, float hw,
                                       float hh, float c, float s) {
    const float dx = px - cx, dy = py - cy, dz = pz - cz;
    const float a = dx * c, b = dy * s;
    const float lx = a + b;
    const float a2 = dy * c, b2 = dx * s;
    const float ly = a2 - b2;
    return fabsf(dz) <= hh && fabsf(lx) < hl && fabsf(ly) < hw;
}

// §28.1 the local anchor of a RoI: clamped extents and the diagonal
struct RoiAnchor { float la, wa, ha, dg; };
__device__ __forceinline__ RoiAnchor roi_anchor(const float *roi) {
    RoiAnchor a;
    a.la = fmaxf(roi[3], 1e-5f);
    a.wa = fmaxf(roi[4], 1e-5f);
    a.ha = fmaxf(roi[5], 1e-5f);
    a.dg = sqrtf((a.la * a.la) + (a.wa * a.wa));
    return a;
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
