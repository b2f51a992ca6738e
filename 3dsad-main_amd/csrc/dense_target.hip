// Dense head target assignment (SPEC.md §26): ground-truth boxes -> what an anchor head / a centre head is trained
// against.  The inverse of dense_head.hip: same anchor scalars, same K, same k numbering, same tiles (dense_tile.h).
//
// anchor targets  two passes over the anchors, neither of which materialises an anchor or a [K,G] IoU matrix.  A workgroup owns
//                 an anchor tile (dense_tile.h) and holds the scene's G <= 1024 nearest-BEV rectangles and labels in LDS (5 words per box).
//   pass 1        best[b,g] = max over the anchors g is eligible for of iou(k,g).  A thread walks the boxes for its anchors
//                 (the LDS reads are broadcasts); where a box meets a cell of the wave, the wave reduces its 64 IoUs and
//                 one lane folds the result into the workgroup's value by an LDS atomicMax on the float's bit pattern
//                 (IoUs are >= 0: unsigned order is float order); a workgroup issues one global atomicMax per box it met.
//                 A maximum does not depend on the order of its operands, so best is exact and the same in every run.
//   cull          both passes first mark, in a 1024-bit LDS mask, the boxes whose rectangle can meet the tile at all
//                 (cull_gts: conservative, so no output bit depends on it) and walk only those, in ascending g.
//   pass 2        recomputes the IoUs of a row with the SAME __device__ function on the SAME values, applies the rule,
//                 encodes, and stores the rows of the tile through an LDS image in memory order (flush_spans of §25).
//   The forced test is iou(k,g) == best[g] on two results of rect_iou.  The library is built with -ffp-contract=off and
//   every operation of rect_iou is one IEEE binary32 operation, so the two passes produce the same bits and == is safe.
// centre targets  gather form: a workgroup owns a 16 x 16 tile of cells, culls the scene's boxes against the tile (window
//                 meets tile) into an LDS list, and every thread takes, for each class plane, the maximum over the listed
//                 boxes: each element of the map is stored exactly once, no atomics on memory, no zero fill, either layout.
//                 The list's order varies from run to run; the maximum over it does not.  A second launch, one thread per
//                 box, writes ind and anno.
#include "box_geom.h"
#include <math.h>

namespace {

#include "dense_tile.h"

constexpr int MAXRAD = 64;
constexpr int CT = 16;             // a centre tile is CT x CT cells
constexpr float PI_F = 3.14159265358979323846f;
constexpr float PI4_F = 0.78539816339744830962f;
constexpr float TWO_PI_F = 6.283185307179586476925286766559f;
// tab = the anchor table (dense_tile.h) | pos_thr[16] | neg_thr[16] | size_class[16] (int bits)
constexpr int T_POS = T_N, T_NEG = T_N + 16, T_SC = T_N + 32, T_END = T_N + 48;

struct TgtP {
    const float *gt;
    const int32_t *gl;
    int32_t *labels, *match, *dir_target;
    float *reg, *max_iou;
    unsigned *best;
    int G, D, HW, A, nb, use_sc;
    int tiles, chunks;
    float dir_offset, period;
    AnchorTab tab;
    float pos[16], neg[16];
    int32_t sc[16];
};

struct CtrP {
    const float *gt;
    const int32_t *gl;
    float *hm;
    int32_t *ind;
    float *anno;
    int G, D, C, H, W, nhwc, min_radius, vel, tx;
    float lo_x, lo_y, sx, sy, mo;
};

// §26.1 the nearest-BEV rectangle of a box: (x0, x1, y0, y1)
__device__ __forceinline__ float4 nearest_rect(float cx, float cy, float l, float w, float yaw) {
    const float n = floorf((yaw / PI_F) + 0.5f);
    const float ang = fabsf(yaw - (n * PI_F));
    const bool keep = ang < PI4_F;
    const float ex = keep ? l : w, ey = keep ? w : l;
    const float hx = ex * 0.5f, hy = ey * 0.5f;
    return make_float4(cx - hx, cx + hx, cy - hy, cy + hy);
}

// §26.1 the IoU of two rectangles.  Both passes call this, and only this, on the same values.
__device__ __forceinline__ float rect_iou(const float4 a, const float4 g) {
    float ix = fminf(a.y, g.y) - fmaxf(a.x, g.x);
    ix = ix > 0.0f ? ix : 0.0f;
    float iy = fminf(a.w, g.w) - fmaxf(a.z, g.z);
    iy = iy > 0.0f ? iy : 0.0f;
    const float inter = ix * iy;
    const float area_a = (a.y - a.x) * (a.w - a.z);
    const float area_g = (g.y - g.x) * (g.w - g.z);
    const float den = fmaxf((area_a + area_g) - inter, 1e-6f);
    return inter / den;
}

// the anchor table and the per-size entries behind it -> LDS (the caller synchronises)
__device__ __forceinline__ void load_tabs(const TgtP &p, float *tab) {
    load_tab(p.tab, tab);
    const int t = threadIdx.x;
    if (t >= T_POS && t < T_END) tab[t] = t < T_NEG ? p.pos[t - T_POS] : t < T_SC ? p.neg[t - T_NEG] : __int_as_float(p.sc[t - T_SC]);
}

// the scene's rectangles and labels -> LDS (the caller synchronises)
__device__ __forceinline__ void load_gts(const TgtP &p, int b, float4 *grect, int *glab) {
    for (int g = threadIdx.x; g < p.G; g += DENSE_THREADS) {
        const float *r = p.gt + ((size_t)b * p.G + g) * p.D;
        grect[g] = nearest_rect(r[0], r[1], r[3], r[4], r[6]);
        glab[g] = p.gl[(size_t)b * p.G + g];
    }
}

__device__ __forceinline__ bool eligible(const TgtP &p, const float *tab, int s, int label) {
    return label >= 0 && (!p.use_sc || label == __float_as_int(tab[T_SC + s]));
}

// The cull: bit g of `mask` is set iff box g's rectangle can meet an anchor of the tile.  An IoU is > 0 only if the two
// rectangles overlap, and every anchor rectangle of the tile lies inside [xlo, xhi] x [ylo, yhi]: the anchor centres of the
// tile's first and last column / row are the extremes (x0 + x * sx is monotonic in x after rounding too), and subtracting the
// largest half extent of any size from the smallest centre rounds to no more than any anchor's own x0 (rounding is monotonic).
// A box that fails the test has IoU exactly 0 with every anchor of the tile, which is what leaving it out computes: best[]
// only takes values > 0, and pass 2 falls back to the lowest eligible box when a row met nothing (see anchor_assign_kernel).
// Bits are walked in ascending g, so ties still go to the lowest g.
__device__ __forceinline__ void cull_gts(const AnchorTab &p, int G, const float *tab, const float4 *grect, unsigned *mask, int cell0, int ncell) {
    const int y_first = cell0 / p.W, y_last = (cell0 + ncell - 1) / p.W;
    const int x_first = y_first == y_last ? cell0 - y_first * p.W : 0;
    const int x_last = y_first == y_last ? cell0 + ncell - 1 - y_first * p.W : p.W - 1;
    const float xa = p.x0 + ((float)x_first * p.sx), xb = p.x0 + ((float)x_last * p.sx);
    const float ya = p.y0 + ((float)y_first * p.sy), yb = p.y0 + ((float)y_last * p.sy);
    float half = 0.0f;
    for (int i = 0; i < 3 * 16; i += 3) half = fmaxf(half, fmaxf(tab[i], tab[i + 1]) * 0.5f);      // (unused sizes are 0)
    const float xlo = fminf(xa, xb) - half, xhi = fmaxf(xa, xb) + half;
    const float ylo = fminf(ya, yb) - half, yhi = fmaxf(ya, yb) + half;
    for (int w = threadIdx.x; w < MAXG / 32; w += DENSE_THREADS) mask[w] = 0u;
    __syncthreads();
    for (int g = threadIdx.x; g < G; g += DENSE_THREADS) {
        const float4 r = grect[g];
        if (r.y >= xlo && r.x <= xhi && r.w >= ylo && r.z <= yhi) atomicOr(&mask[g >> 5], 1u << (g & 31));
    }
    __syncthreads();
}

__global__ __launch_bounds__(DENSE_THREADS) void anchor_best_kernel(const TgtP p) {
    __shared__ float tab[T_END];
    __shared__ float4 grect[MAXG];
    __shared__ int glab[MAXG];
    __shared__ unsigned sbest[MAXG];
    __shared__ unsigned gmask[MAXG / 32];
    load_tabs(p, tab);
    const AnchorTile t = anchor_tile(p.chunks, p.HW, p.A);
    const int b = t.b, lane = t.lane;
    load_gts(p, b, grect, glab);
    for (int g = threadIdx.x; g < p.G; g += DENSE_THREADS) sbest[g] = 0u;
    __syncthreads();
    cull_gts(p.tab, p.G, tab, grect, gmask, t.cell0, t.ncell);
    for (int pass = 0; 4 * pass < t.acn; ++pass) {
        if (t.al(pass) >= t.acn) continue;                           // (the whole wave: one anchor per wave)
        const bool live = lane < t.ncell;
        const Anchor an = anchor_of(p.tab, tab, t.a0 + t.al(pass), t.cell0 + (live ? lane : 0));
        const float4 ar = nearest_rect(an.xa, an.ya, an.la, an.wa, an.ra);
        for (int w32 = 0; w32 * 32 < p.G; ++w32) {
            for (unsigned bits = gmask[w32]; bits; bits &= bits - 1) {       // (LDS broadcast: the same for the whole wave)
                const int g = w32 * 32 + __ffs(bits) - 1;
                if (!eligible(p, tab, an.s, glab[g])) continue;
                const float iou = live ? rect_iou(ar, grect[g]) : 0.0f;
                if (__ballot(iou > 0.0f) == 0ull) continue;
                float w = iou;
#pragma unroll
                for (int off = 32; off; off >>= 1) w = fmaxf(w, __shfl_xor(w, off));
                if (lane == 0) atomicMax(&sbest[g], __float_as_uint(w));
            }
        }
    }
    __syncthreads();
    for (int g = threadIdx.x; g < p.G; g += DENSE_THREADS)
        if (sbest[g]) atomicMax(&p.best[(size_t)b * p.G + g], sbest[g]);
}

__global__ __launch_bounds__(DENSE_THREADS) void anchor_assign_kernel(const TgtP p) {
    __shared__ float tab[T_END];
    __shared__ float4 grect[MAXG];
    __shared__ int glab[MAXG];
    __shared__ float gbest[MAXG];
    __shared__ float oreg[TC * AC * 7];
    __shared__ float omax[TC * AC];
    __shared__ int32_t olabel[TC * AC];
    __shared__ int32_t omatch[TC * AC];
    __shared__ int32_t odir[TC * AC];
    __shared__ unsigned gmask[MAXG / 32];
    __shared__ int first[16];
    load_tabs(p, tab);
    const AnchorTile t = anchor_tile(p.chunks, p.HW, p.A);
    load_gts(p, t.b, grect, glab);
    for (int g = threadIdx.x; g < p.G; g += DENSE_THREADS) gbest[g] = __uint_as_float(p.best[(size_t)t.b * p.G + g]);
    if (threadIdx.x < 16) first[threadIdx.x] = MAXG;
    __syncthreads();
    // first[s] = the lowest box eligible for size s: j of a row that meets no box (every IoU 0: the lowest eligible g attains it)
    for (int i = threadIdx.x; i < p.G * 16; i += DENSE_THREADS) {
        const int g = i >> 4, sz = i & 15;
        if (sz * p.tab.nr < p.A && eligible(p, tab, sz, glab[g])) atomicMin(&first[sz], g);
    }
    cull_gts(p.tab, p.G, tab, grect, gmask, t.cell0, t.ncell);
    for (int pass = 0; 4 * pass < t.acn; ++pass) {
        if (!t.active(pass)) continue;
        const Anchor an = anchor_of(p.tab, tab, t.a0 + t.al(pass), t.cell0 + t.lane);
        const float4 ar = nearest_rect(an.xa, an.ya, an.la, an.wa, an.ra);
        float m = 0.0f;
        int j = -1;
        bool forced = false;
        for (int w32 = 0; w32 * 32 < p.G; ++w32) {
            for (unsigned bits = gmask[w32]; bits; bits &= bits - 1) {
                const int g = w32 * 32 + __ffs(bits) - 1;
                if (!eligible(p, tab, an.s, glab[g])) continue;
                const float iou = rect_iou(ar, grect[g]);
                if (iou > m) { m = iou; j = g; }                     // strict: a tie stays with the lowest g
                const float bg = gbest[g];
                forced = forced || (bg > 0.0f && iou == bg);
            }
        }
        if (j < 0 && first[an.s] < MAXG) j = first[an.s];            // every IoU of the row is 0: m = 0 at the lowest eligible box
        const bool positive = forced || (j >= 0 && m >= tab[T_POS + an.s]);
        float res[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        int label, match = -1, bin = -1;
        if (positive) {
            residual_encode(an, p.gt + ((size_t)t.b * p.G + j) * p.D, res);
            label = glab[j];
            match = j;
            if (p.nb) {
                const float rg = res[6] + an.ra;
                const float v = rg - p.dir_offset;
                const float o = v - (floorf(v / TWO_PI_F) * TWO_PI_F);
                bin = (int)floorf(o / p.period);
                bin = min(max(bin, 0), p.nb - 1);
            }
        } else {
            label = (j < 0 || m < tab[T_NEG + an.s]) ? -1 : -2;
        }
        const int slot = t.slot(pass);
#pragma unroll
        for (int q = 0; q < 7; ++q) oreg[slot * 7 + q] = res[q];
        omax[slot] = m;
        olabel[slot] = label;
        omatch[slot] = match;
        odir[slot] = bin;
    }
    __syncthreads();
    t.store(oreg, p.reg, 7);
    t.store(omax, p.max_iou, 1);
    t.store(olabel, p.labels, 1);
    t.store(omatch, p.match, 1);
    if (p.nb) t.store(odir, p.dir_target, 1);
}

// §26.2: one box.  false: unassigned
struct CBox {
    float fx, fy, den;
    int ix, iy, rad;
};

__device__ __forceinline__ bool center_box(const CtrP &p, const float *r, int label, CBox &o) {
    if (label < 0 || label >= p.C) return false;
    o.fx = (r[0] - p.lo_x) / p.sx;
    o.fy = (r[1] - p.lo_y) / p.sy;
    const float wr = r[3] / p.sx, hr = r[4] / p.sy;
    if (wr <= 0.0f || hr <= 0.0f) return false;
    if (!(o.fx >= 0.0f && o.fx < (float)p.W && o.fy >= 0.0f && o.fy < (float)p.H)) return false;
    o.ix = (int)floorf(o.fx);
    o.iy = (int)floorf(o.fy);
    // CenterNet's gaussian_radius((height, width) = (hr, wr), min_overlap), its three roots in the source's order
    const float mo = p.mo;
    const float hw = hr + wr;
    const float area = wr * hr;
    const float c1 = (area * (1.0f - mo)) / (1.0f + mo);
    const float sq1 = sqrtf((hw * hw) - (4.0f * c1));
    const float r1 = (hw + sq1) / 2.0f;
    const float b2 = 2.0f * hw;
    const float c2 = (1.0f - mo) * area;
    const float sq2 = sqrtf((b2 * b2) - (16.0f * c2));
    const float r2 = (b2 + sq2) / 2.0f;
    const float a3 = 4.0f * mo;
    const float b3 = (-2.0f * mo) * hw;
    const float c3 = (mo - 1.0f) * area;
    const float sq3 = sqrtf((b3 * b3) - ((4.0f * a3) * c3));
    const float r3 = (b3 + sq3) / 2.0f;
    const float rr = fminf(fminf(r1, r2), r3);
    o.rad = max(p.min_radius, (int)fminf(rr, (float)MAXRAD));
    const float sigma = (float)(2 * o.rad + 1) / 6.0f;
    o.den = (2.0f * sigma) * sigma;
    return true;
}

__global__ __launch_bounds__(DENSE_THREADS) void center_map_kernel(const CtrP p) {
    __shared__ int lix[MAXG], liy[MAXG], lrad[MAXG], llab[MAXG];
    __shared__ float lden[MAXG];
    __shared__ int count;
    const int b = blockIdx.y;
    const int ty = blockIdx.x / p.tx, tx = blockIdx.x - ty * p.tx;
    const int x0 = tx * CT, y0 = ty * CT;
    if (threadIdx.x == 0) count = 0;
    __syncthreads();
    for (int g = threadIdx.x; g < p.G; g += DENSE_THREADS) {
        const int label = p.gl[(size_t)b * p.G + g];
        CBox bx;
        if (!center_box(p, p.gt + ((size_t)b * p.G + g) * p.D, label, bx)) continue;
        if (bx.ix + bx.rad < x0 || bx.ix - bx.rad > x0 + CT - 1 || bx.iy + bx.rad < y0 || bx.iy - bx.rad > y0 + CT - 1) continue;
        const int slot = atomicAdd(&count, 1);                      // (LDS; slot < G <= MAXG)
        lix[slot] = bx.ix; liy[slot] = bx.iy; lrad[slot] = bx.rad; llab[slot] = label; lden[slot] = bx.den;
    }
    __syncthreads();
    const int n = count;
    const int x = x0 + (threadIdx.x & (CT - 1)), y = y0 + (threadIdx.x >> 4);
    if (x >= p.W || y >= p.H) return;
    const int cell = y * p.W + x, HW = p.H * p.W;
    for (int c = 0; c < p.C; ++c) {
        float v = 0.0f;
        for (int i = 0; i < n; ++i) {
            if (llab[i] != c) continue;
            const int dx = x - lix[i], dy = y - liy[i], rad = lrad[i];
            if (dx < -rad || dx > rad || dy < -rad || dy > rad) continue;
            v = fmaxf(v, expf(-(float)(dx * dx + dy * dy) / lden[i]));
        }
        p.hm[map_at(p.nhwc, b, c, cell, p.C, HW)] = v;
    }
}

__global__ __launch_bounds__(DENSE_THREADS) void center_anno_kernel(const CtrP p) {
    const int g = blockIdx.x * DENSE_THREADS + threadIdx.x, b = blockIdx.y;
    if (g >= p.G) return;
    const size_t row = (size_t)b * p.G + g;
    const float *r = p.gt + row * p.D;
    const int na = p.vel ? 10 : 8;
    float *out = p.anno + row * na;
    CBox bx;
    if (!center_box(p, r, p.gl[row], bx)) {
        p.ind[row] = -1;
        for (int q = 0; q < na; ++q) out[q] = 0.0f;
        return;
    }
    p.ind[row] = bx.iy * p.W + bx.ix;
    float s, c;
    sincos_r(r[6], s, c);
    out[0] = bx.fx - (float)bx.ix;
    out[1] = bx.fy - (float)bx.iy;
    out[2] = r[2];
    out[3] = logf(r[3]);
    out[4] = logf(r[4]);
    out[5] = logf(r[5]);
    out[6] = s;
    out[7] = c;
    if (p.vel) { out[8] = r[7]; out[9] = r[8]; }
}

// what both operators ask of the ground truth
int gt_ok(const char *fn, const float *gt_boxes, const int32_t *gt_labels, int B, int G, int D) {
    SAD_REQUIRE(B >= 1 && G >= 0, "%s: need B >= 1 and G >= 0 (got %d, %d)", fn, B, G);
    SAD_REQUIRE(D >= 7, "%s: gt_boxes rows have D = %d columns (need D >= 7)", fn, D);
    SAD_REQUIRE(G == 0 || (gt_boxes && gt_labels), "%s: NULL pointer (gt_boxes, gt_labels)", fn);
    if (G > MAXG) return sad::fail(SAD_EUNSUPPORTED, "%s: G = %d boxes per scene (0 .. 1024 supported)", fn, G);
    if (B > 65535) return sad::fail(SAD_EUNSUPPORTED, "%s: B = %d (1 .. 65535 supported)", fn, B);
    return SAD_OK;
}

}  // namespace

SAD_API size_t sad_anchor_targets_workspace_bytes(int B, int G) {
    if (B < 1 || G < 0 || G > MAXG) return 0;
    return (size_t)B * (size_t)G * sizeof(uint32_t);
}

SAD_API int sad_anchor_targets_f32(const sad_anchor_targets_args *a, sad_stream_t stream) {
    const char *fn = "sad_anchor_targets_f32";
    if (int rc = args_ok(fn, a)) return rc;
    SAD_REQUIRE(a->labels && a->match && a->reg_target && a->max_iou, "%s: NULL pointer", fn);
    SAD_REQUIRE(a->H >= 1 && a->W >= 1, "%s: need H, W >= 1 (got %d, %d)", fn, a->H, a->W);
    SAD_REQUIRE(a->ns >= 1 && a->nr >= 1, "%s: need ns, nr >= 1 (got %d, %d)", fn, a->ns, a->nr);
    SAD_REQUIRE(a->nb == 0 || a->nb >= 2, "%s: nb must be 0 (no direction target) or 2 .. 8 (got %d)", fn, a->nb);
    SAD_REQUIRE((a->nb == 0) == (a->dir_target == nullptr), "%s: dir_target and nb must be given together (nb = %d)", fn, a->nb);
    if (int rc = gt_ok(fn, a->gt_boxes, a->gt_labels, a->B, a->G, a->D)) return rc;
    TgtP p = {};
    if (int rc = fill_anchor_tab(fn, a, &p.tab)) return rc;
    for (int i = 0; i < 3 * a->ns; ++i)
        SAD_REQUIRE(a->sizes[i] > 0.0f, "%s: anchor size %d has a non-positive extent (%g)", fn, i / 3, (double)a->sizes[i]);
    SAD_REQUIRE(a->G == 0 || a->workspace, "%s: NULL workspace (sad_anchor_targets_workspace_bytes(B, G) bytes)", fn);
    const int A = a->ns * a->nr;
    if (!rows_fit(a->B, a->H, a->W, A)) return sad::fail(SAD_EUNSUPPORTED, "%s: B * K = %d * %lld rows (B * K < 2^31 supported)", fn, a->B, (long long)a->H * a->W * A);
    p.gt = a->gt_boxes; p.gl = a->gt_labels;
    p.labels = a->labels; p.match = a->match; p.dir_target = a->dir_target; p.reg = a->reg_target; p.max_iou = a->max_iou;
    p.best = (unsigned *)a->workspace;
    p.G = a->G; p.D = a->D; p.HW = a->H * a->W; p.A = A; p.nb = a->nb; p.use_sc = a->use_size_class != 0;
    p.dir_offset = a->dir_offset; p.period = dir_period(a->nb);
    for (int i = 0; i < a->ns; ++i) { p.pos[i] = a->pos_thr[i]; p.neg[i] = a->neg_thr[i]; p.sc[i] = a->size_class[i]; }
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)anchor_grid_of(p.HW, A, &p.tiles, &p.chunks), a->B);
    if (a->G > 0) {
        if (hipMemsetAsync(a->workspace, 0, sad_anchor_targets_workspace_bytes(a->B, a->G), st) != hipSuccess) return sad::check_launch(fn);
        hipLaunchKernelGGL(anchor_best_kernel, grid, dim3(DENSE_THREADS), 0, st, p);
        if (int rc = sad::check_launch(fn)) return rc;
    }
    hipLaunchKernelGGL(anchor_assign_kernel, grid, dim3(DENSE_THREADS), 0, st, p);
    return sad::check_launch(fn);
}

SAD_API int sad_center_targets_f32(const sad_center_targets_args *a, sad_stream_t stream) {
    const char *fn = "sad_center_targets_f32";
    if (int rc = args_ok(fn, a)) return rc;
    SAD_REQUIRE(a->heatmap, "%s: NULL pointer (heatmap)", fn);
    SAD_REQUIRE(a->layout == SAD_LAYOUT_NCHW || a->layout == SAD_LAYOUT_NHWC, "%s: layout must be SAD_LAYOUT_NCHW or SAD_LAYOUT_NHWC (got %d)", fn, a->layout);
    SAD_REQUIRE(a->H >= 1 && a->W >= 1 && a->C >= 1, "%s: need H, W, C >= 1 (got %d, %d, %d)", fn, a->H, a->W, a->C);
    if (int rc = gt_ok(fn, a->gt_boxes, a->gt_labels, a->B, a->G, a->D)) return rc;
    SAD_REQUIRE(a->G == 0 || (a->ind && a->anno), "%s: NULL pointer (ind, anno)", fn);
    SAD_REQUIRE(a->sx > 0.0f && a->sy > 0.0f, "%s: the cell must be positive (got %g, %g)", fn, (double)a->sx, (double)a->sy);
    SAD_REQUIRE(a->min_overlap > 0.0f && a->min_overlap < 1.0f, "%s: need 0 < min_overlap < 1 (got %g)", fn, (double)a->min_overlap);
    SAD_REQUIRE(a->min_radius >= 0 && a->min_radius <= MAXRAD, "%s: need 0 <= min_radius <= 64 (got %d)", fn, a->min_radius);
    SAD_REQUIRE(!a->vel || a->D >= 9, "%s: vel needs D >= 9 (got %d)", fn, a->D);
    if (a->C > 64) return sad::fail(SAD_EUNSUPPORTED, "%s: C = %d classes (1 .. 64 supported)", fn, a->C);
    if (!rows_fit(a->B, a->H, a->W, 1)) return sad::fail(SAD_EUNSUPPORTED, "%s: B * H * W = %d * %lld cells (B * H * W < 2^31 supported)", fn, a->B, (long long)a->H * a->W);
    CtrP p = {};
    p.gt = a->gt_boxes; p.gl = a->gt_labels; p.hm = a->heatmap; p.ind = a->ind; p.anno = a->anno;
    p.G = a->G; p.D = a->D; p.C = a->C; p.H = a->H; p.W = a->W; p.nhwc = a->layout == SAD_LAYOUT_NHWC;
    p.min_radius = a->min_radius; p.vel = a->vel != 0;
    p.lo_x = a->lo_x; p.lo_y = a->lo_y; p.sx = a->sx; p.sy = a->sy; p.mo = a->min_overlap;
    p.tx = (a->W + CT - 1) / CT;
    const long long tiles = (long long)p.tx * ((a->H + CT - 1) / CT);                           // (<= H * W < 2^31)
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(center_map_kernel, dim3((unsigned)tiles, a->B), dim3(DENSE_THREADS), 0, st, p);
    if (int rc = sad::check_launch(fn)) return rc;
    if (a->G > 0) {
        hipLaunchKernelGGL(center_anno_kernel, dim3((unsigned)((a->G + DENSE_THREADS - 1) / DENSE_THREADS), a->B), dim3(DENSE_THREADS), 0, st, p);
        return sad::check_launch(fn);
    }
    return SAD_OK;
}
