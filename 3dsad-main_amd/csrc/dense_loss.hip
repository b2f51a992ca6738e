// Dense head losses (SPEC.md §27): the maps of an anchor head / a centre head and the targets of §26 -> the per-scene losses
// and the gradient with respect to every map, written in the map's own layout.  The training companion of dense_head.hip and
// dense_target.hip: same K, same k numbering, same channel numbering, same tiles (dense_tile.h).  No float atomics anywhere: every sum is a
// per-thread sum in ascending order, a butterfly over the wave, four wave sums added in order and, in a last small launch, the
// workgroups' partial sums added by one wave per scene (lane l takes workgroups l, l + 64, ... ascending, then the butterfly).
//
// anchor head     memset(num_pos) | count | main | finish.
//   count         num_pos[b] = #(labels >= 0): integer atomics, order-independent.
//   main          a workgroup owns an anchor tile (dense_tile.h).  labels / reg_target / dir_target rows of the tile are contiguous
//                 spans and come in through LDS in memory order (load_spans); per_anchor leaves the same way (flush_spans).
//     nchw        channel planes are unit-stride in the cell: loads and gradient stores of a wave are 256 contiguous bytes.
//     nhwc        a pass (64 cells x 4 anchors) is staged through LDS in memory order (stage_pass), the thread that owns a row overwrites
//                 its values with their gradients, and the image goes back the same way (OUT): class logits in chunks of 8 classes.
// centre head     memset(num_pos) | count | heat map | boxes | finish.
//   heat map      a workgroup owns 256 consecutive cells, one per thread, classes ascending; nhwc staged 16 classes at a time.
//                 It also zero-fills the regression gradients of its cells: the box pass, a later launch, overwrites a few.
//   boxes         one thread per box; the scene's ind[] sits in LDS.  Boxes that share a cell: the lowest g of the cell owns it
//                 and adds the gradients of the others in ascending g (an ordered gather); nobody else stores to that cell.
#include "box_geom.h"
#include <math.h>

namespace {

#include "dense_tile.h"
#include "loss_sums.h"

constexpr int HCH = 16;            // classes per staged chunk (centre head, nhwc)
constexpr float CLAMP_LO = 1e-4f;

struct AncL {
    const float *cls, *reg, *dir, *tgt;
    const int32_t *labels, *dirt;
    int32_t *num_pos;
    float *gcls, *greg, *gdir, *per, *part;
    int HW, A, C, nb, sin_diff, normalize, chunks;
    float alpha, oma, beta, cw[7], scale[3];
};

struct CenL {
    const float *hm, *heatmap, *anno;
    const float *pm[5];            // reg, height, dim, rot, vel
    const int32_t *ind;
    int32_t *num_pos;
    float *ghm, *part_hm, *part_reg;
    float *gm[5];
    int HW, C, G, na, nhwc, normalize, nwg_hm, nwg_reg;
    float cw[10], scale[2];
};

// (block_sum, wave_count, norm_weight, sigmoid2, focal_one and smooth_l1: prims.h; FinP, count_pos_kernel and finish_kernel: loss_sums.h)

// §27.1 regression of one row: r = predictions, t = targets -> term sum (j ascending from +0) and gradients
__device__ __forceinline__ float reg_row(const AncL &p, const float *r, const float *t, bool pos, float wq, float *g) {
    float l = 0.0f;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        float d, extra = 1.0f;
        if (j == 6 && p.sin_diff) {
            float sp, cp, st, ct;
            sincos_r(r[6], sp, cp);
            sincos_r(t[6], st, ct);
            d = sin_diff(sp, cp, st, ct, p.cw[6], extra);
        } else {
            d = (r[j] - t[j]) * p.cw[j];
        }
        float sg;
        const float lj = smooth_l1(d, p.beta, sg);
        float gj = (sg * p.cw[j]) * wq;
        if (j == 6 && p.sin_diff) gj = gj * extra;
        l = l + (pos ? lj * wq : 0.0f);
        g[j] = pos ? gj : 0.0f;
    }
    return l;
}

// §27.1 direction of one row: z = logits (in), gradients (out)
__device__ __forceinline__ float dir_row(const AncL &p, float *z, bool pos, int target, float wq) {
    const bool on = pos && target >= 0 && target < p.nb;
    float m = z[0];
#pragma unroll
    for (int d = 1; d < 8; ++d)
        if (d < p.nb) m = fmaxf(m, z[d]);
    float u[8], s = 0.0f, zt = 0.0f;
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        u[d] = d < p.nb ? expf(z[d] - m) : 0.0f;
        if (d < p.nb) s = s + u[d];
        if (d == target) zt = z[d];
    }
    const float l = ((m + logf(s)) - zt) * wq;
#pragma unroll
    for (int d = 0; d < 8; ++d)
        if (d < p.nb) z[d] = on ? ((u[d] / s) - (d == target ? 1.0f : 0.0f)) * wq : 0.0f;
    return on ? l : 0.0f;
}

// §27.1 classification of one logit -> term (value) and gradient (g)
__device__ __forceinline__ float cls_one(const AncL &p, float x, bool t, bool live, float wq, float &g) {
    return focal_one(p.alpha, p.oma, x, t, live, wq, g);
}

__device__ __forceinline__ size_t plane_at(int ch, int cell, int HW) { return map_at(0, 0, ch, cell, 0, HW); }      // nchw, from the scene's base

template <bool NHWC>
__global__ __launch_bounds__(DENSE_THREADS) void anchor_loss_kernel(const AncL p) {
    __shared__ int32_t slab[TC * AC];
    __shared__ int32_t sdirt[TC * AC];
    __shared__ float stgt[TC * AC * 7];
    __shared__ float oper[TC * AC * 3];
    __shared__ float sreg[NHWC ? DENSE_THREADS * 7 : 1];
    __shared__ float su[NHWC ? DENSE_THREADS * (CCH + 1) : 1];
    __shared__ float red[4];
    const AnchorTile tl = anchor_tile(p.chunks, p.HW, p.A);
    const int b = tl.b, tid = threadIdx.x;
    const size_t HW = (size_t)p.HW;
    tl.load(slab, p.labels, 1);
    tl.load(stgt, p.tgt, 7);
    if (p.nb) tl.load(sdirt, p.dirt, 1);
    const int n = p.num_pos[b];
    const float wq0 = norm_weight(p.scale[0], n, p.normalize), wq1 = norm_weight(p.scale[1], n, p.normalize),
                wq2 = norm_weight(p.scale[2], n, p.normalize);
    // scene bases of the maps (nhwc: rows of the staged passes; nchw: channel planes, addressed by plane_at)
    const float *scls = p.cls + (size_t)b * HW * p.A * p.C;
    float *gcls = p.gcls + (size_t)b * HW * p.A * p.C;
    const float *sregm = p.reg + (size_t)b * HW * p.A * 7;
    float *gregm = p.greg + (size_t)b * HW * p.A * 7;
    const float *sdir = p.nb ? p.dir + (size_t)b * HW * p.A * p.nb : nullptr;
    float *gdirm = p.nb ? p.gdir + (size_t)b * HW * p.A * p.nb : nullptr;
    __syncthreads();
    float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f;
    for (int pass = 0; 4 * pass < tl.acn; ++pass) {
        const bool active = tl.active(pass);
        const int slot = active ? tl.slot(pass) : 0;
        const int a = tl.a0 + (active ? tl.al(pass) : 0), cell = tl.cell0 + (active ? tl.lane : 0);
        const int label = active ? slab[slot] : -2;
        const bool pos = label >= 0;
        // ---- regression
        float r[7], t[7], g[7];
#pragma unroll
        for (int j = 0; j < 7; ++j) t[j] = stgt[slot * 7 + j];
        if (NHWC) {
            __syncthreads();
            stage_pass<false>(tl, pass, sreg, 7, sregm, 7, 0, 7);
            if (p.nb) stage_pass<false>(tl, pass, su, CCH + 1, sdir, p.nb, 0, p.nb);
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 7; ++j) r[j] = sreg[tid * 7 + j];
        }
        // nchw: every value of the row (logits eight at a time) is fetched before the first gradient is stored: one round trip to
        // memory per row, not one per map (the stores in between would otherwise order the loads behind them)
        float z[8], x[CCH];
        if (!NHWC) {
#pragma unroll
            for (int j = 0; j < 7; ++j) r[j] = sregm[plane_at(a * 7 + j, cell, p.HW)];
#pragma unroll
            for (int d = 0; d < 8; ++d) z[d] = d < p.nb ? sdir[plane_at(a * p.nb + d, cell, p.HW)] : 0.0f;
#pragma unroll
            for (int u = 0; u < CCH; ++u) x[u] = u < p.C ? scls[plane_at(a * p.C + u, cell, p.HW)] : 0.0f;
        }
        // (positives are a few rows in a thousand: most waves skip the regression and the direction altogether)
        float l1 = 0.0f;
#pragma unroll
        for (int j = 0; j < 7; ++j) g[j] = 0.0f;
        if (pos) l1 = reg_row(p, r, t, true, wq1, g);
        if (NHWC) {
#pragma unroll
            for (int j = 0; j < 7; ++j) sreg[tid * 7 + j] = g[j];
        } else if (active) {
#pragma unroll
            for (int j = 0; j < 7; ++j) gregm[plane_at(a * 7 + j, cell, p.HW)] = g[j];
        }
        // ---- direction
        float l2 = 0.0f;
        if (p.nb) {
            if (NHWC) {
#pragma unroll
                for (int d = 0; d < 8; ++d) z[d] = d < p.nb ? su[tid * (CCH + 1) + d] : 0.0f;
            }
            const int target = active ? sdirt[slot] : -1;
            if (pos && target >= 0 && target < p.nb) {
                l2 = dir_row(p, z, true, target, wq2);
            } else {
#pragma unroll
                for (int d = 0; d < 8; ++d) z[d] = 0.0f;
            }
#pragma unroll
            for (int d = 0; d < 8; ++d) {
                if (d >= p.nb) continue;
                if (NHWC) su[tid * (CCH + 1) + d] = z[d];
                else if (active) gdirm[plane_at(a * p.nb + d, cell, p.HW)] = z[d];
            }
        }
        if (NHWC) {
            __syncthreads();
            stage_pass<true>(tl, pass, sreg, 7, gregm, 7, 0, 7);
            if (p.nb) stage_pass<true>(tl, pass, su, CCH + 1, gdirm, p.nb, 0, p.nb);
        }
        // ---- classification, classes ascending
        const bool live = label != -2;
        float l0 = 0.0f;
        for (int c0 = 0; c0 < p.C; c0 += CCH) {
            const int len = min(CCH, p.C - c0);
            if (NHWC) {
                __syncthreads();
                stage_pass<false>(tl, pass, su, CCH + 1, scls, p.C, c0, len);
                __syncthreads();
            }
            if (NHWC || c0) {
#pragma unroll
                for (int u = 0; u < CCH; ++u)
                    x[u] = u < len ? (NHWC ? su[tid * (CCH + 1) + u] : scls[plane_at(a * p.C + c0 + u, cell, p.HW)]) : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < CCH; ++u) {
                if (u >= len) continue;
                float gx;
                l0 = l0 + cls_one(p, x[u], label == c0 + u, live, wq0, gx);
                if (NHWC) su[tid * (CCH + 1) + u] = gx;
                else if (active) gcls[plane_at(a * p.C + c0 + u, cell, p.HW)] = gx;
            }
            if (NHWC) {
                __syncthreads();
                stage_pass<true>(tl, pass, su, CCH + 1, gcls, p.C, c0, len);
            }
        }
        if (active) {
            oper[slot * 3] = l0; oper[slot * 3 + 1] = l1; oper[slot * 3 + 2] = l2;
            acc0 = acc0 + l0; acc1 = acc1 + l1; acc2 = acc2 + l2;
        }
    }
    __syncthreads();
    if (p.per) tl.store(oper, p.per, 3);
    const float s0 = block_sum(acc0, red), s1 = block_sum(acc1, red), s2 = block_sum(acc2, red);
    if (tid == 0) {
        float *o = p.part + ((size_t)b * gridDim.x + blockIdx.x) * 3;
        o[0] = s0; o[1] = s1; o[2] = s2;
    }
}

__global__ __launch_bounds__(DENSE_THREADS) void center_count_kernel(const CenL p) {
    const int b = blockIdx.y;
    const size_t n = (size_t)p.C * p.HW;
    const float *t = p.heatmap + (size_t)b * n;
    float v[CNT];
#pragma unroll
    for (int q = 0; q < CNT; ++q) {
        const size_t i = ((size_t)blockIdx.x * CNT + q) * DENSE_THREADS + threadIdx.x;
        v[q] = i < n ? t[i] : 0.0f;
    }
    int cnt = 0;
#pragma unroll
    for (int q = 0; q < CNT; ++q) cnt += v[q] == 1.0f;
    cnt = wave_count(cnt);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&p.num_pos[2 * b], cnt);
    if (blockIdx.x == 0) {
        int nb = 0;
        for (int g = threadIdx.x; g < p.G; g += DENSE_THREADS) {
            const int c = p.ind[(size_t)b * p.G + g];
            if (c >= 0 && c < p.HW) ++nb;
        }
        nb = wave_count(nb);
        if ((threadIdx.x & 63) == 0 && nb) atomicAdd(&p.num_pos[2 * b + 1], nb);
    }
}

// §27.2 one heat-map element -> term (value) and gradient (g)
__device__ __forceinline__ float hm_one(float x, float t, float wq, float &g) {
    const float hi = 1.0f - CLAMP_LO;
    const float e = expf(-fabsf(x));
    float ps, pcs;
    sigmoid2(x, e, ps, pcs);
    const float pr = fminf(fmaxf(ps, CLAMP_LO), hi);
    const bool inside = ps >= CLAMP_LO && ps <= hi;
    const float q = 1.0f - pr;
    float l, gr;
    if (t == 1.0f) {
        const float lg = logf(pr);
        l = (-lg) * (q * q);
        gr = (q * q) * (((2.0f * pr) * lg) - q);
    } else {
        const float lg = logf(q);
        const float w1 = (1.0f - t) * (1.0f - t), w = w1 * w1;
        l = ((-lg) * (pr * pr)) * w;
        gr = (w * (pr * pr)) * (pr - ((2.0f * q) * lg));
    }
    g = inside ? gr * wq : 0.0f;
    return l * wq;
}

// cells of a centre tile <-> lds[cell * (HCH + 1) + e], e < len: classes c0 .. c0 + len - 1 of C, in memory order (nhwc)
template <bool OUT, class P>
__device__ __forceinline__ void stage_cells(float *lds, P *scene, int C, int c0, int len, int cell0, int ncell) {
    const int n = ncell * len;
    for (int i = threadIdx.x; i < n; i += DENSE_THREADS) {
        const int cell = i / len, e = i - cell * len;
        P *g = scene + (size_t)(cell0 + cell) * C + c0 + e;
        if constexpr (OUT) *g = lds[cell * (HCH + 1) + e];
        else lds[cell * (HCH + 1) + e] = *g;
    }
}

template <bool NHWC>
__global__ __launch_bounds__(DENSE_THREADS) void center_hm_kernel(const CenL p) {
    __shared__ float sx[NHWC ? DENSE_THREADS * (HCH + 1) : 1];
    __shared__ float st[NHWC ? DENSE_THREADS * (HCH + 1) : 1];
    __shared__ float red[4];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int cell0 = blockIdx.x * DENSE_THREADS, ncell = min(DENSE_THREADS, p.HW - cell0);
    const bool active = tid < ncell;
    const size_t HW = (size_t)p.HW, base = (size_t)b * p.C * HW;
    const float wq = norm_weight(p.scale[0], p.num_pos[2 * b], p.normalize);
    float acc = 0.0f;
    if (NHWC) {
        for (int c0 = 0; c0 < p.C; c0 += HCH) {
            const int len = min(HCH, p.C - c0);
            __syncthreads();
            stage_cells<false>(sx, p.hm + base, p.C, c0, len, cell0, ncell);
            stage_cells<false>(st, p.heatmap + base, p.C, c0, len, cell0, ncell);
            __syncthreads();
            if (active) {
                for (int u = 0; u < len; ++u) {
                    float g;
                    acc = acc + hm_one(sx[tid * (HCH + 1) + u], st[tid * (HCH + 1) + u], wq, g);
                    sx[tid * (HCH + 1) + u] = g;
                }
            }
            __syncthreads();
            stage_cells<true>(sx, p.ghm + base, p.C, c0, len, cell0, ncell);
        }
    } else if (active) {
        for (int c = 0; c < p.C; ++c) {
            const size_t i = base + (size_t)c * HW + cell0 + tid;
            float g;
            acc = acc + hm_one(p.hm[i], p.heatmap[i], wq, g);
            p.ghm[i] = g;
        }
    }
    // the zero fill of the regression gradients of these cells (the box pass, a later launch, overwrites the boxes' cells):
    // nhwc: the tile's cells are one contiguous run of ncell * CH floats; nchw: one run of ncell floats per channel
    constexpr int CH[5] = {2, 1, 3, 2, 2};
#pragma unroll
    for (int m = 0; m < 5; ++m) {
        if (!p.gm[m]) continue;
        float *g = p.gm[m] + (size_t)b * CH[m] * HW;
        if (NHWC) {
            for (int i = tid; i < ncell * CH[m]; i += DENSE_THREADS) g[(size_t)cell0 * CH[m] + i] = 0.0f;
        } else if (active) {
#pragma unroll
            for (int ch = 0; ch < CH[m]; ++ch) g[(size_t)ch * HW + cell0 + tid] = 0.0f;
        }
    }
    const float s = block_sum(acc, red);
    if (tid == 0) p.part_hm[(size_t)b * p.nwg_hm + blockIdx.x] = s;
}

__global__ __launch_bounds__(DENSE_THREADS) void center_reg_kernel(const CenL p) {
    __shared__ int sind[MAXG];
    __shared__ float red[4];
    const int b = blockIdx.y, tid = threadIdx.x;
    for (int g = tid; g < p.G; g += DENSE_THREADS) sind[g] = p.ind[(size_t)b * p.G + g];
    __syncthreads();
    const float wq = norm_weight(p.scale[1], p.num_pos[2 * b + 1], p.normalize);
    const int g = blockIdx.x * DENSE_THREADS + tid;
    const int cell = g < p.G ? sind[g] : -1;
    float l = 0.0f;
    if (cell >= 0 && cell < p.HW) {
        constexpr int JM[10] = {0, 0, 1, 2, 2, 2, 3, 3, 4, 4}, JC[10] = {0, 1, 0, 0, 1, 2, 0, 1, 0, 1}, CH[5] = {2, 1, 3, 2, 2};
        float pred[10], gs[10];
        const float *an = p.anno + ((size_t)b * p.G + g) * p.na;
        size_t at[10];
#pragma unroll
        for (int j = 0; j < 10; ++j) {
            if (j >= p.na) continue;
            at[j] = map_at(p.nhwc, b, JC[j], cell, CH[JM[j]], p.HW);
            pred[j] = p.pm[JM[j]][at[j]];
            const float d = pred[j] - an[j];
            l = l + (fabsf(d) * p.cw[j]) * wq;
            gs[j] = ((float)((d > 0.0f) - (d < 0.0f)) * p.cw[j]) * wq;
        }
        bool owner = true;
        for (int g2 = 0; g2 < g; ++g2) owner = owner && sind[g2] != cell;
        if (owner) {
            for (int g2 = g + 1; g2 < p.G; ++g2) {
                if (sind[g2] != cell) continue;
                const float *an2 = p.anno + ((size_t)b * p.G + g2) * p.na;
#pragma unroll
                for (int j = 0; j < 10; ++j) {
                    if (j >= p.na) continue;
                    const float d = pred[j] - an2[j];
                    gs[j] = gs[j] + ((float)((d > 0.0f) - (d < 0.0f)) * p.cw[j]) * wq;
                }
            }
#pragma unroll
            for (int j = 0; j < 10; ++j)
                if (j < p.na) p.gm[JM[j]][at[j]] = gs[j];
        }
    }
    const float s = block_sum(l, red);
    if (tid == 0) p.part_reg[(size_t)b * p.nwg_reg + blockIdx.x] = s;
}

}  // namespace

SAD_API size_t sad_anchor_head_loss_workspace_bytes(int B, int H, int W, int A) {
    if (B < 1 || B > 65535 || H < 1 || W < 1 || A < 1 || A > 128) return 0;
    if (!rows_fit(B, H, W, A)) return 0;
    int tiles, chunks;      // (one slot of three partial sums per workgroup of anchor_loss_kernel)
    return (size_t)B * (size_t)anchor_grid_of(H * W, A, &tiles, &chunks) * 3 * sizeof(float);
}

SAD_API size_t sad_center_head_loss_workspace_bytes(int B, int H, int W, int G) {
    if (B < 1 || B > 65535 || H < 1 || W < 1 || G < 0 || G > MAXG) return 0;
    if (!rows_fit(B, H, W, 1)) return 0;
    const long long HW = (long long)H * W;
    return (size_t)B * (size_t)((HW + DENSE_THREADS - 1) / DENSE_THREADS + (G + DENSE_THREADS - 1) / DENSE_THREADS) * sizeof(float);
}

SAD_API int sad_anchor_head_loss_f32(const sad_anchor_head_loss_args *a, sad_stream_t stream) {
    const char *fn = "sad_anchor_head_loss_f32";
    if (int rc = args_ok(fn, a)) return rc;
    SAD_REQUIRE(a->cls && a->reg && a->labels && a->reg_target && a->loss && a->num_pos && a->grad_cls && a->grad_reg && a->workspace,
                "%s: NULL pointer", fn);
    SAD_REQUIRE(a->layout == SAD_LAYOUT_NCHW || a->layout == SAD_LAYOUT_NHWC, "%s: layout must be SAD_LAYOUT_NCHW or SAD_LAYOUT_NHWC (got %d)", fn, a->layout);
    SAD_REQUIRE(a->B >= 1 && a->H >= 1 && a->W >= 1 && a->A >= 1 && a->C >= 1, "%s: need B, H, W, A, C >= 1 (got %d, %d, %d, %d, %d)", fn, a->B,
                a->H, a->W, a->A, a->C);
    SAD_REQUIRE(a->nb == 0 || a->nb >= 2, "%s: nb must be 0 (no direction loss) or 2 .. 8 (got %d)", fn, a->nb);
    SAD_REQUIRE((a->nb == 0) == (a->dir == nullptr) && (a->nb == 0) == (a->dir_target == nullptr) && (a->nb == 0) == (a->grad_dir == nullptr),
                "%s: dir, dir_target, grad_dir and nb must be given together (nb = %d)", fn, a->nb);
    SAD_REQUIRE(a->beta > 0.0f, "%s: need beta > 0 (got %g)", fn, (double)a->beta);
    SAD_REQUIRE(a->alpha >= 0.0f && a->alpha <= 1.0f, "%s: need 0 <= alpha <= 1 (got %g)", fn, (double)a->alpha);
    if (a->B > 65535) return sad::fail(SAD_EUNSUPPORTED, "%s: B = %d (1 .. 65535 supported)", fn, a->B);
    if (a->C > 64) return sad::fail(SAD_EUNSUPPORTED, "%s: C = %d classes (1 .. 64 supported)", fn, a->C);
    if (a->A > 128 || a->nb > 8) return sad::fail(SAD_EUNSUPPORTED, "%s: A = %d, nb = %d (A <= 128, nb <= 8 supported)", fn, a->A, a->nb);
    if (!rows_fit(a->B, a->H, a->W, a->A)) return sad::fail(SAD_EUNSUPPORTED, "%s: B * K = %d * %d * %d * %d rows (B * K < 2^31 supported)", fn, a->B, a->H, a->W, a->A);
    const int HW = a->H * a->W;
    const long long K = (long long)HW * a->A;
    AncL p = {};
    p.cls = a->cls; p.reg = a->reg; p.dir = a->dir; p.tgt = a->reg_target; p.labels = a->labels; p.dirt = a->dir_target;
    p.num_pos = a->num_pos; p.gcls = a->grad_cls; p.greg = a->grad_reg; p.gdir = a->grad_dir; p.per = a->per_anchor;
    p.part = (float *)a->workspace;
    p.HW = HW; p.A = a->A; p.C = a->C; p.nb = a->nb; p.sin_diff = a->sin_diff != 0; p.normalize = a->normalize != 0;
    p.alpha = a->alpha; p.oma = 1.0f - a->alpha; p.beta = a->beta;
    for (int j = 0; j < 7; ++j) p.cw[j] = a->code_weights[j];
    for (int i = 0; i < 3; ++i) p.scale[i] = a->scale[i];
    const hipStream_t st = (hipStream_t)stream;
    int tiles;
    const int nwg = anchor_grid_of(HW, a->A, &tiles, &p.chunks);
    if (hipMemsetAsync(a->num_pos, 0, (size_t)a->B * sizeof(int32_t), st) != hipSuccess) return sad::check_launch(fn);
    hipLaunchKernelGGL(count_pos_kernel, dim3((unsigned)((K + CNT * DENSE_THREADS - 1) / (CNT * DENSE_THREADS)), a->B), dim3(DENSE_THREADS), 0, st, a->labels,
                       (int)K, a->num_pos);
    if (int rc = sad::check_launch(fn)) return rc;
    const dim3 grid((unsigned)nwg, a->B);
    if (a->layout == SAD_LAYOUT_NHWC) hipLaunchKernelGGL(anchor_loss_kernel<true>, grid, dim3(DENSE_THREADS), 0, st, p);
    else hipLaunchKernelGGL(anchor_loss_kernel<false>, grid, dim3(DENSE_THREADS), 0, st, p);
    if (int rc = sad::check_launch(fn)) return rc;
    FinP f = {};
    for (int i = 0; i < 3; ++i) { f.src[i] = p.part + i; f.n[i] = nwg; f.stride[i] = 3; }
    f.ncomp = 3; f.loss = a->loss;
    hipLaunchKernelGGL(finish_kernel, dim3(a->B), dim3(64), 0, st, f);
    return sad::check_launch(fn);
}

SAD_API int sad_center_head_loss_f32(const sad_center_head_loss_args *a, sad_stream_t stream) {
    const char *fn = "sad_center_head_loss_f32";
    if (int rc = args_ok(fn, a)) return rc;
    SAD_REQUIRE(a->hm && a->reg && a->height && a->dim && a->rot && a->heatmap && a->loss && a->num_pos && a->grad_hm && a->grad_reg &&
                    a->grad_height && a->grad_dim && a->grad_rot && a->workspace,
                "%s: NULL pointer", fn);
    SAD_REQUIRE((a->vel == nullptr) == (a->grad_vel == nullptr), "%s: vel and grad_vel must be given together", fn);
    SAD_REQUIRE(a->layout == SAD_LAYOUT_NCHW || a->layout == SAD_LAYOUT_NHWC, "%s: layout must be SAD_LAYOUT_NCHW or SAD_LAYOUT_NHWC (got %d)", fn, a->layout);
    SAD_REQUIRE(a->B >= 1 && a->H >= 1 && a->W >= 1 && a->C >= 1 && a->G >= 0, "%s: need B, H, W, C >= 1 and G >= 0 (got %d, %d, %d, %d, %d)", fn,
                a->B, a->H, a->W, a->C, a->G);
    SAD_REQUIRE(a->G == 0 || (a->ind && a->anno), "%s: NULL pointer (ind, anno)", fn);
    if (a->B > 65535) return sad::fail(SAD_EUNSUPPORTED, "%s: B = %d (1 .. 65535 supported)", fn, a->B);
    if (a->C > 64) return sad::fail(SAD_EUNSUPPORTED, "%s: C = %d classes (1 .. 64 supported)", fn, a->C);
    if (a->G > MAXG) return sad::fail(SAD_EUNSUPPORTED, "%s: G = %d boxes per scene (0 .. 1024 supported)", fn, a->G);
    if (!rows_fit(a->B, a->H, a->W, 1)) return sad::fail(SAD_EUNSUPPORTED, "%s: B * H * W = %d * %lld cells (B * H * W < 2^31 supported)", fn, a->B, (long long)a->H * a->W);
    const int HW = a->H * a->W;
    CenL p = {};
    p.hm = a->hm; p.heatmap = a->heatmap; p.anno = a->anno; p.ind = a->ind; p.num_pos = a->num_pos; p.ghm = a->grad_hm;
    p.pm[0] = a->reg; p.pm[1] = a->height; p.pm[2] = a->dim; p.pm[3] = a->rot; p.pm[4] = a->vel;
    p.gm[0] = a->grad_reg; p.gm[1] = a->grad_height; p.gm[2] = a->grad_dim; p.gm[3] = a->grad_rot; p.gm[4] = a->grad_vel;
    p.HW = HW; p.C = a->C; p.G = a->G; p.na = a->vel ? 10 : 8; p.nhwc = a->layout == SAD_LAYOUT_NHWC; p.normalize = a->normalize != 0;
    p.nwg_hm = (int)(((long long)HW + DENSE_THREADS - 1) / DENSE_THREADS);
    p.nwg_reg = (a->G + DENSE_THREADS - 1) / DENSE_THREADS;
    p.part_hm = (float *)a->workspace;
    p.part_reg = p.part_hm + (size_t)a->B * p.nwg_hm;
    for (int j = 0; j < 10; ++j) p.cw[j] = a->code_weights[j];
    p.scale[0] = a->scale[0]; p.scale[1] = a->scale[1];
    const hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(a->num_pos, 0, (size_t)a->B * 2 * sizeof(int32_t), st) != hipSuccess) return sad::check_launch(fn);
    const long long nel = (long long)HW * a->C;
    hipLaunchKernelGGL(center_count_kernel, dim3((unsigned)((nel + CNT * DENSE_THREADS - 1) / (CNT * DENSE_THREADS)), a->B), dim3(DENSE_THREADS), 0, st, p);
    if (int rc = sad::check_launch(fn)) return rc;
    const dim3 grid((unsigned)p.nwg_hm, a->B);
    if (p.nhwc) hipLaunchKernelGGL(center_hm_kernel<true>, grid, dim3(DENSE_THREADS), 0, st, p);
    else hipLaunchKernelGGL(center_hm_kernel<false>, grid, dim3(DENSE_THREADS), 0, st, p);
    if (int rc = sad::check_launch(fn)) return rc;
    if (a->G > 0) {
        hipLaunchKernelGGL(center_reg_kernel, dim3((unsigned)p.nwg_reg, a->B), dim3(DENSE_THREADS), 0, st, p);
        if (int rc = sad::check_launch(fn)) return rc;
    }
    FinP f = {};
    f.src[0] = p.part_hm; f.n[0] = p.nwg_hm; f.stride[0] = 1;
    f.src[1] = p.part_reg; f.n[1] = p.nwg_reg; f.stride[1] = 1;
    f.ncomp = 2; f.loss = a->loss;
    hipLaunchKernelGGL(finish_kernel, dim3(a->B), dim3(64), 0, st, f);
    return sad::check_launch(fn);
}
