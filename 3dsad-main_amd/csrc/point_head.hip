// Point head targets and loss (SPEC.md §31): what the size-adaptive cluster layer (§8: c[B,K,6]) and the box / class head
// (§9: o[B,K,C+7]) are trained against, and the loss on top with its gradient with respect to both.  The point-path
// counterpart of dense_target.hip / dense_loss.hip (§26 / §27) and roi_head.hip / roi_loss.hip (§28 / §29): same arithmetic
// rules, same label values, same normaliser, same sums, no float atomics.  M is the number of points of a scene (K = 256 in
// the detector, 16 384 for a per-point head); rows are point-major, as PackedMLP.rows leaves them.
//
// point_targets   one launch, grid (ceil(M / 256), B), one point per thread, no workspace, no atomics.
//   staging       the scene's boxes go to LDS once per workgroup: centre, extents, sincos_r(yaw) and (g << 4 | class), 9 words
//                 per box.  Padding rows (label outside [0, C), an extent <= 0) are dropped here: a pass of 256 rows is
//                 compacted in order (a ballot per wave, the four wave counts through LDS), so slot order is g order.
//   a point       walks the slots in ascending order until inside(xyz, box, 0) (§19.1: box_geom.h): the LDS reads are
//                 broadcasts.  A point without a box walks them again with the extents enlarged by extra_width (the band).
//                 The matched box gives the centre-ness at cand and the three targets; the yaw comes from the box's row.
//   stores        labels / match / centerness are unit-stride; the 3- and 7-column rows leave through LDS in memory order.
// point_head_loss memset(num_pos) | count | main | finish (loss_sums.h), §27.1's sequence.
//   main          grid (ceil(M / 256), B), one point per thread.  The rows of 256 points (o, c, reg_target, shift_target,
//                 size_target) are contiguous runs: they come in through LDS in memory order, the thread that owns a row reads
//                 it (o at an odd stride: no bank conflict), overwrites o and c with their gradients, and grad_o / grad_c leave
//                 the same way.  Four block_sums, one slot of four partial sums per workgroup.
#include "box_geom.h"
#include <math.h>

namespace {

#include "prims.h"
#include "loss_sums.h"

constexpr int PH_THREADS = 256, PH_MAXG = 1024, PH_MAXC = 16;
constexpr int PH_OW = PH_MAXC + 7;          // an o row in LDS: C + 7 words at stride PH_OW (odd)

struct PtT {
    const float *xyz, *cand, *gt;
    const int32_t *gl;
    int32_t *labels, *match;
    float *cent, *shift, *size, *reg;
    int M, G, D, C;
    float e2, shift_max, sa[3], anchors[3 * PH_MAXC];
};

struct PtL {
    const float *o, *c, *cent, *tgt, *sht, *szt;
    const int32_t *labels;
    const int32_t *num_pos;
    float *go, *gc, *per, *part;
    int M, C, focal, normalize;
    float alpha, oma, beta, shift_max, cw[7], scale[4];
};

__device__ __forceinline__ float clampf(float v, float lim) { return fminf(fmaxf(v, -lim), lim); }

// §31.1 one axis of the centre-ness: h = half extent, l = the local coordinate
__device__ __forceinline__ float axis_ratio(float h, float l) {
    const float f = h + l, bk = h - l;
    const float mn = fmaxf(fminf(f, bk), 0.0f), mx = fmaxf(f, bk);
    return mx > 0.0f ? mn / mx : 0.0f;
}

// rows of `n` points x `w` words: LDS (stride `ws`) <-> memory (stride w), in memory order
template <bool OUT, class P>
__device__ __forceinline__ void stage_rows(float *lds, int ws, P *mem, int w, int n) {
    for (int i = threadIdx.x; i < n * w; i += PH_THREADS) {
        const int r = i / w, e = i - r * w;
        if constexpr (OUT) mem[i] = lds[r * ws + e];
        else lds[r * ws + e] = mem[i];
    }
}

__global__ __launch_bounds__(PH_THREADS) void point_targets_kernel(const PtT p) {
    __shared__ float4 s_a[PH_MAXG];                    // cx, cy, cz, l
    __shared__ float4 s_b[PH_MAXG];                    // w, h, cos, sin
    __shared__ int s_k[PH_MAXG];                       // g << 4 | class
    __shared__ float s_reg[PH_THREADS * 7], s_sh[PH_THREADS * 3], s_sz[PH_THREADS * 3];
    __shared__ int wcnt[PH_THREADS / 64];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // ---- the scene's boxes, padding rows dropped, order kept
    int n = 0;
    for (int g0 = 0; g0 < p.G; g0 += PH_THREADS) {
        const int g = g0 + tid;
        float r[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        int cls = -1;
        if (g < p.G) {
            const float *row = p.gt + ((size_t)b * p.G + g) * p.D;
#pragma unroll
            for (int j = 0; j < 7; ++j) r[j] = row[j];
            cls = p.gl[(size_t)b * p.G + g];
        }
        const bool ok = gt_row_valid(cls, p.C, r);
        const u64 m = __ballot(ok);
        const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        if (lane == 0) wcnt[wave] = __popcll(m);
        __syncthreads();
        int at = n + rank;
        for (int w = 0; w < wave; ++w) at += wcnt[w];
        // (not BoxK: the band test needs the raw extents)
        if (ok) {                                       // (at < n + 256 <= G <= PH_MAXG)
            float s, c;
            sincos_r(r[6], s, c);
            s_a[at] = make_float4(r[0], r[1], r[2], r[3]);
            s_b[at] = make_float4(r[4], r[5], c, s);
            s_k[at] = (g << 4) | cls;
        }
        n += ((wcnt[0] + wcnt[1]) + wcnt[2]) + wcnt[3];
        __syncthreads();
    }
    // ---- one point
    const int m0 = blockIdx.x * PH_THREADS, nrow = min(PH_THREADS, p.M - m0);
    const bool act = tid < nrow;
    const size_t row0 = (size_t)b * p.M + m0, row = row0 + (act ? tid : 0);
    const float px = p.xyz[row * 3], py = p.xyz[row * 3 + 1], pz = p.xyz[row * 3 + 2];
    int j = -1;
    for (int i = 0; i < n && j < 0; ++i) {
        const float4 a = s_a[i], bb = s_b[i];
        if (inside(px, py, pz, a.x, a.y, a.z, 0.5f * a.w, 0.5f * bb.x, 0.5f * bb.y, bb.z, bb.w)) j = i;
    }
    bool band = false;
    if (j < 0) {
        for (int i = 0; i < n && !band; ++i) {
            const float4 a = s_a[i], bb = s_b[i];
            band = inside(px, py, pz, a.x, a.y, a.z, 0.5f * (a.w + p.e2), 0.5f * (bb.x + p.e2), 0.5f * (bb.y + p.e2), bb.z, bb.w);
        }
    }
    int label = band ? -2 : -1, match = -1;
    float cent = 0.0f, sh[3] = {0.f, 0.f, 0.f}, sz[3] = {0.f, 0.f, 0.f}, rt[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (j >= 0) {
        const float4 a = s_a[j], bb = s_b[j];
        label = s_k[j] & 15;
        match = s_k[j] >> 4;
        const float ctr[3] = {a.x, a.y, a.z}, ext[3] = {a.w, bb.x, bb.y}, pt[3] = {px, py, pz};
        float q[3] = {px, py, pz};
        if (p.cand) {
#pragma unroll
            for (int d = 0; d < 3; ++d) q[d] = p.cand[row * 3 + d];
        }
        // centre-ness at q, in the box's frame (lx, ly, dz: §19.1's)
        const float dx = q[0] - a.x, dy = q[1] - a.y, dz = q[2] - a.z;
        float lx, ly;
        to_frame(dx, dy, bb.z, bb.w, lx, ly);
        const float rx = axis_ratio(0.5f * a.w, lx), ry = axis_ratio(0.5f * bb.x, ly), rz = axis_ratio(0.5f * bb.y, dz);
        cent = cbrtf((rx * ry) * rz);
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            sh[d] = clampf(ctr[d] - pt[d], p.shift_max);
            const float qd = ext[d] / p.sa[d];
            const float u = fmaxf((2.0f * qd) - 1.0f, 0.0f);
            sz[d] = fminf(sqrtf(u) - 1.0f, 1.0f);
            rt[d] = ctr[d] - q[d];
            rt[3 + d] = clampf(logf(ext[d] / p.anchors[label * 3 + d]), 2.0f);
        }
        rt[6] = p.gt[((size_t)b * p.G + match) * p.D + 6];
    }
    if (act) {
        p.labels[row] = label;
        p.match[row] = match;
        p.cent[row] = cent;
#pragma unroll
        for (int d = 0; d < 3; ++d) { s_sh[tid * 3 + d] = sh[d]; s_sz[tid * 3 + d] = sz[d]; }
#pragma unroll
        for (int q = 0; q < 7; ++q) s_reg[tid * 7 + q] = rt[q];
    }
    __syncthreads();
    stage_rows<true>(s_sh, 3, p.shift + row0 * 3, 3, nrow);
    stage_rows<true>(s_sz, 3, p.size + row0 * 3, 3, nrow);
    stage_rows<true>(s_reg, 7, p.reg + row0 * 7, 7, nrow);
}

// §31.2 box regression of one positive row: r = o[C .. C + 6], t = reg_target -> the term; r becomes the gradients
__device__ __forceinline__ float reg_row(const PtL &p, float *r, const float *t, float wq) {
    float l = 0.0f;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        float d, extra = 1.0f;
        bool pass = true;
        if (j == 6) {
            float sp, cp, st, ct;
            sincos_r(r[6], sp, cp);
            sincos_r(t[6], st, ct);
            d = sin_diff(sp, cp, st, ct, p.cw[6], extra);
        } else if (j >= 3) {
            pass = r[j] >= -2.0f && r[j] <= 2.0f;
            d = (clampf(r[j], 2.0f) - t[j]) * p.cw[j];
        } else {
            d = (r[j] - t[j]) * p.cw[j];
        }
        float sg;
        const float lj = smooth_l1(d, p.beta, sg);
        float gj = (sg * p.cw[j]) * wq;
        if (j == 6) gj = gj * extra;
        l = l + (lj * wq);
        r[j] = pass ? gj : 0.0f;
    }
    return l;
}

// §31.2 shift / size of one positive row: x = three columns of c, clamped to +-lim, against t -> the term; x becomes the gradients
__device__ __forceinline__ float c_row(const PtL &p, float *x, const float *t, float lim, float wq) {
    float l = 0.0f;
#pragma unroll
    for (int d3 = 0; d3 < 3; ++d3) {
        const bool pass = x[d3] >= -lim && x[d3] <= lim;
        float sg;
        const float lj = smooth_l1(clampf(x[d3], lim) - t[d3], p.beta, sg);
        l = l + (lj * wq);
        x[d3] = pass ? sg * wq : 0.0f;
    }
    return l;
}

__global__ __launch_bounds__(PH_THREADS) void point_loss_kernel(const PtL p) {
    __shared__ float s_o[PH_THREADS * PH_OW];          // o rows in, grad_o rows out
    __shared__ float s_c[PH_THREADS * 7];              // c rows in, grad_c rows out (6 words at stride 7)
    __shared__ float s_tgt[PH_THREADS * 7], s_sht[PH_THREADS * 3], s_szt[PH_THREADS * 3];
    __shared__ float red[4];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int m0 = blockIdx.x * PH_THREADS, nrow = min(PH_THREADS, p.M - m0);
    const bool act = tid < nrow;
    const size_t row0 = (size_t)b * p.M + m0, row = row0 + (act ? tid : 0);
    const int W = p.C + 7;
    stage_rows<false>(s_o, PH_OW, p.o + row0 * W, W, nrow);
    stage_rows<false>(s_tgt, 7, p.tgt + row0 * 7, 7, nrow);
    if (p.c) stage_rows<false>(s_c, 7, p.c + row0 * 6, 6, nrow);
    if (p.sht) stage_rows<false>(s_sht, 3, p.sht + row0 * 3, 3, nrow);
    if (p.szt) stage_rows<false>(s_szt, 3, p.szt + row0 * 3, 3, nrow);
    const int n = p.num_pos[b];
    const float wq0 = norm_weight(p.scale[0], n, p.normalize), wq1 = norm_weight(p.scale[1], n, p.normalize),
                wq2 = norm_weight(p.scale[2], n, p.normalize), wq3 = norm_weight(p.scale[3], n, p.normalize);
    const int label = act ? p.labels[row] : -2;
    const bool pos = label >= 0, live = label != -2;
    const float soft = (pos && p.cent) ? p.cent[row] : 1.0f;
    __syncthreads();
    float l0 = 0.0f, l1 = 0.0f, l2 = 0.0f, l3 = 0.0f;
    if (act) {
        float *o = s_o + tid * PH_OW;
        // ---- classification, classes ascending
        for (int ch = 0; ch < p.C; ++ch) {
            const bool hot = label == ch;
            float g;
            l0 = l0 + (p.focal ? focal_one(p.alpha, p.oma, o[ch], hot, live, wq0, g) : bce_one(o[ch], hot ? soft : 0.0f, live, wq0, g));
            o[ch] = g;
        }
        // ---- box regression, shift and size: positives only, results selected
        float r[7], x[6];
#pragma unroll
        for (int q = 0; q < 7; ++q) r[q] = 0.0f;
#pragma unroll
        for (int q = 0; q < 6; ++q) x[q] = 0.0f;
        if (pos) {
            float t[7];
#pragma unroll
            for (int q = 0; q < 7; ++q) { r[q] = o[p.C + q]; t[q] = s_tgt[tid * 7 + q]; }
            l1 = reg_row(p, r, t, wq1);
            if (p.sht) {
#pragma unroll
                for (int q = 0; q < 3; ++q) { x[q] = s_c[tid * 7 + q]; t[q] = s_sht[tid * 3 + q]; }
                l2 = c_row(p, x, t, p.shift_max, wq2);
            }
            if (p.szt) {
#pragma unroll
                for (int q = 0; q < 3; ++q) { x[3 + q] = s_c[tid * 7 + 3 + q]; t[q] = s_szt[tid * 3 + q]; }
                l3 = c_row(p, x + 3, t, 1.0f, wq3);
            }
        }
#pragma unroll
        for (int q = 0; q < 7; ++q) o[p.C + q] = r[q];
        if (p.c) {
#pragma unroll
            for (int q = 0; q < 6; ++q) s_c[tid * 7 + q] = x[q];
        }
        if (p.per) {
            float *per = p.per + row * 4;
            per[0] = l0; per[1] = l1; per[2] = l2; per[3] = l3;
        }
    }
    __syncthreads();
    stage_rows<true>(s_o, PH_OW, p.go + row0 * W, W, nrow);
    if (p.c) stage_rows<true>(s_c, 7, p.gc + row0 * 6, 6, nrow);
    const float s0 = block_sum(l0, red), s1 = block_sum(l1, red), s2 = block_sum(l2, red), s3 = block_sum(l3, red);
    if (tid == 0) {
        float *out = p.part + ((size_t)b * gridDim.x + blockIdx.x) * 4;
        out[0] = s0; out[1] = s1; out[2] = s2; out[3] = s3;
    }
}

// what both operators ask of the shape: rows are numbered in int
int shape_ok(const char *fn, int B, int M, int C) {
    SAD_REQUIRE(B >= 1 && M >= 1 && C >= 1, "%s: need B, M, C >= 1 (got %d, %d, %d)", fn, B, M, C);
    if (B > 65535) return sad::fail(SAD_EUNSUPPORTED, "%s: B = %d (1 .. 65535 supported)", fn, B);
    if (C > PH_MAXC) return sad::fail(SAD_EUNSUPPORTED, "%s: C = %d classes (1 .. 16 supported)", fn, C);
    if ((long long)B * M >= (1LL << 31)) return sad::fail(SAD_EUNSUPPORTED, "%s: B * M = %d * %d rows (B * M < 2^31 supported)", fn, B, M);
    return SAD_OK;
}

inline int workgroups(int M) { return (int)(((long long)M + PH_THREADS - 1) / PH_THREADS); }

}  // namespace

SAD_API int sad_point_targets_f32(const sad_point_targets_args *a, sad_stream_t stream) {
    const char *fn = "sad_point_targets_f32";
    if (int rc = args_ok(fn, a)) return rc;
    SAD_REQUIRE(a->xyz && a->labels && a->match && a->centerness && a->shift_target && a->size_target && a->reg_target, "%s: NULL pointer", fn);
    SAD_REQUIRE(a->G >= 0, "%s: need G >= 0 (got %d)", fn, a->G);
    SAD_REQUIRE(a->D >= 7, "%s: gt_boxes rows have D = %d columns (need D >= 7)", fn, a->D);
    SAD_REQUIRE(a->G == 0 || (a->gt_boxes && a->gt_labels), "%s: NULL pointer (gt_boxes, gt_labels)", fn);
    if (int rc = shape_ok(fn, a->B, a->M, a->C)) return rc;
    if (a->G > PH_MAXG) return sad::fail(SAD_EUNSUPPORTED, "%s: G = %d boxes per scene (0 .. 1024 supported)", fn, a->G);
    for (int i = 0; i < 3 * a->C; ++i)
        SAD_REQUIRE(a->anchors[i] > 0.0f, "%s: anchor %d has a non-positive extent (%g)", fn, i / 3, (double)a->anchors[i]);
    SAD_REQUIRE(a->size_anchor[0] > 0.0f && a->size_anchor[1] > 0.0f && a->size_anchor[2] > 0.0f, "%s: size_anchor must be positive", fn);
    SAD_REQUIRE(a->shift_max >= 0.0f && a->extra_width >= 0.0f, "%s: need shift_max >= 0 and extra_width >= 0 (got %g, %g)", fn,
                (double)a->shift_max, (double)a->extra_width);
    PtT p = {};
    p.xyz = a->xyz; p.cand = a->cand; p.gt = a->gt_boxes; p.gl = a->gt_labels;
    p.labels = a->labels; p.match = a->match; p.cent = a->centerness; p.shift = a->shift_target; p.size = a->size_target; p.reg = a->reg_target;
    p.M = a->M; p.G = a->G; p.D = a->D; p.C = a->C;
    p.e2 = 2.0f * a->extra_width; p.shift_max = a->shift_max;
    for (int i = 0; i < 3; ++i) p.sa[i] = a->size_anchor[i];
    for (int i = 0; i < 3 * a->C; ++i) p.anchors[i] = a->anchors[i];
    hipLaunchKernelGGL(point_targets_kernel, dim3((unsigned)workgroups(a->M), a->B), dim3(PH_THREADS), 0, (hipStream_t)stream, p);
    return sad::check_launch(fn);
}

SAD_API size_t sad_point_head_loss_workspace_bytes(int B, int M) {
    if (B < 1 || B > 65535 || M < 1 || (long long)B * M >= (1LL << 31)) return 0;
    return (size_t)B * (size_t)workgroups(M) * 4 * sizeof(float);      // (one slot of four partial sums per workgroup of point_loss_kernel)
}

SAD_API int sad_point_head_loss_f32(const sad_point_head_loss_args *a, sad_stream_t stream) {
    const char *fn = "sad_point_head_loss_f32";
    if (int rc = args_ok(fn, a)) return rc;
    SAD_REQUIRE(a->o && a->labels && a->reg_target && a->loss && a->num_pos && a->grad_o && a->workspace, "%s: NULL pointer", fn);
    SAD_REQUIRE(a->c || (!a->shift_target && !a->size_target), "%s: shift_target / size_target given without c", fn);
    SAD_REQUIRE(!a->c || a->shift_target || a->size_target, "%s: c given without shift_target or size_target", fn);
    SAD_REQUIRE((a->c == nullptr) == (a->grad_c == nullptr), "%s: grad_c must be given iff c is", fn);
    SAD_REQUIRE(a->cls_loss == SAD_POINT_CLS_BCE || a->cls_loss == SAD_POINT_CLS_FOCAL, "%s: cls_loss must be SAD_POINT_CLS_BCE or SAD_POINT_CLS_FOCAL (got %d)", fn, a->cls_loss);
    SAD_REQUIRE(a->beta > 0.0f, "%s: need beta > 0 (got %g)", fn, (double)a->beta);
    SAD_REQUIRE(a->alpha >= 0.0f && a->alpha <= 1.0f, "%s: need 0 <= alpha <= 1 (got %g)", fn, (double)a->alpha);
    SAD_REQUIRE(!a->shift_target || a->shift_max >= 0.0f, "%s: need shift_max >= 0 (got %g)", fn, (double)a->shift_max);
    if (int rc = shape_ok(fn, a->B, a->M, a->C)) return rc;
    PtL p = {};
    p.o = a->o; p.c = a->c; p.cent = a->centerness; p.tgt = a->reg_target; p.sht = a->shift_target; p.szt = a->size_target;
    p.labels = a->labels; p.num_pos = a->num_pos;
    p.go = a->grad_o; p.gc = a->grad_c; p.per = a->per_point; p.part = (float *)a->workspace;
    p.M = a->M; p.C = a->C; p.focal = a->cls_loss == SAD_POINT_CLS_FOCAL; p.normalize = a->normalize != 0;
    p.alpha = a->alpha; p.oma = 1.0f - a->alpha; p.beta = a->beta; p.shift_max = a->shift_max;
    for (int j = 0; j < 7; ++j) p.cw[j] = a->code_weights[j];
    for (int i = 0; i < 4; ++i) p.scale[i] = a->scale[i];
    const hipStream_t st = (hipStream_t)stream;
    const int nwg = workgroups(a->M);
    if (hipMemsetAsync(a->num_pos, 0, (size_t)a->B * sizeof(int32_t), st) != hipSuccess) return sad::check_launch(fn);
    hipLaunchKernelGGL(count_pos_kernel, dim3((unsigned)(((long long)a->M + CNT * 256 - 1) / (CNT * 256)), a->B), dim3(256), 0, st, a->labels, a->M, a->num_pos);
    if (int rc = sad::check_launch(fn)) return rc;
    hipLaunchKernelGGL(point_loss_kernel, dim3((unsigned)nwg, a->B), dim3(PH_THREADS), 0, st, p);
    if (int rc = sad::check_launch(fn)) return rc;
    FinP f = {};
    for (int i = 0; i < 4; ++i) { f.src[i] = p.part + i; f.n[i] = nwg; f.stride[i] = 4; }
    f.ncomp = 4; f.loss = a->loss;
    hipLaunchKernelGGL(finish_kernel, dim3(a->B), dim3(64), 0, st, f);
    return sad::check_launch(fn);
}
