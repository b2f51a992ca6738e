// Dense head decode (SPEC.md §25): the raw maps of an anchor head / a centre head -> boxes[B,K,D], scores[B,K], labels[B,K],
// what sad_nms_boxes_f32 takes.  One launch per call, no atomics, every output element stored once.
//
// anchor, dense   a workgroup owns a tile of 64 cells x up to 8 anchors: lane = cell (y * W + x), wave + 4 * pass = anchor (dense_tile.h).
//   nchw          channel planes are unit-stride in the cell, so every load of a wave is 256 contiguous bytes.
//   nhwc          the channels of a cell are contiguous: a pass (64 cells x 4 anchors) is staged through LDS by all 256 threads walking
//                 the floats in memory order (stage_pass; class logits in chunks of 8 classes), and a thread reads its row from LDS.
//   output        rows k = cell * A + a of a tile are one contiguous span (A <= 8) or one span of 8 rows per cell: the thread that decoded
//                 a row puts it into an LDS image, which the workgroup stores in memory order (flush_spans): no stores 28 bytes apart.
// centre, dense   a workgroup owns 256 consecutive cells, one per thread; the 3 x 3 test reads the neighbours where
//                 they are (rows above and below are the same 256-byte spans one row away).
// index           one thread per output row p, 256 consecutive p per workgroup; the row's reads are gathers.
#include "common.h"
#include <math.h>

namespace {

#include "dense_tile.h"

constexpr int MAXD = 9;

struct AncP {
    const float *cls, *reg, *dir;
    const int32_t *index;
    float *boxes, *scores;
    int32_t *labels;
    // (this order keeps the dense kernels' SGPR spills at 42 / 2, nhwc / nchw; others give up to 52: after any change here rerun
    // tools/kernel_resources.py dense_head)
    float dir_limit; int HW, C, tiles, nb, chunks; float dir_offset; int P, A; float period; AnchorTab tab; int nhwc;
};

struct CenP {
    const float *hm, *reg, *height, *dim, *rot, *vel;
    const int32_t *index;
    float *boxes, *scores;
    int32_t *labels;
    int HW, H, W, C, D, P, nhwc, log_dim, peak;
    float lo_x, lo_y, sx, sy;
};

// values straight from memory, either layout
struct AncDirect {
    const AncP &p;
    int b, a, cell;
    __device__ __forceinline__ float reg(int j) const { return p.reg[map_at(p.nhwc, b, a * 7 + j, cell, p.A * 7, p.HW)]; }
    __device__ __forceinline__ float dir(int d) const { return p.dir[map_at(p.nhwc, b, a * p.nb + d, cell, p.A * p.nb, p.HW)]; }
    __device__ __forceinline__ float cls(int c) const { return p.cls[map_at(p.nhwc, b, a * p.C + c, cell, p.A * p.C, p.HW)]; }
};

// values of the thread's row from the staged pass (nhwc).  Every thread of the workgroup makes the same calls: cls() stages
// the next chunk of classes between two barriers.
struct AncStaged {
    const AncP &p;
    float *sreg, *su;
    const float *scene_cls;
    const AnchorTile t;
    int pass;
    __device__ __forceinline__ float reg(int j) const { return sreg[threadIdx.x * 7 + j]; }
    __device__ __forceinline__ float dir(int d) const { return su[threadIdx.x * (CCH + 1) + d]; }
    __device__ __forceinline__ float cls(int c) const {
        if ((c & (CCH - 1)) == 0) {
            __syncthreads();
            stage_pass<false>(t, pass, su, CCH + 1, scene_cls, p.C, c, min(CCH, p.C - c));
            __syncthreads();
        }
        return su[threadIdx.x * (CCH + 1) + (c & (CCH - 1))];
    }
};

// §25.1: one row
template <class F>
__device__ __forceinline__ void anchor_row(const AncP &p, const float *tab, int a, int cell, const F &f, float *box, float &score, int &label) {
    const Anchor an = anchor_of(p.tab, tab, a, cell);
    // every value of the row is fetched before the first is used (logits eight at a time, unrolled): one round trip to memory
    // per row, not one per map and logit
    float t[7], dv[8], cv[CCH];
#pragma unroll
    for (int j = 0; j < 7; ++j) t[j] = f.reg(j);
#pragma unroll
    for (int d = 0; d < 8; ++d) dv[d] = d < p.nb ? f.dir(d) : -INFINITY;
#pragma unroll
    for (int u = 0; u < CCH; ++u) cv[u] = u < p.C ? f.cls(u) : -INFINITY;
    residual_decode(an, t, box);
    if (p.nb) {
        int bin = 0;
        float best = dv[0];
#pragma unroll
        for (int d = 1; d < 8; ++d)
            if (dv[d] > best) { best = dv[d]; bin = d; }      // strict: a tie stays with the lowest bin
        const float v = box[6] - p.dir_offset;
        const float q = floorf((v / p.period) + p.dir_limit);
        const float rot = v - (q * p.period);
        box[6] = (rot + p.dir_offset) + (p.period * (float)bin);
    }
    float m = -INFINITY;
    label = 0;
    for (int c0 = 0;;) {
#pragma unroll
        for (int u = 0; u < CCH; ++u)
            if (cv[u] > m) { m = cv[u]; label = c0 + u; }    // (-inf never wins: a row of -inf logits keeps label 0)
        c0 += CCH;
        if (c0 >= p.C) break;
#pragma unroll
        for (int u = 0; u < CCH; ++u) cv[u] = c0 + u < p.C ? f.cls(c0 + u) : -INFINITY;
    }
    score = 1.0f / (1.0f + expf(-m));
}

template <bool NHWC>
__global__ __launch_bounds__(DENSE_THREADS) void anchor_dense_kernel(const AncP p) {
    __shared__ float tab[T_N];
    __shared__ float obox[TC * AC * 7];
    __shared__ float oscore[TC * AC];
    __shared__ int32_t olabel[TC * AC];
    __shared__ float sreg[NHWC ? DENSE_THREADS * 7 : 1];
    __shared__ float su[NHWC ? DENSE_THREADS * (CCH + 1) : 1];
    load_tab(p.tab, tab);
    __syncthreads();
    const AnchorTile t = anchor_tile(p.chunks, p.HW, p.A);
    for (int pass = 0; 4 * pass < t.acn; ++pass) {
        const bool active = t.active(pass);
        float box[7], score = 0.0f;
        int label = 0;
        if (NHWC) {
            const AncStaged f{p, sreg, su, p.cls + (size_t)t.b * p.HW * p.A * p.C, t, pass};
            __syncthreads();
            stage_pass<false>(t, pass, sreg, 7, p.reg + (size_t)t.b * p.HW * p.A * 7, 7, 0, 7);
            if (p.nb) stage_pass<false>(t, pass, su, CCH + 1, p.dir + (size_t)t.b * p.HW * p.A * p.nb, p.nb, 0, p.nb);
            __syncthreads();
            // (rows that are not active read stale LDS; their results are dropped below)
            anchor_row(p, tab, active ? t.a0 + t.al(pass) : t.a0, active ? t.cell0 + t.lane : t.cell0, f, box, score, label);
        } else if (active) {
            const AncDirect f{p, t.b, t.a0 + t.al(pass), t.cell0 + t.lane};
            anchor_row(p, tab, t.a0 + t.al(pass), t.cell0 + t.lane, f, box, score, label);
        }
        if (active) {
            const int slot = t.slot(pass);
#pragma unroll
            for (int j = 0; j < 7; ++j) obox[slot * 7 + j] = box[j];
            oscore[slot] = score;
            olabel[slot] = label;
        }
    }
    __syncthreads();
    t.store(obox, p.boxes, 7);
    t.store(oscore, p.scores, 1);
    t.store(olabel, p.labels, 1);
}

// the rows of 256 consecutive output positions, decoded by their threads into rows[], go out in memory order
__device__ __forceinline__ void flush_block(const float *obox, const float *oscore, const int32_t *olabel, float *boxes, float *scores,
                                            int32_t *labels, size_t row0, int n, int D) {
    __syncthreads();
    flush_spans(obox, boxes + row0 * D, 1, n * D, 0);
    flush_spans(oscore, scores + row0, 1, n, 0);
    flush_spans(olabel, labels + row0, 1, n, 0);
}

__global__ __launch_bounds__(DENSE_THREADS) void anchor_index_kernel(const AncP p) {
    __shared__ float tab[T_N];
    __shared__ float obox[DENSE_THREADS * 7];
    __shared__ float oscore[DENSE_THREADS];
    __shared__ int32_t olabel[DENSE_THREADS];
    load_tab(p.tab, tab);
    __syncthreads();
    const int b = blockIdx.y;
    const int p0 = blockIdx.x * DENSE_THREADS, n = min(DENSE_THREADS, p.P - p0);
    const int t = threadIdx.x;
    if (t < n) {
        const int k = p.index[(size_t)b * p.P + p0 + t];
        float box[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, score = -INFINITY;
        int label = -1;
        if (k >= 0 && k < p.HW * p.A) {
            const int cell = k / p.A, a = k - cell * p.A;
            const AncDirect f{p, b, a, cell};
            anchor_row(p, tab, a, cell, f, box, score, label);
        }
#pragma unroll
        for (int j = 0; j < 7; ++j) obox[t * 7 + j] = box[j];
        oscore[t] = score;
        olabel[t] = label;
    }
    flush_block(obox, oscore, olabel, p.boxes, p.scores, p.labels, (size_t)b * p.P + p0, n, 7);
}

// §25.2: one row
__device__ __forceinline__ void center_row(const CenP &p, int b, int cell, float *box, float &score, int &label) {
    const int y = cell / p.W, x = cell - y * p.W;
    const float r0 = p.reg[map_at(p.nhwc, b, 0, cell, 2, p.HW)], r1 = p.reg[map_at(p.nhwc, b, 1, cell, 2, p.HW)];
    box[0] = (((float)x + r0) * p.sx) + p.lo_x;
    box[1] = (((float)y + r1) * p.sy) + p.lo_y;
    box[2] = p.height[(size_t)b * p.HW + cell];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float d = p.dim[map_at(p.nhwc, b, j, cell, 3, p.HW)];
        box[3 + j] = p.log_dim ? expf(d) : d;
    }
    box[6] = atan2f(p.rot[map_at(p.nhwc, b, 0, cell, 2, p.HW)], p.rot[map_at(p.nhwc, b, 1, cell, 2, p.HW)]);
    if (p.vel) {
        box[7] = p.vel[map_at(p.nhwc, b, 0, cell, 2, p.HW)];
        box[8] = p.vel[map_at(p.nhwc, b, 1, cell, 2, p.HW)];
    }
    float m = 0.0f;
    label = -1;
    for (int c0 = 0; c0 < p.C; c0 += CCH) {
        float cv[CCH];                                   // eight logits in flight together (see anchor_row)
#pragma unroll
        for (int u = 0; u < CCH; ++u) cv[u] = c0 + u < p.C ? p.hm[map_at(p.nhwc, b, c0 + u, cell, p.C, p.HW)] : 0.0f;
#pragma unroll
        for (int u = 0; u < CCH; ++u) {
            const int c = c0 + u;
            if (c >= p.C) break;
            const float v = cv[u];
            bool part = true;
            if (p.peak) {
                for (int dy = -1; dy <= 1; ++dy) {
                    const int yy = y + dy;
                    if (yy < 0 || yy >= p.H) continue;
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int xx = x + dx;
                        if (xx < 0 || xx >= p.W || (dy == 0 && dx == 0)) continue;
                        part = part && v >= p.hm[map_at(p.nhwc, b, c, yy * p.W + xx, p.C, p.HW)];
                    }
                }
            }
            if (part && (label < 0 || v > m)) { m = v; label = c; }
        }
    }
    score = label < 0 ? 0.0f : 1.0f / (1.0f + expf(-m));
}

__global__ __launch_bounds__(DENSE_THREADS) void center_kernel(const CenP p) {
    __shared__ float obox[DENSE_THREADS * MAXD];
    __shared__ float oscore[DENSE_THREADS];
    __shared__ int32_t olabel[DENSE_THREADS];
    const int b = blockIdx.y;
    const int n_rows = p.index ? p.P : p.HW;
    const int p0 = blockIdx.x * DENSE_THREADS, n = min(DENSE_THREADS, n_rows - p0);
    const int t = threadIdx.x;
    if (t < n) {
        const int k = p.index ? p.index[(size_t)b * p.P + p0 + t] : p0 + t;
        float box[MAXD] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, score = -INFINITY;
        int label = -1;
        if (k >= 0 && k < p.HW) center_row(p, b, k, box, score, label);
#pragma unroll
        for (int j = 0; j < MAXD; ++j)
            if (j < p.D) obox[t * p.D + j] = box[j];
        oscore[t] = score;
        olabel[t] = label;
    }
    flush_block(obox, oscore, olabel, p.boxes, p.scores, p.labels, (size_t)b * n_rows + p0, n, p.D);
}

// the shape rules both operators share: B, H, W, C, layout, index / P; K = H * W * A
int shape_ok(const char *fn, int B, int H, int W, int C, int A, int layout, const int32_t *index, int P) {
    SAD_REQUIRE(layout == SAD_LAYOUT_NCHW || layout == SAD_LAYOUT_NHWC, "%s: layout must be SAD_LAYOUT_NCHW or SAD_LAYOUT_NHWC (got %d)", fn, layout);
    SAD_REQUIRE(B >= 1 && H >= 1 && W >= 1 && C >= 1, "%s: need B, H, W, C >= 1 (got %d, %d, %d, %d)", fn, B, H, W, C);
    SAD_REQUIRE(index == nullptr || P >= 1, "%s: index needs P >= 1 (got %d)", fn, P);
    if (B > 65535) return sad::fail(SAD_EUNSUPPORTED, "%s: B = %d (1 .. 65535 supported)", fn, B);
    if (C > 64) return sad::fail(SAD_EUNSUPPORTED, "%s: C = %d classes (1 .. 64 supported)", fn, C);
    if (!rows_fit(B, H, W, A)) return sad::fail(SAD_EUNSUPPORTED, "%s: B * K = %d * %lld rows (B * K < 2^31 supported)", fn, B, (long long)H * W * A);
    if (index && (long long)B * P >= (1LL << 31)) return sad::fail(SAD_EUNSUPPORTED, "%s: B * P = %d * %d rows (B * P < 2^31 supported)", fn, B, P);
    return SAD_OK;
}

}  // namespace

SAD_API int sad_anchor_decode_f32(const sad_anchor_decode_args *a, sad_stream_t stream) {
    const char *fn = "sad_anchor_decode_f32";
    if (int rc = args_ok(fn, a)) return rc;
    SAD_REQUIRE(a->cls && a->reg && a->boxes && a->scores && a->labels, "%s: NULL pointer", fn);
    SAD_REQUIRE(a->ns >= 1 && a->nr >= 1, "%s: need ns, nr >= 1 (got %d, %d)", fn, a->ns, a->nr);
    SAD_REQUIRE(a->nb == 0 || a->nb >= 2, "%s: nb must be 0 (no direction map) or 2 .. 8 (got %d)", fn, a->nb);
    SAD_REQUIRE((a->nb == 0) == (a->dir == nullptr), "%s: dir and nb must be given together (nb = %d)", fn, a->nb);
    AncP p = {};
    if (int rc = fill_anchor_tab(fn, a, &p.tab)) return rc;
    const int A = a->ns * a->nr;
    if (int rc = shape_ok(fn, a->B, a->H, a->W, a->C, A, a->layout, a->index, a->P)) return rc;
    p.cls = a->cls; p.reg = a->reg; p.dir = a->dir; p.index = a->index;
    p.boxes = a->boxes; p.scores = a->scores; p.labels = a->labels;
    p.HW = a->H * a->W; p.A = A; p.C = a->C; p.nb = a->nb; p.P = a->P;
    p.nhwc = a->layout == SAD_LAYOUT_NHWC;
    p.dir_offset = a->dir_offset; p.dir_limit = a->dir_limit_offset; p.period = dir_period(a->nb);
    const hipStream_t st = (hipStream_t)stream;
    if (a->index) {
        hipLaunchKernelGGL(anchor_index_kernel, dim3((unsigned)((a->P + DENSE_THREADS - 1) / DENSE_THREADS), a->B), dim3(DENSE_THREADS), 0, st, p);
        return sad::check_launch(fn);
    }
    const dim3 grid((unsigned)anchor_grid_of(p.HW, A, &p.tiles, &p.chunks), a->B);
    if (p.nhwc) hipLaunchKernelGGL(anchor_dense_kernel<true>, grid, dim3(DENSE_THREADS), 0, st, p);
    else hipLaunchKernelGGL(anchor_dense_kernel<false>, grid, dim3(DENSE_THREADS), 0, st, p);
    return sad::check_launch(fn);
}

SAD_API int sad_center_decode_f32(const sad_center_decode_args *a, sad_stream_t stream) {
    const char *fn = "sad_center_decode_f32";
    if (int rc = args_ok(fn, a)) return rc;
    SAD_REQUIRE(a->hm && a->reg && a->height && a->dim && a->rot && a->boxes && a->scores && a->labels, "%s: NULL pointer", fn);
    if (int rc = shape_ok(fn, a->B, a->H, a->W, a->C, 1, a->layout, a->index, a->P)) return rc;
    CenP p = {};
    p.hm = a->hm; p.reg = a->reg; p.height = a->height; p.dim = a->dim; p.rot = a->rot; p.vel = a->vel; p.index = a->index;
    p.boxes = a->boxes; p.scores = a->scores; p.labels = a->labels;
    p.HW = a->H * a->W; p.H = a->H; p.W = a->W; p.C = a->C; p.D = a->vel ? 9 : 7; p.P = a->P;
    p.nhwc = a->layout == SAD_LAYOUT_NHWC;
    p.log_dim = a->log_dim != 0; p.peak = a->peak != 0;
    p.lo_x = a->lo_x; p.lo_y = a->lo_y; p.sx = a->sx; p.sy = a->sy;
    const int rows = a->index ? a->P : p.HW;
    hipLaunchKernelGGL(center_kernel, dim3((unsigned)((rows + DENSE_THREADS - 1) / DENSE_THREADS), a->B), dim3(DENSE_THREADS), 0, (hipStream_t)stream, p);
    return sad::check_launch(fn);
}
