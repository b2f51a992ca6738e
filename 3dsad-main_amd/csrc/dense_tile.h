// What dense_head.hip (§25), dense_target.hip (§26) and dense_loss.hip (§27) share, one definition each: the anchor tile (device side
// and launch grid), the anchor table with the residual coder, map indexing, the tile-image copies and the host checks.  Included
// inside each file's anonymous namespace, after common.h, like prims.h (which it includes).
#pragma once
#include "prims.h"

// threads per workgroup; cells and anchors of an anchor tile; class logits per staged chunk (nhwc); ground-truth boxes per scene
constexpr int DENSE_THREADS = 256, TC = 64, AC = 8, CCH = 8, MAXG = 1024;
// element (b, ch, cell) of a map with CH channels
__device__ __forceinline__ size_t map_at(int nhwc, int b, int ch, int cell, int CH, int HW) {
    return nhwc ? ((size_t)b * HW + cell) * CH + ch : ((size_t)b * CH + ch) * HW + cell;
}

// ---- tile image <-> memory ---------------------------------------------------------------------------------------------------
// The rows of a tile move through an LDS image in memory order: `ncell` spans of `seg` elements, span c at mem[c * stride], back to
// back in the image.  All threads call these; consecutive threads touch consecutive elements.  When one chunk of anchors covers the
// row (seg == stride) the tile is a single run and no index is divided.
template <class T> __device__ __forceinline__ void flush_spans(const T *img, T *dst, int ncell, int seg, size_t stride) {
    const int n = ncell * seg;
    if ((size_t)seg == stride)
        for (int i = threadIdx.x; i < n; i += DENSE_THREADS) dst[i] = img[i];
    else
        for (int i = threadIdx.x; i < n; i += DENSE_THREADS) dst[(size_t)(i / seg) * stride + i % seg] = img[i];
}
template <class T> __device__ __forceinline__ void load_spans(T *img, const T *src, int ncell, int seg, size_t stride) {
    const int n = ncell * seg;
    if ((size_t)seg == stride)
        for (int i = threadIdx.x; i < n; i += DENSE_THREADS) img[i] = src[i];
    else
        for (int i = threadIdx.x; i < n; i += DENSE_THREADS) img[i] = src[(size_t)(i / seg) * stride + i % seg];
}

// ---- the anchor tile ---------------------------------------------------------------------------------------------------------
// A workgroup owns 64 cells x up to 8 anchors of scene b: lane = cell, wave + 4 * pass = anchor; blockIdx.x = tile * chunks +
// chunk.  Rows k = cell * A + a: the tile's rows are `ncell` spans of `acn` rows, A rows apart, the first at k0().  By value.
struct AnchorTile {
    int b, HW, A, cell0, ncell, a0, acn, lane, wave;
    __device__ __forceinline__ size_t k0() const { return ((size_t)b * HW + cell0) * A + a0; }
    // of a pass: the thread's anchor in the chunk, has it a row, its place in a tile image, first anchor, anchors; then rows[B, K, w] <-> image
    __device__ __forceinline__ int al(int pass) const { return 4 * pass + wave; }
    __device__ __forceinline__ bool active(int pass) const { return lane < ncell && al(pass) < acn; }
    __device__ __forceinline__ int slot(int pass) const { return lane * acn + al(pass); }
    __device__ __forceinline__ int pa0(int pass) const { return a0 + 4 * pass; }
    __device__ __forceinline__ int na(int pass) const { return min(4, acn - 4 * pass); }
    template <class T> __device__ __forceinline__ void store(const T *img, T *rows, int w) const { flush_spans(img, rows + k0() * w, ncell, acn * w, (size_t)A * w); }
    template <class T> __device__ __forceinline__ void load(T *img, const T *rows, int w) const { load_spans(img, rows + k0() * w, ncell, acn * w, (size_t)A * w); }
};
__device__ __forceinline__ AnchorTile anchor_tile(int chunks, int HW, int A) {
    const int tile = blockIdx.x / chunks, cell0 = tile * TC, a0 = (blockIdx.x - tile * chunks) * AC;
    return {(int)blockIdx.y, HW, A, cell0, min(TC, HW - cell0), a0, min(AC, A - a0), (int)(threadIdx.x & 63), (int)(threadIdx.x >> 6)};
}
// the host side: tiles of a scene, chunks of a tile; returns their product, the workgroups per scene (HW < 2^31: rows_fit)
inline int anchor_grid_of(int HW, int A, int *tiles, int *chunks) {
    *tiles = (int)(((long long)HW + TC - 1) / TC);
    *chunks = (A + AC - 1) / AC;
    return *tiles * *chunks;      // (<= K / 8 + tiles + chunks: far below 2^31)
}
// The channels-last (nhwc) passes of the anchor head: rows (al, cell) of a pass <-> lds[(al * TC + cell) * ld + e], e < len: channels
// ch0 .. ch0 + len - 1 of anchor pa0 + al out of CHA per anchor.  All threads walk the pass in memory order; OUT: back to memory.
// (the tile by reference: by value the nhwc loss kernel spills one SGPR more)
template <bool OUT, class P>
__device__ __forceinline__ void stage_pass(const AnchorTile &t, int pass, float *lds, int ld, P *scene, int CHA, int ch0, int len) {
    const int na = t.na(pass), n = t.ncell * na * len;
    for (int i = threadIdx.x; i < n; i += DENSE_THREADS) {
        const int row = i / len, e = i - row * len, cell = row / na, al = row - cell * na;
        P *g = scene + ((size_t)(t.cell0 + cell) * t.A + t.pa0(pass) + al) * CHA + ch0 + e;
        if constexpr (OUT) *g = lds[(al * TC + cell) * ld + e];
        else lds[(al * TC + cell) * ld + e] = *g;
    }
}

// ---- the anchor table ----------------------------------------------------------------------------------------------------------
// By value in the kernel arguments, copied to LDS once per workgroup (the index path addresses it per lane): tab = sizes[48] |
// z_center[16] | rotations[8]; the target kernels append their per-size entries from T_N on.
constexpr int T_ZC = 48, T_ROT = 64, T_N = 72;
struct AnchorTab { float x0, y0, sx, sy; int W, nr; float sizes[48], zc[16], rot[8]; };
struct Anchor { float xa, ya, za, la, wa, ha, ra; int s; };
__device__ __forceinline__ void load_tab(const AnchorTab &a, float *tab) {      // (the caller synchronises)
    if (const int t = threadIdx.x; t < T_N) tab[t] = t < T_ZC ? a.sizes[t] : t < T_ROT ? a.zc[t - T_ZC] : a.rot[t - T_ROT];
}
__device__ __forceinline__ Anchor anchor_of(const AnchorTab &p, const float *tab, int a, int cell) {      // a = s * nr + r, cell = y * W + x
    const int s = a / p.nr, r = a - s * p.nr;
    const int y = cell / p.W, x = cell - y * p.W;
    return {p.x0 + ((float)x * p.sx), p.y0 + ((float)y * p.sy), tab[T_ZC + s], tab[3 * s], tab[3 * s + 1], tab[3 * s + 2], tab[T_ROT + r], s};
}
// The ResidualCoder and its inverse.  decode: residuals t[7] -> box[7] (box[6] before the direction bin); encode: a ground-truth
// row r -> residuals t[7].  Every operation is one IEEE binary32 operation in this order (the library is built without contraction).
__device__ __forceinline__ float anchor_diag(const Anchor &an) { return sqrtf((an.la * an.la) + (an.wa * an.wa)); }
__device__ __forceinline__ void residual_decode(const Anchor &an, const float *t, float *box) {
    const float dg = anchor_diag(an), scale[3] = {dg, dg, an.ha}, at[3] = {an.xa, an.ya, an.za}, dim[3] = {an.la, an.wa, an.ha};
#pragma unroll
    for (int j = 0; j < 3; ++j) box[j] = (t[j] * scale[j]) + at[j];
#pragma unroll
    for (int j = 0; j < 3; ++j) box[3 + j] = expf(t[3 + j]) * dim[j];
    box[6] = t[6] + an.ra;
}
__device__ __forceinline__ void residual_encode(const Anchor &an, const float *r, float *t) {
    const float dg = anchor_diag(an), scale[3] = {dg, dg, an.ha}, at[3] = {an.xa, an.ya, an.za}, dim[3] = {an.la, an.wa, an.ha};
#pragma unroll
    for (int j = 0; j < 3; ++j) t[j] = (r[j] - at[j]) / scale[j];
#pragma unroll
    for (int j = 0; j < 3; ++j) t[3 + j] = logf(fmaxf(r[3 + j], 1e-5f) / dim[j]);
    t[6] = r[6] - an.ra;
}
// the width of a direction bin: 2 pi / nb in double, rounded once
inline float dir_period(int nb) { return nb ? (float)(6.283185307179586476925286766559 / (double)nb) : 0.0f; }

// ---- host checks ---------------------------------------------------------------------------------------------------------------
// (args_ok, the struct_size check of every argument block: common.h)
// Rows are numbered in int: H * W, K = H * W * A and B * K stay below 2^31 (centre head: A = 1).  B, H, W >= 1 and A <= 128 are checked
// before: H * W < 2^62 is exact, and a product is multiplied further only once it is known to be below 2^31.  The caller words the refusal.
inline bool rows_fit(int B, int H, int W, int A) {
    const long long HW = (long long)H * W, lim = 1LL << 31;
    return HW < lim && HW * A < lim && B * (HW * A) < lim;
}
// the upper limits of the anchor set of sad_anchor_decode_args / _targets_args (same field names); its scalars -> the kernel's block
template <class T> int fill_anchor_tab(const char *fn, const T *a, AnchorTab *tab) {
    if (a->ns > 16 || a->nr > 8 || a->nb > 8)
        return sad::fail(SAD_EUNSUPPORTED, "%s: ns = %d, nr = %d, nb = %d (ns <= 16, nr <= 8, nb <= 8 supported)", fn, a->ns, a->nr, a->nb);
    tab->x0 = a->x0; tab->y0 = a->y0; tab->sx = a->sx; tab->sy = a->sy; tab->W = a->W; tab->nr = a->nr;
    for (int i = 0; i < 3 * a->ns; ++i) tab->sizes[i] = a->sizes[i];
    for (int i = 0; i < a->ns; ++i) tab->zc[i] = a->z_center[i];
    for (int i = 0; i < a->nr; ++i) tab->rot[i] = a->rotations[i];
    return SAD_OK;
}
