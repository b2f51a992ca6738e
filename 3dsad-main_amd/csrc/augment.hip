// Training augmentation (SPEC.md §35): the global flip / rotation / scale / translation of a labelled scene (§35.1) and
// ground-truth database sampling (§35.2), both on the device, reproducible from the caller's seed through §17's integer hash.
//
// global_augment   one launch.  Every thread draws its scene's transform itself (seven hashes and one sincos_r), so the points,
//                  the box rows and `params` leave in the same launch: workgroups [0, np) own 256 point rows each, the next ones
//                  256 box rows each, the last ones write params.
// gt_paste         four launches, nothing read back:
//   select         one workgroup per scene.  The valid ground-truth rows are counted per class (LDS integer atomics), the Q
//                  candidate slots are drawn and staged as §13 local corners, centres and areas; the Q x G tests against the
//                  ground truth (tiles of 256 rows) or into the initial removed-words, the Q x Q / 2 tests among live slots fill the
//                  suppression matrix in nms_core.h's layout (row p, word k: whom p suppresses), spread over all threads; one wave
//                  walks the chunks with chunk_decide.  Stores keep, db_index, the merged boxes and labels and, for the point pass,
//                  the accepted boxes' inside() constants, their database entries and the exclusive prefix of their point counts.
//   count          one workgroup per 256 rows of a scene (the workgroup -> scene map is a prefix of ceil(N_b / 256), written by
//                  select).  inside() against the accepted boxes in LDS; the survivors' ballots (one u64 per wave) and the
//                  workgroup's count go to the workspace: the test runs once.
//   scan           one workgroup: exclusive prefixes of the pasted-point counts over scenes and of the survivor counts over
//                  workgroups -> out_offsets.
//   write          survivors go to out_offsets[b] + pasted_b + (survivors of the scene's earlier workgroups) + the rank inside the
//                  workgroup (ballot / popcount): file order kept.  One more workgroup per (scene, accepted rank) copies an
//                  object's rows.  Cp = 4 rows move as one 16-byte load and store.  With params the rows pass xform_point.
// Integer atomics only (LDS, or-ed bits and class counts: no output bit depends on their order), no float atomics.
#include "box_geom.h"
#include <math.h>

namespace {

#include "prims.h"       // u64, readlane_u64, h17
#include "nms_core.h"    // pair_suppresses, chunk_decide

constexpr int AUG_T = 256;
constexpr int AUG_MAXQ = 512, AUG_WORDS = AUG_MAXQ / 64, AUG_MAXC = SAD_PASTE_MAX_CLASSES, AUG_GT = 256;
constexpr int AUG_SCAN_T = 1024;
constexpr unsigned AUG_DRAW_GLOBAL = 0xA0000000u, AUG_DRAW_PASTE = 0xC0000000u;      // §35: index ranges of the draws

// ---- §35.1 the transform --------------------------------------------------------------------------------------------------
struct Xf { bool fx, fy; float th, c, s, sg, tx, ty, tz; };

__device__ __forceinline__ float draw_u(unsigned h) { return (float)(h >> 8) * 5.9604644775390625e-8f; }      // [0, 1), exact
__device__ __forceinline__ float draw_range(unsigned h, float lo, float hi) {
    const float d = hi - lo;
    const float m = draw_u(h) * d;
    return lo + m;
}

struct XfCfg { unsigned seed; int flip_x, flip_y; float rot_lo, rot_hi, sc_lo, sc_hi, tr[3]; };

__device__ __forceinline__ Xf xf_draw(const XfCfg &g, unsigned b) {
    Xf t;
    t.fx = g.flip_x && (h17(g.seed, b, AUG_DRAW_GLOBAL + 0u) >> 31);
    t.fy = g.flip_y && (h17(g.seed, b, AUG_DRAW_GLOBAL + 1u) >> 31);
    t.th = draw_range(h17(g.seed, b, AUG_DRAW_GLOBAL + 2u), g.rot_lo, g.rot_hi);
    sincos_r(t.th, t.s, t.c);
    t.sg = draw_range(h17(g.seed, b, AUG_DRAW_GLOBAL + 3u), g.sc_lo, g.sc_hi);
    t.tx = draw_range(h17(g.seed, b, AUG_DRAW_GLOBAL + 4u), -g.tr[0], g.tr[0]);
    t.ty = draw_range(h17(g.seed, b, AUG_DRAW_GLOBAL + 5u), -g.tr[1], g.tr[1]);
    t.tz = draw_range(h17(g.seed, b, AUG_DRAW_GLOBAL + 6u), -g.tr[2], g.tr[2]);
    return t;
}
__device__ __forceinline__ void xf_store(const Xf &t, float *p) {
    p[0] = (float)((int)t.fx + 2 * (int)t.fy); p[1] = t.th; p[2] = t.c; p[3] = t.s; p[4] = t.sg; p[5] = t.tx; p[6] = t.ty; p[7] = t.tz;
}
__device__ __forceinline__ Xf xf_load(const float *p) {
    Xf t;
    const int f = (int)p[0];
    t.fx = f & 1; t.fy = (f >> 1) & 1;
    t.th = p[1]; t.c = p[2]; t.s = p[3]; t.sg = p[4]; t.tx = p[5]; t.ty = p[6]; t.tz = p[7];
    return t;
}
// flip, rotate, scale of a vector's x, y (a velocity stops here)
__device__ __forceinline__ void xform_vec(const Xf &t, float &x, float &y) {
    if (t.fx) y = -y;
    if (t.fy) x = -x;
    const float a = x * t.c, b = y * t.s;
    const float a2 = x * t.s, b2 = y * t.c;
    x = (a - b) * t.sg;
    y = (a2 + b2) * t.sg;
}
__device__ __forceinline__ void xform_point(const Xf &t, float &x, float &y, float &z) {
    xform_vec(t, x, y);
    x = x + t.tx;
    y = y + t.ty;
    z = (z * t.sg) + t.tz;
}
// one box row of D columns, src -> dst: centre as a point, extents scaled, yaw flipped and turned, a velocity as a vector
__device__ __forceinline__ void xform_box(const Xf &t, const float *src, float *dst, int D, bool vel) {
    float r[9];
#pragma unroll
    for (int j = 0; j < 7; ++j) r[j] = src[j];
    r[7] = vel ? src[7] : 0.0f; r[8] = vel ? src[8] : 0.0f;
    xform_point(t, r[0], r[1], r[2]);
    r[3] = r[3] * t.sg; r[4] = r[4] * t.sg; r[5] = r[5] * t.sg;
    if (t.fx) r[6] = -r[6];
    if (t.fy) r[6] = -(r[6] + 3.14159274f);
    r[6] = r[6] + t.th;
    if (vel) xform_vec(t, r[7], r[8]);
#pragma unroll
    for (int j = 0; j < 7; ++j) dst[j] = r[j];
    for (int j = 7; j < D; ++j) dst[j] = (vel && j == 7) ? r[7] : ((vel && j == 8) ? r[8] : src[j]);
}
// one point row of Cp words, src -> dst, columns 3.. bit copies; !on: a bit copy of the whole row
__device__ __forceinline__ void move_row(bool on, const Xf &t, const float *src, float *dst, int Cp) {
    if (Cp == 4) {
        float4 v = *reinterpret_cast<const float4 *>(src);
        if (on) xform_point(t, v.x, v.y, v.z);
        *reinterpret_cast<float4 *>(dst) = v;
        return;
    }
    float x = src[0], y = src[1], z = src[2];
    if (on) xform_point(t, x, y, z);
    dst[0] = x; dst[1] = y; dst[2] = z;
    for (int j = 3; j < Cp; ++j) dst[j] = src[j];
}

// the last b in [0, B) with tab[b] <= v (tab ascending, tab[0] <= v < tab[B])
__device__ __forceinline__ int scene_of(const int *tab, int B, int v) {
    int lo = 0, hi = B;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tab[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

struct GlobArgs {
    const float *pts, *gt;
    const int32_t *offsets;
    float *pts_out, *gt_out, *params;
    int B, N, total, Cp, G, D, vel;
    unsigned np, nb;                         // workgroups of the point rows, of the box rows
    XfCfg cfg;
};

__global__ __launch_bounds__(AUG_T) void global_augment_kernel(const GlobArgs p) {
    const unsigned blk = blockIdx.x;
    const int tid = threadIdx.x;
    if (blk < p.np) {
        const long long row = (long long)blk * AUG_T + tid;
        int b;
        if (p.offsets) {
            if (row >= p.offsets[p.B] || row < p.offsets[0]) return;
            b = scene_of(p.offsets, p.B, (int)row);
        } else {
            if (row >= p.total) return;
            b = (int)(row / p.N);
        }
        const Xf t = xf_draw(p.cfg, (unsigned)b);
        move_row(true, t, p.pts + (size_t)row * p.Cp, p.pts_out + (size_t)row * p.Cp, p.Cp);
    } else if (blk < p.np + p.nb) {
        const long long row = (long long)(blk - p.np) * AUG_T + tid;
        if (row >= (long long)p.B * p.G) return;
        const Xf t = xf_draw(p.cfg, (unsigned)(row / p.G));
        xform_box(t, p.gt + (size_t)row * p.D, p.gt_out + (size_t)row * p.D, p.D, p.vel);
    } else {
        const int b = (int)(blk - p.np - p.nb) * AUG_T + tid;
        if (b >= p.B) return;
        xf_store(xf_draw(p.cfg, (unsigned)b), p.params + (size_t)b * 8);
    }
}

// ---- §35.2 gt_paste ---------------------------------------------------------------------------------------------------------
// The workspace.  Per scene (PasteWs::scene): n_acc, pasted rows | acc_start [Q] | acc_db [Q] | consts [Q][8].  Then bs [B + 1]
// (first workgroup of a scene), ppre [B + 1] (pasted rows of the scenes before), excl [NB + 1] (survivors of the workgroups before;
// holds the counts until the scan), mask [NB][4] u64 (the survivors' ballots).
struct PasteWs {
    unsigned char *base;
    int B, Q, NB;
    __host__ __device__ static size_t scene_bytes(int Q) { return sad::al16(8 + (size_t)Q * 8 + (size_t)Q * 32); }
    __host__ __device__ size_t off_bs() const { return (size_t)B * scene_bytes(Q); }
    __host__ __device__ size_t off_ppre() const { return off_bs() + sad::al16((size_t)(B + 1) * 4); }
    __host__ __device__ size_t off_excl() const { return off_ppre() + sad::al16((size_t)(B + 1) * 4); }
    __host__ __device__ size_t off_mask() const { return off_excl() + sad::al16((size_t)(NB + 1) * 4); }
    __host__ __device__ size_t bytes() const { return off_mask() + (size_t)NB * 32; }
    __device__ int *hdr(int b) const { return (int *)(base + (size_t)b * scene_bytes(Q)); }
    __device__ int *acc_start(int b) const { return hdr(b) + 2; }
    __device__ int *acc_db(int b) const { return hdr(b) + 2 + Q; }
    __device__ float *consts(int b) const { return (float *)(hdr(b) + 2 + 2 * Q); }
    __device__ int *bs() const { return (int *)(base + off_bs()); }
    __device__ int *ppre() const { return (int *)(base + off_ppre()); }
    __device__ int *excl() const { return (int *)(base + off_excl()); }
    __device__ u64 *mask() const { return (u64 *)(base + off_mask()); }
};

struct PasteArgs {
    const float *pts, *gt, *dbp, *dbb, *params;
    const int32_t *offsets, *gl, *dbo;
    int32_t *keep, *dbi, *lout, *npasted, *ooff;
    float *bout, *pout;
    PasteWs ws;
    int B, Cp, G, D, C, Q, Pmax, vel;
    unsigned seed;
    float e;
    int coff[AUG_MAXC + 1], snum[AUG_MAXC], base[AUG_MAXC + 1];
};

__device__ __forceinline__ int obj_rows(const PasteArgs &p, int d) { return min(p.dbo[d + 1] - p.dbo[d], p.Pmax); }

__global__ __launch_bounds__(AUG_T) void paste_select_kernel(const PasteArgs p) {
    __shared__ float s_cx[AUG_MAXQ][4], s_cy[AUG_MAXQ][4], s_ctr[AUG_MAXQ][2], s_area[AUG_MAXQ];
    __shared__ float g_cx[AUG_GT][4], g_cy[AUG_GT][4], g_ctr[AUG_GT][2], g_area[AUG_GT];
    __shared__ int g_ok[AUG_GT];
    __shared__ int s_d[AUG_MAXQ], s_pc[AUG_MAXQ];
    __shared__ u64 s_mask[AUG_MAXQ][AUG_WORDS];
    __shared__ u64 s_rem[AUG_WORDS], s_kept[AUG_WORDS];
    __shared__ float s_poly[4 * 10 * AUG_T];           // per-thread clipping scratch, thread-interleaved
    __shared__ int s_cnt[AUG_MAXC], s_blk;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Q = p.Q, G = p.G, D = p.D;
    const float *gt = p.gt + (size_t)b * G * D;
    const int32_t *gl = p.gl + (size_t)b * G;

    if (tid < AUG_MAXC) s_cnt[tid] = 0;
    if (tid < AUG_WORDS) { s_rem[tid] = 0ull; s_kept[tid] = 0ull; }
    if (tid == 0) s_blk = 0;
    for (int i = tid; i < Q * AUG_WORDS; i += AUG_T) (&s_mask[0][0])[i] = 0ull;
    __syncthreads();
    // ---- cnt_b(c): the valid ground-truth rows per class; the scene's first workgroup of the point pass
    for (int g = tid; g < G; g += AUG_T) {
        const int cls = gl[g];
        if (gt_row_valid(cls, p.C, gt + (size_t)g * D)) atomicAdd(&s_cnt[cls], 1);
    }
    {
        int nb = 0;
        for (int s = tid; s < b; s += AUG_T) nb += (p.offsets[s + 1] - p.offsets[s] + AUG_T - 1) / AUG_T;
        if (nb) atomicAdd(&s_blk, nb);
    }
    __syncthreads();
    if (tid == 0) {
        p.ws.bs()[b] = s_blk;
        if (b == p.B - 1) p.ws.bs()[p.B] = s_blk + (p.offsets[b + 1] - p.offsets[b] + AUG_T - 1) / AUG_T;
    }
    // ---- the candidate slots
    for (int q = tid; q < Q; q += AUG_T) {
        int c = 0;
        while (q >= p.base[c + 1]) ++c;                 // (q < Q = base[C])
        const int j = q - p.base[c], nc = p.coff[c + 1] - p.coff[c];
        const bool active = nc > 0 && j < p.snum[c] - s_cnt[c];
        int d = -1;
        if (active) {
            d = p.coff[c] + (int)(h17(p.seed, (unsigned)b, AUG_DRAW_PASTE + (unsigned)q) % (unsigned)nc);
            box_footprint(p.dbb + (size_t)d * D, s_cx[q], s_cy[q], s_ctr[q], s_area[q]);
        } else {
            atomicOr(&s_rem[q >> 6], 1ull << (q & 63));
        }
        s_d[q] = d;
        p.dbi[(size_t)b * Q + q] = d;
    }
    __syncthreads();
    // ---- candidates against the ground truth: a hit removes the slot before the walk
    for (int g0 = 0; g0 < G; g0 += AUG_GT) {
        const int tn = min(AUG_GT, G - g0);
        if (tid < tn) {
            const int g = g0 + tid, cls = gl[g];
            const float *r = gt + (size_t)g * D;
            const bool ok = gt_row_valid(cls, p.C, r);
            g_ok[tid] = ok;
            if (ok) box_footprint(r, g_cx[tid], g_cy[tid], g_ctr[tid], g_area[tid]);
        }
        __syncthreads();
        for (int i = tid; i < Q * tn; i += AUG_T) {
            const int q = i / tn, g = i - q * tn;
            if (s_d[q] < 0 || !g_ok[g]) continue;
            if (pair_suppresses<AUG_T>(s_cx[q], s_cy[q], s_ctr[q], s_area[q], g_cx[g], g_cy[g], g_ctr[g], g_area[g], 0.0f, s_poly + tid))
                atomicOr(&s_rem[q >> 6], 1ull << (q & 63));
        }
        __syncthreads();
    }
    // ---- live slots among themselves: row p, word k, bit l = slot 64k + l (later than p) collides with p
    for (int i = tid; i < Q * Q; i += AUG_T) {
        const int pr = i / Q, q = i - pr * Q;
        if (q <= pr || ((s_rem[pr >> 6] >> (pr & 63)) & 1ull) || ((s_rem[q >> 6] >> (q & 63)) & 1ull)) continue;
        if (pair_suppresses<AUG_T>(s_cx[q], s_cy[q], s_ctr[q], s_area[q], s_cx[pr], s_cy[pr], s_ctr[pr], s_area[pr], 0.0f, s_poly + tid))
            atomicOr(&s_mask[pr][q >> 6], 1ull << (q & 63));
    }
    __syncthreads();
    // ---- the greedy walk in slot order, 64 slots at a time (wave 0; every wave takes the barriers)
    const int nch = (Q + 63) >> 6;
    for (int c = 0; c < nch; ++c) {
        if (wave == 0) {
            const int pr = 64 * c + lane;
            const u64 own = pr < Q ? s_mask[pr][c] : 0ull;
            const u64 kept = chunk_decide(own, Q, c, s_rem[c]);
            if (lane == 0) s_kept[c] = kept;
            if ((kept >> lane) & 1ull) {
                for (int k = c + 1; k < nch; ++k) {
                    const u64 wk = s_mask[pr][k];
                    if (wk) atomicOr(&s_rem[k], wk);
                }
            }
        }
        __syncthreads();
    }
    // ---- results
    for (int q = tid; q < Q; q += AUG_T) {
        const bool k = (s_kept[q >> 6] >> (q & 63)) & 1ull;
        p.keep[(size_t)b * Q + q] = k;
        s_pc[q] = k ? obj_rows(p, s_d[q]) : 0;
    }
    __syncthreads();
    int nacc = 0;
    for (int k = 0; k < nch; ++k) nacc += __popcll(s_kept[k]);
    const Xf *tp = nullptr;
    Xf t;
    if (p.params) { t = xf_load(p.params + (size_t)b * 8); tp = &t; }
    float *bo = p.bout + (size_t)b * (G + Q) * D;
    int32_t *lo = p.lout + (size_t)b * (G + Q);
    for (int q = tid; q < Q; q += AUG_T) {
        if (!((s_kept[q >> 6] >> (q & 63)) & 1ull)) continue;
        int rank = __popcll(s_kept[q >> 6] & ((1ull << (q & 63)) - 1ull)), start = 0;
        for (int k = 0; k < (q >> 6); ++k) rank += __popcll(s_kept[k]);
        for (int i = 0; i < q; ++i) start += s_pc[i];
        const int d = s_d[q];
        const float *row = p.dbb + (size_t)d * D;
        p.ws.acc_start(b)[rank] = start;
        p.ws.acc_db(b)[rank] = d;
        float *k8 = p.ws.consts(b) + (size_t)rank * 8;
        // BoxK's fields in its order, box_consts written out
        float s, c;
        sincos_r(row[6], s, c);
        const float e2 = 2.0f * p.e;
        k8[0] = row[0]; k8[1] = row[1]; k8[2] = row[2];
        k8[3] = 0.5f * (row[3] + e2); k8[4] = 0.5f * (row[4] + e2); k8[5] = 0.5f * (row[5] + e2);
        k8[6] = c; k8[7] = s;
        int cls = 0;
        while (q >= p.base[cls + 1]) ++cls;
        float *dst = bo + (size_t)(G + rank) * D;
        if (tp) xform_box(t, row, dst, D, p.vel);
        else for (int j = 0; j < D; ++j) dst[j] = row[j];
        lo[G + rank] = cls;
    }
    if (tid == 0) {
        int tot = 0;
        for (int i = 0; i < Q; ++i) tot += s_pc[i];
        p.ws.hdr(b)[0] = nacc;
        p.ws.hdr(b)[1] = tot;
        p.npasted[b] = nacc;
    }
    for (int r = nacc + tid; r < Q; r += AUG_T) {       // the rows behind the accepted ones: zero, label -1
        float *dst = bo + (size_t)(G + r) * D;
        if (tp) {
            float z[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, o[9];
            xform_box(t, z, o, min(D, 9), p.vel);
            for (int j = 0; j < D; ++j) dst[j] = j < 9 ? o[j] : 0.0f;
        } else {
            for (int j = 0; j < D; ++j) dst[j] = 0.0f;
        }
        lo[G + r] = -1;
    }
    for (int g = tid; g < G; g += AUG_T) {              // the scene's own rows
        const float *row = gt + (size_t)g * D;
        float *dst = bo + (size_t)g * D;
        if (tp) xform_box(t, row, dst, D, p.vel);
        else for (int j = 0; j < D; ++j) dst[j] = row[j];
        lo[g] = gl[g];
    }
}

// the scene and the first row of workgroup `id` of the point pass; false: a surplus workgroup
__device__ __forceinline__ bool paste_block(const PasteArgs &p, int id, int &b, int &row0, int &rows) {
    const int *bs = p.ws.bs();
    if (id >= bs[p.B]) return false;
    b = scene_of(bs, p.B, id);
    row0 = p.offsets[b] + (id - bs[b]) * AUG_T;
    rows = min(AUG_T, p.offsets[b + 1] - row0);
    return true;
}

__global__ __launch_bounds__(AUG_T) void paste_count_kernel(const PasteArgs p) {
    __shared__ float s_k[AUG_MAXQ * 8];
    __shared__ int s_w[AUG_T / 64];
    const int id = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int b, row0, rows;
    if (!paste_block(p, id, b, row0, rows)) {           // (uniform)
        if (tid == 0) p.ws.excl()[id] = 0;
        return;
    }
    const int n = p.ws.hdr(b)[0];
    const float *k8 = p.ws.consts(b);
    for (int i = tid; i < n * 8; i += AUG_T) s_k[i] = k8[i];
    __syncthreads();
    bool surv = tid < rows;
    if (surv) {
        const float *r = p.pts + (size_t)(row0 + tid) * p.Cp;
        const float px = r[0], py = r[1], pz = r[2];
        for (int i = 0; i < n && surv; ++i) {
            const float *k = s_k + i * 8;
            surv = !inside(px, py, pz, k[0], k[1], k[2], k[3], k[4], k[5], k[6], k[7]);
        }
    }
    const u64 m = __ballot(surv);
    if (lane == 0) { p.ws.mask()[(size_t)id * 4 + wave] = m; s_w[wave] = __popcll(m); }
    __syncthreads();
    if (tid == 0) p.ws.excl()[id] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

// exclusive prefix of v[0 .. n) in place, v[n] = the total; one workgroup of AUG_SCAN_T threads, each owning a run of v
__device__ void block_excl_scan(int *v, int n, int *s_sum) {
    const int tid = threadIdx.x;
    const int seg = (n + AUG_SCAN_T - 1) / AUG_SCAN_T;
    const int lo = min(tid * seg, n), hi = min(lo + seg, n);
    int sum = 0;
    for (int i = lo; i < hi; ++i) sum += v[i];
    s_sum[tid] = sum;
    __syncthreads();
    for (int off = 1; off < AUG_SCAN_T; off <<= 1) {
        const int add = tid >= off ? s_sum[tid - off] : 0;
        __syncthreads();
        s_sum[tid] += add;
        __syncthreads();
    }
    int run = s_sum[tid] - sum;
    for (int i = lo; i < hi; ++i) { const int x = v[i]; v[i] = run; run += x; }
    if (tid == AUG_SCAN_T - 1) v[n] = s_sum[tid];
    __syncthreads();
}

__global__ __launch_bounds__(AUG_SCAN_T) void paste_scan_kernel(const PasteArgs p) {
    __shared__ int s_sum[AUG_SCAN_T];
    int *ppre = p.ws.ppre(), *excl = p.ws.excl();
    for (int b = threadIdx.x; b < p.B; b += AUG_SCAN_T) ppre[b] = p.ws.hdr(b)[1];
    __syncthreads();
    block_excl_scan(ppre, p.B, s_sum);
    block_excl_scan(excl, p.ws.NB, s_sum);
    const int *bs = p.ws.bs();
    for (int b = threadIdx.x; b <= p.B; b += AUG_SCAN_T) p.ooff[b] = ppre[b] + excl[bs[b]];
}

__global__ __launch_bounds__(AUG_T) void paste_write_kernel(const PasteArgs p) {
    const int id = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    Xf t = {};
    const bool on = p.params != nullptr;
    if (id < p.ws.NB) {                                  // survivors of 256 scene rows, file order kept
        int b, row0, rows;
        if (!paste_block(p, id, b, row0, rows)) return;
        const u64 *mk = p.ws.mask() + (size_t)id * 4;
        const u64 m = mk[wave];
        if (!((m >> lane) & 1ull)) return;
        int rank = __popcll(m & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) rank += __popcll(mk[w]);
        const int *excl = p.ws.excl();
        const size_t dst = (size_t)p.ooff[b] + p.ws.hdr(b)[1] + (excl[id] - excl[p.ws.bs()[b]]) + rank;
        if (on) t = xf_load(p.params + (size_t)b * 8);
        move_row(on, t, p.pts + (size_t)(row0 + tid) * p.Cp, p.pout + dst * p.Cp, p.Cp);
        return;
    }
    const int o = id - p.ws.NB, b = o / p.Q, r = o - b * p.Q;      // the object of accepted rank r
    if (r >= p.ws.hdr(b)[0]) return;
    const int d = p.ws.acc_db(b)[r], n = obj_rows(p, d);
    const size_t src = (size_t)p.dbo[d], dst = (size_t)p.ooff[b] + p.ws.acc_start(b)[r];
    if (on) t = xf_load(p.params + (size_t)b * 8);
    for (int i = tid; i < n; i += AUG_T) move_row(on, t, p.dbp + (src + i) * p.Cp, p.pout + (dst + i) * p.Cp, p.Cp);
}

int paste_blocks(int B, int total) { return (total + AUG_T - 1) / AUG_T + B; }

}  // namespace

SAD_API int sad_global_augment_f32(const sad_global_augment_args *a, sad_stream_t stream) {
    const char *fn = "sad_global_augment_f32";
    if (int rc = args_ok(fn, a)) return rc;
    SAD_REQUIRE(a->B >= 1 && a->B <= 65535, "%s: need 1 <= B <= 65535 (got %d)", fn, a->B);
    SAD_REQUIRE(a->total >= 0 && a->Cp >= 3, "%s: need total >= 0 and Cp >= 3 (got %d, %d)", fn, a->total, a->Cp);
    SAD_REQUIRE(a->offsets || (a->N >= 0 && (long long)a->B * a->N == a->total), "%s: without offsets total must be B * N", fn);
    SAD_REQUIRE(a->G >= 0 && a->G <= 1024, "%s: need 0 <= G <= 1024 (got %d)", fn, a->G);
    SAD_REQUIRE(a->G == 0 || a->D >= 7, "%s: box rows have D = %d columns (need D >= 7)", fn, a->D);
    SAD_REQUIRE(!a->with_velocity || a->D >= 9, "%s: with_velocity needs D >= 9 (got %d)", fn, a->D);
    SAD_REQUIRE(a->params && (a->total == 0 || (a->points && a->points_out)) && (a->G == 0 || (a->gt_boxes && a->boxes_out)), "%s: NULL pointer", fn);
    SAD_REQUIRE(a->scale_lo > 0.0f && a->scale_hi >= a->scale_lo, "%s: need 0 < scale_lo <= scale_hi", fn);
    SAD_REQUIRE(a->rot_hi >= a->rot_lo && fabsf(a->rot_lo) < 1e4f && fabsf(a->rot_hi) < 1e4f, "%s: need rot_lo <= rot_hi, both below 1e4 in magnitude", fn);
    SAD_REQUIRE(a->translate[0] >= 0.0f && a->translate[1] >= 0.0f && a->translate[2] >= 0.0f, "%s: translate must be >= 0", fn);
    SAD_REQUIRE(a->Cp != 4 || ((uintptr_t)a->points % 16 == 0 && (uintptr_t)a->points_out % 16 == 0), "%s: rows of 4 columns must be 16-byte aligned", fn);
    GlobArgs p = {};
    p.pts = a->points; p.gt = a->gt_boxes; p.offsets = a->offsets;
    p.pts_out = a->points_out; p.gt_out = a->boxes_out; p.params = a->params;
    p.B = a->B; p.N = a->N > 0 ? a->N : 1; p.total = a->total; p.Cp = a->Cp; p.G = a->G; p.D = a->D; p.vel = a->with_velocity != 0;
    p.np = sad::blocks_for((unsigned long long)a->total, AUG_T);
    p.nb = sad::blocks_for((unsigned long long)a->B * a->G, AUG_T);
    p.cfg.seed = a->seed; p.cfg.flip_x = a->flip_x != 0; p.cfg.flip_y = a->flip_y != 0;
    p.cfg.rot_lo = a->rot_lo; p.cfg.rot_hi = a->rot_hi; p.cfg.sc_lo = a->scale_lo; p.cfg.sc_hi = a->scale_hi;
    for (int k = 0; k < 3; ++k) p.cfg.tr[k] = a->translate[k];
    hipLaunchKernelGGL(global_augment_kernel, dim3(p.np + p.nb + sad::blocks_for(a->B, AUG_T)), dim3(AUG_T), 0, (hipStream_t)stream, p);
    return sad::check_launch(fn);
}

SAD_API size_t sad_gt_paste_workspace_bytes(int B, int Q, int total) {
    if (B < 1 || B > 65535 || Q < 1 || Q > AUG_MAXQ || total < 0) return 0;
    PasteWs w = {nullptr, B, Q, paste_blocks(B, total)};
    return w.bytes();
}

SAD_API int sad_gt_paste_f32(const sad_gt_paste_args *a, sad_stream_t stream) {
    const char *fn = "sad_gt_paste_f32";
    if (int rc = args_ok(fn, a)) return rc;
    SAD_REQUIRE(a->B >= 1 && a->B <= 65535, "%s: need 1 <= B <= 65535 (got %d)", fn, a->B);
    SAD_REQUIRE(a->total >= 0 && a->Cp >= 3, "%s: need total >= 0 and Cp >= 3 (got %d, %d)", fn, a->total, a->Cp);
    SAD_REQUIRE(a->G >= 0 && a->G <= 1024, "%s: need 0 <= G <= 1024 (got %d)", fn, a->G);
    SAD_REQUIRE(a->D >= 7, "%s: box rows have D = %d columns (need D >= 7)", fn, a->D);
    SAD_REQUIRE(!a->with_velocity || a->D >= 9, "%s: with_velocity needs D >= 9 (got %d)", fn, a->D);
    SAD_REQUIRE(a->C >= 1 && a->C <= AUG_MAXC, "%s: need 1 <= C <= %d classes (got %d)", fn, AUG_MAXC, a->C);
    SAD_REQUIRE(a->Ndb >= 1 && a->max_obj_points >= 0, "%s: need Ndb >= 1 and max_obj_points >= 0", fn);
    long long Q = 0;
    SAD_REQUIRE(a->class_offsets[0] == 0 && a->class_offsets[a->C] == a->Ndb, "%s: class_offsets must run from 0 to Ndb", fn);
    for (int c = 0; c < a->C; ++c) {
        SAD_REQUIRE(a->class_offsets[c + 1] >= a->class_offsets[c], "%s: class_offsets must ascend", fn);
        SAD_REQUIRE(a->sample_num[c] >= 0 && a->sample_num[c] <= 65536, "%s: sample_num[%d] = %d", fn, c, a->sample_num[c]);
        Q += a->sample_num[c];
    }
    SAD_REQUIRE(Q >= 1, "%s: no candidate slot (the sum of sample_num is 0)", fn);
    if (Q > AUG_MAXQ) return sad::fail(SAD_EUNSUPPORTED, "%s: Q=%lld candidate slots > %d", fn, Q, AUG_MAXQ);
    SAD_REQUIRE(a->remove_extra_width >= 0.0f, "%s: remove_extra_width must be >= 0", fn);
    const long long need = (long long)a->total + (long long)a->B * Q * a->max_obj_points;
    SAD_REQUIRE(a->R >= need, "%s: out_points has %lld rows, needs total + B*Q*max_obj_points = %lld", fn, a->R, need);
    if (need >= (1ll << 31) / a->Cp) return sad::fail(SAD_EUNSUPPORTED, "%s: %lld output rows of %d columns pass 2^31 words", fn, need, a->Cp);
    SAD_REQUIRE(a->offsets && a->db_points && a->db_offsets && a->db_boxes && a->keep && a->db_index && a->boxes_out && a->labels_out
                && a->num_pasted && a->out_points && a->out_offsets && a->workspace && (a->total == 0 || a->points)
                && (a->G == 0 || (a->gt_boxes && a->gt_labels)), "%s: NULL pointer", fn);
    SAD_REQUIRE((uintptr_t)a->workspace % 16 == 0, "%s: workspace must be 16-byte aligned", fn);
    SAD_REQUIRE(a->Cp != 4 || ((uintptr_t)a->points % 16 == 0 && (uintptr_t)a->db_points % 16 == 0 && (uintptr_t)a->out_points % 16 == 0),
                "%s: rows of 4 columns must be 16-byte aligned", fn);
    PasteArgs p = {};
    p.pts = a->points; p.gt = a->gt_boxes; p.dbp = a->db_points; p.dbb = a->db_boxes; p.params = a->params;
    p.offsets = a->offsets; p.gl = a->gt_labels; p.dbo = a->db_offsets;
    p.keep = a->keep; p.dbi = a->db_index; p.lout = a->labels_out; p.npasted = a->num_pasted; p.ooff = a->out_offsets;
    p.bout = a->boxes_out; p.pout = a->out_points;
    p.B = a->B; p.Cp = a->Cp; p.G = a->G; p.D = a->D; p.C = a->C; p.Q = (int)Q; p.Pmax = a->max_obj_points; p.vel = a->with_velocity != 0;
    p.seed = a->seed; p.e = a->remove_extra_width;
    p.ws = PasteWs{(unsigned char *)a->workspace, a->B, (int)Q, paste_blocks(a->B, a->total)};
    for (int c = 0; c < a->C; ++c) { p.coff[c] = a->class_offsets[c]; p.snum[c] = a->sample_num[c]; p.base[c + 1] = p.base[c] + a->sample_num[c]; }
    p.coff[a->C] = a->class_offsets[a->C];
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(paste_select_kernel, dim3(a->B), dim3(AUG_T), 0, st, p);
    hipLaunchKernelGGL(paste_count_kernel, dim3(p.ws.NB), dim3(AUG_T), 0, st, p);
    hipLaunchKernelGGL(paste_scan_kernel, dim3(1), dim3(AUG_SCAN_T), 0, st, p);
    hipLaunchKernelGGL(paste_write_kernel, dim3(p.ws.NB + a->B * (int)Q), dim3(AUG_T), 0, st, p);
    return sad::check_launch(fn);
}
