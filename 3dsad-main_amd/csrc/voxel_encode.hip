// Voxel feature encoder (SPEC.md §24): decorate the members of every voxel, one §6 layer, maximum over the voxel.
//
// lists    the ordered member lists of §20.5 (voxel.hip: count, CSR, rank), then mean[B*V,3] by one thread per (voxel, axis)
//          walking its list in ascending row order: the additions of §20.5, one division.
// pack     W[Cout,Cin] -> the A-fragment image of v_mfma_f32_32x32x2_f32 (bias[NP] | [tile][k-group][lane] float4, as
//          mlp_pack.hip), zero padded to 32 channels and 8 inputs; it lives in the workspace, so the entry point takes raw W.
// encode   ONE launch with two kinds of workgroup.
//   tile   wave w of the grid owns the voxels whose list STARTS at a list position in [32 w, 32 w + 32).  It walks 32
//          positions at a time from 32 w until its last voxel ends: lane (j, h) builds the decorated row of position j in
//          registers (the B operand, fed as in mlp_rows.hip), the accumulators start at the bias and k ascends, and the
//          32 x 64 result goes through the wave's own LDS stage so that lane = channel can walk the rows in list order with a
//          running (max, arg) in two registers.  A voxel longer than a tile is carried in those registers into the next
//          tile of the SAME wave, so no partial maximum ever leaves a wave: no atomics, no order to depend on, and each
//          (voxel, channel) is stored once, 256 contiguous bytes per voxel and 64 channels.  One giant voxel is therefore
//          walked by one wave (the waves whose span lies inside it find nothing they own and leave).
//   zero   one thread per (voxel, 4 channels): voxels without members get 0 / arg -1 (and, with pointwise, the rows that
//          are in no list get 0) in the same launch, so no fill pass runs before or after.
// decorate the unfused rows [total, Cin] through the same row_elem(), what the backward and the tests use.
#include "common.h"
#include "voxel_csr.h"
#include <math.h>

namespace {

#include "vox_hash.h"
#include "reg_common.h"

struct EncP {
    const float *points;
    const int32_t *p2v, *offsets, *coors;
    const float *vox_feat, *mean;
    const int32_t *start, *cnt, *sorted;
    const float *wimg;                  // bias[32 CT] | fragments [tile][k-group][lane] float4
    float *pooled;
    int32_t *arg;
    float *pointwise;
    int total, B, C, V, Cv, Cin, Cout, KG, CT, T, cc, vc, relu, vec_pw;
    unsigned nvox, tile_blocks;
    float vs[3], lo[3];
};

// members of all voxels together (the end of the last list)
__device__ __forceinline__ int list_end(const EncP &p) {
    const int m = p.start[p.nvox - 1] + p.cnt[p.nvox - 1];
    return min(max(m, 0), p.total);
}

// column k of the decorated row of member i of voxel s (§24): every operation rounded on its own
__device__ __forceinline__ float row_elem(const EncP &p, int i, unsigned s, int k) {
    const float *pt = p.points + (size_t)i * p.C;
    if (k < p.C) return pt[k];
    k -= p.C;
    if (p.cc) {
        if (k < 3) return pt[k] - p.mean[(size_t)s * 3 + k];
        k -= 3;
    }
    if (p.vc) {
        if (k < 3) {
            const float g = (float)p.coors[(size_t)s * 3 + (2 - k)];        // coors are (z,y,x)
            const float v = k == 0 ? p.vs[0] : k == 1 ? p.vs[1] : p.vs[2];
            const float lo = k == 0 ? p.lo[0] : k == 1 ? p.lo[1] : p.lo[2];
            const float ctr = (g * v) + ((0.5f * v) + lo);
            return pt[k] - ctr;
        }
        k -= 3;
    }
    return k < p.Cv ? p.vox_feat[(size_t)s * p.Cv + k] : 0.0f;
}

struct Member {
    int i;          // global row, -1: no list entry at this position
    unsigned s;     // voxel b * V + v
    int st, rank;   // start of the voxel's list, position inside it
    int n, nn;      // list length, members (the first T of it)
};

__device__ __forceinline__ Member member_at(const EncP &p, int pos, int M) {
    Member m = {-1, 0u, 0, 0, 0, 0};
    if (pos >= M) return m;
    const int i = p.sorted[pos];
    if (i < 0 || i >= p.total) return m;
    const int v = p.p2v[i];
    if (v < 0 || v >= p.V) return m;
    m.s = (unsigned)scene_of(p.offsets, p.B, i) * (unsigned)p.V + (unsigned)v;
    m.st = p.start[m.s];
    m.n = min(p.cnt[m.s], p.total - m.st);
    m.nn = p.T > 0 ? min(m.n, p.T) : m.n;
    m.rank = pos - m.st;
    if (m.rank >= 0 && m.rank < m.n) m.i = i;
    return m;
}

// mean[s, d] over the members, §20.5: the first, then one addition per member in ascending row order, one division
__global__ __launch_bounds__(VX_THREADS) void enc_mean_kernel(const float *__restrict__ points, int C, const int32_t *__restrict__ start,
                                                              const int32_t *__restrict__ cnt, const int32_t *__restrict__ sorted, int T,
                                                              int total, unsigned nvox, float *__restrict__ mean) {
    const unsigned long long e = (unsigned long long)blockIdx.x * VX_THREADS + threadIdx.x;
    if (e >= (unsigned long long)nvox * 3) return;
    const unsigned s = (unsigned)(e / 3);
    const int d = (int)(e - (unsigned long long)s * 3);
    const int st = start[s];
    int n = min(cnt[s], total - st);
    if (T > 0) n = min(n, T);
    if (n <= 0) { mean[e] = 0.0f; return; }
    const int32_t *m = sorted + st;
    float acc = points[(size_t)m[0] * C + d];
    for (int k = 1; k < n; ++k) acc = acc + points[(size_t)m[k] * C + d];
    mean[e] = acc / (float)n;
}

__global__ __launch_bounds__(256) void enc_pack_kernel(const float *__restrict__ W, const float *__restrict__ bias, int Cin, int Cout, int KP,
                                                       int NP, float *__restrict__ dst) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < NP) { dst[t] = t < Cout ? bias[t] : 0.0f; return; }
    const long long q = t - NP;
    if (q >= (long long)NP * KP) return;
    const int e = (int)(q & 3), lane = (int)((q >> 2) & 63);
    const long long blk = q >> 8;                    // tile * KG + k-group
    const int KG = KP >> 3;
    const int g = (int)(blk % KG), tile = (int)(blk / KG);
    const int oc = tile * 32 + (lane & 31), k = 8 * g + 2 * e + (lane >> 5);
    dst[t] = (k < Cin && oc < Cout) ? W[(size_t)oc * Cin + k] : 0.0f;
}

// rows[total, Cin]: thread (x, k) writes column k of the row at list position x, and zeros for row x if it is in no list
__global__ __launch_bounds__(VX_THREADS) void enc_decorate_kernel(const EncP p, float *__restrict__ rows) {
    const unsigned long long e = (unsigned long long)blockIdx.x * VX_THREADS + threadIdx.x;
    if (e >= (unsigned long long)p.total * (unsigned)p.Cin) return;
    const int x = (int)(e / (unsigned)p.Cin), k = (int)(e - (unsigned long long)x * (unsigned)p.Cin);
    const Member m = member_at(p, x, list_end(p));
    if (m.i >= 0) rows[(size_t)m.i * p.Cin + k] = m.rank < m.nn ? row_elem(p, m.i, m.s, k) : 0.0f;
    const int v = p.p2v[x];
    if (v < 0 || v >= p.V) rows[e] = 0.0f;
}

constexpr int ST = 68;            // floats per row of a wave's stage: 64 channels + 4 (16-byte rows, conflict-free columns)

__device__ __forceinline__ void zero_role(const EncP &p) {
    const int C4 = (p.Cout + 3) >> 2;
    unsigned long long q = (unsigned long long)(blockIdx.x - p.tile_blocks) * 256 + threadIdx.x;
    const unsigned long long nz = (unsigned long long)p.nvox * C4;
    if (q < nz) {
        const unsigned s = (unsigned)(q / (unsigned)C4);
        const int c0 = 4 * (int)(q - (unsigned long long)s * (unsigned)C4);
        if (min(p.cnt[s], p.total - p.start[s]) > 0) return;
        const size_t o = (size_t)s * p.Cout + c0;
        if ((p.Cout & 3) == 0 && p.vec_pw) {          // (vec_pw: every output base is 16-byte aligned)
            *reinterpret_cast<float4 *>(p.pooled + o) = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p.arg) *reinterpret_cast<int4 *>(p.arg + o) = make_int4(-1, -1, -1, -1);
        } else {
            for (int u = 0; u < 4 && c0 + u < p.Cout; ++u) {
                p.pooled[o + u] = 0.0f;
                if (p.arg) p.arg[o + u] = -1;
            }
        }
        return;
    }
    q -= nz;
    if (!p.pointwise || q >= (unsigned long long)p.total * C4) return;
    const int i = (int)(q / (unsigned)C4);
    const int c0 = 4 * (int)(q - (unsigned long long)i * (unsigned)C4);
    const int v = p.p2v[i];
    if (v >= 0 && v < p.V) return;                     // (in a list: its owner writes it)
    const size_t o = (size_t)i * p.Cout + c0;
    if ((p.Cout & 3) == 0 && p.vec_pw) *reinterpret_cast<float4 *>(p.pointwise + o) = make_float4(0.f, 0.f, 0.f, 0.f);
    else
        for (int u = 0; u < 4 && c0 + u < p.Cout; ++u) p.pointwise[o + u] = 0.0f;
}

__global__ __launch_bounds__(256) void voxel_encode_kernel(const EncP p) {
    if (blockIdx.x >= p.tile_blocks) { zero_role(p); return; }
    __shared__ __attribute__((aligned(16))) float stage_all[4][32 * ST];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    float *stage = stage_all[wave];
    const int M = list_end(p);
    const long long base_ll = 32LL * ((long long)blockIdx.x * 4 + wave);
    if (base_ll >= M) return;                          // (wave-uniform; no barrier is ever used in this kernel)
    const int base = (int)base_ll;
    const float4 *wfrag = reinterpret_cast<const float4 *>(p.wimg + 32 * p.CT);
    const int npair = (p.CT + 1) >> 1;
#pragma unroll 1
    for (int pr = 0; pr < npair; ++pr) {
        const int c = 64 * pr + lane;                  // the channel this lane walks
        int tl[2];
        tl[0] = 2 * pr;
        tl[1] = 2 * pr + 1 < p.CT ? 2 * pr + 1 : 2 * pr;
        const bool two = 2 * pr + 1 < p.CT;
        float run = 0.0f;
        int runarg = -1;
#pragma unroll 1
        for (int tile = 0;; ++tile) {
            const long long pos_ll = base_ll + 32LL * tile + j;
            const Member m = member_at(p, pos_ll < M ? (int)pos_ll : M, M);
            const bool owned = m.i >= 0 && m.st >= base && m.st - base < 32;
            const bool live = owned && m.rank < m.nn;
            const unsigned lm = (unsigned)__ballot(live);          // (both lane halves hold the same rows)
            if (lm) {
                f32x16 acc[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const float *bias = p.wimg + 32 * tl[t];
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        const float4 bv = *reinterpret_cast<const float4 *>(bias + 8 * a + 4 * h);
                        acc[t][4 * a] = bv.x; acc[t][4 * a + 1] = bv.y; acc[t][4 * a + 2] = bv.z; acc[t][4 * a + 3] = bv.w;
                    }
                }
#pragma unroll 1
                for (int g = 0; g < p.KG; ++g) {
                    float x[4], ops[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int k = 8 * g + 4 * h + e;
                        x[e] = (live && k < p.Cin) ? row_elem(p, m.i, m.s, k) : 0.0f;
                    }
                    to_operands(x[0], x[1], x[2], x[3], ops);
                    acc[0] = mma4(acc[0], wfrag[((size_t)tl[0] * p.KG + g) * 64 + lane], ops);
                    if (two) acc[1] = mma4(acc[1], wfrag[((size_t)tl[1] * p.KG + g) * 64 + lane], ops);
                }
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const f32x16 y = p.relu ? relu16(acc[t]) : acc[t];
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        const float4 yv = make_float4(y[4 * a], y[4 * a + 1], y[4 * a + 2], y[4 * a + 3]);
                        *reinterpret_cast<float4 *>(stage + j * ST + 32 * t + 8 * a + 4 * h) = yv;
                        if (p.pointwise && live && (t == 0 || two)) {
                            const int co = 32 * tl[t] + 8 * a + 4 * h;
                            float *o = p.pointwise + (size_t)m.i * p.Cout + co;
                            if (co + 3 < p.Cout && p.vec_pw && (p.Cout & 3) == 0) *reinterpret_cast<float4 *>(o) = yv;
                            else {
                                if (co < p.Cout) o[0] = yv.x;
                                if (co + 1 < p.Cout) o[1] = yv.y;
                                if (co + 2 < p.Cout) o[2] = yv.z;
                                if (co + 3 < p.Cout) o[3] = yv.w;
                            }
                        }
                    }
                }
            }
            if (p.pointwise && owned && !live && h == 0) {         // list entries past the first T: not members, zeros
                float *o = p.pointwise + (size_t)m.i * p.Cout;
                for (int u = 64 * pr; u < 64 * pr + 64 && u < p.Cout; ++u) o[u] = 0.0f;
            }
            __builtin_amdgcn_wave_barrier();
            if (lm) {
                unsigned rem = lm;
                while (rem) {                                      // wave-uniform: the live rows of the tile in list order
                    const int r = __builtin_ctz(rem);
                    rem &= rem - 1;
                    const unsigned sr = (unsigned)__builtin_amdgcn_readlane((int)m.s, r);
                    const int ir = __builtin_amdgcn_readlane(m.i, r);
                    const int rk = __builtin_amdgcn_readlane(m.rank, r);
                    const int nr = __builtin_amdgcn_readlane(m.nn, r);
                    const float y = stage[r * ST + lane];
                    if (rk == 0 || y > run) { run = y; runarg = ir; }      // strict: a tie stays with the lowest row
                    if (rk == nr - 1 && c < p.Cout) {
                        const size_t o = (size_t)sr * p.Cout + c;
                        p.pooled[o] = run;
                        if (p.arg) p.arg[o] = runarg;
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
            // the voxel of the last position goes on in the next tile: it is this wave's last voxel
            const bool more = owned && m.rank + 1 < (p.pointwise ? m.n : m.nn);
            if (!((__ballot(more) >> 31) & 1ull)) break;
        }
    }
}

using sad::blocks_for;

struct EncWs { size_t lists, mean, wimg, bytes; };

EncWs enc_ws(int total, int B, int V, int Cin, int Cout) {
    EncWs w;
    const size_t NP = ((size_t)Cout + 31) / 32 * 32, KP = ((size_t)Cin + 7) / 8 * 8;
    sad::Carve c;
    w.lists = c.take(sad::voxel_ws_bytes(total, B, V));
    w.mean = c.take((size_t)B * V * 3 * 4);
    w.wimg = c.take(Cout > 0 ? (NP + NP * KP) * 4 : 0);
    w.bytes = c.o + 16;
    return w;
}

// the checks both entry points share, and the fields of EncP that do not depend on the layer
int enc_common(const char *fn, const float *points, const int32_t *p2v, const int32_t *offsets, const int32_t *coors, const float *vox_feat,
               int total, int B, int C, int V, int Cv, const float *voxel_size, const float *point_range, int flags, int max_points,
               const void *workspace, EncP &p) {
    SAD_REQUIRE(offsets && workspace && (total == 0 || (points && p2v)), "%s: NULL pointer", fn);
    SAD_REQUIRE((flags & ~(SAD_VFE_CLUSTER_CENTER | SAD_VFE_VOXEL_CENTER | SAD_VFE_RELU)) == 0, "%s: unknown flag bits in %d", fn, flags);
    const int cc = (flags & SAD_VFE_CLUSTER_CENTER) != 0, vc = (flags & SAD_VFE_VOXEL_CENTER) != 0;
    SAD_REQUIRE(C >= ((cc || vc) ? 3 : 1), "%s: point rows need C >= %d floats (got %d)", fn, (cc || vc) ? 3 : 1, C);
    SAD_REQUIRE(Cv >= 0 && (Cv == 0) == (vox_feat == nullptr), "%s: vox_feat and Cv must be given together (Cv = %d)", fn, Cv);
    SAD_REQUIRE(max_points >= 0, "%s: max_points must be >= 1, or 0 for no cap (got %d)", fn, max_points);
    SAD_REQUIRE(!vc || (coors && voxel_size && point_range), "%s: voxel_center needs coors, voxel_size and point_range", fn);
    if (int rc = sad::voxel_sizes_ok(fn, total, B, V)) return rc;
    SAD_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: workspace must be 16-byte aligned", fn);
    const long long Cin = (long long)C + 3 * cc + 3 * vc + Cv;
    if (Cin < 1 || Cin > 256) return sad::fail(SAD_EUNSUPPORTED, "%s: Cin = %lld rows (1 .. 256 supported)", fn, Cin);
    p.points = points; p.p2v = p2v; p.offsets = offsets; p.coors = coors; p.vox_feat = vox_feat;
    p.total = total; p.B = B; p.C = C; p.V = V; p.Cv = Cv; p.Cin = (int)Cin; p.T = max_points; p.cc = cc; p.vc = vc;
    p.relu = (flags & SAD_VFE_RELU) != 0;
    p.nvox = (unsigned)B * (unsigned)V;
    for (int d = 0; d < 3; ++d) {
        p.vs[d] = vc ? voxel_size[d] : 0.0f;
        p.lo[d] = vc ? point_range[d] : 0.0f;
        SAD_REQUIRE(isfinite(p.vs[d]) && isfinite(p.lo[d]), "%s: voxel_size and point_range must be finite (axis %d)", fn, d);
    }
    return SAD_OK;
}

// lists + mean (if the cluster centre is asked for)
void enc_lists(EncP &p, char *ws, const EncWs &w, hipStream_t st) {
    sad::VoxLists ml;
    sad::voxel_member_lists(p.p2v, p.offsets, p.total, p.B, p.V, ws + w.lists, st, ml);
    p.start = ml.start; p.cnt = ml.cnt; p.sorted = ml.sorted;
    float *mean = (float *)(ws + w.mean);
    p.mean = mean;
    if (p.cc && p.total > 0)
        hipLaunchKernelGGL(enc_mean_kernel, dim3(blocks_for((unsigned long long)p.nvox * 3, VX_THREADS)), dim3(VX_THREADS), 0, st, p.points,
                           p.C, p.start, p.cnt, p.sorted, p.T, p.total, p.nvox, mean);
}

}  // namespace

SAD_API int sad_voxel_encode_workspace_bytes(int total_points, int B, int max_voxels, int Cin, int Cout, size_t *out) {
    SAD_REQUIRE(out, "sad_voxel_encode_workspace_bytes: NULL out");
    *out = 0;
    if (int rc = sad::voxel_sizes_ok("sad_voxel_encode_workspace_bytes", total_points, B, max_voxels)) return rc;
    if (Cin < 1 || Cin > 256 || Cout < 0 || Cout > 256)
        return sad::fail(SAD_EUNSUPPORTED, "sad_voxel_encode_workspace_bytes: Cin = %d, Cout = %d (1 .. 256 supported)", Cin, Cout);
    *out = enc_ws(total_points, B, max_voxels, Cin, Cout).bytes;
    return SAD_OK;
}

SAD_API int sad_voxel_decorate_f32(const float *points, const int32_t *point2voxel, const int32_t *offsets, const int32_t *coors,
                                   const float *vox_feat, int total_points, int B, int C, int max_voxels, int Cv, const float *voxel_size,
                                   const float *point_range, int flags, int max_points, float *rows, void *workspace, sad_stream_t stream) {
    EncP p = {};
    if (int rc = enc_common("sad_voxel_decorate_f32", points, point2voxel, offsets, coors, vox_feat, total_points, B, C, max_voxels, Cv, voxel_size,
                            point_range, flags, max_points, workspace, p))
        return rc;
    SAD_REQUIRE(total_points == 0 || rows, "sad_voxel_decorate_f32: NULL rows");
    if (total_points == 0) return SAD_OK;
    const hipStream_t st = (hipStream_t)stream;
    enc_lists(p, (char *)workspace, enc_ws(total_points, B, max_voxels, p.Cin, 0), st);
    hipLaunchKernelGGL(enc_decorate_kernel, dim3(blocks_for((unsigned long long)total_points * p.Cin, VX_THREADS)), dim3(VX_THREADS), 0, st,
                       p, rows);
    return sad::check_launch("sad_voxel_decorate_f32");
}

SAD_API int sad_voxel_encode_f32(const float *points, const int32_t *point2voxel, const int32_t *offsets, const int32_t *coors,
                                 const float *vox_feat, int total_points, int B, int C, int max_voxels, int Cv, const float *voxel_size,
                                 const float *point_range, const float *weight, const float *bias, int Cout, int flags, int max_points,
                                 float *pooled, int32_t *arg, float *pointwise, void *workspace, sad_stream_t stream) {
    EncP p = {};
    if (int rc = enc_common("sad_voxel_encode_f32", points, point2voxel, offsets, coors, vox_feat, total_points, B, C, max_voxels, Cv, voxel_size,
                            point_range, flags, max_points, workspace, p))
        return rc;
    SAD_REQUIRE(weight && bias && pooled, "sad_voxel_encode_f32: NULL weight / bias / pooled");
    if (Cout < 1 || Cout > 256) return sad::fail(SAD_EUNSUPPORTED, "sad_voxel_encode_f32: Cout = %d (1 .. 256 supported)", Cout);
    const unsigned long long nout = (unsigned long long)p.nvox * Cout;
    if (nout >= (1ull << 40)) return sad::fail(SAD_EUNSUPPORTED, "sad_voxel_encode_f32: pooled[B,V,Cout] of %llu floats is too large", nout);
    p.Cout = Cout;
    p.KG = (p.Cin + 7) / 8;
    p.CT = (Cout + 31) / 32;
    p.pooled = pooled; p.arg = arg; p.pointwise = pointwise;
    p.vec_pw = (((uintptr_t)pooled | (uintptr_t)arg | (uintptr_t)pointwise) & 15) == 0;
    const unsigned long long C4 = ((unsigned long long)Cout + 3) / 4;
    // (each count fits blocks_for's unsigned: nvox < 2^31, total <= 2^30, C4 <= 64; their sum is checked in 64 bits)
    const unsigned long long tile_blocks = blocks_for(blocks_for((unsigned long long)total_points, 32), 4);
    const unsigned long long zero_blocks = blocks_for((unsigned long long)p.nvox * C4 + (pointwise ? (unsigned long long)total_points * C4 : 0ull), 256);
    if (tile_blocks + zero_blocks >= (1ull << 31)) return sad::fail(SAD_EUNSUPPORTED, "sad_voxel_encode_f32: too many workgroups");
    p.tile_blocks = (unsigned)tile_blocks;
    const hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    const EncWs w = enc_ws(total_points, B, max_voxels, p.Cin, Cout);
    enc_lists(p, ws, w, st);
    float *wimg = (float *)(ws + w.wimg);
    p.wimg = wimg;
    const int NP = 32 * p.CT, KP = 8 * p.KG;
    hipLaunchKernelGGL(enc_pack_kernel, dim3(blocks_for((unsigned long long)NP + (unsigned long long)NP * KP, 256)), dim3(256), 0, st, weight,
                       bias, p.Cin, Cout, KP, NP, wimg);
    hipLaunchKernelGGL(voxel_encode_kernel, dim3((unsigned)(tile_blocks + zero_blocks)), dim3(256), 0, st, p);
    return sad::check_launch("sad_voxel_encode_f32");
}
