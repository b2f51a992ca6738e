// Sparse 3-D convolution (SPEC.md §21): the rulebook (which input row every kernel offset of every output row reads), the
// convolution itself and the scatter to a dense tensor.  The upstream reference has no such operator; the semantics are SPEC.md's own.
//
// rulebook   the input rows go into a coordinate table of vox_hash.h under (scene << 32 | (z*Gy + y)*Gx + x) with their row;
//            nbr[o, kk] is then one lookup per (output row, kernel offset).  The strided form finds its output sites with a SECOND
//            table keyed by output site that takes the candidate numbers i*Kvol + kk, and the first-appearance numbering of
//            vox_hash.h over the candidates numbers the sites.  Nothing read back depends on the order of an atomic.  `count`
//            ends with out_offsets[B+1] on the device, `fill` numbers the openers and does the lookups.
// conv       output-stationary implicit GEMM on v_mfma_f32_32x32x2_f32.  A workgroup (4 waves) owns TR = 64 or 128 output rows and
//            ALL output channels; every output element lives in one accumulator from the bias to the store, kk ascending and ci
//            ascending inside, which is SPEC §21.2's fmaf chain bit for bit (no split K, no atomics).  Per kk: the tile's neighbour
//            rows are gathered into LDS (zero rows for -1, Cin padded with zeros to a multiple of 8), the weights come fragment-
//            shaped from the packed image (coalesced 1-KB loads, L2-resident) and lane (j, h) reads c0..c3 / c4..c7 of its row per
//            k-group, two v_permlane32_swap making the four B operands (reg_common.h, as in mlp_rows.hip).  A kk no row of the
//            workgroup's tile needs is skipped with its gather and barriers; a kk none of a wave's 32 rows needs is skipped by that
//            wave.  Both are exact: the skipped steps would add fmaf(w, 0, acc).
// dense      lowest row of every cell by atomicMin into an int grid (the workspace), then ONE pass that writes every element of
//            dense[B,C,Oz,Oy,Ox] once: the row's value or zero.
#include "common.h"
#include <algorithm>
#include <limits.h>

namespace {

#include "vox_hash.h"
#include "reg_common.h"

// (z, y, x) order throughout
struct SpGeo {
    int G[3], O[3], K[3], s[3], p[3];
    int Kvol;
};

__device__ __forceinline__ void kk_split(int kk, const SpGeo &g, int *k) {
    const int kyx = g.K[1] * g.K[2];
    k[0] = kk / kyx;
    const int r = kk - k[0] * kyx;
    k[1] = r / g.K[2];
    k[2] = r - k[1] * g.K[2];
}

// ---- rulebook ---------------------------------------------------------------------------------------------------
// (the input table, the rows under (scene << 32 | cell): launch_coord_rows of vox_hash.h)

// nbr[o, kk] = lowest input row of o's scene at out_coors[o] * s - p + k, or -1.  Rows at and above the true total
// (out_offsets[B]; a fill with spare capacity) get nbr -1 and coordinates -1.
__global__ __launch_bounds__(VX_THREADS) void sp_nbr_kernel(int32_t *out_coors, const int32_t *__restrict__ out_offsets, int rows, int B, SpGeo g,
                                                            CoordTable t, int pad_coors, int32_t *__restrict__ nbr) {
    const long long e = (long long)blockIdx.x * VX_THREADS + threadIdx.x;
    if (e >= (long long)rows * g.Kvol) return;
    const int o = (int)(e / g.Kvol), kk = (int)(e - (long long)o * g.Kvol);
    if (o >= out_offsets[B]) {
        nbr[e] = -1;
        if (pad_coors && kk == 0) { out_coors[(size_t)o * 3] = -1; out_coors[(size_t)o * 3 + 1] = -1; out_coors[(size_t)o * 3 + 2] = -1; }
        return;
    }
    int k[3];
    kk_split(kk, g, k);
    const int32_t *c = out_coors + (size_t)o * 3;
    // 64-bit: o * s reaches G + 2 p - K, which passes 2^31 - 1 on a grid near the cell limit
    const long long z = (long long)c[0] * g.s[0] - g.p[0] + k[0], y = (long long)c[1] * g.s[1] - g.p[1] + k[1],
                    x = (long long)c[2] * g.s[2] - g.p[2] + k[2];
    int r = -1;
    if (z >= 0 && z < g.G[0] && y >= 0 && y < g.G[1] && x >= 0 && x < g.G[2]) {
        const u64 k64 = ((u64)(unsigned)scene_of(out_offsets, B, o) << 32) | (unsigned)(((int)z * g.G[1] + (int)y) * g.G[2] + (int)x);
        const int slot = t.find(k64);
        if (slot >= 0) r = t.lowest(slot);
    }
    nbr[e] = r;
}

// candidate c = i * Kvol + kk names the output site o with o * s = coors[i] + p - k, if the division is exact and o in range
__device__ __forceinline__ bool cand_site(const int32_t *__restrict__ coors, int c, const SpGeo &g, int &i, int *o) {
    i = c / g.Kvol;
    int k[3];
    kk_split(c - i * g.Kvol, g, k);
    bool ok = true;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        // unsigned: coors + p passes 2^31 - 1 on a grid near the cell limit (it stays below 2^32: p <= 65535)
        const int x = coors[(size_t)i * 3 + d];
        const unsigned xp = (unsigned)x + (unsigned)g.p[d];
        const unsigned t = xp - (unsigned)k[d];
        const unsigned q = t / (unsigned)g.s[d];
        ok = ok && x >= 0 && xp >= (unsigned)k[d] && q * (unsigned)g.s[d] == t && q < (unsigned)g.O[d];
        o[d] = (int)q;
    }
    return ok;
}

__device__ __forceinline__ u64 site_key(const int32_t *__restrict__ offsets, int B, int i, const int *o, const SpGeo &g) {
    return ((u64)(unsigned)scene_of(offsets, B, i) << 32) | (unsigned)((o[0] * g.O[1] + o[1]) * g.O[2] + o[2]);
}

// the candidates of the strided form and the opener of vox_hash.h's numbering over them: a candidate is an opener iff it is
// the lowest candidate of its output site
struct CandOpener {
    using index = long long;
    const int32_t *coors, *offsets;
    int n, B;                 // n = NC = Nv * Kvol candidates
    SpGeo g;
    CoordTable t;             // keyed by output site
    // o[3] = the site of c (whenever c names one)
    __device__ __forceinline__ bool operator()(long long c, int *o) const {
        if (c >= n) return false;
        int i;
        if (!cand_site(coors, (int)c, g, i, o)) return false;
        const int slot = t.find(site_key(offsets, B, i, o, g));
        return slot >= 0 && t.lowest(slot) == (int)c;
    }
    __device__ __forceinline__ bool operator()(long long c) const { int o[3]; return (*this)(c, o); }
    __device__ __forceinline__ long long first_of(int row) const { return min((long long)max(row, 0) * g.Kvol, (long long)n); }
};

__global__ __launch_bounds__(VX_THREADS) void sp_cand_insert_kernel(const CandOpener op) {
    const long long c = (long long)blockIdx.x * VX_THREADS + threadIdx.x;
    if (c >= op.n) return;
    int i, o[3];
    if (!cand_site(op.coors, (int)c, op.g, i, o)) return;
    op.t.insert_min(site_key(op.offsets, op.B, i, o, op.g), (int)c);
}

// out_offsets[b] = openers among the candidates of the rows below offsets[b]
__global__ __launch_bounds__(VX_SCAN_THREADS) void sp_scan_kernel(const CandOpener op, int32_t *wavecnt, int nw, int32_t *__restrict__ out_offsets) {
    __shared__ int s_w[VX_SCAN_THREADS / 64 + 1];
    opener_scan(op, op.offsets, op.B, wavecnt, nw, out_offsets, s_w);
}

// openers write their site at their number (global output row = openers before it), below the capacity
__global__ __launch_bounds__(VX_THREADS) void sp_number_kernel(const CandOpener op, const int32_t *__restrict__ wavepre, int capacity,
                                                               int32_t *__restrict__ out_coors) {
    const long long c = (long long)blockIdx.x * VX_THREADS + threadIdx.x;
    int o[3];
    const bool open = op(c, o);
    const int below = openers_below(open);
    if (!open) return;
    const int n = wavepre[c >> 6] + below;
    if (n < 0 || n >= capacity) return;
    out_coors[(size_t)n * 3 + 0] = o[0];
    out_coors[(size_t)n * 3 + 1] = o[1];
    out_coors[(size_t)n * 3 + 2] = o[2];
}

// ---- weights ------------------------------------------------------------------------------------------------------
// packed image: NP = 32 * nct biases (zero beyond Cout / without a bias), then [kk][channel tile][k-group][lane] x float4:
// component e of lane (i, h) = W[kk][32 tile + i][8 g + 2 e + h], zero outside Cout x Cin
__global__ __launch_bounds__(VX_THREADS) void spconv_pack_kernel(const float *__restrict__ W, const float *__restrict__ bias, int Kvol, int Cin, int Cout,
                                                                 int KG, int nct, float *__restrict__ packed) {
    const long long e = (long long)blockIdx.x * VX_THREADS + threadIdx.x;
    const int NP = 32 * nct;
    if (e < NP) packed[e] = (bias && e < Cout) ? bias[e] : 0.0f;
    const long long nf4 = (long long)Kvol * nct * KG * 64;
    if (e >= nf4) return;
    const int lane = (int)(e & 63);
    long long r = e >> 6;
    const int gq = (int)(r % KG);
    r /= KG;
    const int tile = (int)(r % nct), kk = (int)(r / nct);
    const int co = 32 * tile + (lane & 31), hh = lane >> 5;
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int ci = 8 * gq + 2 * q + hh;
        v[q] = (co < Cout && ci < Cin) ? W[((size_t)kk * Cout + co) * Cin + ci] : 0.0f;
    }
    reinterpret_cast<float4 *>(packed + NP)[e] = make_float4(v[0], v[1], v[2], v[3]);
}

// ---- convolution ----------------------------------------------------------------------------------------------------
struct ConvJob {
    const float *feat;
    const int32_t *nbr;
    const float *packed;
    const float *residual;
    float *out;
    int Nv, No, Kvol, Cin, Cout;
    int KG, nct, LDX;             // k-groups of 8, channel tiles of 32, floats between rows of the LDS image
    int relu, vec_in, vec_out;
};

// WR waves along the rows x 4 / WR along the channels; a wave owns RS 32-row subtiles x NT 32-channel tiles
template <int WR, int RS, int NT>
__global__ __launch_bounds__(256) void spconv_kernel(const ConvJob jb) {
    constexpr int TR = 32 * WR * RS;
    extern __shared__ __attribute__((aligned(16))) float sp_smem[];
    float *s_x = sp_smem;                                        // [TR][LDX]
    int *s_nbr = reinterpret_cast<int *>(sp_smem + TR * jb.LDX);  // [TR][Kvol]
    unsigned *s_mask = reinterpret_cast<unsigned *>(s_nbr + TR * jb.Kvol);   // [TR / 32]: bit kk = some row of the subtile has a neighbour at kk
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int wr = wave % WR, wc = wave / WR;
    const int Kvol = jb.Kvol, KG = jb.KG, LDX = jb.LDX, nct = jb.nct;
    const long long row0 = (long long)blockIdx.x * TR;

    if (tid < TR / 32) s_mask[tid] = 0u;
    __syncthreads();
    for (int idx = tid; idx < TR * Kvol; idx += 256) {
        const int r = idx / Kvol, kk = idx - r * Kvol;
        const long long row = row0 + r;
        int n = row < jb.No ? jb.nbr[row * Kvol + kk] : -1;
        if (n >= jb.Nv) n = -1;                                  // (never read outside feat, whatever the caller passed)
        s_nbr[idx] = n;
        if (n >= 0) atomicOr(&s_mask[r >> 5], 1u << kk);
    }
    __syncthreads();
    unsigned all = 0u, sub[RS];
#pragma unroll
    for (int q = 0; q < TR / 32; ++q) all |= s_mask[q];
    all = __builtin_amdgcn_readfirstlane(all);
#pragma unroll
    for (int rs = 0; rs < RS; ++rs) sub[rs] = __builtin_amdgcn_readfirstlane(s_mask[wr * RS + rs]);

    int tile[NT];
    f32x16 acc[RS][NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        tile[t] = wc * NT + t < nct ? wc * NT + t : nct - 1;     // (a surplus tile repeats the last one and stores nothing)
        const float *bias = jb.packed + tile[t] * 32;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const float4 bv = *reinterpret_cast<const float4 *>(bias + 8 * a + 4 * h);
#pragma unroll
            for (int rs = 0; rs < RS; ++rs) {
                acc[rs][t][4 * a] = bv.x; acc[rs][t][4 * a + 1] = bv.y; acc[rs][t][4 * a + 2] = bv.z; acc[rs][t][4 * a + 3] = bv.w;
            }
        }
    }
    const float4 *wimg = reinterpret_cast<const float4 *>(jb.packed + 32 * nct);
    const int CQ = 2 * KG;                                       // float4 per row of the LDS image

#pragma unroll 1
    for (int kk = 0; kk < Kvol; ++kk) {
        if (!((all >> kk) & 1u)) continue;                       // (workgroup-uniform: no row of the tile reads this offset)
        __syncthreads();                                         // the previous offset's rows are no longer read
        for (int idx = tid; idx < TR * CQ; idx += 256) {
            const int r = idx / CQ, q = idx - r * CQ;
            const int n = s_nbr[r * Kvol + kk];
            const int c0 = 4 * q;
            *reinterpret_cast<float4 *>(s_x + r * LDX + c0) = row_quad(jb.feat, n, jb.Cin, c0, jb.Cin, jb.vec_in);
        }
        __syncthreads();
        bool any = false;
#pragma unroll
        for (int rs = 0; rs < RS; ++rs) any = any || ((sub[rs] >> kk) & 1u);
        if (!any) continue;                                      // (wave-uniform: none of this wave's rows reads this offset)
        const float4 *wk[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) wk[t] = wimg + ((size_t)kk * nct + tile[t]) * KG * 64 + lane;
        float4 an[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) an[t] = wk[t][0];
#pragma unroll 1
        for (int g = 0; g < KG; ++g) {
            float4 a[NT];
            const int gn = g + 1 < KG ? g + 1 : g;
#pragma unroll
            for (int t = 0; t < NT; ++t) { a[t] = an[t]; an[t] = wk[t][(size_t)gn * 64]; }     // the next k-group's weights are in flight during the MFMAs
#pragma unroll
            for (int rs = 0; rs < RS; ++rs) {
                if ((sub[rs] >> kk) & 1u) {
                    const float4 xv = *reinterpret_cast<const float4 *>(s_x + ((wr * RS + rs) * 32 + j) * LDX + 8 * g + 4 * h);
                    float ops[4];
                    to_operands(xv.x, xv.y, xv.z, xv.w, ops);
#pragma unroll
                    for (int t = 0; t < NT; ++t) acc[rs][t] = mma4(acc[rs][t], a[t], ops);
                }
            }
        }
    }

    // ---- epilogue: lane = row, registers 4a .. 4a+3 = channels 32 tile + 8 a + 4 h .. + 3 ----
#pragma unroll
    for (int rs = 0; rs < RS; ++rs) {
        const long long row = row0 + (wr * RS + rs) * 32 + j;
        if (row >= jb.No) continue;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (wc * NT + t >= nct) continue;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const int co = tile[t] * 32 + 8 * a + 4 * h;
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc[rs][t][4 * a + e];
                const size_t at = (size_t)row * jb.Cout + co;
                if (jb.residual) {
                    if (co + 3 < jb.Cout && jb.vec_out) {
                        const float4 rv = *reinterpret_cast<const float4 *>(jb.residual + at);
                        v[0] = v[0] + rv.x; v[1] = v[1] + rv.y; v[2] = v[2] + rv.z; v[3] = v[3] + rv.w;
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (co + e < jb.Cout) v[e] = v[e] + jb.residual[at + e];
                    }
                }
                if (jb.relu) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.0f ? v[e] : 0.0f;
                }
                if (co + 3 < jb.Cout && jb.vec_out) {
                    *reinterpret_cast<float4 *>(jb.out + at) = make_float4(v[0], v[1], v[2], v[3]);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (co + e < jb.Cout) jb.out[at + e] = v[e];
                }
            }
        }
    }
}

// ---- dense ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VX_THREADS) void dense_init_kernel(int32_t *__restrict__ cell, unsigned n) { grid_fill(cell, n, INT_MAX); }

__global__ __launch_bounds__(VX_THREADS) void dense_owner_kernel(const int32_t *__restrict__ coors, const int32_t *__restrict__ offsets, int No, int B, int Oz,
                                                                 int Oy, int Ox, int32_t *cell) {
    const int r = blockIdx.x * VX_THREADS + threadIdx.x;
    if (r >= No) return;
    const int z = coors[(size_t)r * 3], y = coors[(size_t)r * 3 + 1], x = coors[(size_t)r * 3 + 2];
    if (z < 0 || z >= Oz || y < 0 || y >= Oy || x < 0 || x >= Ox) return;
    const size_t at = (((size_t)scene_of(offsets, B, r) * Oz + z) * Oy + y) * Ox + x;
    keep_min(&cell[at], r);
}

__global__ __launch_bounds__(VX_THREADS) void dense_write_kernel(const float *__restrict__ feat, const int32_t *__restrict__ cell, int C, unsigned cells,
                                                                 unsigned long long n, float *__restrict__ dense) {
    const unsigned long long e = (unsigned long long)blockIdx.x * VX_THREADS + threadIdx.x;
    if (e >= n) return;
    const unsigned long long bc = e / cells;
    const unsigned at = (unsigned)(e - bc * cells);
    const unsigned b = (unsigned)(bc / (unsigned)C), c = (unsigned)(bc - (unsigned long long)b * (unsigned)C);
    const int r = cell[(size_t)b * cells + at];
    dense[e] = r != INT_MAX ? feat[(size_t)r * C + c] : 0.0f;
}

// ---- host side ----------------------------------------------------------------------------------------------------------
using sad::al16;
using sad::blocks_for;
#include "spconv_limits.h"

// kernel / stride / padding / shapes of §21: subm ignores stride and padding (1 and K / 2)
int sp_geo(const char *fn, const int *shape, const int *kernel, const int *stride, const int *padding, int subm, SpGeo &g) {
    SAD_REQUIRE(kernel && (subm || (stride && padding)), "%s: NULL kernel / stride / padding", fn);
    long long cells = 1, ocells = 1;
    g.Kvol = 1;
    for (int d = 0; d < 3; ++d) {
        const int K = kernel[d];
        SAD_REQUIRE(K >= 1, "%s: kernel size %d on axis %d must be >= 1", fn, K, d);
        if (K > 3) return sad::fail(SAD_EUNSUPPORTED, "%s: kernel size %d on axis %d (1 .. 3 are implemented)", fn, K, d);
        g.K[d] = K;
        g.Kvol *= K;
        if (subm) {
            SAD_REQUIRE(K % 2 == 1, "%s: a submanifold convolution needs odd kernel sizes (axis %d: %d)", fn, d, K);
            SAD_REQUIRE(!stride || stride[d] == 1, "%s: a submanifold convolution has stride 1 (axis %d: %d)", fn, d, stride[d]);
            SAD_REQUIRE(!padding || padding[d] == K / 2, "%s: a submanifold convolution has padding K / 2 (axis %d: %d)", fn, d, padding[d]);
            g.s[d] = 1;
            g.p[d] = K / 2;
        } else {
            SAD_REQUIRE(stride[d] >= 1 && padding[d] >= 0, "%s: stride must be >= 1 and padding >= 0 (axis %d: %d, %d)", fn, d, stride[d], padding[d]);
            if (stride[d] > 65535 || padding[d] > 65535) return sad::fail(SAD_EUNSUPPORTED, "%s: stride / padding above 65535 (axis %d)", fn, d);
            g.s[d] = stride[d];
            g.p[d] = padding[d];
        }
        if (shape) {
            SAD_REQUIRE(shape[d] >= 1, "%s: spatial_shape[%d] = %d must be >= 1", fn, d, shape[d]);
            g.G[d] = shape[d];
            cells *= shape[d];
            if (cells > 2147483647LL) return sad::fail(SAD_EUNSUPPORTED, "%s: spatial_shape exceeds 2^31 - 1 cells", fn);
            const long long span = (long long)shape[d] + 2LL * g.p[d] - K;
            SAD_REQUIRE(span >= 0, "%s: axis %d: the kernel (%d) does not fit the padded grid (%d + 2 * %d)", fn, d, K, shape[d], g.p[d]);
            g.O[d] = (int)(span / g.s[d]) + 1;
            ocells *= g.O[d];
            if (ocells > 2147483647LL) return sad::fail(SAD_EUNSUPPORTED, "%s: the output shape exceeds 2^31 - 1 cells", fn);
        } else {
            g.G[d] = g.O[d] = 1;
        }
    }
    return SAD_OK;
}

// the workspace (NULL: a size query): the input rows by cell; (strided form) the candidates by output site and their per-64 opener counts
struct SpWs {
    CoordTable in, sites;
    int32_t *wavecnt;
    size_t bytes;
};

// the distinct output sites of the strided form: at most prod ceil(K_d / s_d) per input row
inline long long sp_max_sites(int Nv, const SpGeo &g) {
    long long per = 1;
    for (int d = 0; d < 3; ++d) per *= (g.K[d] + g.s[d] - 1) / g.s[d];
    return per * Nv;
}

int sp_sizes_ok(const char *fn, long long Nv, int B, const SpGeo &g, int subm) {
    SAD_REQUIRE(B >= 1 && B <= 65535, "%s: B must be in 1 .. 65535 (got %d)", fn, B);
    SAD_REQUIRE(Nv >= 0 && Nv <= (1 << 30), "%s: Nv must be in 0 .. 2^30 (got %lld)", fn, Nv);
    if (int rc = sp_rows_ok(fn, "Nv", Nv, g.Kvol)) return rc;
    if (!subm && sp_max_sites((int)Nv, g) > (1LL << 30)) return sad::fail(SAD_EUNSUPPORTED, "%s: more than 2^30 possible output sites", fn);
    return SAD_OK;
}

SpWs sp_ws(void *ws, int Nv, const SpGeo &g, int subm) {
    SpWs w = {};
    sad::Carve c;
    w.in = CoordTable(ws, c, (unsigned long long)Nv);
    if (!subm) {
        w.sites = CoordTable(ws, c, (unsigned long long)sp_max_sites(Nv, g));
        w.wavecnt = (int32_t *)((uintptr_t)ws + c.take((((size_t)Nv * g.Kvol + 63) / 64 + 2) * 4));
    }
    w.bytes = c.o + 16;
    return w;
}

template <int WR, int RS, int NT>
int launch_conv(const ConvJob &jb, hipStream_t st) {
    constexpr int TR = 32 * WR * RS;
    const size_t lds = ((size_t)TR * jb.LDX + (size_t)TR * jb.Kvol + TR / 32 + 4) * 4;
    if (lds > 160 * 1024) return sad::fail(SAD_EUNSUPPORTED, "sad_spconv_f32: %zu bytes of LDS needed", lds);
    static std::atomic<uint64_t> done{0};
    sad::lds_attr_once(done, reinterpret_cast<const void *>(&spconv_kernel<WR, RS, NT>), 160 * 1024);
    const long long grid = ((long long)jb.No + TR - 1) / TR;
    hipLaunchKernelGGL((spconv_kernel<WR, RS, NT>), dim3((unsigned)grid), dim3(256), lds, st, jb);
    return sad::check_launch("sad_spconv_f32");
}

}  // namespace

SAD_API int sad_spconv_workspace_bytes(int Nv, int B, const int *kernel, const int *stride, int subm, size_t *out) {
    SAD_REQUIRE(out, "sad_spconv_workspace_bytes: NULL out");
    *out = 0;
    SpGeo g;
    const int zero[3] = {0, 0, 0};
    if (int rc = sp_geo("sad_spconv_workspace_bytes", nullptr, kernel, subm ? nullptr : stride, subm ? nullptr : zero, subm, g)) return rc;
    if (int rc = sp_sizes_ok("sad_spconv_workspace_bytes", Nv, B, g, subm)) return rc;
    *out = sp_ws(nullptr, Nv, g, subm).bytes;
    return SAD_OK;
}

SAD_API int sad_spconv_index_subm(const int32_t *coors, const int32_t *offsets, int Nv, int B, const int *spatial_shape, const int *kernel,
                                  int32_t *nbr, void *workspace, sad_stream_t stream) {
    SAD_REQUIRE(offsets && workspace && spatial_shape && (Nv == 0 || (coors && nbr)), "sad_spconv_index_subm: NULL pointer");
    SAD_REQUIRE(aligned16(workspace), "sad_spconv_index_subm: workspace must be 16-byte aligned");
    SpGeo g;
    if (int rc = sp_geo("sad_spconv_index_subm", spatial_shape, kernel, nullptr, nullptr, 1, g)) return rc;
    if (int rc = sp_sizes_ok("sad_spconv_index_subm", Nv, B, g, 1)) return rc;
    if (Nv == 0) return SAD_OK;
    const SpWs w = sp_ws(workspace, Nv, g, 1);
    const hipStream_t st = (hipStream_t)stream;
    launch_coord_rows(coors, offsets, Nv, B, g.G[1], g.G[2], w.in, st);
    hipLaunchKernelGGL(sp_nbr_kernel, dim3(blocks_for((unsigned long long)Nv * g.Kvol, VX_THREADS)), dim3(VX_THREADS), 0, st, (int32_t *)coors, offsets, Nv,
                       B, g, w.in, 0, nbr);
    return sad::check_launch("sad_spconv_index_subm");
}

SAD_API int sad_spconv_index_count(const int32_t *coors, const int32_t *offsets, int Nv, int B, const int *spatial_shape, const int *kernel,
                                   const int *stride, const int *padding, int32_t *out_offsets, void *workspace, sad_stream_t stream) {
    SAD_REQUIRE(offsets && out_offsets && workspace && spatial_shape && (Nv == 0 || coors), "sad_spconv_index_count: NULL pointer");
    SAD_REQUIRE(aligned16(workspace), "sad_spconv_index_count: workspace must be 16-byte aligned");
    SpGeo g;
    if (int rc = sp_geo("sad_spconv_index_count", spatial_shape, kernel, stride, padding, 0, g)) return rc;
    if (int rc = sp_sizes_ok("sad_spconv_index_count", Nv, B, g, 0)) return rc;
    const SpWs w = sp_ws(workspace, Nv, g, 0);
    const hipStream_t st = (hipStream_t)stream;
    const int NC = Nv * g.Kvol, nw = (NC + 63) / 64;
    const CandOpener op = {coors, offsets, NC, B, g, w.sites};
    const dim3 gc(blocks_for((unsigned long long)NC, VX_THREADS)), tb(VX_THREADS);
    launch_coord_rows(coors, offsets, Nv, B, g.G[1], g.G[2], w.in, st);
    launch_coord_clear(w.sites, st);
    if (NC > 0) {
        hipLaunchKernelGGL(sp_cand_insert_kernel, gc, tb, 0, st, op);
        hipLaunchKernelGGL(opener_flags_kernel<CandOpener>, gc, tb, 0, st, op, w.wavecnt);
    }
    hipLaunchKernelGGL(sp_scan_kernel, dim3(1), dim3(VX_SCAN_THREADS), 0, st, op, w.wavecnt, nw, out_offsets);
    return sad::check_launch("sad_spconv_index_count");
}

SAD_API int sad_spconv_index_fill(const int32_t *coors, const int32_t *offsets, int Nv, int B, const int *spatial_shape, const int *kernel,
                                  const int *stride, const int *padding, const int32_t *out_offsets, int capacity, int32_t *out_coors, int32_t *nbr,
                                  void *workspace, sad_stream_t stream) {
    SAD_REQUIRE(offsets && out_offsets && workspace && spatial_shape && (Nv == 0 || coors) && (capacity == 0 || (out_coors && nbr)),
                "sad_spconv_index_fill: NULL pointer");
    SAD_REQUIRE(capacity >= 0, "sad_spconv_index_fill: capacity must be >= 0 (got %d)", capacity);
    SAD_REQUIRE(aligned16(workspace), "sad_spconv_index_fill: workspace must be 16-byte aligned");
    SpGeo g;
    if (int rc = sp_geo("sad_spconv_index_fill", spatial_shape, kernel, stride, padding, 0, g)) return rc;
    if (int rc = sp_sizes_ok("sad_spconv_index_fill", Nv, B, g, 0)) return rc;
    if (int rc = sp_rows_ok("sad_spconv_index_fill", "capacity", capacity, g.Kvol)) return rc;
    if (capacity == 0) return SAD_OK;
    const SpWs w = sp_ws(workspace, Nv, g, 0);
    const hipStream_t st = (hipStream_t)stream;
    const int NC = Nv * g.Kvol;
    if (NC > 0) {
        const CandOpener op = {coors, offsets, NC, B, g, w.sites};
        hipLaunchKernelGGL(sp_number_kernel, dim3(blocks_for((unsigned long long)NC, VX_THREADS)), dim3(VX_THREADS), 0, st, op,
                           (const int32_t *)w.wavecnt, capacity, out_coors);
    }
    hipLaunchKernelGGL(sp_nbr_kernel, dim3(blocks_for((unsigned long long)capacity * g.Kvol, VX_THREADS)), dim3(VX_THREADS), 0, st, out_coors, out_offsets,
                       capacity, B, g, w.in, 1, nbr);
    return sad::check_launch("sad_spconv_index_fill");
}

SAD_API size_t sad_spconv_packed_floats(int Kvol, int Cin, int Cout) {
    if (Kvol < 1 || Kvol > SP_MAX_KVOL || Cin < 1 || Cout < 1 || Cin > SP_MAX_C || Cout > SP_MAX_C) return 0;
    const size_t nct = ((size_t)Cout + 31) / 32, KG = ((size_t)Cin + 7) / 8;
    return 32 * nct + (size_t)Kvol * nct * KG * 256;
}

SAD_API int sad_spconv_pack_f32(const float *W, const float *bias, int Kvol, int Cin, int Cout, float *packed, sad_stream_t stream) {
    SAD_REQUIRE(W && packed, "sad_spconv_pack_f32: NULL pointer");
    if (int rc = sp_channels_ok("sad_spconv_pack_f32", Kvol, Cin, Cout)) return rc;
    SAD_REQUIRE(aligned16(packed), "sad_spconv_pack_f32: packed must be 16-byte aligned");
    const int nct = (Cout + 31) / 32, KG = (Cin + 7) / 8;
    const unsigned long long n = std::max<unsigned long long>((unsigned long long)Kvol * nct * KG * 64, 32ull * nct);
    hipLaunchKernelGGL(spconv_pack_kernel, dim3(blocks_for(n, VX_THREADS)), dim3(VX_THREADS), 0, (hipStream_t)stream, W, bias, Kvol, Cin, Cout, KG, nct,
                       packed);
    return sad::check_launch("sad_spconv_pack_f32");
}

SAD_API int sad_spconv_f32(const float *feat, const int32_t *nbr, const float *packed, const float *residual, int relu, int Nv, int No, int Kvol,
                           int Cin, int Cout, float *out, sad_stream_t stream) {
    SAD_REQUIRE(packed && (No == 0 || (nbr && out)) && (Nv == 0 || feat), "sad_spconv_f32: NULL pointer");
    SAD_REQUIRE(Nv >= 0 && No >= 0, "sad_spconv_f32: Nv and No must be >= 0 (got %d, %d)", Nv, No);
    if (int rc = sp_channels_ok("sad_spconv_f32", Kvol, Cin, Cout)) return rc;
    if (int rc = sp_rows_ok("sad_spconv_f32", "No", No, Kvol)) return rc;
    SAD_REQUIRE(aligned16(packed), "sad_spconv_f32: packed must be 16-byte aligned");
    if (No == 0) return SAD_OK;
    ConvJob jb = {feat, nbr, packed, residual, out, Nv, No, Kvol, Cin, Cout};
    jb.KG = (Cin + 7) / 8;
    jb.nct = (Cout + 31) / 32;
    jb.LDX = 8 * jb.KG + 4;           // (16-byte aligned rows, four banks apart)
    jb.relu = relu != 0;
    jb.vec_in = Cin % 4 == 0 && aligned16(feat);
    jb.vec_out = Cout % 4 == 0 && aligned16(out) && aligned16(residual);
    const hipStream_t st = (hipStream_t)stream;
    if (jb.nct == 1) return launch_conv<4, 1, 1>(jb, st);     // 128 rows x 32 channels
    if (jb.nct == 2) return launch_conv<2, 1, 1>(jb, st);     //  64 rows x 64
    if (jb.nct <= 4) return launch_conv<1, 2, 1>(jb, st);     //  64 rows x 128
    return launch_conv<1, 2, 2>(jb, st);                      //  64 rows x 256
}

SAD_API int sad_sparse_to_dense_workspace_bytes(int B, const int *out_shape, size_t *out) {
    SAD_REQUIRE(out && out_shape, "sad_sparse_to_dense_workspace_bytes: NULL pointer");
    *out = 0;
    SAD_REQUIRE(B >= 1 && B <= 65535 && out_shape[0] >= 1 && out_shape[1] >= 1 && out_shape[2] >= 1,
                "sad_sparse_to_dense_workspace_bytes: B in 1 .. 65535 and a positive shape expected");
    const unsigned long long cells = (unsigned long long)out_shape[0] * out_shape[1] * out_shape[2];
    if (cells > 2147483647ull || cells * B > 2147483647ull)
        return sad::fail(SAD_EUNSUPPORTED, "sad_sparse_to_dense_workspace_bytes: B * Oz * Oy * Ox must be at most 2^31 - 1");
    *out = al16((size_t)cells * B * 4) + 16;
    return SAD_OK;
}

SAD_API int sad_sparse_to_dense_f32(const float *feat, const int32_t *out_coors, const int32_t *out_offsets, int No, int B, int C,
                                    const int *out_shape, float *dense, void *workspace, sad_stream_t stream) {
    SAD_REQUIRE(out_offsets && dense && workspace && out_shape && (No == 0 || (feat && out_coors)), "sad_sparse_to_dense_f32: NULL pointer");
    SAD_REQUIRE(No >= 0 && C >= 1, "sad_sparse_to_dense_f32: No >= 0 and C >= 1 expected (got %d, %d)", No, C);
    size_t bytes = 0;
    if (int rc = sad_sparse_to_dense_workspace_bytes(B, out_shape, &bytes)) return rc;
    const unsigned cells = (unsigned)out_shape[0] * (unsigned)out_shape[1] * (unsigned)out_shape[2];
    const unsigned long long n = (unsigned long long)B * C * cells;
    if (n >= (1ull << 38)) return sad::fail(SAD_EUNSUPPORTED, "sad_sparse_to_dense_f32: dense[B,C,Oz,Oy,Ox] of %llu floats is too large", n);
    const hipStream_t st = (hipStream_t)stream;
    int32_t *cell = (int32_t *)workspace;
    const unsigned ncell = cells * (unsigned)B;
    hipLaunchKernelGGL(dense_init_kernel, dim3(std::min(blocks_for(ncell, VX_THREADS), 16384u)), dim3(VX_THREADS), 0, st, cell, ncell);
    if (No > 0)
        hipLaunchKernelGGL(dense_owner_kernel, dim3(blocks_for((unsigned long long)No, VX_THREADS)), dim3(VX_THREADS), 0, st, out_coors, out_offsets, No, B,
                           out_shape[0], out_shape[1], out_shape[2], cell);
    hipLaunchKernelGGL(dense_write_kernel, dim3(blocks_for(n, VX_THREADS)), dim3(VX_THREADS), 0, st, feat, cell, C, cells, n, dense);
    return sad::check_launch("sad_sparse_to_dense_f32");
}
