// Backward of the sparse 3-D convolution (SPEC.md §21.4).  The upstream reference has no such operator; the semantics are SPEC.md's own.
//
// transpose  nbrT[i, kk] = the lowest output row o with nbr[o, kk] == i, or -1: fill with -1 (all ones, the largest unsigned), an
//            unsigned atomicMin per valid rulebook entry, then a counting pass for `collisions` (entries that lost their slot to a
//            lower row).  Integer atomics only; nothing that is read back depends on their order.
// grad_feat  needs no kernel of its own: it is sad_spconv_f32 over (g, nbrT, pack(W^T)) (spconv.hip), §21.4.
// grad_W     per kernel offset kk the GEMM g^T [Cout x rows] . gathered feat [rows x Cin] with the OUTPUT ROWS as the reduction
//            dimension, on v_mfma_f32_32x32x2_f32 (A = two rows of g, B = the same two rows of the gathered feat).  A workgroup
//            (4 waves) owns a contiguous range of 64-row tiles and one block of at most 128 x 128 of [Cout x Cin]; a first pass over
//            its part of nbr leaves one mask of needed offsets per tile in LDS.  Then kk ascending: the block's partial stays in
//            accumulator registers over every tile of the range that needs kk (the others cost one LDS read), each such tile's g rows
//            and neighbour rows go through LDS (zero rows for -1, zero columns beyond the block), and the partial is flushed ONCE
//            per (workgroup, kk) by float atomics into grad_W, which the call zeroed.  The order of those additions is not fixed:
//            two calls on the same input may differ in the last bits (SPEC §21.4 allows it; exact inputs are exact in any order).
//            With few output-channel tiles the idle waves split the rows of a tile instead (their partials meet in the atomics).
// grad_bias  column sums of g: per-workgroup partial sums over 1024 rows, one float atomic per (workgroup, channel).
#include "common.h"
#include <algorithm>
#include <limits.h>

namespace {

#include "vox_hash.h"
#include "reg_common.h"

using sad::blocks_for;
#include "spconv_limits.h"
constexpr int SG_TR = 64, SG_MAX_TILES = 1024, SG_BIAS_ROWS = 1024;

// ---- transposed rulebook ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VX_THREADS) void spt_fill_kernel(int32_t *__restrict__ nbrT, unsigned n, int32_t *__restrict__ collisions) {
    grid_fill(nbrT, n, -1);
    if (blockIdx.x == 0 && threadIdx.x == 0) *collisions = 0;
}

__global__ __launch_bounds__(VX_THREADS) void spt_scatter_kernel(const int32_t *__restrict__ nbr, unsigned n, int Kvol, int Nv, unsigned *nbrT) {
    const unsigned e = blockIdx.x * VX_THREADS + threadIdx.x;
    if (e >= n) return;
    const int i = nbr[e];
    if (i < 0 || i >= Nv) return;
    const unsigned o = e / (unsigned)Kvol, kk = e - o * (unsigned)Kvol;
    keep_min(nbrT + (size_t)i * Kvol + kk, o);          // (unsigned: the fill's -1 is the largest)
}

__global__ __launch_bounds__(VX_THREADS) void spt_count_kernel(const int32_t *__restrict__ nbr, unsigned n, int Kvol, int Nv,
                                                               const int32_t *__restrict__ nbrT, int32_t *collisions) {
    const unsigned e = blockIdx.x * VX_THREADS + threadIdx.x;
    bool lost = false;
    if (e < n) {
        const int i = nbr[e];
        if (i >= 0 && i < Nv) {
            const unsigned o = e / (unsigned)Kvol, kk = e - o * (unsigned)Kvol;
            lost = nbrT[(size_t)i * Kvol + kk] != (int)o;
        }
    }
    const unsigned long long m = __ballot(lost);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(collisions, __builtin_popcountll(m));
}

// ---- grad_bias ------------------------------------------------------------------------------------------------------
// CP = the power of two >= Cout (<= 256): thread = (row lane, channel)
__global__ __launch_bounds__(256) void spg_bias_kernel(const float *__restrict__ g, int No, int Cout, int CP, float *grad_bias) {
    __shared__ float s_sum[256];
    const int tid = threadIdx.x, c = tid & (CP - 1), rl = tid / CP, nrl = 256 / CP;
    const long long r0 = (long long)blockIdx.x * SG_BIAS_ROWS, r1 = r0 + SG_BIAS_ROWS < No ? r0 + SG_BIAS_ROWS : No;
    float sum = 0.0f;
    if (c < Cout)
        for (long long r = r0 + rl; r < r1; r += nrl) sum += g[r * Cout + c];
    s_sum[tid] = sum;
    __syncthreads();
    if (rl == 0 && c < Cout) {
        for (int q = 1; q < nrl; ++q) sum += s_sum[q * CP + c];
        unsafeAtomicAdd(grad_bias + c, sum);
    }
}

// ---- grad_W ---------------------------------------------------------------------------------------------------------
struct GradJob {
    const float *feat;
    const int32_t *nbr;
    const float *g;
    float *gw;
    int Nv, No, Kvol, Cin, Cout;
    int nib;                      // blocks along Cin (blockIdx.y = co block * nib + ci block)
    int bco, bci;                 // channels of a block along Cout / Cin (multiples of 32, <= 128)
    int WC, LDG, LDF;             // waves along Cout (1, 2, 4); floats between rows of the two LDS images
    int tiles_per_wg, ntiles;
    int vec_f, vec_g;
};

// NT = 32-channel tiles of Cin a wave holds (the LDS image of feat is 32 NT wide); a wave owns ONE 32-channel tile of Cout
template <int NT>
__global__ __launch_bounds__(256) void spconv_grad_w_kernel(const GradJob jb) {
    extern __shared__ __attribute__((aligned(16))) float sg_smem[];
    float *s_f = sg_smem;                                        // [SG_TR][LDF]
    float *s_g = s_f + SG_TR * jb.LDF;                           // [SG_TR][LDG]
    unsigned *s_mask = reinterpret_cast<unsigned *>(s_g + SG_TR * jb.LDG);   // [tiles_per_wg]: bit kk = some row of the tile has a neighbour at kk
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int Kvol = jb.Kvol, LDF = jb.LDF, LDG = jb.LDG, WC = jb.WC;
    const int wc = wave & (WC - 1), wk = wave / WC, RW = SG_TR / (4 / WC);   // this wave: channel tile wc of the block, rows wk RW .. + RW of every tile
    const int cb = blockIdx.y / jb.nib, ib = blockIdx.y - cb * jb.nib;
    const int co0 = cb * jb.bco, ci0 = ib * jb.bci;
    const int vco = min(jb.bco, jb.Cout - co0), vci = min(jb.bci, jb.Cin - ci0);   // valid columns of the two images (zero beyond)
    const int tile0 = blockIdx.x * jb.tiles_per_wg, nt = min(jb.tiles_per_wg, jb.ntiles - tile0);
    const long long rowbeg = (long long)tile0 * SG_TR, rowlim = rowbeg + (long long)nt * SG_TR, rowend = rowlim < jb.No ? rowlim : jb.No;

    for (int t = tid; t < nt; t += 256) s_mask[t] = 0u;
    __syncthreads();
    for (long long e = rowbeg * Kvol + tid; e < rowend * Kvol; e += 256) {
        const int n = jb.nbr[e];
        if (n < 0 || n >= jb.Nv) continue;                       // (never read outside feat, whatever the caller passed)
        const long long row = e / Kvol;
        const int kk = (int)(e - row * Kvol), t = (int)((row - rowbeg) >> 6);
        if (!((s_mask[t] >> kk) & 1u)) atomicOr(&s_mask[t], 1u << kk);
    }
    __syncthreads();
    unsigned all = 0u;
    for (int t = 0; t < nt; ++t) all |= s_mask[t];
    all = __builtin_amdgcn_readfirstlane(all);

    const int CQF = 8 * NT, CQG = 8 * WC;                        // float4 per row of the two images
#pragma unroll 1
    for (int kk = 0; kk < Kvol; ++kk) {
        if (!((all >> kk) & 1u)) continue;                       // (workgroup-uniform: no row of the range reads this offset; grad_W[kk] of it stays zero)
        f32x16 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[t][q] = 0.0f;
#pragma unroll 1
        for (int tt = 0; tt < nt; ++tt) {
            if (!((s_mask[tt] >> kk) & 1u)) continue;            // (workgroup-uniform)
            const long long row0 = rowbeg + (long long)tt * SG_TR;
            __syncthreads();                                     // the previous tile's rows are no longer read
            for (int idx = tid; idx < SG_TR * CQF; idx += 256) {
                const int r = idx / CQF, c0 = 4 * (idx - r * CQF);
                const long long row = row0 + r;
                int n = row < jb.No ? jb.nbr[row * Kvol + kk] : -1;
                if (n >= jb.Nv) n = -1;
                // (vec_f: Cin % 4 == 0, so vci is a multiple of 4 too)
                *reinterpret_cast<float4 *>(s_f + r * LDF + c0) = row_quad(jb.feat + ci0, n, jb.Cin, c0, vci, jb.vec_f);
            }
            for (int idx = tid; idx < SG_TR * CQG; idx += 256) {
                const int r = idx / CQG, c0 = 4 * (idx - r * CQG);
                const long long row = row0 + r;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (row < jb.No && c0 < vco) {
                    const float *src = jb.g + (size_t)row * jb.Cout + co0 + c0;
                    if (jb.vec_g) {
                        v = *reinterpret_cast<const float4 *>(src);
                    } else {
                        v.x = src[0];
                        if (c0 + 1 < vco) v.y = src[1];
                        if (c0 + 2 < vco) v.z = src[2];
                        if (c0 + 3 < vco) v.w = src[3];
                    }
                }
                *reinterpret_cast<float4 *>(s_g + r * LDG + c0) = v;
            }
            __syncthreads();
            // lane (j, h): A = g[row r + h][32 wc + j], B = feat row of (r + h) [32 t + j]; LDG, LDF = 32 mod 64 floats: the two half-waves
            // read disjoint banks
            const float *pa = s_g + (wk * RW + h) * LDG + wc * 32 + j;
            const float *pb = s_f + (wk * RW + h) * LDF + j;
            for (int r = 0; r < RW; r += 2) {
                const float a = pa[r * LDG];
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, pb[r * LDF + 32 * t], acc[t], 0, 0, 0);
            }
        }
        // ---- flush: lane = input channel 32 t + j, registers 4a .. 4a+3 = output channels 32 wc + 8 a + 4 h .. + 3 ----
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int ci = 32 * t + j;
            if (ci >= vci) continue;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int co = wc * 32 + 8 * a + 4 * h + e;
                    if (co < vco) unsafeAtomicAdd(jb.gw + ((size_t)kk * jb.Cout + co0 + co) * jb.Cin + ci0 + ci, acc[t][4 * a + e]);
                }
            }
        }
    }
}

template <int NT>
int launch_grad_w(const GradJob &jb, unsigned nranges, unsigned nblk, hipStream_t st) {
    const size_t lds = ((size_t)SG_TR * (jb.LDF + jb.LDG) + jb.tiles_per_wg + 4) * 4;
    static std::atomic<uint64_t> done{0};
    sad::lds_attr_once(done, reinterpret_cast<const void *>(&spconv_grad_w_kernel<NT>), 160 * 1024);
    hipLaunchKernelGGL((spconv_grad_w_kernel<NT>), dim3(nranges, nblk), dim3(256), lds, st, jb);
    return sad::check_launch("sad_spconv_grad_weight_f32");
}

inline int pow2_tiles(int t) { return t >= 3 ? 4 : t; }          // 1, 2, 3, 4 tiles -> 1, 2, 4, 4
inline int lds_stride(int width) { return (width / 32) % 2 ? width : width + 32; }   // = 32 mod 64 floats

}  // namespace

SAD_API int sad_spconv_index_transpose(const int32_t *nbr, int No, int Nv, int Kvol, int32_t *nbrT, int32_t *collisions, sad_stream_t stream) {
    SAD_REQUIRE(collisions && (No == 0 || nbr) && (Nv == 0 || nbrT), "sad_spconv_index_transpose: NULL pointer");
    SAD_REQUIRE(No >= 0 && Nv >= 0, "sad_spconv_index_transpose: No and Nv must be >= 0 (got %d, %d)", No, Nv);
    if (int rc = sp_kvol_ok("sad_spconv_index_transpose", Kvol)) return rc;
    if (int rc = sp_rows_ok("sad_spconv_index_transpose", "No", No, Kvol)) return rc;
    if (int rc = sp_rows_ok("sad_spconv_index_transpose", "Nv", Nv, Kvol)) return rc;
    const hipStream_t st = (hipStream_t)stream;
    const unsigned nT = (unsigned)Nv * (unsigned)Kvol, n = (unsigned)No * (unsigned)Kvol;
    const unsigned fb = std::min(blocks_for(nT, VX_THREADS), 16384u);
    hipLaunchKernelGGL(spt_fill_kernel, dim3(fb ? fb : 1), dim3(VX_THREADS), 0, st, nbrT, nT, collisions);
    if (n > 0 && nT > 0) {
        hipLaunchKernelGGL(spt_scatter_kernel, dim3(blocks_for(n, VX_THREADS)), dim3(VX_THREADS), 0, st, nbr, n, Kvol, Nv, (unsigned *)nbrT);
        hipLaunchKernelGGL(spt_count_kernel, dim3(blocks_for(n, VX_THREADS)), dim3(VX_THREADS), 0, st, nbr, n, Kvol, Nv, (const int32_t *)nbrT, collisions);
    }
    return sad::check_launch("sad_spconv_index_transpose");
}

SAD_API int sad_spconv_grad_weight_workspace_bytes(int No, int Kvol, int Cin, int Cout, size_t *out) {
    SAD_REQUIRE(out, "sad_spconv_grad_weight_workspace_bytes: NULL out");
    *out = 0;
    SAD_REQUIRE(No >= 0, "sad_spconv_grad_weight_workspace_bytes: No must be >= 0 (got %d)", No);
    if (int rc = sp_channels_ok("sad_spconv_grad_weight_workspace_bytes", Kvol, Cin, Cout)) return rc;
    return SAD_OK;                                               // the partials meet in grad_W itself (float atomics): no scratch
}

SAD_API int sad_spconv_grad_weight_f32(const float *feat, const int32_t *nbr, const float *g, int Nv, int No, int Kvol, int Cin, int Cout,
                                       float *grad_W, float *grad_bias, void *workspace, sad_stream_t stream) {
    (void)workspace;
    SAD_REQUIRE((grad_W || grad_bias) && (No == 0 || g) && (!grad_W || ((No == 0 || nbr) && (Nv == 0 || feat))), "sad_spconv_grad_weight_f32: NULL pointer");
    SAD_REQUIRE(Nv >= 0 && No >= 0, "sad_spconv_grad_weight_f32: Nv and No must be >= 0 (got %d, %d)", Nv, No);
    if (int rc = sp_channels_ok("sad_spconv_grad_weight_f32", Kvol, Cin, Cout)) return rc;
    if (int rc = sp_rows_ok("sad_spconv_grad_weight_f32", "No", No, Kvol)) return rc;
    const hipStream_t st = (hipStream_t)stream;
    if ((grad_W && hipMemsetAsync(grad_W, 0, (size_t)Kvol * Cout * Cin * sizeof(float), st) != hipSuccess) ||
        (grad_bias && hipMemsetAsync(grad_bias, 0, (size_t)Cout * sizeof(float), st) != hipSuccess))
        return sad::check_launch("sad_spconv_grad_weight_f32");
    if (No == 0) return SAD_OK;
    if (grad_bias) {
        int CP = 1;
        while (CP < Cout) CP <<= 1;
        hipLaunchKernelGGL(spg_bias_kernel, dim3(blocks_for((unsigned long long)No, SG_BIAS_ROWS)), dim3(256), 0, st, g, No, Cout, CP, grad_bias);
    }
    if (Nv == 0 || !grad_W) return sad::check_launch("sad_spconv_grad_weight_f32");      // (grad_W == NULL: a frozen weight pays for the column sums only)
    GradJob jb = {feat, nbr, g, grad_W, Nv, No, Kvol, Cin, Cout};
    const int ncot = (Cout + 31) / 32, ncit = (Cin + 31) / 32;   // 32-channel tiles, 1 .. 8 each
    const int ncb = (ncot + 3) / 4;
    jb.nib = (ncit + 3) / 4;
    const int tco = (ncot + ncb - 1) / ncb, tci = (ncit + jb.nib - 1) / jb.nib;   // tiles per block, 1 .. 4
    jb.bco = 32 * tco;
    jb.bci = 32 * tci;
    jb.WC = pow2_tiles(tco);
    const int NT = pow2_tiles(tci);
    jb.LDG = lds_stride(32 * jb.WC);
    jb.LDF = lds_stride(32 * NT);
    jb.ntiles = (int)(((long long)No + SG_TR - 1) / SG_TR);
    const int nblk = ncb * jb.nib;
    // row ranges: a grid of two workgroups per compute unit over all blocks (the 128 x 128 block keeps ONE resident per unit: 84 KB of LDS,
    // so half of that grid starts when the first half ends); the test knob spconv_grad_ranges overrides the count
    const int knob = sad::get_option(sad::OPT_SPCONV_GRAD_RANGES);
    const int target = knob > 0 ? knob : std::max(1, 2 * sad::device_cus() / nblk);
    jb.tiles_per_wg = std::min(SG_MAX_TILES, std::max(1, (jb.ntiles + target - 1) / target));
    const unsigned nranges = (unsigned)((jb.ntiles + jb.tiles_per_wg - 1) / jb.tiles_per_wg);
    jb.vec_f = Cin % 4 == 0 && aligned16(feat);
    jb.vec_g = Cout % 4 == 0 && aligned16(g);
    if (NT == 1) return launch_grad_w<1>(jb, nranges, (unsigned)nblk, st);
    if (NT == 2) return launch_grad_w<2>(jb, nranges, (unsigned)nblk, st);
    return launch_grad_w<4>(jb, nranges, (unsigned)nblk, st);
}
