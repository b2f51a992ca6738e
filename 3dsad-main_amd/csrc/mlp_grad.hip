// Backward of the MLP chains (SPEC.md §32): the grouped chain + max-pool of §6 and plain rows.  The upstream reference has no such
// operator; the semantics are SPEC.md's own.
//
// Nothing but the inputs and the pooled output is kept between forward and backward: §6 is bit-reproducible, so the activations
// are RECOMPUTED here (same fmaf chain, k ascending, on v_mfma_f32_32x32x2_f32) and every routing decision (ReLU live or dead,
// which sample won the max) is taken on those bits.  `mismatch` counts the (group, channel) pairs whose pooled value no recomputed
// row attains: 0 whenever `pooled` came from the library's forward with the same weights.
//
// rows      the rows that exist, max(cnt, 1) per group, numbered by the forward's row-packing scan (mlp_rowscan.hip, its split form:
//           gstart[g] = first packed row of group g); without counts row = g S + s.  Groups are processed in chunks of Gc groups, a
//           chunk's rows are at most Gc S: the activations X_0 .. X_L of ONE chunk, [rows, C_l] each, live in the workspace.  The row
//           count of a chunk is only known on the device: grids are sized for Gc S rows and tiles beyond the count leave at once.
// gather    X_0 = [xyz[idx] - new_xyz | feat[idx]]; a skipped group (skip_empty, cnt == 0) gets a zero row (its coordinates may be NaN).
// recompute X_l = act(b_l + X_{l-1} W_l^T): one generic MFMA GEMM (below) per layer, bias in the accumulators, k ascending.
// route     one wave per group: arg[o] = the lowest row with X_L == pooled, D_L = grad_out at that row where X_L > 0, written over X_L.
// grad_W    D_l^T X_{l-1}, the rows as the reduction dimension, split over the workgroups of blockIdx.z, each flushing its
//           partial once with float atomics into the zeroed output; grad_b: column sums of D_l, atomics likewise.
// D_{l-1}   D_l W_l with the ReLU selection on X_{l-1} in the epilogue, written over X_{l-1} (after grad_W_l has read it).
// layer 1   G_0 only for the columns that are asked for, written over X_0, scattered by float atomics into grad_feat / grad_xyz
//           (zeros are not sent); grad_new_xyz is a per-group sum without atomics.
// The three GEMMs are ONE kernel: C[i][j] (+)= sum_k A(i,k) B(k,j) with strided operands staged through LDS k-major, a 128 x 64
// tile per workgroup, wave w holding rows 32 w .. 32 w + 31 of it in two accumulators.  In every product of a chain i is a
// channel index and j or k the row index, so a lane's 16 accumulator values are 16 channels of one row.
#include "common.h"
#include <algorithm>

namespace {

#include "reg_common.h"

using sad::blocks_for;
// LDS row strides = 33 mod 64 floats: a k-fast fill (16 .. 32 consecutive k of one column per wave step) and the two half-waves of a
// fragment read (rows k and k + 1) both spread over the banks
constexpr int MG_TI = 128, MG_TJ = 64, MG_TK = 32, MG_LDA = 161, MG_LDB = 97;
constexpr int MG_HDR = 64;                                                       // bytes in front of the workspace: int32 mismatch
enum { MG_FWD = 0, MG_DGRAD = 1, MG_WGRAD = 2 };
enum { NEED_FEAT = 1, NEED_XYZ = 2, NEED_NEW_XYZ = 4, NEED_PARAMS = 8 };

// the rows of one chunk: groups g0 .. g1 - 1 (grouped form) or `nhost` plain rows
struct Chunk {
    const int *gs;                 // gstart[ngroups + 1] of the scan, NULL: no counts (row = g S + s) or plain rows
    const int *row_src, *row_gid;  // the scan's row map (with gs)
    int g0, g1, S;
    int nhost, cap;                // rows when gs == NULL; capacity of the chunk's buffers in rows
};
__device__ __forceinline__ int gstart_of(const Chunk &c, int g) { return c.gs ? c.gs[g] : g * c.S; }
__device__ __forceinline__ int chunk_rows(const Chunk &c) {
    const int n = c.gs ? c.gs[c.g1] - c.gs[c.g0] : c.nhost;
    return n < 0 ? 0 : (n > c.cap ? c.cap : n);                 // (never beyond the buffers, whatever the counts held)
}

struct Gemm {
    const float *A; long long sai, sak;
    const float *B; long long sbk, sbj;
    int I, J, K;                   // bounds; the row dimension (J, or K of MG_WGRAD) is the chunk's
    Chunk ch;
    const float *bias;             // MG_FWD: start value of row i
    int relu;                      // MG_FWD
    const float *sel; long long ldsel;   // MG_DGRAD: keep C[i][j] where sel[j][i] > 0 (NULL: keep all)
    float *C; long long sci, scj;
};

template <int MODE>
__global__ __launch_bounds__(256) void mg_gemm_kernel(const Gemm p) {
    __shared__ float s_a[MG_TK * MG_LDA];
    __shared__ float s_b[MG_TK * MG_LDB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, h = lane >> 5;
    const int rows = chunk_rows(p.ch);
    const int J = MODE == MG_WGRAD ? p.J : rows;
    int kbeg = 0, kend = p.K;
    if (MODE == MG_WGRAD) {                                      // the rows that exist, dealt evenly to the workgroups of blockIdx.z
        const int klen = ((rows + (int)gridDim.z - 1) / (int)gridDim.z + MG_TK - 1) / MG_TK * MG_TK;
        kbeg = blockIdx.z * klen;
        kend = min(rows, kbeg + klen);
    }
    const int i0 = blockIdx.y * MG_TI, j0 = blockIdx.x * MG_TJ;
    if (j0 >= J || kbeg >= kend) return;                         // (workgroup-uniform)
    f32x16 acc[2];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = i0 + 32 * wave + 8 * a + 4 * h + e;
            const float v = (MODE == MG_FWD && i < p.I) ? p.bias[i] : 0.0f;
            acc[0][4 * a + e] = v;
            acc[1][4 * a + e] = v;
        }
    const bool a_kfast = p.sak == 1, b_kfast = p.sbk == 1;
#pragma unroll 1
    for (int k0 = kbeg; k0 < kend; k0 += MG_TK) {
        __syncthreads();                                         // the previous images are no longer read
        for (int e = tid; e < MG_TK * MG_TI; e += 256) {
            const int kk = a_kfast ? e % MG_TK : e / MG_TI, i = a_kfast ? e / MG_TK : e % MG_TI;
            float v = 0.0f;
            if (i0 + i < p.I && k0 + kk < kend) v = p.A[(long long)(i0 + i) * p.sai + (long long)(k0 + kk) * p.sak];
            s_a[kk * MG_LDA + i] = v;
        }
        for (int e = tid; e < MG_TK * MG_TJ; e += 256) {
            const int kk = b_kfast ? e % MG_TK : e / MG_TJ, jj = b_kfast ? e / MG_TK : e % MG_TJ;
            float v = 0.0f;
            if (j0 + jj < J && k0 + kk < kend) v = p.B[(long long)(k0 + kk) * p.sbk + (long long)(j0 + jj) * p.sbj];
            s_b[kk * MG_LDB + jj] = v;
        }
        __syncthreads();
        // lane (j, h): A[32 wave + j][kk + h], B[kk + h][j] and B[kk + h][32 + j]; k ascending
        const float *pa = s_a + h * MG_LDA + 32 * wave + j;
        const float *pb = s_b + h * MG_LDB + j;
#pragma unroll
        for (int kk = 0; kk < MG_TK; kk += 2) {
            const float a = pa[kk * MG_LDA];
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, pb[kk * MG_LDB], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, pb[kk * MG_LDB + 32], acc[1], 0, 0, 0);
        }
    }
    // lane = column 32 t + j, registers 4 a .. 4 a + 3 = rows 32 wave + 8 a + 4 h .. + 3
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int jj = j0 + 32 * t + j;
        if (jj >= J) continue;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = i0 + 32 * wave + 8 * a + 4 * h + e;
                if (i >= p.I) continue;
                float v = acc[t][4 * a + e];
                float *dst = p.C + (long long)i * p.sci + (long long)jj * p.scj;
                if (MODE == MG_FWD) {
                    *dst = p.relu ? (v > 0.0f ? v : 0.0f) : v;
                } else if (MODE == MG_DGRAD) {
                    if (p.sel && !(p.sel[(long long)jj * p.ldsel + i] > 0.0f)) v = 0.0f;    // (a selection: NaN is dead)
                    *dst = v;
                } else if (v != 0.0f) {                          // (NaN != 0: it is sent)
                    unsafeAtomicAdd(dst, v);
                }
            }
    }
}

struct GatherJob {
    const float *xyz, *new_xyz, *feat;
    const int32_t *idx, *cnt;
    int ld_feat, N, M, C, skip_empty;
    long long ngroups, npoints;    // B M, B N
    Chunk ch;
    float *x0;                     // [rows, 3 + C]
};

// packed row q of the launch -> (source point, group), both inside their arrays whatever idx / the row map held
__device__ __forceinline__ void row_of(const GatherJob &jb, int q, long long &src, long long &g) {
    if (jb.ch.gs) {
        src = jb.ch.row_src[q];
        g = jb.ch.row_gid[q] & sad::GID_MASK;
    } else {
        g = q / jb.ch.S;
        int n = jb.idx[q];
        n = n < 0 ? 0 : (n >= jb.N ? jb.N - 1 : n);
        src = (g / jb.M) * jb.N + n;
    }
    src = src < 0 ? 0 : (src >= jb.npoints ? jb.npoints - 1 : src);
    g = g < 0 ? 0 : (g >= jb.ngroups ? jb.ngroups - 1 : g);
}

__global__ __launch_bounds__(256) void mg_gather_kernel(const GatherJob jb) {
    const int C0 = 3 + jb.C, rows = chunk_rows(jb.ch);
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long lr = e / C0;
    if (lr >= rows) return;
    const int c = (int)(e - lr * C0);
    long long src, g;
    row_of(jb, gstart_of(jb.ch, jb.ch.g0) + (int)lr, src, g);
    float v = 0.0f;
    if (!(jb.skip_empty && jb.cnt && jb.cnt[g] <= 0))
        v = c < 3 ? jb.xyz[src * 3 + c] - jb.new_xyz[g * 3 + c] : jb.feat[src * jb.ld_feat + (c - 3)];
    jb.x0[e] = v;
}

// the inverse: G_0 [rows, 3 + C], columns c_lo .. c_hi - 1 of it, into grad_xyz [B N, 3] / grad_feat [B N, C]
__global__ __launch_bounds__(256) void mg_scatter_kernel(const GatherJob jb, int c_lo, int c_hi, float *grad_xyz, float *grad_feat) {
    const int C0 = 3 + jb.C, W = c_hi - c_lo, rows = chunk_rows(jb.ch);
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long lr = e / W;
    if (lr >= rows) return;
    const int c = c_lo + (int)(e - lr * W);
    const float v = jb.x0[lr * C0 + c];
    if (!(v != 0.0f)) return;
    long long src, g;
    row_of(jb, gstart_of(jb.ch, jb.ch.g0) + (int)lr, src, g);
    if (c < 3) {
        if (grad_xyz) unsafeAtomicAdd(grad_xyz + src * 3 + c, v);
    } else if (grad_feat) {
        unsafeAtomicAdd(grad_feat + src * jb.C + (c - 3), v);
    }
}

// grad_new_xyz[g][d] = - sum over the group's rows of G_0[row][d]: every group lies in one chunk, plain stores
__global__ __launch_bounds__(256) void mg_new_xyz_kernel(const Chunk ch, const float *g0buf, int C0, float *grad_new_xyz) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int g = ch.g0 + e / 3, d = e % 3;
    if (g >= ch.g1) return;
    const int rows = chunk_rows(ch), base = gstart_of(ch, ch.g0);
    int rb = gstart_of(ch, g) - base, re = gstart_of(ch, g + 1) - base;
    rb = rb < 0 ? 0 : rb;
    re = re > rows ? rows : re;
    float s = 0.0f;
    for (int r = rb; r < re; ++r) s += g0buf[(long long)r * C0 + d];
    grad_new_xyz[(long long)g * 3 + d] = 0.0f - s;
}

struct RouteJob {
    Chunk ch;
    float *xl;                     // [rows, CL]: X_L in, D_L out
    int CL;
    const float *pooled; long long ldp;      // row g at pooled + g ldp
    const float *gout; long long ldg;
    const int32_t *cnt;
    int skip_empty;
    int *mismatch;
};

__global__ __launch_bounds__(256) void mg_route_kernel(const RouteJob jb) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = jb.ch.g0 + blockIdx.x * 4 + wave;
    if (g >= jb.ch.g1) return;
    const int rows = chunk_rows(jb.ch), base = gstart_of(jb.ch, jb.ch.g0);
    int rb = gstart_of(jb.ch, g) - base, re = gstart_of(jb.ch, g + 1) - base;
    rb = rb < 0 ? 0 : rb;
    re = re > rows ? rows : re;
    const bool dead = jb.skip_empty && jb.cnt && jb.cnt[g] <= 0;
    int bad = 0;
    for (int o = lane; o < jb.CL; o += 64) {
        const float pv = jb.pooled[(long long)g * jb.ldp + o], go = jb.gout[(long long)g * jb.ldg + o];
        int arg = -1;
        if (!dead) {
            for (int r = rb; r < re; ++r)
                if (jb.xl[(long long)r * jb.CL + o] == pv) { arg = r; break; }
            if (arg < 0) ++bad;
        }
        for (int r = rb; r < re; ++r) {
            float *px = jb.xl + (long long)r * jb.CL + o;
            *px = (r == arg && *px > 0.0f) ? go : 0.0f;
        }
    }
    for (int off = 32; off >= 1; off >>= 1) bad += __shfl_xor(bad, off, 64);
    if (lane == 0 && bad) atomicAdd(jb.mismatch, bad);
}

// plain rows: D_L = grad_out where X_L > 0 (relu) or everywhere, written over X_L
__global__ __launch_bounds__(256) void mg_rows_dl_kernel(float *xl, int CL, int rows, const float *gout, long long ldg, int relu) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long r = e / CL;
    if (r >= rows) return;
    const int o = (int)(e - r * CL);
    const float go = gout[r * ldg + o];
    xl[e] = (!relu || xl[e] > 0.0f) ? go : 0.0f;
}

// grad_b[o] += sum over the chunk's rows of D[row][o]: 64 channels x 4 row lanes per workgroup, 512 rows each
__global__ __launch_bounds__(256) void mg_colsum_kernel(const Chunk ch, const float *d, int Co, float *grad_b) {
    __shared__ float s_sum[256];
    const int tid = threadIdx.x, c = blockIdx.y * 64 + (tid & 63), rl = tid >> 6;
    const int rows = chunk_rows(ch);
    const int r0 = blockIdx.x * 512, r1 = min(rows, r0 + 512);
    float sum = 0.0f;
    if (c < Co)
        for (int r = r0 + rl; r < r1; r += 4) sum += d[(long long)r * Co + c];
    s_sum[tid] = sum;
    __syncthreads();
    if (rl == 0 && c < Co) {
        for (int q = 1; q < 4; ++q) sum += s_sum[q * 64 + (tid & 63)];
        if (sum != 0.0f) unsafeAtomicAdd(grad_b + c, sum);
    }
}

template <int MODE>
void launch_gemm(const Gemm &p, int jmax, int nz, hipStream_t st) {
    if (p.I < 1 || jmax < 1) return;
    hipLaunchKernelGGL((mg_gemm_kernel<MODE>), dim3(blocks_for(jmax, MG_TJ), blocks_for(p.I, MG_TI), nz), dim3(256), 0, st, p);
}

long long sum_dims(const int *dims, int from, int L) {
    long long s = 0;
    for (int l = from; l <= L; ++l) s += dims[l];
    return s;
}

int mg_shape_ok(const char *fn, int B, int M, int S, int L, const int *dims) {
    SAD_REQUIRE(dims, "%s: NULL dims", fn);
    SAD_REQUIRE(B >= 1 && M >= 1, "%s: B and M must be >= 1 (got %d, %d)", fn, B, M);
    SAD_REQUIRE(L >= 1 && L <= SAD_MAX_LAYERS, "%s: L = %d (1 .. %d layers)", fn, L, SAD_MAX_LAYERS);
    SAD_REQUIRE(S >= 1 && S <= 64, "%s: S = %d (1 .. 64 samples)", fn, S);
    for (int l = 0; l <= L; ++l) SAD_REQUIRE(dims[l] >= 1 && dims[l] <= 65536, "%s: dims[%d] = %d (1 .. 65536)", fn, l, dims[l]);
    if ((long long)B * M * S >= (1LL << 29)) return sad::fail(SAD_EUNSUPPORTED, "%s: B * M * S must be below 2^29", fn);
    return SAD_OK;
}

struct Plan { size_t table, act0, per_row; long long min_rows, all_rows; };
// grouped: X_0 .. X_L of a chunk; plain rows: X_1 .. X_L (X_0 is the caller's x)
Plan mg_plan(int B, int M, int S, int grouped, int has_cnt, int L, const int *dims) {
    Plan pl;
    pl.table = (grouped && has_cnt) ? sad::al16(sad_mlp_workspace_bytes(B, M, S)) : 0;
    pl.act0 = MG_HDR + pl.table;
    pl.per_row = sizeof(float) * (size_t)sum_dims(dims, grouped ? 0 : 1, L);
    const long long ng = (long long)B * M;
    pl.min_rows = std::min<long long>(ng, 64) * S;               // at least 64 groups (or rows) per chunk
    pl.all_rows = ng * S;
    return pl;
}

}  // namespace

SAD_API int sad_mlp_grad_workspace_bytes(int B, int M, int S, int grouped, int has_cnt, int L, const int *dims, size_t *min_bytes, size_t *full_bytes) {
    SAD_REQUIRE(min_bytes && full_bytes, "sad_mlp_grad_workspace_bytes: NULL out");
    *min_bytes = *full_bytes = 0;
    if (int rc = mg_shape_ok("sad_mlp_grad_workspace_bytes", B, M, grouped ? S : 1, L, dims)) return rc;
    const Plan pl = mg_plan(B, M, grouped ? S : 1, grouped, has_cnt, L, dims);
    *min_bytes = pl.act0 + pl.per_row * (size_t)pl.min_rows;
    *full_bytes = pl.act0 + pl.per_row * (size_t)pl.all_rows;
    return SAD_OK;
}

SAD_API int sad_mlp_grad_f32(const sad_mlp_grad_args *a, sad_stream_t stream) {
    const char *fn = "sad_mlp_grad_f32";
    if (int rc = args_ok(fn, a)) return rc;
    const bool grouped = a->idx != nullptr;
    const int S = grouped ? a->S : 1, L = a->L;
    if (int rc = mg_shape_ok(fn, a->B, a->M, S, L, a->dims)) return rc;
    const int *dims = a->dims;
    const int C0 = dims[0], CL = dims[L];
    SAD_REQUIRE(a->workspace && (uintptr_t)a->workspace % 16 == 0, "%s: workspace must be non-NULL and 16-byte aligned", fn);
    SAD_REQUIRE(a->grad_out && a->ld_grad >= 1 && a->col_off >= 0 && a->col_off + CL <= a->ld_grad, "%s: grad_out: need col_off + C_L <= ld_grad", fn);
    SAD_REQUIRE((a->need & ~15) == 0 && a->need != 0, "%s: need = %d (a non-empty mask of bits 1, 2, 4, 8)", fn, a->need);
    for (int l = 0; l < L; ++l) {
        SAD_REQUIRE(a->W[l] && a->b[l], "%s: NULL weights of layer %d", fn, l);
        if (a->need & NEED_PARAMS) SAD_REQUIRE(a->grad_W[l] && a->grad_b[l], "%s: NULL grad_W / grad_b of layer %d", fn, l);
    }
    if (grouped) {
        SAD_REQUIRE(a->xyz && a->new_xyz && a->pooled, "%s: NULL xyz / new_xyz / pooled", fn);
        SAD_REQUIRE(a->N >= 1 && a->C >= 0 && C0 == a->C + 3, "%s: dims[0] = %d, C + 3 = %d", fn, C0, a->C + 3);
        SAD_REQUIRE(a->C == 0 || (a->feat && a->ld_feat >= a->C), "%s: feat: NULL or ld_feat < C", fn);
        SAD_REQUIRE(a->ld_pooled >= 1 && a->pooled_off >= 0 && a->pooled_off + CL <= a->ld_pooled, "%s: pooled: need pooled_off + C_L <= ld_pooled", fn);
        SAD_REQUIRE(a->relu_mask == (1 << L) - 1, "%s: a grouped chain has a ReLU after every layer", fn);
        SAD_REQUIRE(!(a->need & NEED_FEAT) || (a->C > 0 && a->grad_feat), "%s: grad_feat asked for without features or buffer", fn);
        SAD_REQUIRE(!(a->need & NEED_XYZ) || a->grad_xyz, "%s: NULL grad_xyz", fn);
        SAD_REQUIRE(!(a->need & NEED_NEW_XYZ) || a->grad_new_xyz, "%s: NULL grad_new_xyz", fn);
        if ((long long)a->B * a->N >= (1LL << 31)) return sad::fail(SAD_EUNSUPPORTED, "%s: B * N must be below 2^31", fn);
    } else {
        SAD_REQUIRE(a->B == 1 && a->feat && a->ld_feat >= C0 && a->C == C0, "%s: plain rows: B = 1, x [M, dims[0]] in feat, C = dims[0]", fn);
        SAD_REQUIRE((a->need & (NEED_XYZ | NEED_NEW_XYZ)) == 0, "%s: plain rows have no coordinate gradients", fn);
        SAD_REQUIRE(!(a->need & NEED_FEAT) || a->grad_feat, "%s: NULL grad_x", fn);
    }
    const bool has_cnt = grouped && a->cnt;
    const Plan pl = mg_plan(a->B, a->M, S, grouped, has_cnt, L, dims);
    SAD_REQUIRE(a->workspace_bytes >= pl.act0 + pl.per_row * (size_t)pl.min_rows, "%s: workspace of %zu bytes is below the minimum (sad_mlp_grad_workspace_bytes)", fn, a->workspace_bytes);
    const hipStream_t st = (hipStream_t)stream;
    const long long ng = (long long)a->B * a->M;
    char *ws = (char *)a->workspace;
    int *mismatch = (int *)ws;
    bool ok = hipMemsetAsync(ws, 0, MG_HDR, st) == hipSuccess;
    if (a->need & NEED_PARAMS)
        for (int l = 0; l < L && ok; ++l)
            ok = hipMemsetAsync(a->grad_W[l], 0, sizeof(float) * (size_t)dims[l + 1] * dims[l], st) == hipSuccess &&
                 hipMemsetAsync(a->grad_b[l], 0, sizeof(float) * (size_t)dims[l + 1], st) == hipSuccess;
    if (ok && grouped && (a->need & NEED_FEAT)) ok = hipMemsetAsync(a->grad_feat, 0, sizeof(float) * (size_t)a->B * a->N * a->C, st) == hipSuccess;
    if (ok && grouped && (a->need & NEED_XYZ)) ok = hipMemsetAsync(a->grad_xyz, 0, sizeof(float) * (size_t)a->B * a->N * 3, st) == hipSuccess;
    if (!ok) return sad::check_launch(fn);

    Chunk base{};
    base.S = S;
    if (has_cnt) {
        // the forward's scan in its split form: the row map and gstart[g], the first packed row of every group
        int *tab = (int *)(ws + MG_HDR);
        sad::ScanJob sj = sad::make_scan_job(a->cnt, (int)ng, S, 32, tab, 0, a->idx, a->N, a->M);
        sj.split = 1;
        sj.cont0 = nullptr;
        sj.cont_cols = 0;
        if (int rc = sad::launch_rowscan_multi(&sj, 1, st)) return rc;
        base.gs = sj.gstart;
        base.row_src = sj.row_src;
        base.row_gid = sj.row_gid;
    }
    // chunk size from the byte budget: whole groups, S rows each at most
    const long long room = (long long)((a->workspace_bytes - pl.act0) / pl.per_row);
    long long gc = std::min(ng, room / S);
    if (gc * S > (1LL << 30)) gc = (1LL << 30) / S;
    float *X[SAD_MAX_LAYERS + 1];
    {
        float *p = (float *)(ws + pl.act0);
        for (int l = 0; l <= L; ++l) {
            X[l] = (l == 0 && !grouped) ? nullptr : p;
            if (X[l]) p += (size_t)gc * S * dims[l];
        }
    }
    const int cus = sad::device_cus();
    const bool want_g0 = grouped ? (a->need & (NEED_FEAT | NEED_XYZ | NEED_NEW_XYZ)) != 0 : (a->need & NEED_FEAT) != 0;
    for (long long g0 = 0; g0 < ng; g0 += gc) {
        Chunk ch = base;
        ch.g0 = (int)g0;
        ch.g1 = (int)std::min(ng, g0 + gc);
        ch.cap = (ch.g1 - ch.g0) * S;
        ch.nhost = ch.cap;
        const int cap = ch.cap;
        const float *x0 = grouped ? X[0] : a->feat + (size_t)g0 * a->ld_feat;
        const long long ldx0 = grouped ? C0 : a->ld_feat;
        GatherJob gj{};
        if (grouped) {
            gj.xyz = a->xyz; gj.new_xyz = a->new_xyz; gj.feat = a->feat; gj.idx = a->idx; gj.cnt = a->cnt;
            gj.ld_feat = a->ld_feat; gj.N = a->N; gj.M = a->M; gj.C = a->C; gj.skip_empty = a->skip_empty;
            gj.ngroups = ng; gj.npoints = (long long)a->B * a->N; gj.ch = ch; gj.x0 = X[0];
            hipLaunchKernelGGL(mg_gather_kernel, dim3(blocks_for((unsigned long long)cap * C0, 256)), dim3(256), 0, st, gj);
        }
        // ---- recompute X_1 .. X_L: C[i = channel][j = row] = b[i] + sum_k W[i][k] X[j][k] ----
        for (int l = 1; l <= L; ++l) {
            Gemm p{};
            p.A = a->W[l - 1]; p.sai = dims[l - 1]; p.sak = 1;
            p.B = l == 1 ? x0 : X[l - 1]; p.sbk = 1; p.sbj = l == 1 ? ldx0 : dims[l - 1];
            p.I = dims[l]; p.J = cap; p.K = dims[l - 1]; p.ch = ch;
            p.bias = a->b[l - 1]; p.relu = (a->relu_mask >> (l - 1)) & 1;
            p.C = X[l]; p.sci = 1; p.scj = dims[l];
            launch_gemm<MG_FWD>(p, cap, 1, st);
        }
        // ---- D_L over X_L ----
        if (grouped) {
            RouteJob rj{};
            rj.ch = ch; rj.xl = X[L]; rj.CL = CL;
            rj.pooled = a->pooled + a->pooled_off; rj.ldp = a->ld_pooled;
            rj.gout = a->grad_out + a->col_off; rj.ldg = a->ld_grad;
            rj.cnt = a->cnt; rj.skip_empty = a->skip_empty; rj.mismatch = mismatch;
            hipLaunchKernelGGL(mg_route_kernel, dim3(blocks_for(ch.g1 - ch.g0, 4)), dim3(256), 0, st, rj);
        } else {
            hipLaunchKernelGGL(mg_rows_dl_kernel, dim3(blocks_for((unsigned long long)cap * CL, 256)), dim3(256), 0, st, X[L], CL, cap,
                               a->grad_out + (size_t)g0 * a->ld_grad + a->col_off, (long long)a->ld_grad, (a->relu_mask >> (L - 1)) & 1);
        }
        for (int l = L; l >= 1; --l) {
            const int Co = dims[l], Ci = dims[l - 1];
            const float *xin = l == 1 ? x0 : X[l - 1];
            const long long ldin = l == 1 ? ldx0 : Ci;
            if (a->need & NEED_PARAMS) {
                // grad_W[i = o][j = k] += sum_rows D[row][o] X[row][k]
                Gemm p{};
                p.A = X[l]; p.sai = 1; p.sak = Co;
                p.B = xin; p.sbk = ldin; p.sbj = 1;
                p.I = Co; p.J = Ci; p.K = cap; p.ch = ch;
                p.C = a->grad_W[l - 1]; p.sci = Ci; p.scj = 1;
                const long long tiles = (long long)blocks_for(Ci, MG_TJ) * blocks_for(Co, MG_TI);
                // two workgroups per compute unit over all blocks, 64 rows each at least if every slot of the chunk were a row
                const long long nz = std::max<long long>(1, std::min<long long>(2LL * cus / tiles, (cap + 63) / 64));
                launch_gemm<MG_WGRAD>(p, Ci, (int)nz, st);
                hipLaunchKernelGGL(mg_colsum_kernel, dim3(blocks_for(cap, 512), blocks_for(Co, 64)), dim3(256), 0, st, ch, (const float *)X[l], Co, a->grad_b[l - 1]);
            }
            if (l == 1 && !want_g0) break;
            // G[i = k][j = row] = sum_o W[o][k] D[row][o], selected by X_{l-1} > 0, over X_{l-1} (layer 1: the columns asked for)
            int c_lo = 0, c_hi = Ci;
            if (l == 1 && grouped) {
                if (!(a->need & (NEED_XYZ | NEED_NEW_XYZ))) c_lo = 3;
                if (!(a->need & NEED_FEAT)) c_hi = 3;
            }
            Gemm p{};
            p.A = a->W[l - 1] + c_lo; p.sai = 1; p.sak = Ci;
            p.B = X[l]; p.sbk = 1; p.sbj = Co;
            p.I = c_hi - c_lo; p.J = cap; p.K = Co; p.ch = ch;
            if (l > 1 && ((a->relu_mask >> (l - 2)) & 1)) { p.sel = X[l - 1]; p.ldsel = Ci; }
            if (l == 1 && !grouped) { p.C = a->grad_feat + (size_t)g0 * C0; p.scj = C0; }
            else { p.C = X[l - 1] + c_lo; p.scj = Ci; }
            p.sci = 1;
            launch_gemm<MG_DGRAD>(p, cap, 1, st);
            if (l == 1 && grouped) {
                if (a->need & (NEED_FEAT | NEED_XYZ)) {
                    const int s_lo = (a->need & NEED_XYZ) ? 0 : 3, s_hi = (a->need & NEED_FEAT) ? C0 : 3;
                    hipLaunchKernelGGL(mg_scatter_kernel, dim3(blocks_for((unsigned long long)cap * (s_hi - s_lo), 256)), dim3(256), 0, st, gj, s_lo, s_hi,
                                       (a->need & NEED_XYZ) ? a->grad_xyz : nullptr, (a->need & NEED_FEAT) ? a->grad_feat : nullptr);
                }
                if (a->need & NEED_NEW_XYZ)
                    hipLaunchKernelGGL(mg_new_xyz_kernel, dim3(blocks_for((unsigned long long)(ch.g1 - ch.g0) * 3, 256)), dim3(256), 0, st, ch, (const float *)X[0], C0, a->grad_new_xyz);
            }
        }
    }
    return sad::check_launch(fn);
}
