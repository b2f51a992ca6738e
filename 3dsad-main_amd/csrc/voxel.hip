// Voxelization (SPEC.md §20): voxel_coords, the dynamic voxel index, hard voxelization and the ordered reduction over voxels.
// Ragged input throughout: points[total, C] + offsets[B+1] (device).  Every result is a function of the input alone: atomics
// are used only where their order cannot show (first row of a key = atomicMin, member counts = atomicAdd, placement inside
// an UNORDERED member list that is ranked afterwards).
//
// voxel numbering (§20.2): the first-appearance numbering of vox_hash.h over the rows, ALL scenes as one list.
//   insert   one lane per point: key = (gz*Gy + gy)*Gx + gx goes into the coordinate table as (scene << 32 | key) with the row.
//   number   the voxel number of an opener is (openers before it) - (openers before its scene); numbers >= V are dropped — the
//            walk-continues rule of §20.2 needs nothing more.  Openers write their number, the voxel's (z,y,x) and p2v; follow:
//            the other points copy their opener's number and every taken point counts into count[b,v].
// member order (§20.3 / §20.4 / §20.5): CSR over the voxels (segment starts = a scan of the counts), members placed with a
// per-voxel cursor in arrival order, then RANKED: the rank of row i in its voxel is the number of members below i, so
// sorted[start + rank] = i puts every list in ascending row order whatever the arrival order was (lists are a handful of
// entries on LiDAR scenes; a list of length N costs N^2 compares of one broadcast load each and still comes out right).
// voxelize writes voxels[B,V,T,C] exactly once, rows and zeros in the same pass.  voxel_reduce walks sorted lists, one
// thread per (voxel, channel), one rounding per addition.  The backward is a gather.
#include "common.h"
#include "voxel_csr.h"
#include <algorithm>
#include <limits.h>
#include <math.h>

namespace {

#include "vox_hash.h"

struct VoxGrid {
    float lo[3], v[3], Gf[3];
    int G[3];
};

// §20.1: one subtraction, one correctly rounded division, one floor per axis; validity compared as floats
__device__ __forceinline__ bool voxel_of(const float *__restrict__ p, const VoxGrid &g, int &gx, int &gy, int &gz) {
    const float dx = p[0] - g.lo[0], dy = p[1] - g.lo[1], dz = p[2] - g.lo[2];
    const float qx = dx / g.v[0], qy = dy / g.v[1], qz = dz / g.v[2];
    const float fx = floorf(qx), fy = floorf(qy), fz = floorf(qz);
    const bool ok = fx >= 0.0f && fx < g.Gf[0] && fy >= 0.0f && fy < g.Gf[1] && fz >= 0.0f && fz < g.Gf[2];
    gx = ok ? (int)fx : -1;
    gy = ok ? (int)fy : -1;
    gz = ok ? (int)fz : -1;
    return ok;
}

// ---- voxel_coords ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VX_THREADS) void voxel_coords_kernel(const float *__restrict__ points, const int32_t *__restrict__ offsets,
                                                                  int total, int B, int C, VoxGrid g, int32_t *__restrict__ coors) {
    const int i = blockIdx.x * VX_THREADS + threadIdx.x;
    if (i >= total) return;
    int gx, gy, gz;
    voxel_of(points + (size_t)i * C, g, gx, gy, gz);
    int4 *o = (int4 *)coors + i;
    *o = make_int4(scene_of(offsets, B, i), gz, gy, gx);
}

// ---- numbering ------------------------------------------------------------------------------------------------
// grid-stride fill of whatever is passed: the coordinate table (empty), per-voxel ints cnt / fill (0), coors (-1)
__global__ __launch_bounds__(VX_THREADS) void voxel_init_kernel(CoordTable t, int32_t *__restrict__ cnt, int32_t *__restrict__ fill,
                                                                int32_t *__restrict__ coors, unsigned nvox) {
    const unsigned stride = gridDim.x * VX_THREADS;
    const unsigned t0 = blockIdx.x * VX_THREADS + threadIdx.x;
    if (t.keys) t.clear();
    for (unsigned s = t0; s < nvox; s += stride) {
        if (cnt) cnt[s] = 0;
        if (fill) fill[s] = 0;
    }
    if (coors) {
        for (unsigned s = t0; s < nvox; s += stride) {
            coors[(size_t)s * 3 + 0] = -1;
            coors[(size_t)s * 3 + 1] = -1;
            coors[(size_t)s * 3 + 2] = -1;
        }
    }
}

__global__ __launch_bounds__(VX_THREADS) void voxel_insert_kernel(const float *__restrict__ points, const int32_t *__restrict__ offsets,
                                                                  int total, int B, int C, VoxGrid g, CoordTable t, int32_t *__restrict__ pslot) {
    const int i = blockIdx.x * VX_THREADS + threadIdx.x;
    if (i >= total) return;
    int gx, gy, gz;
    if (!voxel_of(points + (size_t)i * C, g, gx, gy, gz)) {
        pslot[i] = -1;
        return;
    }
    const int key = (gz * g.G[1] + gy) * g.G[0] + gx;
    const u64 k64 = ((u64)(unsigned)scene_of(offsets, B, i) << 32) | (unsigned)key;
    pslot[i] = t.insert_min(k64, i);
}

// the opener of vox_hash.h's numbering: a point is an opener iff it is the lowest row of its key
struct VoxOpener {
    using index = int;
    const int32_t *pslot;     // [n]: the table slot of every point's key, -1 outside the grid
    CoordTable t;
    int n;                    // total points
    __device__ __forceinline__ int slot_of(int i) const { return i < n ? pslot[i] : -1; }
    __device__ __forceinline__ bool opens(int slot, int i) const { return slot >= 0 && t.lowest(slot) == i; }   // slot = slot_of(i)
    __device__ __forceinline__ bool operator()(int i) const { return opens(slot_of(i), i); }
    __device__ __forceinline__ int first_of(int row) const { return min(max(row, 0), n); }
};

// P[b] = openers in rows below offsets[b] (b = 0 .. B); voxel_num[b] = min(V, openers of b)
__global__ __launch_bounds__(VX_SCAN_THREADS) void voxel_scan_kernel(const VoxOpener op, const int32_t *__restrict__ offsets, int B, int32_t *wavecnt,
                                                                     int nw, int V, int32_t *P, int32_t *__restrict__ voxel_num) {
    __shared__ int s_w[VX_SCAN_THREADS / 64 + 1];
    opener_scan(op, offsets, B, wavecnt, nw, P, s_w);
    __syncthreads();
    for (int b = threadIdx.x; b < B; b += VX_SCAN_THREADS) voxel_num[b] = min(max(P[b + 1] - P[b], 0), V);
}

// openers: voxel number, p2v and the voxel's (z,y,x); invalid points: p2v = -1
__global__ __launch_bounds__(VX_THREADS) void voxel_number_kernel(const VoxOpener op, const int32_t *__restrict__ offsets,
                                                                  const int32_t *__restrict__ wavepre, const int32_t *__restrict__ P, int B, int V,
                                                                  int Gx, int Gy, int32_t *__restrict__ p2v, int32_t *__restrict__ coors) {
    const int i = blockIdx.x * VX_THREADS + threadIdx.x;
    const int slot = op.slot_of(i);                        // (read once: it also tells the rows outside the grid)
    const bool open = op.opens(slot, i);
    const int below = openers_below(open);
    if (i >= op.n) return;
    if (slot < 0) { p2v[i] = -1; return; }
    if (!open) return;
    const int b = scene_of(offsets, B, i);
    const int vn = wavepre[i >> 6] + below - P[b];
    if (vn < 0 || vn >= V) { p2v[i] = -1; return; }       // the voxel cap: this key is dropped, with every later point of it
    p2v[i] = vn;
    const int key = (int)(unsigned)(op.t.keys[slot] & 0xFFFFFFFFull);
    const int gx = key % Gx, q = key / Gx;
    int32_t *c = coors + ((size_t)b * V + vn) * 3;
    c[0] = q / Gy;
    c[1] = q % Gy;
    c[2] = gx;
}

// the other valid points take their opener's number; every taken point counts
__global__ __launch_bounds__(VX_THREADS) void voxel_follow_kernel(const VoxOpener op, const int32_t *__restrict__ offsets, int B, int V, int32_t *p2v,
                                                                  int32_t *count) {
    const int i = blockIdx.x * VX_THREADS + threadIdx.x, total = op.n;
    if (i >= total) return;
    const int slot = op.pslot[i];
    if (slot < 0) return;
    const int first = op.t.lowest(slot);
    int v;
    if (first == i) v = p2v[i];
    else {
        v = (first >= 0 && first < total) ? p2v[first] : -1;   // (an opener: written by the previous launch, not by this one)
        p2v[i] = v;
    }
    if (v >= 0 && v < V) atomicAdd(&count[(size_t)scene_of(offsets, B, i) * V + v], 1);
}

// ---- CSR of the members, in ascending row order ------------------------------------------------------------------
// count[b,v] from a caller's p2v (voxel_reduce): numbers outside [0, V) count as -1
__global__ __launch_bounds__(VX_THREADS) void voxel_count_kernel(const int32_t *__restrict__ p2v, const int32_t *__restrict__ offsets, int total,
                                                                 int B, int V, int32_t *count) {
    const int i = blockIdx.x * VX_THREADS + threadIdx.x;
    if (i >= total) return;
    const int v = p2v[i];
    if (v >= 0 && v < V) atomicAdd(&count[(size_t)scene_of(offsets, B, i) * V + v], 1);
}

// blocksum[k] = members of voxels 1024 k .. 1024 k + 1023 (all scenes' voxels as one list of nvox)
__global__ __launch_bounds__(VX_SCAN_THREADS) void voxel_blocksum_kernel(const int32_t *__restrict__ cnt, unsigned nvox, int32_t *__restrict__ blocksum) {
    __shared__ int s_w[VX_SCAN_THREADS / 64 + 1];
    const unsigned s = blockIdx.x * VX_SCAN_THREADS + threadIdx.x;
    int tot;
    block_excl_scan(s < nvox ? cnt[s] : 0, s_w, tot);
    if (threadIdx.x == 0) blocksum[blockIdx.x] = tot;
}

// start[s] = members of the voxels below s; num_points (optional) = min(count, T)
__global__ __launch_bounds__(VX_SCAN_THREADS) void voxel_start_kernel(const int32_t *__restrict__ cnt, unsigned nvox, const int32_t *__restrict__ blocksum,
                                                                      int32_t *__restrict__ start, int T, int32_t *__restrict__ num_points) {
    __shared__ int s_w[VX_SCAN_THREADS / 64 + 1];
    int before = 0, tot;
    for (unsigned k = threadIdx.x; k < blockIdx.x; k += VX_SCAN_THREADS) before += blocksum[k];
    block_excl_scan(before, s_w, tot);
    const int base = tot;
    const unsigned s = blockIdx.x * VX_SCAN_THREADS + threadIdx.x;
    const int c = s < nvox ? cnt[s] : 0;
    const int ex = block_excl_scan(c, s_w, tot);
    if (s < nvox) {
        start[s] = base + ex;
        if (num_points) num_points[s] = min(c, T);
    }
}

// members[start + arrival order] = row (arrival order is arbitrary: the ranking below removes it)
__global__ __launch_bounds__(VX_THREADS) void voxel_fill_kernel(const int32_t *__restrict__ p2v, const int32_t *__restrict__ offsets, int total, int B,
                                                                int V, const int32_t *__restrict__ start, const int32_t *__restrict__ cnt,
                                                                int32_t *fill, int32_t *__restrict__ members) {
    const int i = blockIdx.x * VX_THREADS + threadIdx.x;
    if (i >= total) return;
    const int v = p2v[i];
    if (v < 0 || v >= V) return;
    const size_t s = (size_t)scene_of(offsets, B, i) * V + v;
    const int k = atomicAdd(&fill[s], 1);
    const long long pos = (long long)start[s] + k;
    if (k < cnt[s] && pos < total) members[pos] = i;
}

// sorted[start + (members of the voxel below row i)] = i
__global__ __launch_bounds__(VX_THREADS) void voxel_rank_kernel(const int32_t *__restrict__ p2v, const int32_t *__restrict__ offsets, int total, int B,
                                                                int V, const int32_t *__restrict__ start, const int32_t *__restrict__ cnt,
                                                                const int32_t *__restrict__ members, int32_t *__restrict__ sorted) {
    const int i = blockIdx.x * VX_THREADS + threadIdx.x;
    if (i >= total) return;
    const int v = p2v[i];
    if (v < 0 || v >= V) return;
    const size_t s = (size_t)scene_of(offsets, B, i) * V + v;
    const int st = start[s];
    const int c = min(cnt[s], total - st);
    int r = 0;
    for (int k = 0; k < c; ++k) r += members[st + k] < i;
    sorted[st + r] = i;
}

// ---- hard voxelization: every float of voxels[B,V,T,C] is written once ------------------------------------------
// one thread per 4 consecutive floats of the output (nq chunks; the tail chunk may be short)
template <bool VEC>
__global__ __launch_bounds__(VX_THREADS) void voxelize_write_kernel(const float *__restrict__ points, const int32_t *__restrict__ start,
                                                                    const int32_t *__restrict__ cnt, const int32_t *__restrict__ sorted, int C,
                                                                    int T, unsigned TC, unsigned long long nfloats, float *__restrict__ voxels) {
    const unsigned long long q = (unsigned long long)blockIdx.x * VX_THREADS + threadIdx.x;
    const unsigned long long e0 = q * 4;
    if (e0 >= nfloats) return;
    unsigned s;                                         // voxel (b * V + v)
    if (nfloats <= 0xFFFFFFFFull) s = (unsigned)e0 / TC;     // (uniform: 32-bit division whenever the output is below 16 GiB)
    else s = (unsigned)(e0 / TC);
    unsigned r = (unsigned)(e0 - (unsigned long long)s * TC);
    unsigned t = r / (unsigned)C, c = r - t * (unsigned)C;
    int n = min(cnt[s], T), st = start[s];
    int row = (int)t < n ? sorted[st + t] : -1;
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        v[u] = row >= 0 ? points[(size_t)row * C + c] : 0.0f;
        if (++c == (unsigned)C) {
            c = 0;
            if (++t == (unsigned)T) {
                t = 0;
                ++s;
                if ((unsigned long long)s * TC >= nfloats) { n = 0; st = 0; }
                else { n = min(cnt[s], T); st = start[s]; }
            }
            row = (int)t < n ? sorted[st + t] : -1;
        }
    }
    if (VEC) {
        *(float4 *)(voxels + e0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (e0 + u < nfloats) voxels[e0 + u] = v[u];
    }
}

// ---- reduction over voxels -----------------------------------------------------------------------------------
// one thread per (voxel, channel): the members in ascending row order, one rounding per addition
__global__ __launch_bounds__(VX_THREADS) void voxel_reduce_kernel(const float *__restrict__ feat, const int32_t *__restrict__ start,
                                                                  const int32_t *__restrict__ cnt, const int32_t *__restrict__ sorted, int Cf,
                                                                  unsigned long long nout, int total, int mode, float *__restrict__ out,
                                                                  int32_t *__restrict__ arg, int32_t *__restrict__ count) {
    const unsigned long long e = (unsigned long long)blockIdx.x * VX_THREADS + threadIdx.x;
    if (e >= nout) return;
    const unsigned s = (unsigned)(e / (unsigned)Cf);
    const int c = (int)(e - (unsigned long long)s * (unsigned)Cf);
    const int st = start[s];
    const int n = min(cnt[s], total - st);
    if (count && c == 0) count[s] = n;
    if (n <= 0) {
        out[e] = 0.0f;
        if (arg) arg[e] = -1;
        return;
    }
    const int32_t *m = sorted + st;
    int best = m[0];
    float acc = feat[(size_t)best * Cf + c];
    if (mode == SAD_VOXEL_MAX) {
#pragma unroll 4
        for (int k = 1; k < n; ++k) {
            const int j = m[k];
            const float x = feat[(size_t)j * Cf + c];
            if (x > acc) { acc = x; best = j; }
        }
        arg[e] = best;
    } else {
#pragma unroll 4
        for (int k = 1; k < n; ++k) acc = acc + feat[(size_t)m[k] * Cf + c];
        if (mode == SAD_VOXEL_MEAN) acc = acc / (float)n;
    }
    out[e] = acc;
}

// backward: a gather.  aux = count[B,V] (mean) or arg[B,V,Cf] (max)
__global__ __launch_bounds__(VX_THREADS) void voxel_reduce_grad_kernel(const float *__restrict__ grad_out, const int32_t *__restrict__ p2v,
                                                                       const int32_t *__restrict__ offsets, const int32_t *__restrict__ aux,
                                                                       int total, int B, int Cf, int V, int mode, float *__restrict__ grad_feat) {
    const unsigned long long e = (unsigned long long)blockIdx.x * VX_THREADS + threadIdx.x;
    if (e >= (unsigned long long)total * Cf) return;
    const int i = (int)(e / (unsigned)Cf), c = (int)(e - (unsigned long long)i * (unsigned)Cf);
    const int v = p2v[i];
    float g = 0.0f;
    if (v >= 0 && v < V) {
        const size_t s = (size_t)scene_of(offsets, B, i) * V + v;
        const float go = grad_out[s * Cf + c];
        if (mode == SAD_VOXEL_SUM) g = go;
        else if (mode == SAD_VOXEL_MEAN) g = go / (float)aux[s];
        else g = aux[s * Cf + c] == i ? go : 0.0f;
    }
    grad_feat[e] = g;
}

// ---- host side ------------------------------------------------------------------------------------------------
using sad::blocks_for;

// workspace layout: the coordinate table of `total` keys in workspace `ws` (NULL: a size query), the rest in bytes from the base
struct VoxWs {
    CoordTable t;
    size_t pslot, wavecnt, P, blocksum, start, fill, cnt, p2v, members, sorted, bytes;
};

VoxWs vox_ws(void *ws, int total, int B, int V) {
    VoxWs w;
    const size_t nvox = (size_t)B * V, nw = ((size_t)total + 63) / 64;
    sad::Carve c;
    w.t = CoordTable(ws, c, (unsigned long long)total);
    w.pslot = c.take((size_t)total * 4);
    w.wavecnt = c.take((nw + 1) * 4);
    w.P = c.take(((size_t)B + 1) * 4);
    w.blocksum = c.take((nvox / VX_SCAN_THREADS + 1) * 4);
    w.start = c.take(nvox * 4);
    w.fill = c.take(nvox * 4);
    w.cnt = c.take(nvox * 4);
    w.p2v = c.take((size_t)total * 4);
    w.members = c.take((size_t)total * 4);
    w.sorted = c.take((size_t)total * 4);
    w.bytes = c.o + 16;
    return w;
}

constexpr int VX_MAX_TOTAL = 1 << 30;

int vox_sizes_ok(const char *fn, long long total, int B, long long V) {
    SAD_REQUIRE(B >= 1 && B <= 65535, "%s: B must be in 1 .. 65535 (got %d)", fn, B);
    SAD_REQUIRE(total >= 0 && total <= VX_MAX_TOTAL, "%s: total_points must be in 0 .. 2^30 (got %lld)", fn, total);
    SAD_REQUIRE(V >= 1 && (long long)B * V < (1LL << 31), "%s: max_voxels must be >= 1 and B * max_voxels < 2^31 (got %lld)", fn, V);
    return SAD_OK;
}

// §20.1 grid: G_d = (int)rintf((hi_d - lo_d) / v_d), every G_d >= 1, Gx * Gy * Gz <= 2^31 - 1
int vox_grid(const char *fn, const float *voxel_size, const float *point_range, VoxGrid &g) {
    SAD_REQUIRE(voxel_size && point_range, "%s: NULL voxel_size / point_range", fn);
    long long cells = 1;
    for (int d = 0; d < 3; ++d) {
        const float v = voxel_size[d], lo = point_range[d], hi = point_range[3 + d];
        SAD_REQUIRE(v > 0.0f && isfinite(v) && isfinite(lo) && isfinite(hi), "%s: voxel_size must be > 0 and the range finite (axis %d)", fn, d);
        volatile float ext = hi - lo;
        volatile float q = ext / v;
        const float r = rintf(q);
        if (!(r >= 1.0f)) return sad::fail(SAD_EUNSUPPORTED, "%s: grid dimension %d is %g (< 1)", fn, d, (double)r);
        if (!(r < 2147483648.0f)) return sad::fail(SAD_EUNSUPPORTED, "%s: grid dimension %d is %g (> 2^31 - 1 cells)", fn, d, (double)r);
        g.lo[d] = lo;
        g.v[d] = v;
        g.G[d] = (int)r;
        g.Gf[d] = (float)g.G[d];
        cells *= g.G[d];
        if (cells > 2147483647LL)
            return sad::fail(SAD_EUNSUPPORTED, "%s: grid %d x %d x %d exceeds 2^31 - 1 cells", fn, g.G[0], d > 0 ? g.G[1] : 1, d > 1 ? g.G[2] : 1);
    }
    return SAD_OK;
}

// t (keys == NULL: no table) is cleared, cnt / fill / coors (each optional) are filled
inline void launch_init(const CoordTable &t, int32_t *cnt, int32_t *fill, int32_t *coors, unsigned nvox, hipStream_t st) {
    const unsigned long long n = std::max<unsigned long long>(t.keys ? t.mask + 1ull : 0ull, nvox);
    const unsigned blocks = (unsigned)std::min<unsigned long long>(blocks_for(n, VX_THREADS), 16384ull);
    hipLaunchKernelGGL(voxel_init_kernel, dim3(blocks ? blocks : 1), dim3(VX_THREADS), 0, st, t, cnt, fill, coors, nvox);
}

// §20.2: p2v[total], coors[B,V,3], count[B,V], voxel_num[B].  `fill` (optional): zeroed for a CSR that follows
void launch_numbering(const float *points, const int32_t *offsets, int total, int B, int C, const VoxGrid &g, int V, char *ws, const VoxWs &w,
                      int32_t *p2v, int32_t *coors, int32_t *count, int32_t *voxel_num, int32_t *fill, hipStream_t st) {
    int32_t *pslot = (int32_t *)(ws + w.pslot), *wavecnt = (int32_t *)(ws + w.wavecnt), *P = (int32_t *)(ws + w.P);
    const VoxOpener op = {pslot, w.t, total};
    const unsigned nvox = (unsigned)B * (unsigned)V;
    const int nw = (total + 63) / 64;
    const dim3 gp(blocks_for((unsigned long long)total, VX_THREADS)), tb(VX_THREADS);
    launch_init(w.t, count, fill, coors, nvox, st);
    if (total > 0) {
        hipLaunchKernelGGL(voxel_insert_kernel, gp, tb, 0, st, points, offsets, total, B, C, g, w.t, pslot);
        hipLaunchKernelGGL(opener_flags_kernel<VoxOpener>, gp, tb, 0, st, op, wavecnt);
    }
    hipLaunchKernelGGL(voxel_scan_kernel, dim3(1), dim3(VX_SCAN_THREADS), 0, st, op, offsets, B, wavecnt, nw, V, P, voxel_num);
    if (total > 0) {
        hipLaunchKernelGGL(voxel_number_kernel, gp, tb, 0, st, op, offsets, wavecnt, P, B, V, g.G[0], g.G[1], p2v, coors);
        hipLaunchKernelGGL(voxel_follow_kernel, gp, tb, 0, st, op, offsets, B, V, p2v, count);
    }
}

// count[B,V] (final) + p2v -> start, sorted (fill zeroed on entry).  num_points (optional) = min(count, T)
void launch_csr(const int32_t *p2v, const int32_t *offsets, int total, int B, int V, const int32_t *cnt, char *ws, const VoxWs &w, int T,
                int32_t *num_points, hipStream_t st) {
    int32_t *blocksum = (int32_t *)(ws + w.blocksum), *start = (int32_t *)(ws + w.start), *fill = (int32_t *)(ws + w.fill);
    int32_t *members = (int32_t *)(ws + w.members), *sorted = (int32_t *)(ws + w.sorted);
    const unsigned nvox = (unsigned)B * (unsigned)V;
    const dim3 gv(blocks_for(nvox, VX_SCAN_THREADS)), gp(blocks_for((unsigned long long)total, VX_THREADS));
    hipLaunchKernelGGL(voxel_blocksum_kernel, gv, dim3(VX_SCAN_THREADS), 0, st, cnt, nvox, blocksum);
    hipLaunchKernelGGL(voxel_start_kernel, gv, dim3(VX_SCAN_THREADS), 0, st, cnt, nvox, blocksum, start, T, num_points);
    if (total > 0) {
        hipLaunchKernelGGL(voxel_fill_kernel, gp, dim3(VX_THREADS), 0, st, p2v, offsets, total, B, V, start, cnt, fill, members);
        hipLaunchKernelGGL(voxel_rank_kernel, gp, dim3(VX_THREADS), 0, st, p2v, offsets, total, B, V, start, cnt, members, sorted);
    }
}

}  // namespace

namespace sad {

size_t voxel_ws_bytes(int total, int B, int V) { return vox_ws(nullptr, total, B, V).bytes; }

int voxel_sizes_ok(const char *fn, long long total, int B, long long V) { return vox_sizes_ok(fn, total, B, V); }

void voxel_member_lists(const int32_t *p2v, const int32_t *offsets, int total, int B, int V, void *workspace, hipStream_t st,
                        VoxLists &out) {
    const VoxWs w = vox_ws(workspace, total, B, V);
    char *ws = (char *)workspace;
    int32_t *cnt = (int32_t *)(ws + w.cnt);
    launch_init(CoordTable{}, cnt, (int32_t *)(ws + w.fill), nullptr, (unsigned)B * (unsigned)V, st);
    if (total > 0)
        hipLaunchKernelGGL(voxel_count_kernel, dim3(blocks_for((unsigned long long)total, VX_THREADS)), dim3(VX_THREADS), 0, st, p2v, offsets,
                           total, B, V, cnt);
    launch_csr(p2v, offsets, total, B, V, cnt, ws, w, 0, nullptr, st);
    out.start = (const int32_t *)(ws + w.start);
    out.cnt = cnt;
    out.sorted = (const int32_t *)(ws + w.sorted);
}

}  // namespace sad

SAD_API int sad_voxel_workspace_bytes(int total_points, int B, int max_voxels, size_t *out) {
    SAD_REQUIRE(out, "sad_voxel_workspace_bytes: NULL out");
    *out = 0;
    if (int rc = vox_sizes_ok("sad_voxel_workspace_bytes", total_points, B, max_voxels)) return rc;
    *out = vox_ws(nullptr, total_points, B, max_voxels).bytes;
    return SAD_OK;
}

SAD_API int sad_voxel_coords_f32(const float *points, const int32_t *offsets, int total_points, int B, int C, const float *voxel_size,
                                 const float *point_range, int32_t *coors, sad_stream_t stream) {
    SAD_REQUIRE(offsets && (total_points == 0 || (points && coors)), "sad_voxel_coords_f32: NULL pointer");
    SAD_REQUIRE(C >= 3, "sad_voxel_coords_f32: point rows need C >= 3 floats (got %d)", C);
    if (int rc = vox_sizes_ok("sad_voxel_coords_f32", total_points, B, 1)) return rc;
    SAD_REQUIRE(((uintptr_t)coors & 15) == 0, "sad_voxel_coords_f32: coors must be 16-byte aligned");
    VoxGrid g;
    if (int rc = vox_grid("sad_voxel_coords_f32", voxel_size, point_range, g)) return rc;
    if (total_points == 0) return SAD_OK;
    hipLaunchKernelGGL(voxel_coords_kernel, dim3(blocks_for((unsigned long long)total_points, VX_THREADS)), dim3(VX_THREADS), 0, (hipStream_t)stream,
                       points, offsets, total_points, B, C, g, coors);
    return sad::check_launch("sad_voxel_coords_f32");
}

SAD_API int sad_voxel_index_f32(const float *points, const int32_t *offsets, int total_points, int B, int C, const float *voxel_size,
                                const float *point_range, int max_voxels, int32_t *point2voxel, int32_t *coors, int32_t *count,
                                int32_t *voxel_num, void *workspace, sad_stream_t stream) {
    SAD_REQUIRE(offsets && coors && count && voxel_num && workspace && (total_points == 0 || (points && point2voxel)),
                "sad_voxel_index_f32: NULL pointer");
    SAD_REQUIRE(C >= 3, "sad_voxel_index_f32: point rows need C >= 3 floats (got %d)", C);
    if (int rc = vox_sizes_ok("sad_voxel_index_f32", total_points, B, max_voxels)) return rc;
    SAD_REQUIRE(((uintptr_t)workspace & 15) == 0, "sad_voxel_index_f32: workspace must be 16-byte aligned");
    VoxGrid g;
    if (int rc = vox_grid("sad_voxel_index_f32", voxel_size, point_range, g)) return rc;
    const VoxWs w = vox_ws(workspace, total_points, B, max_voxels);
    launch_numbering(points, offsets, total_points, B, C, g, max_voxels, (char *)workspace, w, point2voxel, coors, count, voxel_num, nullptr,
                     (hipStream_t)stream);
    return sad::check_launch("sad_voxel_index_f32");
}

SAD_API int sad_voxelize_f32(const float *points, const int32_t *offsets, int total_points, int B, int C, const float *voxel_size,
                             const float *point_range, int max_points, int max_voxels, float *voxels, int32_t *coors, int32_t *num_points,
                             int32_t *voxel_num, void *workspace, sad_stream_t stream) {
    SAD_REQUIRE(offsets && voxels && coors && num_points && voxel_num && workspace && (total_points == 0 || points), "sad_voxelize_f32: NULL pointer");
    SAD_REQUIRE(C >= 3, "sad_voxelize_f32: point rows need C >= 3 floats (got %d)", C);
    SAD_REQUIRE(max_points >= 1, "sad_voxelize_f32: max_points must be >= 1 (got %d)", max_points);
    if (int rc = vox_sizes_ok("sad_voxelize_f32", total_points, B, max_voxels)) return rc;
    SAD_REQUIRE(((uintptr_t)workspace & 15) == 0, "sad_voxelize_f32: workspace must be 16-byte aligned");
    const unsigned long long TC = (unsigned long long)max_points * C;
    const unsigned long long nfloats = (unsigned long long)B * max_voxels * TC;
    if (TC >= (1ull << 31) || nfloats >= (1ull << 40))
        return sad::fail(SAD_EUNSUPPORTED, "sad_voxelize_f32: voxels[B,V,T,C] of %llu floats is too large", nfloats);
    VoxGrid g;
    if (int rc = vox_grid("sad_voxelize_f32", voxel_size, point_range, g)) return rc;
    const VoxWs w = vox_ws(workspace, total_points, B, max_voxels);
    char *ws = (char *)workspace;
    const hipStream_t st = (hipStream_t)stream;
    int32_t *cnt = (int32_t *)(ws + w.cnt), *p2v = (int32_t *)(ws + w.p2v);
    launch_numbering(points, offsets, total_points, B, C, g, max_voxels, ws, w, p2v, coors, cnt, voxel_num, (int32_t *)(ws + w.fill), st);
    launch_csr(p2v, offsets, total_points, B, max_voxels, cnt, ws, w, max_points, num_points, st);
    const unsigned nb = blocks_for((nfloats + 3) / 4, VX_THREADS);
    const int32_t *start = (const int32_t *)(ws + w.start), *sorted = (const int32_t *)(ws + w.sorted);
    if (((uintptr_t)voxels & 15) == 0 && nfloats % 4 == 0)
        hipLaunchKernelGGL(voxelize_write_kernel<true>, dim3(nb), dim3(VX_THREADS), 0, st, points, start, cnt, sorted, C, max_points, (unsigned)TC,
                           nfloats, voxels);
    else
        hipLaunchKernelGGL(voxelize_write_kernel<false>, dim3(nb), dim3(VX_THREADS), 0, st, points, start, cnt, sorted, C, max_points, (unsigned)TC,
                           nfloats, voxels);
    return sad::check_launch("sad_voxelize_f32");
}

SAD_API int sad_voxel_reduce_f32(const float *feat, const int32_t *point2voxel, const int32_t *offsets, int total_points, int B, int Cf,
                                 int max_voxels, int mode, float *out, int32_t *arg, int32_t *count, void *workspace, sad_stream_t stream) {
    SAD_REQUIRE(offsets && out && workspace && (total_points == 0 || (feat && point2voxel)), "sad_voxel_reduce_f32: NULL pointer");
    SAD_REQUIRE(mode == SAD_VOXEL_SUM || mode == SAD_VOXEL_MEAN || mode == SAD_VOXEL_MAX, "sad_voxel_reduce_f32: mode must be 0 (sum), 1 (mean) or 2 (max), got %d",
                mode);
    SAD_REQUIRE(mode != SAD_VOXEL_MAX || arg, "sad_voxel_reduce_f32: mode max needs the arg output");
    SAD_REQUIRE(Cf >= 1, "sad_voxel_reduce_f32: Cf must be >= 1 (got %d)", Cf);
    if (int rc = vox_sizes_ok("sad_voxel_reduce_f32", total_points, B, max_voxels)) return rc;
    SAD_REQUIRE(((uintptr_t)workspace & 15) == 0, "sad_voxel_reduce_f32: workspace must be 16-byte aligned");
    const unsigned long long nout = (unsigned long long)B * max_voxels * Cf;
    if (nout >= (1ull << 40)) return sad::fail(SAD_EUNSUPPORTED, "sad_voxel_reduce_f32: out[B,V,Cf] of %llu floats is too large", nout);
    const hipStream_t st = (hipStream_t)stream;
    sad::VoxLists ml;
    sad::voxel_member_lists(point2voxel, offsets, total_points, B, max_voxels, workspace, st, ml);
    hipLaunchKernelGGL(voxel_reduce_kernel, dim3(blocks_for(nout, VX_THREADS)), dim3(VX_THREADS), 0, st, feat, ml.start, ml.cnt, ml.sorted, Cf, nout,
                       total_points, mode, out, mode == SAD_VOXEL_MAX ? arg : nullptr, count);
    return sad::check_launch("sad_voxel_reduce_f32");
}

SAD_API int sad_voxel_reduce_grad_f32(const float *grad_out, const int32_t *point2voxel, const int32_t *offsets, int total_points, int B, int Cf,
                                      int max_voxels, int mode, const int32_t *count_or_arg, float *grad_feat, sad_stream_t stream) {
    SAD_REQUIRE(offsets && grad_out && (total_points == 0 || (point2voxel && grad_feat)), "sad_voxel_reduce_grad_f32: NULL pointer");
    SAD_REQUIRE(mode == SAD_VOXEL_SUM || mode == SAD_VOXEL_MEAN || mode == SAD_VOXEL_MAX,
                "sad_voxel_reduce_grad_f32: mode must be 0 (sum), 1 (mean) or 2 (max), got %d", mode);
    SAD_REQUIRE(mode == SAD_VOXEL_SUM || count_or_arg, "sad_voxel_reduce_grad_f32: mean needs count[B,V], max needs arg[B,V,Cf]");
    SAD_REQUIRE(Cf >= 1, "sad_voxel_reduce_grad_f32: Cf must be >= 1 (got %d)", Cf);
    if (int rc = vox_sizes_ok("sad_voxel_reduce_grad_f32", total_points, B, max_voxels)) return rc;
    if (total_points == 0) return SAD_OK;
    const unsigned long long n = (unsigned long long)total_points * Cf;
    SAD_REQUIRE(n < (1ull << 40), "sad_voxel_reduce_grad_f32: total_points * Cf too large");
    hipLaunchKernelGGL(voxel_reduce_grad_kernel, dim3(blocks_for(n, VX_THREADS)), dim3(VX_THREADS), 0, (hipStream_t)stream, grad_out, point2voxel,
                       offsets, count_or_arg, total_points, B, Cf, max_voxels, mode, grad_feat);
    return sad::check_launch("sad_voxel_reduce_grad_f32");
}
