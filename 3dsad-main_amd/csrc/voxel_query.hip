// Voxel RoI pooling, the index side (SPEC.md §30): the G x G x G grid points of every RoI, and for every query point the non-empty
// voxels of one backbone scale within a Manhattan range and a radius, in walk order.  What a Voxel R-CNN / PV-RCNN RoI-grid head
// needs between nms_boxes (§23) and the grouped MLP + max (§6).  No gradients, no atomics on an output, nothing read back.
//
// roi_grid_points  one launch, one thread per grid point: §28.2's rotation of the point's offset in the RoI's frame.  A row beyond
//                  roi_count is never read; its points are quiet NaN, which voxel_query treats as an empty query.
// voxel_query      three launches.  The voxels go into the coordinate table of vox_hash.h under (scene << 32 | cell) with their
//                  global row (launch_coord_rows: clear, insert_min; the lowest row owns a duplicated coordinate), the table the
//                  rulebook of spconv.hip builds.  Then ONE WAVE PER QUERY POINT walks the (2rz+1)(2ry+1)(2rx+1) candidate cells, dz slowest
//                  and dx fastest, 64 consecutive candidates per step: a lane decodes its candidate by two integer divisions
//                  (arithmetic, not an LDS table: a table of up to 17^3 entries would have to be filled by every workgroup, for
//                  four queries of at most 77 steps, and would put a barrier and an LDS allocation into a kernel that otherwise has
//                  neither; the divisions sit in the shadow of the table probes), tests the cell against the grid, probes the
//                  table and compares d2(centre, query) < r2.  A ballot and the count of accepted lanes below give a lane its
//                  slot, so the walk order is kept without an atomic, and the wave leaves the walk as soon as S are accepted.
//                  The padding (the first accepted row, §3) is stored by all lanes; every slot of a row of idx is written once.
//                  A workgroup is four waves = four queries of one scene (blockIdx.y); the waves share nothing, so the workgroup
//                  is only the unit that is placed: 256 threads put one wave on each SIMD and eight workgroups fill a CU.
#include "box_geom.h"
#include <algorithm>
#include <limits.h>
#include <math.h>

namespace {

#include "vox_hash.h"

constexpr int VQ_WAVES = 4;                 // queries per workgroup
constexpr int VQ_MAX_RANGE = 8, VQ_MAX_S = 128, RGP_MAX_G = 16;

struct VqP {
    CoordTable t;
    const float *new_xyz;
    int32_t *idx, *cnt;
    int M, S;
    int G[3], r[3];                         // (z, y, x)
    float v[3], lo[3];                      // (x, y, z)
    float r2;
};

// §24 voxel centre of cell g on one axis
__device__ __forceinline__ float cell_centre(int g, float v, float lo) { return ((float)g * v) + ((0.5f * v) + lo); }

__global__ __launch_bounds__(VQ_WAVES * 64) void voxel_query_kernel(const VqP p) {
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * VQ_WAVES + (threadIdx.x >> 6);
    if (m >= p.M) return;                               // (the whole wave)
    const int b = blockIdx.y;
    const size_t q = (size_t)b * p.M + m;
    const float *pt = p.new_xyz + q * 3;
    const float px = pt[0], py = pt[1], pz = pt[2];
    // §20.1's cell of the query: one subtraction, one correctly rounded division, one floor per axis
    const float fx = floorf((px - p.lo[0]) / p.v[0]), fy = floorf((py - p.lo[1]) / p.v[1]), fz = floorf((pz - p.lo[2]) / p.v[2]);
    int32_t *row = p.idx + q * p.S;
    int acc = 0, first = 0;
    if (fabsf(fx) < 1073741824.0f && fabsf(fy) < 1073741824.0f && fabsf(fz) < 1073741824.0f) {    // (false for NaN and Inf: an empty query)
        const int qx = (int)fx, qy = (int)fy, qz = (int)fz;
        const int nx = 2 * p.r[2] + 1, nyx = (2 * p.r[1] + 1) * nx, T = (2 * p.r[0] + 1) * nyx;
        for (int base = 0; base < T && acc < p.S; base += 64) {
            const int c = base + lane;
            bool ok = false;
            int r = 0;
            if (c < T) {
                const int iz = c / nyx, rem = c - iz * nyx, iy = rem / nx, ix = rem - iy * nx;
                const int z = qz + (iz - p.r[0]), y = qy + (iy - p.r[1]), x = qx + (ix - p.r[2]);
                if ((unsigned)z < (unsigned)p.G[0] && (unsigned)y < (unsigned)p.G[1] && (unsigned)x < (unsigned)p.G[2]) {
                    const int slot = p.t.find(((u64)(unsigned)b << 32) | (unsigned)((z * p.G[1] + y) * p.G[2] + x));
                    if (slot >= 0) {
                        ok = sad::d2f(cell_centre(x, p.v[0], p.lo[0]), cell_centre(y, p.v[1], p.lo[1]), cell_centre(z, p.v[2], p.lo[2]), px, py, pz) < p.r2;
                        r = p.t.lowest(slot);
                    }
                }
            }
            const u64 mask = __ballot(ok);
            if (mask) {                                 // (wave-uniform)
                if (acc == 0) first = __shfl(r, __builtin_ctzll(mask));
                const int s = acc + __builtin_popcountll(mask & ((1ull << lane) - 1ull));
                if (ok && s < p.S) row[s] = r;
                acc += __builtin_popcountll(mask);
            }
        }
    }
    const int n = min(acc, p.S);
    for (int s = n + lane; s < p.S; s += 64) row[s] = first;      // §3's padding: the first accepted row, 0 for an empty query
    if (lane == 0) p.cnt[q] = n;
}

__global__ __launch_bounds__(256) void roi_grid_points_kernel(const float *__restrict__ rois, const int32_t *__restrict__ roi_count, int R, int D, int G,
                                                              long long total, float *__restrict__ pts) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int G3 = G * G * G;
    const long long br = t / G3;
    const int g = (int)(t - br * G3);
    const int b = (int)(br / R);
    float *o = pts + t * 3;
    const int nb = roi_count ? min(max(roi_count[b], 0), R) : R;
    if ((int)(br - (long long)b * R) >= nb) {           // a row beyond the scene's candidates is never read
        o[0] = o[1] = o[2] = __builtin_nanf("");
        return;
    }
    const float *roi = rois + br * D;
    const int ix = g / (G * G), iy = (g / G) % G, iz = g % G;
    const float Gf = (float)G;
    const float lx = ((((float)ix + 0.5f) / Gf) * roi[3]) - (0.5f * roi[3]);
    const float ly = ((((float)iy + 0.5f) / Gf) * roi[4]) - (0.5f * roi[4]);
    const float lz = ((((float)iz + 0.5f) / Gf) * roi[5]) - (0.5f * roi[5]);
    float s, c, x, y;
    sincos_r(roi[6], s, c);
    from_frame(lx, ly, c, s, x, y);
    o[0] = x + roi[0];
    o[1] = y + roi[1];
    o[2] = lz + roi[2];
}

}  // namespace

SAD_API size_t sad_voxel_query_workspace_bytes(int Nv) {
    if (Nv < 0 || Nv > (1 << 30)) return 0;
    sad::Carve c;
    const CoordTable t(nullptr, c, (unsigned long long)Nv);     // (a size query: the slices are taken, nothing is dereferenced)
    (void)t;
    return c.o;
}

SAD_API int sad_voxel_query_f32(const sad_voxel_query_args *a, sad_stream_t stream) {
    const char *fn = "sad_voxel_query_f32";
    if (int rc = args_ok(fn, a)) return rc;
    SAD_REQUIRE(a->B >= 1 && a->M >= 0 && a->Nv >= 0 && a->S >= 1, "%s: need B, S >= 1 and M, Nv >= 0 (got %d, %d, %d, %d)", fn, a->B, a->S, a->M, a->Nv);
    SAD_REQUIRE(a->offsets && (a->Nv == 0 || a->coors) && (a->M == 0 || (a->new_xyz && a->idx && a->cnt)), "%s: NULL pointer", fn);
    long long cells = 1;
    for (int d = 0; d < 3; ++d) {
        SAD_REQUIRE(a->max_range[d] >= 0, "%s: max_range[%d] = %d must be >= 0", fn, d, a->max_range[d]);
        SAD_REQUIRE(a->spatial_shape[d] >= 1, "%s: spatial_shape[%d] = %d must be >= 1", fn, d, a->spatial_shape[d]);
        SAD_REQUIRE(a->voxel_size[d] > 0.0f && isfinite(a->voxel_size[d]) && isfinite(a->lo[d]), "%s: voxel_size must be > 0 and the range finite (axis %d)",
                    fn, d);
    }
    SAD_REQUIRE(a->radius > 0.0f, "%s: radius must be > 0 (got %g)", fn, (double)a->radius);
    for (int d = 0; d < 3; ++d) {
        if (a->max_range[d] > VQ_MAX_RANGE) return sad::fail(SAD_EUNSUPPORTED, "%s: max_range[%d] = %d (at most %d)", fn, d, a->max_range[d], VQ_MAX_RANGE);
        cells *= a->spatial_shape[d];
        if (cells > 2147483647LL) return sad::fail(SAD_EUNSUPPORTED, "%s: spatial_shape exceeds 2^31 - 1 cells", fn);
    }
    if (a->S > VQ_MAX_S) return sad::fail(SAD_EUNSUPPORTED, "%s: S = %d (at most %d)", fn, a->S, VQ_MAX_S);
    if (a->B > 65535) return sad::fail(SAD_EUNSUPPORTED, "%s: B = %d (at most 65535)", fn, a->B);
    if ((long long)a->B * a->M * a->S >= (1LL << 31)) return sad::fail(SAD_EUNSUPPORTED, "%s: B * M * S = %d * %d * %d (must be below 2^31)", fn, a->B, a->M, a->S);
    if (a->Nv > (1 << 30)) return sad::fail(SAD_EUNSUPPORTED, "%s: Nv = %d (at most 2^30)", fn, a->Nv);
    SAD_REQUIRE(a->workspace, "%s: NULL workspace (sad_voxel_query_workspace_bytes(Nv) bytes)", fn);
    SAD_REQUIRE(((uintptr_t)a->workspace & 15) == 0, "%s: the workspace must be 16-byte aligned", fn);
    if (a->M == 0) return SAD_OK;
    VqP p = {};
    sad::Carve c;
    p.t = CoordTable(a->workspace, c, (unsigned long long)a->Nv);
    p.new_xyz = a->new_xyz; p.idx = a->idx; p.cnt = a->cnt; p.M = a->M; p.S = a->S;
    for (int d = 0; d < 3; ++d) { p.G[d] = a->spatial_shape[d]; p.r[d] = a->max_range[d]; p.v[d] = a->voxel_size[d]; p.lo[d] = a->lo[d]; }
    volatile float r2 = a->radius * a->radius;          // (one binary32 rounding)
    p.r2 = r2;
    const hipStream_t st = (hipStream_t)stream;
    launch_coord_rows(a->coors, a->offsets, a->Nv, a->B, p.G[1], p.G[2], p.t, st);
    if (int rc = sad::check_launch(fn)) return rc;
    hipLaunchKernelGGL(voxel_query_kernel, dim3(sad::blocks_for((unsigned long long)a->M, VQ_WAVES), a->B), dim3(VQ_WAVES * 64), 0, st, p);
    return sad::check_launch(fn);
}

SAD_API int sad_roi_grid_points_f32(const sad_roi_grid_points_args *a, sad_stream_t stream) {
    const char *fn = "sad_roi_grid_points_f32";
    if (int rc = args_ok(fn, a)) return rc;
    SAD_REQUIRE(a->rois && a->pts, "%s: NULL pointer", fn);
    SAD_REQUIRE(a->B >= 1 && a->R >= 1 && a->G >= 1, "%s: need B, R, G >= 1 (got %d, %d, %d)", fn, a->B, a->R, a->G);
    SAD_REQUIRE(a->D >= 7, "%s: rois rows have D = %d columns (need D >= 7)", fn, a->D);
    if (a->G > RGP_MAX_G) return sad::fail(SAD_EUNSUPPORTED, "%s: G = %d (at most %d)", fn, a->G, RGP_MAX_G);
    if (a->B > 65535) return sad::fail(SAD_EUNSUPPORTED, "%s: B = %d (at most 65535)", fn, a->B);
    const long long total = (long long)a->B * a->R * (a->G * a->G * a->G);
    if (total >= (1LL << 31)) return sad::fail(SAD_EUNSUPPORTED, "%s: B * R * G^3 = %lld points (must be below 2^31)", fn, total);
    hipLaunchKernelGGL(roi_grid_points_kernel, dim3(sad::blocks_for((unsigned long long)total, 256)), dim3(256), 0, (hipStream_t)stream, a->rois,
                       a->roi_count, a->R, a->D, a->G, total, a->pts);
    return sad::check_launch(fn);
}
