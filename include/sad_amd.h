/*
 * sad_amd.h — C-ABI of libsad_amd.so: hand-written gfx950 (MI355X) HIP kernels for the
 * set-abstraction + size-adaptive-clustering hot path.
 *
 * Reference interface replaced: none exists.  The upstream reference is a two-line README
 * (/root/reference/README.md:1-2) and defines no operator/FFI surface; the entry points below are
 * the ones BASELINE.json north_star names ("fps / ball_query / group_points / sa_module ... through
 * a thin C-ABI extension"), with the semantics frozen in this repository's SPEC.md (section cited
 * per function).  The Python binding a maintainer would add is in INTEGRATION.md.
 *
 * Contract (all functions):
 *  - plain pointers and sizes only; no torch / C++ types cross the boundary;
 *  - every data pointer is DEVICE memory owned by the caller (inputs, outputs and workspace); the
 *    library never allocates, frees or retains device memory; pointer ARRAYS and small parameter
 *    arrays (dims, radii, nsamples) are HOST memory read before the call returns;
 *  - work is enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream) of the
 *    current device and the call returns without synchronising;
 *  - returns 0 on success, a negative SAD_E* code otherwise; sad_last_error() gives a
 *    thread-local message; nothing throws across the boundary; re-entrant, no global mutable
 *    state other than the tuning options below.
 */
#ifndef SAD_AMD_H
#define SAD_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SAD_OK 0
#define SAD_EINVAL (-1)       /* bad argument (NULL pointer, size out of range, ...) */
#define SAD_EUNSUPPORTED (-2) /* shape outside what the kernels implement */
#define SAD_ELAUNCH (-3)      /* HIP reported a launch error */

#define SAD_MAX_LAYERS 4
#define SAD_MAX_RADII 4

typedef void *sad_stream_t; /* hipStream_t */

/* ABI version: bumped whenever a public struct layout or a signature changes (2 = sad_mlp_args / sad_mlp_bf16_args
 * start with struct_size; 3 = sad_mlp_args.c_out in the former tail padding, sad_mlp_padded_dims, sad_copy_rows_u32;
 * 4 = split pooling: sad_mlp_bf16_args.cont / n_pool / pool_*, sad_mlp_rowscan_split, sad_mlp_cont_bytes, larger row-packing tables).  The structs additionally carry their own size: a caller built against another header is
 * refused with SAD_EINVAL instead of being read past its end. */
#define SAD_ABI_VERSION 4
int sad_version(void);
const char *sad_last_error(void);
/* Tuning / A-B knobs (process-wide; defaults 0 = automatic).  Returns SAD_EINVAL for an unknown key.
 *   fps_variant  1 pair kernel, 2 key kernel, 3 wave buckets, 4 cell buckets (second form of the kernel: the default for
 *                N <= 16384), 5 cell buckets over sorted records (default for 16384 < N <= 65536), 6 cell buckets, FIRST form of
 *                the kernel (lane-elected publish, five writelanes per bucket update: kept as the A/B baseline of round 4)
 *   fps_threads  cell-bucket geometry waves*100 + slots (e.g. 1616, 832); old kernels: 1024/512/256 threads
 *   fps_dpp      1 = DPP reductions in the pair kernel
 *   bq_variant   1 = grid query: always the LDS-bitmap path (no 64-lane sort for centroids with <= 64 candidates);
 *                2 = grid query: ONE LDS bitmap set per workgroup (round 3's layout) instead of one per two waves;
 *                grid vs scan is the caller's choice: sad_ball_query_grid_f32 / sad_ball_query_multi_f32
 *   group_variant 1 = L2-gather group_points kernel only (no LDS staging)
 *   mlp_rw, mlp_budget_kb, mlp_force, mlp_dedup_f, mlp_nodedup, mlp_static, mlp_dyn_slots, mlp_noxcd: f32 chain geometry overrides
 *                (see sad_mlp_args.geometry; mlp_nodedup = 1 computes the padding rows too)
 *   mlp_layer_queue 1 = the layer-streamed chain kernel (geometry 3) pulls its items from per-XCD queues owned by the
 *                launching stream instead of a static round-robin.  Beside an FPS kernel of another stream the cluster
 *                dispatch of the benchmark is 15 % shorter (905 vs 1 080 us), alone 2 % longer, and the pipelined step
 *                (two main streams always busy) 1.5 % slower: off by default.  Same results either way.
 *   mlp_rows_form 1 = the bf16 row-streaming layer (sad_mlp_chain_bf16, one plain layer) always in its first form (rows straight to
 *                registers, register-staged weights) instead of the tiled GEMM fed by LDS-DMA that serves bf16 rows with
 *                K % 64 == 0.  Same results either way (the same products in the same order).
 * Test knobs of the item queues of the cooperative chain kernel (geometry 4; tables of >= 257 groups):
 *   mlp_steal_after v > 0: a workgroup treats the queue of its own XCD as empty after v - 1 items and takes its items from
 *                the other queues, one at a time and with nothing prefetched, so the cross-queue / weight-ring refill
 *                path that normally runs only at the tail of a dispatch runs all the time (same results);
 *   mlp_check_inuse 1: every dispatch stamps its id into the queue header and flags a conflict when it finds another
 *                dispatch's id there (two dispatches sharing one workspace at the same time).
 * Instrumentation ints of a row-packing table (sad_mlp_args.workspace as int32[]; zeroed by the row-packing scan,
 * accumulated by the launches that reuse the table): [5] weight-ring refills, [6] id of the dispatch that owns the
 * queues right now (0 = none), [7] != 0: a conflict was seen. */
#define SAD_WS_REFILLS 5
#define SAD_WS_INUSE 6
#define SAD_WS_CONFLICT 7
int sad_set_option(const char *key, int value);

/* SPEC.md §2.  xyz[B,N,3] -> idx[B,M].  N < 2048 needs no workspace; otherwise pass
 * sad_fps_workspace_bytes(B,N) bytes of 16-byte aligned device workspace (Z-order permutation for
 * the bucketed kernels; + sorted point records for 16384 < N <= 65536).  Without a workspace,
 * N <= 16384 falls back to the plain register-resident scan. */
size_t sad_fps_workspace_bytes(int B, int N);
int sad_fps_f32(const float *xyz, int B, int N, int M, int32_t *idx, void *workspace,
                sad_stream_t stream);

/* SPEC.md §15.  Feature-distance FPS: xyz[B,N,3], feat point-major [B,N,C]
 * with row stride ld_feat (floats) -> idx[B,M]; N <= 16384.  Two phases on the given stream: all
 * N x N distances in the exact §15 order (sad_pairdist_f32, parallel over the chip) into
 * `workspace` (sad_ffps_workspace_bytes(B,N) = B*N*N*4 bytes), then the serial sampling chain
 * reading one matrix row per step. */
size_t sad_ffps_workspace_bytes(int B, int N);
int sad_pairdist_f32(const float *xyz, const float *feat, int ld_feat, int B, int N, int C,
                     float w_xyz, float *dmat, sad_stream_t stream);
int sad_ffps_f32(const float *xyz, const float *feat, int ld_feat, int B, int N, int C, int M,
                 float w_xyz, int32_t *idx, void *workspace, sad_stream_t stream);

/* SPEC.md §5.  gather_xyz: xyz[B,N,3], idx[B,M] -> out[B,M,3].
 * gather_points: src[B,C,N], idx[B,M] -> out[B,C,M]; elem_size 2 or 4 bytes.
 * group_points:  feat[B,C,N], idx[B,M,S] -> out[B,C,M,S]; elem_size 2 or 4 bytes. */
int sad_gather_xyz_f32(const float *xyz, const int32_t *idx, int B, int N, int M, float *out,
                       sad_stream_t stream);
int sad_gather_points(const void *src, const int32_t *idx, int B, int C, int N, int M,
                      int elem_size, void *out, sad_stream_t stream);
int sad_group_points(const void *feat, const int32_t *idx, int B, int C, int N, int M, int S,
                     int elem_size, void *out, sad_stream_t stream);

/* SPEC.md §16: backward of the unfused operators.
 * group_points_grad: grad_out[B,C,M,S], idx[B,M,S] -> grad_feat[B,C,N] += scatter-add (float
 * atomics; grad_feat must be zero, or hold a gradient to accumulate into, on entry); S = 1 is
 * gather_points_grad.  max_pool_s: x[B,C,M,S] -> out[B,C,M], arg[B,C,M] (ties -> lowest s);
 * max_pool_s_grad: grad_out[B,C,M], arg -> grad_x[B,C,M,S]. */
int sad_group_points_grad_f32(const float *grad_out, const int32_t *idx, int B, int C, int N, int M,
                              int S, float *grad_feat, sad_stream_t stream);
/* Same sum into a POINT-MAJOR gradient grad_feat_pm[B,N,C] (zero / accumulate on entry): channels on
 * the lanes, so the float atomics are 256 contiguous bytes per wave instruction (full memory-side
 * rate, ~16x the channel-major scatter).  Transpose afterwards if a [B,C,N] gradient is needed. */
int sad_group_points_grad_pm_f32(const float *grad_out, const int32_t *idx, int B, int C, int N,
                                 int M, int S, float *grad_feat_pm, sad_stream_t stream);
int sad_max_pool_s_f32(const float *x, int B, int C, int M, int S, float *out, int32_t *arg,
                       sad_stream_t stream);
int sad_max_pool_s_grad_f32(const float *grad_out, const int32_t *arg, int B, int C, int M, int S,
                            float *grad_x, sad_stream_t stream);

/* SPEC.md §3.  xyz[B,N,3], new_xyz[B,M,3] -> idx[B,M,S], 1 <= S <= 64.
 * radius_pc == NULL: scalar `radius`; else per-centroid radius_pc[B,M] (adaptive) and `radius`
 * is ignored. */
int sad_ball_query_f32(const float *xyz, const float *new_xyz, float radius,
                       const float *radius_pc, int B, int N, int M, int S, int32_t *idx,
                       sad_stream_t stream);
/* Multi-radius form: d2 evaluated once per pair, SPEC.md §3 applied per radius.  radii[n_radii] and
 * nsamples[n_radii] are host arrays, idx[n_radii] a host array of device pointers (idx[r] is
 * [B,M,nsamples[r]]).  With radius_pc != NULL the radius of branch r for centroid (b,m) is
 * radii[r] * radius_pc[b,m] (one binary32 multiply; SPEC.md §8 step 5).
 * cnt (may be NULL, entries may be NULL): host array of device pointers; cnt[r][b,m] receives the
 * number of accepted points capped at nsamples[r] — the rows of the group that are not padding. */
int sad_ball_query_multi_f32(const float *xyz, const float *new_xyz, int n_radii,
                             const float *radii, const float *radius_pc, const int *nsamples,
                             int32_t *const *idx, int32_t *const *cnt, int B, int N, int M,
                             sad_stream_t stream);

/* Same results as sad_ball_query_multi_f32 with scalar radii, computed through a per-scene uniform
 * grid (cell edge > max radius): each centroid tests only the 27 cells around it and index order is
 * restored through an LDS bitmap.  Needs sad_ball_query_grid_workspace_bytes(B,N) bytes of 16-byte
 * aligned device workspace (rebuilt on every call); N <= 65536. */
size_t sad_ball_query_grid_workspace_bytes(int B, int N);
int sad_ball_query_grid_f32(const float *xyz, const float *new_xyz, int n_radii, const float *radii,
                            const int *nsamples, int32_t *const *idx, int32_t *const *cnt, int B,
                            int N, int M, void *workspace, sad_stream_t stream);

/* SPEC.md §17 (the step before the path).  Ragged scenes -> fixed point count:
 * points[total, C] (C floats per point), offsets[B+1] (device, int32; scene b owns rows offsets[b] ..
 * offsets[b+1]-1) -> out[B, n_points, C].  Deterministic for (seed, scene); integer arithmetic only, so the
 * rows equal those of the numpy loader (io.fix_size) and of the oracle. */
int sad_subsample_pad_f32(const float *points, const int32_t *offsets, int B, int C, int n_points,
                          unsigned seed, float *out, sad_stream_t stream);

/* Strided row copy in 4-byte words (no arithmetic: exact): row r of dst = words [0, row_words) of row r of src, rows
 * src_stride_words / dst_stride_words apart (dst_stride_words >= row_words; src rows may overlap dst rows never).  What the
 * host side uses instead of a framework copy wherever a strided view has to become a packed operand on the step — the
 * coordinates / features of a [B,N,3+C] point array, the centroid prefix of a nested sampling stage, the candidate rows of the
 * cluster layer — so that every device operation of a step is a launch of this library (and can be recorded and replayed:
 * 3dsad-main_amd/plan.py).  No reference counterpart (/root/reference/README.md:1-2). */
int sad_copy_rows_u32(const void *src, long long src_stride_words, void *dst, long long dst_stride_words,
                      long long n_rows, long long row_words, sad_stream_t stream);

/* SPEC.md §18 (feature propagation).  Additions of ABI 4: the version is unchanged.
 * three_nn: unknown[B,n,3], known[B,m,3] (m >= 1) -> dist2[B,n,3], idx[B,n,3]: the three smallest (d2, j), ascending,
 * ties -> lowest j; slots k >= m hold d2 = +inf, idx = 0.  w (may be NULL) -> [B,n,3] interpolation weights of §18.
 * Option "nn_variant": 0 LDS tiles, one unknown point per lane (default); 1 scalar loads; 2 LDS tiles, two points per lane.
 * three_interpolate: out = (w0*f[idx0] + w1*f[idx1]) + w2*f[idx2], exact.  point_major = 0: feat[B,C,m] -> out[B,C,n]
 * (ld_out = n, col_off = 0); point_major = 1: feat[B,m,C] -> out[(b*n+i)*ld_out + col_off + c] (ld_out >= col_off + C):
 * a column slice of wider rows, the other columns untouched.  Indices must be in [0,m) (one outside reads a zero feature).
 * three_interpolate_grad: grad_out [B,C,n] (point_major = 0) or [B,n,C] (1), idx, w -> grad_feat_pm[B,m,C] += w_k * grad_out
 * at idx_k (float atomics, order unspecified; zero or a gradient to accumulate into on entry).  Always point-major: transpose
 * afterwards for [B,C,m].  idx and w get no gradient. */
int sad_three_nn_f32(const float *unknown, const float *known, int B, int n, int m, float *dist2,
                     int32_t *idx, float *w, sad_stream_t stream);
int sad_three_interpolate_f32(const float *feat, const int32_t *idx, const float *w, int B, int C,
                              int m, int n, int point_major, float *out, int ld_out, int col_off,
                              sad_stream_t stream);
int sad_three_interpolate_grad_f32(const float *grad_out, const int32_t *idx, const float *w, int B,
                                   int C, int n, int m, int point_major, float *grad_feat_pm,
                                   sad_stream_t stream);

/* SPEC.md §19 (box operators).  Additions of ABI 4: the version is unchanged.  Boxes are rows of D >= 7 floats
 * (cx, cy, cz, l, w, h, yaw, ...), row stride D: the detector's 9-column boxes and 7-column boxes both pass.  No gradients.
 * boxes_iou: a[B,Ka,Da], b[B,Kb,Db] -> iou[B,Ka,Kb]; mode SAD_IOU_BEV = §13 iou_bev(a_i, b_j), SAD_IOU_3D = §19.3.  Any K.
 * points_in_boxes: xyz[B,N,3] -> box_idx[B,N] = the lowest k whose box contains the point (§19.1, e = 0), else -1.
 * roipoint_pool3d: per box, the first S points (ascending n) inside the box enlarged by extra_width (§19.2), repeated
 * cyclically -> pooled[B,K,S,3+C] rows [xyz || feat] (feat [B,N,C] point-major; NULL when C = 0), empty[B,K] (1: no point,
 * rows and idx zero), idx[B,K,S] (may be NULL).  1 <= S <= 8192 (SAD_EUNSUPPORTED above: the selection is held in LDS). */
#define SAD_IOU_BEV 0
#define SAD_IOU_3D 1
int sad_boxes_iou_f32(const float *a, const float *b, int B, int Ka, int Kb, int Da, int Db, int mode,
                      float *iou, sad_stream_t stream);
int sad_points_in_boxes_f32(const float *xyz, const float *boxes, int B, int N, int K, int D,
                            int32_t *box_idx, sad_stream_t stream);
int sad_roipoint_pool3d_f32(const float *xyz, const float *feat, const float *boxes, int B, int N,
                            int K, int D, int C, float extra_width, int S, float *pooled,
                            int32_t *empty, int32_t *idx, sad_stream_t stream);

/* SPEC.md §20 (voxelization).  Additions of ABI 4: the version is unchanged.  Ragged input as in §17: points[total_points, C]
 * (C >= 3 floats per row, columns 0..2 = x, y, z), offsets[B+1] (device, int32, non-decreasing, offsets[0] = 0, offsets[B] =
 * total_points; a scene may be empty).  voxel_size[3] = (vx,vy,vz) and point_range[6] = (x0,y0,z0,x1,y1,z1) are HOST arrays.
 * Grid G_d = (int)rintf((hi_d - lo_d) / v_d); a dimension below 1 or more than 2^31 - 1 cells in all: SAD_EUNSUPPORTED.
 * A point is valid iff 0 <= floorf((p_d - lo_d) / v_d) < G_d on every axis (on lo: valid, on hi: not).  Every result is a
 * function of the input alone (no dependence on the order of any atomic), bit for bit.
 * voxel_coords: -> coors[total_points,4] = (b, gz, gy, gx), or (b,-1,-1,-1) for an invalid point; coors 16-byte aligned.
 * voxel_index: voxels are numbered per scene in order of first appearance; a key first met when max_voxels exist is dropped
 *   with all its later points, the walk continues (§20.2) -> point2voxel[total_points] (scene-local number or -1),
 *   coors[B,V,3] (z,y,x), count[B,V] (all members, uncapped), voxel_num[B]; rows v >= voxel_num[b]: coors -1, count 0.
 * voxelize: -> voxels[B,V,T,C]: slot t of voxel v = the row of its t-th member in ascending row order (t < min(count, T)),
 *   every other float 0 — each float is written exactly once, no fill needed; coors[B,V,3], num_points[B,V] = min(count, T),
 *   voxel_num[B].  T = max_points >= 1, V = max_voxels >= 1.
 * voxel_reduce: feat[total_points,Cf], point2voxel (numbers outside [0,V) count as -1) -> out[B,V,Cf]: SAD_VOXEL_SUM adds the
 *   members in ascending row order, one rounding per addition; SAD_VOXEL_MEAN divides that sum once by (float)count;
 *   SAD_VOXEL_MAX the maximum, arg[B,V,Cf] = the global row of the first member that attains it (NULL for the other modes).
 *   Empty voxels: 0 and arg -1.  count (may be NULL) -> [B,V] member counts (what the mean's backward needs).
 * voxel_reduce_grad: grad_out[B,V,Cf] -> grad_feat[total_points,Cf], a gather: sum grad_out[b,p2v]; mean the same / (float)
 *   count (count_or_arg = count[B,V]); max grad_out where arg == row, else 0 (count_or_arg = arg[B,V,Cf]); p2v = -1: 0.
 * workspace: sad_voxel_workspace_bytes(total_points, B, max_voxels, &bytes) bytes of 16-byte aligned device scratch, contents
 * arbitrary on entry, reusable by the next call on the same stream.  total_points <= 2^30, B <= 65535, B * max_voxels < 2^31. */
#define SAD_VOXEL_SUM 0
#define SAD_VOXEL_MEAN 1
#define SAD_VOXEL_MAX 2
int sad_voxel_workspace_bytes(int total_points, int B, int max_voxels, size_t *bytes);
int sad_voxel_coords_f32(const float *points, const int32_t *offsets, int total_points, int B, int C,
                         const float *voxel_size, const float *point_range, int32_t *coors,
                         sad_stream_t stream);
int sad_voxel_index_f32(const float *points, const int32_t *offsets, int total_points, int B, int C,
                        const float *voxel_size, const float *point_range, int max_voxels,
                        int32_t *point2voxel, int32_t *coors, int32_t *count, int32_t *voxel_num,
                        void *workspace, sad_stream_t stream);
int sad_voxelize_f32(const float *points, const int32_t *offsets, int total_points, int B, int C,
                     const float *voxel_size, const float *point_range, int max_points, int max_voxels,
                     float *voxels, int32_t *coors, int32_t *num_points, int32_t *voxel_num,
                     void *workspace, sad_stream_t stream);
int sad_voxel_reduce_f32(const float *feat, const int32_t *point2voxel, const int32_t *offsets,
                         int total_points, int B, int Cf, int max_voxels, int mode, float *out,
                         int32_t *arg, int32_t *count, void *workspace, sad_stream_t stream);
int sad_voxel_reduce_grad_f32(const float *grad_out, const int32_t *point2voxel, const int32_t *offsets,
                              int total_points, int B, int Cf, int max_voxels, int mode,
                              const int32_t *count_or_arg, float *grad_feat, sad_stream_t stream);

/* SPEC.md §24 (voxel feature encoder).  Additions of ABI 4: the version is unchanged.  points[total_points, C], offsets[B+1] and
 * point2voxel[total_points] as for voxel_reduce (numbers outside [0, max_voxels) count as -1).  The members of voxel (b,v) are
 * the rows with point2voxel == v in ascending row order, with max_points = T >= 1 only the first T of them (0: no cap); there
 * are no padding slots.  flags: SAD_VFE_CLUSTER_CENTER appends points[i,0:3] - mean (mean: §20.5 over the members),
 * SAD_VFE_VOXEL_CENTER appends points[i,0:3] - ((float)g_d * v_d + (0.5f * v_d + lo_d)) with g from coors[B,V,3] (z,y,x) and
 * the HOST arrays voxel_size[3], point_range[6] (all three may be NULL without that flag); vox_feat[B,V,Cv] (NULL with Cv = 0)
 * is appended last.  Cin = C + 3 + 3 + Cv as flagged, 1 <= Cin <= 256 (SAD_EUNSUPPORTED above); decorations need C >= 3.
 * voxel_decorate: -> rows[total_points, Cin], zeros for rows that are not members.
 * voxel_encode: the fused form.  y = one §6 layer of the decorated row (acc = bias[o]; k ascending: acc = fmaf(W[o][k],
 *   row[k], acc); SAD_VFE_RELU: acc > 0 ? acc : 0) with weight[Cout,Cin], bias[Cout] on the device, 1 <= Cout <= 256
 *   (SAD_EUNSUPPORTED above) -> pooled[B,V,Cout] = the maximum over the members, 0 without members; arg[B,V,Cout] (may be
 *   NULL) = the lowest member row that attains it, -1 without members; pointwise[total_points,Cout] (may be NULL) = y of every
 *   member row, 0 for the others.  Every output float is written exactly once: no fill is needed before the call.
 *   B * max_voxels * Cout < 2^40.  Bit-equal from call to call; equal to the reference under == (sign of a zero unspecified).
 * workspace: sad_voxel_encode_workspace_bytes(total_points, B, max_voxels, Cin, Cout, &bytes) bytes of 16-byte aligned device
 * scratch (Cout = 0: what voxel_decorate needs), contents arbitrary on entry, reusable by the next call on the same stream. */
#define SAD_VFE_CLUSTER_CENTER 1
#define SAD_VFE_VOXEL_CENTER 2
#define SAD_VFE_RELU 4
int sad_voxel_encode_workspace_bytes(int total_points, int B, int max_voxels, int Cin, int Cout, size_t *bytes);
int sad_voxel_decorate_f32(const float *points, const int32_t *point2voxel, const int32_t *offsets,
                           const int32_t *coors, const float *vox_feat, int total_points, int B, int C,
                           int max_voxels, int Cv, const float *voxel_size, const float *point_range,
                           int flags, int max_points, float *rows, void *workspace, sad_stream_t stream);
int sad_voxel_encode_f32(const float *points, const int32_t *point2voxel, const int32_t *offsets,
                         const int32_t *coors, const float *vox_feat, int total_points, int B, int C,
                         int max_voxels, int Cv, const float *voxel_size, const float *point_range,
                         const float *weight, const float *bias, int Cout, int flags, int max_points,
                         float *pooled, int32_t *arg, float *pointwise, void *workspace, sad_stream_t stream);

/* SPEC.md §21 (sparse 3-D convolution).  Additions of ABI 4: the version is unchanged.  A sparse tensor is feat[Nv,C] f32,
 * coors[Nv,3] int32 (z,y,x), offsets[B+1] int32 on the device (scene b owns rows offsets[b] .. offsets[b+1]-1, offsets[0] = 0,
 * offsets[B] = Nv, a scene may be empty) and a HOST spatial_shape[3] = (Gz,Gy,Gx), at most 2^31 - 1 cells.  kernel, stride and
 * padding are HOST arrays of 3 ints in (z,y,x) order: kernel sizes 1 .. 3, stride >= 1, padding >= 0.  Coordinates outside the
 * grid are undefined behaviour.  kk = (kz*Ky + ky)*Kx + kx; nbr[o,kk] = the lowest input row of o's scene at
 * out_coors[o]*s - p + k, or -1.  Nv <= 2^30, Nv * Kvol < 2^31, B <= 65535.
 *
 * workspace: sad_spconv_workspace_bytes(Nv, B, kernel, stride, subm, &bytes) bytes of 16-byte aligned device scratch (stride is
 *   ignored and may be NULL when subm != 0).  Contents arbitrary on entry.  index_count leaves in it what index_fill needs: the
 *   two calls share one workspace, on one stream, with nothing of the library in between.
 * index_subm: odd kernel sizes, stride 1, padding K/2: the outputs ARE the inputs (out_coors = coors, out_offsets = offsets);
 *   -> nbr[Nv,Kvol].
 * index_count: the strided form, first half -> out_offsets[B+1] on the device (out_offsets[B] = No, the number of active output
 *   sites, numbered per scene in order of first appearance over the candidates (input row, kk) ascending).
 * index_fill: second half, with the out_offsets of index_count -> out_coors[capacity,3], nbr[capacity,Kvol]: rows below
 *   min(No, capacity) are filled, rows from No up to capacity get -1; nothing is written at or beyond capacity.
 * pack: W[Kvol,Cout,Cin] row-major (+ bias[Cout] or NULL) -> packed[sad_spconv_packed_floats(Kvol,Cin,Cout)] floats, 16-byte
 *   aligned: the fragment image the convolution reads.  1 <= Cin, Cout <= 256 (SAD_EUNSUPPORTED above; packed_floats returns 0).
 * spconv: out[No,Cout] = bias + sum over kk ascending, ci ascending of W[kk][co][ci] * feat[nbr[o,kk]][ci] (fmaf chain, §21.2),
 *   then + residual[No,Cout] (may be NULL), then ReLU if relu != 0.  nbr entries outside [0, Nv) count as -1.
 * sparse_to_dense: -> dense[B,C,Oz,Oy,Ox], zero where no row is, the lowest row of a cell elsewhere; rows with a coordinate
 *   outside out_shape are skipped.  workspace: sad_sparse_to_dense_workspace_bytes(B, out_shape, &bytes), B*Oz*Oy*Ox < 2^31. */
int sad_spconv_workspace_bytes(int Nv, int B, const int *kernel, const int *stride, int subm, size_t *bytes);
int sad_spconv_index_subm(const int32_t *coors, const int32_t *offsets, int Nv, int B, const int *spatial_shape,
                          const int *kernel, int32_t *nbr, void *workspace, sad_stream_t stream);
int sad_spconv_index_count(const int32_t *coors, const int32_t *offsets, int Nv, int B, const int *spatial_shape,
                           const int *kernel, const int *stride, const int *padding, int32_t *out_offsets,
                           void *workspace, sad_stream_t stream);
int sad_spconv_index_fill(const int32_t *coors, const int32_t *offsets, int Nv, int B, const int *spatial_shape,
                          const int *kernel, const int *stride, const int *padding, const int32_t *out_offsets,
                          int capacity, int32_t *out_coors, int32_t *nbr, void *workspace, sad_stream_t stream);
size_t sad_spconv_packed_floats(int Kvol, int Cin, int Cout);
int sad_spconv_pack_f32(const float *W, const float *bias, int Kvol, int Cin, int Cout, float *packed,
                        sad_stream_t stream);
int sad_spconv_f32(const float *feat, const int32_t *nbr, const float *packed, const float *residual, int relu,
                   int Nv, int No, int Kvol, int Cin, int Cout, float *out, sad_stream_t stream);
int sad_sparse_to_dense_workspace_bytes(int B, const int *out_shape, size_t *bytes);
int sad_sparse_to_dense_f32(const float *feat, const int32_t *out_coors, const int32_t *out_offsets, int No, int B,
                            int C, const int *out_shape, float *dense, void *workspace, sad_stream_t stream);
/* SPEC.md §21.4 (backward of the sparse convolution; additions of ABI 4 as well).  g[No,Cout] is the gradient of the output AFTER
 * the ReLU mask (g = out > 0 ? grad_out : 0 is the caller's).
 * index_transpose: nbr[No,Kvol] -> nbrT[Nv,Kvol], nbrT[i,kk] = the lowest o with nbr[o,kk] == i or -1, and *collisions (device) =
 *   the number of (o,kk) with i = nbr[o,kk] in [0, Nv) and nbrT[i,kk] != o.  Entries outside [0, Nv) count as -1.
 *   No * Kvol, Nv * Kvol < 2^31.  grad_feat[Nv,Cin] is then sad_spconv_f32(g, nbrT, pack(W^T), NULL, 0, No, Nv, Kvol, Cout, Cin),
 *   W^T[kk][ci][co] = W[kk][co][ci]: the true gradient iff *collisions == 0.
 * grad_weight: grad_W[Kvol,Cout,Cin] = sum over o with nbr[o,kk] >= 0 of g[o][co] * feat[nbr[o,kk]][ci] and, unless NULL,
 *   grad_bias[Cout] = sum over o of g[o][co]; both are OVERWRITTEN (zeros for No = 0 or Nv = 0).  either may be NULL (not both): a NULL grad_W
 *   launches the column sums only.  binary32 sums whose order is not specified: float atomics, so two calls may differ in the last
 *   bits.  Option "spconv_grad_ranges" (test knob): n > 0 = split the output rows into about n ranges of 64-row tiles (at most 1024
 *   tiles each, more ranges beyond), 0 = sized by the device (default).  1 <= Cin, Cout <= 256, Kvol <= 27.  workspace:
 *   sad_spconv_grad_weight_workspace_bytes(No, Kvol, Cin, Cout, &bytes) bytes of 16-byte aligned device scratch; this form needs
 *   none (bytes = 0, workspace may then be NULL). */
int sad_spconv_index_transpose(const int32_t *nbr, int No, int Nv, int Kvol, int32_t *nbrT, int32_t *collisions,
                               sad_stream_t stream);
int sad_spconv_grad_weight_workspace_bytes(int No, int Kvol, int Cin, int Cout, size_t *bytes);
int sad_spconv_grad_weight_f32(const float *feat, const int32_t *nbr, const float *g, int Nv, int No, int Kvol, int Cin,
                               int Cout, float *grad_W, float *grad_bias, void *workspace, sad_stream_t stream);
/* SPEC.md §22 (sparse max pool over a rulebook and its backward; additions of ABI 4 as well).  nbr[No,Kvol] is any rulebook of §21
 * (Kvol <= 27), nbrT[Nv,Kvol] its transpose (sad_spconv_index_transpose).  1 <= C, Nv * C and No * C < 2^31 (SAD_EUNSUPPORTED above).
 * max_pool: out[No,C] = per channel the maximum of feat[nbr[o,kk]][c] over the entries in [0, Nv), walked kk ascending, a later one
 *   replacing the first only if strictly greater (ties, -0.0f against +0.0f included, stay with the lowest kk): a bit copy of one
 *   input element; arg[No,C] = the GLOBAL input row it came from.  A row without a valid entry: 0.0f and -1.  NaN undefined.
 * max_pool_grad: grad_feat[Nv,C] (OVERWRITTEN) = from +0.0f, kk ascending, + g[o][c] for o = nbrT[i,kk] in [0, No) with
 *   arg[o][c] == i: a gather, no atomics, the same bits on every call; the true gradient iff the transpose has no collisions.
 * The inverse convolution of §22.3 has no entry point of its own: it is sad_spconv_f32(feat, nbrT, packed, residual, relu, No, Nv,
 *   Kvol, Cin, Cout, out) with the rows of the rulebook's output in the place of Nv and those of its input in the place of No. */
int sad_spconv_max_pool_f32(const float *feat, const int32_t *nbr, int Nv, int No, int Kvol, int C, float *out, int32_t *arg,
                            sad_stream_t stream);
int sad_spconv_max_pool_grad_f32(const float *g, const int32_t *arg, const int32_t *nbrT, int Nv, int No, int Kvol, int C,
                                 float *grad_feat, sad_stream_t stream);

/* SPEC.md §4.  -> idx[B,M,K] sorted by (d2, index); K <= 64, K <= N. */
int sad_knn_f32(const float *xyz, const float *new_xyz, int B, int N, int M, int K, int32_t *idx,
                sad_stream_t stream);

/* ---- grouped point-feature MLP (SPEC.md §6) ------------------------------------------------
 * Weights are repacked once into MFMA A-fragment order.  dims[L+1] = {C_in, C_1, ..., C_L} (host).
 * first_has_xyz != 0: the first layer's input is [rel_xyz(3) || feat(C_in-3)].
 * W[l] is [dims[l+1], dims[l]] row-major, bias[l] is [dims[l+1]] (host arrays of device pointers).
 * `packed` needs sad_mlp_packed_floats() floats. */
size_t sad_mlp_packed_floats(int L, const int *dims, int first_has_xyz);
int sad_mlp_pack_f32(int L, const int *dims, int first_has_xyz, const float *const *W,
                     const float *const *bias, float *packed, sad_stream_t stream);

typedef struct sad_mlp_args {
    size_t struct_size;   /* = sizeof(sad_mlp_args) of the header the caller was built against */
    /* grouped mode (idx != NULL): rows are (b, m, s); input row = [xyz[idx]-new_xyz || feat[idx]] */
    const float *xyz;     /* [B,N,3]                                   (grouped mode) */
    const float *new_xyz; /* [B,M,3]                                   (grouped mode) */
    const int32_t *idx;   /* [B,M,S] or NULL                                          */
    /* optional [B,M]: leading rows of each group that are not padding (from ball query); NULL =
     * derived from idx as "last sample that differs from the first, + 1" */
    const int32_t *cnt;
    /* optional, grouped mode with cnt: sad_mlp_workspace_bytes(B, M, S) bytes of 16-byte aligned
     * device scratch.  The surviving rows of ALL groups are then packed globally (one prefix-sum
     * workgroup) and a persistent grid pulls full passes from a work counter; without it each
     * workgroup packs only its own groups.  The table also holds the work counters / item queues of the
     * kernel that consumes it, so ONE dispatch at a time may use a given workspace (dispatches that run
     * side by side on different streams need a workspace each; a prescanned table may be reused by
     * consecutive launches of geometry 2 / 3 / 4 on one stream — they re-arm what they use). */
    void *workspace;
    /* features: grouped mode: point-major [B,N,C] with row stride ld_feat (NULL iff C == 0);
     * plain mode (idx == NULL): rows [B*M, C] with row stride ld_feat */
    const float *feat;
    int ld_feat;
    int B, N, M, S, C; /* plain mode: N ignored, S must be 1 */
    /* layers */
    int L;                        /* 1..SAD_MAX_LAYERS */
    int dims[SAD_MAX_LAYERS + 1]; /* dims[0] = C (+3 in grouped mode) */
    const float *packed;          /* from sad_mlp_pack_f32 with the same L, dims, first_has_xyz */
    int relu_mask;                /* bit l set = ReLU after layer l */
    /* output: point-major rows.  grouped mode: max over the S samples of each (b,m) ->
     * out[(b*M+m)*ld_out + col_off + o]; plain mode: out[row*ld_out + col_off + o].
     * GROUPED MODE NEEDS THE OUTPUT SLICE ZERO-INITIALISED: groups whose rows straddle two row tiles
     * are combined with an atomic max (every layer of a grouped chain must carry a ReLU, so outputs
     * are >= 0).  Trailing samples that repeat a group's first index (ball-query padding) are not
     * computed at all — a duplicate row cannot change the max. */
    float *out;
    int ld_out;
    int col_off;
    /* workgroup geometry: 0 = built-in heuristic; else W*100 + log2(WN)*10 + RW with W in {4,8}
     * waves, WN waves along the 32-channel output tiles, RW in {1,2,4} row tiles of 32 rows per
     * wave.  A geometry that does not fit LDS returns SAD_EUNSUPPORTED (autotuners skip it).
     * + 1000*f (f = 1..7): grouped mode, a workgroup owns 2^f * R / S groups (default 8: it assumes
     * about one row in eight survives the padding removal).
     * + 10000*d: d = 1 forces global row packing (needs cnt + workspace), d = 2 forbids it.
     * + 100000: with RW = 1, the (output tile, row tile) items of every layer are dealt round-robin
     *   to all W waves instead of the fixed WN x WM grid (no wave idles in a layer narrower than WN tiles).
     * + 200000: with RW = 1 (4 or 8 waves), a wave computes two output tiles per round as two
     *   independent accumulator chains sharing the activation operand (+300000 = both).
     * Other kernels (grouped mode with cnt + workspace; SAD_EUNSUPPORTED where they do not apply):
     *   1 = row-per-lane vector-ALU kernel (two narrow SA1 shapes);
     *   2 = register-resident chain: one wave carries a 32-row tile through a 3-layer chain in registers
     *       (compiled shapes: the SA stages of the KITTI / nuScenes topology and BASELINE configs[0]);
     *   3 = layer-streamed chain: one launch per layer, (128 rows x 128 output channels) work items,
     *       activations between layers in `scratch` (wide chains with few rows: the cluster layer); also
     *       on plain rows (idx == NULL) when C % 8 == 0 and every width, C_out included, is a multiple of 128;
     *   4 = cooperative register-resident chain: as 2, but the four waves of a workgroup walk four tiles
     *       through the chain in lockstep and share the weight stream through an LDS ring (one global load per
     *       16 MFMAs instead of one per 4; compiled for the SA2 / SA3 shapes 67 -> 64 -> {64,96} -> 128 and
     *       131 -> 128 -> {128,192,256} -> 256);
     *   5 = row-streaming layer: ONE plain layer (idx == NULL, L == 1, C % 8 == 0, 16-byte aligned rows): a wave owns 32 rows
     *       and all output channels of its item, its input rows never pass through LDS (the stage aggregations). */
    int geometry;
    /* geometry 3 only: sad_mlp_scratch_bytes(B, M, S, L, dims) bytes of 16-byte aligned device scratch */
    void *scratch;
    size_t scratch_bytes;
    /* != 0: `workspace` already holds the row-packing table of (cnt, idx) from sad_mlp_rowscan (geometries 2,
     * 3 and 4 only): the chain launches no scan of its own.  The scan needs coordinates-side data only, so a
     * caller can run it right behind the ball query on another stream, off the MLP stream's critical path. */
    int prescanned;
    /* ABI 3 (occupies what was tail padding of the ABI-2 struct: sizeof is unchanged, a zeroed ABI-2 struct means 0).
     * != 0: the chain was packed ZERO-PADDED onto wider dims (sad_mlp_padded_dims): `dims` are the padded ones, C + 3 <= dims[0]
     * feature channels exist per row and only the first c_out <= dims[L] output channels are stored.  The padded weights
     * and biases are zeros, so every fmaf chain gains only exact +0 terms behind its real ones: same results.  Grouped mode,
     * geometries 2 and 4 (register-resident / cooperative chain) only — that is what it is for: a chain that is not a
     * compiled shape runs on the compiled shape that dominates it. */
    int c_out;
} sad_mlp_args;
size_t sad_mlp_workspace_bytes(int B, int M, int S);
/* Row-packing tables of n (<= SAD_MAX_RADII) chains over the same (B, N, M): cnt[i] [B,M] and idx[i] [B,M,S[i]] from the
 * ball query -> workspace[i] (sad_mlp_workspace_bytes(B, M, S[i]) bytes each, 16-byte aligned).  Two launches
 * for all n.  Pass the workspaces to sad_mlp_chain_f32 with prescanned = 1. */
int sad_mlp_rowscan(int n, const int32_t *const *cnt, const int32_t *const *idx, const int *S, int B, int N,
                    int M, void *const *workspace, sad_stream_t stream);
/* The same, and it prepares the pooled-output buffers so that they need NO zero fill: for chain i, columns
 * [col_off[i], col_off[i] + cout[i]) of the rows out[i][(b*M+m)*ld_out[i] + ...] are set to zero for exactly the groups
 * whose packed rows straddle a 32-row tile — the only ones the chain kernels of geometries 2 / 3 / 4 (bf16: 2) combine
 * with an atomic max; every other group is written with plain stores.  (A 32-scene KITTI-shaped step otherwise zero-fills
 * 217 MB of pooling buffers.)  A scan that sad_mlp_chain[_multi]_f32 / _bf16 launches itself (prescanned == 0, geometries
 * 2 / 3 / 4) does the same with the call's own `out`.  The tiled kernels (geometry 0 / tile heights) still need `out`
 * zeroed by the caller. */
int sad_mlp_rowscan_init(int n, const int32_t *const *cnt, const int32_t *const *idx, const int *S, int B, int N,
                         int M, void *const *workspace, float *const *out, const int *ld_out, const int *col_off,
                         const int *cout, sad_stream_t stream);
size_t sad_mlp_scratch_bytes(int B, int M, int S, int L, const int *dims);
/* The `geometry` a caller that does not autotune should pass for a GROUPED chain of this shape when it provides
 * cnt + workspace (+ scratch for 3): 4 (cooperative register-resident chain: the SA3 shapes), 2 (register-resident
 * chain: the other compiled shapes), 3 (layer-streamed chain: every padded width a multiple of 128), else a code of the tiled
 * kernel (eight waves, round-robin items, workgroup-local row packing: what the autotuner picks for chains that are not
 * compiled shapes; a caller retries with 0 = built-in heuristic when it is refused with SAD_EUNSUPPORTED: LDS).  Matches what
 * the autotuner picks on the KITTI-shaped benchmark; never 0 for a valid chain. */
int sad_mlp_preferred_geometry(int L, const int *dims);
/* Is there a compiled shape of the register-resident chain kernels that DOMINATES this grouped 3-layer chain (every padded
 * width >= the chain's) at no more than 1.6 x its flops?  Returns 1 and the dims to pack for in padded[0..L] (pack the chain's
 * weights zero-padded to them, call with sad_mlp_args.dims = padded, C = the true feature channels, c_out = the true output
 * width), else 0.  C must be 0, 1 or a multiple of 4 (the kernels' feature-row layouts).  A chain that IS a compiled shape
 * returns 0 (nothing to pad). */
int sad_mlp_padded_dims(int L, const int *dims, int *padded);
int sad_mlp_chain_f32(const sad_mlp_args *args, sad_stream_t stream);
/* n independent chains (typically the branches of one multi-radius stage, each writing its own
 * column slice) in one dispatch when they share a wave count: the light chains fill the tail of the
 * heavy one and the launch gaps disappear.  Same results as n sad_mlp_chain_f32 calls. */
int sad_mlp_chain_multi_f32(const sad_mlp_args *const *args, int n, sad_stream_t stream);

/* SPEC.md §14 — the same chain in bfloat16 on the matrix cores (BASELINE.json configs[4]).
 * Weights are rounded to bf16 and laid out in MFMA fragment order by sad_mlp_pack_bf16 (W/bias as
 * for sad_mlp_pack_f32; `packed` needs sad_mlp_packed_bytes_bf16() bytes, 16-byte aligned).
 * Fields as in sad_mlp_args, except: feat is bf16 (feat_bf16 = 1) or f32 (0, rounded on load) with
 * ld_feat in ELEMENTS; grouped output is f32 and must be zero on entry (atomic max merge); plain
 * output is f32 or bf16 (out_bf16). */
size_t sad_mlp_packed_bytes_bf16(int L, const int *dims, int first_has_xyz);
int sad_mlp_pack_bf16(int L, const int *dims, int first_has_xyz, const float *const *W,
                      const float *const *bias, void *packed, sad_stream_t stream);
typedef struct sad_mlp_bf16_args {
    size_t struct_size;   /* = sizeof(sad_mlp_bf16_args) */
    const float *xyz;     /* [B,N,3] f32                               (grouped mode) */
    const float *new_xyz; /* [B,M,3] f32                               (grouped mode) */
    const int32_t *idx;   /* [B,M,S] or NULL (plain mode)                             */
    const void *feat;     /* grouped: point-major [B,N,C]; plain: rows [B*M, C]        */
    int feat_bf16;
    int ld_feat;
    int B, N, M, S, C;
    int L;
    int dims[SAD_MAX_LAYERS + 1];
    const void *packed;
    int relu_mask;
    void *out;
    int out_bf16;
    int ld_out;
    int col_off;
    /* optional, grouped mode: cnt[B,M] from the ball query + sad_mlp_workspace_bytes(B,M,S) bytes of
     * 16-byte aligned scratch -> only the leading cnt rows of each group are computed (rows that
     * repeat the first neighbour cannot change the max); both NULL = dense rows */
    const int32_t *cnt;
    void *workspace;
    /* 0 = built-in choice (128 rows per tile, fewer if LDS demands); else rows per tile 32/64/128/256
     * (more rows amortise the per-tile gather latency of narrow chains; SAD_EUNSUPPORTED if LDS is short);
     * 2 = register-resident chain (grouped 3-layer chains with cnt + workspace whose shape is compiled: the SA stages
     *     and the cluster layer of the KITTI / nuScenes / TINY topologies and configs[0]; 16-byte bf16 feature rows,
     *     or at most 13 feature channels of either type): one wave carries a 32-row tile through the chain in
     *     registers, weights through an LDS ring, pooled rows staged in LDS and stored once per group;
     * 3 = row-streaming layer (plain single layers: C % 8 == 0, 16-byte aligned rows; also what 0 picks for them):
     *     every input row is read once per 128 output channels, weights shared through LDS */
    int geometry;
    /* != 0: `workspace` already holds the row-packing table of (cnt, idx) from sad_mlp_rowscan (geometry 2 only) */
    int prescanned;
    /* Split pooling (ABI 4; grouped mode, geometry 2, out_bf16 = 1): the pooled rows leave as bf16 with PLAIN stores and nothing
     * needs a zero fill.  A group whose packed rows lie in several 32-row tiles (about one in eight) is not combined in memory:
     * its rows in the tile where they begin pool into out[g], its rows in a later tile t into row t of `cont`
     * (sad_mlp_cont_bytes() bytes, 16-byte aligned, row stride = dims[3] elements; row 0 is all zero).  The true pooled row is
     * the element-wise maximum of the two or three — taken by the layer that reads them: a plain-mode call with n_pool > 0.
     * Exact: rounding to bf16 is monotone, so max(bf16(a), bf16(b)) = bf16(max(a, b)), and every consumer of pooled rows
     * rounds them to bf16 on load.  Needs dims[3], ld_out and col_off multiples of 8, `out` 16-byte aligned, and a table made
     * by this call's own scan (prescanned = 0) or by sad_mlp_rowscan_split. */
    void *cont;
    /* plain mode, one layer (geometry 0 / 3), feat_bf16 = 1: the input rows are the split-pooled outputs of n_pool chains side
     * by side — columns of width pool_cols[i] (multiples of 16, adding up to C) pooled by the chain with nsample pool_S[i],
     * row-packing table pool_ws[i] and continuation rows pool_cont[i]; B * M = the chains' groups.  0 = ordinary rows. */
    int n_pool;
    const void *pool_ws[SAD_MAX_RADII];
    const void *pool_cont[SAD_MAX_RADII];
    int pool_S[SAD_MAX_RADII];
    int pool_cols[SAD_MAX_RADII];
} sad_mlp_bf16_args;
/* bytes of the continuation-row buffer of a split-pooled chain with B * M groups of at most S rows and cout output channels */
size_t sad_mlp_cont_bytes(int B, int M, int S, int cout);
/* sad_mlp_rowscan for chains whose pooled output is split (sad_mlp_bf16_args.cont): also marks the continuation rows in the row
 * map, records the first packed row of every group behind it and zeroes row 0 of cont[i] (cout[i] = the chain's output channels). */
int sad_mlp_rowscan_split(int n, const int32_t *const *cnt, const int32_t *const *idx, const int *S, int B, int N,
                          int M, void *const *workspace, void *const *cont, const int *cout, sad_stream_t stream);
/* 2 when sad_mlp_chain_bf16 has a register-resident kernel for this grouped chain (dims[0] = C + 3), else 0 */
int sad_mlp_preferred_geometry_bf16(int L, const int *dims);
int sad_mlp_chain_bf16(const sad_mlp_bf16_args *args, sad_stream_t stream);
/* n independent bf16 chains in one dispatch (see sad_mlp_chain_multi_f32). */
int sad_mlp_chain_multi_bf16(const sad_mlp_bf16_args *const *args, int n, sad_stream_t stream);

/* SPEC.md §8 steps 2-4.  xyz3[B,M3,3], c[B,K,6] -> cand[B,K,3], radius[B,K]; anchor[3] host. */
int sad_candidates_f32(const float *xyz3, const float *c, int B, int M3, int K, float shift_max,
                       float r_min, float r_max, const float *anchor, float *cand, float *radius,
                       sad_stream_t stream);
/* SPEC.md §33.1: the backward of sad_candidates_f32 with respect to c.  c[B,K,6], grad_cand[B,K,3] -> grad_c[B,K,6]:
 * grad_c[.., d] = grad_cand[.., d] where -shift_max <= c[.., d] <= shift_max (bounds included; a selection, a NaN c gives +0),
 * else +0; grad_c[.., 3 + d] = +0 (the size columns feed the radius of an index decision only).  One launch, every element
 * written, no workspace, bit-equal from call to call.  shift_max negative or NaN: SAD_EINVAL; B > 65535: SAD_EUNSUPPORTED. */
int sad_candidates_grad_f32(const float *c, const float *grad_cand, int B, int K, float shift_max, float *grad_c,
                            sad_stream_t stream);
/* SPEC.md §33.2: the backward of a packed prefix copy (rows [0, K) of every scene).  g[B,K,C] -> out[B,M,C]: rows < K are g's,
 * rows K .. M-1 are +0; one launch, every element of out written exactly once.  1 <= K <= M. */
int sad_prefix_rows_grad_f32(const float *g, int B, int K, int M, int C, float *out, sad_stream_t stream);
/* SPEC.md §9.  cand[B,K,3], o[B,K,10] -> boxes[B,K,9]; anchors[9] host (3 classes x lwh). */
int sad_decode_boxes_f32(const float *cand, const float *o, int B, int K, const float *anchors,
                         float *boxes, sad_stream_t stream);

/* SPEC.md §13.  Rotated-box NMS in bird's-eye view, one scene per workgroup.
 * boxes[B,K,9] (x,y,z,l,w,h,yaw,score,label), K <= 512 -> keep[B,K] (0/1), order[B,K] (kept indices
 * in rank order, -1 padded), count[B]. */
int sad_nms_bev_f32(const float *boxes, int B, int K, float iou_thr, float score_thr, int32_t *keep,
                    int32_t *order, int32_t *count, sad_stream_t stream);
/* Same result with sad_nms_bev_workspace_bytes(B,K) bytes of 16-byte aligned scratch: the K x K
 * suppression matrix is computed by B*K waves spread over the chip instead of one workgroup per scene. */
size_t sad_nms_bev_workspace_bytes(int B, int K);
int sad_nms_bev_ws_f32(const float *boxes, int B, int K, float iou_thr, float score_thr, int32_t *keep,
                       int32_t *order, int32_t *count, void *workspace, sad_stream_t stream);

/* SPEC.md §23.  Box selection and rotated-box NMS at scale: any K, scores (and labels) in their own tensors.
 * boxes[B,K,D] (D >= 7; only cx,cy,cz,l,w,h,yaw are read), scores[B,K], labels[B,K] or NULL (NULL = class-agnostic; any
 * int32 is a class) -> keep[B,K] (0/1), order[B,P] (kept indices in rank order, -1 padded), count[B].
 * Candidates (score >= score_thr) are ranked by (score desc, index asc), the best pre_max go on, the greedy walk of §13
 * suppresses within a class only and stops after post_max kept boxes.  pre_max / post_max <= 0 are invalid (SAD_EINVAL):
 * pass K for "no limit".  Shape rule: order has P = min(K, pre_max, post_max) columns.  Limits: 1 <= B <= 65535,
 * B*K < 2^31, min(K, pre_max) <= 16384 (SAD_EUNSUPPORTED above; workspace_bytes then returns 0).
 * Workspace law: sad_nms_boxes_workspace_bytes(B, K, pre_max) bytes, 16-byte aligned, contents irrelevant before and
 * after the call: per scene, with P' = min(K, pre_max), 64 + 60 P' + 8 P' ceil(P'/64) bytes rounded up to 16 (the
 * suppression matrix is P' x ceil(P'/64) words; 8 P' of it are the centres the pair test subtracts, SPEC.md §13: always
 * ask the function, the law has grown before).  keep, order and count are fully written by the call.  Four launches
 * whose dimensions depend on (B, K, pre_max) only; nothing is read back and nothing synchronises. */
size_t sad_nms_boxes_workspace_bytes(int B, int K, int pre_max);
int sad_nms_boxes_f32(const float *boxes, int D, const float *scores, const int32_t *labels, int B, int K,
                      float iou_thr, float score_thr, int pre_max, int post_max, int32_t *keep, int32_t *order,
                      int32_t *count, void *workspace, sad_stream_t stream);

/* SPEC.md §25.  Dense head decode: the raw maps of a BEV head -> boxes[B,K,D], scores[B,K], labels[B,K], the inputs of
 * sad_nms_boxes_f32.  Inference only.  Maps are contiguous f32 in the layout named by `layout` and are read where they are:
 * SAD_LAYOUT_NCHW [B, channels, H, W] or SAD_LAYOUT_NHWC [B, H, W, channels], the same channel numbering in both.
 * With index[B,P] (int32, may be NULL) only the rows k = index[b,p] are decoded and the outputs are [B,P,...]: an entry
 * outside [0, K) gives a zero box, score -inf and label -1; duplicates are allowed.  Outputs are fully written by the call.
 * One launch whose dimensions depend on the shapes only; nothing is read back and nothing synchronises.
 * Common limits: 1 <= B <= 65535, 1 <= C <= 64, B*K < 2^31, B*P < 2^31 (SAD_EUNSUPPORTED above); a NULL pointer, a wrong
 * struct_size, a size below 1 or another layout code: SAD_EINVAL.  NaN in a map is undefined behaviour. */
#define SAD_LAYOUT_NCHW 0
#define SAD_LAYOUT_NHWC 1

/* §25.1 anchor head (SECOND, PointPillars, PV-RCNN's RPN).  A = ns * nr anchors per cell, a = s * nr + r (sizes outer);
 * K = H*W*A, k = (y*W + x)*A + a.  cls has A*C channels (a*C + c), reg A*7 (a*7 + j), dir A*nb (a*nb + d); dir == NULL
 * iff nb == 0, else 2 <= nb <= 8.  1 <= ns <= 16, 1 <= nr <= 8 (SAD_EUNSUPPORTED above).  The anchor of (y, x, s, r) is
 * (x0 + x*sx, y0 + y*sy, z_center[s], sizes[3s .. 3s+2] = (l, w, h), rotations[r]); no anchor tensor is read.
 * boxes[.,7] = (cx, cy, cz, l, w, h, yaw): ResidualCoder.decode, then the direction bin with period 2*pi/nb when dir is
 * given; score = sigmoid(max class logit), label = the lowest class that attains it. */
typedef struct sad_anchor_decode_args {
    size_t struct_size;   /* = sizeof(sad_anchor_decode_args) */
    const float *cls, *reg, *dir;
    const int32_t *index; /* [B,P] or NULL */
    int B, H, W, C, nb, ns, nr, layout, P;
    float sizes[48];      /* [ns,3] (l, w, h) */
    float z_center[16];   /* [ns] */
    float rotations[8];   /* [nr] */
    float x0, y0, sx, sy; /* centre of cell (0, 0) and the step between cell centres */
    float dir_offset, dir_limit_offset;
    float *boxes;         /* [B,K,7] or [B,P,7] */
    float *scores;        /* [B,K] or [B,P] */
    int32_t *labels;      /* [B,K] or [B,P] */
} sad_anchor_decode_args;
int sad_anchor_decode_f32(const sad_anchor_decode_args *args, sad_stream_t stream);

/* §25.2 centre head (CenterPoint, one task per call).  hm[B,C,H,W], reg[.,2,.,.], height[.,1,.,.], dim[.,3,.,.],
 * rot[.,2,.,.] (sine, cosine), vel[.,2,.,.] or NULL; K = H*W, k = y*W + x.  boxes[.,D], D = 9 with vel (columns 7, 8 = vel)
 * else 7: cx = (x + reg0)*sx + lo_x, cy likewise, cz = height, (l, w, h) = exp(dim) if log_dim else dim, yaw =
 * atan2(rot0, rot1).  score / label as in §25.1 over the C heat-map channels; with peak != 0 only the classes whose logit
 * is >= its (up to 8) in-image neighbours take part, and a cell where none does gets score 0 and label -1. */
typedef struct sad_center_decode_args {
    size_t struct_size;   /* = sizeof(sad_center_decode_args) */
    const float *hm, *reg, *height, *dim, *rot, *vel;
    const int32_t *index; /* [B,P] or NULL */
    int B, H, W, C, layout, P, log_dim, peak;
    float lo_x, lo_y, sx, sy;
    float *boxes, *scores;
    int32_t *labels;
} sad_center_decode_args;
int sad_center_decode_f32(const sad_center_decode_args *args, sad_stream_t stream);

/* SPEC.md §26.  Dense head target assignment: ground-truth boxes -> what a dense head is trained against; the inverse of
 * §25 with the same anchor scalars, K, k numbering and layouts.  No gradients.  gt_boxes[B,G,D] f32 (D >= 7, rows
 * (cx,cy,cz,l,w,h,yaw,...)), gt_labels[B,G] int32 (0-based classes; a negative label marks a padding row).
 * 0 <= G <= 1024 (SAD_EUNSUPPORTED above); with G == 0 the two pointers may be NULL.  Outputs are fully written by the
 * call.  A fixed sequence of launches whose dimensions depend on the shapes only; nothing is read back, nothing
 * synchronises, and two calls are bit-equal.  NaN in gt_boxes is undefined behaviour. */

/* §26.1 anchor head targets: the per-class (size_class) or class-agnostic max-IoU assigner of SECOND / PointPillars on
 * the nearest-BEV (axis-aligned) IoU, anchors generated from the scalars below as in §25.1 (no anchor tensor, no [K,G]
 * matrix).  labels[B,K]: class of the matched box for a positive, -1 background, -2 ignored; match[B,K]: the matched g or
 * -1; reg_target[B,K,7]: ResidualCoder.encode for a positive, else 0; max_iou[B,K]; dir_target[B,K] (NULL iff nb == 0,
 * else 2 <= nb <= 8): the direction bin of a positive, else -1.  1 <= ns <= 16, 1 <= nr <= 8, B <= 65535, B*K < 2^31
 * (SAD_EUNSUPPORTED above); an anchor size <= 0: SAD_EINVAL.  workspace: sad_anchor_targets_workspace_bytes(B, G) bytes
 * (0: may be NULL), zeroed by the call itself. */
typedef struct sad_anchor_targets_args {
    size_t struct_size;   /* = sizeof(sad_anchor_targets_args) */
    const float *gt_boxes;
    const int32_t *gt_labels;
    int B, G, D, H, W, ns, nr, nb;
    int use_size_class;   /* 0: every size takes every class (size_class is not read) */
    float sizes[48];      /* [ns,3] (l, w, h) */
    float z_center[16];   /* [ns] */
    float rotations[8];   /* [nr] */
    float pos_thr[16], neg_thr[16]; /* [ns] */
    int32_t size_class[16];         /* [ns]: the class size s is matched against */
    float x0, y0, sx, sy; /* centre of cell (0, 0) and the step between cell centres */
    float dir_offset;
    int32_t *labels, *match;
    float *reg_target, *max_iou;
    int32_t *dir_target;
    void *workspace;
} sad_anchor_targets_args;
size_t sad_anchor_targets_workspace_bytes(int B, int G);   /* 4*B*G; 0 outside B >= 1, 0 <= G <= 1024 */
int sad_anchor_targets_f32(const sad_anchor_targets_args *args, sad_stream_t stream);

/* §26.2 centre head targets (CenterPoint, one task per call).  A label outside [0, C) is padding.  heatmap[B,C,H,W]
 * (SAD_LAYOUT_NHWC: [B,H,W,C]): the maximum over the boxes of a class of the CenterNet Gaussian drawn around the box's
 * cell, 0 where no box reaches; ind[B,G]: iy*W + ix of an assigned box, else -1; anno[B,G,8 (vel: 10)] =
 * (fx - ix, fy - iy, cz, log l, log w, log h, sin yaw, cos yaw[, vx, vy]), zero for an unassigned box.  A box whose
 * centre lies outside the map is unassigned (not clamped onto the border).  1 <= C <= 64, B <= 65535, B*H*W < 2^31
 * (SAD_EUNSUPPORTED above); sx, sy > 0, 0 < min_overlap < 1, 0 <= min_radius <= 64, vel needs D >= 9 (SAD_EINVAL). */
typedef struct sad_center_targets_args {
    size_t struct_size;   /* = sizeof(sad_center_targets_args) */
    const float *gt_boxes;
    const int32_t *gt_labels;
    int B, G, D, C, H, W, layout, min_radius, vel;
    float lo_x, lo_y, sx, sy, min_overlap;
    float *heatmap;
    int32_t *ind;
    float *anno;
} sad_center_targets_args;
int sad_center_targets_f32(const sad_center_targets_args *args, sad_stream_t stream);

/* SPEC.md §27.  Dense head losses: the maps of a dense head and the targets of §26 -> per-scene losses and the gradient with
 * respect to every map, written in the map's own layout (no permuted copy); K, the k numbering, the channel numbering and
 * the layouts are §25's.  Component i of scene b is weighted by wq_i = scale[i] / (float)max(n_b, 1) (normalize != 0) or
 * scale[i] (normalize == 0): scenes are independent; a batch-wide normaliser is normalize = 0 and a division by the caller.
 * Outputs are fully written by the call.  A fixed sequence of memsets and launches whose dimensions depend on the shapes
 * only; nothing is read back, nothing synchronises, no float atomics: two calls are bit-equal.  NaN in an input is
 * undefined behaviour.  Limits: 1 <= B <= 65535, 1 <= C <= 64, A <= 128, nb 0 or 2 .. 8, G <= 1024, B*K < 2^31
 * (SAD_EUNSUPPORTED above); a NULL pointer, a wrong struct_size, beta <= 0, alpha outside [0, 1], another layout code, dir
 * without nb or the reverse: SAD_EINVAL. */

/* §27.1 anchor head: sigmoid focal classification (gamma = 2) over the rows with labels != -2, smooth-L1 regression with
 * the sine-difference yaw (sin_diff != 0) and softmax cross-entropy over the nb direction bins, both over the positives
 * (labels >= 0); num_pos[b] = the scene's positives.  labels / reg_target / dir_target are §26.1's.  dir, dir_target and
 * grad_dir are NULL iff nb == 0 (loss[.,2] = 0).  per_anchor[B,K,3] (may be NULL): the row's terms per component.
 * workspace: sad_anchor_head_loss_workspace_bytes(B, H, W, A) bytes (the workgroups' partial sums), contents irrelevant. */
typedef struct sad_anchor_head_loss_args {
    size_t struct_size;   /* = sizeof(sad_anchor_head_loss_args) */
    const float *cls, *reg, *dir;  /* maps: A*C, A*7, A*nb channels */
    const int32_t *labels;         /* [B,K] */
    const float *reg_target;       /* [B,K,7] */
    const int32_t *dir_target;     /* [B,K] */
    int B, H, W, A, C, nb, layout, sin_diff, normalize;
    float alpha, beta;
    float code_weights[7];
    float scale[3];       /* cls, reg, dir */
    float *loss;          /* [B,3] */
    int32_t *num_pos;     /* [B] */
    float *grad_cls, *grad_reg, *grad_dir; /* shapes and layout of the maps */
    float *per_anchor;
    void *workspace;
} sad_anchor_head_loss_args;
size_t sad_anchor_head_loss_workspace_bytes(int B, int H, int W, int A);   /* 12*B*ceil(H*W/64)*ceil(A/8); 0 outside the limits */
int sad_anchor_head_loss_f32(const sad_anchor_head_loss_args *args, sad_stream_t stream);

/* §27.2 centre head (CenterPoint, one task per call): CenterNet's penalty-reduced focal loss of the clamped sigmoid of hm
 * against heatmap (same layout), and L1 of the regression maps at the cells ind[B,G] against anno[B,G,8 (vel: 10)], the
 * outputs of §26.2.  num_pos[B,2] = (cells with heatmap == 1, boxes with 0 <= ind < H*W): the two normalisers.  The
 * regression gradients are zero outside the boxes' cells; boxes that share a cell add up in ascending g.  vel and grad_vel
 * are NULL together.  With G == 0 ind and anno may be NULL.  workspace: sad_center_head_loss_workspace_bytes(B, H, W, G). */
typedef struct sad_center_head_loss_args {
    size_t struct_size;   /* = sizeof(sad_center_head_loss_args) */
    const float *hm, *reg, *height, *dim, *rot, *vel;
    const float *heatmap;
    const int32_t *ind;
    const float *anno;
    int B, H, W, C, G, layout, normalize;
    float code_weights[10];
    float scale[2];       /* hm, reg */
    float *loss;          /* [B,2] */
    int32_t *num_pos;     /* [B,2] */
    float *grad_hm, *grad_reg, *grad_height, *grad_dim, *grad_rot, *grad_vel;
    void *workspace;
} sad_center_head_loss_args;
size_t sad_center_head_loss_workspace_bytes(int B, int H, int W, int G);   /* 4*B*(ceil(H*W/256) + ceil(G/256)); 0 outside the limits */
int sad_center_head_loss_f32(const sad_center_head_loss_args *args, sad_stream_t stream);

/* SPEC.md §28.  RoI head: which of the nms_boxes survivors a second stage trains on, their matched ground truth in the
 * RoI's frame, and the residual code with its inverse.  Box rows and padded ground truth as in §19 / §26 (a negative
 * label marks a padding row, 0 <= G <= 1024, G == 0 with NULL pointers).  No gradients.  Outputs are fully written by
 * the call.  A fixed sequence of launches whose dimensions depend on the shapes only; nothing is read back, nothing
 * synchronises, no float atomics: two calls are bit-equal.  NaN in an input or |yaw| >= 1e4 is undefined behaviour. */
#define SAD_ROI_CLS_ROI_IOU 0
#define SAD_ROI_CLS_CLS 1

/* §28.1 proposal sampling and targets.  rois[B,R,D] (D >= 7); roi_count[B] or NULL (the candidates of scene b are rows
 * r < clamp(roi_count[b], 0, R), rows beyond are never read); roi_labels[B,R] or NULL (not NULL: a RoI is matched against
 * the boxes of its own class only).  m(r) = the largest §19.3 3-D IoU over the eligible boxes, j(r) = the lowest box that
 * attains it (-1 without one).  fg: m >= fg_thr; hard: bg_lo <= m < fg_thr; easy: m < bg_lo.  Of the S slots the first
 * min(fg_max, n_fg, S) hold the fg candidates with the smallest (h(b, r), r), the others draw with replacement from hard
 * (floor((S - nf) * hard_ratio) of them, at most n_hard) and easy by h(b, 0x80000000 + i) mod the class count, h = the hash
 * of sad_subsample_pad_f32 under `seed`.  Per slot: index (the RoI's row), match (j), labels, iou (m), cls_target (1 above
 * cls_fg_thr, 0 below cls_bg_thr, between them (m - cls_bg_thr) / (cls_fg_thr - cls_bg_thr) or, SAD_ROI_CLS_CLS, -1),
 * reg_valid (j >= 0 and m > reg_fg_thr), rois_s[.,7], gt_local[.,7] (the box in the RoI's frame, heading in [-pi/2, pi/2])
 * and reg_target[.,7] (residuals against the RoI's extents); a scene without candidates gives (-1, -1, -1, 0, -1, 0, 0...).
 * 1 <= B <= 65535, 1 <= R <= 4096, 1 <= S <= 1024 (SAD_EUNSUPPORTED above); need 0 <= bg_lo <= fg_thr, fg_thr > 0,
 * cls_bg_thr < cls_fg_thr, 0 <= hard_ratio <= 1, fg_max >= 0 (SAD_EINVAL).  workspace: sad_roi_targets_workspace_bytes(B, R)
 * bytes ((m, j) per RoI), contents irrelevant. */
typedef struct sad_roi_targets_args {
    size_t struct_size;   /* = sizeof(sad_roi_targets_args) */
    const float *rois;
    const int32_t *roi_count, *roi_labels;
    const float *gt_boxes;
    const int32_t *gt_labels;
    int B, R, D, G, Dg, S, fg_max, cls_mode;
    unsigned seed;
    float fg_thr, bg_lo, hard_ratio, reg_fg_thr, cls_fg_thr, cls_bg_thr;
    int32_t *index, *match, *labels;   /* [B,S] */
    float *iou, *cls_target;           /* [B,S] */
    int32_t *reg_valid;                /* [B,S] */
    float *rois_s, *gt_local, *reg_target; /* [B,S,7] */
    void *workspace;
} sad_roi_targets_args;
size_t sad_roi_targets_workspace_bytes(int B, int R);   /* 8*B*R; 0 outside 1 <= B <= 65535, 1 <= R <= 4096 */
int sad_roi_targets_f32(const sad_roi_targets_args *args, sad_stream_t stream);

/* §28.2 the inverse of §28.1's code: rois[B,S,D] (D >= 7), reg[B,S,7] -> boxes[B,S,7].  One launch.  B*S < 2^31. */
int sad_roi_decode_f32(const float *rois, int D, const float *reg, int B, int S, float *boxes, sad_stream_t stream);

/* SPEC.md §29.  RoI head loss on §28.1's targets, read where they are, with the gradient with respect to both predictions:
 * binary cross-entropy of the logit rcnn_cls against the soft target cls_target over the rows with cls_target >= 0 (-1: the
 * ignored band and the empty slot), smooth-L1 of rcnn_reg against reg_target and, with rois and gt_local (both or neither),
 * the corner loss of the decoded box against gt_local in the RoI's frame, both over the rows with reg_valid != 0.
 * num[B,2] = (n_cls, n_reg); component i is weighted scale[i] / (float)max(n, 1) (n = n_cls for i = 0, n_reg for i = 1, 2)
 * or, normalize == 0, scale[i]: the normaliser is per scene.  rois[B,S,D] (D >= 7): columns 3..5 are read at row stride D.
 * grad_corner is given iff the corner component is on (without it loss[.,2] = 0); per_roi[B,S,3] may be NULL.  What
 * reg_target, gt_local or rois hold in a row with reg_valid == 0 never reaches a result.  One launch, one workgroup per scene,
 * no workspace, no memset, no atomics; outputs are fully written; nothing is read back, nothing synchronises; two calls are
 * bit-equal.  |rcnn_reg[.,6]| >= 1e4 is undefined behaviour.  1 <= B <= 65535, 1 <= S <= 1024 (SAD_EUNSUPPORTED above); a
 * NULL required pointer, a wrong struct_size, a size below 1, D < 7, beta <= 0 or NaN, rois without gt_local or the reverse,
 * grad_corner given or missing against them: SAD_EINVAL. */
typedef struct sad_roi_head_loss_args {
    size_t struct_size;   /* = sizeof(sad_roi_head_loss_args) */
    const float *rcnn_cls;         /* [B,S] */
    const float *rcnn_reg;         /* [B,S,7] */
    const float *cls_target;       /* [B,S] */
    const int32_t *reg_valid;      /* [B,S] */
    const float *reg_target;       /* [B,S,7] */
    const float *rois;             /* [B,S,D] or NULL */
    const float *gt_local;         /* [B,S,7] or NULL */
    int B, S, D, normalize;
    float beta;
    float code_weights[7];
    float scale[3];       /* cls, reg, corner */
    float *loss;          /* [B,3] */
    int32_t *num;         /* [B,2] */
    float *grad_cls;      /* [B,S] */
    float *grad_reg;      /* [B,S,7] */
    float *grad_corner;   /* [B,S,7] or NULL */
    float *per_roi;       /* [B,S,3] or NULL */
} sad_roi_head_loss_args;
int sad_roi_head_loss_f32(const sad_roi_head_loss_args *args, sad_stream_t stream);

/* SPEC.md §30.  Voxel RoI pooling, the index side: the grid points of the RoIs and the ordered voxel neighbourhood of every query
 * point at one backbone scale.  No gradients.  Outputs are fully written by the call.  A fixed sequence of launches whose dimensions
 * depend on the shapes only; nothing is read back, nothing synchronises, no atomics on an output: two calls are bit-equal. */

/* rois[B,R,D] (D >= 7, rows (cx,cy,cz,l,w,h,yaw,...)), roi_count[B] or NULL (as §28.1: rows r >= clamp(roi_count[b], 0, R) are never
 * read) -> pts[B,R,G^3,3]: grid point g = (ix*G + iy)*G + iz at ((i + 0.5) / G - 0.5) * extent per axis in the RoI's frame, rotated
 * and moved as in §28.2; quiet NaN for the rows beyond roi_count (an empty query of sad_voxel_query_f32).  One launch.
 * 1 <= G <= 16, B <= 65535, B*R*G^3 < 2^31 (SAD_EUNSUPPORTED above); a NULL required pointer, a wrong struct_size, a size below 1,
 * D < 7: SAD_EINVAL. */
typedef struct sad_roi_grid_points_args {
    size_t struct_size;   /* = sizeof(sad_roi_grid_points_args) */
    const float *rois;
    const int32_t *roi_count;
    int B, R, D, G;
    float *pts;
} sad_roi_grid_points_args;
int sad_roi_grid_points_f32(const sad_roi_grid_points_args *args, sad_stream_t stream);

/* coors[Nv,3] (z,y,x) / offsets[B+1] / spatial_shape (Gz,Gy,Gx): a §21 sparse tensor; voxel_size (vx,vy,vz): that scale's; lo
 * (x0,y0,z0): the low corner of the point range; new_xyz[B,M,3] -> idx[B,M,S] (global rows in [0,Nv)), cnt[B,M].  The cell of a
 * query is §20.1's; its candidates are the cells within max_range (rz,ry,rx) of it, walked dz slowest, dx fastest, ascending; a
 * candidate counts if it is inside the grid, the query's scene holds a voxel there (the lowest row of a duplicated coordinate) and
 * d2(voxel centre (§24), query) < radius^2, strict.  The first S fill idx in walk order, the rest repeat the first; cnt =
 * min(accepted, S); a query whose cell is not finite or beyond 2^30 (NaN, Inf) is empty: cnt 0, idx 0.  Nv == 0 and M == 0 are valid
 * (coors / new_xyz, idx, cnt may then be NULL).  workspace: sad_voxel_query_workspace_bytes(Nv) bytes (the coordinate table: a power of two >= 2 Nv
 * slots, 8 + 4 bytes each), 16-byte aligned, contents irrelevant.  Three launches.
 * 0 <= max_range <= 8, 1 <= S <= 128, B <= 65535, B*M*S < 2^31, Nv <= 2^30, Gz*Gy*Gx <= 2^31 - 1 (SAD_EUNSUPPORTED above); a NULL
 * required pointer, a wrong struct_size, B or S below 1, a negative size or range, voxel_size <= 0, radius <= 0 or NaN: SAD_EINVAL. */
typedef struct sad_voxel_query_args {
    size_t struct_size;   /* = sizeof(sad_voxel_query_args) */
    const int32_t *coors, *offsets;
    const float *new_xyz;
    int Nv, B, M, S;
    int spatial_shape[3]; /* (Gz,Gy,Gx) */
    int max_range[3];     /* (rz,ry,rx) */
    float voxel_size[3];  /* (vx,vy,vz) */
    float lo[3];          /* (x0,y0,z0) */
    float radius;
    int32_t *idx;         /* [B,M,S] */
    int32_t *cnt;         /* [B,M] */
    void *workspace;
} sad_voxel_query_args;
size_t sad_voxel_query_workspace_bytes(int Nv);   /* 0 outside 0 <= Nv <= 2^30 */
int sad_voxel_query_f32(const sad_voxel_query_args *args, sad_stream_t stream);

/* SPEC.md §31.  Point head: what the size-adaptive cluster layer (§8, c[B,M,6]) and the box / class head (§9, o[B,M,C+7]) are
 * trained against, and the loss on top with its gradients.  Rows are point-major, M points per scene (the detector: M = K).
 * Padded ground truth as in §26 (a label outside [0, C) or a non-positive extent marks a padding row, 0 <= G <= 1024, G == 0
 * with NULL pointers).  Outputs are fully written by the call.  A fixed sequence of memsets and launches whose dimensions
 * depend on the shapes only; nothing is read back, nothing synchronises, no float atomics: two calls are bit-equal.  NaN in an
 * input or |yaw| >= 1e4 is undefined behaviour.  1 <= B <= 65535, 1 <= C <= 16, B*M < 2^31 (SAD_EUNSUPPORTED above). */

/* §31.1 targets.  A point is assigned by its origin xyz[B,M,3]: match = the lowest g with §19.1 inside(xyz, box_g, 0), labels =
 * that box's class; inside no box but inside some box enlarged by extra_width: labels -2 (ignored); else -1 (background).
 * cand[B,M,3] (NULL: xyz) is where the head predicts from: centerness (the cube root of the product of min/max of the
 * distances to the two faces per axis, in the box's frame; 0 outside the box) and reg_target[.,7] (centre - cand,
 * clamp(log(size / anchors[class]), +-2), yaw: §9's code inverted) are taken there; shift_target[.,3] =
 * clamp(centre - xyz, +-shift_max) and size_target[.,3] = min(sqrt(max(2 size / size_anchor - 1, 0)) - 1, 1) invert §8 steps 2
 * and 3.  Non-positive rows: match -1, centerness 0, zero targets.  One launch, no workspace, no atomics.  A NULL required
 * pointer, a wrong struct_size, a size below 1, D < 7, an anchor <= 0, shift_max < 0 or extra_width < 0: SAD_EINVAL. */
typedef struct sad_point_targets_args {
    size_t struct_size;   /* = sizeof(sad_point_targets_args) */
    const float *xyz;              /* [B,M,3] */
    const float *cand;             /* [B,M,3] or NULL */
    const float *gt_boxes;         /* [B,G,D] */
    const int32_t *gt_labels;      /* [B,G] */
    int B, M, G, D, C;
    float anchors[48];    /* [C,3] */
    float size_anchor[3];
    float shift_max, extra_width;
    int32_t *labels, *match;       /* [B,M] */
    float *centerness;             /* [B,M] */
    float *shift_target, *size_target; /* [B,M,3] */
    float *reg_target;             /* [B,M,7] */
} sad_point_targets_args;
int sad_point_targets_f32(const sad_point_targets_args *args, sad_stream_t stream);

/* §31.2 loss on §31.1's targets, read where they are, with the gradient with respect to o and c.  Component i of scene b is
 * weighted scale[i] / (float)max(num_pos[b], 1) (normalize != 0) or scale[i]; num_pos[b] = #(labels >= 0).  Classification
 * over the rows with labels != -2 and every class channel: SAD_POINT_CLS_BCE, §29's binary cross-entropy against the soft
 * target centerness (NULL: 1) at the label's channel of a positive row and 0 elsewhere, or SAD_POINT_CLS_FOCAL, §27.1's sigmoid
 * focal loss on the hard target.  Box regression over the positives: §27.1's smooth-L1 with the sine-difference yaw of
 * o[C .. C+6] (columns 3..5 clamped to +-2 first; the gradient passes where -2 <= x <= 2) against reg_target.  Shift / size
 * (present iff c and shift_target / size_target are given): smooth-L1 of clamp(c[0:3], +-shift_max) / clamp(c[3:6], +-1) over
 * the positives, same gradient rule.  loss[B,4] = (cls, reg, shift, size); grad_o[B,M,C+7]: d loss[.,0] in the first C
 * columns, d loss[.,1] in the last 7; grad_c[B,M,6] (given iff c is): d loss[.,2] in columns 0..2, d loss[.,3] in 3..5;
 * per_point[B,M,4] may be NULL.  workspace: sad_point_head_loss_workspace_bytes(B, M) bytes (the workgroups' partial sums),
 * contents irrelevant.  A NULL required pointer, a wrong struct_size, a size below 1, beta <= 0 or NaN, alpha outside [0, 1],
 * another cls_loss code, c without a target or a target without c, grad_c given or missing against c: SAD_EINVAL. */
#define SAD_POINT_CLS_BCE 0
#define SAD_POINT_CLS_FOCAL 1
typedef struct sad_point_head_loss_args {
    size_t struct_size;   /* = sizeof(sad_point_head_loss_args) */
    const float *o;                /* [B,M,C+7] */
    const float *c;                /* [B,M,6] or NULL */
    const int32_t *labels;         /* [B,M] */
    const float *centerness;       /* [B,M] or NULL */
    const float *reg_target;       /* [B,M,7] */
    const float *shift_target;     /* [B,M,3] or NULL */
    const float *size_target;      /* [B,M,3] or NULL */
    int B, M, C, cls_loss, normalize;
    float alpha, beta, shift_max;
    float code_weights[7];
    float scale[4];       /* cls, reg, shift, size */
    float *loss;          /* [B,4] */
    int32_t *num_pos;     /* [B] */
    float *grad_o;        /* [B,M,C+7] */
    float *grad_c;        /* [B,M,6] or NULL */
    float *per_point;     /* [B,M,4] or NULL */
    void *workspace;
} sad_point_head_loss_args;
size_t sad_point_head_loss_workspace_bytes(int B, int M);   /* 16*B*ceil(M/256); 0 outside the limits */
int sad_point_head_loss_f32(const sad_point_head_loss_args *args, sad_stream_t stream);

/* SPEC.md §32 (backward of the MLP chains; additions of ABI 4 as well).  One entry serves both forms: idx != NULL is the grouped
 * chain + max-pool of §6, idx == NULL plain rows.  The activations are recomputed (§6 is bit-reproducible), so the call needs the
 * forward's inputs, its pooled output (grouped form) and the UNPACKED layers W[l] [dims[l+1], dims[l]] row-major, b[l] [dims[l+1]].
 * grouped: xyz[B,N,3], feat[B,N,C] at row stride ld_feat (NULL iff C == 0), new_xyz[B,M,3], idx[B,M,S], cnt[B,M] or NULL (every
 *   slot is a row), dims[0] = C + 3, relu_mask = all layers; pooled / grad_out: row g = b M + m at g * ld + offset, C_L wide.
 *   skip_empty != 0: groups with cnt == 0 contribute to no gradient (their coordinates may be NaN).
 * plain rows: B = 1, M = R rows, x[R, dims[0]] in feat at row stride ld_feat, C = dims[0], any relu_mask (bit l = ReLU after
 *   layer l, counted from 0), grad_out[R, C_L] likewise; grad_x[R, dims[0]] contiguous goes to grad_feat.
 * need: SAD_GRAD_FEAT | SAD_GRAD_XYZ | SAD_GRAD_NEW_XYZ | SAD_GRAD_PARAMS; what is not asked for is neither computed nor
 *   written, and its pointer may be NULL.  grad_feat[B,N,C], grad_xyz[B,N,3], grad_new_xyz[B,M,3], grad_W[l], grad_b[l] are
 *   OVERWRITTEN.  binary32 sums whose order is not specified (float atomics): two calls may differ in the last bits.
 * workspace: 16-byte aligned, workspace_bytes >= *min_bytes of sad_mlp_grad_workspace_bytes; the groups (rows) are processed in
 *   chunks that fit, *full_bytes holds all of them at once.  Its first int32 is `mismatch` after the call: the (group, channel)
 *   pairs whose pooled value no recomputed row attains; 0 whenever pooled came from sad_mlp_chain_f32 with the same layers.
 * 1 <= L <= SAD_MAX_LAYERS, S <= 64, B * M * S < 2^29 (SAD_EUNSUPPORTED above), every width 1 .. 65536. */
#define SAD_GRAD_FEAT 1
#define SAD_GRAD_XYZ 2
#define SAD_GRAD_NEW_XYZ 4
#define SAD_GRAD_PARAMS 8
typedef struct sad_mlp_grad_args {
    size_t struct_size;   /* = sizeof(sad_mlp_grad_args) */
    const float *xyz;              /* [B,N,3] (grouped) */
    const float *new_xyz;          /* [B,M,3] (grouped) */
    const float *feat;             /* [B,N,C] or NULL; plain rows: x */
    const int32_t *idx;            /* [B,M,S]; NULL = plain rows */
    const int32_t *cnt;            /* [B,M] or NULL */
    int ld_feat;
    int B, N, M, S, C;
    int L;
    int dims[SAD_MAX_LAYERS + 1];
    const float *W[SAD_MAX_LAYERS];
    const float *b[SAD_MAX_LAYERS];
    int relu_mask;
    int skip_empty;
    const float *pooled;           /* grouped: the forward's output */
    int ld_pooled, pooled_off;
    const float *grad_out;
    int ld_grad, col_off;
    int need;
    float *grad_feat;              /* plain rows: grad_x */
    float *grad_xyz;
    float *grad_new_xyz;
    float *grad_W[SAD_MAX_LAYERS];
    float *grad_b[SAD_MAX_LAYERS];
    void *workspace;
    size_t workspace_bytes;
} sad_mlp_grad_args;
int sad_mlp_grad_workspace_bytes(int B, int M, int S, int grouped, int has_cnt, int L, const int *dims, size_t *min_bytes,
                                 size_t *full_bytes);
int sad_mlp_grad_f32(const sad_mlp_grad_args *args, sad_stream_t stream);

/* SPEC.md §34 (additions of ABI 4 as well).  Rotated IoU losses of ALIGNED pairs, pred[i] against target[i], with the analytic
 * gradient with respect to pred.  pred[N,Dp], target[N,Dt]: box rows of D >= 7 floats as in §19 (seven columns are read, row
 * stride D); weight[N] or NULL.  iou[N] = §19.3's IoU of the pair (mode SAD_IOU_BEV / SAD_IOU_3D), equal to the diagonal entry
 * of sad_boxes_iou_f32 bit for bit.  loss[N] = weight * (1 - iou), kind SAD_IOU_LOSS_DIOU adds rho^2 / c^2 (the squared centre
 * distance over the squared diagonal of the box aligned with the TARGET's axes around both footprints; with z and the height
 * intervals in mode 3-D).  grad[N,7] = d loss / d pred (given iff need_grad != 0); the target is a constant.  A row with
 * weight == 0 gives loss = grad = +0 whatever its boxes hold, iou as computed.
 * code SAD_IOU_CODE_ROI: pred is a RoI head's residual rcnn_reg, target is §28.1's gt_local, rois[N,Dr] (columns 3..5 are read)
 * is required; the box is decoded in the RoI's frame as §29's corner loss decodes it, grad is with respect to the residuals and
 * decoded[N,7] (or NULL) receives the box.  With SAD_IOU_CODE_BOX rois and decoded are NULL.
 * One launch, one lane per pair, no workspace, no memset, no atomics; outputs are fully written; nothing is read back, nothing
 * synchronises; two calls are bit-equal.  |yaw| >= 1e4 and a non-finite box in a row of non-zero weight are undefined behaviour.
 * A NULL required pointer, a wrong struct_size, N < 1, D < 7, another mode, kind or code, rois given or missing against code,
 * decoded with SAD_IOU_CODE_BOX, grad given or missing against need_grad: SAD_EINVAL. */
#define SAD_IOU_LOSS_IOU 0
#define SAD_IOU_LOSS_DIOU 1
#define SAD_IOU_CODE_BOX 0
#define SAD_IOU_CODE_ROI 1
typedef struct sad_rotated_iou_loss_args {
    size_t struct_size;   /* = sizeof(sad_rotated_iou_loss_args) */
    const float *pred;             /* [N,Dp] */
    const float *target;           /* [N,Dt] */
    const float *weight;           /* [N] or NULL */
    const float *rois;             /* [N,Dr] or NULL */
    int N, Dp, Dt, Dr;
    int mode, kind, code, need_grad;
    float *loss;          /* [N] */
    float *iou;           /* [N] */
    float *grad;          /* [N,7] or NULL */
    float *decoded;       /* [N,7] or NULL */
} sad_rotated_iou_loss_args;
int sad_rotated_iou_loss_f32(const sad_rotated_iou_loss_args *args, sad_stream_t stream);

/* SPEC.md §35 (additions of ABI 4 as well).  Training augmentation on the device, reproducible from `seed` (the caller mixes its
 * step counter into it): every draw is §17's integer hash h(seed, scene, index) on index ranges of its own.
 *
 * §35.1 sad_global_augment_f32: one flip / rotation / scale / translation per scene, applied to the scene's points and box rows.
 * points[total,Cp] ragged with offsets[B+1], or offsets == NULL: B scenes of N rows each (total = B*N); Cp >= 3, columns 3..
 * are copied.  gt_boxes[B,G,D] rows of D >= 7 floats as in §19 (G >= 0); with_velocity (needs D >= 9) treats columns 7, 8 as a
 * vector: flipped, rotated and scaled, not translated.  Every box row is transformed, padding included; yaw is not wrapped.
 * params[B,8] = (flips, theta, cos, sin, scale, tx, ty, tz), flips = flip_x + 2 * flip_y as a float.  One launch.
 *
 * §35.2 sad_gt_paste_f32: ground-truth database sampling.  The database: db_points[.,Cp], db_offsets[Ndb+1], db_boxes[Ndb,D],
 * entries sorted by class, class c = entries class_offsets[c] .. class_offsets[c+1]-1 (host array, C <= 16 classes).  Q = the sum
 * of sample_num[c] candidate slots per scene (Q <= 512, else SAD_EUNSUPPORTED); a slot is accepted greedily in slot order iff it
 * is active and its BEV IoU with every valid ground-truth row and every accepted earlier slot is not > 0.  Outputs: keep[B,Q],
 * db_index[B,Q] (-1 = inactive), boxes_out[B,G+Q,D] / labels_out[B,G+Q] (the G rows, the accepted boxes in slot order, zero rows
 * with label -1), num_pasted[B], out_points[R,Cp] (per scene: the accepted objects' points, then the scene's points outside
 * every accepted box enlarged by remove_extra_width, in file order) and out_offsets[B+1]; rows at or beyond out_offsets[B] are
 * not written.  R >= total + B*Q*max_obj_points (SAD_EINVAL otherwise); an object's rows beyond max_obj_points are not pasted.
 * params != NULL: §35.1's transform is applied to every stored point and every row of boxes_out.  Four launches, no float
 * atomics, nothing read back, two calls bit-equal.  workspace: sad_gt_paste_workspace_bytes(B, Q, total) bytes, 16-byte aligned. */
typedef struct sad_global_augment_args {
    size_t struct_size;   /* = sizeof(sad_global_augment_args) */
    const float *points;           /* [total,Cp] */
    const int32_t *offsets;        /* [B+1] or NULL */
    const float *gt_boxes;         /* [B,G,D] or NULL when G == 0 */
    int B, N, total, Cp, G, D;
    unsigned seed;
    int flip_x, flip_y, with_velocity;
    float rot_lo, rot_hi, scale_lo, scale_hi;
    float translate[3];
    float *points_out;             /* [total,Cp] */
    float *boxes_out;              /* [B,G,D] or NULL when G == 0 */
    float *params;                 /* [B,8] */
} sad_global_augment_args;
int sad_global_augment_f32(const sad_global_augment_args *args, sad_stream_t stream);

#define SAD_PASTE_MAX_CLASSES 16
typedef struct sad_gt_paste_args {
    size_t struct_size;   /* = sizeof(sad_gt_paste_args) */
    const float *points;           /* [total,Cp] */
    const int32_t *offsets;        /* [B+1] */
    const float *gt_boxes;         /* [B,G,D] or NULL when G == 0 */
    const int32_t *gt_labels;      /* [B,G] or NULL when G == 0 */
    const float *db_points;        /* [.,Cp] */
    const int32_t *db_offsets;     /* [Ndb+1] */
    const float *db_boxes;         /* [Ndb,D] */
    const float *params;           /* [B,8] or NULL */
    int B, total, Cp, G, D, C, Ndb, max_obj_points, with_velocity;
    int class_offsets[SAD_PASTE_MAX_CLASSES + 1];
    int sample_num[SAD_PASTE_MAX_CLASSES];
    unsigned seed;
    float remove_extra_width;
    long long R;                   /* rows of out_points */
    int32_t *keep;                 /* [B,Q] */
    int32_t *db_index;             /* [B,Q] */
    float *boxes_out;              /* [B,G+Q,D] */
    int32_t *labels_out;           /* [B,G+Q] */
    int32_t *num_pasted;           /* [B] */
    float *out_points;             /* [R,Cp] */
    int32_t *out_offsets;          /* [B+1] */
    void *workspace;
} sad_gt_paste_args;
size_t sad_gt_paste_workspace_bytes(int B, int Q, int total);   /* 0 outside 1 <= B <= 65535, 1 <= Q <= 512, total >= 0 */
int sad_gt_paste_f32(const sad_gt_paste_args *args, sad_stream_t stream);

/* SPEC.md §36 (additions of ABI 4 as well).  Detection evaluation on the device.
 *
 * §36.1 sad_det_match_f32: per scene, the live detections (k < det_count[b] clamped to [0,K], or K without det_count, and
 * 0 <= det_labels < C) are walked in §23's rank order (score descending, index ascending) and assigned to the ground truth of
 * their class, independently for each of the T thresholds thr[C,T] (device memory).  The pair value is §19.3's IoU (metric
 * SAD_DET_IOU_BEV / SAD_DET_IOU3D, detection as a, ground truth as b: sad_boxes_iou_f32's bits; accepted iff v > thr, larger is
 * better) or the centre distance sqrtf(dx*dx + dy*dy) (SAD_DET_DIST: accepted iff v < thr, smaller is better).  The best
 * accepted box that is not ignored and not yet taken at t wins (lowest g on a tie): code 1, match g, value v, gt_det[g,t] = k;
 * else the best accepted ignored box absorbs the detection: code -1, match g, value v (ignored boxes are never taken); else
 * code 0, match -1, value 0.  A row that is not live gets (-1, -1, 0) and is never read beyond det_count.  A ground-truth label
 * outside [0, C) is padding; gt_det is -1 where nothing took the box; n_gt[B,C] counts the valid boxes that are not ignored.
 * G = 0 comes with NULL gt pointers.  One launch, one workgroup per scene, no workspace, no atomics on memory, every output
 * fully written, nothing read back; two calls are bit-equal.  K, G <= 1024, C <= 64, T <= 8, B <= 65535, else
 * SAD_EUNSUPPORTED.  NaN in any value that is read is undefined behaviour.
 *
 * §36.2 sad_det_ap_keys_f32 / sad_det_ap_f32: AP over N accumulated rows (scores[N], labels[N], code[N,T]).  keys[N] is the
 * composite key (class, or C for a label outside [0, C)) << 32 | descending-ordered score bits, -0 as +0; the caller sorts it
 * STABLY and passes the sorted keys with the permutation (int64 each).  For (c, t) the rows of class c with code != -1 in
 * that order give tp_i, fp_i, rec_i = (float)tp_i / (float)n_gt[c], prec_i = (float)tp_i / (float)(tp_i + fp_i), env_i =
 * max_{j >= i} prec_j; for k = first .. points, prec[c,t,k - first] = env at the first i with rec_i >= (float)k / (float)points,
 * or 0; ap = (sum_k fmaxf(s_k - floor, 0)) / ((float)(points - first + 1) * (1.0f - floor)), summed in ascending k;
 * max_recall = the last rec_i (0 without rows), n_det = the rows counted.  n_gt[c] == 0: ap = -1, prec = 0, max_recall = 0.
 * N * T < 2^31, points <= 128, C <= 64, T <= 8, else SAD_EUNSUPPORTED; 0 <= first <= points, 0 <= floor < 1. */
#define SAD_DET_IOU_BEV 0
#define SAD_DET_IOU3D 1
#define SAD_DET_DIST 2
typedef struct sad_det_match_args {
    size_t struct_size;   /* = sizeof(sad_det_match_args) */
    const float *det_boxes;        /* [B,K,D] */
    const float *det_scores;       /* [B,K] */
    const int32_t *det_labels;     /* [B,K] */
    const int32_t *det_count;      /* [B] or NULL */
    const float *gt_boxes;         /* [B,G,Dg] or NULL when G == 0 */
    const int32_t *gt_labels;      /* [B,G] or NULL when G == 0 */
    const int32_t *gt_ignore;      /* [B,G] or NULL */
    const float *thr;              /* [C,T] */
    int B, K, D, G, Dg, C, T, metric;
    int32_t *code;                 /* [B,K,T] */
    int32_t *match;                /* [B,K,T] */
    float *value;                  /* [B,K,T] */
    int32_t *gt_det;               /* [B,G,T] or NULL when G == 0 */
    int32_t *n_gt;                 /* [B,C] */
} sad_det_match_args;
int sad_det_match_f32(const sad_det_match_args *args, sad_stream_t stream);
int sad_det_ap_keys_f32(const float *scores, const int32_t *labels, long long N, int C, long long *keys, sad_stream_t stream);
typedef struct sad_det_ap_args {
    size_t struct_size;   /* = sizeof(sad_det_ap_args) */
    const long long *keys;         /* [N] sorted */
    const long long *perm;         /* [N] the permutation that sorted them */
    const int32_t *code;           /* [N,T] */
    const int32_t *n_gt;           /* [C] */
    long long N;
    int C, T, points, first;
    float floor;
    float *ap;                     /* [C,T] */
    float *prec;                   /* [C,T,points - first + 1] */
    float *max_recall;             /* [C,T] */
    int32_t *n_det;                /* [C,T] */
} sad_det_ap_args;
int sad_det_ap_f32(const sad_det_ap_args *args, sad_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SAD_AMD_H */
