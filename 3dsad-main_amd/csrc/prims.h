// Device primitives that more than one translation unit needs: the vector types of the MFMA kernels, the cross-lane
// (DPP / readlane) unsigned maxima of the samplers, the LDS-DMA load with its wait, the integer hash of SPEC.md §17, the
// float atomic max of the pooled outputs and the sums, counts, normaliser, sigmoid pair and per-element losses of the loss kernels (§27, §29, §31).  Included inside each file's anonymous namespace, like reg_common.h, vox_hash.h and dense_tile.h (which include it).
// ONE definition of each: a helper moves here when a second family needs it; a helper with a single user stays in that file,
// and what only one family shares lives in that family's header (the dense heads' tile-image copies: dense_tile.h; the NMS
// pair test, ranking, chunk chain, workspace view and mask kernel: nms_core.h).
#pragma once

typedef unsigned long long u64;
typedef float f32x16 __attribute__((ext_vector_type(16)));      // accumulator of a 32x32 MFMA
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));      // A / B operand of v_mfma_f32_32x32x16_bf16
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

// ---- cross-lane maxima, 64-bit -------------------------------------------------------------------------------------------
// The FPS arg-max key is float_bits(min_dist) << 32 | ~index: unsigned max = largest distance, ties -> lowest index
// (min-distances are >= 0, so their bit patterns order like the floats).  DPP controls used throughout:
// 0xB1 quad_perm [1,0,3,2], 0x4E quad_perm [2,3,0,1], 0x141 row_half_mirror, 0x140 row_mirror — an in-row butterfly
// on the DPP path (no LDS crossbar) after which every lane of a row of 16 holds the row's maximum.
template <int CTRL>
__device__ __forceinline__ u64 dpp_u64(u64 v) {
    const unsigned lo = __builtin_amdgcn_update_dpp(0u, (unsigned)v, CTRL, 0xF, 0xF, false);
    const unsigned hi = __builtin_amdgcn_update_dpp(0u, (unsigned)(v >> 32), CTRL, 0xF, 0xF, false);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 umax64(u64 a, u64 b) { return a > b ? a : b; }
__device__ __forceinline__ u64 row_max_u64(u64 k) {  // max over each row of 16 lanes
    k = umax64(k, dpp_u64<0xB1>(k));
    k = umax64(k, dpp_u64<0x4E>(k));
    k = umax64(k, dpp_u64<0x141>(k));
    k = umax64(k, dpp_u64<0x140>(k));
    return k;
}
__device__ __forceinline__ u64 readlane_u64(u64 v, int l) {
    const unsigned lo = __builtin_amdgcn_readlane((unsigned)v, l);
    const unsigned hi = __builtin_amdgcn_readlane((unsigned)(v >> 32), l);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 wave_max_u64(u64 k) {   // wave-uniform result
    k = row_max_u64(k);
    return umax64(umax64(readlane_u64(k, 0), readlane_u64(k, 16)), umax64(readlane_u64(k, 32), readlane_u64(k, 48)));
}

// ---- cross-lane maxima, 32-bit -------------------------------------------------------------------------------------------
// A 64-bit key max is done as max(high words), then max of the low words among the lanes that hold that high word — two
// cheap v_max_u32 butterflies instead of 64-bit compare/select chains.
template <int CTRL>
__device__ __forceinline__ unsigned dpp_max_u32(unsigned v) {
    const unsigned o = __builtin_amdgcn_update_dpp(0u, v, CTRL, 0xF, 0xF, false);
    return o > v ? o : v;
}
template <int STEPS>
__device__ __forceinline__ unsigned row_max_u32(unsigned v) {   // max over aligned groups of 2^STEPS lanes (<= 16)
    if constexpr (STEPS >= 1) v = dpp_max_u32<0xB1>(v);
    if constexpr (STEPS >= 2) v = dpp_max_u32<0x4E>(v);
    if constexpr (STEPS >= 3) v = dpp_max_u32<0x141>(v);
    if constexpr (STEPS >= 4) v = dpp_max_u32<0x140>(v);
    return v;
}
// The 64-lane maximum in three forms.  All return the same wave-uniform value; they differ in how the four row maxima are
// combined, i.e. in what the wave issues on a serial sampling step — which is what bounds FPS.
//
// wave_max_u32: four v_readlane + three scalar max, everything after the row butterfly is scalar.  The earliest bucketed
// sampler (fps_bucket_kernel, fps_bucket.hip), which predates the instruction counting of the later forms.
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {  // wave-uniform result
    v = row_max_u32<4>(v);
    const unsigned a = __builtin_amdgcn_readlane(v, 0), b = __builtin_amdgcn_readlane(v, 16);
    const unsigned c = __builtin_amdgcn_readlane(v, 32), d = __builtin_amdgcn_readlane(v, 48);
    const unsigned ab = a > b ? a : b, cd = c > d ? c : d;
    return ab > cd ? ab : cd;
}
// wave_max_u32_bcast: the cross-row part as two row_bcast DPP steps through the builtin and ONE v_readlane of lane 63.  The
// first form of the cell-bucket samplers (fps_cell_kernel, fps_cellg_kernel: fps_bucket.hip) and the distance-matrix sampler
// (fps_dmat_kernel: ffps.hip).  hipcc expands each builtin step into v_mov + v_mov_dpp + v_max.
__device__ __forceinline__ unsigned wave_max_u32_bcast(unsigned v) {
    v = row_max_u32<4>(v);
    unsigned o = __builtin_amdgcn_update_dpp(v, v, 0x142, 0xA, 0xF, false);   // row_bcast:15 -> rows 1,3
    v = o > v ? o : v;
    o = __builtin_amdgcn_update_dpp(v, v, 0x143, 0xC, 0xF, false);            // row_bcast:31 -> rows 2,3
    v = o > v ? o : v;
    return __builtin_amdgcn_readlane(v, 63);
}
// wave_max_u32_b: the same two steps as single v_max_u32_dpp instructions in inline asm (one instruction per step instead
// of three).  The second and third form of the cell-bucket samplers (fps_cell2_kernel, fps_cell3_kernel, fps_cellg2_kernel:
// fps_bucket.hip), where every instruction a wave issues per step counts against the SIMD's shared issue port.
__device__ __forceinline__ unsigned wave_max_u32_b(unsigned v) {   // wave-uniform result (SGPR)
    v = row_max_u32<4>(v);
    // row_bcast:15 -> rows 1, 3; row_bcast:31 -> rows 2, 3; dst == src1, so the rows left out keep their value
    // (no wait states are inserted inside asm: two after the VALU write of v, two between the DPP steps)
    asm("s_nop 1\n\tv_max_u32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
        "s_nop 1\n\tv_max_u32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf" : "+v"(v));
    return __builtin_amdgcn_readlane(v, 63);
}

// ---- LDS-DMA -------------------------------------------------------------------------------------------------------------
// One wave-wide 16-byte LDS-DMA: global_load_lds_dwordx4, 1 KB lands at lds_dst + 16 * lane (lds_dst is wave-uniform).  M0
// carries the LDS address and is the compiler's (hipcc lowers register-indexed vectors through it), so it is saved and
// restored in the statement that uses it.  The compiler keeps no count of these loads, hence no wait of its own: they are
// retired by a counted wait_vm and published by a barrier — a stage is read in the phase AFTER the barrier that follows its wait.
__device__ __forceinline__ void glds16(const void *gsrc, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(__builtin_amdgcn_readfirstlane(lds_dst)));
    // (no "memory" clobber: with one, the by-value argument block is kept in scratch and re-read through it; the statements are volatile,
    // so they keep their order among themselves and relative to the barriers, which is all the rings need)
}
template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N)); }

// ---- the integer hash of SPEC.md §17 ---------------------------------------------------------------------------------------
// h(seed, b, i): a pure 32-bit integer function, the same in io.fix_size, the oracle, subsample_pad (head.hip) and the RoI
// sampler (roi_head.hip).
__device__ __forceinline__ unsigned mix32(unsigned a) {
    a ^= a >> 16; a *= 0x85EBCA6Bu; a ^= a >> 13; a *= 0xC2B2AE35u; a ^= a >> 16;
    return a;
}
__device__ __forceinline__ unsigned h17(unsigned seed, unsigned b, unsigned i) {
    return mix32(seed * 0x9E3779B1u + b * 0x85EBCA77u + i * 0xC2B2AE3Du + 0x27D4EB2Fu);
}

// ---- float atomic max ------------------------------------------------------------------------------------------------------
// Valid ONLY for values >= +0 (outputs of a ReLU) merged into a buffer that starts at zero: such floats order like their
// bit patterns read as unsigned integers, and 0 is the neutral element.  A negative value or -0 would win every comparison.
__device__ __forceinline__ void atomic_max_pos(float *addr, float v) {
    atomicMax(reinterpret_cast<unsigned *>(addr), __builtin_bit_cast(unsigned, v));
}

// ---- the loss kernels (dense_loss.hip §27, roi_loss.hip §29, point_head.hip §31) ------------------------------------------------
// the sum of a workgroup of 256 threads: butterfly over the wave (every lane ends with the same bits: + is commutative), then the
// four wave sums in order.  Every thread of the workgroup calls it; `red` has 4 floats.
__device__ __forceinline__ float block_sum(float v, float *red) {
#pragma unroll
    for (int off = 32; off; off >>= 1) v = v + __shfl_xor(v, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

__device__ __forceinline__ int wave_count(int v) {
#pragma unroll
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// §27 the weight of a component: scale / (float)max(n, 1), or scale
__device__ __forceinline__ float norm_weight(float scale, int n, int normalize) {
    return normalize ? scale / (float)max(n, 1) : scale;
}

// §27.1 the sigmoid and its complement
__device__ __forceinline__ void sigmoid2(float x, float e, float &p, float &pc) {
    const float den = 1.0f + e;
    const float big = 1.0f / den, small = e / den;
    p = x >= 0.0f ? big : small;
    pc = x >= 0.0f ? small : big;
}

// §27.1 sigmoid focal classification (gamma = 2) of one logit against a hard target -> term (value) and gradient (g)
__device__ __forceinline__ float focal_one(float alpha, float oma, float x, bool t, bool live, float wq, float &g) {
    const float e = expf(-fabsf(x));
    float pr, pc;
    sigmoid2(x, e, pr, pc);
    const float bce = (fmaxf(x, 0.0f) - (t ? x : 0.0f)) + log1pf(e);
    const float pt = t ? pc : pr;
    const float aw = t ? alpha : oma;
    const float l = (aw * (pt * pt)) * bce;
    const float gt = ((-alpha) * (pc * pc)) * (((2.0f * pr) * bce) + pc);
    const float gf = (oma * (pr * pr)) * (((2.0f * pc) * bce) + pr);
    g = live ? (t ? gt : gf) * wq : 0.0f;
    return live ? l * wq : 0.0f;
}

// §29 binary cross-entropy of one logit against a soft target -> term (value) and gradient (g)
__device__ __forceinline__ float bce_one(float x, float t, bool live, float wq, float &g) {
    const float e = expf(-fabsf(x));
    float pr, pc;
    sigmoid2(x, e, pr, pc);
    const float bce = (fmaxf(x, 0.0f) - (x * t)) + log1pf(e);
    g = live ? (pr - t) * wq : 0.0f;
    return live ? bce * wq : 0.0f;
}

// §27.1 smooth-L1 of one weighted difference d -> the term (value) and its derivative with respect to d (sg)
__device__ __forceinline__ float smooth_l1(float d, float beta, float &sg) {
    const float a = fabsf(d);
    const bool quad = a < beta;
    sg = quad ? d / beta : (float)((d > 0.0f) - (d < 0.0f));
    return quad ? ((0.5f * a) * a) / beta : a - (0.5f * beta);
}

// §27.1 the sine-difference yaw term: sin(p - t) * cw6 for smooth_l1, and extra = cos(p - t), the factor its gradient picks up
__device__ __forceinline__ float sin_diff(float sp, float cp, float st, float ct, float cw6, float &extra) {
    const float d = ((sp * ct) - (cp * st)) * cw6;
    extra = (cp * ct) + (sp * st);
    return d;
}
