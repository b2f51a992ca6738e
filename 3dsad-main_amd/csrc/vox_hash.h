// Coordinate table, first-appearance numbering and scans shared by voxelization (voxel.hip, SPEC.md §20), the sparse-convolution
// rulebook (spconv.hip, SPEC.md §21) and its transpose (spconv_grad.hip).  Included inside each file's anonymous namespace.
//
// table      CoordTable: ONE open-addressing table of a power of two >= 2 * (keys) slots: 64-bit keys (scene << 32 | cell), 64-bit
//            CAS, linear probing; the value of a key is the LOWEST number inserted under it (keep_min), so nothing that is read back
//            depends on the order of an atomic.
// numbering  (§20.2) elements (rows, or the candidates of the strided rulebook) are numbered by first appearance of their key: an
//            element is an OPENER iff it is the lowest number under its key.  flags: openers are counted per 64 elements by a
//            ballot; scan: one workgroup scans the counts in place and takes the prefix at every scene start; number: an opener's
//            number is the prefix of its 64 plus the openers in the lower lanes.  The user's opener object Op has: Op::index,
//            the type of an element number (int keeps 32-bit index arithmetic); index n, the number of elements;
//            bool operator()(e), is e an opener (false for e >= n); index first_of(row), the first element of input row `row`
//            (offsets[b] goes in; clamped to 0 .. n).
// scans      exclusive scans over the 1024 threads of a workgroup, and of an int array in place by one workgroup.
// rows       the table of a sparse tensor's rows (§21): clear + insert, with their launches.
#pragma once
#include "prims.h"       // u64

constexpr int VX_THREADS = 256;
constexpr int VX_SCAN_THREADS = 1024;
constexpr u64 VX_EMPTY = ~0ull;

// largest b in [0, B-1] with offsets[b] <= i: the scene that owns row i (empty scenes own nothing)
__device__ __forceinline__ int scene_of(const int32_t *__restrict__ off, int B, int i) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// *p = min(*p, v) (T = unsigned: on a buffer filled with -1, the largest).  Values only go down: a stale value is a larger one, so
// a caller that sees a lower one can skip the atomic
template <class T>
__device__ __forceinline__ void keep_min(T *p, T v) {
    if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > v) atomicMin(p, v);
}

// a[0..n) = v by the whole grid (workgroups of VX_THREADS)
__device__ __forceinline__ void grid_fill(int32_t *__restrict__ a, unsigned n, int v) {
    const unsigned stride = gridDim.x * VX_THREADS;
    for (unsigned s = blockIdx.x * VX_THREADS + threadIdx.x; s < n; s += stride) a[s] = v;
}

struct CoordTable {
    u64 *keys;           // [mask + 1]
    int32_t *vals;       // [mask + 1]: the lowest number inserted under the key
    unsigned mask;       // slots - 1
    int shift;           // maps a 64-bit hash onto the slots

    CoordTable() = default;
    // a table for `nkeys` keys, a power of two >= 2 * nkeys (>= 2) slots, in the next two slices of workspace `ws` (NULL: a size
    // query: the slices are taken, nothing is dereferenced)
    CoordTable(void *ws, sad::Carve &c, unsigned long long nkeys) {
        unsigned cap = 2;
        while ((unsigned long long)cap < 2ull * nkeys) cap <<= 1;
        keys = (u64 *)((uintptr_t)ws + c.take((size_t)cap * 8));
        vals = (int32_t *)((uintptr_t)ws + c.take((size_t)cap * 4));
        mask = cap - 1;
        shift = 64 - __builtin_ctz(cap);
    }

    // every slot empty, by the whole grid (workgroups of VX_THREADS)
    __device__ __forceinline__ void clear() const {
        const unsigned stride = gridDim.x * VX_THREADS;
        for (unsigned s = blockIdx.x * VX_THREADS + threadIdx.x; s <= mask; s += stride) { keys[s] = VX_EMPTY; vals[s] = INT_MAX; }
    }

    __device__ __forceinline__ unsigned slot0(u64 k64) const { return (unsigned)((k64 * 0x9E3779B97F4A7C15ull) >> shift); }

    // k64 goes in if it is new, and v stays if it is the lowest number under k64.  Returns the slot; -1 only if the table were full
    // (it holds at most half as many keys as slots: an empty slot is met long before a full round)
    __device__ __forceinline__ int insert_min(u64 k64, int v) const {
        unsigned h = slot0(k64);
        int slot = -1;
        for (unsigned n = 0; n <= mask; ++n) {
            u64 cur = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == VX_EMPTY) {
                cur = atomicCAS(&keys[h], VX_EMPTY, k64);
                if (cur == VX_EMPTY) cur = k64;
            }
            if (cur == k64) { slot = (int)h; break; }
            h = (h + 1) & mask;
        }
        if (slot >= 0) keep_min(&vals[slot], v);          // (behind the loop, where the lanes of a wave do it together)
        return slot;
    }

    // slot of k64 in a table nobody writes any more, -1 if the key is absent
    __device__ __forceinline__ int find(u64 k64) const {
        unsigned h = slot0(k64);
        for (unsigned n = 0; n <= mask; ++n) {
            const u64 cur = keys[h];
            if (cur == k64) return (int)h;
            if (cur == VX_EMPTY) return -1;
            h = (h + 1) & mask;
        }
        return -1;
    }

    // the lowest number inserted under the key of `slot` (a table nobody writes any more)
    __device__ __forceinline__ int lowest(int slot) const { return vals[slot]; }
};

// ---- the table of a sparse tensor's rows (§21) --------------------------------------------------------------------
// every slot empty; then row i of coors [Nv,3] (z,y,x) goes in under (its scene << 32 | (z * Gy + y) * Gx + x): the lowest row
// owns a duplicated coordinate.  The rulebook (spconv.hip) and the voxel query (voxel_query.hip) build their input table this way.
__global__ __launch_bounds__(VX_THREADS) void coord_clear_kernel(CoordTable t) { t.clear(); }

__global__ __launch_bounds__(VX_THREADS) void coord_insert_rows_kernel(const int32_t *__restrict__ coors, const int32_t *__restrict__ offsets, int Nv,
                                                                       int B, int Gy, int Gx, CoordTable t) {
    const int i = blockIdx.x * VX_THREADS + threadIdx.x;
    if (i >= Nv) return;
    const int32_t *c = coors + (size_t)i * 3;
    const int key = (c[0] * Gy + c[1]) * Gx + c[2];
    t.insert_min(((u64)(unsigned)scene_of(offsets, B, i) << 32) | (unsigned)key, i);
}

inline void launch_coord_clear(const CoordTable &t, hipStream_t st) {
    const unsigned long long slots = t.mask + 1ull;
    hipLaunchKernelGGL(coord_clear_kernel, dim3(slots > 16384ull * VX_THREADS ? 16384u : sad::blocks_for(slots, VX_THREADS)), dim3(VX_THREADS), 0, st, t);
}

inline void launch_coord_rows(const int32_t *coors, const int32_t *offsets, int Nv, int B, int Gy, int Gx, const CoordTable &t, hipStream_t st) {
    launch_coord_clear(t, st);
    if (Nv > 0)
        hipLaunchKernelGGL(coord_insert_rows_kernel, dim3(sad::blocks_for((unsigned long long)Nv, VX_THREADS)), dim3(VX_THREADS), 0, st, coors, offsets, Nv,
                           B, Gy, Gx, t);
}

__device__ __forceinline__ int wave_incl_scan(int x, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(x, d);
        if (lane >= d) x += t;
    }
    return x;
}

// exclusive scan over the VX_SCAN_THREADS threads of a workgroup; total = sum of all.  s_w: 17 ints of LDS
__device__ __forceinline__ int block_excl_scan(int v, int *s_w, int &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int inc = wave_incl_scan(v, lane);
    __syncthreads();                                        // (s_w of a previous call is no longer read)
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int w = 0; w < VX_SCAN_THREADS / 64; ++w) { const int t = s_w[w]; s_w[w] = run; run += t; }
        s_w[VX_SCAN_THREADS / 64] = run;
    }
    __syncthreads();
    total = s_w[VX_SCAN_THREADS / 64];
    return s_w[wave] + inc - v;
}

// one workgroup: a[0..n) -> exclusive prefix in place, a[n] = total
__device__ __forceinline__ void scan_in_place(int32_t *a, int n, int *s_w) {
    const int chunk = (n + VX_SCAN_THREADS - 1) / VX_SCAN_THREADS;
    const int k0 = min(n, (int)threadIdx.x * chunk), k1 = min(n, k0 + chunk);
    int sum = 0;
    for (int k = k0; k < k1; ++k) sum += a[k];
    int tot;
    int run = block_excl_scan(sum, s_w, tot);
    for (int k = k0; k < k1; ++k) { const int t = a[k]; a[k] = run; run += t; }
    if (threadIdx.x == 0) a[n] = tot;
    __syncthreads();
}

// ---- first-appearance numbering ---------------------------------------------------------------------------------
// flags: wavecnt[w] = openers among elements 64 w .. 64 w + 63
template <class Op>
__global__ __launch_bounds__(VX_THREADS) void opener_flags_kernel(const Op op, int32_t *__restrict__ wavecnt) {
    const typename Op::index e = (typename Op::index)blockIdx.x * VX_THREADS + threadIdx.x;
    const unsigned long long m = __ballot(op(e));
    if ((threadIdx.x & 63) == 0 && e < op.n) wavecnt[e >> 6] = __builtin_popcountll(m);
}

// scan, one workgroup of VX_SCAN_THREADS: wavecnt[nw + 1] -> exclusive prefixes in place; P[b] = openers among the elements of the
// rows below offsets[b] (b = 0 .. B).  s_w: 17 ints of LDS
template <class Op>
__device__ __forceinline__ void opener_scan(const Op &op, const int32_t *__restrict__ offsets, int B, int32_t *wavecnt, int nw, int32_t *P,
                                            int *s_w) {
    scan_in_place(wavecnt, nw, s_w);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int b = wave; b <= B; b += VX_SCAN_THREADS / 64) {
        const typename Op::index o = op.first_of(offsets[b]);
        const int w = (int)(o >> 6);
        const typename Op::index r = ((typename Op::index)w << 6) + lane;
        const unsigned long long m = __ballot(r < o && op(r));
        if (lane == 0) P[b] = wavecnt[w] + __builtin_popcountll(m);      // (w <= nw: wavecnt[nw] is the total)
    }
}

// number: the openers in the lanes below this one (all 64 lanes call it); opener e's number is the scanned wavecnt[e >> 6] + this
__device__ __forceinline__ int openers_below(bool open) {
    const unsigned long long m = __ballot(open);
    return __builtin_popcountll(m & ((1ull << (threadIdx.x & 63)) - 1ull));
}
