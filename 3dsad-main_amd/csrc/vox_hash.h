// Coordinate hash table and scans shared by voxelization (voxel.hip, SPEC.md §20) and the sparse-convolution rulebook
// (spconv.hip, SPEC.md §21).  Included inside each file's anonymous namespace.
//
// table    ONE open-addressing table of a power of two >= 2 * (keys) slots: 64-bit keys (scene << 32 | cell), 64-bit CAS,
//          linear probing; the value of a key is the LOWEST number inserted under it (atomicMin), so nothing that is read
//          back depends on the order of an atomic.
// scans    exclusive scans over the 1024 threads of a workgroup, and of an int array in place by one workgroup.
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

__device__ __forceinline__ unsigned hash_slot0(u64 k64, int shift) { return (unsigned)((k64 * 0x9E3779B97F4A7C15ull) >> shift); }

// slot of k64, inserted if new; -1 only if the table were full (it holds at most cap / 2 keys: an empty slot is met long
// before a full round)
__device__ __forceinline__ int hash_insert(u64 *tkeys, unsigned mask, int shift, u64 k64) {
    unsigned h = hash_slot0(k64, shift);
    int slot = -1;
    for (unsigned n = 0; n <= mask; ++n) {
        u64 cur = __hip_atomic_load(&tkeys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == VX_EMPTY) {
            cur = atomicCAS(&tkeys[h], VX_EMPTY, k64);
            if (cur == VX_EMPTY) cur = k64;
        }
        if (cur == k64) { slot = (int)h; break; }
        h = (h + 1) & mask;
    }
    return slot;
}

// values only go down: a stale value is a larger one, so a caller that sees a lower one can skip the atomic
__device__ __forceinline__ void hash_min(int32_t *tvals, int slot, int i) {
    if (__hip_atomic_load(&tvals[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > i) atomicMin(&tvals[slot], i);
}

// slot of k64 in a table nobody writes any more, -1 if the key is absent
__device__ __forceinline__ int hash_find(const u64 *__restrict__ tkeys, unsigned mask, int shift, u64 k64) {
    unsigned h = hash_slot0(k64, shift);
    for (unsigned n = 0; n <= mask; ++n) {
        const u64 cur = tkeys[h];
        if (cur == k64) return (int)h;
        if (cur == VX_EMPTY) return -1;
        h = (h + 1) & mask;
    }
    return -1;
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

// a power of two >= 2 * keys (>= 2) and the shift that maps a 64-bit hash onto it
inline void hash_capacity(unsigned long long keys, unsigned &cap, int &shift) {
    cap = 2;
    int lg = 1;
    while ((unsigned long long)cap < 2ull * keys) { cap <<= 1; ++lg; }
    shift = 64 - lg;
}
