// The two small launches around the main pass of a loss with per-workgroup partial sums (SPEC.md §27 "Sums" and "Launches"),
// shared by dense_loss.hip (§27) and point_head.hip (§31.2): the positive count before it and the ordered sum after it.
// Included inside each file's anonymous namespace, after prims.h (wave_count).
#pragma once

constexpr int CNT = 16;            // elements per thread of the count kernels (workgroups of 256 threads)

struct FinP {
    const float *src[4];
    int n[4], stride[4], ncomp;
    float *loss;
};

// num_pos[b] += #(labels[b, :] >= 0): integer atomics, order-independent.  grid (ceil(K / (CNT * 256)), B); num_pos starts at 0
__global__ __launch_bounds__(256) void count_pos_kernel(const int32_t *labels, int K, int32_t *num_pos) {
    const int b = blockIdx.y;
    const int32_t *row = labels + (size_t)b * K;
    int v[CNT];
#pragma unroll
    for (int q = 0; q < CNT; ++q) {                                   // (independent loads, issued together)
        const long long i = ((long long)blockIdx.x * CNT + q) * 256 + threadIdx.x;
        v[q] = i < K ? row[i] : -1;
    }
    int cnt = 0;
#pragma unroll
    for (int q = 0; q < CNT; ++q) cnt += v[q] >= 0;
    __shared__ int wsum[4];
    cnt = wave_count(cnt);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = cnt;
    __syncthreads();
    // one atomic per workgroup: positives are spread over the rows, and an atomic per wave queues thousands on B addresses
    if (threadIdx.x == 0 && wsum[0] + wsum[1] + wsum[2] + wsum[3]) atomicAdd(&num_pos[b], wsum[0] + wsum[1] + wsum[2] + wsum[3]);
}

// one wave per scene: loss[b, i] = the partial sums of component i, lane l adding workgroups l, l + 64, ... in ascending order
__global__ __launch_bounds__(64) void finish_kernel(const FinP p) {
    const int b = blockIdx.x, lane = threadIdx.x;
    for (int i = 0; i < p.ncomp; ++i) {
        const float *src = p.src[i] + (size_t)b * p.n[i] * p.stride[i];
        float v = 0.0f;
        for (int w = lane; w < p.n[i]; w += 64) v = v + src[(size_t)w * p.stride[i]];
#pragma unroll
        for (int off = 32; off; off >>= 1) v = v + __shfl_xor(v, off);
        if (lane == 0) p.loss[(size_t)b * p.ncomp + i] = v;
    }
}
