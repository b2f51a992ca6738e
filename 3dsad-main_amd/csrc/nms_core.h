// What the rotated-box NMS pipelines share (SPEC.md §13, §23): nms_bev_kernel and nms_prep / mask / walk (nms.hip), nmsx_select /
// rank / mask / walk (nms_select.hip).  §23 promises identical keep decisions, so the pair test, the candidate ranking, the
// decision chain of a chunk of 64 ranks, the per-scene workspace view and the mask kernel have ONE definition each, here.
// Included inside each file's anonymous namespace, after box_geom.h (poly_clip_area, iou_of) and prims.h (u64, readlane_u64).
#pragma once

// Does box p suppress box q?  IoU of §13 on local corners, centres (pc, qc: x, y) and areas, clipped in q's frame; `scratch` is the thread's slot of the clipping lists in LDS.
// The areas come by reference, so each caller decides when they are read: nms_bev_kernel's sit in LDS and are read where the
// sum needs them, after the clip (read ahead of it they cost that kernel 3 %); the mask kernel loads its global one into a
// register ahead of the clip, which hides the load (after the clip it costs that kernel 3 %).
template <int STRIDE>
__device__ __forceinline__ bool pair_suppresses(const float *pcx, const float *pcy, const float *pc, const float &pa, const float *qcx,
                                                const float *qcy, const float *qc, const float &qa, float iou_thr, float *scratch) {
    const float inter = poly_clip_area<STRIDE>(pcx, pcy, pc[0] - qc[0], pc[1] - qc[1], qcx, qcy, scratch);
    return iou_of(inter, pa, qa) > iou_thr;
}

// One workgroup of THREADS threads ranks a scene of K <= 512 boxes (scores in column 7 of 9): keep = 0, order = -1, then an
// O(K^2) counting rank among the candidates (score >= score_thr) by (score descending, index ascending) into s_rank2idx.
// Returns the candidate count n; s_rank2idx[0 .. n - 1] is visible to every thread on return.  Three barriers: scores and the
// zeroed counter | the ranks | the count (the counter is zeroed before the first one: after the ranking, as nms_bev_kernel had
// it, nms_prep_kernel needs 103 scalar registers instead of 57 and loses an occupancy step).
template <int THREADS>
__device__ __forceinline__ int rank_candidates(const float *bx, int K, float score_thr, int32_t *kp, int32_t *od,
                                               float *s_score, int *s_rank2idx, int *s_n) {
    const int tid = threadIdx.x;
    for (int i = tid; i < K; i += THREADS) {
        s_score[i] = bx[i * 9 + 7];
        kp[i] = 0;
        od[i] = -1;
    }
    if (tid == 0) *s_n = 0;
    __syncthreads();
    int nloc = 0;
    for (int i = tid; i < K; i += THREADS) {
        const float si = s_score[i];
        if (si >= score_thr) {
            int r = 0;
            for (int j = 0; j < K; ++j) {
                const float sj = s_score[j];
                r += (sj >= score_thr) && (sj > si || (sj == si && j < i));
            }
            s_rank2idx[r] = i;
            ++nloc;
        }
    }
    __syncthreads();                       // every rank is stored before the first count arrives
    atomicAdd(s_n, nloc);
    __syncthreads();
    return *s_n;
}

// The greedy decisions inside chunk c (ranks 64c .. 64c + 63, one per lane of one wave) as a scalar chain.  `own` is the lane's
// own word of the suppression matrix (whom it suppresses inside the chunk; 0 past n), `rem_word` the chunk's removed-word left
// by earlier chunks (wave-uniform).  Returns the 64-bit mask of the kept ranks, before any cap.  Only boxes whose own word is
// non-zero change anything for their chunk mates: the chain jumps from one such box to the next, everything alive in between
// is kept as it stands (a few steps per chunk: ctz, two lane reads, masks).
__device__ __forceinline__ u64 chunk_decide(u64 own, int n, int c, u64 rem_word) {
    const int left = n - 64 * c;
    const u64 valid = left >= 64 ? ~0ull : ((1ull << left) - 1ull);
    const u64 rem_lo = (u64)(unsigned)__builtin_amdgcn_readfirstlane((int)(rem_word & 0xFFFFFFFFull));
    const u64 rem_hi = (u64)(unsigned)__builtin_amdgcn_readfirstlane((int)(rem_word >> 32));
    u64 alive = valid & ~(rem_lo | (rem_hi << 32));
    u64 kept = 0ull;
    const u64 nz = __ballot(own != 0ull);
    while (true) {
        const u64 cand = alive & nz;
        if (cand == 0ull) {
            kept |= alive;
            break;
        }
        const int i = __builtin_amdgcn_readfirstlane(__builtin_ctzll(cand));
        const u64 upto = (2ull << i) - 1ull;                 // ranks 0 .. i of the chunk
        kept |= alive & upto;                                // i itself (alive), and the inert ones below it
        alive &= ~(readlane_u64(own, i) | upto);
    }
    return kept;
}

// Per-scene slices of a caller's workspace, in rank order.  A layout L carves them: L::scene_bytes(P) is its byte law,
// L::view(base, scene, P) fills this view (L::View may add fields of its own), L::LABELS says whether `label` exists.
struct NmsWs {
    int *n;               // the candidate count (first int of the scene's header)
    int *rank2idx;        // [P]
    int *label;           // [P], nullptr without classes
    float *area;          // [P]
    float *cx, *cy;       // [P][4] local corners (offsets from the centre)
    float *ctr;           // [P][2] centre x, y
    u64 *mask;            // [P][W] row p, word k: bit l = the box of rank 64k + l is suppressed by rank p (words k >= p / 64 only)
    int W;                // mask row stride in words
};

// The upper triangle of the n x n suppression matrix: one WAVE per ranked box, 16 boxes per workgroup, grid (ceil(P / 16), B).
// Lane l tests box p against box 64k + l, the ballot is the mask word.  Row p gets its words k = p / 64 .. ceil(n / 64) - 1 (the
// diagonal word onwards); the others are NOT stored: no walk reads them.  With labels a pair of different classes is decided
// without clipping.  Surplus workgroups exit on n.
constexpr int NMS_ROWS_PER_WG = 16;
template <class L>
__global__ __launch_bounds__(256) void nms_mask_kernel(int P, float iou_thr, int has_labels, void *__restrict__ wsbase) {
    __shared__ float s_poly[4 * 10 * 256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const auto w = L::view(wsbase, blockIdx.y, P);
    const int n = w.n[0];
    if (blockIdx.x * NMS_ROWS_PER_WG >= n) return;               // surplus workgroup (uniform)
    const int nch = (n + 63) >> 6;
    for (int rr = wave; rr < NMS_ROWS_PER_WG; rr += 4) {
        const int p = blockIdx.x * NMS_ROWS_PER_WG + rr;
        if (p >= n) continue;                                    // wave-uniform
        float pcx[4], pcy[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { pcx[k] = w.cx[p * 4 + k]; pcy[k] = w.cy[p * 4 + k]; }
        const float pc[2] = {w.ctr[p * 2], w.ctr[p * 2 + 1]};
        const float pa = w.area[p];
        const int pl = L::LABELS ? w.label[p] : 0;
        for (int k = p >> 6; k < nch; ++k) {
            const int q = 64 * k + lane;
            bool sup = false;
            if (q > p && q < n && !(L::LABELS && has_labels && w.label[q] != pl)) {
                float qcx[4], qcy[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) { qcx[c] = w.cx[q * 4 + c]; qcy[c] = w.cy[q * 4 + c]; }
                const float qc[2] = {w.ctr[q * 2], w.ctr[q * 2 + 1]};
                const float qa = w.area[q];                      // (ahead of the clip)
                sup = pair_suppresses<256>(pcx, pcy, pc, pa, qcx, qcy, qc, qa, iou_thr, s_poly + tid);
            }
            const u64 word = __ballot(sup);
            if (lane == 0) w.mask[(size_t)p * w.W + k] = word;
        }
    }
}
