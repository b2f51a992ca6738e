// Box selection and rotated-box NMS at scale for gfx950 (SPEC.md §23): any K, scores and labels in their own tensors,
// top-`pre_max` pre-selection, class-aware suppression, `post_max` cap.  The IoU is §13's, through box_geom.h, so the
// keep decisions are the ones of nms.hip and of the CPU oracle.  Four launches whose dimensions depend on (B, K, P) alone
// (P = min(K, pre_max) <= 16 384); the data-dependent number of selected boxes n lives in the workspace and surplus
// workgroups exit on it.  No device-to-host read, no host synchronisation.
//   select (one workgroup per scene): order-preserving 32-bit keys, radix select of the P-th largest key (four 8-bit
//           histogram passes over the scene's scores), exact counts above / at the threshold key, then an index-ordered
//           compaction: everything above the threshold key plus the LOWEST-INDEX ties at it.  Also initialises keep / order.
//   rank   (256 selected boxes per workgroup): exact counting rank by (key desc, index asc) with the n packed
//           (key, ~index) words staged through LDS; writes rank2idx, local corners, centres, areas, labels in rank order.
//   mask   (one wave per ranked box): nms_core.h's mask kernel on this file's layout, row stride ceil(P/64) words, labels on.
//   walk   (one workgroup per scene): chunk_decide (nms_core.h) on wave 0; the words a chunk's kept rows suppress in later
//           chunks are or-ed into LDS by all four waves (thread k owns word k: no atomics).
// The pair test, the chain of a chunk, the mask kernel and the workspace view are nms_core.h's, shared with nms.hip.  Here:
// the selection, the ranking of the selected boxes, the nms_boxes workspace law and the four-wave walk with its post cap.
#include "box_geom.h"

namespace {

#include "prims.h"       // u64, readlane_u64
#include "nms_core.h"

constexpr int NMSX_MAXP = 16384;
constexpr int NMSX_MAXW = NMSX_MAXP / 64;        // 256 removed-words per scene, held in LDS by the walk

// Descending score order and `score >= score_thr` as unsigned compares: sign-flipped float bits, both zeros one key.
__device__ __forceinline__ unsigned score_key(float s) {
    unsigned b = __float_as_uint(s);
    if ((b << 1) == 0u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ int lanes_below(u64 ballot) {      // set bits of `ballot` in the lanes below this one
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ballot, 0u));
}

// per scene (8-byte items first; the scene stride is a multiple of 16): hdr [16] ints, sel [P], mask [P][W], cx, cy [P][4],
// ctr [P][2], rank2idx, label, area [P], with W = ceil(P / 64)
struct NmsxLayout {
    struct View : NmsWs {
        int *hdr;         // [16]: n, n_above, take, threshold key (n = hdr)
        u64 *sel;         // [P]   selected boxes, unranked: key << 32 | ~index
    };
    static constexpr bool LABELS = true;
    __host__ __device__ static size_t scene_bytes(int P) {
        const size_t W = (size_t)(P + 63) / 64;
        const size_t b = 64 + (size_t)P * 8 + (size_t)P * W * 8 + (size_t)P * 16 * 2 + (size_t)P * 8 + (size_t)P * 4 * 3;
        return sad::al16(b);
    }
    __device__ __forceinline__ static View view(void *base, int scene, int P) {
        unsigned char *q = (unsigned char *)base + (size_t)scene * scene_bytes(P);
        View w;
        w.W = (P + 63) >> 6;
        w.n = w.hdr = (int *)q; q += 64;
        w.sel = (u64 *)q; q += (size_t)P * 8;
        w.mask = (u64 *)q; q += (size_t)P * w.W * 8;
        w.cx = (float *)q; q += (size_t)P * 16;
        w.cy = (float *)q; q += (size_t)P * 16;
        w.ctr = (float *)q; q += (size_t)P * 8;
        w.rank2idx = (int *)q; q += (size_t)P * 4;
        w.label = (int *)q; q += (size_t)P * 4;
        w.area = (float *)q;
        return w;
    }
};

// ---- select ---------------------------------------------------------------------------------------------------------
// T_k = max(P-th largest key of the scene, key(score_thr)).  n_above = #(key > T_k) <= P - 1 and the selection is those
// plus the first take = min(#(key == T_k), P - n_above) ties in index order: exactly ranks 0 .. n - 1 of §23, n = n_above
// + take <= P.  Every write into `sel` is guarded by slot < P on top of that, whatever the counts say.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void nmsx_select_kernel(const float *__restrict__ scores, int K, int P, int Pout,
                                                              float score_thr, int32_t *__restrict__ keep,
                                                              int32_t *__restrict__ order, void *__restrict__ wsbase) {
    constexpr int NW = THREADS / 64;
    __shared__ unsigned s_hist[256], s_scan[256];
    __shared__ unsigned s_digit, s_left, s_above, s_tie;
    __shared__ unsigned s_wa[NW], s_wt[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned uK = (unsigned)K;
    const float *sc = scores + (size_t)blockIdx.x * K;
    int32_t *kp = keep + (size_t)blockIdx.x * K, *od = order + (size_t)blockIdx.x * Pout;
    const auto w = NmsxLayout::view(wsbase, blockIdx.x, P);

    for (unsigned i = tid; i < uK; i += THREADS) kp[i] = 0;
    for (int i = tid; i < Pout; i += THREADS) od[i] = -1;

    // the P-th largest key (it exists: P <= K), eight bits at a time from the top
    unsigned prefix = 0u, left = (unsigned)P;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        if (tid < 256) s_hist[tid] = 0u;
        if (tid == 0) { s_digit = 0u; s_left = 1u; }
        __syncthreads();
        unsigned cur = 0u, run = 0u;               // equal digits in a row cost one LDS atomic (scores cluster in few bins)
        for (unsigned i = tid; i < uK; i += THREADS) {
            const unsigned key = score_key(sc[i]);
            if (pass == 0 || (key >> (shift + 8)) == prefix) {
                const unsigned d = (key >> shift) & 255u;
                if (d != cur && run) { atomicAdd(&s_hist[cur], run); run = 0u; }
                cur = d;
                ++run;
            }
        }
        if (run) atomicAdd(&s_hist[cur], run);
        __syncthreads();
        // inclusive suffix sums of the histogram: bin t holds the left-th largest iff above(t) < left <= above(t) + hist[t]
        const unsigned v = tid < 256 ? s_hist[tid] : 0u;
        if (tid < 256) s_scan[tid] = v;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const unsigned x = (tid < 256 && tid + off < 256) ? s_scan[tid + off] : 0u;
            __syncthreads();
            if (tid < 256) s_scan[tid] += x;
            __syncthreads();
        }
        if (tid < 256) {
            const unsigned incl = s_scan[tid], above = incl - v;
            if (above < left && left <= incl) { s_digit = (unsigned)tid; s_left = left - above; }
        }
        __syncthreads();
        prefix = (prefix << 8) | s_digit;
        left = s_left;
        __syncthreads();
    }
    const unsigned kthr = score_key(score_thr);
    const unsigned Tk = prefix > kthr ? prefix : kthr;

    // exact counts above and at the threshold key
    if (tid == 0) { s_above = 0u; s_tie = 0u; }
    __syncthreads();
    unsigned ca = 0u, ct = 0u;
    for (unsigned i = tid; i < uK; i += THREADS) {
        const unsigned key = score_key(sc[i]);
        ca += key > Tk;
        ct += key == Tk;
    }
    if (ca) atomicAdd(&s_above, ca);
    if (ct) atomicAdd(&s_tie, ct);
    __syncthreads();
    const unsigned uP = (unsigned)P;
    const unsigned n_above = s_above < uP ? s_above : uP;
    const unsigned take = s_tie < uP - n_above ? s_tie : uP - n_above;
    if (tid == 0) { w.hdr[0] = (int)(n_above + take); w.hdr[1] = (int)n_above; w.hdr[2] = (int)take; w.hdr[3] = (int)Tk; }

    // compaction in index order: ballot + mbcnt inside a wave, wave totals through LDS in wave order, running bases in registers
    unsigned run_a = 0u, run_t = 0u;
    for (unsigned base = 0; base < uK; base += THREADS) {
        const unsigned i = base + tid;
        const bool in = i < uK;
        const unsigned key = in ? score_key(sc[i]) : 0u;
        const bool ab = in && key > Tk, ti = in && key == Tk;
        const u64 bab = __ballot(ab), bti = __ballot(ti);
        if (lane == 0) { s_wa[wave] = __builtin_popcountll(bab); s_wt[wave] = __builtin_popcountll(bti); }
        __syncthreads();
        unsigned offa = 0u, offt = 0u, tota = 0u, tott = 0u;
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            const unsigned a = s_wa[k], t = s_wt[k];
            if (k < wave) { offa += a; offt += t; }
            tota += a; tott += t;
        }
        const u64 comp = ((u64)key << 32) | (u64)(~i);
        if (ab) {
            const unsigned slot = run_a + offa + (unsigned)lanes_below(bab);
            if (slot < uP) w.sel[slot] = comp;
        }
        if (ti) {
            const unsigned o = run_t + offt + (unsigned)lanes_below(bti);      // this tie's ordinal in index order
            if (o < take) {
                const unsigned slot = n_above + o;
                if (slot < uP) w.sel[slot] = comp;
            }
        }
        run_a += tota; run_t += tott;
        __syncthreads();
    }
}

// ---- rank -----------------------------------------------------------------------------------------------------------
// rank(j) = #{m : (key_m, ~idx_m) > (key_j, ~idx_j)} over the n selected boxes: distinct indices give distinct ranks in
// 0 .. n - 1 < P.
constexpr int NMSX_RANK_TILE = 2048;
__global__ __launch_bounds__(256) void nmsx_rank_kernel(const float *__restrict__ boxes, int D, const int32_t *__restrict__ labels,
                                                        int K, int P, void *__restrict__ wsbase) {
    __shared__ u64 s_c[NMSX_RANK_TILE];
    const int tid = threadIdx.x;
    const auto w = NmsxLayout::view(wsbase, blockIdx.y, P);
    const int n = w.n[0];
    const int j = blockIdx.x * 256 + tid;
    if (blockIdx.x * 256 >= n) return;                           // surplus workgroup (uniform)
    const bool have = j < n;
    const u64 cj = have ? w.sel[j] : ~0ull;
    int r = 0;
    for (int base = 0; base < n; base += NMSX_RANK_TILE) {
        const int m = n - base < NMSX_RANK_TILE ? n - base : NMSX_RANK_TILE;
        __syncthreads();
        for (int t = tid; t < m; t += 256) s_c[t] = w.sel[base + t];
        __syncthreads();
#pragma unroll 8
        for (int t = 0; t < m; ++t) r += s_c[t] > cj;
    }
    if (have && r < n) {
        const int idx = (int)~(unsigned)cj;
        const size_t row = (size_t)blockIdx.y * K + (size_t)idx;
        const float *b = boxes + row * D;
        box_footprint(b, w.cx + r * 4, w.cy + r * 4, w.ctr + r * 2, w.area[r]);
        w.rank2idx[r] = idx;
        w.label[r] = labels ? labels[row] : 0;
    }
}

// ---- walk -----------------------------------------------------------------------------------------------------------
// Greedy walk, 64 ranks (one chunk) at a time.  Wave 0 decides a chunk with chunk_decide (the scalar chain over the chunk's
// own words), cuts it at post_max and writes keep / order (positions nk + prefix < min(n, post_max) <= Pout).
// Then thread t or-s the words k = c + 1 + t of the chunk's kept rows into s_rem[k]: coalesced along a row, sixteen
// independent loads in flight, and a one-wave loop over the rows' later words (a dependent-latency chain at n = 16 384) is gone.
__global__ __launch_bounds__(256) void nmsx_walk_kernel(int K, int P, int Pout, int post_max, int32_t *__restrict__ keep,
                                                        int32_t *__restrict__ order, int32_t *__restrict__ count,
                                                        void *__restrict__ wsbase) {
    __shared__ u64 s_rem[NMSX_MAXW];
    __shared__ u64 s_kept;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const auto w = NmsxLayout::view(wsbase, blockIdx.x, P);
    int32_t *kp = keep + (size_t)blockIdx.x * K, *od = order + (size_t)blockIdx.x * Pout;
    const int n = __builtin_amdgcn_readfirstlane(w.n[0]);
    const int W = w.W, nch = (n + 63) >> 6;                      // nch <= W <= NMSX_MAXW
    s_rem[tid] = 0ull;
    __syncthreads();
    int nk = 0;
    for (int c = 0; c < nch; ++c) {                              // (uniform)
        if (wave == 0) {
            const int p = 64 * c + lane;
            const bool have = p < n;
            const u64 own = have ? w.mask[(size_t)p * W + c] : 0ull;       // suppressed by p inside its chunk
            const int idx = have ? w.rank2idx[p] : 0;
            u64 kept = chunk_decide(own, n, c, s_rem[c]);
            // post cap: the first post_max - nk kept boxes of the chunk (nk < post_max here)
            const int before = __builtin_popcountll(kept & ((1ull << lane) - 1ull));
            const bool mine = ((kept >> lane) & 1ull) && before < post_max - nk;
            kept = __ballot(mine);
            if (mine) {
                od[nk + before] = idx;
                kp[idx] = 1;
            }
            if (lane == 0) s_kept = kept;
        }
        __syncthreads();
        const u64 kept = s_kept;
        nk += __builtin_popcountll(kept);
        if (nk >= post_max) break;                               // (uniform)
        const int k = c + 1 + tid;
        if (k < nch && kept != 0ull) {
            const size_t r0 = (size_t)(64 * c + __builtin_ctzll(kept)) * W + k;    // a kept row: a valid address for the idle slots
            u64 acc = 0ull;
            for (int i0 = 0; i0 < 64; i0 += 16) {
                if (((kept >> i0) & 0xFFFFull) == 0ull) continue;
                u64 v[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const bool on = (kept >> (i0 + j)) & 1ull;
                    v[j] = w.mask[on ? (size_t)(64 * c + i0 + j) * W + k : r0];
                    if (!on) v[j] = 0ull;
                }
#pragma unroll
                for (int j = 0; j < 16; ++j) acc |= v[j];
            }
            s_rem[k] |= acc;
        }
        __syncthreads();
    }
    if (tid == 0) count[blockIdx.x] = nk;
}

inline int nmsx_P(int K, int pre_max) { return K < pre_max ? K : pre_max; }

}  // namespace

SAD_API size_t sad_nms_boxes_workspace_bytes(int B, int K, int pre_max) {
    if (B < 1 || B > 65535 || K < 1 || pre_max < 1 || (long long)B * K >= (1ll << 31)) return 0;
    const int P = nmsx_P(K, pre_max);
    if (P > NMSX_MAXP) return 0;
    return (size_t)B * NmsxLayout::scene_bytes(P);
}

SAD_API int sad_nms_boxes_f32(const float *boxes, int D, const float *scores, const int32_t *labels, int B, int K,
                              float iou_thr, float score_thr, int pre_max, int post_max, int32_t *keep, int32_t *order,
                              int32_t *count, void *workspace, sad_stream_t stream) {
    SAD_REQUIRE(boxes && scores && keep && order && count && workspace, "sad_nms_boxes_f32: NULL pointer");
    SAD_REQUIRE(D >= 7, "sad_nms_boxes_f32: box rows need D >= 7 floats (cx,cy,cz,l,w,h,yaw), got D=%d", D);
    SAD_REQUIRE(B >= 1 && B <= 65535 && K >= 1, "sad_nms_boxes_f32: need 1 <= B <= 65535, K >= 1");
    SAD_REQUIRE(pre_max >= 1 && post_max >= 1, "sad_nms_boxes_f32: need pre_max >= 1 and post_max >= 1 (pass K for no limit)");
    SAD_REQUIRE((uintptr_t)workspace % 16 == 0, "sad_nms_boxes_f32: workspace must be 16-byte aligned");
    if ((long long)B * K >= (1ll << 31)) return sad::fail(SAD_EUNSUPPORTED, "sad_nms_boxes_f32: B*K=%lld >= 2^31", (long long)B * K);
    const int P = nmsx_P(K, pre_max);
    if (P > NMSX_MAXP)
        return sad::fail(SAD_EUNSUPPORTED, "sad_nms_boxes_f32: min(K, pre_max)=%d > %d (set pre_max)", P, NMSX_MAXP);
    const int Pout = P < post_max ? P : post_max;
    hipStream_t st = (hipStream_t)stream;
    if (K <= 4096)
        hipLaunchKernelGGL((nmsx_select_kernel<256>), dim3(B), dim3(256), 0, st, scores, K, P, Pout, score_thr, keep, order, workspace);
    else
        hipLaunchKernelGGL((nmsx_select_kernel<1024>), dim3(B), dim3(1024), 0, st, scores, K, P, Pout, score_thr, keep, order, workspace);
    hipLaunchKernelGGL(nmsx_rank_kernel, dim3((P + 255) / 256, B), dim3(256), 0, st, boxes, D, labels, K, P, workspace);
    hipLaunchKernelGGL(nms_mask_kernel<NmsxLayout>, dim3((P + NMS_ROWS_PER_WG - 1) / NMS_ROWS_PER_WG, B), dim3(256), 0, st, P, iou_thr,
                       labels ? 1 : 0, workspace);
    hipLaunchKernelGGL(nmsx_walk_kernel, dim3(B), dim3(256), 0, st, K, P, Pout, post_max, keep, order, count, workspace);
    return sad::check_launch("sad_nms_boxes_f32");
}
