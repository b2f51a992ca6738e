// Detection evaluation (SPEC.md §36): the score-ordered assignment of detections to ground truth (det_match) and
// precision / recall / AP over everything accumulated (det_ap_keys + det_ap).  The pair value of the IoU metrics is §19.3's,
// through box_geom.h's one definition per formula, so it equals sad_boxes_iou_f32 bit for bit.
//
// det_match: ONE workgroup per scene, four waves.  The workgroup stages the footprints of the scene's valid ground-truth boxes
// in LDS (box_footprint3d; the centres alone for the distance metric) and ranks the live detections with an O(K^2) counting rank
// (§23's rule, as nms_core.h's rank_candidates: the live test replaces the score threshold).  Then ONE WAVE takes each class
// of the scene (classes dealt round robin), so there is no barrier inside the walk: it visits the ranking 64 ranks at a time
// (a ballot picks its class), and per detection its lanes hold the ground-truth boxes, 64 per trip.  The boxes are not
// compacted by class: a trip without a box of the class is skipped on a ballot, and at evaluation sizes (G of a few dozen) a
// class's boxes fill one trip either way.  The clip of a pair is computed once and shared by all T thresholds; per threshold a
// lane keeps its best (ordered value bits, ~g) key over the trips, one for the boxes that count and one for the ignored ones,
// and one wave_max_u64 each decides.  The taken set is one int of T bits per box in LDS, touched only by the lane that holds the
// box (g & 63), as is the box's gt_det row in memory: same thread, same address, program order.  No [K,G] matrix, no workspace,
// no atomics of any kind; every output element is stored by exactly one thread.
//
// det_ap: rows are visited through the permutation of ONE stable sort on det_ap_keys' composite key (class, descending score),
// so class c is a segment found by two binary searches.  One workgroup per (c, t): an integer count of the segment gives the
// totals, then a REVERSE walk in chunks of 256 rows with the counts and the running maximum carried: row i's tp_i / fp_i are
// total - (what lies behind it), its envelope is the maximum of the precisions from i on, so no per-row buffer exists.  The
// sample of recall position k is the envelope at the true positive whose running count is m_k, the smallest count whose recall
// reaches r_k (found per k by bisection on the same float expression); that row stores it.
#include "box_geom.h"

namespace {

#include "prims.h"       // u64, wave_max_u64

constexpr int DM_THREADS = 256;
constexpr int DM_MAXK = 1024, DM_MAXG = 1024, DM_MAXC = 64, DM_MAXT = 8;
constexpr int DM_POLY = 4 * 10 * DM_THREADS;            // floats of clipping scratch, thread-interleaved
constexpr int AP_THREADS = 256;
constexpr int AP_MAXP = 128;

struct MatchParams {
    const float *det_boxes, *det_scores;
    const int32_t *det_labels, *det_count;
    const float *gt_boxes;
    const int32_t *gt_labels, *gt_ignore;
    const float *thr;
    int K, D, G, Dg, C, T, metric;
    int32_t *code, *match;
    float *value;
    int32_t *gt_det, *n_gt;
};

// dynamic LDS of det_match_kernel, in 4-byte words: the clipping scratch, the detections (score, class or -1, rank -> index),
// the boxes (class or -1, ignore, taken bits) and, for the IoU metrics, 13 words of footprint per box (centre only: 2)
__host__ __device__ inline size_t dm_lds_words(int K, int G, int metric) {
    return (size_t)(metric == SAD_DET_DIST ? 0 : DM_POLY) + 3 * (size_t)K + 3 * (size_t)G + (size_t)(metric == SAD_DET_DIST ? 2 : 13) * G + 4;
}

__global__ __launch_bounds__(DM_THREADS) void det_match_kernel(MatchParams p) {
    extern __shared__ float s_dyn[];
    const int K = p.K, G = p.G, C = p.C, T = p.T;
    const bool dist = p.metric == SAD_DET_DIST;
    float *s_poly = s_dyn;
    float *s_score = s_poly + (dist ? 0 : DM_POLY);
    int *s_lab = (int *)(s_score + K);
    int *s_rank2idx = s_lab + K;
    int *s_glab = s_rank2idx + K;
    int *s_gign = s_glab + G;
    int *s_taken = s_gign + G;
    int *s_n = s_taken + G;
    float *s_gf = (float *)(s_n + 4);                    // [13][G] (IoU metrics) or [2][G]: ctr x, ctr y, corners x4, y4, z, h, measure
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x;
    const float *db = p.det_boxes + (size_t)b * K * p.D;
    int nb = p.det_count ? p.det_count[b] : K;
    nb = nb < 0 ? 0 : (nb > K ? K : nb);

    // 1. stage: detections (rows beyond nb are never read), boxes; the outputs of the rows no wave will visit
    for (int k = tid; k < K; k += DM_THREADS) {
        int lab = -1;
        float sc = 0.0f;
        if (k < nb) {
            lab = p.det_labels[(size_t)b * K + k];
            sc = p.det_scores[(size_t)b * K + k];
            if (lab < 0 || lab >= C) lab = -1;
        }
        s_lab[k] = lab;
        s_score[k] = sc;
        if (lab < 0) {
            const size_t o = ((size_t)b * K + k) * T;
            for (int t = 0; t < T; ++t) { p.code[o + t] = -1; p.match[o + t] = -1; p.value[o + t] = 0.0f; }
        }
    }
    for (int g = tid; g < G; g += DM_THREADS) {
        int lab = p.gt_labels[(size_t)b * G + g];
        if (lab < 0 || lab >= C) lab = -1;
        s_glab[g] = lab;
        s_gign[g] = p.gt_ignore ? (p.gt_ignore[(size_t)b * G + g] != 0) : 0;
        s_taken[g] = 0;
        if (lab < 0) {
            const size_t o = ((size_t)b * G + g) * T;
            for (int t = 0; t < T; ++t) p.gt_det[o + t] = -1;
        } else {
            const float *bx = p.gt_boxes + ((size_t)b * G + g) * p.Dg;
            if (dist) {
                s_gf[g] = bx[0]; s_gf[G + g] = bx[1];
            } else {
                float cx[4], cy[4], ctr[2], z, h, vol;
                box_footprint3d(bx, cx, cy, ctr, z, h, vol);
                s_gf[g] = ctr[0]; s_gf[G + g] = ctr[1];
#pragma unroll
                for (int q = 0; q < 4; ++q) { s_gf[(2 + q) * G + g] = cx[q]; s_gf[(6 + q) * G + g] = cy[q]; }
                s_gf[10 * G + g] = z; s_gf[11 * G + g] = h;
                s_gf[12 * G + g] = p.metric == SAD_DET_IOU3D ? vol : bx[3] * bx[4];
            }
        }
    }
    __syncthreads();

    // 2. rank the live detections: score descending, index ascending (floats compared as floats: -0 and +0 tie)
    int nloc = 0;
    for (int i = tid; i < K; i += DM_THREADS) {
        if (s_lab[i] < 0) continue;
        const float si = s_score[i];
        int r = 0;
        for (int j = 0; j < K; ++j) {
            const float sj = s_score[j];
            r += (s_lab[j] >= 0) && (sj > si || (sj == si && j < i));
        }
        s_rank2idx[r] = i;
        ++nloc;
    }
    nloc = wave_count(nloc);
    if (lane == 0) s_n[wave] = nloc;
    __syncthreads();
    const int n = ((s_n[0] + s_n[1]) + s_n[2]) + s_n[3];

    // 3. the walk: one wave per class
    for (int c = wave; c < C; c += DM_THREADS / 64) {
        float thr[DM_MAXT];
#pragma unroll
        for (int t = 0; t < DM_MAXT; ++t) thr[t] = t < T ? p.thr[c * T + t] : 0.0f;
        // the class's boxes: gt_det rows start at -1 (stored by the lane that may store a detection there later), n_gt
        int ngt = 0;
        for (int g0 = 0; g0 < G; g0 += 64) {
            const int g = g0 + lane;
            const bool mine = g < G && s_glab[g] == c;
            if (mine) {
                const size_t o = ((size_t)b * G + g) * T;
                for (int t = 0; t < T; ++t) p.gt_det[o + t] = -1;
            }
            ngt += __builtin_popcountll(__ballot(mine && !s_gign[g]));
        }
        if (lane == 0) p.n_gt[(size_t)b * C + c] = ngt;

        for (int r0 = 0; r0 < n; r0 += 64) {
            const int r = r0 + lane;
            const int kr = r < n ? s_rank2idx[r] : -1;
            u64 todo = __ballot(kr >= 0 && s_lab[kr] == c);
            while (todo) {
                const int j = __builtin_amdgcn_readfirstlane(__builtin_ctzll(todo));
                todo &= todo - 1ull;
                const int k = __builtin_amdgcn_readlane(kr, j);
                // the detection's footprint (wave-uniform: every lane computes the same)
                const float *bx = db + (size_t)k * p.D;
                float acx[4], acy[4], actr[2], az = 0.0f, ah = 0.0f, ameas = 0.0f;
                if (dist) {
                    actr[0] = bx[0]; actr[1] = bx[1];
                } else {
                    float vol;
                    box_footprint3d(bx, acx, acy, actr, az, ah, vol);
                    ameas = p.metric == SAD_DET_IOU3D ? vol : bx[3] * bx[4];
                }
                u64 bestn[DM_MAXT], besti[DM_MAXT];
#pragma unroll
                for (int t = 0; t < DM_MAXT; ++t) { bestn[t] = 0ull; besti[t] = 0ull; }
                for (int g0 = 0; g0 < G; g0 += 64) {
                    const int g = g0 + lane;
                    const bool mine = g < G && s_glab[g] == c;
                    if (!__ballot(mine)) continue;                      // (wave-uniform)
                    if (mine) {
                        float v;
                        const float bc0 = s_gf[g], bc1 = s_gf[G + g];
                        if (dist) {
                            const float dx = actr[0] - bc0, dy = actr[1] - bc1;
                            v = sqrtf((dx * dx) + (dy * dy));
                        } else {
                            float qcx[4], qcy[4];
#pragma unroll
                            for (int q = 0; q < 4; ++q) { qcx[q] = s_gf[(2 + q) * G + g]; qcy[q] = s_gf[(6 + q) * G + g]; }
                            float inter = poly_clip_area<DM_THREADS>(acx, acy, actr[0] - bc0, actr[1] - bc1, qcx, qcy, s_poly + tid);
                            if (p.metric == SAD_DET_IOU3D) inter = inter * height_overlap(ah, s_gf[11 * G + g], az, s_gf[10 * G + g]);
                            v = iou_of(inter, ameas, s_gf[12 * G + g]);
                        }
                        // v >= +0: its bits order like the value; better = larger (IoU) / smaller (distance), then the lower g
                        const unsigned vb = __builtin_bit_cast(unsigned, v);
                        const u64 key = ((u64)(dist ? ~vb : vb) << 32) | (unsigned)~g;
                        const int taken = s_taken[g];
                        const bool ign = s_gign[g] != 0;
#pragma unroll
                        for (int t = 0; t < DM_MAXT; ++t) {
                            const bool acc = t < T && (dist ? v < thr[t] : v > thr[t]);
                            if (acc && ign) besti[t] = umax64(besti[t], key);
                            if (acc && !ign && !((taken >> t) & 1)) bestn[t] = umax64(bestn[t], key);
                        }
                    }
                }
                const size_t o = ((size_t)b * K + k) * T;
#pragma unroll
                for (int t = 0; t < DM_MAXT; ++t) {
                    if (t >= T) break;
                    const u64 kn = wave_max_u64(bestn[t]);
                    const u64 kw = kn ? kn : wave_max_u64(besti[t]);
                    const int g = kw ? (int)~(unsigned)kw : -1;
                    const unsigned vb = dist ? ~(unsigned)(kw >> 32) : (unsigned)(kw >> 32);
                    if (kn && lane == (g & 63)) {
                        s_taken[g] |= 1 << t;
                        p.gt_det[((size_t)b * G + g) * T + t] = k;
                    }
                    if (lane == 0) {
                        p.code[o + t] = kn ? 1 : (kw ? -1 : 0);
                        p.match[o + t] = g;
                        p.value[o + t] = kw ? __builtin_bit_cast(float, vb) : 0.0f;
                    }
                }
            }
        }
    }
}

// ---- AP ------------------------------------------------------------------------------------------------------------------
// the composite sort key of a row: (class, or C for a row of no class) << 32 | descending-ordered score bits; -0 sorts as +0
__global__ __launch_bounds__(256) void det_ap_keys_kernel(const float *__restrict__ scores, const int32_t *__restrict__ labels,
                                                          long long N, int C, long long *__restrict__ keys) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float s = scores[i] + 0.0f;
    const unsigned u = __builtin_bit_cast(unsigned, s);
    const unsigned asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    const int lab = labels[i];
    const long long cls = (lab < 0 || lab >= C) ? C : lab;
    keys[i] = (cls << 32) | (long long)(unsigned)~asc;
}

__device__ __forceinline__ long long ap_lower_bound(const long long *keys, long long N, long long key) {
    long long lo = 0, hi = N;
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

struct ApParams {
    const long long *keys, *perm;        // sorted keys and the permutation that sorted them
    const int32_t *code, *n_gt;
    long long N;
    int C, T, points, first;
    float floor;
    float *ap, *prec, *max_recall;
    int32_t *n_det;
};

// grid (T, C)
__global__ __launch_bounds__(AP_THREADS) void det_ap_kernel(ApParams p) {
    __shared__ int s_m[AP_MAXP + 1];             // m_k: the smallest true-positive count whose recall reaches r_k
    __shared__ float s_s[AP_MAXP + 1];           // the samples
    __shared__ int s_cnt[2][AP_THREADS / 64];
    __shared__ float s_max[AP_THREADS / 64];
    const int t = blockIdx.x, c = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = p.T, P = p.points - p.first + 1;
    const int ngt = p.n_gt[c];
    const long long lo = ap_lower_bound(p.keys, p.N, (long long)c << 32), hi = ap_lower_bound(p.keys, p.N, (long long)(c + 1) << 32);
    const float fng = (float)ngt;

    // totals of the segment
    int tp = 0, fp = 0;
    for (long long i = lo + tid; i < hi; i += AP_THREADS) {
        const int cd = p.code[(size_t)p.perm[i] * T + t];
        tp += cd == 1; fp += cd == 0;
    }
    tp = wave_count(tp); fp = wave_count(fp);
    if (lane == 0) { s_cnt[0][wave] = tp; s_cnt[1][wave] = fp; }
    for (int k = tid; k <= AP_MAXP; k += AP_THREADS) {
        s_s[k] = 0.0f;
        int m = 0x7FFFFFFF;
        if (k >= p.first && k <= p.points && ngt > 0) {
            const float rk = (float)k / (float)p.points;
            int a = 0, z = ngt;                  // (float)z / fng = 1 >= rk holds
            while (a < z) {
                const int mid = a + ((z - a) >> 1);
                if ((float)mid / fng >= rk) z = mid; else a = mid + 1;
            }
            m = a;
        }
        s_m[k] = m;
    }
    __syncthreads();
    const int TP = ((s_cnt[0][0] + s_cnt[0][1]) + s_cnt[0][2]) + s_cnt[0][3];
    const int FP = ((s_cnt[1][0] + s_cnt[1][1]) + s_cnt[1][2]) + s_cnt[1][3];

    // the reverse walk (nothing to sample without ground truth)
    int tp_after = 0, fp_after = 0;
    float env_after = 0.0f;
    for (long long end = hi; end > lo && ngt > 0; end -= AP_THREADS) {
        __syncthreads();                         // the previous chunk's wave sums are read
        const long long i = end - AP_THREADS + tid;
        const int cd = i >= lo ? p.code[(size_t)p.perm[i] * T + t] : -1;
        const bool is_tp = cd == 1, is_fp = cd == 0;
        const u64 mt = __ballot(is_tp), mf = __ballot(is_fp);
        const u64 above = lane == 63 ? 0ull : (~0ull << (lane + 1));
        if (lane == 0) { s_cnt[0][wave] = __builtin_popcountll(mt); s_cnt[1][wave] = __builtin_popcountll(mf); }
        __syncthreads();
        int tb = tp_after + __builtin_popcountll(mt & above), fb = fp_after + __builtin_popcountll(mf & above);   // counts behind the row
        for (int w = wave + 1; w < AP_THREADS / 64; ++w) { tb += s_cnt[0][w]; fb += s_cnt[1][w]; }
        const int tpi = TP - tb, fpi = FP - fb;
        const float pr = (is_tp || is_fp) ? (float)tpi / (float)(tpi + fpi) : 0.0f;
        // suffix maximum over the chunk (max is exact: any order gives the same bits), then what lies behind the chunk
        float e = pr;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const float o = __shfl_down(e, off);
            if (lane + off < 64) e = fmaxf(e, o);
        }
        if (lane == 0) s_max[wave] = e;
        __syncthreads();
        for (int w = wave + 1; w < AP_THREADS / 64; ++w) e = fmaxf(e, s_max[w]);
        e = fmaxf(e, env_after);
        if (is_tp) {
            // every k whose m_k is this row's count (m_k is non-decreasing in k)
            for (int k = p.first; k <= p.points; ++k)
                if (s_m[k] == tpi) s_s[k] = e;
        }
        env_after = fmaxf(fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3])), env_after);
        tp_after += ((s_cnt[0][0] + s_cnt[0][1]) + s_cnt[0][2]) + s_cnt[0][3];
        fp_after += ((s_cnt[1][0] + s_cnt[1][1]) + s_cnt[1][2]) + s_cnt[1][3];
    }
    __syncthreads();
    // m_k == 0 (r_k == 0): the first counted row, whose envelope is the maximum of all
    const size_t o = (size_t)c * T + t;
    for (int k = tid; k < P; k += AP_THREADS) {
        const int kk = p.first + k;
        float s = s_s[kk];
        if (ngt > 0 && s_m[kk] == 0 && TP + FP > 0) s = env_after;
        s_s[kk] = s;
        p.prec[o * P + k] = s;
    }
    __syncthreads();
    if (tid == 0) {
        float ap = -1.0f;
        if (ngt > 0) {
            float sum = 0.0f;
            for (int k = p.first; k <= p.points; ++k) sum = sum + fmaxf(s_s[k] - p.floor, 0.0f);
            ap = sum / ((float)P * (1.0f - p.floor));
        }
        p.ap[o] = ap;
        p.max_recall[o] = ngt > 0 ? (float)TP / fng : 0.0f;
        p.n_det[o] = TP + FP;
    }
}

}  // namespace

SAD_API int sad_det_match_f32(const sad_det_match_args *a, sad_stream_t stream) {
    const char *fn = "sad_det_match_f32";
    if (const int rc = args_ok(fn, a)) return rc;
    SAD_REQUIRE(a->det_boxes && a->det_scores && a->det_labels && a->thr, "%s: NULL input pointer", fn);
    SAD_REQUIRE(a->code && a->match && a->value && a->n_gt, "%s: NULL output pointer", fn);
    SAD_REQUIRE(a->B >= 1 && a->K >= 1 && a->G >= 0, "%s: B, K >= 1 and G >= 0 expected (got %d, %d, %d)", fn, a->B, a->K, a->G);
    SAD_REQUIRE(a->D >= 7, "%s: detection rows need D >= 7 fields (got %d)", fn, a->D);
    SAD_REQUIRE(a->G == 0 || a->Dg >= 7, "%s: ground-truth rows need D >= 7 fields (got %d)", fn, a->Dg);
    SAD_REQUIRE(a->G == 0 || (a->gt_boxes && a->gt_labels && a->gt_det), "%s: G = %d needs gt_boxes, gt_labels and gt_det", fn, a->G);
    SAD_REQUIRE(a->metric == SAD_DET_IOU_BEV || a->metric == SAD_DET_IOU3D || a->metric == SAD_DET_DIST,
                "%s: metric must be 0 (BEV IoU), 1 (3-D IoU) or 2 (centre distance), got %d", fn, a->metric);
    SAD_REQUIRE(a->C >= 1 && a->T >= 1, "%s: C, T >= 1 expected (got %d, %d)", fn, a->C, a->T);
    if (a->K > DM_MAXK || a->G > DM_MAXG || a->C > DM_MAXC || a->T > DM_MAXT || a->B > 65535)
        return sad::fail(SAD_EUNSUPPORTED, "%s: K=%d, G=%d, C=%d, T=%d, B=%d beyond K <= %d, G <= %d, C <= %d, T <= %d, B <= 65535", fn,
                         a->K, a->G, a->C, a->T, a->B, DM_MAXK, DM_MAXG, DM_MAXC, DM_MAXT);
    MatchParams p;
    p.det_boxes = a->det_boxes; p.det_scores = a->det_scores; p.det_labels = a->det_labels; p.det_count = a->det_count;
    p.gt_boxes = a->gt_boxes; p.gt_labels = a->gt_labels; p.gt_ignore = a->G ? a->gt_ignore : nullptr; p.thr = a->thr;
    p.K = a->K; p.D = a->D; p.G = a->G; p.Dg = a->Dg; p.C = a->C; p.T = a->T; p.metric = a->metric;
    p.code = a->code; p.match = a->match; p.value = a->value; p.gt_det = a->gt_det; p.n_gt = a->n_gt;
    static std::atomic<uint64_t> attr_done{0};
    sad::lds_attr_once(attr_done, reinterpret_cast<const void *>(&det_match_kernel), 160 * 1024);
    const size_t lds = dm_lds_words(a->K, a->G, a->metric) * 4;
    hipLaunchKernelGGL(det_match_kernel, dim3(a->B), dim3(DM_THREADS), lds, (hipStream_t)stream, p);
    return sad::check_launch(fn);
}

SAD_API int sad_det_ap_keys_f32(const float *scores, const int32_t *labels, long long N, int C, long long *keys, sad_stream_t stream) {
    const char *fn = "sad_det_ap_keys_f32";
    SAD_REQUIRE(N >= 0 && C >= 1, "%s: N >= 0 and C >= 1 expected (got %lld, %d)", fn, N, C);
    SAD_REQUIRE(N == 0 || (scores && labels && keys), "%s: NULL pointer", fn);
    if (N >= (1LL << 31) || C > DM_MAXC) return sad::fail(SAD_EUNSUPPORTED, "%s: N=%lld, C=%d beyond N < 2^31, C <= %d", fn, N, C, DM_MAXC);
    if (N == 0) return SAD_OK;
    hipLaunchKernelGGL(det_ap_keys_kernel, dim3(sad::blocks_for((unsigned long long)N, 256)), dim3(256), 0, (hipStream_t)stream, scores,
                       labels, N, C, keys);
    return sad::check_launch(fn);
}

SAD_API int sad_det_ap_f32(const sad_det_ap_args *a, sad_stream_t stream) {
    const char *fn = "sad_det_ap_f32";
    if (const int rc = args_ok(fn, a)) return rc;
    SAD_REQUIRE(a->N >= 0 && a->C >= 1 && a->T >= 1, "%s: N >= 0 and C, T >= 1 expected (got %lld, %d, %d)", fn, a->N, a->C, a->T);
    SAD_REQUIRE(a->N == 0 || (a->keys && a->perm && a->code), "%s: NULL input pointer", fn);
    SAD_REQUIRE(a->n_gt && a->ap && a->prec && a->max_recall && a->n_det, "%s: NULL pointer", fn);
    SAD_REQUIRE(a->points >= 1 && a->first >= 0 && a->first <= a->points, "%s: 0 <= first <= points and points >= 1 expected (got %d, %d)",
                fn, a->first, a->points);
    SAD_REQUIRE(a->floor >= 0.0f && a->floor < 1.0f, "%s: floor must lie in [0, 1) (got %g)", fn, (double)a->floor);
    if (a->points > AP_MAXP || a->C > DM_MAXC || a->T > DM_MAXT || a->N * a->T >= (1LL << 31))
        return sad::fail(SAD_EUNSUPPORTED, "%s: points=%d, C=%d, T=%d, N=%lld beyond points <= %d, C <= %d, T <= %d, N*T < 2^31", fn,
                         a->points, a->C, a->T, a->N, AP_MAXP, DM_MAXC, DM_MAXT);
    ApParams p;
    p.keys = a->keys; p.perm = a->perm; p.code = a->code; p.n_gt = a->n_gt;
    p.N = a->N; p.C = a->C; p.T = a->T; p.points = a->points; p.first = a->first; p.floor = a->floor;
    p.ap = a->ap; p.prec = a->prec; p.max_recall = a->max_recall; p.n_det = a->n_det;
    hipLaunchKernelGGL(det_ap_kernel, dim3(a->T, a->C), dim3(AP_THREADS), 0, (hipStream_t)stream, p);
    return sad::check_launch(fn);
}
