// COCO-protocol matching of detections to ground truth for a whole test split in one launch.
//
// Replaces, for evaluation.coco_eval_bbox(device=...) (CocoDataset.evaluate / CityscapesDataset.evaluate 'bbox', EvalHook,
// test_robustness.py):
//   pycocotools cocoeval.py  COCOeval.evaluateImg - the greedy, score-ordered matching of one (image, category) with crowd
//                            regions and per-area-range "ignore" sets, once per area range, ten thresholds each -
//   pycocotools maskApi      bbIou (maskUtils.iou on [x, y, w, h] boxes, intersection over the detection's area for a crowd),
// as evaluation._evaluate_img / _iou_xywh restate them (the host path and the yardstick of tests/test_hip_coco_eval.py).
// A segment is one (image, category) pair: its detections dets[det_off[s] .. det_off[s+1]) in descending score order and its
// boxes gts[gt_off[s] .. gt_off[s+1]) in annotation order.
//
// One single-wave workgroup per segment (a Cityscapes segment holds 0 - 20 detections and 0 - 30 boxes: the launch is
// latency-bound, and with one wave every barrier is free and all control flow below is uniform over the workgroup).
//   lane l < n_thr * n_area owns ONE matching: area range l / n_thr, threshold l % n_thr - row l of the outputs.  The greedy
//   order is a true dependency, so a lane walks the detections one after the other; the 40 matchings of the protocol run
//   side by side.
//   shared by all lanes, computed by all 64: per detection the fp64 IoU row against the boxes (one box per lane and pass, in
//   the host's operation order: the library is built with -ffp-contract=off, fp64 division is correctly rounded, min / max
//   propagate NaN as numpy's do), and per box the 64-bit mask "ignored in lane l's area range".
//   per lane: the best non-ignored and the best ignored candidate of the walk in annotation order, each updated on
//   iou >= best (the later box wins among equals); the ignored one counts only when there is no non-ignored one - the
//   single pass equivalent of the host's walk over the boxes sorted by their ignore flag.  "Taken" is one bit per (box,
//   lane) in a 64-bit word per box; a crowd is never marked taken.
// A segment of at most LDS_GTS boxes stages boxes, masks and taken-words in LDS once.  A larger one walks its boxes in chunks
// of LDS_GTS per detection and keeps the taken-words in the caller's workspace (the slice of the segment's own boxes: only
// this workgroup touches it, it zeroes it itself).  Detections pass through LDS LDS_DETS at a time.
// LDS: 4 KB boxes + 1 KB IoU row + 1 KB ignore masks + 1 KB taken words + 2 KB detections: 9.1 KB, 17 workgroups per CU by LDS.
// Every offset read from the device arrays is clamped to [0, n_det] / [0, n_gt] before it indexes anything.
#include "common.h"
#include "oadg_hip.h"

namespace {

constexpr int THREADS = 64;                    // one wave
constexpr int LANES = OADG_COCO_MAX_LANES;
constexpr int LDS_GTS = OADG_COCO_LDS_GTS;     // boxes of a segment staged at once
constexpr int LDS_DETS = OADG_COCO_LDS_DETS;   // detections staged at once
static_assert(LANES == THREADS && LDS_DETS <= THREADS, "one lane per matching, one lane per staged detection");
typedef unsigned long long u64;

struct Params {
    double thr[LANES];       // [n_thr]
    double lo[LANES];        // [n_area]
    double hi[LANES];
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// numpy's minimum / maximum: a NaN operand is the result
__device__ __forceinline__ double np_min(double a, double b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }
__device__ __forceinline__ double np_max(double a, double b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

__global__ __launch_bounds__(THREADS) void coco_match_kernel(const double* __restrict__ dets, const int* __restrict__ det_off,
                                                             const double* __restrict__ gts,
                                                             const double* __restrict__ gt_area,
                                                             const uint8_t* __restrict__ gt_crowd,
                                                             const int* __restrict__ gt_off, int n_det, int n_gt, Params p,
                                                             int n_thr, int n_area, uint8_t* __restrict__ flags,
                                                             int* __restrict__ match, u64* ws) {
    __shared__ double sbox[LDS_GTS][4];
    __shared__ double sdet[LDS_DETS][4];
    __shared__ double siou[LDS_GTS];
    __shared__ u64 sign[LDS_GTS];              // bit l: the box is ignored in lane l's area range
    __shared__ u64 staken[LDS_GTS];            // bit l: the box is matched in lane l's matching (never set for a crowd)
    __shared__ uint8_t scrowd[LDS_GTS];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int d0 = clampi(det_off[s], 0, n_det), d1 = clampi(det_off[s + 1], d0, n_det);
    const int g0 = clampi(gt_off[s], 0, n_gt), g1 = clampi(gt_off[s + 1], g0, n_gt);
    const int nd = d1 - d0, ng = g1 - g0;
    if (nd == 0) return;                                             // (uniform: the whole workgroup leaves)
    const bool active = tid < n_thr * n_area;
    const int a = active ? tid / n_thr : 0, t = active ? tid % n_thr : 0;
    const double thr = p.thr[t], lo = p.lo[a], hi = p.hi[a];
    const u64 tmask = n_thr >= 64 ? ~0ull : (1ull << n_thr) - 1ull, bit = 1ull << tid;
    const bool one = ng <= LDS_GTS;                                  // the whole segment is staged once
    if (!one) {
        for (int j = tid; j < ng; j += THREADS) ws[g0 + j] = 0ull;
        __threadfence();
        __syncthreads();
    }
    // boxes [c0, c0 + cn) of the segment -> LDS, with their ignore masks and taken words
    auto stage = [&](int c0, int cn) {
        for (int j = tid; j < cn; j += THREADS) {
            const size_t g = (size_t)g0 + c0 + j;
            for (int k = 0; k < 4; ++k) sbox[j][k] = gts[g * 4 + k];
            const double ar = gt_area[g];
            const bool crowd = gt_crowd[g] != 0;
            u64 ig = 0ull;
            for (int r = 0; r < n_area; ++r)
                if (crowd || ar < p.lo[r] || ar > p.hi[r]) ig |= tmask << (r * n_thr);
            sign[j] = ig;
            scrowd[j] = crowd;
            staken[j] = one ? 0ull : __hip_atomic_load(&ws[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    };
    if (one) stage(0, ng);                                           // (the barrier behind the first IoU row covers it)
    for (int base = 0; base < nd; base += LDS_DETS) {
        const int bn = nd - base < LDS_DETS ? nd - base : LDS_DETS;
        __syncthreads();                                             // the previous detections have been read by every lane
        if (tid < bn)
            for (int k = 0; k < 4; ++k) sdet[tid][k] = dets[((size_t)d0 + base + tid) * 4 + k];
        __syncthreads();
        for (int i = 0; i < bn; ++i) {
            const double dx = sdet[i][0], dy = sdet[i][1], dw = sdet[i][2], dh = sdet[i][3];
            const double da = dw * dh;
            double best_reg = thr, best_ign = thr;
            int m_reg = -1, m_ign = -1;
            bool m_ign_crowd = false;
            for (int c0 = 0; c0 < ng; c0 += LDS_GTS) {
                const int cn = ng - c0 < LDS_GTS ? ng - c0 : LDS_GTS;
                if (!one) {
                    stage(c0, cn);                                   // (the previous chunk was released by the barrier below)
                    __syncthreads();
                }
                for (int j = tid; j < cn; j += THREADS) {
                    const double gx = sbox[j][0], gy = sbox[j][1], gw = sbox[j][2], gh = sbox[j][3];
                    const double iw = np_min(dx + dw, gx + gw) - np_max(dx, gx);
                    const double ih = np_min(dy + dh, gy + gh) - np_max(dy, gy);
                    const double inter = np_max(iw, 0.0) * np_max(ih, 0.0);
                    const double ga = gw * gh;
                    const double uni = scrowd[j] ? da : (da + ga) - inter;
                    siou[j] = uni > 0.0 ? inter / uni : 0.0;
                }
                __syncthreads();
                if (active) {
                    for (int j = 0; j < cn; ++j) {
                        if ((staken[j] >> tid) & 1ull) continue;
                        const double iou = siou[j];
                        if ((sign[j] >> tid) & 1ull) {
                            if (!(iou < best_ign)) { best_ign = iou; m_ign = c0 + j; m_ign_crowd = scrowd[j] != 0; }
                        } else if (!(iou < best_reg)) { best_reg = iou; m_reg = c0 + j; }
                    }
                }
                __syncthreads();                                     // the row and the chunk have been read by every lane
            }
            if (active) {
                const int m = m_reg >= 0 ? m_reg : m_ign;
                uint8_t f;
                if (m < 0) f = (da < lo || da > hi) ? 2 : 0;
                else f = m_reg >= 0 ? 1 : 2;
                if (m >= 0 && !(m_reg < 0 && m_ign_crowd)) {
                    if (one) atomicOr(&staken[m], bit);
                    else atomicOr(&ws[(size_t)g0 + m], bit);
                }
                const size_t o = (size_t)tid * n_det + d0 + base + i;
                flags[o] = f;
                if (match) match[o] = m;
            }
            if (!one) {                                              // the taken bits are at the device before the next staging
                __threadfence();
                __syncthreads();
            }
        }
    }
}

}  // namespace

extern "C" size_t oadg_coco_match_workspace_bytes(int n_seg, int n_det, int n_gt, int n_thr, int n_area) {
    if (n_seg < 0 || n_det < 0 || n_gt < 0 || n_thr < 1 || n_area < 1 || n_thr > LANES || n_area > LANES ||
        n_thr * n_area > LANES)
        return 0;
    const size_t b = (size_t)n_gt * sizeof(u64);
    return b < 8 ? 8 : b;
}

extern "C" int oadg_coco_match(const double* dets, const int32_t* det_off, const double* gts, const double* gt_area,
                               const uint8_t* gt_crowd, const int32_t* gt_off, int n_seg, int n_det, int n_gt,
                               const double* iou_thrs_host, int n_thr, const double* area_rng_host, int n_area,
                               uint8_t* flags, int32_t* match, void* workspace, size_t workspace_bytes, void* stream) {
    const size_t need = oadg_coco_match_workspace_bytes(n_seg, n_det, n_gt, n_thr, n_area);
    if (need == 0 || !iou_thrs_host || !area_rng_host) return OADG_EARG;
    if (n_seg > 0 && (!det_off || !gt_off)) return OADG_EARG;
    if (n_det > 0 && (!dets || ((uintptr_t)dets & 7) || !flags || ((uintptr_t)match & 3))) return OADG_EARG;
    if (n_gt > 0 && (!gts || ((uintptr_t)gts & 7) || !gt_area || ((uintptr_t)gt_area & 7) || !gt_crowd)) return OADG_EARG;
    if (!workspace || ((uintptr_t)workspace & 7)) return OADG_EARG;
    if (workspace_bytes < need) return OADG_ESIZE;
    if (n_seg == 0 || n_det == 0) return OADG_OK;
    Params p;
    for (int k = 0; k < LANES; ++k) {
        p.thr[k] = k < n_thr ? iou_thrs_host[k] : 2.0;
        p.lo[k] = k < n_area ? area_rng_host[2 * k] : 0.0;
        p.hi[k] = k < n_area ? area_rng_host[2 * k + 1] : 0.0;
    }
    coco_match_kernel<<<dim3((unsigned)n_seg), dim3(THREADS), 0, (hipStream_t)stream>>>(
        dets, det_off, gts, gt_area, gt_crowd, gt_off, n_det, n_gt, p, n_thr, n_area, flags, match, (u64*)workspace);
    OADG_LAUNCH_CHECK();
    return OADG_OK;
}
