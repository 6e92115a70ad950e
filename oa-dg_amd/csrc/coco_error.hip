// COCO error analysis: the plain matchings and the two "ignore confusion" matchings of a whole test split in one launch.
//
// Replaces, for evaluation.coco_error_analysis(device=...) (tools/analysis_tools/coco_error_analysis.py):
//   tools/analysis_tools/coco_error_analysis.py  analyze_results / analyze_individual_category of the reference - one COCOeval
//                            at IoU 0.75 / 0.5 / 0.1 plus, per class, two COCOevals at IoU 0.1 on a deep copy of the dataset in
//                            which the boxes of the other classes (of the same supercategory / of any class) are relabelled
//                            `ignore = 1, iscrowd = 1, category_id = catId`: 1 + 2 K evaluations of the split -
//   pycocotools cocoeval.py  COCOeval.evaluateImg and maskApi bbIou, as in csrc/coco_eval.hip,
// as evaluation.coco_error_flags_host restates them on evaluation._evaluate_img (the yardstick of tests/test_hip_coco_error.py).
// A segment is one (image, category k) pair, s = image * K + k: its detections dets[det_off[s] .. det_off[s+1]) in descending
// score order, and ALL boxes of the image, gts[img_off[i] .. img_off[i+1]) in annotation order, each with its own category.
// The boxes of an image are stored once, not once per category that relabels them.
//
// One single-wave workgroup per segment, as csrc/coco_eval.hip (every barrier is free, all control flow is uniform).
//   lane l < (n_thr + 2) * n_area owns ONE matching: area range l / (n_thr + 2), row l % (n_thr + 2) - row l of the output.
//   Rows 0 .. n_thr-1 are the plain matchings at thrs[t]; row n_thr ignores confusion inside the supercategory, row n_thr + 1
//   confusion with every class, both at sim_thr.
//   shared by all lanes, computed by all 64: per detection the fp64 IoU row against the boxes (the host's operation order,
//   -ffp-contract=off, NaN-propagating min / max).  A box has ONE IoU whatever the lane - plain for an own-class box that is
//   no crowd, intersection / detection area for an own-class crowd and for every foreign box (the relabelling makes it a crowd) -
//   and two 64-bit masks: "present in lane l's matching" and "ignored in lane l's matching".
//     own class:                        present everywhere, ignored iff crowd or area outside the lane's range
//     foreign, same supercategory:      present in rows n_thr and n_thr + 1, ignored there
//     foreign, another supercategory:   present in row n_thr + 1, ignored there
//   per lane: the single pass of csrc/coco_eval.hip over the boxes that are present (best non-ignored and best ignored
//   candidate, each updated on iou >= best; the ignored one counts only without a non-ignored one).
// Only own-class boxes that are no crowd are ever marked taken, and a box has one class: the workspace word of a box is read
// and written by ONE workgroup, the segment of the box's own class, although K segments stage the same boxes (the others
// take 0 for it without reading the word).
// An image of at most LDS_GTS boxes is staged once, taken words in LDS.  A larger one walks its boxes in chunks of LDS_GTS per
// detection and keeps its taken words in the workspace (zeroed here, by the owning workgroup).  Detections pass through LDS
// LDS_DETS at a time.
// LDS: 8 KB boxes + 2 KB IoU row + 3 x 2 KB masks and taken words + 256 B crowd + 2 KB detections: 18.3 KB, 8 workgroups per CU.
// Every offset and every category read from the device arrays is clamped before it indexes anything.
#include "common.h"
#include "oadg_hip.h"

namespace {

constexpr int THREADS = 64;                          // one wave
constexpr int LANES = OADG_COCO_MAX_LANES;           // matchings of one call
constexpr int LDS_GTS = OADG_COCO_ERROR_LDS_GTS;     // boxes of an image staged at once
constexpr int LDS_DETS = OADG_COCO_ERROR_LDS_DETS;   // detections staged at once
static_assert(LANES == THREADS && LDS_DETS <= THREADS, "one lane per matching, one lane per staged detection");
typedef unsigned long long u64;

struct Params {
    double thr[LANES];       // [n_thr + 2]: the plain thresholds, then sim_thr twice
    double lo[LANES];        // [n_area]
    double hi[LANES];
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// numpy's minimum / maximum: a NaN operand is the result
__device__ __forceinline__ double np_min(double a, double b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }
__device__ __forceinline__ double np_max(double a, double b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

__global__ __launch_bounds__(THREADS) void coco_error_kernel(const double* __restrict__ dets, const int* __restrict__ det_off,
                                                             const double* __restrict__ gts,
                                                             const double* __restrict__ gt_area,
                                                             const uint8_t* __restrict__ gt_crowd,
                                                             const int* __restrict__ gt_cat, const int* __restrict__ img_off,
                                                             const int* __restrict__ cat_super, int K, int n_det, int n_gt,
                                                             Params p, int n_thr, int n_area, uint8_t* __restrict__ flags,
                                                             u64* ws) {
    __shared__ double sbox[LDS_GTS][4];
    __shared__ double sdet[LDS_DETS][4];
    __shared__ double siou[LDS_GTS];
    __shared__ u64 spres[LDS_GTS];             // bit l: the box takes part in lane l's matching
    __shared__ u64 sign[LDS_GTS];              // bit l: the box is ignored in lane l's matching
    __shared__ u64 staken[LDS_GTS];            // bit l: the box is matched in lane l's matching (own class, no crowd, only)
    __shared__ uint8_t scrowd[LDS_GTS];        // the IoU is intersection / detection area; never taken
    const int s = blockIdx.x, tid = threadIdx.x;
    const int img = s / K, k = s % K;
    const int d0 = clampi(det_off[s], 0, n_det), d1 = clampi(det_off[s + 1], d0, n_det);
    const int g0 = clampi(img_off[img], 0, n_gt), g1 = clampi(img_off[img + 1], g0, n_gt);
    const int nd = d1 - d0, ng = g1 - g0;
    if (nd == 0) return;                                             // (uniform: the whole workgroup leaves)
    const int R = n_thr + 2;
    const bool active = tid < R * n_area;
    const int a = active ? tid / R : 0, r = active ? tid % R : 0;
    const double thr = p.thr[r], lo = p.lo[a], hi = p.hi[a];
    const u64 bit = 1ull << tid;
    // rows of one area range: all R of them, the two variant rows, the last row
    const u64 rows_all = R >= 64 ? ~0ull : (1ull << R) - 1ull, rows_sim = 3ull << n_thr, rows_oth = 2ull << n_thr;
    u64 every = 0ull, every_sim = 0ull, every_oth = 0ull;           // the same, over all area ranges
    for (int q = 0; q < n_area; ++q) {
        every |= rows_all << (q * R);
        every_sim |= rows_sim << (q * R);
        every_oth |= rows_oth << (q * R);
    }
    const int my_super = cat_super[k];
    const bool one = ng <= LDS_GTS;                                  // the whole image is staged once
    if (!one) {
        for (int j = tid; j < ng; j += THREADS)
            if (gt_cat[g0 + j] == k) ws[g0 + j] = 0ull;              // (this segment owns the words of its own class)
        __threadfence();
        __syncthreads();
    }
    // boxes [c0, c0 + cn) of the image -> LDS, with their masks and taken words
    auto stage = [&](int c0, int cn) {
        for (int j = tid; j < cn; j += THREADS) {
            const size_t g = (size_t)g0 + c0 + j;
            for (int c = 0; c < 4; ++c) sbox[j][c] = gts[g * 4 + c];
            const int cat = gt_cat[g];
            u64 pres, ig;
            bool crowd;
            if (cat == k) {
                const double ar = gt_area[g];
                crowd = gt_crowd[g] != 0;
                pres = every;
                ig = 0ull;
                for (int q = 0; q < n_area; ++q)
                    if (crowd || ar < p.lo[q] || ar > p.hi[q]) ig |= rows_all << (q * R);
            } else if (cat >= 0 && cat < K) {
                crowd = true;                                        // relabelled: iscrowd = 1, so ignored wherever present
                pres = cat_super[cat] == my_super ? every_sim : every_oth;
                ig = pres;
            } else {                                                 // no category of the split: in no matching
                crowd = true;
                pres = 0ull;
                ig = 0ull;
            }
            spres[j] = pres;
            sign[j] = ig;
            scrowd[j] = crowd;
            staken[j] = (one || cat != k) ? 0ull : __hip_atomic_load(&ws[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    };
    if (one) stage(0, ng);                                           // (the barrier behind the first IoU row covers it)
    for (int base = 0; base < nd; base += LDS_DETS) {
        const int bn = nd - base < LDS_DETS ? nd - base : LDS_DETS;
        __syncthreads();                                             // the previous detections have been read by every lane
        if (tid < bn)
            for (int c = 0; c < 4; ++c) sdet[tid][c] = dets[((size_t)d0 + base + tid) * 4 + c];
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
                        if (!((spres[j] >> tid) & 1ull) || ((staken[j] >> tid) & 1ull)) continue;
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
                if (m >= 0 && !(m_reg < 0 && m_ign_crowd)) {         // (own class and no crowd: this workgroup's word)
                    if (one) atomicOr(&staken[m], bit);
                    else atomicOr(&ws[(size_t)g0 + m], bit);
                }
                flags[(size_t)tid * n_det + d0 + base + i] = f;
            }
            if (!one) {                                              // the taken bits are at the device before the next staging
                __threadfence();
                __syncthreads();
            }
        }
    }
}

}  // namespace

extern "C" size_t oadg_coco_error_workspace_bytes(int n_img, int num_classes, int n_det, int n_gt, int n_thr, int n_area) {
    if (n_img < 0 || num_classes < 1 || n_det < 0 || n_gt < 0 || n_thr < 0 || n_area < 1 || n_thr > LANES || n_area > LANES ||
        (n_thr + 2) * n_area > LANES || (long long)n_img * num_classes > 2147483647LL)
        return 0;
    const size_t b = (size_t)n_gt * sizeof(u64);
    return b < 8 ? 8 : b;
}

extern "C" int oadg_coco_error_match(const double* dets, const int32_t* det_off, const double* gts, const double* gt_area,
                                     const uint8_t* gt_crowd, const int32_t* gt_cat, const int32_t* img_off,
                                     const int32_t* cat_super, int n_img, int num_classes, int n_det, int n_gt,
                                     const double* iou_thrs_host, int n_thr, double sim_thr, const double* area_rng_host,
                                     int n_area, uint8_t* flags, void* workspace, size_t workspace_bytes, void* stream) {
    const size_t need = oadg_coco_error_workspace_bytes(n_img, num_classes, n_det, n_gt, n_thr, n_area);
    if (need == 0 || (n_thr > 0 && !iou_thrs_host) || !area_rng_host) return OADG_EARG;
    if (!det_off || ((uintptr_t)det_off & 3) || !img_off || ((uintptr_t)img_off & 3) || !cat_super || ((uintptr_t)cat_super & 3))
        return OADG_EARG;
    if (n_det > 0 && (!dets || ((uintptr_t)dets & 7) || !flags)) return OADG_EARG;
    if (n_gt > 0 && (!gts || ((uintptr_t)gts & 7) || !gt_area || ((uintptr_t)gt_area & 7) || !gt_crowd || !gt_cat ||
                     ((uintptr_t)gt_cat & 3)))
        return OADG_EARG;
    if (!workspace || ((uintptr_t)workspace & 7)) return OADG_EARG;
    if (workspace_bytes < need) return OADG_ESIZE;
    if (n_img == 0 || n_det == 0) return OADG_OK;
    Params p;
    for (int k = 0; k < LANES; ++k) {
        p.thr[k] = k < n_thr ? iou_thrs_host[k] : (k < n_thr + 2 ? sim_thr : 2.0);
        p.lo[k] = k < n_area ? area_rng_host[2 * k] : 0.0;
        p.hi[k] = k < n_area ? area_rng_host[2 * k + 1] : 0.0;
    }
    coco_error_kernel<<<dim3((unsigned)(n_img * num_classes)), dim3(THREADS), 0, (hipStream_t)stream>>>(
        dets, det_off, gts, gt_area, gt_crowd, gt_cat, img_off, cat_super, num_classes, n_det, n_gt, p, n_thr, n_area, flags,
        (u64*)workspace);
    OADG_LAUNCH_CHECK();
    return OADG_OK;
}
