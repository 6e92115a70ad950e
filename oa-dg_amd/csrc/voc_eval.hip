// VOC-protocol matching of detections to ground truth for a whole test split in one launch.
//
// Replaces, for SdgodDataset.evaluate (evaluation.eval_map_voc):
//   mmdet/core/evaluation/mean_ap.py:357-380   pool.starmap(tpfp_default, ...) - one numpy problem per (image, class),
//   mmdet/core/evaluation/mean_ap.py:196-267   tpfp_default (area_ranges=None),
//   mmdet/core/evaluation/bbox_overlaps.py     bbox_overlaps (fp32, legacy "+ 1" extents or modern ones).
// A segment is one (image, class) pair: its detections dets[det_off[s] .. det_off[s+1]) and its boxes
// gts[gt_off[s] .. gt_off[s+1]), the first gt_reg[s] of them regular, the rest "ignore" regions (difficult objects).
//
// One single-wave workgroup per segment (most segments hold 0 - 20 detections and 0 - 10 boxes; the launch is latency-bound,
// and with one wave every barrier is free and all control flow below is uniform over the workgroup):
//   pass 1  each detection walks the segment's boxes, staged through LDS in chunks of CHUNK, computes the fp32 IoU in the
//           host's operation order (the library is built with -ffp-contract=off; the division is correctly rounded) and keeps
//           the largest value and the LOWEST index that attains it (numpy's max / argmax); per threshold, a detection with
//           iou_max >= thr whose best box is a regular one claims it with one 64-bit atomic min of
//           (~orderable(score) << 32) | index_in_segment.  The smallest key is the highest score, the lowest index among
//           equal scores - the stable descending order of the host - whatever the order of arrival.
//   pass 2  flags: 0 = best box is an ignored one, 1 = the winner of a regular box, 2 = everything else.
// The claim keys live in LDS when the segment has at most KEYS regular boxes, else in the caller's workspace (the slice of
// the segment's own boxes: only this workgroup touches it, it initialises it itself).
// LDS: the workgroup always reserves MAX_THR * KEYS keys (8 KB) + one chunk of boxes (2 KB), although a typical call passes
// one or two thresholds and a segment holds fewer than 10 boxes: about 16 single-wave workgroups per CU instead of 32.  At
// 0.3 ms for the 183,106 segments of a night-sunny split that residency is not what bounds the launch; sizing the keys by
// n_thr (dynamic LDS) is the change to make if it ever is.
// Every offset read from the device arrays is clamped to [0, n_det] / [0, n_gt] before it indexes anything.
#include "common.h"
#include "oadg_hip.h"

namespace {

constexpr int THREADS = 64;        // one wave
constexpr int CHUNK = 128;         // boxes staged in LDS per pass over the detections
constexpr int KEYS = 128;          // regular boxes per segment whose claim keys fit in LDS
constexpr int MAX_THR = OADG_VOC_MAX_THRS;
constexpr unsigned long long NO_CLAIM = ~0ull;

struct Thresholds {
    float t[MAX_THR];
};

// monotone float -> uint map (a < b  <=>  orderable(a) < orderable(b)); -0.0 is folded to +0.0
__device__ __forceinline__ unsigned orderable(float f) {
    unsigned u = __float_as_uint(f);
    if (f == 0.0f) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(THREADS) void voc_tpfp_kernel(const float* __restrict__ dets, const int* __restrict__ det_off,
                                                           const float* __restrict__ gts, const int* __restrict__ gt_off,
                                                           const int* __restrict__ gt_reg, int n_det, int n_gt,
                                                           Thresholds thr, int n_thr, float ex, float* __restrict__ iou_max,
                                                           int* __restrict__ iou_arg, uint8_t* __restrict__ flags,
                                                           unsigned long long* ws_keys) {
    __shared__ float4 box[CHUNK];
    __shared__ unsigned long long key[MAX_THR * KEYS];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int d0 = clampi(det_off[s], 0, n_det), d1 = clampi(det_off[s + 1], d0, n_det);
    const int g0 = clampi(gt_off[s], 0, n_gt), g1 = clampi(gt_off[s + 1], g0, n_gt);
    const int nd = d1 - d0, ng = g1 - g0, nreg = clampi(gt_reg[s], 0, ng);
    if (nd == 0) return;                                             // (uniform: the whole workgroup leaves)
    const bool in_lds = nreg <= KEYS;
    for (int t = 0; t < n_thr; ++t)
        for (int j = tid; j < nreg; j += THREADS) {
            if (in_lds) key[t * KEYS + j] = NO_CLAIM;
            else ws_keys[(size_t)t * n_gt + g0 + j] = NO_CLAIM;
        }
    __syncthreads();
    // ---- pass 1
    for (int base = 0; base < nd; base += THREADS) {
        const int i = base + tid;
        const bool live = i < nd;
        float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f, score = 0.f;
        if (live) {
            const float* d = dets + (size_t)(d0 + i) * 5;
            x1 = d[0]; y1 = d[1]; x2 = d[2]; y2 = d[3]; score = d[4];
        }
        const float area_d = (x2 - x1 + ex) * (y2 - y1 + ex);
        float best = 0.f;
        int arg = -1;
        for (int c0 = 0; c0 < ng; c0 += CHUNK) {
            const int cn = ng - c0 < CHUNK ? ng - c0 : CHUNK;
            __syncthreads();                                         // the previous chunk has been read by every lane
            for (int j = tid; j < cn; j += THREADS) box[j] = reinterpret_cast<const float4*>(gts)[g0 + c0 + j];
            __syncthreads();
            if (live) {
                for (int j = 0; j < cn; ++j) {
                    const float4 g = box[j];
                    const float area_g = (g.z - g.x + ex) * (g.w - g.y + ex);
                    const float xs = fmaxf(x1, g.x), ys = fmaxf(y1, g.y), xe = fminf(x2, g.z), ye = fminf(y2, g.w);
                    const float ov = fmaxf(xe - xs + ex, 0.f) * fmaxf(ye - ys + ex, 0.f);
                    const float un = fmaxf(area_d + area_g - ov, 1e-6f);
                    const float iou = __fdiv_rn(ov, un);
                    if (arg < 0 || iou > best) { best = iou; arg = c0 + j; }
                }
            }
        }
        if (live) {
            iou_max[d0 + i] = best;
            iou_arg[d0 + i] = arg;
            if (arg >= 0 && arg < nreg) {
                const unsigned long long mine = ((unsigned long long)(~orderable(score)) << 32) | (unsigned)i;
                for (int t = 0; t < n_thr; ++t)
                    if (best >= thr.t[t]) {
                        if (in_lds) atomicMin(&key[t * KEYS + arg], mine);
                        else atomicMin(&ws_keys[(size_t)t * n_gt + g0 + arg], mine);
                    }
            }
        }
    }
    __syncthreads();
    // ---- pass 2
    for (int base = 0; base < nd; base += THREADS) {
        const int i = base + tid;
        if (i >= nd) continue;
        const float best = iou_max[d0 + i];                         // (written by this very thread above)
        const int arg = iou_arg[d0 + i];
        const float score = dets[(size_t)(d0 + i) * 5 + 4];
        const unsigned long long mine = ((unsigned long long)(~orderable(score)) << 32) | (unsigned)i;
        for (int t = 0; t < n_thr; ++t) {
            uint8_t f = 2;
            if (arg >= 0 && best >= thr.t[t]) {
                if (arg >= nreg) f = 0;
                else {
                    const unsigned long long win =
                        in_lds ? key[t * KEYS + arg]
                               : __hip_atomic_load(&ws_keys[(size_t)t * n_gt + g0 + arg], __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT);
                    f = win == mine ? 1 : 2;
                }
            }
            flags[(size_t)t * n_det + d0 + i] = f;
        }
    }
}

}  // namespace

extern "C" size_t oadg_voc_tpfp_workspace_bytes(int n_seg, int n_det, int n_gt, int n_thr) {
    if (n_seg < 0 || n_det < 0 || n_gt < 0 || n_thr < 1 || n_thr > MAX_THR) return 0;
    const size_t b = (size_t)n_thr * (size_t)n_gt * sizeof(unsigned long long);
    return b < 8 ? 8 : b;
}

extern "C" int oadg_voc_tpfp(const float* dets, const int32_t* det_off, const float* gts, const int32_t* gt_off,
                             const int32_t* gt_reg, int n_seg, int n_det, int n_gt, const float* iou_thrs_host, int n_thr,
                             int legacy, float* iou_max, int32_t* iou_arg, uint8_t* flags, void* workspace,
                             size_t workspace_bytes, void* stream) {
    if (n_seg < 0 || n_det < 0 || n_gt < 0 || n_thr < 1 || n_thr > MAX_THR || !iou_thrs_host) return OADG_EARG;
    if (n_seg > 0 && (!det_off || !gt_off || !gt_reg)) return OADG_EARG;
    if (n_det > 0 && (!dets || !iou_max || !iou_arg || !flags)) return OADG_EARG;
    if (n_gt > 0 && (!gts || ((uintptr_t)gts & 15))) return OADG_EARG;               // (boxes are read 16 bytes at a time)
    if (!workspace || ((uintptr_t)workspace & 7)) return OADG_EARG;
    if (workspace_bytes < oadg_voc_tpfp_workspace_bytes(n_seg, n_det, n_gt, n_thr)) return OADG_ESIZE;
    if (n_seg == 0 || n_det == 0) return OADG_OK;
    Thresholds thr;
    for (int t = 0; t < MAX_THR; ++t) thr.t[t] = t < n_thr ? iou_thrs_host[t] : 2.0f;
    voc_tpfp_kernel<<<dim3((unsigned)n_seg), dim3(THREADS), 0, (hipStream_t)stream>>>(
        dets, det_off, gts, gt_off, gt_reg, n_det, n_gt, thr, n_thr, legacy ? 1.0f : 0.0f, iou_max, iou_arg, flags,
        (unsigned long long*)workspace);
    OADG_LAUNCH_CHECK();
    return OADG_OK;
}
