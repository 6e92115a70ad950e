// Confusion counts of a whole test split in one launch.
//
// Replaces, for evaluation.calculate_confusion_matrix (tools/analysis_tools/confusion_matrix.py):
//   tools/analysis_tools/confusion_matrix.py:95-142   analyze_per_img_dets - classes x detections x boxes in Python, per image,
//   mmdet/core/evaluation/bbox_overlaps.py            bbox_overlaps (fp32, modern extents).
// A segment is one IMAGE: its detections dets[det_off[s] .. det_off[s+1]) with their classes det_cls (the caller has already
// dropped the ones under the score threshold) and its boxes gts[gt_off[s] .. gt_off[s+1]) with their labels gt_lab.  Unlike
// the VOC and COCO matchings nothing is claimed: a detection of class c is compared with EVERY box of the image,
//   every box j with iou >= thr          cm[gt_lab[j]][c] += 1   (and box j is "found" when gt_lab[j] == c),
//   no such box                          cm[C][c] += 1           (background false positive),
//   after all detections, box j unfound  cm[gt_lab[j]][C] += 1   (false negative).
//
// One single-wave workgroup per image, shaped like voc_tpfp_kernel (a Cityscapes image holds up to 100 detections and about
// 20 boxes: the launch is latency-bound, every barrier is free): each lane takes a detection and walks the image's boxes,
// staged through LDS in chunks of CHUNK with their labels, computing the fp32 IoU in the host's operation order (the library
// is built with -ffp-contract=off; the division is correctly rounded).
//   counts  per workgroup in LDS (32-bit cells) when (C + 1)^2 <= CELLS and the image has fewer than 2^32 (detection, box)
//           pairs; only the non-zero cells are flushed, with one 64-bit global atomic add each.  Otherwise every count is a
//           global atomic add on the output.
//   found   one word per box in LDS when the image has at most BOXES boxes, else in the caller's workspace (the slice of
//           the image's own boxes: only this workgroup touches it, it initialises it itself).
// All results are integers: the order of the atomics cannot change them, the output equals the host's with ==.
// Every offset is clamped to [0, n_det] / [0, n_gt] before it indexes anything; a detection whose class or a box whose
// label lies outside [0, C) takes no part (the pack refuses them on the host: this only keeps a bad array in bounds).
#include "common.h"
#include "oadg_hip.h"

namespace {

constexpr int THREADS = 64;                          // one wave
constexpr int CHUNK = OADG_CONFUSION_CHUNK;          // boxes staged in LDS per pass over the detections
constexpr int BOXES = OADG_CONFUSION_LDS_BOXES;      // boxes per image whose "found" words fit in LDS
constexpr int CELLS = OADG_CONFUSION_LDS_CELLS;      // (C + 1)^2 up to which the counts of an image are kept in LDS

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(THREADS) void confusion_kernel(const float* __restrict__ dets, const int* __restrict__ det_cls,
                                                            const int* __restrict__ det_off, const float* __restrict__ gts,
                                                            const int* __restrict__ gt_lab, const int* __restrict__ gt_off,
                                                            int n_det, int n_gt, int C, float thr, float ex,
                                                            unsigned long long* __restrict__ out, unsigned* ws_found) {
    __shared__ float4 box[CHUNK];
    __shared__ int lab[CHUNK];
    __shared__ unsigned found[BOXES];
    __shared__ unsigned cell[CELLS];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int d0 = clampi(det_off[s], 0, n_det), d1 = clampi(det_off[s + 1], d0, n_det);
    const int g0 = clampi(gt_off[s], 0, n_gt), g1 = clampi(gt_off[s + 1], g0, n_gt);
    const int nd = d1 - d0, ng = g1 - g0;
    if (nd == 0 && ng == 0) return;                                  // (uniform: the whole workgroup leaves)
    const int row = C + 1;
    const size_t n_cell = (size_t)row * row;
    const bool cells_in_lds = n_cell <= (size_t)CELLS && (unsigned long long)nd * (unsigned long long)ng < (1ull << 32);
    const bool found_in_lds = ng <= BOXES;
    unsigned* fnd = found_in_lds ? found : ws_found + g0;
    if (cells_in_lds)
        for (int k = tid; k < (int)n_cell; k += THREADS) cell[k] = 0u;
    for (int j = tid; j < ng; j += THREADS) fnd[j] = 0u;
    __syncthreads();
    auto count = [&](int r, int c) {
        const size_t k = (size_t)r * row + c;
        if (cells_in_lds) atomicAdd(&cell[k], 1u);
        else atomicAdd(&out[k], 1ull);
    };
    // ---- the detections, THREADS at a time
    for (int base = 0; base < nd; base += THREADS) {
        const int i = base + tid;
        int c = -1;
        float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f;
        if (i < nd) {
            const float4 d = reinterpret_cast<const float4*>(dets)[d0 + i];
            x1 = d.x; y1 = d.y; x2 = d.z; y2 = d.w;
            c = det_cls[d0 + i];
        }
        const bool live = c >= 0 && c < C;
        const float area_d = (x2 - x1 + ex) * (y2 - y1 + ex);
        int matched = 0;
        for (int c0 = 0; c0 < ng; c0 += CHUNK) {
            const int cn = ng - c0 < CHUNK ? ng - c0 : CHUNK;
            __syncthreads();                                         // the previous chunk has been read by every lane
            for (int j = tid; j < cn; j += THREADS) {
                box[j] = reinterpret_cast<const float4*>(gts)[g0 + c0 + j];
                lab[j] = gt_lab[g0 + c0 + j];
            }
            __syncthreads();
            if (live) {
                for (int j = 0; j < cn; ++j) {
                    const float4 g = box[j];
                    const int l = lab[j];
                    const float area_g = (g.z - g.x + ex) * (g.w - g.y + ex);
                    const float xs = fmaxf(x1, g.x), ys = fmaxf(y1, g.y), xe = fminf(x2, g.z), ye = fminf(y2, g.w);
                    const float ov = fmaxf(xe - xs + ex, 0.f) * fmaxf(ye - ys + ex, 0.f);
                    const float un = fmaxf(area_d + area_g - ov, 1e-6f);
                    const float iou = __fdiv_rn(ov, un);
                    if (iou >= thr && l >= 0 && l < C) {
                        ++matched;
                        count(l, c);
                        if (l == c) atomicOr(&fnd[c0 + j], 1u);
                    }
                }
            }
        }
        if (live && matched == 0) count(C, c);
    }
    __syncthreads();
    // ---- the boxes no detection of their own label matched
    for (int j = tid; j < ng; j += THREADS) {
        const unsigned f = found_in_lds ? found[j] : __hip_atomic_load(&ws_found[g0 + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int l = gt_lab[g0 + j];
        if (f == 0u && l >= 0 && l < C) count(l, C);
    }
    if (!cells_in_lds) return;                                       // (uniform)
    __syncthreads();
    for (int k = tid; k < (int)n_cell; k += THREADS) {
        const unsigned v = cell[k];
        if (v) atomicAdd(&out[k], (unsigned long long)v);
    }
}

}  // namespace

extern "C" size_t oadg_confusion_workspace_bytes(int n_seg, int n_det, int n_gt, int num_classes) {
    if (n_seg < 0 || n_det < 0 || n_gt < 0 || num_classes < 1 || num_classes > OADG_CONFUSION_MAX_CLASSES) return 0;
    const size_t b = (size_t)n_gt * sizeof(unsigned);
    return b < 8 ? 8 : b;
}

extern "C" int oadg_confusion_count(const float* dets, const int32_t* det_cls, const int32_t* det_off, const float* gts,
                                    const int32_t* gt_lab, const int32_t* gt_off, int n_seg, int n_det, int n_gt,
                                    int num_classes, float tp_iou_thr, int64_t* counts, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    if (n_seg < 0 || n_det < 0 || n_gt < 0 || num_classes < 1 || num_classes > OADG_CONFUSION_MAX_CLASSES) return OADG_EARG;
    if (!counts || ((uintptr_t)counts & 7)) return OADG_EARG;
    if (n_seg > 0 && (!det_off || !gt_off)) return OADG_EARG;
    if (n_det > 0 && (!dets || !det_cls || ((uintptr_t)dets & 15))) return OADG_EARG;      // (read 16 bytes at a time)
    if (n_gt > 0 && (!gts || !gt_lab || ((uintptr_t)gts & 15))) return OADG_EARG;
    if (!workspace || ((uintptr_t)workspace & 3)) return OADG_EARG;
    if (workspace_bytes < oadg_confusion_workspace_bytes(n_seg, n_det, n_gt, num_classes)) return OADG_ESIZE;
    const size_t n_cell = (size_t)(num_classes + 1) * (size_t)(num_classes + 1);
    hipError_t e = hipMemsetAsync(counts, 0, n_cell * sizeof(int64_t), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    if (n_seg == 0 || (n_det == 0 && n_gt == 0)) return OADG_OK;
    confusion_kernel<<<dim3((unsigned)n_seg), dim3(THREADS), 0, (hipStream_t)stream>>>(
        dets, det_cls, det_off, gts, gt_lab, gt_off, n_det, n_gt, num_classes, tp_iou_thr, 0.0f,
        (unsigned long long*)counts, (unsigned*)workspace);
    OADG_LAUNCH_CHECK();
    return OADG_OK;
}
