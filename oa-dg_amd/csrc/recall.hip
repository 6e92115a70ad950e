// Proposal recall: Hosang's greedy bipartite matching of boxes to proposals for a whole test split and every proposal budget
// in one launch.
//
// Replaces, for evaluation.eval_recalls(device=...) (CocoDataset.fast_eval_recall, proposal_evaluate 'proposal_fast' /
// 'recall', tools/test.py --eval proposal_fast / recall):
//   mmdet/core/evaluation/recall.py:11-41      _recalls - per image and per budget G rounds, each an argmax over a G x P IoU
//                                              matrix and the rewrite of one row and one column to -1 -,
//   mmdet/core/evaluation/bbox_overlaps.py     bbox_overlaps (fp32, legacy "+ 1" extents or modern ones),
// as evaluation.recall_ious_host restates them (the host path and the yardstick of tests/test_hip_recall.py).
// An image owns its proposals props[prop_off[i] .. prop_off[i+1]) - in evaluation order, cut to the largest budget - and its
// boxes gts[gt_off[i] .. gt_off[i+1]).  Budget k sees the first n = min(nums[k], P_i) proposals (the "columns").
//
// One single-wave workgroup per (image, budget): with one wave every barrier is free and all control flow below is uniform
// over the workgroup.  NO G x P matrix exists anywhere.  Per box the workgroup keeps a cached (best IoU over the live columns,
// lowest column that attains it); an IoU is recomputed from the coordinates whenever it is needed again:
//   start    every box: lanes over the columns, each keeps its largest value and lowest column, then a butterfly over the
//            wave with the rule "larger value, or the same value at a lower column".
//   round j  lanes over the boxes -> the largest cached value and the LOWEST live box that holds it (the same butterfly);
//            out[j] = that value; the box and its column retire; only the live boxes whose cached column has just retired
//            are recomputed (found by ballot, so the loop over them is uniform).  A cached pair whose column is still live is
//            still what numpy's argmax over the rewritten matrix returns: a retired column holds -1, below every IoU.
//            Once no column is live every remaining round records -1; no proposal at all records 0 for every box.
// IoUs are fp32 in the host's operation order (the library is built with -ffp-contract=off; the division is correctly
// rounded), so the values are the host's bit for bit.  Finite inputs only: with a NaN the kernel still terminates, indexes
// nothing out of range and writes every element, but promises no value.
// Proposals and their "retired" bytes live in LDS while n <= LDS_PROPS, the cached pairs while G_i <= LDS_GTS.  Beyond either
// capacity that state lives in the caller's workspace (the slices of this image and budget: only this workgroup touches
// them, it initialises them itself; read and written with agent-scope atomics, as a lane reads what another lane wrote)
// and the proposals are read from global memory, 64 consecutive ones per pass.  Any P and any G are correct.
// LDS: 16 KB proposals + 1 KB retired bytes + 2 KB cached pairs = 19 KB, 8 single-wave workgroups per CU by LDS.
// Every offset read from the device arrays is clamped to [0, n_prop] / [0, n_gt] before it indexes anything.
#include <climits>

#include "common.h"
#include "oadg_hip.h"

namespace {

constexpr int THREADS = 64;                        // one wave
constexpr int LDS_PROPS = OADG_RECALL_LDS_PROPS;   // columns of an (image, budget) staged in LDS
constexpr int LDS_GTS = OADG_RECALL_LDS_GTS;       // boxes of an image whose cached pairs fit in LDS
constexpr int MAX_NUMS = OADG_RECALL_MAX_NUMS;
constexpr float RETIRED = -2.0f;                   // cached value of a retired box: below every IoU and below -1

struct Nums {
    int n[MAX_NUMS];
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <typename T>
__device__ __forceinline__ T ws_get(const T* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename T>
__device__ __forceinline__ void ws_put(T* p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// (value, index) of the whole wave in every lane: the larger value, among equal values the lower index
__device__ __forceinline__ void wave_best(float& v, int& i) {
    for (int m = THREADS / 2; m >= 1; m >>= 1) {
        const float ov = __shfl_xor(v, m, THREADS);
        const int oi = __shfl_xor(i, m, THREADS);
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
}

__global__ __launch_bounds__(THREADS) void recall_match_kernel(const float4* __restrict__ props, const int* __restrict__ prop_off,
                                                               const float4* __restrict__ gts, const int* __restrict__ gt_off,
                                                               int n_prop, int n_gt, Nums nums, float ex,
                                                               float* __restrict__ out, float* ws_val, int* ws_col,
                                                               unsigned char* ws_dead) {
    __shared__ float4 sprop[LDS_PROPS];
    __shared__ unsigned char sdead[LDS_PROPS];
    __shared__ float sval[LDS_GTS];
    __shared__ int scol[LDS_GTS];
    const int img = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
    const int p0 = clampi(prop_off[img], 0, n_prop), p1 = clampi(prop_off[img + 1], p0, n_prop);
    const int g0 = clampi(gt_off[img], 0, n_gt), g1 = clampi(gt_off[img + 1], g0, n_gt);
    const int ng = g1 - g0;
    if (ng == 0) return;                                             // (uniform: the whole workgroup leaves)
    const int n = clampi(nums.n[k], 0, p1 - p0);
    float* o = out + (size_t)k * n_gt + g0;
    if (n == 0) {                                                    // recall.py:22-24: no column, every box scores 0
        for (int j = tid; j < ng; j += THREADS) o[j] = 0.0f;
        return;
    }
    const bool p_lds = n <= LDS_PROPS, g_lds = ng <= LDS_GTS;
    float* wval = ws_val + (size_t)k * n_gt + g0;
    int* wcol = ws_col + (size_t)k * n_gt + g0;
    unsigned char* wdead = ws_dead + (size_t)k * n_prop + p0;
    // (workspace state is written and read with agent-scope atomics, which go past the L1: the barriers' workgroup-scope
    //  ordering is all a lane needs to see what another lane of this wave stored - no device-wide fence per round)
    auto get_val = [&](int b) { return g_lds ? sval[b] : ws_get(wval + b); };
    auto get_col = [&](int b) { return g_lds ? scol[b] : ws_get(wcol + b); };
    auto set_pair = [&](int b, float v, int c) {
        if (g_lds) { sval[b] = v; scol[b] = c; }
        else { ws_put(wval + b, v); ws_put(wcol + b, c); }
    };
    for (int c = tid; c < n; c += THREADS) {
        if (p_lds) { sprop[c] = props[p0 + c]; sdead[c] = 0; }
        else ws_put(wdead + c, (unsigned char)0);
    }
    __syncthreads();
    // box b: the largest IoU over the live columns and the lowest column that attains it -> its cached pair
    auto recompute = [&](int b) {
        const float4 g = gts[g0 + b];
        const float area_g = (g.z - g.x + ex) * (g.w - g.y + ex);
        float best = -1.0f;
        int col = INT_MAX;
        for (int c = tid; c < n; c += THREADS) {
            if (p_lds ? sdead[c] : ws_get(wdead + c)) continue;
            const float4 p = p_lds ? sprop[c] : props[p0 + c];
            const float area_p = (p.z - p.x + ex) * (p.w - p.y + ex);
            const float xs = fmaxf(g.x, p.x), ys = fmaxf(g.y, p.y), xe = fminf(g.z, p.z), ye = fminf(g.w, p.w);
            const float ov = fmaxf(xe - xs + ex, 0.f) * fmaxf(ye - ys + ex, 0.f);
            const float un = fmaxf(area_g + area_p - ov, 1e-6f);
            const float iou = __fdiv_rn(ov, un);
            if (iou > best) { best = iou; col = c; }                 // (ascending c: the lowest column of this lane)
        }
        wave_best(best, col);
        if (tid == 0) set_pair(b, best, col);
    };
    for (int b = 0; b < ng; ++b) recompute(b);
    __syncthreads();
    int live_cols = n;
    for (int j = 0; j < ng; ++j) {
        if (live_cols <= 0) {                                        // the surplus boxes of an image with more boxes than columns
            for (int r = j + tid; r < ng; r += THREADS) o[r] = -1.0f;
            break;
        }
        float best = RETIRED;
        int box = INT_MAX;
        for (int b = tid; b < ng; b += THREADS) {
            const float v = get_val(b);
            if (v > best) { best = v; box = b; }                     // (ascending b: the lowest box of this lane)
        }
        wave_best(best, box);
        const bool found = box < ng;                                 // (false only where a NaN left nothing comparable)
        const int col = found ? get_col(box) : -1;
        const bool col_ok = col >= 0 && col < n;
        __syncthreads();                                             // every lane has read the pairs of this round
        if (tid == 0) {
            o[j] = found ? best : -1.0f;
            if (found) set_pair(box, RETIRED, -1);
            if (col_ok) {
                if (p_lds) sdead[col] = 1;
                else ws_put(wdead + col, (unsigned char)1);
            }
        }
        live_cols = col_ok ? live_cols - 1 : 0;
        __syncthreads();
        if (live_cols <= 0) continue;
        for (int base = 0; base < ng; base += THREADS) {
            const int b = base + tid;
            const bool hit = b < ng && get_val(b) > RETIRED && get_col(b) == col;
            unsigned long long m = __ballot(hit);
            while (m) {                                              // (uniform: the ballot is the same in every lane)
                const int l = __ffsll((long long)m) - 1;
                m &= m - 1;
                recompute(base + l);
            }
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" size_t oadg_recall_match_workspace_bytes(int n_img, int n_prop, int n_gt, int n_nums) {
    if (n_img < 0 || n_prop < 0 || n_gt < 0 || n_nums < 1 || n_nums > MAX_NUMS) return 0;
    const size_t b = (size_t)n_nums * ((size_t)n_gt * (sizeof(float) + sizeof(int)) + (size_t)n_prop);
    return b < 8 ? 8 : b;
}

extern "C" int oadg_recall_match(const float* props, const int32_t* prop_off, const float* gts, const int32_t* gt_off,
                                 int n_img, int n_prop, int n_gt, const int32_t* nums_host, int n_nums, int legacy,
                                 float* out, void* workspace, size_t workspace_bytes, void* stream) {
    const size_t need = oadg_recall_match_workspace_bytes(n_img, n_prop, n_gt, n_nums);
    if (need == 0 || !nums_host) return OADG_EARG;
    if (n_img > 0 && (!prop_off || !gt_off)) return OADG_EARG;
    if (n_prop > 0 && (!props || ((uintptr_t)props & 15))) return OADG_EARG;         // (boxes are read 16 bytes at a time)
    if (n_gt > 0 && (!gts || ((uintptr_t)gts & 15) || !out || ((uintptr_t)out & 3))) return OADG_EARG;
    if (!workspace || ((uintptr_t)workspace & 7)) return OADG_EARG;
    if (workspace_bytes < need) return OADG_ESIZE;
    if (n_img == 0 || n_gt == 0) return OADG_OK;
    Nums nums;
    for (int k = 0; k < MAX_NUMS; ++k) nums.n[k] = k < n_nums ? nums_host[k] : 0;
    float* ws_val = (float*)workspace;
    int* ws_col = (int*)(ws_val + (size_t)n_nums * n_gt);
    unsigned char* ws_dead = (unsigned char*)(ws_col + (size_t)n_nums * n_gt);
    recall_match_kernel<<<dim3((unsigned)n_img, (unsigned)n_nums), dim3(THREADS), 0, (hipStream_t)stream>>>(
        (const float4*)props, prop_off, (const float4*)gts, gt_off, n_prop, n_gt, nums, legacy ? 1.0f : 0.0f, out, ws_val,
        ws_col, ws_dead);
    OADG_LAUNCH_CHECK();
    return OADG_OK;
}
