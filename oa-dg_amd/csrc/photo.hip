// PhotoMetricDistortion + CutOut + Normalize + Pad for a whole batch in one launch (C ABI and the per-pixel contract:
// include/oadg_hip.h, oadg_photo_normalize_batch).
//   reference: mmdet/datasets/pipelines/transforms.py:941-1041, :1874-1944, :618-629, :699-701
// The reference turns the image into a float32 array and makes about seven numpy passes over it; here a pixel is read once
// (3 bytes), carried through the whole chain in registers and written once (6 or 12 bytes): no float image exists in HBM.
// The HSV round trip is OpenCV's documented float32 algorithm with H in 0..360 (what mmcv.bgr2hsv / hsv2bgr call), restated
// operation by operation - every +, -, *, / below is one correctly rounded fp32 operation, in this order, nothing contracted
// (-ffp-contract=off) - so that a numpy float32 restatement gives the same bits (tests/test_photometric.py).  It is NOT
// csrc/corrupt.hip's HSV (skimage's formula).
//
// Mapping: one thread per 4 consecutive pixels of an OUTPUT row, grid.y = image.  The 12 input bytes of a group start at
// any byte (3 W is no multiple of 4, an image of a batch tensor starts anywhere): they are fetched as the up to four aligned
// dwords that hold them - never a dword that holds none of the image's bytes - and shifted into place (v_alignbyte_b32).
// A wave reads 768 contiguous bytes per load instruction instead of 64 bytes at stride 3 with byte loads.  The 48 (fp32) or
// 24 (bf16) output bytes of a group are 16- / 8-byte aligned whenever Wp is a multiple of 4 and the slices are aligned
// (size_divisor = 32: always): three dwordx4 / dwordx2 stores; any other Wp, the ragged end of a row included, takes
// element stores.  The flags, parameters and holes of an image are uniform over a workgroup: they sit in scalar registers
// and every branch on them is uniform.
#include <float.h>

#include "common.h"
#include "oadg_hip.h"

namespace {

struct PhotoNorm {
    float mean[3], stdinv[3];
    int to_rgb;
};

constexpr int PX = 4;   // pixels per thread

// transforms.py:987-1028 on one pixel (b, g, r), float32
__device__ __forceinline__ void photo_chain(float& b, float& g, float& r, const oadg_photo_image& im) {
    const int fl = im.flags;
    if (fl & OADG_PHOTO_DELTA) { b += im.delta; g += im.delta; r += im.delta; }
    if (fl & OADG_PHOTO_ALPHA_PRE) { b *= im.alpha_pre; g *= im.alpha_pre; r *= im.alpha_pre; }
    // BGR -> HSV (always: the round trip is not the identity in float32)
    const float v = fmaxf(fmaxf(b, g), r), vmin = fminf(fminf(b, g), r);
    const float diff = v - vmin;
    float s = diff / (fabsf(v) + FLT_EPSILON);
    const float d = 60.f / (diff + FLT_EPSILON);
    float h;
    if (v == r) h = (g - b) * d;
    else if (v == g) h = (b - r) * d + 120.f;
    else h = (r - g) * d + 240.f;
    if (h < 0.f) h += 360.f;
    if (fl & OADG_PHOTO_SAT) s *= im.sat;
    if (fl & OADG_PHOTO_HUE) {
        h += im.hue;
        if (h > 360.f) h -= 360.f;      // the reference's two masked assignments, one after the other
        if (h < 0.f) h += 360.f;
    }
    // HSV -> BGR
    if (s == 0.f) {
        b = g = r = v;
    } else {
        float h6 = h * (float)(6.0 / 360.0);
        if (h6 < 0.f) h6 += 6.f;
        else if (h6 >= 6.f) h6 -= 6.f;
        const float fl6 = floorf(h6);
        int sector = (int)fl6;
        float f = h6 - fl6;
        if ((unsigned)sector >= 6u) { sector = 0; f = 0.f; }
        const float t0 = v, t1 = v * (1.f - s), t2 = v * (1.f - s * f), t3 = v * (1.f - s * (1.f - f));
        // (b, g, r) = tab[{1,3,0}, {1,0,2}, {3,0,1}, {0,2,1}, {0,1,3}, {2,1,0}][sector], as selects (no indexed registers)
        b = sector <= 1 ? t1 : sector == 2 ? t3 : sector == 5 ? t2 : t0;
        g = sector == 0 ? t3 : sector <= 2 ? t0 : sector == 3 ? t2 : t1;
        r = sector == 0 ? t0 : sector == 1 ? t2 : sector <= 3 ? t1 : sector == 4 ? t3 : t0;
    }
    if (fl & OADG_PHOTO_ALPHA_POST) { b *= im.alpha_post; g *= im.alpha_post; r *= im.alpha_post; }
    if (fl & OADG_PHOTO_PERM) {
        const float c0 = b, c1 = g, c2 = r;
        b = im.perm[0] == 0 ? c0 : im.perm[0] == 1 ? c1 : c2;
        g = im.perm[1] == 0 ? c0 : im.perm[1] == 1 ? c1 : c2;
        r = im.perm[2] == 0 ? c0 : im.perm[2] == 1 ? c1 : c2;
    }
}

// bit k set: pixel (x0 + k, y) lies in one of the image's holes
__device__ __forceinline__ unsigned hole_mask(const int32_t* __restrict__ rects, const oadg_photo_image& im, int x0, int y) {
    unsigned m = 0;
    for (int i = 0; i < im.n_rects; ++i) {
        const int32_t* q = rects + 4 * ((long)im.rect_off + i);
        const int x1 = q[0], y1 = q[1], x2 = q[2], y2 = q[3];
        if (y >= y1 && y < y2) {
#pragma unroll
            for (int k = 0; k < PX; ++k) m |= (x0 + k >= x1 && x0 + k < x2) ? 1u << k : 0u;
        }
    }
    return m;
}

template <typename T>
__global__ __launch_bounds__(256) void photo_normalize_kernel(const oadg_photo_image* __restrict__ table,
                                                              const int32_t* __restrict__ rects, PhotoNorm nrm,
                                                              T* __restrict__ out, int Hp, int Wp, int groups_x,
                                                              size_t image_stride, int wide) {
    const oadg_photo_image im = table[blockIdx.y];
    const long gi = (long)blockIdx.x * 256 + threadIdx.x;
    if (gi >= (long)Hp * groups_x) return;
    const int y = (int)(gi / groups_x), x0 = (int)(gi - (long)y * groups_x) * PX;
    const int n_out = min(PX, Wp - x0);                                     // 1..4 pixels of this group are inside the row
    const int n_in = y < im.H ? max(0, min(n_out, im.W - x0)) : 0;          // of which this many are image, the rest pad
    float val[3 * PX];
#pragma unroll
    for (int i = 0; i < 3 * PX; ++i) val[i] = 0.f;
    if (n_in > 0) {
        // the 3 * n_in bytes from `a` on, out of the aligned dwords that hold them
        const uintptr_t a = (uintptr_t)im.img + ((size_t)y * im.W + x0) * 3;
        const unsigned sh = (unsigned)(a & 3);
        // (a pointer read from the table is a generic one to the compiler: say that it is global memory, or the loads are flat)
        const __attribute__((address_space(1))) uint32_t* q = (const __attribute__((address_space(1))) uint32_t*)(a - sh);
        const int nd = (int)(sh + 3 * n_in + 3) >> 2;                       // 1..4
        uint32_t dw[PX];
#pragma unroll
        for (int j = 0; j < PX; ++j) dw[j] = j < nd ? q[j] : 0u;
        uint32_t w[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) w[j] = __builtin_amdgcn_alignbyte(dw[j + 1], dw[j], sh);
        const int fl = im.flags;
        const unsigned holes = im.n_rects > 0 ? hole_mask(rects, im, x0, y) : 0u;
#pragma unroll
        for (int k = 0; k < PX; ++k) {
            if (k >= n_in) break;
            float px[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) px[c] = (float)((w[(3 * k + c) >> 2] >> (8 * ((3 * k + c) & 3))) & 0xffu);
            const bool hole = (holes >> k) & 1u;
            if (hole && !(fl & OADG_PHOTO_CUTOUT_LAST)) { px[0] = im.fill[0]; px[1] = im.fill[1]; px[2] = im.fill[2]; }
            if (fl & OADG_PHOTO_PRESENT) photo_chain(px[0], px[1], px[2], im);
            if (hole && (fl & OADG_PHOTO_CUTOUT_LAST)) { px[0] = im.fill[0]; px[1] = im.fill[1]; px[2] = im.fill[2]; }
            // mmcv.imnormalize: BGR->RGB swap, then (x - mean) * (1 / std) in float32
#pragma unroll
            for (int c = 0; c < 3; ++c) val[3 * k + c] = (px[nrm.to_rgb ? 2 - c : c] - nrm.mean[c]) * nrm.stdinv[c];
        }
    }
    T* o = out + (size_t)blockIdx.y * image_stride + ((size_t)y * Wp + x0) * 3;
    if constexpr (sizeof(T) == 4) {
        if (wide) {         // Wp % 4 == 0: every group is whole and 48 bytes from a 16-byte aligned row start
#pragma unroll
            for (int j = 0; j < 3; ++j)
                ((float4*)o)[j] = make_float4(val[4 * j], val[4 * j + 1], val[4 * j + 2], val[4 * j + 3]);
            return;
        }
#pragma unroll
        for (int i = 0; i < 3 * PX; ++i)
            if (i < 3 * n_out) o[i] = val[i];
    } else {
        unsigned short hv[3 * PX];
#pragma unroll
        for (int i = 0; i < 3 * PX; ++i) hv[i] = f32_to_bf16(val[i]);
        if (wide) {         // 24 bytes from an 8-byte aligned row start
#pragma unroll
            for (int j = 0; j < 3; ++j)
                ((uint2*)o)[j] = make_uint2((unsigned)hv[4 * j] | ((unsigned)hv[4 * j + 1] << 16),
                                            (unsigned)hv[4 * j + 2] | ((unsigned)hv[4 * j + 3] << 16));
            return;
        }
#pragma unroll
        for (int i = 0; i < 3 * PX; ++i)
            if (i < 3 * n_out) o[i] = hv[i];
    }
}

}  // namespace

extern "C" {

int oadg_photo_normalize_batch(const oadg_photo_image* table, int n_images, const int32_t* rects, const float* mean_host,
                               const float* stdinv_host, int to_rgb, void* out, int out_dtype, int Hp, int Wp,
                               size_t out_image_stride_elems, void* stream) {
    if (!table || !out || !mean_host || !stdinv_host || n_images < 0 || n_images > 65535 || Hp <= 0 || Wp <= 0 ||
        (out_dtype != 0 && out_dtype != 1) || out_image_stride_elems < (size_t)Hp * Wp * 3)
        return OADG_EARG;
    if (n_images == 0) return OADG_OK;
    PhotoNorm nrm;
    for (int c = 0; c < 3; ++c) { nrm.mean[c] = mean_host[c]; nrm.stdinv[c] = stdinv_host[c]; }
    nrm.to_rgb = to_rgb;
    const int groups_x = (Wp + PX - 1) / PX;
    const long blocks = ((long)Hp * groups_x + 255) / 256;
    if (blocks > 0x7fffffffL) return OADG_EARG;
    const size_t esz = out_dtype == 1 ? 2 : 4, align = 4 * esz;         // a group's stores: dwordx4 (fp32) / dwordx2 (bf16)
    const int wide = Wp % PX == 0 && (uintptr_t)out % align == 0 && (out_image_stride_elems * esz) % align == 0;
    const dim3 grid((unsigned)blocks, (unsigned)n_images);
    hipStream_t st = (hipStream_t)stream;
    if (out_dtype == 1)
        hipLaunchKernelGGL((photo_normalize_kernel<unsigned short>), grid, dim3(256), 0, st, table, rects, nrm,
                           (unsigned short*)out, Hp, Wp, groups_x, out_image_stride_elems, wide);
    else
        hipLaunchKernelGGL((photo_normalize_kernel<float>), grid, dim3(256), 0, st, table, rects, nrm, (float*)out, Hp, Wp,
                           groups_x, out_image_stride_elems, wide);
    OADG_LAUNCH_CHECK();
    return OADG_OK;
}

}  // extern "C"
