// The inverse half of libjpeg's integer JPEG pixel arithmetic, shared by the device kernels and the host twins of
// jpeg_decode.hip (file -> pixels) and recompress.hip (pixels -> quantized coefficients -> pixels): the islow IDCT with its
// range limit (jidctint.c), h2v1 / h2v2 fancy upsampling (jdsample.c) and the YCbCr -> RGB conversion (jdcolor.c), byte for
// byte as PIL / OpenCV decode under libjpeg-turbo's defaults.  tests/test_jpeg_decode.py and tests/test_recompress.py pin it.
#pragma once
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------------
// pixel stage: shared by the device kernels and the host twin

constexpr int kConstBits = 13, kPass1Bits = 2;
#define JFIX(x) ((int)((x) * (1 << kConstBits) + 0.5))
#define YFIX(x) ((int)((x) * 65536.0 + 0.5))

__host__ __device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// libjpeg's post-IDCT range_limit[v & RANGE_MASK] (v already descaled, centred on 0)
__host__ __device__ __forceinline__ int range_limit(int v) {
    const int w = ((v + 512) & 1023) - 512 + 128;
    return w < 0 ? 0 : (w > 255 ? 255 : w);
}

// One 1-D islow butterfly over x0..x7 (frequency order); out[k] before descaling, per jidctint.c.
__host__ __device__ __forceinline__ void idct_1d(int x0, int x1, int x2, int x3, int x4, int x5, int x6, int x7, int* o) {
    int z1 = (x2 + x6) * JFIX(0.541196100);
    const int t2 = z1 + x6 * (-JFIX(1.847759065));
    const int t3 = z1 + x2 * JFIX(0.765366865);
    const int t0 = (x0 + x4) * (1 << kConstBits);
    const int t1 = (x0 - x4) * (1 << kConstBits);
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    int a0 = x7, a1 = x5, a2 = x3, a3 = x1;
    z1 = a0 + a3;
    int z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const int z5 = (z3 + z4) * JFIX(1.175875602);
    a0 *= JFIX(0.298631336);
    a1 *= JFIX(2.053119869);
    a2 *= JFIX(3.072711026);
    a3 *= JFIX(1.501321110);
    z1 *= -JFIX(0.899976223);
    z2 *= -JFIX(2.562915447);
    z3 *= -JFIX(1.961570560);
    z4 *= -JFIX(0.390180644);
    z3 += z5;
    z4 += z5;
    a0 += z1 + z3;
    a1 += z2 + z4;
    a2 += z2 + z3;
    a3 += z1 + z4;
    o[0] = t10 + a3; o[7] = t10 - a3;
    o[1] = t11 + a2; o[6] = t11 - a2;
    o[2] = t12 + a1; o[5] = t12 - a1;
    o[3] = t13 + a0; o[4] = t13 - a0;
}

// in: the block's dequantized coefficients, column-major (in[u * 8 + v] = horizontal frequency u, vertical v);
// out: 8 x 8 samples, row-major
__host__ __device__ __forceinline__ void idct_islow(const int* in, uint8_t* out) {
    int ws[64];     // ws[row * 8 + col] after the column pass
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int* c = in + u * 8;
        int o[8];
        idct_1d(c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], o);
#pragma unroll
        for (int r = 0; r < 8; ++r) ws[r * 8 + u] = descale(o[r], kConstBits - kPass1Bits);
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int* w = ws + r * 8;
        int o[8];
        idct_1d(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], o);
#pragma unroll
        for (int x = 0; x < 8; ++x) out[r * 8 + x] = (uint8_t)range_limit(descale(o[x], kConstBits + kPass1Bits + 3));
    }
}

// chroma sample of output pixel (x, y): component plane p (row stride `stride`, true extent cw x ch), sampled hf x vf
// below the luma (1 or 2 each).  jdsample.c: h2v1_fancy_upsample / h2v2_fancy_upsample when the component is wider than 2
// samples, h2v1_upsample / h2v2_upsample (replication) otherwise; clamping the neighbour index to the true extent is the
// edge replication of libjpeg's first / last column special cases and of its context rows (jdmainct.c).
__host__ __device__ __forceinline__ int chroma_at(const uint8_t* p, int stride, int cw, int ch, int hf, int vf, int x,
                                                  int y) {
    if (hf == 1) return p[(long)y * stride + x];
    const int cx = x >> 1;
    if (cw <= 2) return p[(long)(vf == 2 ? y >> 1 : y) * stride + cx];
    if (vf == 1) {
        const uint8_t* r = p + (long)y * stride;
        const int near3 = r[cx] * 3;
        return (x & 1) ? (near3 + r[cx + 1 < cw ? cx + 1 : cw - 1] + 2) >> 2 : (near3 + r[cx > 0 ? cx - 1 : 0] + 1) >> 2;
    }
    const int cy = y >> 1;
    const int fy = (y & 1) ? (cy + 1 < ch ? cy + 1 : ch - 1) : (cy > 0 ? cy - 1 : 0);
    const uint8_t* rn = p + (long)cy * stride;
    const uint8_t* rf = p + (long)fy * stride;
    const int cs = 3 * rn[cx] + rf[cx];
    if (x & 1) {
        const int c2 = cx + 1 < cw ? cx + 1 : cw - 1;
        return (3 * cs + 3 * rn[c2] + rf[c2] + 7) >> 4;
    }
    const int c2 = cx > 0 ? cx - 1 : 0;
    return (3 * cs + 3 * rn[c2] + rf[c2] + 8) >> 4;
}

__host__ __device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// jdcolor.c ycc_rgb_convert; o = B, G, R
__host__ __device__ __forceinline__ void ycc_to_bgr(int y, int cb, int cr, uint8_t* o) {
    cb -= 128;
    cr -= 128;
    o[0] = (uint8_t)clamp255(y + ((YFIX(1.77200) * cb + 32768) >> 16));
    o[1] = (uint8_t)clamp255(y + ((-YFIX(0.34414) * cb - YFIX(0.71414) * cr + 32768) >> 16));
    o[2] = (uint8_t)clamp255(y + ((YFIX(1.40200) * cr + 32768) >> 16));
}

}  // namespace
