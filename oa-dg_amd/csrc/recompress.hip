// The two Pillow-only corruptions of the robustness benchmark on the DEVICE, byte for byte as the host path
// (pipelines/corrupt.py jpeg_compression / pixelate; `Corrupt`, mmdet/datasets/pipelines/transforms.py:1277-1317 ->
// imagecorruptions.corrupt).
//
// jpeg_compression = Image.save(JPEG, quality=q) + Image.open: a JPEG round trip.  The entropy coder between the two halves
// is lossless, so decode(encode(x)) is: colour conversion, 4:2:0 downsampling, forward DCT, quantize | dequantize, inverse
// DCT, fancy upsampling, colour conversion - no Huffman code anywhere.  The forward half restates libjpeg's integer
// arithmetic (libjpeg-turbo under Pillow's defaults):
//   - colour: jccolor.c rgb_ycc_convert (SCALEBITS 16; the chroma rounding term is ONE_HALF - 1 on top of 128 << 16)
//   - sampling 4:2:0 (Pillow's default at every quality): jcsample.c h2v2_downsample, (p00 + p01 + p10 + p11 + bias) >> 2
//     with bias 1 in even output columns and 2 in odd ones
//   - padding: the right edge is replicated BEFORE downsampling (jcsample.c expand_right_edge: the full-resolution column is
//     clamped to W - 1), the bottom edge AFTER it (jcprepct.c pre_process_data expands the bottom of the downsampled
//     buffer): the ceil(H / 2) true chroma rows are computed - the source row clamped to H - 1, which only matters for odd
//     H - and the last of them is repeated downwards.  Clamping the full-resolution row instead differs at every even H
//     that is no multiple of 16 (40 x 56 is the smallest case that shows it)
//   - forward DCT: jfdctint.c jpeg_fdct_islow on sample - 128 (CONST_BITS 13, PASS1_BITS 2, rows then columns); the output
//     is scaled by 8
//   - quantization: jcdctmgr.c, k = (|c| + 4 q) / (8 q) with the sign restored (plain truncating division: what
//     libjpeg-turbo's reciprocal form computes); dequantization k * q in int32
// and the inverse half is jpeg_islow.h, the functions the file reader (jpeg_decode.hip) decodes with.
// The saturation rule of the reader holds here as well (jpeg_decode.hip idct_forms_agree): libjpeg-turbo's C and SIMD IDCT
// forms agree only while every dequantized coefficient and every column-pass value lies within +-16383 and every descaled
// sample within [-512, 511].  A block outside raises its image's flag and the caller recomputes that image with Pillow.
// Two launches for the batch: one thread per 8 x 8 block of every component (gather, FDCT, quantize, bounds, IDCT, eight
// 8-byte row stores into the component plane), then one thread per 4 output pixels (upsampling + colour).
//
// pixelate = Image.resize(BOX) down + Image.resize(NEAREST) up.  The coefficient and index tables are computed on the host
// in double (Pillow's precompute_coeffs / normalize_coeffs_8bpc and the accumulating affine scan); the device applies
// them: clip8(((1 << 21) + sum px * k) >> 22) along one axis into a uint8 image (Pillow rounds between its two passes, so
// the intermediate is uint8 here too), then the gather.  The sums are 64-bit: the kernel does not rely on the weights of a
// row summing to 2^22.
//
// There is no floating point in this file.  Every function that computes is __host__ __device__: oadg_jpeg_recompress_host
// and oadg_pil_pixelate_host run the same source without a GPU (tests/test_recompress.py).
#include <stdlib.h>
#include <string.h>
#include "common.h"
#include "jpeg_islow.h"
#include "oadg_hip.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------------
// JPEG round trip: shared by the device kernels and the host twin

// An image's component planes in its workspace slot: cbw x cbh chroma blocks (= 16 x 16 MCUs), twice as many luma blocks
// each way.  Y at 0 (row stride cbw * 16), Cb at cbw * cbh * 256, Cr at cbw * cbh * 320 (row stride cbw * 8).
struct Planes {
    int H, W, cbw, cbh;
    __host__ __device__ Planes(int h, int w) : H(h), W(w), cbw((w + 15) / 16), cbh((h + 15) / 16) {}
    __host__ __device__ long blocks() const { return (long)cbw * cbh * 6; }
    __host__ __device__ long slot() const { return blocks() * 64; }
    __host__ __device__ long offset(int comp) const { return comp ? (long)cbw * cbh * (192 + 64 * comp) : 0; }
    __host__ __device__ int stride(int comp) const { return comp ? cbw * 8 : cbw * 16; }
};

// jccolor.c rgb_ycc_convert, one component (0 = Y, 1 = Cb, 2 = Cr) of the pixel at p (R, G, B)
__host__ __device__ __forceinline__ int rgb_to_ycc(const uint8_t* p, int comp) {
    const int r = p[0], g = p[1], b = p[2];
    if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// the 64 samples - 128 of block (bx, by) of a component, row-major, with libjpeg's edge padding (see the file comment)
__host__ __device__ __forceinline__ void gather_block(const uint8_t* img, int H, int W, int comp, int bx, int by, int* d) {
    if (comp == 0) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int y = by * 8 + r < H ? by * 8 + r : H - 1;
            const uint8_t* row = img + (long)y * W * 3;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int x = bx * 8 + c < W ? bx * 8 + c : W - 1;
                d[r * 8 + c] = rgb_to_ycc(row + (long)x * 3, 0) - 128;
            }
        }
        return;
    }
    const int ch = (H + 1) / 2;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int cy = by * 8 + r < ch ? by * 8 + r : ch - 1;          // bottom edge: the last DOWNSAMPLED row repeats
        const uint8_t* r0 = img + (long)(2 * cy) * W * 3;
        const uint8_t* r1 = img + (long)(2 * cy + 1 < H ? 2 * cy + 1 : H - 1) * W * 3;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int cx = bx * 8 + c;
            const long x0 = (long)(2 * cx < W ? 2 * cx : W - 1) * 3;     // right edge: the full-resolution column is clamped
            const long x1 = (long)(2 * cx + 1 < W ? 2 * cx + 1 : W - 1) * 3;
            const int sum = rgb_to_ycc(r0 + x0, comp) + rgb_to_ycc(r0 + x1, comp) + rgb_to_ycc(r1 + x0, comp) +
                            rgb_to_ycc(r1 + x1, comp);
            d[r * 8 + c] = ((sum + 1 + (cx & 1)) >> 2) - 128;
        }
    }
}

// One 1-D pass of jfdctint.c jpeg_fdct_islow over d[0], d[s], ... d[7 s], in place.  Outputs 0 and 4 are shifted left by
// `up` or descaled by `down04`; the others are descaled by `down`.
__host__ __device__ __forceinline__ void fdct_1d(int* d, int s, int up, int down04, int down) {
    const int tmp0 = d[0] + d[7 * s], tmp7 = d[0] - d[7 * s];
    const int tmp1 = d[s] + d[6 * s], tmp6 = d[s] - d[6 * s];
    const int tmp2 = d[2 * s] + d[5 * s], tmp5 = d[2 * s] - d[5 * s];
    const int tmp3 = d[3 * s] + d[4 * s], tmp4 = d[3 * s] - d[4 * s];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    d[0] = down04 ? descale(tmp10 + tmp11, down04) : (tmp10 + tmp11) * (1 << up);
    d[4 * s] = down04 ? descale(tmp10 - tmp11, down04) : (tmp10 - tmp11) * (1 << up);
    int z1 = (tmp12 + tmp13) * JFIX(0.541196100);
    d[2 * s] = descale(z1 + tmp13 * JFIX(0.765366865), down);
    d[6 * s] = descale(z1 + tmp12 * (-JFIX(1.847759065)), down);
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * JFIX(1.175875602);
    const int a4 = tmp4 * JFIX(0.298631336), a5 = tmp5 * JFIX(2.053119869);
    const int a6 = tmp6 * JFIX(3.072711026), a7 = tmp7 * JFIX(1.501321110);
    z1 *= -JFIX(0.899976223);
    z2 *= -JFIX(2.562915447);
    z3 *= -JFIX(1.961570560);
    z4 *= -JFIX(0.390180644);
    z3 += z5;
    z4 += z5;
    d[7 * s] = descale(a4 + z1 + z3, down);
    d[5 * s] = descale(a5 + z2 + z4, down);
    d[3 * s] = descale(a6 + z2 + z3, down);
    d[s] = descale(a7 + z1 + z4, down);
}

// d: 64 samples - 128, row-major -> the coefficients scaled by 8, d[v * 8 + u] = vertical frequency v, horizontal u
__host__ __device__ __forceinline__ void fdct_islow(int* d) {
#pragma unroll
    for (int r = 0; r < 8; ++r) fdct_1d(d + r * 8, 1, kPass1Bits, 0, kConstBits - kPass1Bits);
#pragma unroll
    for (int c = 0; c < 8; ++c) fdct_1d(d + c, 8, 0, kPass1Bits, kConstBits + kPass1Bits);
}

// d: fdct_islow's output; q: the component's table in natural order (q[v * 8 + u], every entry >= 1) -> in: the dequantized
// coefficients as idct_islow reads them (column-major: in[u * 8 + v]).  Returns the sum of their magnitudes.
__host__ __device__ __forceinline__ int quantize_dequantize(const int* d, const uint16_t* q, int* in) {
    int mag = 0;
#pragma unroll
    for (int v = 0; v < 8; ++v) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int c = d[v * 8 + u];
            const unsigned qv = q[v * 8 + u] ? q[v * 8 + u] : 1u;
            const unsigned k = ((unsigned)(c < 0 ? -c : c) + 4u * qv) / (8u * qv);
            const int deq = (int)(k * qv);
            mag += deq;
            in[u * 8 + v] = c < 0 ? -deq : deq;
        }
    }
    return mag;
}

// Which of the three bounds of the saturation rule the dequantized block `in` (column-major) breaks: bit 0 a coefficient
// outside +-16383, bit 1 a column-pass value outside +-16383, bit 2 a descaled sample outside [-512, 511].  0: libjpeg-turbo's
// C and SIMD IDCT forms both compute what idct_islow computes (jpeg_decode.hip idct_forms_agree has the reasoning).
enum { kBoundCoef = 1, kBoundColumn = 2, kBoundSample = 4 };
__host__ __device__ __forceinline__ int idct_bounds(const int* in) {
    int broken = 0, ws[64], o[8];
#pragma unroll
    for (int k = 0; k < 64; ++k)
        if (in[k] < -16383 || in[k] > 16383) broken |= kBoundCoef;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int* c = in + u * 8;
        idct_1d(c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], o);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            ws[r * 8 + u] = descale(o[r], kConstBits - kPass1Bits);
            if (ws[r * 8 + u] < -16383 || ws[r * 8 + u] > 16383) broken |= kBoundColumn;
        }
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int* w = ws + r * 8;
        idct_1d(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], o);
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            const int v = descale(o[x], kConstBits + kPass1Bits + 3);
            if (v < -512 || v > 511) broken |= kBoundSample;
        }
    }
    return broken;
}

// A block whose dequantized magnitudes sum to S has samples within 0.25 S and column-pass values within 4 * 1.39 S
// (jpeg_decode.hip kPlainSum): at S <= 2000 it is inside all three bounds and is not looked at further.
constexpr int kPlainSum = 2000;

// block b of an image (luma blocks first, then Cb, then Cr; row-major in each grid): gather .. IDCT -> px (row-major), the
// component and the block's position.  Returns whether the block is inside the bounds of the saturation rule.
__host__ __device__ __forceinline__ bool recompress_block(const uint8_t* img, const Planes& g, const uint16_t* qt, long b,
                                                          uint8_t* px, int& comp, int& bx, int& by) {
    const long luma = (long)g.cbw * g.cbh * 4, chroma = (long)g.cbw * g.cbh;
    comp = b < luma ? 0 : (b < luma + chroma ? 1 : 2);
    const long k = comp ? b - luma - (comp - 1) * chroma : b;
    const int bw = comp ? g.cbw : g.cbw * 2;
    bx = (int)(k % bw);
    by = (int)(k / bw);
    int d[64], in[64];
    gather_block(img, g.H, g.W, comp, bx, by, d);
    fdct_islow(d);
    const int mag = quantize_dequantize(d, qt + (comp ? 64 : 0), in);
    const bool ok = mag <= kPlainSum || idct_bounds(in) == 0;
    idct_islow(in, px);
    return ok;
}

// output pixel (x, y) of an image from its component planes; o = the input's channel order (channel 0 is what the colour
// conversion takes for R)
__host__ __device__ __forceinline__ void recompress_pixel(const uint8_t* planes, const Planes& g, int x, int y, uint8_t* o) {
    const int cw = (g.W + 1) / 2, ch = (g.H + 1) / 2;
    const int Y = planes[(long)y * g.stride(0) + x];
    const int cb = chroma_at(planes + g.offset(1), g.stride(1), cw, ch, 2, 2, x, y);
    const int cr = chroma_at(planes + g.offset(2), g.stride(2), cw, ch, 2, 2, x, y);
    uint8_t bgr[3];
    ycc_to_bgr(Y, cb, cr, bgr);
    o[0] = bgr[2];
    o[1] = bgr[1];
    o[2] = bgr[0];
}

// ------------------------------------------------------------------------------------------------------------------------
// Pillow's resampling: shared by the device kernels and the host twin

__host__ __device__ __forceinline__ uint8_t clip8(long long v) {
    const long long s = v >> 22;
    return (uint8_t)(s < 0 ? 0 : (s > 255 ? 255 : s));
}

// ImagingResampleHorizontal_8bpc / Vertical_8bpc for one output pixel: the taps are the pixels p + t * step for t in
// [lo, lo + cnt) of a line of `size` pixels (taps outside it are left out: the host builds none), weights k[0 .. cnt)
__host__ __device__ __forceinline__ void resample_pixel(const uint8_t* p, long step, int size, int lo, int cnt,
                                                        const int32_t* k, uint8_t* o) {
    long long s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
    for (int t = 0; t < cnt; ++t) {
        const int i = lo + t;
        if (i < 0 || i >= size) continue;
        const uint8_t* q = p + (long)i * step;
        s0 += (long long)q[0] * k[t];
        s1 += (long long)q[1] * k[t];
        s2 += (long long)q[2] * k[t];
    }
    o[0] = clip8(s0);
    o[1] = clip8(s1);
    o[2] = clip8(s2);
}

// pixel (oy, ox) of image `src` [H][W][3] resampled along `axis` (0: rows, the output is [out_size][W][3]; 1: columns,
// [H][out_size][3])
__host__ __device__ __forceinline__ void box_pixel(const uint8_t* src, int H, int W, int axis, const int32_t* bounds,
                                                   const int32_t* coeffs, int ksize, int oy, int ox, uint8_t* o) {
    const int i = axis ? ox : oy;
    const int lo = bounds[2 * i], cnt = bounds[2 * i + 1] < ksize ? bounds[2 * i + 1] : ksize;
    if (axis) resample_pixel(src + (long)oy * W * 3, 3, W, lo, cnt, coeffs + (long)i * ksize, o);
    else resample_pixel(src + (long)ox * 3, (long)W * 3, H, lo, cnt, coeffs + (long)i * ksize, o);
}

// ImagingScaleAffine with the NEAREST filter: pixel (y, x) of the output = src[ymap[y]][xmap[x]], 0 where the scan left the
// source (an index outside it)
__host__ __device__ __forceinline__ void nearest_pixel(const uint8_t* src, int h, int w, const int32_t* ymap,
                                                       const int32_t* xmap, int y, int x, uint8_t* o) {
    const int sy = ymap[y], sx = xmap[x];
    if (sy < 0 || sy >= h || sx < 0 || sx >= w) {
        o[0] = o[1] = o[2] = 0;
        return;
    }
    const uint8_t* p = src + ((long)sy * w + sx) * 3;
    o[0] = p[0];
    o[1] = p[1];
    o[2] = p[2];
}

// ------------------------------------------------------------------------------------------------------------------------
// device stage

__global__ __launch_bounds__(256) void recompress_block_kernel(const uint8_t* __restrict__ in, int H, int W,
                                                               const uint16_t* __restrict__ qt,
                                                               uint8_t* __restrict__ planes, int32_t* __restrict__ flags) {
    const Planes g(H, W);
    const long b = (long)blockIdx.x * 256 + threadIdx.x;
    if (b >= g.blocks()) return;
    const int img = blockIdx.y;
    uint8_t px[64];
    int comp, bx, by;
    if (!recompress_block(in + (long)img * H * W * 3, g, qt, b, px, comp, bx, by)) flags[img] = 1;
    uint8_t* dst = planes + (long)img * g.slot() + g.offset(comp) + (long)by * 8 * g.stride(comp) + bx * 8;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        uint2 v;
        v.x = px[r * 8] | (px[r * 8 + 1] << 8) | (px[r * 8 + 2] << 16) | ((unsigned)px[r * 8 + 3] << 24);
        v.y = px[r * 8 + 4] | (px[r * 8 + 5] << 8) | (px[r * 8 + 6] << 16) | ((unsigned)px[r * 8 + 7] << 24);
        *reinterpret_cast<uint2*>(dst + (long)r * g.stride(comp)) = v;
    }
}

// one thread per 4 horizontally adjacent output pixels: 12 bytes out (three 4-byte stores when the row allows it)
__global__ __launch_bounds__(256) void recompress_color_kernel(const uint8_t* __restrict__ planes,
                                                               uint8_t* __restrict__ out, int n, int H, int W, int aligned) {
    const Planes g(H, W);
    const int W4 = (W + 3) >> 2;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)n * H * W4) return;
    const int gx = (int)(t % W4);
    const long r = t / W4;
    const int y = (int)(r % H), img = (int)(r / H);
    const uint8_t* pl = planes + (long)img * g.slot();
    uint8_t* o = out + (((long)img * H + y) * W + gx * 4) * 3;
    const int x0 = gx * 4;
    if (aligned && x0 + 4 <= W) {
        uint8_t px[12];
#pragma unroll
        for (int k = 0; k < 4; ++k) recompress_pixel(pl, g, x0 + k, y, px + 3 * k);
        unsigned* o4 = reinterpret_cast<unsigned*>(o);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            o4[k] = px[4 * k] | (px[4 * k + 1] << 8) | (px[4 * k + 2] << 16) | ((unsigned)px[4 * k + 3] << 24);
    } else {
        for (int k = 0; k < 4 && x0 + k < W; ++k) recompress_pixel(pl, g, x0 + k, y, o + 3 * k);
    }
}

// one thread per output pixel of the batch
__global__ __launch_bounds__(256) void pil_box_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int n,
                                                      int H, int W, int axis, int oh, int ow,
                                                      const int32_t* __restrict__ bounds,
                                                      const int32_t* __restrict__ coeffs, int ksize) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)n * oh * ow) return;
    const int ox = (int)(t % ow);
    const long r = t / ow;
    const int oy = (int)(r % oh), img = (int)(r / oh);
    box_pixel(src + (long)img * H * W * 3, H, W, axis, bounds, coeffs, ksize, oy, ox, dst + t * 3);
}

__global__ __launch_bounds__(256) void pil_nearest_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int n,
                                                          int h, int w, int H, int W, const int32_t* __restrict__ ymap,
                                                          const int32_t* __restrict__ xmap) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)n * H * W) return;
    const int x = (int)(t % W);
    const long r = t / W;
    const int y = (int)(r % H), img = (int)(r / H);
    nearest_pixel(src + (long)img * h * w * 3, h, w, ymap, xmap, y, x, dst + t * 3);
}

constexpr long kMaxGrid = 0x7fffffffL;

}  // namespace

extern "C" size_t oadg_jpeg_recompress_workspace_bytes(int n, int H, int W) {
    if (n < 1 || H < 1 || W < 1) return 0;
    return (size_t)n * (size_t)Planes(H, W).slot();
}

extern "C" int oadg_jpeg_recompress_u8(const uint8_t* in, int n, int H, int W, const uint16_t* qt, uint8_t* planes,
                                       size_t planes_bytes, uint8_t* out, int32_t* flags, void* stream) {
    if (!in || !qt || !planes || !out || !flags || n < 1 || n > 65535 || H < 1 || W < 1) return OADG_EARG;
    if ((uintptr_t)planes % 8) return OADG_EARG;
    if (planes_bytes < oadg_jpeg_recompress_workspace_bytes(n, H, W)) return OADG_ESIZE;
    const Planes g(H, W);
    const long threads = (long)n * H * ((W + 3) / 4);
    if ((g.blocks() + 255) / 256 > kMaxGrid || (threads + 255) / 256 > kMaxGrid) return OADG_EARG;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(flags, 0, (size_t)n * sizeof(int32_t), s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(recompress_block_kernel, dim3((unsigned)oadg_cdiv(g.blocks(), 256), (unsigned)n), dim3(256), 0, s, in,
                       H, W, qt, planes, flags);
    OADG_LAUNCH_CHECK();
    const int aligned = (W % 4 == 0) && ((uintptr_t)out % 4 == 0);
    hipLaunchKernelGGL(recompress_color_kernel, dim3((unsigned)oadg_cdiv(threads, 256)), dim3(256), 0, s,
                       (const uint8_t*)planes, out, n, H, W, aligned);
    OADG_LAUNCH_CHECK();
    return OADG_OK;
}

extern "C" int oadg_jpeg_recompress_host(const uint8_t* in, int n, int H, int W, const uint16_t* qt_host, uint8_t* out,
                                         int32_t* flags) {
    if (!in || !qt_host || !out || !flags || n < 1 || H < 1 || W < 1) return OADG_EARG;
    for (int k = 0; k < 128; ++k)
        if (qt_host[k] < 1) return OADG_EARG;
    const Planes g(H, W);
    uint8_t* planes = (uint8_t*)malloc((size_t)g.slot());
    if (!planes) return OADG_EIO;
    for (int i = 0; i < n; ++i) {
        const uint8_t* img = in + (long)i * H * W * 3;
        flags[i] = 0;
        for (long b = 0; b < g.blocks(); ++b) {
            uint8_t px[64];
            int comp, bx, by;
            if (!recompress_block(img, g, qt_host, b, px, comp, bx, by)) flags[i] = 1;
            for (int r = 0; r < 8; ++r)
                memcpy(planes + g.offset(comp) + ((long)by * 8 + r) * g.stride(comp) + bx * 8, px + r * 8, 8);
        }
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) recompress_pixel(planes, g, x, y, out + (((long)i * H + y) * W + x) * 3);
    }
    free(planes);
    return OADG_OK;
}

extern "C" int oadg_jpeg_recompress_bounds_host(const int32_t* dequantized) {
    if (!dequantized) return OADG_EARG;
    int in[64];
    for (int k = 0; k < 64; ++k) in[k] = dequantized[k];
    return idct_bounds(in);
}

static int box_args_ok(int n, int H, int W, int axis, int out_size, int ksize) {
    return n >= 1 && H >= 1 && W >= 1 && (axis == 0 || axis == 1) && out_size >= 1 && ksize >= 1;
}

extern "C" int oadg_pil_box_resize_u8(const uint8_t* src, uint8_t* dst, int n, int H, int W, int axis, int out_size,
                                      const int32_t* bounds, const int32_t* coeffs, int ksize, void* stream) {
    if (!src || !dst || !bounds || !coeffs || !box_args_ok(n, H, W, axis, out_size, ksize)) return OADG_EARG;
    const int oh = axis ? H : out_size, ow = axis ? out_size : W;
    const long threads = (long)n * oh * ow;
    if ((threads + 255) / 256 > kMaxGrid) return OADG_EARG;
    hipLaunchKernelGGL(pil_box_kernel, dim3((unsigned)oadg_cdiv(threads, 256)), dim3(256), 0, (hipStream_t)stream, src, dst,
                       n, H, W, axis, oh, ow, bounds, coeffs, ksize);
    OADG_LAUNCH_CHECK();
    return OADG_OK;
}

extern "C" int oadg_pil_nearest_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w, int H, int W,
                                   const int32_t* ymap, const int32_t* xmap, void* stream) {
    if (!src || !dst || !ymap || !xmap || n < 1 || h < 1 || w < 1 || H < 1 || W < 1) return OADG_EARG;
    const long threads = (long)n * H * W;
    if ((threads + 255) / 256 > kMaxGrid) return OADG_EARG;
    hipLaunchKernelGGL(pil_nearest_kernel, dim3((unsigned)oadg_cdiv(threads, 256)), dim3(256), 0, (hipStream_t)stream, src,
                       dst, n, h, w, H, W, ymap, xmap);
    OADG_LAUNCH_CHECK();
    return OADG_OK;
}

extern "C" int oadg_pil_pixelate_host(const uint8_t* in, int n, int H, int W, int oh, int ow, const int32_t* xbounds,
                                      const int32_t* xcoeffs, int xksize, const int32_t* ybounds, const int32_t* ycoeffs,
                                      int yksize, const int32_t* ymap, const int32_t* xmap, uint8_t* out) {
    if (!in || !out || !xbounds || !xcoeffs || !ybounds || !ycoeffs || !ymap || !xmap) return OADG_EARG;
    if (!box_args_ok(n, H, W, 1, ow, xksize) || !box_args_ok(n, H, ow, 0, oh, yksize)) return OADG_EARG;
    uint8_t* wide = (uint8_t*)malloc((size_t)H * ow * 3);       // after the horizontal pass
    uint8_t* small = (uint8_t*)malloc((size_t)oh * ow * 3);     // after the vertical pass
    if (!wide || !small) {
        free(wide);
        free(small);
        return OADG_EIO;
    }
    for (int i = 0; i < n; ++i) {
        const uint8_t* img = in + (long)i * H * W * 3;
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < ow; ++x) box_pixel(img, H, W, 1, xbounds, xcoeffs, xksize, y, x, wide + ((long)y * ow + x) * 3);
        for (int y = 0; y < oh; ++y)
            for (int x = 0; x < ow; ++x) box_pixel(wide, H, ow, 0, ybounds, ycoeffs, yksize, y, x, small + ((long)y * ow + x) * 3);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) nearest_pixel(small, oh, ow, ymap, xmap, y, x, out + (((long)i * H + y) * W + x) * 3);
    }
    free(wide);
    free(small);
    return OADG_OK;
}
