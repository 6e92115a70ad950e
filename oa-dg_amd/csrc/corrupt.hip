// The deterministic image work of the robustness benchmark's corruptions, on a resident uint8 [N, H, W, 3] batch.
//
// Replaces, for `Corrupt.batch` (pipelines/corrupt.py; mmdet/datasets/pipelines/transforms.py:1277-1317 ->
// imagecorruptions.corrupt), the numpy / scipy float64 calls of nine names:
//   gaussian_blur, glass_blur, elastic_transform  scipy.ndimage.gaussian_filter  -> oadg_corrupt_correlate1d (+ epilogue)
//   defocus_blur       scipy.ndimage.correlate of each channel with the disk, mode 'mirror' -> oadg_corrupt_defocus
//   zoom_blur          scipy.ndimage.zoom(order=1) of centre crops, accumulated         -> oadg_corrupt_zoom_blur
//   motion_blur        the package's shift-and-accumulate loop                          -> oadg_corrupt_motion_blur_u8
//   snow               zoom of the drawn layer, motion blur of it, the blend            -> oadg_corrupt_snow_*
//   elastic_transform  scipy.ndimage.map_coordinates(order=1, mode='reflect')           -> oadg_corrupt_elastic
//   brightness, saturate  skimage rgb2hsv / hsv2rgb round trip                           -> oadg_corrupt_hsv
// Every step uses the host's arithmetic type (float64, or float32 where numpy's promotion leaves the host in float32),
// the host's operation order and no contraction (Makefile: -ffp-contract=off; no fma here), so the bytes equal the host
// path's.  The random draws stay on the host (numpy's global stream); the caller uploads them, the filter weights and
// the uint8 -> float tables (computed by numpy, so no device division stands between a byte and its value).
//
// scipy's order-1 interpolation (zoom, map_coordinates): weights w0 = 1 - f, w1 = 1 - w0 (not f: 1 ulp apart in
// float64), the sum t = 0 + v00*wy0*wx0 + v01*wy0*wx1 + v10*wy1*wx0 + v11*wy1*wx1, products left to right.
#include <math.h>
#include "common.h"
#include "../../include/oadg_hip.h"

namespace {

constexpr int TPB = 256;

__host__ __device__ inline int grid_for(long total) {
    const long b = (total + TPB - 1) / TPB;
    return (int)(b < 16384 ? (b < 1 ? 1 : b) : 16384);
}

// index i of a line of n samples, extended as scipy extends it: 0 nearest (edge), 1 reflect (half-sample symmetric,
// period 2n), 2 mirror (reflect-101, period 2n - 2)
__device__ __forceinline__ long fold_index(long i, long n, int mode) {
    if (i >= 0 && i < n) return i;
    if (mode == OADG_CORRUPT_NEAREST || n == 1) return i < 0 ? 0 : n - 1;
    if (mode == OADG_CORRUPT_MIRROR) {
        const long p = 2 * n - 2;
        i = (i < 0 ? -i : i) % p;
        return i >= n ? p - i : i;
    }
    const long p = 2 * n;
    i %= p;
    if (i < 0) i += p;
    return i >= n ? p - 1 - i : i;
}

// map_coordinate(in, len, NI_EXTEND_REFLECT) of scipy: a coordinate folded into range before interpolation
__device__ __forceinline__ double fold_coord_reflect(double in, long len) {
    if (in < 0) {
        if (len <= 1) return 0.0;
        const long sz2 = 2 * len;
        if (in < -sz2) in = (double)(sz2 * (long)(-in / sz2)) + in;
        in = in < -len ? in + sz2 : -in - 1;
    } else if (in > len - 1) {
        if (len <= 1) return 0.0;
        const long sz2 = 2 * len;
        in -= (double)(sz2 * (long)(in / sz2));
        if (in >= len) in = sz2 - in - 1;
    }
    return in;
}

// ---------------------------------------------------------------------------------------------- separable correlation
// scipy's correlate1d with a symmetric kernel: out = a[0]*w[r], then out += (a[-j] + a[j]) * w[r-j] for j = r ... 1
__global__ __launch_bounds__(TPB) void correlate1d_kernel(const void* __restrict__ src, int src_u8,
                                                          const double* __restrict__ lut, double* __restrict__ dst,
                                                          long total, int H, int W, int C, int axis,
                                                          const double* __restrict__ w, int r, int mode) {
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const long x = (i / C) % W, y = (i / C / W) % H;
        const long n = axis == 0 ? H : W, pos = axis == 0 ? y : x, stride = axis == 0 ? (long)W * C : C;
        const long base = i - pos * stride;
        const uint8_t* s8 = (const uint8_t*)src;
        const double* s64 = (const double*)src;
        auto at = [&](long p) -> double {
            const long k = base + fold_index(p, n, mode) * stride;
            return src_u8 ? lut[s8[k]] : s64[k];
        };
        double t = at(pos) * w[r];
        for (int j = -r; j < 0; ++j) t = t + (at(pos + j) + at(pos - j)) * w[r + j];
        dst[i] = t;
    }
}

__global__ __launch_bounds__(TPB) void epilogue_kernel(const double* __restrict__ src, void* __restrict__ dst, long total,
                                                       int kind, double scale) {
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        double v = src[i];
        if (kind == OADG_CORRUPT_TO_F32) {
            ((float*)dst)[i] = (float)(v * scale);
            continue;
        }
        if (kind == OADG_CORRUPT_TO_U8_CLIP) v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
        v = v * 255.0;
        v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);          // (the host's values never leave [0, 255] here)
        ((uint8_t*)dst)[i] = (uint8_t)(int)v;
    }
}

// ---------------------------------------------------------------------------------------------- defocus_blur
// scipy's correlate (mode 'mirror') of each channel: taps in row-major kernel order, |w| > DBL_EPSILON only
__global__ __launch_bounds__(TPB) void defocus_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                      long npix, int H, int W, const int32_t* __restrict__ dydx,
                                                      const double* __restrict__ tw, int ntaps,
                                                      const double* __restrict__ lut) {
    __shared__ double l[256];
    for (int k = threadIdx.x; k < 256; k += TPB) l[k] = lut[k];
    __syncthreads();
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < npix; i += (long)gridDim.x * TPB) {
        const long x = i % W, y = (i / W) % H, img = i / ((long)W * H);
        const uint8_t* s = src + img * (long)H * W * 3;
        double t0 = 0.0, t1 = 0.0, t2 = 0.0;
        for (int k = 0; k < ntaps; ++k) {
            const long yy = fold_index(y + dydx[2 * k], H, OADG_CORRUPT_MIRROR);
            const long xx = fold_index(x + dydx[2 * k + 1], W, OADG_CORRUPT_MIRROR);
            const uint8_t* p = s + (yy * W + xx) * 3;
            const double wk = tw[k];
            t0 = t0 + wk * l[p[0]];
            t1 = t1 + wk * l[p[1]];
            t2 = t2 + wk * l[p[2]];
        }
        const double t[3] = {t0, t1, t2};
        for (int c = 0; c < 3; ++c) {
            const double v = (t[c] < 0.0 ? 0.0 : (t[c] > 1.0 ? 1.0 : t[c])) * 255.0;
            dst[i * 3 + c] = (uint8_t)(int)v;
        }
    }
}

// ---------------------------------------------------------------------------------------------- order-1 zoom
// one interpolation axis of scipy's zoom (order 1, mode 'constant', grid_mode False): output index o of a crop of n
// samples; false when the coordinate lies past the last sample (cval 0)
__device__ __forceinline__ bool zoom_axis(long o, double ratio, long n, long* i0, long* i1, double* w0, double* w1) {
    const double c = (double)o * ratio;
    if (c > (double)(n - 1)) return false;
    const double f0 = floor(c);
    const double f = c - f0;
    *i0 = (long)f0;
    *i1 = *i0 + 1 < n ? *i0 + 1 : (n > 1 ? n - 2 : 0);   // (weight 0: the tap past the end)
    *w0 = 1.0 - f;
    *w1 = 1.0 - *w0;
    return true;
}

// zoom_blur: x = float32(u8 / 255.), out = sum over factors of float32(zoom(crop))[:H, :W], then (x + out) / (nz + 1)
__global__ __launch_bounds__(TPB) void zoom_blur_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                        long npix, int H, int W, const double* __restrict__ ratios,
                                                        const int32_t* __restrict__ geo, int nz,
                                                        const float* __restrict__ lut) {
    __shared__ float l[256];
    for (int k = threadIdx.x; k < 256; k += TPB) l[k] = lut[k];
    __syncthreads();
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < npix; i += (long)gridDim.x * TPB) {
        const long x = i % W, y = (i / W) % H, img = i / ((long)W * H);
        const uint8_t* s = src + img * (long)H * W * 3;
        float out[3] = {0.f, 0.f, 0.f};
        for (int z = 0; z < nz; ++z) {
            const int top = geo[4 * z], left = geo[4 * z + 1], ch = geo[4 * z + 2], cw = geo[4 * z + 3];
            long y0, y1, x0, x1;
            double wy0, wy1, wx0, wx1;
            const bool in = zoom_axis(y, ratios[2 * z], ch, &y0, &y1, &wy0, &wy1) &&
                            zoom_axis(x, ratios[2 * z + 1], cw, &x0, &x1, &wx0, &wx1);
            for (int c = 0; c < 3; ++c) {
                double t = 0.0;
                if (in) {
                    const double v00 = l[s[((top + y0) * W + left + x0) * 3 + c]];
                    const double v01 = l[s[((top + y0) * W + left + x1) * 3 + c]];
                    const double v10 = l[s[((top + y1) * W + left + x0) * 3 + c]];
                    const double v11 = l[s[((top + y1) * W + left + x1) * 3 + c]];
                    t = t + v00 * wy0 * wx0;
                    t = t + v01 * wy0 * wx1;
                    t = t + v10 * wy1 * wx0;
                    t = t + v11 * wy1 * wx1;
                }
                out[c] = out[c] + (float)t;
            }
        }
        const float d = (float)(nz + 1);
        for (int c = 0; c < 3; ++c) {
            float v = (l[s[(y * W + x) * 3 + c]] + out[c]) / d;
            v = (v < 0.f ? 0.f : (v > 1.f ? 1.f : v)) * 255.f;
            dst[i * 3 + c] = (uint8_t)(int)v;
        }
    }
}

// snow: the drawn float64 layer [h, w] zoomed from its centre crop without the trim ([Ho, Wo]), then
// layer[layer < thresh] = 0 and clip to [0, 1]
__global__ __launch_bounds__(TPB) void snow_layer_kernel(const double* __restrict__ src, double* __restrict__ dst,
                                                         long total, int h, int w, int top, int left, int ch, int cw,
                                                         int Ho, int Wo, double ry, double rx, double thresh) {
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const long x = i % Wo, y = (i / Wo) % Ho, img = i / ((long)Wo * Ho);
        const double* s = src + img * (long)h * w;
        long y0, y1, x0, x1;
        double wy0, wy1, wx0, wx1;
        double t = 0.0;
        if (zoom_axis(y, ry, ch, &y0, &y1, &wy0, &wy1) && zoom_axis(x, rx, cw, &x0, &x1, &wx0, &wx1)) {
            t = t + s[(top + y0) * w + left + x0] * wy0 * wx0;
            t = t + s[(top + y0) * w + left + x1] * wy0 * wx1;
            t = t + s[(top + y1) * w + left + x0] * wy1 * wx0;
            t = t + s[(top + y1) * w + left + x1] * wy1 * wx1;
        }
        if (t < thresh) t = 0.0;
        dst[i] = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    }
}

// ---------------------------------------------------------------------------------------------- motion blur
// the package's loop: blurred = blurred + k[i] * shift(x, dx_i, dy_i) (edge-replicating shift), float64, in order;
// taps [N][T][2] = (dx, dy) per image, counts[N] = the taps before the loop's early break
__global__ __launch_bounds__(TPB) void motion_blur_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                             long total, int H, int W, const int32_t* __restrict__ taps,
                                                             const int32_t* __restrict__ counts,
                                                             const double* __restrict__ k, int T) {
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const long c = i % 3, x = (i / 3) % W, y = (i / 3 / W) % H, img = i / (3L * W * H);
        const uint8_t* s = src + img * (long)H * W * 3;
        const int32_t* tp = taps + img * 2L * T;
        const int n = counts[img] < T ? counts[img] : T;
        double acc = 0.0;
        for (int j = 0; j < n; ++j) {
            long sy = y - tp[2 * j + 1], sx = x - tp[2 * j];
            sy = sy < 0 ? 0 : (sy > H - 1 ? H - 1 : sy);
            sx = sx < 0 ? 0 : (sx > W - 1 ? W - 1 : sx);
            acc = acc + k[j] * (double)s[(sy * W + sx) * 3 + c];
        }
        acc = acc < 0.0 ? 0.0 : (acc > 255.0 ? 255.0 : acc);
        dst[i] = (uint8_t)(int)acc;
    }
}

// snow's layer: the same loop over a float64 plane [Ho, Wo], then np.round(layer * 255).astype(uint8)
__global__ __launch_bounds__(TPB) void motion_blur_f64_kernel(const double* __restrict__ src, uint8_t* __restrict__ dst,
                                                              long total, int H, int W, const int32_t* __restrict__ taps,
                                                              const int32_t* __restrict__ counts,
                                                              const double* __restrict__ k, int T) {
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const long x = i % W, y = (i / W) % H, img = i / ((long)W * H);
        const double* s = src + img * (long)H * W;
        const int32_t* tp = taps + img * 2L * T;
        const int n = counts[img] < T ? counts[img] : T;
        double acc = 0.0;
        for (int j = 0; j < n; ++j) {
            long sy = y - tp[2 * j + 1], sx = x - tp[2 * j];
            sy = sy < 0 ? 0 : (sy > H - 1 ? H - 1 : sy);
            sx = sx < 0 ? 0 : (sx > W - 1 ? W - 1 : sx);
            acc = acc + k[j] * s[sy * W + sx];
        }
        double v = rint(acc * 255.0);
        v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);
        dst[i] = (uint8_t)(int)v;
    }
}

// snow's blend: x = c6*x + (1 - c6)*max(x, gray(x)*1.5 + 0.5) in float32, then x + layer + rot180(layer) in float64
__global__ __launch_bounds__(TPB) void snow_blend_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ q,
                                                         uint8_t* __restrict__ dst, long npix, int h, int w, int Ho,
                                                         int Wo, float c6, float omc6, const float* __restrict__ lut32,
                                                         const double* __restrict__ lut64) {
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < npix; i += (long)gridDim.x * TPB) {
        const long x = i % w, y = (i / w) % h, img = i / ((long)w * h);
        const uint8_t* p = src + i * 3;
        const float x0 = lut32[p[0]], x1 = lut32[p[1]], x2 = lut32[p[2]];
        float g = (float)0.299 * x0;                     // (numpy casts the float64 constants to float32)
        g = g + (float)0.587 * x1;
        g = g + (float)0.114 * x2;
        g = g * 1.5f;
        g = g + 0.5f;
        const uint8_t* qi = q + img * (long)Ho * Wo;
        const double lay = lut64[qi[y * Wo + x]], rot = lut64[qi[(h - 1 - y) * Wo + (w - 1 - x)]];
        const float xs[3] = {x0, x1, x2};
        for (int c = 0; c < 3; ++c) {
            const float m = xs[c] > g ? xs[c] : g;
            float a = c6 * xs[c];
            const float b = omc6 * m;
            a = a + b;
            double v = (double)a + lay;
            v = v + rot;
            v = (v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v)) * 255.0;
            dst[i * 3 + c] = (uint8_t)(int)v;
        }
    }
}

// ---------------------------------------------------------------------------------------------- elastic_transform
// map_coordinates(img[..., c], [y + dy, x + dx], order=1, mode='reflect') on float32 img, output float32
__global__ __launch_bounds__(TPB) void elastic_kernel(const uint8_t* __restrict__ src, const float* __restrict__ dx,
                                                      const float* __restrict__ dy, uint8_t* __restrict__ dst, long npix,
                                                      int H, int W, const float* __restrict__ lut) {
    __shared__ float l[256];
    for (int k = threadIdx.x; k < 256; k += TPB) l[k] = lut[k];
    __syncthreads();
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < npix; i += (long)gridDim.x * TPB) {
        const long x = i % W, y = (i / W) % H, img = i / ((long)W * H);
        const uint8_t* s = src + img * (long)H * W * 3;
        const double cy = fold_coord_reflect((double)y + (double)dy[i], H);
        const double cx = fold_coord_reflect((double)x + (double)dx[i], W);
        const double fy0 = floor(cy), fx0 = floor(cx);
        const double wy0 = 1.0 - (cy - fy0), wx0 = 1.0 - (cx - fx0);
        const double wy1 = 1.0 - wy0, wx1 = 1.0 - wx0;
        const long y0 = fold_index((long)fy0, H, OADG_CORRUPT_REFLECT), y1 = fold_index((long)fy0 + 1, H, OADG_CORRUPT_REFLECT);
        const long x0 = fold_index((long)fx0, W, OADG_CORRUPT_REFLECT), x1 = fold_index((long)fx0 + 1, W, OADG_CORRUPT_REFLECT);
        for (int c = 0; c < 3; ++c) {
            double t = 0.0;
            t = t + (double)l[s[(y0 * W + x0) * 3 + c]] * wy0 * wx0;
            t = t + (double)l[s[(y0 * W + x1) * 3 + c]] * wy0 * wx1;
            t = t + (double)l[s[(y1 * W + x0) * 3 + c]] * wy1 * wx0;
            t = t + (double)l[s[(y1 * W + x1) * 3 + c]] * wy1 * wx1;
            float v = (float)t;
            v = (v < 0.f ? 0.f : (v > 1.f ? 1.f : v)) * 255.f;
            dst[i * 3 + c] = (uint8_t)(int)v;
        }
    }
}

// ---------------------------------------------------------------------------------------------- brightness, saturate
// skimage rgb2hsv / hsv2rgb as pipelines/corrupt.py restates them, one pixel at a time in float64
__global__ __launch_bounds__(TPB) void hsv_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, long npix,
                                                  int which, double a, double b, const double* __restrict__ lut) {
    __shared__ double l[256];
    for (int k = threadIdx.x; k < 256; k += TPB) l[k] = lut[k];
    __syncthreads();
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < npix; i += (long)gridDim.x * TPB) {
        const double r = l[src[i * 3]], g = l[src[i * 3 + 1]], bl = l[src[i * 3 + 2]];
        const double mx = fmax(fmax(r, g), bl), mn = fmin(fmin(r, g), bl);
        double v = mx;
        const double delta = mx - mn;
        double s = delta == 0.0 ? 0.0 : delta / v;
        if (v == 0.0) s = 0.0;
        double h = 0.0;
        if (r == v) h = (g - bl) / delta;                 // the later masks override the earlier ones
        if (g == v) h = 2.0 + (bl - r) / delta;
        if (bl == v) h = 4.0 + (r - g) / delta;
        h = h / 6.0;
        {                                                 // numpy's remainder(h, 1.0)
            double m = fmod(h, 1.0);
            if (m != 0.0) {
                if (m < 0.0) m += 1.0;
            } else {
                m = 0.0;
            }
            h = m;
        }
        if (delta == 0.0) h = 0.0;
        if (isnan(h)) h = 0.0;
        if (isnan(s)) s = 0.0;
        if (isnan(v)) v = 0.0;
        if (which == OADG_CORRUPT_BRIGHTNESS) {
            v = v + a;
            v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
        } else {
            s = s * a;
            s = s + b;
            s = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);
        }
        const double h6 = h * 6.0;
        const double hf = floor(h6);
        const double f = h6 - hf;
        const double p = v * (1.0 - s);
        const double q = v * (1.0 - f * s);
        const double t = v * (1.0 - (1.0 - f) * s);
        const int hi = ((int)(uint8_t)(int)hf) % 6;
        double o0, o1, o2;
        switch (hi) {
            case 0: o0 = v; o1 = t; o2 = p; break;
            case 1: o0 = q; o1 = v; o2 = p; break;
            case 2: o0 = p; o1 = v; o2 = t; break;
            case 3: o0 = p; o1 = q; o2 = v; break;
            case 4: o0 = t; o1 = p; o2 = v; break;
            default: o0 = v; o1 = p; o2 = q; break;
        }
        const double o[3] = {o0, o1, o2};
        for (int c = 0; c < 3; ++c) {
            const double e = (o[c] < 0.0 ? 0.0 : (o[c] > 1.0 ? 1.0 : o[c])) * 255.0;
            dst[i * 3 + c] = (uint8_t)(int)e;
        }
    }
}

}  // namespace

extern "C" {

int oadg_corrupt_correlate1d(const void* src, int src_u8, const double* lut, double* dst, int N, int H, int W, int C,
                             int axis, const double* weights, int radius, int mode, void* stream) {
    if (!src || !dst || !weights || (src_u8 && !lut) || N < 1 || H < 1 || W < 1 || C < 1 || axis < 0 || axis > 1 ||
        radius < 0 || mode < OADG_CORRUPT_NEAREST || mode > OADG_CORRUPT_MIRROR || (const void*)dst == src)
        return OADG_EARG;
    const long total = (long)N * H * W * C;
    hipLaunchKernelGGL(correlate1d_kernel, dim3(grid_for(total)), dim3(TPB), 0, (hipStream_t)stream, src, src_u8, lut,
                       dst, total, H, W, C, axis, weights, radius, mode);
    OADG_LAUNCH_CHECK();
    return OADG_OK;
}

int oadg_corrupt_epilogue(const double* src, void* dst, long n, int kind, double scale, void* stream) {
    if (!src || !dst || n < 1 || kind < OADG_CORRUPT_TO_U8_CLIP || kind > OADG_CORRUPT_TO_F32) return OADG_EARG;
    hipLaunchKernelGGL(epilogue_kernel, dim3(grid_for(n)), dim3(TPB), 0, (hipStream_t)stream, src, dst, n, kind, scale);
    OADG_LAUNCH_CHECK();
    return OADG_OK;
}

int oadg_corrupt_defocus(const uint8_t* src, uint8_t* dst, int N, int H, int W, const int32_t* dydx,
                         const double* weights, int ntaps, const double* lut, void* stream) {
    if (!src || !dst || src == dst || !dydx || !weights || !lut || N < 1 || H < 1 || W < 1 || ntaps < 1)
        return OADG_EARG;
    const long npix = (long)N * H * W;
    hipLaunchKernelGGL(defocus_kernel, dim3(grid_for(npix)), dim3(TPB), 0, (hipStream_t)stream, src, dst, npix, H, W,
                       dydx, weights, ntaps, lut);
    OADG_LAUNCH_CHECK();
    return OADG_OK;
}

int oadg_corrupt_zoom_blur(const uint8_t* src, uint8_t* dst, int N, int H, int W, const double* ratios,
                           const int32_t* geo, int nz, const float* lut, void* stream) {
    if (!src || !dst || src == dst || !ratios || !geo || !lut || N < 1 || H < 1 || W < 1 || nz < 1) return OADG_EARG;
    const long npix = (long)N * H * W;
    hipLaunchKernelGGL(zoom_blur_kernel, dim3(grid_for(npix)), dim3(TPB), 0, (hipStream_t)stream, src, dst, npix, H, W,
                       ratios, geo, nz, lut);
    OADG_LAUNCH_CHECK();
    return OADG_OK;
}

int oadg_corrupt_snow_layer(const double* src, double* dst, int N, int h, int w, int top, int left, int ch, int cw,
                            int Ho, int Wo, double ry, double rx, double thresh, void* stream) {
    if (!src || !dst || N < 1 || h < 1 || w < 1 || Ho < 1 || Wo < 1 || ch < 1 || cw < 1 || top < 0 || left < 0 ||
        top + ch > h || left + cw > w)
        return OADG_EARG;
    const long total = (long)N * Ho * Wo;
    hipLaunchKernelGGL(snow_layer_kernel, dim3(grid_for(total)), dim3(TPB), 0, (hipStream_t)stream, src, dst, total, h, w,
                       top, left, ch, cw, Ho, Wo, ry, rx, thresh);
    OADG_LAUNCH_CHECK();
    return OADG_OK;
}

int oadg_corrupt_motion_blur_u8(const uint8_t* src, uint8_t* dst, int N, int H, int W, const int32_t* taps,
                                const int32_t* counts, const double* kernel, int T, void* stream) {
    if (!src || !dst || src == dst || !taps || !counts || !kernel || N < 1 || H < 1 || W < 1 || T < 1) return OADG_EARG;
    const long total = (long)N * H * W * 3;
    hipLaunchKernelGGL(motion_blur_u8_kernel, dim3(grid_for(total)), dim3(TPB), 0, (hipStream_t)stream, src, dst, total,
                       H, W, taps, counts, kernel, T);
    OADG_LAUNCH_CHECK();
    return OADG_OK;
}

int oadg_corrupt_motion_blur_f64(const double* src, uint8_t* dst, int N, int H, int W, const int32_t* taps,
                                 const int32_t* counts, const double* kernel, int T, void* stream) {
    if (!src || !dst || !taps || !counts || !kernel || N < 1 || H < 1 || W < 1 || T < 1) return OADG_EARG;
    const long total = (long)N * H * W;
    hipLaunchKernelGGL(motion_blur_f64_kernel, dim3(grid_for(total)), dim3(TPB), 0, (hipStream_t)stream, src, dst, total,
                       H, W, taps, counts, kernel, T);
    OADG_LAUNCH_CHECK();
    return OADG_OK;
}

int oadg_corrupt_snow_blend(const uint8_t* src, const uint8_t* layer, uint8_t* dst, int N, int h, int w, int Ho, int Wo,
                            float c6, float one_minus_c6, const float* lut32, const double* lut64, void* stream) {
    if (!src || !layer || !dst || src == dst || !lut32 || !lut64 || N < 1 || h < 1 || w < 1 || Ho < h || Wo < w)
        return OADG_EARG;
    const long npix = (long)N * h * w;
    hipLaunchKernelGGL(snow_blend_kernel, dim3(grid_for(npix)), dim3(TPB), 0, (hipStream_t)stream, src, layer, dst, npix,
                       h, w, Ho, Wo, c6, one_minus_c6, lut32, lut64);
    OADG_LAUNCH_CHECK();
    return OADG_OK;
}

int oadg_corrupt_elastic(const uint8_t* src, const float* dx, const float* dy, uint8_t* dst, int N, int H, int W,
                         const float* lut, void* stream) {
    if (!src || !dx || !dy || !dst || src == dst || !lut || N < 1 || H < 1 || W < 1) return OADG_EARG;
    const long npix = (long)N * H * W;
    hipLaunchKernelGGL(elastic_kernel, dim3(grid_for(npix)), dim3(TPB), 0, (hipStream_t)stream, src, dx, dy, dst, npix,
                       H, W, lut);
    OADG_LAUNCH_CHECK();
    return OADG_OK;
}

int oadg_corrupt_hsv(const uint8_t* src, uint8_t* dst, long npix, int which, double a, double b, const double* lut,
                     void* stream) {
    if (!src || !dst || !lut || npix < 1 || which < OADG_CORRUPT_BRIGHTNESS || which > OADG_CORRUPT_SATURATE)
        return OADG_EARG;
    hipLaunchKernelGGL(hsv_kernel, dim3(grid_for(npix)), dim3(TPB), 0, (hipStream_t)stream, src, dst, npix, which, a, b,
                       lut);
    OADG_LAUNCH_CHECK();
    return OADG_OK;
}

}  // extern "C"
