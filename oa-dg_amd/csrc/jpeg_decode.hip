// JPEG file -> BGR uint8 [H][W][3]: entropy stage on the HOST (one call per image, without the interpreter lock), pixel
// stage on the DEVICE (one batch, two launches), written from ITU-T T.81.
//
// Replaces, for the input path of tools/train.py on the Diverse-Weather (S-DGOD) JPEG files:
//   mmdet/datasets/pipelines/loading.py:18-98  LoadImageFromFile (mmcv.imfrombytes -> cv2.imdecode, colour, BGR)
// The bar is byte equality with PIL / OpenCV under their defaults (libjpeg-turbo: JDCT_ISLOW, fancy upsampling, no block
// smoothing), so every stage after the Huffman decode restates libjpeg's integer arithmetic exactly:
//   - IDCT: jidctint.c jpeg_idct_islow (Loeffler-Ligtenberg-Moschytz, CONST_BITS 13, PASS1_BITS 2, columns then rows),
//     then the post-IDCT range limit range_limit[v & 1023] = clamp(((v + 512) mod 1024) - 512 + 128, 0, 255)
//   - chroma: jdsample.c h2v1 / h2v2 "fancy" triangle upsampling with its alternating rounding biases, edges replicated at
//     the component's true extent; plain replication when the component is at most 2 samples wide (libjpeg's own rule)
//   - colour: jdcolor.c ycc_rgb_convert with the IJG fixed-point tables (SCALEBITS 16)
// Covered: SOF0 / SOF1, 8-bit, Huffman, one scan holding every component, 8- or 16-bit DQT, DRI / RSTn, byte stuffing and
// fill bytes, grey or YCbCr with luma sampling 1x1, 2x1 or 2x2 and chroma 1x1.  Everything else returns OADG_EUNSUPPORTED
// (the caller decodes that file with PIL); a truncated or corrupt stream returns OADG_EFORMAT (the caller hands the file to
// PIL, so the error users see is PIL's).
// The rule for untrusted bytes: OADG_OK only for a file PIL loads, with PIL's bytes; no read or write outside the file
// and the caller's buffers whatever the bytes are.  Where in doubt the file is rejected - stricter than libjpeg is fine,
// laxer is not.  What tests/jpeg_cases.py + tests/test_decoder_robustness.py pin (PIL the judge of every file):
//   decoded: fill bytes before any marker (RSTn and EOI too), bytes after EOI, COM / APPn (an APP1 holding a whole JPEG:
//     the size is the outer frame's), tables packed in one segment or one each, defined twice (the last definition
//     holds), placed after SOF, in unused slots, a 16-bit DQT under SOF0, DRI given twice / 0 / beyond the MCU count,
//     grey files with any sampling factors (ignored: one block per MCU), and the colour space as libjpeg infers it
//     (jdapimin.c default_decompress_parms): JFIF wins over an Adobe marker and over component ids, Adobe transform 1 and
//     ids 1,2,3 without JFIF are YCbCr
//   declined (OADG_EUNSUPPORTED): ids 'R','G','B' or Adobe transform 0 without JFIF (RGB-coded), 12-bit, every frame type
//     but SOF0 / SOF1, height 0 / DNL, 4:4:0 and any chroma factor but 1x1, 4 components, a second scan, and a block
//     where libjpeg-turbo's C and SIMD IDCT forms would disagree (idct_forms_agree below: only pathological streams)
//   rejected: a Huffman table with more codes of a length than the length holds or an all-ones code (checked before any
//     lookup entry is written), wrong Tc / Th / Tq / Pq, DC symbols above 15, segment lengths that are short, long (SOF,
//     SOS and DRI lengths must be exact, as in libjpeg) or past the end of the file, a second SOF, SOS before SOF or
//     with other components, ids or tables than the frame defined, spectral selection other than 0 / 63 / 0, restart
//     markers out of order, missing, surplus or without DRI, codes no table assigns, AC runs past coefficient 63, DC
//     categories above 11, data or EOI missing, anything but FF after SOI (PIL knows a JPEG by FF D8 FF) and segments
//     under a reserved marker code (TEM, 02 .. BF, JPGn, DHP, EXP: libjpeg and PIL stop there)
//   swept: every prefix of a file is rejected; every header byte set to 00, FF, b ^ 01, b ^ 80 and 1500 files of
//     extreme coefficients either decode to PIL's bytes or are rejected.
// make -C oa-dg_amd/csrc decoder-asan runs the host stage over all of them under AddressSanitizer + UBSan.
// The IDCT, upsampling and colour functions are __host__ __device__: oadg_jpeg_decode_bgr runs the same source on the host.
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "common.h"
#include "jpeg_islow.h"
#include "oadg_hip.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------------
// pixel stage: the IDCT, upsampling and colour functions are jpeg_islow.h (recompress.hip uses them too)

// output pixel (x, y) of an image whose component planes start at `planes` (sample offsets = the coefficient offsets)
__host__ __device__ __forceinline__ void pixel_bgr(const oadg_jpeg_desc& d, const uint8_t* planes, int x, int y,
                                                   uint8_t* o) {
    const int Y = planes[d.off[0] + (long)y * d.bw[0] * 8 + x];
    if (d.ncomp == 1) {
        o[0] = o[1] = o[2] = (uint8_t)Y;
        return;
    }
    const int hf = d.hmax, vf = d.vmax;
    const int cb = chroma_at(planes + d.off[1], d.bw[1] * 8, d.cw[1], d.ch[1], hf, vf, x, y);
    const int cr = chroma_at(planes + d.off[2], d.bw[2] * 8, d.cw[2], d.ch[2], hf, vf, x, y);
    ycc_to_bgr(Y, cb, cr, o);
}

// ------------------------------------------------------------------------------------------------------------------------
// device stage

// a descriptor the colour kernel may read planes through: every sample it can touch lies inside the image's slot
__device__ __forceinline__ bool desc_ok(const oadg_jpeg_desc& d, int H, int W, long long slot) {
    if ((d.ncomp != 1 && d.ncomp != 3) || d.height != H || d.width != W) return false;
    if (d.ncomp == 3 && (d.hmax < 1 || d.hmax > 2 || d.vmax < 1 || d.vmax > d.hmax)) return false;   // 1x1, 2x1, 2x2
    for (int c = 0; c < d.ncomp; ++c) {
        const int hf = c ? d.hmax : 1, vf = c ? d.vmax : 1;
        if (d.off[c] < 0 || d.off[c] + (long)d.bw[c] * d.bh[c] * 64 > slot) return false;
        if ((long)d.cw[c] * hf < W || (long)d.ch[c] * vf < H || d.cw[c] > d.bw[c] * 8 || d.ch[c] > d.bh[c] * 8)
            return false;
    }
    return true;
}

// one thread per 8 x 8 block of every image in the batch: 16-byte coefficient / table loads (a column each), int32
// dequantization, the islow IDCT, eight 8-byte row stores into the component plane
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const int16_t* __restrict__ coef,
                                                        const oadg_jpeg_desc* __restrict__ desc, long long slot,
                                                        uint8_t* __restrict__ planes) {
    const int img = blockIdx.y;
    const oadg_jpeg_desc& d = desc[img];
    const int nc = d.ncomp;
    if (nc != 1 && nc != 3) return;
    long b = (long)blockIdx.x * 256 + threadIdx.x;
    int c = 0;
    long nb = (long)d.bw[0] * d.bh[0];
    while (b >= nb) {
        b -= nb;
        if (++c >= nc) return;
        nb = (long)d.bw[c] * d.bh[c];
    }
    const long base = d.off[c];
    if (base < 0 || base + nb * 64 > slot || (base & 63)) return;      // (the host stage guarantees it; never read past)
    const int16_t* src = coef + (long)img * slot + base + b * 64;
    const uint16_t* q = d.qt[c];
    int in[64];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int4 cv = *reinterpret_cast<const int4*>(src + u * 8);
        const uint4 qv = *reinterpret_cast<const uint4*>(q + u * 8);
        const int cw[4] = {cv.x, cv.y, cv.z, cv.w};
        const unsigned qw[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            in[u * 8 + 2 * k] = (int)(short)(cw[k] & 0xffff) * (int)(qw[k] & 0xffff);
            in[u * 8 + 2 * k + 1] = (cw[k] >> 16) * (int)(qw[k] >> 16);
        }
    }
    uint8_t px[64];
    idct_islow(in, px);
    const int bw = d.bw[c];
    const long bx = b % bw, by = b / bw;
    uint8_t* dst = planes + (long)img * slot + base + by * 8 * (bw * 8) + bx * 8;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        uint2 v;
        v.x = px[r * 8] | (px[r * 8 + 1] << 8) | (px[r * 8 + 2] << 16) | ((unsigned)px[r * 8 + 3] << 24);
        v.y = px[r * 8 + 4] | (px[r * 8 + 5] << 8) | (px[r * 8 + 6] << 16) | ((unsigned)px[r * 8 + 7] << 24);
        *reinterpret_cast<uint2*>(dst + (long)r * bw * 8) = v;
    }
}

// one thread per 4 horizontally adjacent output pixels: upsampling + colour conversion, 12 bytes out (three 4-byte stores
// when the row allows it)
__global__ __launch_bounds__(256) void jpeg_color_kernel(const oadg_jpeg_desc* __restrict__ desc, long long slot,
                                                         const uint8_t* __restrict__ planes, uint8_t* __restrict__ out,
                                                         int n, int H, int W, int aligned) {
    const int W4 = (W + 3) >> 2;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)n * H * W4) return;
    const int gx = (int)(t % W4);
    const long r = t / W4;
    const int y = (int)(r % H), img = (int)(r / H);
    const oadg_jpeg_desc& d = desc[img];
    if (!desc_ok(d, H, W, slot)) return;
    const uint8_t* pl = planes + (long)img * slot;
    uint8_t* o = out + (((long)img * H + y) * W + gx * 4) * 3;
    const int x0 = gx * 4;
    if (aligned && x0 + 4 <= W) {
        uint8_t px[12];
#pragma unroll
        for (int k = 0; k < 4; ++k) pixel_bgr(d, pl, x0 + k, y, px + 3 * k);
        unsigned* o4 = reinterpret_cast<unsigned*>(o);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            o4[k] = px[4 * k] | (px[4 * k + 1] << 8) | (px[4 * k + 2] << 16) | ((unsigned)px[4 * k + 3] << 24);
    } else {
        for (int k = 0; k < 4 && x0 + k < W; ++k) pixel_bgr(d, pl, x0 + k, y, o + 3 * k);
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// host stage: markers + Huffman decoding

// natural (row-major) index of zig-zag position k (T.81 figure A.6)
const uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct ColumnMajorZigzag {
    uint8_t idx[64];
    ColumnMajorZigzag() {
        for (int k = 0; k < 64; ++k) idx[k] = (uint8_t)((kNatural[k] & 7) * 8 + (kNatural[k] >> 3));
    }
};
const ColumnMajorZigzag kZz;       // zig-zag position -> column-major storage index

struct Huff {
    uint16_t fast[512];     // (length << 8) | symbol for codes of at most 9 bits; 0 = longer
    int maxcode[18];        // largest code of each length, -1 if none (maxcode[17]: sentinel)
    int delta[17];          // symbol index = code + delta[length]
    uint8_t vals[256];
    bool defined;
};

// jdhuff.c jpeg_make_d_derived_tbl: canonical codes, with its checks (no code may be all ones)
int build_huff(Huff& t, const uint8_t* counts, const uint8_t* vals, int nvals, bool dc) {
    memset(t.fast, 0, sizeof(t.fast));
    memcpy(t.vals, vals, (size_t)nvals);
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        const int n = counts[l - 1];
        // more codes than the length holds (or one of all ones): checked BEFORE the lookup entries of this length are
        // written - an oversubscribed length would index past fast[]
        if (code + n >= (1 << l)) return OADG_EFORMAT;
        t.maxcode[l] = n ? code + n - 1 : -1;
        t.delta[l] = k - code;
        for (int i = 0; i < n; ++i, ++code, ++k) {
            if (dc && vals[k] > 15) return OADG_EFORMAT;
            if (l <= 9)
                for (int j = 0; j < (1 << (9 - l)); ++j) t.fast[(code << (9 - l)) | j] = (uint16_t)((l << 8) | vals[k]);
        }
        code <<= 1;
    }
    t.maxcode[17] = INT_MAX;
    t.defined = true;
    return OADG_OK;
}

// MSB-first bit reader over one destuffed entropy segment; past its end it feeds zeros and counts them
struct Bits {
    const uint8_t* p;
    const uint8_t* end;
    uint64_t buf = 0;
    int n = 0;
    long over = 0;
    Bits(const uint8_t* a, const uint8_t* b) : p(a), end(b) {}
    inline void fill() {
        while (n <= 56) {
            uint64_t byte = 0;
            if (p < end) byte = *p++;
            else over += 8;
            buf |= byte << (56 - n);
            n += 8;
        }
    }
    inline unsigned peek(int k) const { return (unsigned)(buf >> (64 - k)); }
    inline void skip(int k) { buf <<= k; n -= k; }
    inline int get(int k) { const int v = (int)peek(k); skip(k); return v; }
    // bits consumed beyond the segment's data
    inline bool overrun() const { return over > 0 && (long)n < over; }
};

inline int huff_decode(Bits& b, const Huff& t) {
    const unsigned e = t.fast[b.peek(9)];
    if (e) {
        b.skip((int)(e >> 8));
        return (int)(e & 255);
    }
    const int code16 = (int)b.peek(16);
    for (int l = 10; l <= 16; ++l) {
        const int code = code16 >> (16 - l);
        if (code <= t.maxcode[l]) {
            b.skip(l);
            return t.vals[code + t.delta[l]];
        }
    }
    return -1;
}

inline int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// one block: zero it, DC difference + AC run/size codes in zig-zag order, stored column-major.  The dequantized value of
// every coefficient must stay within int16 (see the file comment).
inline int decode_block(Bits& b, const Huff& dc, const Huff& ac, int& pred, int16_t* blk, const uint16_t* q, long& mag) {
    memset(blk, 0, 64 * sizeof(int16_t));
    b.fill();
    int s = huff_decode(b, dc);
    if (s < 0 || s > 11) return OADG_EFORMAT;
    if (s) pred += extend(b.get(s), s);
    if (pred < -32768 || pred > 32767) return OADG_EFORMAT;
    if ((long)(pred < 0 ? -pred : pred) * q[0] > 32767) return OADG_EUNSUPPORTED;
    blk[0] = (int16_t)pred;
    mag = (long)(pred < 0 ? -pred : pred) * q[0];
    for (int k = 1; k < 64;) {
        if (b.n < 32) b.fill();
        const int rs = huff_decode(b, ac);
        if (rs < 0) return OADG_EFORMAT;
        const int r = rs >> 4;
        s = rs & 15;
        if (s) {
            k += r;
            if (k > 63 || s > 10) return OADG_EFORMAT;
            const int v = extend(b.get(s), s);
            const int pos = kZz.idx[k];
            const long a = (long)(v < 0 ? -v : v) * q[pos];
            if (a > 32767) return OADG_EUNSUPPORTED;
            mag += a;
            blk[pos] = (int16_t)v;
            ++k;
        } else {
            if (r != 15) break;
            k += 16;
        }
    }
    return OADG_OK;
}

// libjpeg-turbo decodes a block with the C form of jidctint.c or with a SIMD form of it, and the two agree only while
// nothing saturates: the SIMD forms add dequantized coefficients and column-pass results in 16-bit lanes and pack the
// column-pass results and the samples with signed saturation, where the C form keeps ints and wraps the sample through
// range_limit[v & 1023].  With every dequantized coefficient and every column-pass value within +-16383 (so that no
// 16-bit sum of two of them wraps and none saturates) and every descaled sample within [-512, 511] (where wrapping and
// clamping give the same byte) both forms compute what idct_islow computes.  A block outside that is declined.
// kPlainSum: a block whose dequantized magnitudes sum to S has samples within 0.25 S (a basis function's amplitude is at
// most cos^2(pi/16) / 4) and column-pass values within 4 * 1.39 S (PASS1_BITS, the largest butterfly gain), so at
// S <= 2000 it is inside all three bounds with room for the fixed-point rounding and is not looked at further.
constexpr long kPlainSum = 2000;

bool idct_forms_agree(const int16_t* blk, const uint16_t* q) {
    int in[64], ws[64], o[8];
    for (int k = 0; k < 64; ++k) {
        in[k] = (int)blk[k] * (int)q[k];
        if (in[k] < -16383 || in[k] > 16383) return false;
    }
    for (int u = 0; u < 8; ++u) {
        const int* c = in + u * 8;
        idct_1d(c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], o);
        for (int r = 0; r < 8; ++r) {
            ws[r * 8 + u] = descale(o[r], kConstBits - kPass1Bits);
            if (ws[r * 8 + u] < -16383 || ws[r * 8 + u] > 16383) return false;
        }
    }
    for (int r = 0; r < 8; ++r) {
        const int* w = ws + r * 8;
        idct_1d(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], o);
        for (int x = 0; x < 8; ++x) {
            const int v = descale(o[x], kConstBits + kPass1Bits + 3);
            if (v < -512 || v > 511) return false;
        }
    }
    return true;
}

inline unsigned be16(const uint8_t* p) { return ((unsigned)p[0] << 8) | p[1]; }

int read_file(const char* path, uint8_t** data, long* size) {
    FILE* f = fopen(path, "rb");
    if (!f) return OADG_EIO;
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (n < 0) { fclose(f); return OADG_EIO; }
    uint8_t* buf = (uint8_t*)malloc((size_t)n + 1);
    if (!buf) { fclose(f); return OADG_EIO; }
    const size_t got = fread(buf, 1, (size_t)n, f);
    fclose(f);
    if ((long)got != n) { free(buf); return OADG_EIO; }
    *data = buf;
    *size = n;
    return OADG_OK;
}

struct Component { int id, h, v, tq, td, ta; };

struct Decoder {
    const uint8_t* f;
    long size, pos = 2;
    int H = 0, W = 0, nc = 0, sof = -1;
    Component comp[4];
    uint16_t qt[4][64];          // column-major
    bool qdef[4] = {false, false, false, false};
    Huff dc[4], ac[4];
    int restart = 0;
    bool jfif = false, adobe = false;
    int adobe_transform = -1;

    Decoder(const uint8_t* data, long n) : f(data), size(n) {
        for (int i = 0; i < 4; ++i) dc[i].defined = ac[i].defined = false;
    }

    // next marker code at pos (fill bytes skipped), -1 at the end of the file
    int next_marker() {
        while (pos < size && f[pos] != 0xFF) ++pos;       // (libjpeg skips garbage before a marker too, with a warning)
        while (pos < size && f[pos] == 0xFF) ++pos;
        if (pos >= size) return -1;
        return f[pos++];
    }

    int segment(const uint8_t** body, long* len) {
        if (pos + 2 > size) return OADG_EFORMAT;
        const long L = be16(f + pos);
        if (L < 2 || pos + L > size) return OADG_EFORMAT;
        *body = f + pos + 2;
        *len = L - 2;
        pos += L;
        return OADG_OK;
    }

    int parse_sof(const uint8_t* s, long len) {
        if (nc) return OADG_EFORMAT;                       // a second frame header
        if (len < 6) return OADG_EFORMAT;
        H = (int)be16(s + 1);
        W = (int)be16(s + 3);
        nc = s[5];
        if (s[0] != 8) return OADG_EUNSUPPORTED;          // 12-bit samples
        if (W == 0) return OADG_EFORMAT;
        if (H == 0) return OADG_EUNSUPPORTED;             // height given by a DNL marker
        if (nc != 1 && nc != 3) return OADG_EUNSUPPORTED; // CMYK / YCCK, two-component files
        if (len != 6 + 3 * nc) return OADG_EFORMAT;        // (libjpeg: JERR_BAD_LENGTH for a longer one too)
        for (int i = 0; i < nc; ++i) {
            comp[i].id = s[6 + 3 * i];
            comp[i].h = s[7 + 3 * i] >> 4;
            comp[i].v = s[7 + 3 * i] & 15;
            comp[i].tq = s[8 + 3 * i];
            if (comp[i].h < 1 || comp[i].h > 4 || comp[i].v < 1 || comp[i].v > 4 || comp[i].tq > 3) return OADG_EFORMAT;
        }
        return OADG_OK;
    }

    int parse_dqt(const uint8_t* s, long len) {
        long i = 0;
        while (i < len) {
            const int pq = s[i] >> 4, tq = s[i] & 15;
            if (tq > 3 || pq > 1) return OADG_EFORMAT;
            const long need = 1 + 64 * (pq + 1);
            if (i + need > len) return OADG_EFORMAT;
            for (int k = 0; k < 64; ++k)
                qt[tq][kZz.idx[k]] = (uint16_t)(pq ? be16(s + i + 1 + 2 * k) : s[i + 1 + k]);
            qdef[tq] = true;
            i += need;
        }
        return OADG_OK;
    }

    int parse_dht(const uint8_t* s, long len) {
        long i = 0;
        while (i < len) {
            if (i + 17 > len) return OADG_EFORMAT;
            const int tc = s[i] >> 4, th = s[i] & 15;
            if (tc > 1 || th > 3) return OADG_EFORMAT;
            int total = 0;
            for (int k = 0; k < 16; ++k) total += s[i + 1 + k];
            if (total > 256 || i + 17 + total > len) return OADG_EFORMAT;
            const int rc = build_huff(tc ? ac[th] : dc[th], s + i + 1, s + i + 17, total, tc == 0);
            if (rc) return rc;
            i += 17 + total;
        }
        return OADG_OK;
    }

    // a marker code no segment may start with here.  Below 0xC0 (TEM, the reserved codes, a stuffed zero), JPGn, DHP and EXP
    // stop libjpeg (jdmarker.c read_markers: JERR_UNKNOWN_MARKER) or PIL's own marker walk ("no marker found"); RSTn and a
    // second SOI are out of place
    static bool stray_marker(int m) {
        return m < 0xC0 || (m >= 0xD0 && m <= 0xD8) || m == 0xDE || m == 0xDF || (m >= 0xF0 && m <= 0xFD);
    }

    // headers up to the frame (for oadg_jpeg_size) or up to the scan
    int headers(bool stop_at_frame, const uint8_t** sos, long* sos_len) {
        if (size < 4 || f[0] != 0xFF || f[1] != 0xD8) return OADG_EUNSUPPORTED;
        if (f[2] != 0xFF) return OADG_EFORMAT;            // (PIL knows a JPEG by FF D8 FF: garbage right after SOI is no image)
        for (;;) {
            const int m = next_marker();
            if (m < 0 || m == 0xD9 || stray_marker(m)) return OADG_EFORMAT;
            const uint8_t* s;
            long len;
            int rc = segment(&s, &len);
            if (rc) return rc;
            if (m == 0xC0 || m == 0xC1) {
                rc = parse_sof(s, len);
                sof = m;
                if (stop_at_frame && (rc == OADG_OK || rc == OADG_EUNSUPPORTED)) return rc;
                if (rc) return rc;
            } else if (m >= 0xC2 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
                // progressive, lossless, differential or arithmetic-coded frames
                if (stop_at_frame && len >= 5) {
                    H = (int)be16(s + 1);
                    W = (int)be16(s + 3);
                }
                return OADG_EUNSUPPORTED;
            } else if (m == 0xCC || m == 0xC8) {
                return OADG_EUNSUPPORTED;
            } else if (m == 0xC4) {
                if ((rc = parse_dht(s, len))) return rc;
            } else if (m == 0xDB) {
                if ((rc = parse_dqt(s, len))) return rc;
            } else if (m == 0xDD) {
                if (len != 2) return OADG_EFORMAT;
                restart = (int)be16(s);
            } else if (m == 0xE0) {
                if (len >= 5 && memcmp(s, "JFIF\0", 5) == 0) jfif = true;
            } else if (m == 0xEE) {
                if (len >= 12 && memcmp(s, "Adobe", 5) == 0) {
                    adobe = true;
                    adobe_transform = s[11];
                }
            } else if (m == 0xDA) {
                if (!nc) return OADG_EFORMAT;
                *sos = s;
                *sos_len = len;
                return OADG_OK;
            } else if (m == 0xDC) {
                return OADG_EUNSUPPORTED;                 // DNL
            }
        }
    }
};

// Everything the device stage and the host twin need: the descriptor and the quantized coefficients at `coef` (capacity
// in int16 elements).
int entropy_decode(const uint8_t* file, long size, int H, int W, int16_t* coef, size_t capacity, oadg_jpeg_desc* d) {
    Decoder dec(file, size);
    const uint8_t* sos;
    long sos_len;
    int rc = dec.headers(false, &sos, &sos_len);
    if (rc) return rc;
    if (dec.H != H || dec.W != W) return OADG_ESIZE;
    const int nc = dec.nc;
    // colour space as libjpeg infers it (jdapimin.c default_decompress_parms): RGB files are declined
    if (nc == 3) {
        const bool rgb_ids = dec.comp[0].id == 'R' && dec.comp[1].id == 'G' && dec.comp[2].id == 'B';
        if (!dec.jfif && ((dec.adobe && dec.adobe_transform == 0) || (!dec.adobe && rgb_ids))) return OADG_EUNSUPPORTED;
    }
    // scan header
    if (sos_len < 1) return OADG_EFORMAT;
    const int ns = sos[0];
    if (sos_len != 4 + 2 * ns || ns < 1 || ns > 4) return OADG_EFORMAT;      // (libjpeg: the length must be exact)
    if (ns != nc) return OADG_EUNSUPPORTED;               // multi-scan sequential
    for (int i = 0; i < ns; ++i) {
        if (sos[1 + 2 * i] != dec.comp[i].id) return OADG_EUNSUPPORTED;
        dec.comp[i].td = sos[2 + 2 * i] >> 4;
        dec.comp[i].ta = sos[2 + 2 * i] & 15;
        if (dec.comp[i].td > 3 || dec.comp[i].ta > 3) return OADG_EFORMAT;
        if (!dec.dc[dec.comp[i].td].defined || !dec.ac[dec.comp[i].ta].defined) return OADG_EUNSUPPORTED;
        if (!dec.qdef[dec.comp[i].tq]) return OADG_EFORMAT;
    }
    const uint8_t* sp = sos + 1 + 2 * ns;
    if (sp[0] != 0 || sp[1] != 63 || sp[2] != 0) return OADG_EFORMAT;
    // sampling: grey (factors ignored: one block per MCU), or luma 1x1 / 2x1 / 2x2 with chroma 1x1
    int hs[3] = {1, 1, 1}, vs[3] = {1, 1, 1};
    if (nc == 3) {
        for (int i = 0; i < 3; ++i) { hs[i] = dec.comp[i].h; vs[i] = dec.comp[i].v; }
        const bool luma_ok = (hs[0] == 1 && vs[0] == 1) || (hs[0] == 2 && vs[0] == 1) || (hs[0] == 2 && vs[0] == 2);
        if (!luma_ok || hs[1] != 1 || vs[1] != 1 || hs[2] != 1 || vs[2] != 1) return OADG_EUNSUPPORTED;
    }
    memset(d, 0, sizeof(*d));
    const int hmax = hs[0], vmax = vs[0];
    const int mcux = (W + 8 * hmax - 1) / (8 * hmax), mcuy = (H + 8 * vmax - 1) / (8 * vmax);
    long off = 0;
    for (int i = 0; i < nc; ++i) {
        d->h[i] = hs[i];
        d->v[i] = vs[i];
        d->bw[i] = mcux * hs[i];
        d->bh[i] = mcuy * vs[i];
        d->cw[i] = (int)(((long)W * hs[i] + hmax - 1) / hmax);
        d->ch[i] = (int)(((long)H * vs[i] + vmax - 1) / vmax);
        d->off[i] = off;
        off += (long)d->bw[i] * d->bh[i] * 64;
        memcpy(d->qt[i], dec.qt[dec.comp[i].tq], sizeof(d->qt[i]));
    }
    if ((size_t)off > capacity) return OADG_ESIZE;
    // entropy-coded data: destuff into one buffer, splitting it at the restart markers
    const long start = (sp + 3) - file;
    uint8_t* ent = (uint8_t*)malloc((size_t)(size - start) + 1);
    const long mcus = (long)mcux * mcuy;
    const long nseg_want = dec.restart ? (mcus + dec.restart - 1) / dec.restart : 1;
    long* seg = (long*)malloc(sizeof(long) * (size_t)(nseg_want + 1));
    if (!ent || !seg) { free(ent); free(seg); return OADG_EIO; }
    rc = OADG_OK;
    long nseg = 0, w = 0, p = start;
    int end_marker = -1;
    seg[0] = 0;
    while (p < size) {
        const uint8_t* ff = (const uint8_t*)memchr(file + p, 0xFF, (size_t)(size - p));
        const long q = ff ? ff - file : size;
        memcpy(ent + w, file + p, (size_t)(q - p));
        w += q - p;
        p = q;
        if (p >= size) break;
        long m = p + 1;
        while (m < size && file[m] == 0xFF) ++m;          // fill bytes
        if (m >= size) { p = size; break; }
        if (file[m] == 0x00) { ent[w++] = 0xFF; p = m + 1; continue; }
        if (file[m] >= 0xD0 && file[m] <= 0xD7) {
            // RST(k mod 8) must end segment k
            if (!dec.restart || nseg + 1 >= nseg_want || file[m] != 0xD0 + (nseg & 7)) { rc = OADG_EFORMAT; break; }
            seg[++nseg] = w;
            p = m + 1;
            continue;
        }
        end_marker = file[m];
        p = m + 1;
        break;
    }
    seg[nseg + 1] = w;
    if (rc == OADG_OK && (end_marker < 0 || nseg + 1 != nseg_want)) rc = OADG_EFORMAT;     // truncated
    // the markers up to EOI: another scan (multi-scan sequential) or DNL is declined, anything else skipped
    dec.pos = p;
    for (int m = end_marker; rc == OADG_OK && m != 0xD9; m = dec.next_marker()) {
        if (m == 0xDA || m == 0xDC) rc = OADG_EUNSUPPORTED;
        else if (m < 0 || Decoder::stray_marker(m)) rc = OADG_EFORMAT;
        else {
            const uint8_t* s;
            long len;
            rc = dec.segment(&s, &len);
        }
    }
    const Huff* dct[3];
    const Huff* act[3];
    for (int i = 0; i < nc; ++i) { dct[i] = &dec.dc[dec.comp[i].td]; act[i] = &dec.ac[dec.comp[i].ta]; }
    long mcu = 0;
    for (long s = 0; s <= nseg && rc == OADG_OK; ++s) {
        Bits bits(ent + seg[s], ent + seg[s + 1]);
        int pred[3] = {0, 0, 0};
        const long last = dec.restart ? (mcu + dec.restart < mcus ? mcu + dec.restart : mcus) : mcus;
        for (; mcu < last && rc == OADG_OK; ++mcu) {
            const long my = mcu / mcux, mx = mcu % mcux;
            for (int i = 0; i < nc && rc == OADG_OK; ++i) {
                for (int by = 0; by < vs[i] && rc == OADG_OK; ++by)
                    for (int bx = 0; bx < hs[i] && rc == OADG_OK; ++bx) {
                        const long row = my * vs[i] + by, col = mx * hs[i] + bx;
                        int16_t* blk = coef + d->off[i] + (row * d->bw[i] + col) * 64;
                        long mag;
                        rc = decode_block(bits, *dct[i], *act[i], pred[i], blk, d->qt[i], mag);
                        if (rc == OADG_OK && mag > kPlainSum && !idct_forms_agree(blk, d->qt[i])) rc = OADG_EUNSUPPORTED;
                    }
            }
            if (rc == OADG_OK && bits.over > 64) rc = OADG_EFORMAT;     // far past the data
        }
        if (rc == OADG_OK && bits.overrun()) rc = OADG_EFORMAT;
    }
    free(ent);
    free(seg);
    if (rc) return rc;
    d->height = H;
    d->width = W;
    d->hmax = hmax;
    d->vmax = vmax;
    d->mcux = mcux;
    d->mcuy = mcuy;
    d->ncomp = nc;          // last: a descriptor with ncomp 0 is skipped by the device stage
    return OADG_OK;
}

}  // namespace

extern "C" int oadg_jpeg_size(const char* path, int* height, int* width) {
    if (!path || !height || !width) return OADG_EARG;
    uint8_t* file;
    long size;
    int rc = read_file(path, &file, &size);
    if (rc) return rc;
    Decoder dec(file, size);
    const uint8_t* sos;
    long sos_len;
    rc = dec.headers(true, &sos, &sos_len);
    free(file);
    if (dec.W > 0 && dec.H > 0 && (rc == OADG_OK || rc == OADG_EUNSUPPORTED)) {
        *height = dec.H;
        *width = dec.W;
        return OADG_OK;
    }
    return rc ? rc : OADG_EFORMAT;
}

extern "C" size_t oadg_jpeg_coef_capacity(int H, int W) {
    if (H < 1 || W < 1) return 0;
    return (size_t)3 * (size_t)((H + 15) / 16 * 16) * (size_t)((W + 15) / 16 * 16);
}

extern "C" int oadg_jpeg_entropy_decode(const char* path, int H, int W, int16_t* coef_host, size_t capacity,
                                        oadg_jpeg_desc* desc_host) {
    if (desc_host) desc_host->ncomp = 0;
    if (!path || !coef_host || !desc_host || H < 1 || W < 1) return OADG_EARG;
    uint8_t* file;
    long size;
    int rc = read_file(path, &file, &size);
    if (rc) return rc;
    rc = entropy_decode(file, size, H, W, coef_host, capacity, desc_host);
    free(file);
    if (rc) desc_host->ncomp = 0;
    return rc;
}

extern "C" int oadg_jpeg_pixels_bgr(const int16_t* coef, const oadg_jpeg_desc* desc, int n, long long slot,
                                    uint8_t* planes, uint8_t* out, int H, int W, void* stream) {
    if (!coef || !desc || !planes || !out || n < 1 || H < 1 || W < 1 || slot < 64 || (slot & 63)) return OADG_EARG;
    if ((size_t)slot < oadg_jpeg_coef_capacity(H, W)) return OADG_ESIZE;
    hipStream_t s = (hipStream_t)stream;
    const long blocks = slot / 64;
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)oadg_cdiv(blocks, 256), (unsigned)n), dim3(256), 0, s, coef, desc,
                       slot, planes);
    OADG_LAUNCH_CHECK();
    const long threads = (long)n * H * ((W + 3) / 4);
    const int aligned = (W % 4 == 0) && ((uintptr_t)out % 4 == 0);
    hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)oadg_cdiv(threads, 256)), dim3(256), 0, s, desc, slot,
                       (const uint8_t*)planes, out, n, H, W, aligned);
    OADG_LAUNCH_CHECK();
    return OADG_OK;
}

extern "C" int oadg_jpeg_decode_bgr(const char* path, uint8_t* out, int H, int W) {
    if (!path || !out || H < 1 || W < 1) return OADG_EARG;
    const size_t cap = oadg_jpeg_coef_capacity(H, W);
    int16_t* coef = (int16_t*)malloc(cap * sizeof(int16_t));
    uint8_t* planes = (uint8_t*)malloc(cap);
    oadg_jpeg_desc d;
    int rc = (coef && planes) ? oadg_jpeg_entropy_decode(path, H, W, coef, cap, &d) : OADG_EIO;
    if (rc == OADG_OK) {
        int in[64];
        uint8_t px[64];
        for (int c = 0; c < d.ncomp; ++c) {
            const long nb = (long)d.bw[c] * d.bh[c];
            for (long b = 0; b < nb; ++b) {
                const int16_t* src = coef + d.off[c] + b * 64;
                for (int k = 0; k < 64; ++k) in[k] = (int)src[k] * (int)d.qt[c][k];
                idct_islow(in, px);
                const long bx = b % d.bw[c], by = b / d.bw[c];
                for (int r = 0; r < 8; ++r)
                    memcpy(planes + d.off[c] + (by * 8 + r) * (d.bw[c] * 8) + bx * 8, px + r * 8, 8);
            }
        }
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) pixel_bgr(d, planes, x, y, out + ((long)y * W + x) * 3);
    }
    free(coef);
    free(planes);
    return rc;
}
