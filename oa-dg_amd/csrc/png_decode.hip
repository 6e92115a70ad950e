// PNG file -> BGR uint8 [H][W][3] straight into the caller's (pinned) buffer, on the HOST, without the interpreter lock.
//
// Replaces, for the input path of tools/train.py on real files:
//   mmdet/datasets/pipelines/loading.py:33-78  LoadImageFromFile (mmcv.imfrombytes -> cv2.imdecode, colour, BGR)
// A 1024 x 2048 Cityscapes-sized PNG is 30 - 80 ms of inflate + unfilter on one core and a training step consumes four of
// them every ~27 ms: the decode has to run on a dozen threads at once.  PIL decodes in 64 KB pieces and takes the
// interpreter lock back between them (and the caller then copies the image twice: np.asarray + the channel flip); here one
// ctypes call (lock released for its whole duration) inflates the IDAT stream with zlib, undoes the five PNG row filters
// and writes the pixels in OpenCV's channel order at their final place.  PNG is lossless: the bytes equal cv2's / PIL's.
// Covers what such datasets hold: 8-bit grey / RGB / RGBA, non-interlaced (oadg_png_decode_gray16: the 16-bit grey instance
// maps of Cityscapes' gtFine, for tools/dataset_converters/cityscapes.py); anything else returns OADG_EUNSUPPORTED and the
// caller falls back to PIL.  Host code only (compiled by hipcc with the rest of the library, links zlib).
// The rule for untrusted bytes is jpeg_decode.hip's: OADG_OK only for a file PIL loads, with PIL's bytes.  Pinned by
// tests/test_decoder_robustness.py with the writer of tests/jpeg_cases.py (PIL's own encoder never picks Average):
//   decoded: each of the five filters on every row and on the first row alone at 1, 2 (16-bit grey), 3 and 4 bytes per
//     pixel, extents down to 1 x 1; IDAT split after every byte, empty IDAT chunks, ancillary chunks (tEXt, gAMA, tRNS)
//     before the data, scanline data beyond the last row (ignored, as by PIL)
//   declined (OADG_EUNSUPPORTED): interlaced, palette, depth 1 / 2 / 4, 16-bit RGB, grey with alpha, a filter byte above
//     4, a chunk between two IDAT chunks (PIL reports such a file truncated), and every malformed file: a chunk length
//     past the end, data short of the image, IHDR not first, a damaged signature, fewer than 57 bytes, a zlib stream of
//     garbage.  Chunk CRCs are not checked.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>
#include "common.h"
#include "oadg_hip.h"

namespace {

inline unsigned be32(const unsigned char* p) { return ((unsigned)p[0] << 24) | ((unsigned)p[1] << 16) | ((unsigned)p[2] << 8) | p[3]; }

inline int paeth(int a, int b, int c) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// one scanline in place: cur = filtered bytes (n), prev = the reconstructed line above (or zeros)
void unfilter(int type, unsigned char* cur, const unsigned char* prev, long n, int bpp) {
    switch (type) {
        case 0: break;
        case 1: for (long i = bpp; i < n; ++i) cur[i] = (unsigned char)(cur[i] + cur[i - bpp]); break;
        case 2: for (long i = 0; i < n; ++i) cur[i] = (unsigned char)(cur[i] + prev[i]); break;
        case 3:
            for (long i = 0; i < bpp; ++i) cur[i] = (unsigned char)(cur[i] + (prev[i] >> 1));
            for (long i = bpp; i < n; ++i) cur[i] = (unsigned char)(cur[i] + ((cur[i - bpp] + prev[i]) >> 1));
            break;
        default:
            for (long i = 0; i < bpp; ++i) cur[i] = (unsigned char)(cur[i] + prev[i]);
            for (long i = bpp; i < n; ++i) cur[i] = (unsigned char)(cur[i] + paeth(cur[i - bpp], prev[i], prev[i - bpp]));
    }
}

}  // namespace

extern "C" int oadg_png_size(const char* path, int* height, int* width) {
    if (!path || !height || !width) return OADG_EARG;
    FILE* f = fopen(path, "rb");
    if (!f) return OADG_EIO;
    unsigned char h[33];
    const size_t got = fread(h, 1, 33, f);
    fclose(f);
    static const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    if (got < 33 || memcmp(h, sig, 8) != 0 || memcmp(h + 12, "IHDR", 4) != 0) return OADG_EUNSUPPORTED;
    *width = (int)be32(h + 16);
    *height = (int)be32(h + 20);
    return OADG_OK;
}

namespace {

// The whole file -> the inflated, still filtered scanlines of an H x W image: *raw holds h * (*line + 1) bytes (the caller
// frees it), *bytes_pp the bytes per pixel.  `gray16`: accept grey of depth 8 or 16 only (else: 8-bit grey / RGB / RGBA).
int inflate_file(const char* path, int H, int W, bool gray16, unsigned char** raw_out, long* line_out, int* bytes_pp) {
    FILE* f = fopen(path, "rb");
    if (!f) return OADG_EIO;
    fseek(f, 0, SEEK_END);
    const long size = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (size < 57) { fclose(f); return size < 0 ? OADG_EIO : OADG_EUNSUPPORTED; }
    unsigned char* file = (unsigned char*)malloc((size_t)size);
    if (!file) { fclose(f); return OADG_EIO; }
    const size_t got = fread(file, 1, (size_t)size, f);
    fclose(f);
    int rc = OADG_EUNSUPPORTED;
    unsigned char* raw = nullptr;
    static const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    do {
        if ((long)got != size || memcmp(file, sig, 8) != 0 || memcmp(file + 12, "IHDR", 4) != 0) break;
        const long w = be32(file + 16), h = be32(file + 20);
        const int depth = file[24], ctype = file[25], interlace = file[28];
        if (w != W || h != H) { rc = OADG_ESIZE; break; }
        if (interlace != 0) break;
        int bpp;
        if (gray16) {
            if (ctype != 0 || !(depth == 8 || depth == 16)) break;
            bpp = depth / 8;
        } else {
            if (depth != 8 || !(ctype == 0 || ctype == 2 || ctype == 6)) break;
            bpp = ctype == 0 ? 1 : (ctype == 2 ? 3 : 4);
        }
        const long line = w * bpp, need = h * (line + 1);
        if (need > 0x7fffffffL) break;                     // (zlib's avail_out is 32 bits wide)
        raw = (unsigned char*)malloc((size_t)need);
        if (!raw) { rc = OADG_EIO; break; }
        z_stream zs;
        memset(&zs, 0, sizeof(zs));
        if (inflateInit(&zs) != Z_OK) { rc = OADG_EIO; break; }
        zs.next_out = raw;
        zs.avail_out = (uInt)need;
        long pos = 8;
        int zrc = Z_OK;
        bool end = false, idat_seen = false, idat_closed = false, idat_apart = false;
        while (pos + 12 <= size && !end) {
            const unsigned len = be32(file + pos);
            const unsigned char* type = file + pos + 4;
            if (pos + 12 + (long)len > size) break;
            if (memcmp(type, "IDAT", 4) == 0) {
                // the IDAT chunks must follow one another: PIL stops at a chunk between them and reports a truncated file
                if (idat_closed) { idat_apart = true; break; }
                idat_seen = true;
                if (len && zrc == Z_OK) {                  // (an empty IDAT is legal; inflate would answer Z_BUF_ERROR)
                    zs.next_in = file + pos + 8;
                    zs.avail_in = len;
                    zrc = inflate(&zs, Z_NO_FLUSH);
                }
            } else {
                if (idat_seen) idat_closed = true;
                if (memcmp(type, "IEND", 4) == 0) end = true;
            }
            pos += 12 + (long)len;
        }
        const bool complete = !idat_apart && (zrc == Z_STREAM_END || zrc == Z_OK) && zs.total_out == (uLong)need;
        inflateEnd(&zs);
        if (!complete) break;
        *raw_out = raw;
        *line_out = line;
        *bytes_pp = bpp;
        raw = nullptr;
        rc = OADG_OK;
    } while (false);
    free(raw);
    free(file);
    return rc;
}

}  // namespace

extern "C" int oadg_png_decode_bgr(const char* path, uint8_t* out, int H, int W) {
    if (!path || !out || H < 1 || W < 1) return OADG_EARG;
    unsigned char* raw = nullptr;
    long line = 0;
    int bpp = 0;
    int rc = inflate_file(path, H, W, false, &raw, &line, &bpp);
    if (rc != OADG_OK) return rc;
    rc = OADG_EUNSUPPORTED;
    // unfilter in place (a zero line above the first), then the pixels in B, G, R order
    unsigned char* zero = (unsigned char*)calloc((size_t)line, 1);
    if (!zero) { free(raw); return OADG_EIO; }
    const unsigned char* prev = zero;
    bool ok = true;
    for (long y = 0; y < H && ok; ++y) {
        unsigned char* cur = raw + y * (line + 1) + 1;
        const int ft = cur[-1];
        if (ft > 4) { ok = false; break; }
        unfilter(ft, cur, prev, line, bpp);
        uint8_t* o = out + (size_t)y * W * 3;
        if (bpp == 1) for (long x = 0; x < W; ++x) { o[3 * x] = o[3 * x + 1] = o[3 * x + 2] = cur[x]; }
        else for (long x = 0; x < W; ++x) { o[3 * x] = cur[bpp * x + 2]; o[3 * x + 1] = cur[bpp * x + 1]; o[3 * x + 2] = cur[bpp * x]; }
        prev = cur;
    }
    free(zero);
    if (ok) rc = OADG_OK;
    free(raw);
    return rc;
}

// 16-bit greyscale (Cityscapes *_gtFine_instanceIds.png): the same inflate and row filters (the filters work on BYTES, two to
// a pixel), then the big-endian samples as native uint16 [H][W]; 8-bit grey is widened.
extern "C" int oadg_png_decode_gray16(const char* path, uint16_t* out, int H, int W) {
    if (!path || !out || H < 1 || W < 1) return OADG_EARG;
    unsigned char* raw = nullptr;
    long line = 0;
    int bpp = 0;
    int rc = inflate_file(path, H, W, true, &raw, &line, &bpp);
    if (rc != OADG_OK) return rc;
    unsigned char* zero = (unsigned char*)calloc((size_t)line, 1);
    if (!zero) { free(raw); return OADG_EIO; }
    const unsigned char* prev = zero;
    rc = OADG_OK;
    for (long y = 0; y < H; ++y) {
        unsigned char* cur = raw + y * (line + 1) + 1;
        const int ft = cur[-1];
        if (ft > 4) { rc = OADG_EUNSUPPORTED; break; }
        unfilter(ft, cur, prev, line, bpp);
        uint16_t* o = out + (size_t)y * W;
        if (bpp == 1) for (long x = 0; x < W; ++x) o[x] = cur[x];
        else for (long x = 0; x < W; ++x) o[x] = (uint16_t)((cur[2 * x] << 8) | cur[2 * x + 1]);
        prev = cur;
    }
    free(zero);
    free(raw);
    return rc;
}
