// Display-list rasteriser: boxes, filled rectangles and bitmap text painted in place on a resident uint8 [n][H][W][3]
// batch (the loader's layout; the three bytes of a colour are written as given).
//   replaces imshow_det_bboxes  mmdet/core/visualization/image.py (matplotlib on the host) for BaseDetector.show_result and
//            tools/test.py --show-dir; the pixel semantics are Pillow's ImageDraw.rectangle(outline=, width=),
//            rectangle(fill=) and text() with the built-in 6 x 11 bitmap font (font6x11.h, tools/make_font6x11.py).
// A gather, not a scatter: one workgroup per 64 x 16 image tile culls the image's items against the tile into an LDS list
// (in order; the list is walked and emptied whenever the next 256 items might not fit), then every thread walks the list
// back to front for its 4 horizontally adjacent pixels and keeps the first hit of each - the LAST item that covers the
// pixel, painter's order.  A later list overrides an earlier one.  Only painted pixels are stored, nothing is ever read
// from the image, and a tile no item touches costs one pass over the item rows.
// Addresses are formed from the tile's own in-image coordinates only; item coordinates are compared (in 64 bits: any int32
// is a legal coordinate, width or scale) and never index anything.  Text bytes are read at offset + c with
// 0 <= offset, c < length and offset + length <= text_bytes, checked here per item.
#include "common.h"
#include "../../include/oadg_hip.h"
#define OADG_FONT_QUALIFIER __device__ const
#include "font6x11.h"

namespace {

constexpr int TILE_W = 64, TILE_H = 16, PX = 4, THREADS = 256;    // 16 x 16 threads, 4 pixels each
constexpr int CAP = OADG_DRAW_TILE_CAPACITY;
constexpr int ROW = OADG_DRAW_ITEM_INTS;
static_assert(CAP == THREADS, "one source item per thread and pass: a pass must always fit an empty list");
static_assert(TILE_W == 16 * PX && TILE_H * 16 == THREADS, "thread layout");

typedef long long i64;

// a / b for 0 <= a, 0 < b: 32-bit when both fit (every sane display list)
__device__ __forceinline__ i64 div_pos(i64 a, i64 b) {
    return ((a | b) >> 31) == 0 ? (i64)((unsigned)a / (unsigned)b) : a / b;
}

// does item `it` paint anything inside the tile [tx0, tx1] x [ty0, ty1] (inclusive, inside the image)?
__device__ __forceinline__ bool touches(const int* it, int tx0, int ty0, int tx1, int ty1, i64 text_bytes) {
    const int kind = it[0];
    if (kind == OADG_DRAW_OUTLINE || kind == OADG_DRAW_FILL) {
        const i64 x0 = it[1], y0 = it[2], x1 = it[3], y1 = it[4];
        if (x1 < x0 || y1 < y0 || x1 < tx0 || x0 > tx1 || y1 < ty0 || y0 > ty1) return false;
        if (kind == OADG_DRAW_FILL) return true;
        const i64 w = it[5];
        if (w <= 0) return false;
        // the tile lies wholly in the hollow of the box
        return !(tx0 - x0 >= w && x1 - tx1 >= w && ty0 - y0 >= w && y1 - ty1 >= w);
    }
    if (kind == OADG_DRAW_TEXT) {
        const i64 x = it[1], y = it[2], off = it[3], len = it[4], s = it[5];
        if (s < 1 || len < 1 || off < 0 || off + len > text_bytes) return false;
        if (x > tx1 || y > ty1 || y + OADG_FONT_H * s - 1 < ty0) return false;
        return tx0 <= x || div_pos(tx0 - x, OADG_FONT_W * s) < len;
    }
    return false;
}

// the culled list [0, cnt), back to front, for the pixels (px0 .. px0 + nv - 1, py); a hit overrides *mask / col
__device__ __forceinline__ void walk(const int (*list)[ROW], int cnt, int px0, int py, int nv, const unsigned char* text,
                                     unsigned* mask, unsigned* col) {
    const unsigned want = (1u << nv) - 1u;
    unsigned m = 0, c[PX] = {0, 0, 0, 0};
    for (int j = cnt - 1; j >= 0 && m != want; --j) {
        const int* it = list[j];
        const int kind = it[0];
        const unsigned colour = (unsigned)it[6];
        if (kind == OADG_DRAW_TEXT) {
            const i64 s = it[5], dy = (i64)py - it[2];
            if (dy < 0 || dy >= OADG_FONT_H * s) continue;
            const int row = (int)div_pos(dy, s);
            const i64 len = it[4], cell = OADG_FONT_W * s;
#pragma unroll
            for (int k = 0; k < PX; ++k) {
                if (k >= nv || ((m >> k) & 1u)) continue;
                const i64 dx = (i64)(px0 + k) - it[1];
                if (dx < 0) continue;
                const i64 ch = div_pos(dx, cell);
                if (ch >= len) continue;
                const int code = text[(i64)it[3] + ch];
                if (code < OADG_FONT_FIRST || code > OADG_FONT_LAST) continue;
                const int column = (int)div_pos(dx - ch * cell, s);
                if ((OADG_FONT6X11[code - OADG_FONT_FIRST][row] >> (OADG_FONT_W - 1 - column)) & 1) {
                    c[k] = colour;
                    m |= 1u << k;
                }
            }
        } else {   // OUTLINE or FILL (touches() lets nothing else into the list)
            const i64 x0 = it[1], y0 = it[2], x1 = it[3], y1 = it[4], w = it[5];
            if (py < y0 || py > y1) continue;
            const bool whole_row = kind == OADG_DRAW_FILL || (i64)py - y0 < w || y1 - (i64)py < w;
#pragma unroll
            for (int k = 0; k < PX; ++k) {
                const i64 x = px0 + k;
                if (k >= nv || ((m >> k) & 1u) || x < x0 || x > x1) continue;
                if (whole_row || x - x0 < w || x1 - x < w) {
                    c[k] = colour;
                    m |= 1u << k;
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < PX; ++k)
        if ((m >> k) & 1u) col[k] = c[k];
    *mask |= m;
}

__global__ __launch_bounds__(THREADS) void draw_items_kernel(unsigned char* __restrict__ imgs, int H, int W, int tiles_x,
                                                             int tiles_y, const int* __restrict__ items,
                                                             const int* __restrict__ item_off, int n_items,
                                                             const unsigned char* __restrict__ text, i64 text_bytes) {
    __shared__ int list[CAP][ROW];
    __shared__ int wave_hits[THREADS / OADG_WAVE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per_img = tiles_x * tiles_y;
    const int img = blockIdx.x / per_img, t = blockIdx.x - img * per_img;
    const int tx0 = (t % tiles_x) * TILE_W, ty0 = (t / tiles_x) * TILE_H;
    const int tx1 = min(tx0 + TILE_W, W) - 1, ty1 = min(ty0 + TILE_H, H) - 1;
    int begin = item_off[img], end = item_off[img + 1];
    begin = max(begin, 0);
    end = min(end, n_items);
    if (end <= begin) return;                                         // (uniform: the whole workgroup leaves)

    const int px0 = tx0 + (tid & 15) * PX, py = ty0 + (tid >> 4);
    const int nv = (py <= ty1 && px0 <= tx1) ? min(PX, tx1 + 1 - px0) : 0;
    unsigned mask = 0, col[PX] = {0, 0, 0, 0};
    int cnt = 0;
    for (int base = begin; base < end; base += THREADS) {
        const int i = base + tid;
        int row[ROW];
        bool hit = false;
        if (i < end) {
#pragma unroll
            for (int k = 0; k < ROW; ++k) row[k] = items[(i64)i * ROW + k];
            hit = touches(row, tx0, ty0, tx1, ty1, text_bytes);
        }
        const unsigned long long b = __ballot(hit);
        if (lane == 0) wave_hits[wave] = __popcll(b);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < THREADS / OADG_WAVE; ++k) {
            before += k < wave ? wave_hits[k] : 0;
            total += wave_hits[k];
        }
        if (cnt + total > CAP) {                                      // (uniform) walk what is listed, start over
            walk(list, cnt, px0, py, nv, text, &mask, col);
            cnt = 0;
            __syncthreads();
        }
        if (hit) {
            const int slot = cnt + before + __popcll(b & ((1ull << lane) - 1ull));
#pragma unroll
            for (int k = 0; k < ROW; ++k) list[slot][k] = row[k];
        }
        cnt += total;
        __syncthreads();
    }
    walk(list, cnt, px0, py, nv, text, &mask, col);
    if (!mask) return;

    unsigned char* p = imgs + (((i64)img * H + py) * W + px0) * 3;    // px0 <= tx1 < W, py <= ty1 < H here (nv > 0)
    if (mask == 0xfu && (((uintptr_t)p) & 3u) == 0) {                 // 4 painted pixels = 12 bytes = 3 aligned dwords
        const unsigned a = col[0] & 0xffffffu, bb = col[1] & 0xffffffu, cc = col[2] & 0xffffffu, d = col[3] & 0xffffffu;
        unsigned* q = (unsigned*)p;
        q[0] = a | (bb << 24);
        q[1] = (bb >> 8) | (cc << 16);
        q[2] = (cc >> 16) | (d << 8);
    } else {
#pragma unroll
        for (int k = 0; k < PX; ++k)
            if ((mask >> k) & 1u) {                                   // (bit k is only ever set for k < nv)
                p[3 * k + 0] = (unsigned char)(col[k]);
                p[3 * k + 1] = (unsigned char)(col[k] >> 8);
                p[3 * k + 2] = (unsigned char)(col[k] >> 16);
            }
    }
}

}  // namespace

extern "C" int oadg_draw_tile_capacity(void) { return CAP; }

extern "C" int oadg_draw_items_u8(uint8_t* imgs, int n, int H, int W, const int32_t* items, const int32_t* item_off,
                                  int n_items, const uint8_t* text, size_t text_bytes, void* stream) {
    if (n < 0 || H < 1 || W < 1 || n_items < 0 || !item_off || (n > 0 && !imgs) || (n_items > 0 && !items)) return OADG_EARG;
    if ((text_bytes > 0 && !text) || text_bytes > 0x7fffffffu) return OADG_EARG;
    const long tiles_x = oadg_cdiv(W, TILE_W), tiles_y = oadg_cdiv(H, TILE_H);
    if (tiles_x * tiles_y * (long)n > 0x7fffffffL) return OADG_ESIZE;
    if (n == 0 || n_items == 0) return OADG_OK;
    hipLaunchKernelGGL(draw_items_kernel, dim3((unsigned)(tiles_x * tiles_y * n)), dim3(THREADS), 0, (hipStream_t)stream,
                       imgs, H, W, (int)tiles_x, (int)tiles_y, items, item_off, n_items, text, (i64)text_bytes);
    OADG_LAUNCH_CHECK();
    return OADG_OK;
}
