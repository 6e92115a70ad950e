// A resident uint8 [n][H][W][3] batch -> the zlib stream of every image's PNG scanlines, and the stream -> a PNG file.
//
// Replaces, for tools/analysis_tools/get_corrupted_dataset.py:
//   tools/analysis_tools/get_corrupted_dataset.py:83-113  save_data: PIL.Image.fromarray(img).save(save_path) per image -
//   PNG row filtering and zlib deflate (LZ77 + Huffman, level 6) of 6 MB per 1024 x 2048 image on one host core.
// Here the filtered byte stream of an image ((3W+1) bytes per row: filter type, then the filtered R, G, B bytes) is cut
// into SEGMENTS of whole rows (pieces of a row when one row exceeds SEG bytes) and every segment becomes one deflate block
// of LITERALS ONLY that ends on a byte boundary (an empty stored block behind it, as a sync flush), so segments are encoded
// independently and concatenated by plain copies:
//   encode_kernel   one workgroup per segment: stages the raw rows it needs in LDS (16-byte loads; the ragged ends byte by
//                   byte), picks a filter per row (the minimum sum of absolute signed values over None / Sub / Up / Average /
//                   Paeth, or the forced type), filters into LDS with a 257-bin histogram (256 literals + end-of-block),
//                   builds Huffman code lengths limited to 15 bits and the canonical codes (one lane does the serial part),
//                   sums the code lengths of a short span per lane, scans them for bit offsets, ORs the bits into zeroed
//                   LDS words - or lays out a stored block when coding does not make the segment smaller - and writes the
//                   segment with its size and Adler-32 partial sums into its slot of the workspace;
//   scan_kernel     one workgroup per image: exclusive scan of the segment sizes, the Adler-32 of the whole filtered stream
//                   from the partial sums (they compose modulo 65521), the 2-byte header, the final empty block, the trailer;
//   gather_kernel   one workgroup per segment: slot -> its place in the image's contiguous stream.
// Work passes between workgroups across these three launches only; nothing waits inside a launch.  Integer arithmetic,
// atomicOr / atomicAdd on integers and an ordered write: the bytes do not depend on the order of arrival, on the run, or on
// what else is in the batch.  Every LDS index is below the extent derived from SEG next to it; every global index is checked
// against the segment, the slot or the caller's capacity before it is used.
//   oadg_png_write_rgb8 (HOST)  signature, IHDR, IDAT, IEND around a finished stream: PIL's file container.
#include <stdio.h>
#include <zlib.h>

#include "common.h"
#include "oadg_hip.h"

namespace {

constexpr int SEG = 18944;               // filtered bytes of a segment at most (a multiple of 16; 1024 x 2048: three rows)
constexpr int MAX_ROWS = 512;            // rows of a segment at most (narrow images)
constexpr int THREADS = 512;
constexpr int WAVES = THREADS / 64;
constexpr int NSYM = 257;                // 256 literals + end-of-block
constexpr int EOB = 256;
constexpr int MAXLEN = 15;               // deflate's longest code
constexpr int DEEP = 32;                 // unlimited depths are clamped here before the limiter (a segment's is below 24)
constexpr int HDR_BITS = 17 + 19 * 3 + 258 * 4;   // block type, HLIT, HDIST, HCLEN; 19 code-length lengths; 257 + 1 lengths
constexpr int HALF = SEG + 32;           // second staging region of a row piece
constexpr int RAW = 2 * SEG + 64;
constexpr int SCAN = 1024;
constexpr long MAX_W = 1L << 22;         // the per-row sums of the filter choice stay below 2^31

struct Geo {
    int w3, rb;        // raw and filtered bytes per row
    int R, P;          // rows per segment (P == 1), or pieces per row (R == 1)
    int slot;          // bytes of a segment's slot in the workspace (a multiple of 16)
    long nseg, L;      // segments and filtered bytes per image
};

bool geometry(int H, int W, Geo* g) {
    if (H < 1 || W < 1 || W > MAX_W) return false;
    const long rb = 3L * W + 1, L = rb * H;
    if (L >= (1L << 31)) return false;
    g->w3 = 3 * W;
    g->rb = (int)rb;
    g->L = L;
    if (rb <= SEG) {
        g->P = 1;
        g->R = (int)(SEG / rb < MAX_ROWS ? SEG / rb : MAX_ROWS);
        g->nseg = (H + g->R - 1) / g->R;
    } else {
        g->R = 1;
        g->P = (int)((rb + SEG - 1) / SEG);
        g->nseg = (long)H * g->P;
    }
    g->slot = SEG + 32;                  // a stored segment is 5 bytes longer than its data; written in 16-byte chunks
    return true;
}

// filtered bytes [f0, f0 + nbytes) of the image, rows y0 .. y1-1, starting at column c0 of row y0
__host__ __device__ __forceinline__ void segment_range(const Geo& g, int H, long s, int* y0, int* y1, int* c0, int* nbytes) {
    if (g.P == 1) {
        *y0 = (int)(s * g.R);
        *y1 = *y0 + g.R < H ? *y0 + g.R : H;
        *c0 = 0;
        *nbytes = (*y1 - *y0) * g.rb;
    } else {
        *y0 = (int)(s / g.P);
        *y1 = *y0 + 1;
        *c0 = (int)(s % g.P) * SEG;
        *nbytes = g.rb - *c0 < SEG ? g.rb - *c0 : SEG;
    }
}

struct Layout {
    size_t slots, size, off, adler_a, adler_b, total;
};

Layout layout(int n, const Geo& g) {
    Layout l;
    const size_t cells = (size_t)n * (size_t)g.nseg;
    l.slots = 0;                                                  // (16-byte units, then 8-byte, then 4-byte ones)
    l.off = l.slots + cells * (size_t)g.slot;
    l.size = l.off + cells * sizeof(long long);
    l.adler_a = l.size + cells * sizeof(int);
    l.adler_b = l.adler_a + cells * sizeof(unsigned);
    l.total = l.adler_b + cells * sizeof(unsigned);
    return l;
}

// image bytes [lo, hi) -> LDS at dst (16-byte aligned) so that byte lo lands at the returned index: whole 16-byte chunks at
// aligned addresses inside the range as vectors, the chunks at the two ends byte by byte
__device__ __forceinline__ int stage(const uint8_t* im, long lo, long hi, uint8_t* dst) {
    const uint8_t* p = im + lo;
    const int a = (int)((uintptr_t)p & 15);
    const uint8_t* base = p - a;
    const long len = hi - lo, nchunks = (a + len + 15) >> 4;
    for (long c = threadIdx.x; c < nchunks; c += THREADS) {
        const long b0 = 16 * c - a;
        if (b0 >= 0 && b0 + 16 <= len) {
            *reinterpret_cast<uint4*>(dst + 16 * c) = *reinterpret_cast<const uint4*>(base + 16 * c);
        } else {
            for (int j = 0; j < 16; ++j) {
                const long o = b0 + j;
                if (o >= 0 && o < len) dst[16 * c + j] = p[o];
            }
        }
    }
    return a;
}

// emitted byte k of a row (R, G, B order) -> its index in the stored row
__device__ __forceinline__ int ksrc(int k, int bgr) {
    if (!bgr) return k;
    const int p = k / 3;
    return 3 * p + 2 - (k - 3 * p);
}

// the byte and its left / upper / upper-left neighbours (PNG: zero outside the image)
__device__ __forceinline__ void neighbours(const uint8_t* cur, const uint8_t* prev, bool has_prev, int k, int bgr, int* x,
                                           int* a, int* b, int* c) {
    const int ks = ksrc(k, bgr);
    *x = cur[ks];
    *a = k >= 3 ? cur[ks - 3] : 0;
    *b = has_prev ? prev[ks] : 0;
    *c = has_prev && k >= 3 ? prev[ks - 3] : 0;
}

__device__ __forceinline__ int paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return pa <= pb && pa <= pc ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ int apply_filter(int t, int x, int a, int b, int c) {
    const int pred = t == 0 ? 0 : t == 1 ? a : t == 2 ? b : t == 3 ? (a + b) >> 1 : paeth(a, b, c);
    return (x - pred) & 255;
}

__device__ __forceinline__ int abs_signed(int v) { return v < 128 ? v : 256 - v; }

__device__ __forceinline__ void filter_sums(int x, int a, int b, int c, int* s) {
    s[0] += abs_signed(x);
    s[1] += abs_signed((x - a) & 255);
    s[2] += abs_signed((x - b) & 255);
    s[3] += abs_signed((x - ((a + b) >> 1)) & 255);
    s[4] += abs_signed((x - paeth(a, b, c)) & 255);
}

__device__ __forceinline__ int best_filter(const int* s) {
    int best = 0;
    for (int t = 1; t < 5; ++t)
        if (s[t] < s[best]) best = t;
    return best;
}

// exclusive scan of one value per thread over the workgroup; wsum: WAVES ints of LDS
__device__ __forceinline__ int block_exclusive(int v, int* wsum, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int base = 0, all = 0;
    for (int i = 0; i < WAVES; ++i) {
        if (i < wave) base += wsum[i];
        all += wsum[i];
    }
    *total = all;
    __syncthreads();
    return base + inc - v;
}

// Code lengths of a minimum-redundancy code from the counts A[0..n) in ascending order, in place (Moffat & Katajainen,
// "In-place calculation of minimum-redundancy codes", 1995): A[i] becomes the depth of leaf i.  n >= 2.
__device__ void huffman_depths(int* A, int n) {
    A[0] += A[1];
    int root = 0, leaf = 2;
    for (int next = 1; next < n - 1; ++next) {
        if (leaf >= n || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = next; }
        else A[next] = A[leaf++];
        if (leaf >= n || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = next; }
        else A[next] += A[leaf++];
    }
    A[n - 2] = 0;
    for (int next = n - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
    int avail = 1, used = 0, depth = 0, next = n - 1;
    root = n - 2;
    while (avail > 0) {
        while (root >= 0 && A[root] == depth) { ++used; --root; }
        while (avail > used) { A[next--] = depth; --avail; }
        avail = 2 * used;
        ++depth;
        used = 0;
    }
}

// ncodes[l] = leaves at depth l (l <= DEEP) -> the same number of leaves, none deeper than MAXLEN, Kraft sum exactly 1:
// everything deeper moves to MAXLEN (the sum is then too large by a whole number of 2^-MAXLEN), and each step takes one
// leaf off MAXLEN and pairs it with the deepest leaf above MAXLEN, one level further down (the sum drops by 2^-MAXLEN)
__device__ void limit_lengths(int* ncodes) {
    for (int l = MAXLEN + 1; l <= DEEP; ++l) {
        ncodes[MAXLEN] += ncodes[l];
        ncodes[l] = 0;
    }
    unsigned total = 0;
    for (int l = MAXLEN; l > 0; --l) total += (unsigned)ncodes[l] << (MAXLEN - l);
    while (total > (1u << MAXLEN)) {
        --ncodes[MAXLEN];
        for (int l = MAXLEN - 1; l > 0; --l) {
            if (ncodes[l]) {
                --ncodes[l];
                ncodes[l + 1] += 2;
                break;
            }
        }
        --total;
    }
}

__device__ __forceinline__ void put_bits(unsigned* w, int pos, unsigned value, int nbits) {
    const int word = pos >> 5, sh = pos & 31;
    atomicOr(&w[word], value << sh);
    if (sh + nbits > 32) atomicOr(&w[word + 1], value >> (32 - sh));
}

// grid (segments, n)
__global__ __launch_bounds__(THREADS) void encode_kernel(const uint8_t* __restrict__ imgs, int H, Geo g, int bgr, int mode,
                                                         uint8_t* __restrict__ slots, int* __restrict__ segsize,
                                                         unsigned* __restrict__ seg_a, unsigned* __restrict__ seg_b) {
    __shared__ __attribute__((aligned(16))) uint8_t raw[RAW];    // the raw rows; later the segment as it is written
    __shared__ __attribute__((aligned(16))) uint8_t filt[SEG];
    __shared__ unsigned hist[NSYM + 3];
    __shared__ int A[NSYM + 3];
    __shared__ unsigned short S[NSYM + 3], codes[NSYM + 3];
    __shared__ uint8_t lens[NSYM + 3], ftype[MAX_ROWS];
    __shared__ int ncodes[DEEP + 2], nextc[MAXLEN + 1], wsum[WAVES], misc[8];   // misc: 0..4 row sums, 5 used, 6 / 7 Adler
    const int tid = threadIdx.x & (THREADS - 1), lane = tid & 63, wave = tid >> 6;
    const long s = blockIdx.x;
    const uint8_t* im = imgs + (size_t)blockIdx.y * (size_t)H * g.w3;
    int y0, y1, c0, nbytes;
    segment_range(g, H, s, &y0, &y1, &c0, &nbytes);
    const int nrows = y1 - y0;                                    // <= MAX_ROWS
    for (int t = tid; t < NSYM + 3; t += THREADS) {
        hist[t] = t == EOB ? 1u : 0u;
        lens[t] = 0;
    }
    if (tid < 8) misc[tid] = 0;

    // ---- the raw bytes this segment reads: index = cur_off(row) + k, the row above at prev_off + k
    int cur0, prev0;                                              // offsets of row y0 (whole rows: row y at + (y - y0) * w3)
    if (g.P == 1) {
        const int ylo = y0 > 0 ? y0 - 1 : 0;
        const int a = stage(im, (long)ylo * g.w3, (long)y1 * g.w3, raw);      // (R + 1) * w3 + 15 < RAW
        cur0 = a + (y0 - ylo) * g.w3;
        prev0 = cur0 - g.w3;
    } else {
        int klo = c0 - 4 > 0 ? c0 - 4 : 0;
        klo = klo / 3 * 3;
        int khi = (c0 + nbytes - 1 + 2) / 3 * 3;
        khi = khi < g.w3 ? khi : g.w3;                            // khi - klo <= SEG + 8: + 15 of alignment < HALF
        cur0 = HALF + stage(im, (long)y0 * g.w3 + klo, (long)y0 * g.w3 + khi, raw + HALF) - klo;
        prev0 = y0 > 0 ? stage(im, (long)(y0 - 1) * g.w3 + klo, (long)(y0 - 1) * g.w3 + khi, raw) - klo : 0;
    }
    __syncthreads();

    // ---- one filter type per row
    if (mode >= 0) {
        for (int r = tid; r < nrows; r += THREADS) ftype[r] = (uint8_t)mode;
    } else if (g.P == 1) {
        for (int rl = wave; rl < nrows; rl += WAVES) {
            const uint8_t* cur = raw + cur0 + rl * g.w3;
            int sums[5] = {0, 0, 0, 0, 0};
            for (int k = lane; k < g.w3; k += 64) {
                int x, a, b, c;
                neighbours(cur, cur - g.w3, y0 + rl > 0, k, bgr, &x, &a, &b, &c);
                filter_sums(x, a, b, c, sums);
            }
#pragma unroll
            for (int t = 0; t < 5; ++t) sums[t] = wave_sum_i(sums[t]);
            if (lane == 0) ftype[rl] = (uint8_t)best_filter(sums);
        }
    } else {                                                      // a piece: the choice needs the whole row, from memory
        const uint8_t* cur = im + (size_t)y0 * g.w3;
        int sums[5] = {0, 0, 0, 0, 0};
        for (int k = tid; k < g.w3; k += THREADS) {
            int x, a, b, c;
            neighbours(cur, cur - g.w3, y0 > 0, k, bgr, &x, &a, &b, &c);
            filter_sums(x, a, b, c, sums);
        }
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            sums[t] = wave_sum_i(sums[t]);
            if (lane == 0) atomicAdd(&misc[t], sums[t]);
        }
        __syncthreads();
        if (tid == 0) ftype[0] = (uint8_t)best_filter(misc);
    }
    __syncthreads();

    // ---- filter into LDS: histogram and Adler-32 partial sums (a = sum d_i, b = sum (nbytes - i) d_i)
    {
        unsigned sa = 0, sb = 0;                                  // per thread: at most 37 bytes, b < 2^28
        for (int i = tid; i < nbytes; i += THREADS) {
            int rl = 0, col = c0 + i;
            if (g.P == 1) {
                rl = i / g.rb;
                col = i - rl * g.rb;
            }
            const int t = ftype[rl];
            int v = t;
            if (col > 0) {
                const uint8_t* cur = raw + cur0 + rl * g.w3;
                const uint8_t* prev = g.P == 1 ? cur - g.w3 : raw + prev0;
                int x, a, b, c;
                neighbours(cur, prev, y0 + rl > 0, col - 1, bgr, &x, &a, &b, &c);
                v = apply_filter(t, x, a, b, c);
            }
            filt[i] = (uint8_t)v;
            atomicAdd(&hist[v], 1u);
            sa += (unsigned)v;
            sb += (unsigned)(nbytes - i) * (unsigned)v;
        }
        const int ra = wave_sum_i((int)(sa % 65521u)), rb = wave_sum_i((int)(sb % 65521u));
        if (lane == 0) {
            atomicAdd(&misc[6], ra);
            atomicAdd(&misc[7], rb);
        }
    }
    __syncthreads();

    // ---- code lengths: the used symbols in ascending (count, symbol) order by rank, then the serial part on one lane
    if (tid < NSYM) {
        const unsigned c = hist[tid];
        if (c > 0) {
            int rank = 0;
            for (int j = 0; j < NSYM; ++j) {
                const unsigned o = hist[j];
                rank += (o > 0 && (o < c || (o == c && j < tid))) ? 1 : 0;
            }
            A[rank] = (int)c;
            S[rank] = (unsigned short)tid;
            atomicAdd(&misc[5], 1);
        }
    }
    __syncthreads();
    if (tid == 0) {
        const int n = misc[5];                                    // >= 2: a literal and end-of-block
        huffman_depths(A, n);
        for (int l = 0; l <= DEEP + 1; ++l) ncodes[l] = 0;
        for (int i = 0; i < n; ++i) ++ncodes[A[i] < DEEP ? A[i] : DEEP];
        limit_lengths(ncodes);
        int i = 0;                                                // the rarest symbols take the longest codes
        for (int l = MAXLEN; l > 0; --l)
            for (int c = 0; c < ncodes[l] && i < n; ++c) lens[S[i++]] = (uint8_t)l;
        int code = 0;
        nextc[0] = 0;
        for (int l = 1; l <= MAXLEN; ++l) {
            code = (code + ncodes[l - 1]) << 1;
            nextc[l] = code;
        }
    }
    __syncthreads();
    if (tid < NSYM) {
        const int l = lens[tid];
        unsigned code = 0;
        if (l > 0) {
            int before = 0;
            for (int j = 0; j < tid; ++j) before += lens[j] == l ? 1 : 0;
            code = __brev((unsigned)(nextc[l] + before)) >> (32 - l);      // Huffman codes go out most significant bit first
        }
        codes[tid] = (unsigned short)code;
    }
    __syncthreads();

    // ---- bit offsets: every lane owns a span of consecutive bytes
    const int span = (nbytes + THREADS - 1) / THREADS;
    const int b0 = tid * span < nbytes ? tid * span : nbytes, b1 = b0 + span < nbytes ? b0 + span : nbytes;
    int mybits = 0;
    for (int i = b0; i < b1; ++i) mybits += lens[filt[i]];
    int databits;
    const int start = block_exclusive(mybits, wsum, &databits);
    const int eob_at = HDR_BITS + databits;
    const int sync_at = (eob_at + lens[EOB] + 3 + 7) >> 3;        // the byte behind the empty stored block's 3 header bits
    const int coded = sync_at + 4, stored = nbytes + 5;
    const int size = coded < stored ? coded : stored;             // <= SEG + 5
    unsigned* w = reinterpret_cast<unsigned*>(raw);
    if (coded < stored) {
        for (int i = tid; i < (coded + 3) / 4 + 1; i += THREADS) w[i] = 0u;       // (coded + 8 <= SEG + 12 < RAW)
        __syncthreads();
        // dynamic block, not final; 257 literal/length codes, 1 distance code, all 19 code-length lengths
        if (tid == 0) put_bits(w, 0, 4u | (15u << 13), 17);
        if (tid < 19) put_bits(w, 17 + 3 * tid, tid < 3 ? 0u : 4u, 3);     // 16 / 17 / 18 unused; 0 .. 15: four bits each
        if (tid < 258) {
            const unsigned l = tid < NSYM ? lens[tid] : 1u;                 // (the one distance code: length 1, never used)
            put_bits(w, 17 + 57 + 4 * tid, __brev(l) >> 28, 4);
        }
        unsigned long long acc = 0;
        int pos = HDR_BITS + start, word = pos >> 5, nb = pos & 31;
        for (int i = b0; i < b1; ++i) {
            const int v = filt[i];
            acc |= (unsigned long long)codes[v] << nb;
            nb += lens[v];
            if (nb >= 32) {
                atomicOr(&w[word++], (unsigned)acc);
                acc >>= 32;
                nb -= 32;
            }
        }
        if (nb > 0 && (unsigned)acc != 0u) atomicOr(&w[word], (unsigned)acc);
        if (tid == 0) {
            put_bits(w, eob_at, codes[EOB], lens[EOB]);
            put_bits(w, (sync_at + 2) * 8, 0xffffu, 16);          // stored, length 0: 00 00 ff ff
        }
    } else {
        __syncthreads();
        if (tid == 0) {
            raw[0] = 0;                                           // stored, not final
            raw[1] = (uint8_t)(nbytes & 255);
            raw[2] = (uint8_t)(nbytes >> 8);
            raw[3] = (uint8_t)(~nbytes & 255);
            raw[4] = (uint8_t)((~nbytes >> 8) & 255);
        }
        for (int i = tid; i < nbytes; i += THREADS) raw[5 + i] = filt[i];
    }
    __syncthreads();
    const size_t cell = (size_t)blockIdx.y * (size_t)g.nseg + (size_t)s;
    uint4* out = reinterpret_cast<uint4*>(slots + cell * (size_t)g.slot);
    for (int c = tid; c < (size + 15) / 16; c += THREADS) out[c] = reinterpret_cast<const uint4*>(raw)[c];   // <= slot
    if (tid == 0) {
        segsize[cell] = size;
        seg_a[cell] = (unsigned)misc[6] % 65521u;
        seg_b[cell] = (unsigned)misc[7] % 65521u;
    }
}

__device__ __forceinline__ void put_byte(uint8_t* stream, size_t capacity, long long at, unsigned v) {
    if (at >= 0 && (unsigned long long)at < capacity) stream[at] = (uint8_t)v;
}

// grid (n), SCAN threads: off[image][s] = 2 + the sizes of the segments before s; the header, the final block, the trailer
__global__ __launch_bounds__(SCAN) void scan_kernel(const int* __restrict__ segsize, const unsigned* __restrict__ seg_a,
                                                    const unsigned* __restrict__ seg_b, long long* __restrict__ off, int H,
                                                    Geo g, uint8_t* __restrict__ streams, size_t capacity,
                                                    int64_t* __restrict__ stream_bytes) {
    __shared__ long long buf[2 * SCAN];
    const size_t first = (size_t)blockIdx.x * (size_t)g.nseg;
    const int tid = threadIdx.x & (SCAN - 1);
    long long carry = 2;
    for (long base = 0; base < g.nseg; base += SCAN) {
        const long i = base + tid;
        const long long v = i < g.nseg ? segsize[first + i] : 0;
        int src = 0;
        buf[tid] = v;
        __syncthreads();
        for (int o = 1; o < SCAN; o <<= 1) {
            long long t = buf[src * SCAN + tid];
            if (tid >= o) t += buf[src * SCAN + tid - o];
            buf[(src ^ 1) * SCAN + tid] = t;
            __syncthreads();
            src ^= 1;
        }
        if (i < g.nseg) off[first + i] = carry + buf[src * SCAN + tid] - v;
        carry += buf[src * SCAN + SCAN - 1];
        __syncthreads();
    }
    if (tid == 0) {
        unsigned long long a = 1, b = 0;
        for (long s = 0; s < g.nseg; ++s) {
            int y0, y1, c0, nbytes;
            segment_range(g, H, s, &y0, &y1, &c0, &nbytes);
            b = (b + (unsigned long long)(nbytes % 65521) * a + seg_b[first + s]) % 65521ull;
            a = (a + seg_a[first + s]) % 65521ull;
        }
        uint8_t* stream = streams + (size_t)blockIdx.x * capacity;
        put_byte(stream, capacity, 0, 0x78);                      // deflate, 32 KiB window; no preset dictionary, level 0
        put_byte(stream, capacity, 1, 0x01);
        put_byte(stream, capacity, carry, 0x03);                  // final block: fixed codes, end-of-block at once
        put_byte(stream, capacity, carry + 1, 0x00);
        put_byte(stream, capacity, carry + 2, (unsigned)(b >> 8));
        put_byte(stream, capacity, carry + 3, (unsigned)(b & 255));
        put_byte(stream, capacity, carry + 4, (unsigned)(a >> 8));
        put_byte(stream, capacity, carry + 5, (unsigned)(a & 255));
        stream_bytes[blockIdx.x] = carry + 6;
    }
}

// grid (segments, n), 256 threads: the slot's bytes to stream offset off, below capacity; 16-byte stores at aligned addresses
__global__ __launch_bounds__(256) void gather_kernel(const uint8_t* __restrict__ slots, const int* __restrict__ segsize,
                                                     const long long* __restrict__ off, Geo g, uint8_t* __restrict__ streams,
                                                     size_t capacity) {
    const size_t cell = (size_t)blockIdx.y * (size_t)g.nseg + (size_t)blockIdx.x;
    const uint8_t* src = slots + cell * (size_t)g.slot;
    const long long at = off[cell];
    long long size = segsize[cell];                               // <= slot
    if ((unsigned long long)at >= capacity) return;
    if ((unsigned long long)(at + size) > capacity) size = (long long)(capacity - (size_t)at);
    uint8_t* dst = streams + (size_t)blockIdx.y * capacity + (size_t)at;
    long long head = (long long)((16 - ((uintptr_t)dst & 15)) & 15);
    if (head > size) head = size;
    const long long chunks = (size - head) >> 4, tail = head + 16 * chunks;
    for (long long i = threadIdx.x; i < head; i += 256) dst[i] = src[i];
    for (long long c = threadIdx.x; c < chunks; c += 256) {
        const uint8_t* p = src + head + 16 * c;
        unsigned q[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            q[j] = (unsigned)p[4 * j] | ((unsigned)p[4 * j + 1] << 8) | ((unsigned)p[4 * j + 2] << 16) |
                   ((unsigned)p[4 * j + 3] << 24);
        *reinterpret_cast<uint4*>(dst + head + 16 * c) = make_uint4(q[0], q[1], q[2], q[3]);
    }
    for (long long i = tail + threadIdx.x; i < size; i += 256) dst[i] = src[i];
}

bool put_chunk(FILE* f, const char* type, const uint8_t* data, uint32_t len) {
    const uint8_t head[8] = {(uint8_t)(len >> 24), (uint8_t)(len >> 16), (uint8_t)(len >> 8), (uint8_t)len,
                             (uint8_t)type[0], (uint8_t)type[1], (uint8_t)type[2], (uint8_t)type[3]};
    uLong crc = crc32(0L, head + 4, 4);
    if (len) crc = crc32(crc, data, len);
    const uint8_t tail[4] = {(uint8_t)(crc >> 24), (uint8_t)(crc >> 16), (uint8_t)(crc >> 8), (uint8_t)crc};
    return fwrite(head, 1, 8, f) == 8 && (len == 0 || fwrite(data, 1, len, f) == len) && fwrite(tail, 1, 4, f) == 4;
}

}  // namespace

extern "C" size_t oadg_png_encode_stream_capacity(int H, int W) {
    Geo g;
    if (!geometry(H, W, &g)) return 0;
    return (size_t)g.L + 5 * (size_t)g.nseg + 8;                  // every segment stored, header, final block, trailer
}

extern "C" int oadg_png_encode_segments(int H, int W) {
    Geo g;
    if (!geometry(H, W, &g)) return 0;
    return (int)g.nseg;
}

extern "C" size_t oadg_png_encode_workspace_bytes(int n, int H, int W) {
    Geo g;
    if (n < 1 || n > 65535 || !geometry(H, W, &g)) return 0;
    return layout(n, g).total;
}

extern "C" int oadg_png_encode_rgb8(const uint8_t* imgs, int n, int H, int W, int bgr, int filter_mode, uint8_t* streams,
                                    size_t capacity, int64_t* stream_bytes, void* workspace, size_t workspace_bytes,
                                    void* stream) {
    Geo g;
    if (!imgs || !streams || !stream_bytes || !workspace || ((uintptr_t)workspace & 15) || n < 1 || n > 65535 ||
        (bgr != 0 && bgr != 1) || filter_mode < -1 || filter_mode > 4 || !geometry(H, W, &g))
        return OADG_EARG;
    const Layout l = layout(n, g);
    if (workspace_bytes < l.total) return OADG_ESIZE;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    uint8_t* slots = (uint8_t*)(ws + l.slots);
    int* segsize = (int*)(ws + l.size);
    long long* off = (long long*)(ws + l.off);
    unsigned* seg_a = (unsigned*)(ws + l.adler_a);
    unsigned* seg_b = (unsigned*)(ws + l.adler_b);
    const dim3 grid((unsigned)g.nseg, (unsigned)n);
    encode_kernel<<<grid, dim3(THREADS), 0, s>>>(imgs, H, g, bgr, filter_mode, slots, segsize, seg_a, seg_b);
    OADG_LAUNCH_CHECK();
    scan_kernel<<<dim3((unsigned)n), dim3(SCAN), 0, s>>>(segsize, seg_a, seg_b, off, H, g, streams, capacity, stream_bytes);
    OADG_LAUNCH_CHECK();
    gather_kernel<<<grid, dim3(256), 0, s>>>(slots, segsize, off, g, streams, capacity);
    OADG_LAUNCH_CHECK();
    return OADG_OK;
}

extern "C" int oadg_png_write_rgb8(const char* path, const uint8_t* zstream_host, size_t bytes, int H, int W) {
    if (!path || !zstream_host || bytes < 1 || H < 1 || W < 1) return OADG_EARG;
    FILE* f = fopen(path, "wb");
    if (!f) return OADG_EIO;
    static const uint8_t signature[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    const uint8_t ihdr[13] = {(uint8_t)(W >> 24), (uint8_t)(W >> 16), (uint8_t)(W >> 8), (uint8_t)W,
                              (uint8_t)(H >> 24), (uint8_t)(H >> 16), (uint8_t)(H >> 8), (uint8_t)H,
                              8, 2, 0, 0, 0};                     // 8 bits, colour type 2 (RGB), deflate, adaptive, no interlace
    bool ok = fwrite(signature, 1, 8, f) == 8 && put_chunk(f, "IHDR", ihdr, 13);
    const size_t piece = (size_t)1 << 30;                         // (a chunk's length is a 31-bit number)
    for (size_t at = 0; ok && at < bytes; at += piece)
        ok = put_chunk(f, "IDAT", zstream_host + at, (uint32_t)(bytes - at < piece ? bytes - at : piece));
    ok = ok && put_chunk(f, "IEND", nullptr, 0);
    if (fclose(f) != 0) ok = false;
    return ok ? OADG_OK : OADG_EIO;
}
