// Cityscapes gtFine instance-id maps -> what a COCO annotation needs of every instance, for all instances of a map at once.
//
// Replaces, for tools/dataset_converters/cityscapes.py:
//   tools/dataset_converters/cityscapes.py:40-82  load_img_info: per instance id `inst_img == inst_id`, then
//   pycocotools encode / area / toBbox - one pass over the full 1024 x 2048 map PER INSTANCE, on the host.
// Here the maps of a batch are resident (uint16 [n][H][W]) and are read three times in all, whatever the number of instances:
//   oadg_instance_stats          one pass accumulates (pixel count, box) of every id into a dense 65536-entry table per map -
//                                privatised per workgroup in an LDS table keyed by id - and a second kernel compacts the
//                                table into records in ascending id order (np.unique's order);
//   oadg_instance_change_points  the positions where the COLUMN-major flattening of the map (COCO RLE's order) changes value,
//                                as triples (p, value before, value at p) in ascending p: a count pass, a scan, a write pass.
//                                The run lengths of every instance follow from the triples that name it (the tool does that).
// Integer arithmetic only: sums, maxima and an ordered write - the output bytes do not depend on the order of arrival.
// Every LDS index is masked or is a thread index below the array's extent; every global index is checked against H, W,
// the 65536 ids or the caller's capacity before it is used.
#include "common.h"
#include "oadg_hip.h"

namespace {

constexpr int IDS = 65536;               // every uint16 value is a legal id
constexpr int FIELDS = 5;                // per id: count, max x, max y, max (W-1-x), max (H-1-y)   (zero = nothing seen)
constexpr int ST_THREADS = 256;
constexpr int ST_CHUNKS = 4;             // 16-byte chunks (8 pixels) per thread of the statistics pass
constexpr int TAB = 256;                 // slots of the per-workgroup table (a power of two)
constexpr int TAB_SHIFT = 32 - 8;        // hash: the top log2(TAB) bits of id * a golden-ratio constant
constexpr int TAB_PROBES = 16;
constexpr unsigned EMPTY = 0xffffffffu;  // no uint16 id
constexpr int CP_COLS = 64;              // columns of a change-point tile: one wave reads 64 contiguous samples of a row
constexpr int CP_ROWS = 32;              // rows of a segment (one thread walks one column of it)
constexpr int CP_WAVES = 4;              // segments (row blocks) stacked in one workgroup
constexpr int SCAN = 1024;

typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));

struct Layout {
    size_t table, segcnt, segoff, total;   // byte offsets into the workspace
    long nseg;                             // segments per map
    int nrb;                               // row blocks per column
};

Layout layout(int n, int H, int W) {
    Layout l;
    l.nrb = (H + CP_ROWS - 1) / CP_ROWS;
    l.nseg = (long)W * l.nrb;
    l.table = 0;
    l.segcnt = l.table + (size_t)n * FIELDS * IDS * sizeof(int);
    l.segoff = l.segcnt + (size_t)n * l.nseg * sizeof(int);
    l.total = l.segoff + (size_t)n * l.nseg * sizeof(int);
    return l;
}

bool bad_shape(const void* maps, int n, int H, int W, int min_id) {
    if (!maps || ((uintptr_t)maps & 1) || n < 1 || n > 65535 || H < 1 || W < 1 || min_id < 0 || min_id >= IDS) return true;
    if ((long)H * (long)W >= (1L << 31)) return true;                 // p and the counts are int32
    return (W + CP_COLS - 1) / CP_COLS > 65535;                       // (grid.y of the change-point passes)
}

__global__ __launch_bounds__(256) void zero_kernel(int* p, size_t count) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) p[i] = 0;
}

// one horizontal run (id, cnt pixels, columns x0..x1 of row y) into the workgroup's table; a key that finds no slot within
// TAB_PROBES steps goes to the map's table in global memory instead (a tile of a street scene holds few ids: rare)
__device__ __forceinline__ void add_run(unsigned* keys, int* vals, int* g, unsigned id, int cnt, int x0, int x1, int y, int H,
                                        int W) {
    id &= 0xffffu;
    const unsigned h = (id * 2654435761u) >> TAB_SHIFT;
    for (int k = 0; k < TAB_PROBES; ++k) {
        const unsigned s = (h + (unsigned)k) & (TAB - 1);
        const unsigned old = atomicCAS(&keys[s], EMPTY, id);
        if (old == EMPTY || old == id) {
            atomicAdd(&vals[s], cnt);
            atomicMax(&vals[TAB + s], x1);
            atomicMax(&vals[2 * TAB + s], y);
            atomicMax(&vals[3 * TAB + s], W - 1 - x0);
            atomicMax(&vals[4 * TAB + s], H - 1 - y);
            return;
        }
    }
    atomicAdd(&g[id], cnt);
    atomicMax(&g[IDS + id], x1);
    atomicMax(&g[2 * IDS + id], y);
    atomicMax(&g[3 * IDS + id], W - 1 - x0);
    atomicMax(&g[4 * IDS + id], H - 1 - y);
}

// grid (blocks over the map's 16-byte chunks, n).  A chunk is 8 samples at a 16-byte aligned address: the map is read as a
// flat array, so rows whose length is not a multiple of 8 (and maps that do not start on a 16-byte boundary) cost nothing
// but the chunks at the two ends of the map, which are read sample by sample.
__global__ __launch_bounds__(ST_THREADS) void stats_kernel(const uint16_t* __restrict__ maps, int H, int W, int min_id,
                                                           int* __restrict__ table) {
    __shared__ unsigned keys[TAB];
    __shared__ int vals[FIELDS * TAB];
    const long HW = (long)H * W;
    const uint16_t* m = maps + (size_t)blockIdx.y * HW;
    int* g = table + (size_t)blockIdx.y * FIELDS * IDS;
    for (int s = threadIdx.x; s < TAB; s += ST_THREADS) {
        keys[s] = EMPTY;
#pragma unroll
        for (int f = 0; f < FIELDS; ++f) vals[f * TAB + s] = 0;
    }
    __syncthreads();
    const long a = (long)(((uintptr_t)m >> 1) & 7);      // samples between the 16-byte boundary below the map and the map
    const long nchunks = (HW + a + 7) >> 3;
    for (int k = 0; k < ST_CHUNKS; ++k) {
        const long c = ((long)blockIdx.x * ST_CHUNKS + k) * ST_THREADS + threadIdx.x;
        if (c >= nchunks) continue;
        const long lo = 8 * c - a, hi = lo + 8;
        unsigned v[8];
        long first;
        int nv;
        if (lo >= 0 && hi <= HW) {
            const u16x8 q = *reinterpret_cast<const u16x8*>(m + lo);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = q[j];
            first = lo;
            nv = 8;
        } else {
            first = lo > 0 ? lo : 0;
            const long last = hi < HW ? hi : HW;
            nv = (int)(last - first);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = j < nv ? m[first + j] : 0u;
        }
        int y = (int)(first / W), x = (int)(first - (long)y * W);
        unsigned cur = 0;
        int cnt = 0, x0 = 0, x1 = 0, ry = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (j < nv) {
                const unsigned id = v[j];
                if (!(cnt > 0 && id == cur && x != 0)) {          // (x == 0: a new row begins, the run does not continue)
                    if (cnt > 0) add_run(keys, vals, g, cur, cnt, x0, x1, ry, H, W);
                    cur = id; x0 = x; ry = y; cnt = 0;
                }
                if ((int)id >= min_id) { ++cnt; x1 = x; }
                if (++x == W) { x = 0; ++y; }
            }
        }
        if (cnt > 0) add_run(keys, vals, g, cur, cnt, x0, x1, ry, H, W);
    }
    __syncthreads();
    for (int s = threadIdx.x; s < TAB; s += ST_THREADS) {
        const unsigned key = keys[s];
        if (key == EMPTY) continue;
        const unsigned id = key & 0xffffu;
        atomicAdd(&g[id], vals[s]);
        atomicMax(&g[IDS + id], vals[TAB + s]);
        atomicMax(&g[2 * IDS + id], vals[2 * TAB + s]);
        atomicMax(&g[3 * IDS + id], vals[3 * TAB + s]);
        atomicMax(&g[4 * IDS + id], vals[4 * TAB + s]);
    }
}

// inclusive scan of one value per thread over a workgroup of SCAN threads; buf: 2 * SCAN ints of LDS -> (inclusive, total)
__device__ __forceinline__ int block_scan(int v, int* buf, int* total) {
    const int t = threadIdx.x & (SCAN - 1);
    int src = 0;
    buf[t] = v;
    __syncthreads();
    for (int off = 1; off < SCAN; off <<= 1) {
        int s = buf[src * SCAN + t];
        if (t >= off) s += buf[src * SCAN + t - off];
        buf[(src ^ 1) * SCAN + t] = s;
        __syncthreads();
        src ^= 1;
    }
    const int incl = buf[src * SCAN + t];
    *total = buf[src * SCAN + SCAN - 1];
    __syncthreads();
    return incl;
}

// grid (n), SCAN threads: the ids with a non-zero count, >= min_id, in ascending order -> records[map][rank] =
// (id, count, xmin, ymin, xmax, ymax) for rank < capacity; counts[map] = the number of such ids (also when it exceeds capacity)
__global__ __launch_bounds__(SCAN) void stats_compact_kernel(const int* __restrict__ table, int H, int W, int min_id,
                                                             int* __restrict__ records, int capacity, int* __restrict__ counts) {
    __shared__ int part[SCAN];            // [pass of 1024 ids][wave]: the ids present in that wave's 64
    __shared__ int buf[2 * SCAN];
    const int* g = table + (size_t)blockIdx.x * FIELDS * IDS;
    const int tid = threadIdx.x & (SCAN - 1), lane = tid & 63, wave = tid >> 6;      // 16 waves
    for (int it = 0; it < IDS / SCAN; ++it) {
        const int id = it * SCAN + tid;
        const bool present = id >= min_id && g[id] > 0;
        const unsigned long long b = __ballot(present);
        if (lane == 0) part[(it * (SCAN / 64) + wave) & (SCAN - 1)] = __popcll(b);
    }
    __syncthreads();
    const int mine = part[tid];
    int total;
    const int incl = block_scan(mine, buf, &total);
    part[tid] = incl - mine;
    __syncthreads();
    if (tid == 0) counts[blockIdx.x] = total;
    int* out = records + (size_t)blockIdx.x * capacity * 6;
    for (int it = 0; it < IDS / SCAN; ++it) {
        const int id = it * SCAN + tid;
        const int cnt = g[id];
        const bool present = id >= min_id && cnt > 0;
        const unsigned long long b = __ballot(present);
        const int rank = part[(it * (SCAN / 64) + wave) & (SCAN - 1)] + __popcll(b & ((1ull << lane) - 1ull));
        if (present && rank < capacity) {
            int* r = out + (size_t)rank * 6;
            r[0] = id;
            r[1] = cnt;
            r[2] = W - 1 - g[3 * IDS + id];
            r[3] = H - 1 - g[4 * IDS + id];
            r[4] = g[IDS + id];
            r[5] = g[2 * IDS + id];
        }
    }
}

// grid (row blocks / CP_WAVES, columns / CP_COLS, n), 256 threads.  Thread = (column x, row block rb): the segment
// p in [x*H + rb*CP_ROWS, ...) of the column-major order; segment number x*nrb + rb ascends with p.  Lane l of a wave reads
// column x0 + l of one row: 64 contiguous samples.  WRITE false: seg[segment] = its change points; WRITE true: seg[segment]
// is the rank of its first change point within the map, the triples go to triples[map][rank..] while rank < capacity.
template <bool WRITE>
__global__ __launch_bounds__(CP_COLS * CP_WAVES) void change_kernel(const uint16_t* __restrict__ maps, int H, int W, int nrb,
                                                                    int min_id, int* __restrict__ seg, int* __restrict__ triples,
                                                                    int capacity) {
    const int x = blockIdx.y * CP_COLS + (threadIdx.x & 63);
    const long rbl = (long)blockIdx.x * CP_WAVES + (threadIdx.x >> 6);
    if (x >= W || rbl >= nrb) return;
    const int rb = (int)rbl;
    const long HW = (long)H * W;
    const uint16_t* m = maps + (size_t)blockIdx.z * HW;
    const size_t segidx = (size_t)blockIdx.z * ((size_t)W * nrb) + (size_t)x * nrb + rb;
    const int y0 = rb * CP_ROWS, y1 = y0 + CP_ROWS < H ? y0 + CP_ROWS : H;
    bool has_prev = true;
    int prev = 0;
    if (y0 > 0) prev = m[(long)(y0 - 1) * W + x];
    else if (x > 0) prev = m[(long)(H - 1) * W + x - 1];      // the bottom of the column to the left precedes the top of this one
    else has_prev = false;                                     // p = 0
    const long rank0 = WRITE ? (long)seg[segidx] : 0;
    int* out = triples + (WRITE ? (size_t)blockIdx.z * capacity * 3 : 0);
    int cnt = 0;
    for (int y = y0; y < y1; y += 8) {
        int v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = y + j < y1 ? m[(long)(y + j) * W + x] : 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (y + j < y1) {
                const int cur = v[j];
                if (has_prev && cur != prev && (cur >= min_id || prev >= min_id)) {
                    if (WRITE) {
                        const long r = rank0 + cnt;
                        if (r < capacity) {
                            int* t = out + (size_t)r * 3;
                            t[0] = (int)((long)x * H + y + j);
                            t[1] = prev;
                            t[2] = cur;
                        }
                    }
                    ++cnt;
                }
                prev = cur;
                has_prev = true;
            }
        }
    }
    if (!WRITE) seg[segidx] = cnt;
}

// grid (n), SCAN threads: off[map][s] = the sum of cnt[map][0..s), counts[map] = the sum of all
__global__ __launch_bounds__(SCAN) void seg_scan_kernel(const int* __restrict__ cnt, int* __restrict__ off, long nseg,
                                                        int* __restrict__ counts) {
    __shared__ int buf[2 * SCAN];
    const int* c = cnt + (size_t)blockIdx.x * nseg;
    int* o = off + (size_t)blockIdx.x * nseg;
    const int tid = threadIdx.x & (SCAN - 1);
    int carry = 0;
    for (long base = 0; base < nseg; base += SCAN) {
        const long i = base + tid;
        const int v = i < nseg ? c[i] : 0;
        int total;
        const int incl = block_scan(v, buf, &total);
        if (i < nseg) o[i] = carry + incl - v;
        carry += total;
    }
    if (tid == 0) counts[blockIdx.x] = carry;
}

}  // namespace

extern "C" size_t oadg_instance_maps_workspace_bytes(int n, int H, int W) {
    if (n < 1 || H < 1 || W < 1 || (long)H * (long)W >= (1L << 31)) return 0;
    return layout(n, H, W).total;
}

extern "C" int oadg_instance_stats(const uint16_t* maps, int n, int H, int W, int min_id, int32_t* records, int capacity,
                                   int32_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    if (bad_shape(maps, n, H, W, min_id) || capacity < 0 || (capacity > 0 && !records) || !counts || !workspace)
        return OADG_EARG;
    const Layout l = layout(n, H, W);
    if (workspace_bytes < l.total) return OADG_ESIZE;
    hipStream_t s = (hipStream_t)stream;
    int* table = (int*)((char*)workspace + l.table);
    const size_t cells = (size_t)n * FIELDS * IDS;
    zero_kernel<<<dim3((unsigned)((cells + 256 * 16 - 1) / (256 * 16))), dim3(256), 0, s>>>(table, cells);
    OADG_LAUNCH_CHECK();
    const long nchunks = ((long)H * W + 7 + 7) / 8;                   // (at most: a misaligned map has one chunk more)
    const long per_block = (long)ST_THREADS * ST_CHUNKS;
    stats_kernel<<<dim3((unsigned)((nchunks + per_block - 1) / per_block), (unsigned)n), dim3(ST_THREADS), 0, s>>>(
        maps, H, W, min_id, table);
    OADG_LAUNCH_CHECK();
    stats_compact_kernel<<<dim3((unsigned)n), dim3(SCAN), 0, s>>>(table, H, W, min_id, records, capacity, counts);
    OADG_LAUNCH_CHECK();
    return OADG_OK;
}

extern "C" int oadg_instance_change_points(const uint16_t* maps, int n, int H, int W, int min_id, int32_t* triples,
                                           int capacity, int32_t* counts, void* workspace, size_t workspace_bytes,
                                           void* stream) {
    if (bad_shape(maps, n, H, W, min_id) || capacity < 0 || (capacity > 0 && !triples) || !counts || !workspace)
        return OADG_EARG;
    const Layout l = layout(n, H, W);
    if (workspace_bytes < l.total) return OADG_ESIZE;
    hipStream_t s = (hipStream_t)stream;
    int* segcnt = (int*)((char*)workspace + l.segcnt);
    int* segoff = (int*)((char*)workspace + l.segoff);
    const dim3 grid((unsigned)((l.nrb + CP_WAVES - 1) / CP_WAVES), (unsigned)((W + CP_COLS - 1) / CP_COLS), (unsigned)n);
    change_kernel<false><<<grid, dim3(CP_COLS * CP_WAVES), 0, s>>>(maps, H, W, l.nrb, min_id, segcnt, nullptr, 0);
    OADG_LAUNCH_CHECK();
    seg_scan_kernel<<<dim3((unsigned)n), dim3(SCAN), 0, s>>>(segcnt, segoff, l.nseg, counts);
    OADG_LAUNCH_CHECK();
    change_kernel<true><<<grid, dim3(CP_COLS * CP_WAVES), 0, s>>>(maps, H, W, l.nrb, min_id, segoff, triples, capacity);
    OADG_LAUNCH_CHECK();
    return OADG_OK;
}
