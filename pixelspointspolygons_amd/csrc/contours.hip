// p3hip - FFL initial contours: marching squares + contour assembly on the device (predict/ffl/polygonize_utils.py:15-44, which calls
// skimage.measure.find_contours(indicator, level, fully_connected='low', positive_orientation='high') per image on the host).
//   p3_init_contours   fp32 map [B,H,W] (any strides) -> the TensorPoly fields p3_acm_optimize consumes, contours ordered by image, then by their smallest segment key.
//
// A vertex is a crossed grid edge (horizontal edge (r,c): pixels (r,c)-(r,c+1), id r (W-1) + c; vertical edge (r,c): pixels (r,c)-(r+1,c), id H (W-1) + r W + c).
// Linking is by edge identity: every segment from -> to of a cell gives succ[to] = from ('high' walks segments backwards), and an edge is the `to` of at most one
// segment and the `from` of at most one (its two cells), so every array below has ONE writer per element: no atomics, the same bits in every run, and an image's
// contours do not depend on what else is in the batch.
//   1 ic_count      one thread per grid edge: crossed or not (it evaluates the edge's two cells itself), count per 1024-edge tile
//   2 ic_scan_tiles exclusive scan of the tile counts (one workgroup)
//   3 ic_compact    crossed edges -> compact vertices in edge order (image-major): position, succ / pred as edge ids, key of the segment the vertex is the `to` of
//   4 ic_link       edge ids -> vertex ids; state of pass 1
//   5 pass 1, R rounds of pointer doubling along succ: minimum and maximum segment key of the 2^R vertices behind each vertex.  A vertex without successor (the last of
//     an open contour) loops onto itself with the maximum IC_NONE, which therefore marks every vertex of an open contour.
//   6 ic_rank_init  the start of a contour: the vertex without predecessor (open), or the `to` vertex of the largest-key segment (closed: key == maximum).  Starts loop
//     onto themselves; pass 2, R rounds along pred, gives every vertex its start and its distance from it.
//   7 ic_tails      the last vertex of each contour (no successor, or its successor is the start) writes the contour's length at (image, smallest key) of a table over
//     all segment keys; 8-10 scan that table (vertex offsets, contour numbers, longest, totals, status); 11 ic_emit places every vertex.
// R = ceil(log2(edges per image)): no contour has more vertices than its image has edges.
// The two passes exist twice (the same round functions, the same bits):
//   image   ONE launch per pass, one workgroup of 1024 threads per image with a barrier per round (lists never leave their image): 11 kernels and one memset.
//           Taken up to IC_IMAGE_MAX_EDGES edges per image: 85 us against 135 us for 16 tiles of 224 x 224.
//   rounds  one launch per round on a fixed grid over the vertex count read from device memory: 10 + 2 R kernels and one memset (45 in all at R = 17).  For
//           larger maps, where one workgroup would walk an image's vertices alone.
// Either way the number of launches depends on B, H, W only.  P3_IC_DOUBLING=image / rounds forces one (A/B runs and tests; read at every call).
#include "p3_common.h"
#include <stdlib.h>

#pragma clang fp contract(off)

#define IC_THREADS 256
#define IC_ITEMS 4
#define IC_TILE (IC_THREADS * IC_ITEMS)
#define IC_SCAN_THREADS 1024
#define IC_NONE 0x7fffffff
#define IC_MAX_GRID 2048          // workgroups of the grid-stride kernels
#define IC_IMAGE_THREADS 1024
#define IC_LDS_CAP 2048           // vertices of an image whose doubling state stays in LDS: 2 buffers x 16 B x 2048 = 64 KiB
#ifndef IC_IMAGE_MAX_EDGES
#define IC_IMAGE_MAX_EDGES (1 << 17)          // edges per image up to which the one-workgroup-per-image passes are taken (224 x 224: 99904)
#endif

enum { IC_T = 0, IC_R = 1, IC_B = 2, IC_L = 3 };
// the segments from -> to per case = (ul > level) + 2 (ur > level) + 4 (ll > level) + 8 (lr > level), two slots each, 6 and 9 in their fully_connected='low' form:
//   1 T-L | 2 R-T | 3 R-L | 4 L-B | 5 T-B | 6 R-T, L-B | 7 R-B | 8 B-R | 9 T-L, B-R | 10 B-T | 11 B-L | 12 L-R | 13 T-R | 14 L-T
// packed as immediates (a table in memory would cost every crossed edge a dependent load): entry i = 2 case + slot holds 2 bits of IC_SEG_FROM and of IC_SEG_TO
#define IC_SEG_FROM 0x30322821d031100ull
#define IC_SEG_TO 0x11307128223030ull
#define IC_SEG_VALID 0x155d7554u

struct IcMap {
    const float* ind;
    int64_t sb, sr, sc;          // strides in elements
    int B, H, W;
    double level;
    int E, Hh, K;                // edges per image, horizontal edges per image, segment keys per image
    int tpe, tpk;                // tiles per image of the edge space and of the key space
};
struct IcEdge { int succ, pred, key; float2 pos; };          // succ / pred: edge ids inside the image, -1 = none; key: IC_NONE without successor

__device__ __forceinline__ double ic_at(const IcMap& m, int b, int r, int c) { return (double)m.ind[b * m.sb + r * m.sr + c * m.sc]; }

__device__ __forceinline__ int ic_side_edge(const IcMap& m, int r, int c, int side) {
    if (side == IC_T) return r * (m.W - 1) + c;
    if (side == IC_B) return (r + 1) * (m.W - 1) + c;
    if (side == IC_L) return m.Hh + r * m.W + c;
    return m.Hh + r * m.W + c + 1;
}

// what cell (r, c) with these corners makes of its side `side`: the segment that ends there gives the successor and the key, the one that starts there the predecessor
__device__ __forceinline__ void ic_cell_role(const IcMap& m, int r, int c, double ul, double ur, double ll, double lr, int side, IcEdge& e) {
    if (ul != ul || ur != ur || ll != ll || lr != lr) return;          // a cell with a NaN corner emits nothing
    const int cs = (ul > m.level ? 1 : 0) + (ur > m.level ? 2 : 0) + (ll > m.level ? 4 : 0) + (lr > m.level ? 8 : 0);
#pragma unroll
    for (int slot = 0; slot < 2; ++slot) {
        const int i = 2 * cs + slot;
        if (!((IC_SEG_VALID >> i) & 1u)) break;
        const int from = (int)((IC_SEG_FROM >> (2 * i)) & 3ull), to = (int)((IC_SEG_TO >> (2 * i)) & 3ull);
        if (to == side) { e.succ = ic_side_edge(m, r, c, from); e.key = 2 * (r * (m.W - 1) + c) + slot; }
        if (from == side) e.pred = ic_side_edge(m, r, c, to);
    }
}

// the two pixels of edge `id` of image b (id < E)
struct IcEnds { double p, q; int r, c; bool horizontal; };
__device__ __forceinline__ IcEnds ic_ends(const IcMap& m, int b, int id) {
    IcEnds n;
    n.horizontal = id < m.Hh;
    if (n.horizontal) { n.r = id / (m.W - 1); n.c = id - n.r * (m.W - 1); }
    else { const int v = id - m.Hh; n.r = v / m.W; n.c = v - n.r * m.W; }
    n.p = ic_at(m, b, n.r, n.c);
    n.q = n.horizontal ? ic_at(m, b, n.r, n.c + 1) : ic_at(m, b, n.r + 1, n.c);
    return n;
}
// a cell without NaN has a segment on a side exactly when the side's two ends differ
__device__ __forceinline__ bool ic_differ(const IcMap& m, const IcEnds& n) { return n.p == n.p && n.q == n.q && (n.p > m.level) != (n.q > m.level); }

// an edge whose ends differ: false when no segment touches it after all (both of its cells hold a NaN).  The four other corners of its two cells are loaded
// together (clamped into the map where a cell does not exist), then both cells are evaluated from registers.
__device__ __forceinline__ bool ic_edge(const IcMap& m, int b, const IcEnds& n, IcEdge& e) {
    const int r = n.r, c = n.c;
    e.succ = -1; e.pred = -1; e.key = IC_NONE;
    if (n.horizontal) {          // cell (r-1, c) above has the edge as its bottom, cell (r, c) below as its top
        const bool above = r >= 1, below = r <= m.H - 2;
        const int ra = above ? r - 1 : r, rb = below ? r + 1 : r;
        const double a0 = ic_at(m, b, ra, c), a1 = ic_at(m, b, ra, c + 1), b0 = ic_at(m, b, rb, c), b1 = ic_at(m, b, rb, c + 1);
        if (above) ic_cell_role(m, r - 1, c, a0, a1, n.p, n.q, IC_B, e);
        if (below) ic_cell_role(m, r, c, n.p, n.q, b0, b1, IC_T, e);
    } else {                     // cell (r, c-1) on the left has the edge as its right side, cell (r, c) as its left side
        const bool left = c >= 1, right = c <= m.W - 2;
        const int ca = left ? c - 1 : c, cb = right ? c + 1 : c;
        const double a0 = ic_at(m, b, r, ca), a1 = ic_at(m, b, r + 1, ca), b0 = ic_at(m, b, r, cb), b1 = ic_at(m, b, r + 1, cb);
        if (left) ic_cell_role(m, r, c - 1, a0, n.p, a1, n.q, IC_R, e);
        if (right) ic_cell_role(m, r, c, n.p, b0, n.q, b1, IC_L, e);
    }
    if (e.succ < 0 && e.pred < 0) return false;
    const double f = (m.level - n.p) / (n.q - n.p);          // p != q here; one division and one addition in double, rounded to fp32 once
    e.pos = n.horizontal ? make_float2((float)r, (float)((double)c + f)) : make_float2((float)((double)r + f), (float)c);
    return true;
}

// 1: grid (tiles per image, B).  A thread takes IC_ITEMS consecutive edges: their pixels are loaded before any is looked at
__global__ __launch_bounds__(IC_THREADS) void ic_count_kernel(IcMap m, int* tile_sums) {
    __shared__ int lds[IC_THREADS / 64];
    const int b = blockIdx.y, first = blockIdx.x * IC_TILE + threadIdx.x * IC_ITEMS;
    IcEnds n[IC_ITEMS];
#pragma unroll
    for (int j = 0; j < IC_ITEMS; ++j) n[j] = ic_ends(m, b, min(first + j, m.E - 1));
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < IC_ITEMS; ++j) {
        IcEdge e;
        if (first + j < m.E && ic_differ(m, n[j]) && ic_edge(m, b, n[j], e)) ++cnt;
    }
    int total;
    wg_scan<false, int>(cnt, lds, total);
    if (threadIdx.x == 0) tile_sums[b * m.tpe + blockIdx.x] = total;
}

// 2: one workgroup.  sums[0 .. n) -> exclusive prefix sums in place, sums[n] = total
__global__ __launch_bounds__(IC_SCAN_THREADS) void ic_scan_tiles_kernel(int* sums, int n) {
    __shared__ int lds[IC_SCAN_THREADS / 64];
    int carry = 0;
    for (int at = 0; at < n; at += IC_SCAN_THREADS) {
        const int i = at + threadIdx.x;
        const int ex = wg_excl(i < n ? sums[i] : 0, lds, carry);
        if (i < n) sums[i] = ex;
    }
    if (threadIdx.x == 0) sums[n] = carry;
}

// 3: grid (tiles per image, B).  vertex_of [B * E]: the vertex of a crossed edge, -1 otherwise
__global__ __launch_bounds__(IC_THREADS) void ic_compact_kernel(IcMap m, const int* tile_offs, int* vertex_of, float2* vpos, int* vsucc, int* vpred, int* vkey,
                                                                int* vimg) {
    __shared__ int lds[IC_THREADS / 64];
    const int b = blockIdx.y, first = blockIdx.x * IC_TILE + threadIdx.x * IC_ITEMS;
    IcEnds n[IC_ITEMS];
#pragma unroll
    for (int j = 0; j < IC_ITEMS; ++j) n[j] = ic_ends(m, b, min(first + j, m.E - 1));
    IcEdge e[IC_ITEMS];
    bool on[IC_ITEMS];
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < IC_ITEMS; ++j) {
        on[j] = first + j < m.E && ic_differ(m, n[j]) && ic_edge(m, b, n[j], e[j]);
        cnt += on[j] ? 1 : 0;
    }
    int total;
    int v = tile_offs[b * m.tpe + blockIdx.x] + wg_scan<false, int>(cnt, lds, total) - cnt;
#pragma unroll
    for (int j = 0; j < IC_ITEMS; ++j) {
        if (first + j < m.E) vertex_of[(int64_t)b * m.E + first + j] = on[j] ? v : -1;
        if (on[j]) { vpos[v] = e[j].pos; vsucc[v] = e[j].succ; vpred[v] = e[j].pred; vkey[v] = e[j].key; vimg[v] = b; ++v; }
    }
}

// 4: succ / pred become vertex ids (in place); st1 = (next, smallest key, largest key, unused) of pass 1
__global__ __launch_bounds__(IC_THREADS) void ic_link_kernel(const int* nv, int E, const int* vertex_of, const int* vimg, const int* vkey, int* vsucc, int* vpred, int4* st1) {
    const int n = *nv;
    for (int v = blockIdx.x * IC_THREADS + threadIdx.x; v < n; v += gridDim.x * IC_THREADS) {
        const int64_t base = (int64_t)vimg[v] * E;
        const int se = vsucc[v], pe = vpred[v];
        const int s = se >= 0 ? vertex_of[base + se] : -1, p = pe >= 0 ? vertex_of[base + pe] : -1;
        vsucc[v] = s;
        vpred[v] = p;
        const int key = s >= 0 ? vkey[v] : IC_NONE;
        st1[v] = make_int4(s >= 0 ? s : v, key, key, 0);          // smallest: IC_NONE is neutral; largest: IC_NONE marks an open contour
    }
}

__device__ __forceinline__ int4 ic_minmax_step(const int4* src, int v) {
    const int4 a = src[v], s = src[a.x];
    return make_int4(s.x, min(a.y, s.y), max(a.z, s.z), 0);
}
__device__ __forceinline__ int2 ic_rank_step(const int2* src, int v) {
    const int2 a = src[v], s = src[a.x];
    return make_int2(s.x, a.y + s.y);
}
// the start of v's contour loops onto itself at distance 0; everyone else points at its predecessor
__device__ __forceinline__ int2 ic_rank_first(const int4* st1, const int* vpred, const int* vkey, int v) {
    const int p = vpred[v], largest = st1[v].z;
    const bool start = p < 0 || (largest != IC_NONE && vkey[v] == largest);
    return start ? make_int2(v, 0) : make_int2(p, 1);
}

// 5: one round of pass 1
__global__ __launch_bounds__(IC_THREADS) void ic_minmax_round_kernel(const int* nv, const int4* src, int4* dst) {
    const int n = *nv;
    for (int v = blockIdx.x * IC_THREADS + threadIdx.x; v < n; v += gridDim.x * IC_THREADS) dst[v] = ic_minmax_step(src, v);
}
// 6
__global__ __launch_bounds__(IC_THREADS) void ic_rank_init_kernel(const int* nv, const int4* st1, const int* vpred, const int* vkey, int2* st2) {
    const int n = *nv;
    for (int v = blockIdx.x * IC_THREADS + threadIdx.x; v < n; v += gridDim.x * IC_THREADS) st2[v] = ic_rank_first(st1, vpred, vkey, v);
}
// one round of pass 2
__global__ __launch_bounds__(IC_THREADS) void ic_rank_round_kernel(const int* nv, const int2* src, int2* dst) {
    const int n = *nv;
    for (int v = blockIdx.x * IC_THREADS + threadIdx.x; v < n; v += gridDim.x * IC_THREADS) dst[v] = ic_rank_step(src, v);
}
// 5 and 6 of small maps: all rounds of a pass in one launch, one workgroup per image (its vertices are tile_offs[b * tpe] .. tile_offs[(b + 1) * tpe)), a barrier per
// round.  Lists never leave their image.  An image of up to IC_LDS_CAP vertices keeps both buffers in LDS (vertex ids relative to the image's first); a larger one
// ping-pongs in global memory, where a workgroup's own writes are visible to it after the barrier.  The same steps in the same order: the same bits.
__global__ __launch_bounds__(IC_IMAGE_THREADS) void ic_minmax_image_kernel(const int* tile_offs, int tpe, int rounds, int4* a, int4* b) {
    __shared__ int4 sm[2][IC_LDS_CAP];
    const int v0 = tile_offs[blockIdx.x * tpe], v1 = tile_offs[(blockIdx.x + 1) * tpe], n = v1 - v0;
    if (n <= IC_LDS_CAP) {          // uniform over the workgroup
        for (int v = threadIdx.x; v < n; v += IC_IMAGE_THREADS) { int4 t = a[v0 + v]; t.x -= v0; sm[0][v] = t; }
        __syncthreads();
        for (int k = 0; k < rounds; ++k) {
            for (int v = threadIdx.x; v < n; v += IC_IMAGE_THREADS) sm[(k + 1) & 1][v] = ic_minmax_step(sm[k & 1], v);
            __syncthreads();
        }
        int4* out = (rounds & 1) ? b : a;
        for (int v = threadIdx.x; v < n; v += IC_IMAGE_THREADS) { int4 t = sm[rounds & 1][v]; t.x += v0; out[v0 + v] = t; }
        return;
    }
    for (int k = 0; k < rounds; ++k) {
        const int4* src = (k & 1) ? b : a;
        int4* dst = (k & 1) ? a : b;
        for (int v = v0 + threadIdx.x; v < v1; v += IC_IMAGE_THREADS) dst[v] = ic_minmax_step(src, v);
        __syncthreads();
    }
}
__global__ __launch_bounds__(IC_IMAGE_THREADS) void ic_rank_image_kernel(const int* tile_offs, int tpe, int rounds, const int4* st1, const int* vpred, const int* vkey,
                                                                         int2* a, int2* b) {
    __shared__ int2 sm[2][IC_LDS_CAP];
    const int v0 = tile_offs[blockIdx.x * tpe], v1 = tile_offs[(blockIdx.x + 1) * tpe], n = v1 - v0;
    if (n <= IC_LDS_CAP) {
        for (int v = threadIdx.x; v < n; v += IC_IMAGE_THREADS) { int2 t = ic_rank_first(st1, vpred, vkey, v0 + v); t.x -= v0; sm[0][v] = t; }
        __syncthreads();
        for (int k = 0; k < rounds; ++k) {
            for (int v = threadIdx.x; v < n; v += IC_IMAGE_THREADS) sm[(k + 1) & 1][v] = ic_rank_step(sm[k & 1], v);
            __syncthreads();
        }
        int2* out = (rounds & 1) ? b : a;
        for (int v = threadIdx.x; v < n; v += IC_IMAGE_THREADS) { int2 t = sm[rounds & 1][v]; t.x += v0; out[v0 + v] = t; }
        return;
    }
    for (int v = v0 + threadIdx.x; v < v1; v += IC_IMAGE_THREADS) a[v] = ic_rank_first(st1, vpred, vkey, v);
    __syncthreads();
    for (int k = 0; k < rounds; ++k) {
        const int2* src = (k & 1) ? b : a;
        int2* dst = (k & 1) ? a : b;
        for (int v = v0 + threadIdx.x; v < v1; v += IC_IMAGE_THREADS) dst[v] = ic_rank_step(src, v);
        __syncthreads();
    }
}

// 7: klen [B * K] (zeroed before): the contour's vertex count at (image, smallest segment key), written by the contour's last vertex
__global__ __launch_bounds__(IC_THREADS) void ic_tails_kernel(const int* nv, int K, const int4* st1, const int2* st2, const int* vsucc, const int* vimg, int* klen) {
    const int n = *nv;
    for (int v = blockIdx.x * IC_THREADS + threadIdx.x; v < n; v += gridDim.x * IC_THREADS) {
        const int2 me = st2[v];          // (start, distance from it)
        const int s = vsucc[v];
        if (s >= 0 && s != me.x) continue;
        const int key = st1[me.x].y;          // at the start the minimum covers the whole contour
        if (key >= 0 && key < K) klen[(int64_t)vimg[v] * K + key] = me.y + 1;
    }
}

// 8: grid (tiles per image, B) over the key table: (vertices << 32 | contours) and the longest contour per tile
__global__ __launch_bounds__(IC_THREADS) void ic_key_reduce_kernel(int K, int tpk, const int* klen, unsigned long long* tile_sums, int* tile_max) {
    __shared__ unsigned long long lds[IC_THREADS / 64];
    __shared__ int lmax[IC_THREADS / 64];
    const int b = blockIdx.y;
    unsigned long long acc = 0;
    int longest = 0;
#pragma unroll
    for (int j = 0; j < IC_ITEMS; ++j) {
        const int k = blockIdx.x * IC_TILE + threadIdx.x * IC_ITEMS + j;
        const int len = k < K ? klen[(int64_t)b * K + k] : 0;
        if (len > 0) { acc += p3_pack2(len, 1); longest = max(longest, len); }
    }
    const int mx = wg_max(longest, lmax);
    unsigned long long total;
    wg_scan<false, unsigned long long>(acc, lds, total);
    if (threadIdx.x == 0) {
        tile_sums[b * tpk + blockIdx.x] = total;
        tile_max[b * tpk + blockIdx.x] = mx;
    }
}

// 9: one workgroup: exclusive scan of the key tiles in place, the totals and the status
__global__ __launch_bounds__(IC_SCAN_THREADS) void ic_key_scan_tiles_kernel(unsigned long long* sums, const int* tile_max, int B, int tpk, int max_vertices,
                                                                            int max_contours, int32_t* counts, int32_t* n_contours, int32_t* n_vertices,
                                                                            int32_t* status) {
    __shared__ unsigned long long lds[IC_SCAN_THREADS / 64];
    __shared__ int lmax[IC_SCAN_THREADS / 64];
    const int n = B * tpk;
    unsigned long long carry = 0;
    int longest = 0;
    for (int at = 0; at < n; at += IC_SCAN_THREADS) {
        const int i = at + threadIdx.x;
        if (i < n) longest = max(longest, tile_max[i]);
        const unsigned long long ex = wg_excl(i < n ? sums[i] : 0ull, lds, carry);
        if (i < n) sums[i] = ex;
    }
    if (threadIdx.x == 0) sums[n] = carry;
    // the maximum by hand, thread 0 folds the 16 wave maxima below: wg_max here (its two barriers over 16 waves, every thread folding) measured 0.4 us on the 85 us
    // of the whole call, on the one serial workgroup every launch of the stage waits for
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) longest = max(longest, __shfl_xor(longest, o, 64));
    if ((threadIdx.x & 63) == 0) lmax[threadIdx.x >> 6] = longest;
    __syncthreads();          // lmax[], and sums[] of this workgroup, are visible to it
    for (int b = threadIdx.x; b < B; b += IC_SCAN_THREADS) {
        const unsigned long long d = sums[(b + 1) * tpk] - sums[b * tpk];
        n_vertices[b] = p3_hi32(d);
        n_contours[b] = p3_lo32(d);
    }
    if (threadIdx.x == 0) {
        int mx = 0;
        for (int i = 0; i < IC_SCAN_THREADS / 64; ++i) mx = max(mx, lmax[i]);
        const int N = p3_hi32(carry), P = p3_lo32(carry);
        counts[0] = N; counts[1] = P; counts[2] = mx;
        status[0] = (N > max_vertices || P > max_contours) ? 1 : 0;
    }
}

// 10: grid (tiles per image, B): where a contour's key sits, its first vertex slot and its number
__global__ __launch_bounds__(IC_THREADS) void ic_key_place_kernel(int K, int tpk, const int* klen, const unsigned long long* tile_offs, int* koff, int* kidx) {
    __shared__ unsigned long long lds[IC_THREADS / 64];
    const int b = blockIdx.y;
    const int first = blockIdx.x * IC_TILE + threadIdx.x * IC_ITEMS;
    int len[IC_ITEMS];
    unsigned long long mine = 0;
#pragma unroll
    for (int j = 0; j < IC_ITEMS; ++j) {
        len[j] = first + j < K ? klen[(int64_t)b * K + first + j] : 0;
        if (len[j] > 0) mine += p3_pack2(len[j], 1);
    }
    unsigned long long total;
    unsigned long long at = tile_offs[b * tpk + blockIdx.x] + wg_scan<false, unsigned long long>(mine, lds, total) - mine;
#pragma unroll
    for (int j = 0; j < IC_ITEMS; ++j) {
        if (len[j] <= 0) continue;
        koff[(int64_t)b * K + first + j] = p3_hi32(at);
        kidx[(int64_t)b * K + first + j] = p3_lo32(at);
        at += p3_pack2(len[j], 1);
    }
}

// 11: every vertex to its slot; a contour's start writes the contour's row.  Nothing past the capacities.
__global__ __launch_bounds__(IC_THREADS) void ic_emit_kernel(const int* nv, int K, const int4* st1, const int2* st2, const int* vimg, const float2* vpos, const int* klen,
                                                             const int* koff, const int* kidx, int max_vertices, int max_contours, float2* pos, int64_t* poly_slice,
                                                             int32_t* poly_batch, int64_t* batch, uint8_t* is_endpoint) {
    const int n = *nv;
    for (int v = blockIdx.x * IC_THREADS + threadIdx.x; v < n; v += gridDim.x * IC_THREADS) {
        const int2 me = st2[v];
        const int4 head = st1[me.x];
        const int img = vimg[v];
        if (head.y < 0 || head.y >= K) continue;
        const int64_t q = (int64_t)img * K + head.y;
        const int len = klen[q], off = koff[q], at = off + me.y;
        if (at >= 0 && at < max_vertices) {
            pos[at] = vpos[v];
            batch[at] = img;
            is_endpoint[at] = (head.z == IC_NONE && (me.y == 0 || me.y == len - 1)) ? 1 : 0;
        }
        if (me.y == 0) {
            const int p = kidx[q];
            if (p >= 0 && p < max_contours) { poly_slice[2 * p] = off; poly_slice[2 * p + 1] = (int64_t)off + len; poly_batch[p] = img; }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- workspace
struct IcWs {
    int64_t E, K, tpe, tpk, BE, BK;
    int rounds;
    int* vertex_of;
    float2* vpos;
    int *vsucc, *vpred, *vkey, *vimg;
    int4* st[2];          // pass 1 ping-pongs between the two; pass 2 lives in the one pass 1 did not finish in
    int *klen, *koff, *kidx, *esums;
    unsigned long long* ksums;
    int* kmax;
};
static IcWs ic_carve(int B, int H, int W, P3Carve& c) {
    IcWs l;
    memset(&l, 0, sizeof l);
    if (B < 1 || H < 2 || W < 2) return l;
    l.E = (int64_t)H * (W - 1) + (int64_t)(H - 1) * W;
    l.K = 2 * (int64_t)(H - 1) * (W - 1);
    l.tpe = (l.E + IC_TILE - 1) / IC_TILE;
    l.tpk = (l.K + IC_TILE - 1) / IC_TILE;
    l.BE = B * l.E;
    l.BK = B * l.K;
    l.rounds = 1;
    while (((int64_t)1 << l.rounds) < l.E) ++l.rounds;
    l.vertex_of = c.take<int>(l.BE);
    l.vpos = c.take<float2>(l.BE);
    l.vsucc = c.take<int>(l.BE);
    l.vpred = c.take<int>(l.BE);
    l.vkey = c.take<int>(l.BE);
    l.vimg = c.take<int>(l.BE);
    l.st[0] = c.take<int4>(l.BE);
    l.st[1] = c.take<int4>(l.BE);
    l.klen = c.take<int>(l.BK);
    l.koff = c.take<int>(l.BK);
    l.kidx = c.take<int>(l.BK);
    l.esums = c.take<int>(B * l.tpe + 1);
    l.ksums = c.take<unsigned long long>(B * l.tpk + 1);
    l.kmax = c.take<int>(B * l.tpk);
    return l;
}

extern "C" int64_t p3_init_contours_workspace_bytes(int B, int H, int W) {
    P3Carve c = {nullptr, 0};
    ic_carve(B, H, W, c);
    return c.at;
}

extern "C" int p3_init_contours(const float* indicator, int64_t stride_b, int64_t stride_r, int64_t stride_c, int B, int H, int W, double level, int max_vertices,
                                int max_contours, float* pos, int64_t* poly_slice, int32_t* poly_batch, int64_t* batch, uint8_t* is_endpoint, int32_t* counts,
                                int32_t* n_contours, int32_t* n_vertices, int32_t* status, void* workspace, void* stream) {
    P3_CHECK(B >= 1 && H >= 1 && W >= 1 && max_vertices >= 0 && max_contours >= 0, P3_ESHAPE, "p3_init_contours: bad sizes (B, H, W >= 1; capacities >= 0)");
    P3_CHECK((int64_t)B * ((int64_t)H * W) * 2 < ((int64_t)1 << 31), P3_ESHAPE, "p3_init_contours: B * H * W * 2 must stay below 2^31");
    P3_CHECK(indicator && counts && n_contours && n_vertices && status, P3_EINVAL, "p3_init_contours: null pointer");
    P3_CHECK((max_vertices == 0 || (pos && batch && is_endpoint)) && (max_contours == 0 || (poly_slice && poly_batch)), P3_EINVAL,
             "p3_init_contours: null output with a capacity above 0");
    P3_CHECK(level == level, P3_EINVAL, "p3_init_contours: level is NaN");
    hipStream_t s = (hipStream_t)stream;
    if (H < 2 || W < 2) {          // no cell, no contour
        P3_TRY(p3_memset(counts, 0, 3 * sizeof(int32_t), s));
        P3_TRY(p3_memset(n_contours, 0, B * sizeof(int32_t), s));
        P3_TRY(p3_memset(n_vertices, 0, B * sizeof(int32_t), s));
        return p3_memset(status, 0, sizeof(int32_t), s);
    }
    P3_CHECK(workspace, P3_EINVAL, "p3_init_contours: null workspace (p3_init_contours_workspace_bytes(B, H, W))");
    P3_CHECK(B <= 65535, P3_ESHAPE, "p3_init_contours: B > 65535");
    P3Carve carve = {(char*)workspace, 0};
    const IcWs l = ic_carve(B, H, W, carve);
    IcMap m;
    m.ind = indicator; m.sb = stride_b; m.sr = stride_r; m.sc = stride_c; m.B = B; m.H = H; m.W = W; m.level = level;
    m.E = (int)l.E; m.Hh = H * (W - 1); m.K = (int)l.K; m.tpe = (int)l.tpe; m.tpk = (int)l.tpk;
    const int ntile_e = B * (int)l.tpe;
    const int* nv = l.esums + ntile_e;          // the vertex count, on the device
    const int64_t want = (l.BE + IC_THREADS - 1) / IC_THREADS;
    const dim3 vgrid((unsigned)(want < IC_MAX_GRID ? want : IC_MAX_GRID)), egrid((unsigned)l.tpe, (unsigned)B), kgrid((unsigned)l.tpk, (unsigned)B);

    P3_TRY(p3_memset(l.klen, 0, l.BK * sizeof(int), s));
    P3_TRY(p3_launch<ic_count_kernel>(nullptr, egrid, IC_THREADS, 0, s, m, l.esums));
    P3_TRY(p3_launch<ic_scan_tiles_kernel>(nullptr, 1, IC_SCAN_THREADS, 0, s, l.esums, ntile_e));
    P3_TRY(p3_launch<ic_compact_kernel>(nullptr, egrid, IC_THREADS, 0, s, m, l.esums, l.vertex_of, l.vpos, l.vsucc, l.vpred, l.vkey, l.vimg));
    P3_TRY(p3_launch<ic_link_kernel>(nullptr, vgrid, IC_THREADS, 0, s, nv, m.E, l.vertex_of, l.vimg, l.vkey, l.vsucc, l.vpred, l.st[0]));
    const int fin = l.rounds & 1;          // pass 1 ends in st[fin]
    int2* rk[2] = {(int2*)l.st[1 - fin], (int2*)l.st[1 - fin] + l.BE};
    const char* forced = getenv("P3_IC_DOUBLING");
    const bool per_image = (forced && forced[0] == 'i') || (!(forced && forced[0] == 'r') && l.E <= IC_IMAGE_MAX_EDGES);
    if (!per_image) {
        for (int k = 0; k < l.rounds; ++k) P3_TRY(p3_launch<ic_minmax_round_kernel>(nullptr, vgrid, IC_THREADS, 0, s, nv, l.st[k & 1], l.st[(k + 1) & 1]));
        P3_TRY(p3_launch<ic_rank_init_kernel>(nullptr, vgrid, IC_THREADS, 0, s, nv, l.st[fin], l.vpred, l.vkey, rk[0]));
        for (int k = 0; k < l.rounds; ++k) P3_TRY(p3_launch<ic_rank_round_kernel>("ic_rank_round_kernel", vgrid, IC_THREADS, 0, s, nv, rk[k & 1], rk[(k + 1) & 1]));
    } else {
        P3_TRY(p3_launch<ic_minmax_image_kernel>(nullptr, B, IC_IMAGE_THREADS, 0, s, l.esums, m.tpe, l.rounds, l.st[0], l.st[1]));
        P3_TRY(p3_launch<ic_rank_image_kernel>("ic_rank_image_kernel", B, IC_IMAGE_THREADS, 0, s, l.esums, m.tpe, l.rounds, l.st[fin], l.vpred, l.vkey, rk[0], rk[1]));
    }
    const int2* rank = rk[fin];          // pass 2 ends in rk[rounds & 1]
    P3_TRY(p3_launch<ic_tails_kernel>(nullptr, vgrid, IC_THREADS, 0, s, nv, m.K, l.st[fin], rank, l.vsucc, l.vimg, l.klen));
    P3_TRY(p3_launch<ic_key_reduce_kernel>(nullptr, kgrid, IC_THREADS, 0, s, m.K, m.tpk, l.klen, l.ksums, l.kmax));
    P3_TRY(p3_launch<ic_key_scan_tiles_kernel>(nullptr, 1, IC_SCAN_THREADS, 0, s, l.ksums, l.kmax, B, m.tpk, max_vertices, max_contours, counts, n_contours, n_vertices,
                                               status));
    P3_TRY(p3_launch<ic_key_place_kernel>(nullptr, kgrid, IC_THREADS, 0, s, m.K, m.tpk, l.klen, l.ksums, l.koff, l.kidx));
    return p3_launch<ic_emit_kernel>(nullptr, vgrid, IC_THREADS, 0, s, nv, m.K, l.st[fin], rank, l.vimg, l.vpos, l.klen, l.koff, l.kidx, max_vertices, max_contours,
                                     (float2*)pos, poly_slice, poly_batch, batch, is_endpoint);
}
