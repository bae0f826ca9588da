// p3hip - FFL active-skeleton initialisation from marching squares, on the device (predict/ffl/polygonize_asm.py:581-638, get_marching_squares_skeleton, behind
// p3_init_contours), and the plan p3_asm_optimize runs on.
//   p3_skeleton_from_contours   the contour container of p3_init_contours -> the TensorSkeleton fields of skeletons_to_tensorskeleton([contours_to_skeleton(c_b,
//                               min_area) for b]), with the reference's filter (at least 3 vertices, min_area < shoelace area)
//   p3_asm_plan                 path_index / path_delim -> the six arrays of polygonize_asm.AsmPlan, for any skeleton graph
//
// p3_skeleton_from_contours, three launches and one memset whatever the data:
//   1 sk_keep   one workgroup per contour: the shoelace sum in double over the fp32 positions (a lane's terms in index order, lanes by a butterfly, waves in
//               order: a fixed order, the same bits in every run) and the decision kept / dropped.  A closed contour stores n points and has n + 1 vertices.
//   2 sk_scan   one workgroup: exclusive scans (wg_scan) of kept nodes, kept paths and kept closed paths over the contours in container order: the first node,
//               the first slot (nodes + closed paths in front) and the number of every kept path; batch_delim, counts, status, the last path_delim entry.
//   3 sk_emit   one workgroup per kept contour copies its nodes and writes its path.
// Every output element has one writer, nothing is atomic, an image's rows depend on the kept counts in front of it only.
// Closedness is the container's flag (the first vertex is no endpoint), not the reference's test max|c[0] - c[-1]| < 1e-6 on skimage's points.  The two agree
// whenever no pixel equals the level: an open contour's two ends lie on different border edges, and those can only share a point at a grid vertex whose value
// is the level.
//
// p3_asm_plan.  Every path is a connected chain, so the components of the graph are unions of PATHS that share a node; the union-find runs over paths:
//   1 ap_mark        start / end flags of every slot from the interior delimiters, id check (status bit 1; a bad id is clamped before any use), sort keys
//   2 scan           path number of every slot
//   3 sort A         slots by (node, k): a node's occurrences become one run, ascending in k
//   4 ap_groups      first / one-past-last of each node's run
//   5 ap_components  ONE workgroup: neighbours in a run that lie on different paths are the links; path labels start as the path number; a round lowers both
//                    ends of every link to the smaller label and then lets every label jump to its label's label; rounds repeat until one changes nothing.
//   6 ap_node_min    the smallest node id of every component (integer minimum, independent of the order it is taken in)
//   7 sort B         nodes by (smallest id of their component, id): this IS cn_node; a node on no path is its own component
//   8 scans          component numbers, comp_ptr, cn_occ; node_local; 9 ap_slots: run A re-based to cn order gives slot_k and slot_nb.
// Termination of 5: labels are path numbers, they never rise, and every round but the last lowers at least one, so there are at most P^2 + 1 rounds; a label is
// always a path of the same component and the smallest path of a component can never change, so the state in which nothing changes - both ends of every link
// equal - is every path carrying the smallest path number of its component.  That state is unique: whatever order the integer minima land in, the labels, and
// with them every output, are the same bits.  There is no round cap.  The rounds run inside one launch, so the number of launches depends on N and M only.
// The sort is a bitonic sort of 2048-key tiles in LDS and one merge launch per doubling of the run length (each key finds its place in the partner run by
// binary search); all keys are distinct (the low word is the slot or node), so no stability question arises.
// No float arithmetic in p3_asm_plan.  Integer atomics are used only where the value does not depend on their order (minimum, maximum, or).
#include "p3_common.h"

#pragma clang fp contract(off)

typedef unsigned long long sk_u64;

#define SK_THREADS 256
#define SK_SCAN_THREADS 1024
#define SK_MAX_GRID 2048
#define SK_SORT_TILE 2048
#define SK_SCAN_ITEMS 4

// ---------------------------------------------------------------------------------------------------------------- skeleton from contours
struct SkIn {
    const float2* pos;
    const int64_t* slice;
    const int32_t* poly_batch;
    const uint8_t* is_endpoint;
    int N, P, B, filter;
    double min_area;
};

// the contour's first point and point count, clamped into the container
__device__ __forceinline__ void sk_range(const SkIn& in, int p, int& s, int& n) {
    int64_t a = in.slice[2 * (int64_t)p], b = in.slice[2 * (int64_t)p + 1];
    a = a < 0 ? 0 : (a > in.N ? in.N : a);
    b = b < a ? a : (b > in.N ? in.N : b);
    s = (int)a;
    n = (int)(b - a);
}
__device__ __forceinline__ int sk_image(const SkIn& in, int p) {
    const int b = in.poly_batch[p];
    return b < 0 ? 0 : (b >= in.B ? in.B - 1 : b);
}

// 1: grid P.  klen[p] = the contour's nodes if it is kept, else 0; kclosed[p]
__global__ __launch_bounds__(SK_THREADS) void sk_keep_kernel(SkIn in, int* klen, int* kclosed) {
    __shared__ double red[SK_THREADS / 64];
    const int p = blockIdx.x;
    int s, n;
    sk_range(in, p, s, n);
    const int closed = (n > 0 && !in.is_endpoint[s]) ? 1 : 0;
    double acc = 0.0;
    if (in.filter) {
        for (int i = threadIdx.x; i < n; i += SK_THREADS) {
            const float2 a = in.pos[s + i], b = in.pos[s + (i + 1 == n ? 0 : i + 1)];
            acc += (double)a.x * (double)b.y - (double)a.y * (double)b.x;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = red[0];
        for (int w = 1; w < SK_THREADS / 64; ++w) sum += red[w];
        bool keep = n >= 1;
        if (in.filter) keep = keep && n + closed >= 3 && in.min_area < 0.5 * fabs(sum);          // a NaN area is dropped, as the host's comparison drops it
        klen[p] = keep ? n : 0;
        kclosed[p] = closed;
    }
}

// 2: one workgroup
__global__ __launch_bounds__(SK_SCAN_THREADS) void sk_scan_kernel(SkIn in, const int* klen, const int* kclosed, int* noff, int* coff, int* kidx, int max_nodes,
                                                                  int max_slots, int max_paths, int64_t* path_delim, int64_t* batch_delim, int32_t* counts,
                                                                  int32_t* status) {
    __shared__ sk_u64 lds64[SK_SCAN_THREADS / 64];
    __shared__ int lds32[SK_SCAN_THREADS / 64];
    sk_u64 carry = 0;          // nodes << 32 | paths
    int carry_closed = 0, longest = 0;
    for (int at = 0; at < in.P; at += SK_SCAN_THREADS) {
        const int p = at + threadIdx.x;
        const int n = p < in.P ? klen[p] : 0;
        const int c = n > 0 ? kclosed[p] : 0;
        const sk_u64 ex = wg_excl(n > 0 ? p3_pack2(n, 1) : 0ull, lds64, carry);
        const int exc = wg_excl(c, lds32, carry_closed);
        if (p < in.P) {
            noff[p] = p3_hi32(ex);
            coff[p] = exc;
            kidx[p] = p3_lo32(ex);
            // batch_delim[b] = kept paths of the images in front of b: every image between the previous contour's (exclusive) and this one's (inclusive)
            const int cur = sk_image(in, p), prev = p > 0 ? sk_image(in, p - 1) : -1;
            for (int b = prev + 1; b <= cur; ++b) batch_delim[b] = p3_lo32(ex);
            longest = max(longest, n);
        }
    }
    const int longest_all = wg_max(longest, lds32);
    const int nodes = p3_hi32(carry), paths = p3_lo32(carry), slots = nodes + carry_closed;
    const int last = in.P > 0 ? sk_image(in, in.P - 1) : -1;
    for (int b = last + 1 + threadIdx.x; b <= in.B; b += SK_SCAN_THREADS) batch_delim[b] = paths;
    if (threadIdx.x == 0) {
        counts[0] = nodes; counts[1] = slots; counts[2] = paths; counts[3] = longest_all;
        status[0] = (nodes > max_nodes || slots > max_slots || paths > max_paths) ? 1 : 0;
        if (paths <= max_paths) path_delim[paths] = slots;          // path_delim has max_paths + 1 entries
    }
}

// 3: grid P
__global__ __launch_bounds__(SK_THREADS) void sk_emit_kernel(SkIn in, const int* klen, const int* kclosed, const int* noff, const int* coff, const int* kidx,
                                                             int max_nodes, int max_slots, int max_paths, float2* pos, int64_t* degrees, int64_t* path_index,
                                                             int64_t* path_delim, int64_t* batch) {
    const int p = blockIdx.x;
    const int n = klen[p];
    if (n <= 0) return;
    int s, unused;
    sk_range(in, p, s, unused);
    const int closed = kclosed[p], off = noff[p], so = off + coff[p], q = kidx[p], img = sk_image(in, p);
    for (int i = threadIdx.x; i < n; i += SK_THREADS) {
        const int at = off + i, st = so + i;
        if (at < max_nodes) {
            pos[at] = in.pos[s + i];
            degrees[at] = (!closed && (i == 0 || i == n - 1)) ? 1 : 2;
            batch[at] = img;
        }
        if (st < max_slots) path_index[st] = at;
    }
    if (threadIdx.x == 0) {
        if (closed && so + n < max_slots) path_index[so + n] = off;
        if (q < max_paths) path_delim[q] = so;
    }
}

struct SkWs { int *klen, *kclosed, *noff, *coff, *kidx; };
static SkWs sk_carve(int P, P3Carve& c) {
    const int64_t n = P > 0 ? P : 0;
    SkWs l;
    l.klen = c.take<int>(n);
    l.kclosed = c.take<int>(n);
    l.noff = c.take<int>(n);
    l.coff = c.take<int>(n);
    l.kidx = c.take<int>(n);
    return l;
}

extern "C" int64_t p3_skeleton_from_contours_workspace_bytes(int P) {
    P3Carve c = {nullptr, 0};
    sk_carve(P, c);
    return c.at;
}

extern "C" int p3_skeleton_from_contours(const float* pos, int64_t N, const int64_t* poly_slice, const int32_t* poly_batch, const uint8_t* is_endpoint, int P, int B,
                                         int filter, double min_area, int max_nodes, int max_slots, int max_paths, float* out_pos, int64_t* degrees,
                                         int64_t* path_index, int64_t* path_delim, int64_t* batch, int64_t* batch_delim, int32_t* counts, int32_t* status,
                                         void* workspace, void* stream) {
    P3_CHECK(N >= 0 && P >= 0 && B >= 1 && max_nodes >= 0 && max_slots >= 0 && max_paths >= 0, P3_ESHAPE,
             "p3_skeleton_from_contours: bad sizes (N, P >= 0; B >= 1; capacities >= 0)");
    P3_CHECK(N + (int64_t)P < ((int64_t)1 << 31) - 1, P3_ESHAPE, "p3_skeleton_from_contours: N + P must stay below 2^31 - 1");
    P3_CHECK(batch_delim && counts && status, P3_EINVAL, "p3_skeleton_from_contours: null pointer");
    P3_CHECK(min_area == min_area || !filter, P3_EINVAL, "p3_skeleton_from_contours: min_area is NaN");
    const bool empty = P == 0 || N == 0;
    P3_CHECK(empty || (pos && poly_slice && poly_batch && is_endpoint && path_delim && workspace), P3_EINVAL, "p3_skeleton_from_contours: null pointer");
    P3_CHECK(empty || ((max_nodes == 0 || (out_pos && degrees && batch)) && (max_slots == 0 || path_index)), P3_EINVAL,
             "p3_skeleton_from_contours: null output with a capacity above 0");
    hipStream_t s = (hipStream_t)stream;
    P3_TRY(p3_memset(batch_delim, 0, ((int64_t)B + 1) * sizeof(int64_t), s));
    if (empty) {
        P3_TRY(p3_memset(counts, 0, 4 * sizeof(int32_t), s));
        return p3_memset(status, 0, sizeof(int32_t), s);
    }
    SkIn in;
    in.pos = (const float2*)pos; in.slice = poly_slice; in.poly_batch = poly_batch; in.is_endpoint = is_endpoint;
    in.N = (int)N; in.P = P; in.B = B; in.filter = filter ? 1 : 0; in.min_area = min_area;
    P3Carve carve = {(char*)workspace, 0};
    const SkWs l = sk_carve(P, carve);
    P3_TRY(p3_launch<sk_keep_kernel>(nullptr, P, SK_THREADS, 0, s, in, l.klen, l.kclosed));
    P3_TRY(p3_launch<sk_scan_kernel>(nullptr, 1, SK_SCAN_THREADS, 0, s, in, l.klen, l.kclosed, l.noff, l.coff, l.kidx, max_nodes, max_slots, max_paths, path_delim,
                                     batch_delim, counts, status));
    return p3_launch<sk_emit_kernel>(nullptr, P, SK_THREADS, 0, s, in, l.klen, l.kclosed, l.noff, l.coff, l.kidx, max_nodes, max_slots, max_paths, (float2*)out_pos,
                                     degrees, path_index, path_delim, batch);
}

// ---------------------------------------------------------------------------------------------------------------- the plan
__device__ __forceinline__ int ap_in(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }          // whatever a key holds, an index stays inside its array
__device__ __forceinline__ int ap_node(const int64_t* idx, int k, int N) {          // the node of slot k, clamped into [0, N)
    const int64_t v = idx[k];
    return v < 0 ? 0 : (v >= N ? N - 1 : (int)v);
}
// a label another thread of the workgroup may lower meanwhile: read where the atomics land
__device__ __forceinline__ int ap_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// 1: startf / endf (zeroed before) and the keys of sort A.  Repeated delimiters store the same 1 twice.
__global__ __launch_bounds__(SK_THREADS) void ap_mark_kernel(const int64_t* idx, int M, const int64_t* delim, int64_t D, int N, int* startf, int* endf, sk_u64* key,
                                                             int32_t* status) {
    const int64_t span = M > D ? M : D;
    for (int64_t i = blockIdx.x * (int64_t)SK_THREADS + threadIdx.x; i < span; i += (int64_t)gridDim.x * SK_THREADS) {
        if (i < M) {
            const int64_t v = idx[i];
            if (v < 0 || v >= N) atomicOr(status, 2);
            key[i] = p3_pack2(ap_node(idx, (int)i, N), (uint32_t)i);
            if (i == 0) startf[0] = 1;
            if (i == M - 1) endf[M - 1] = 1;
        }
        if (i >= 1 && i < D - 1) {
            const int64_t cut = delim[i];
            if (cut >= 1 && cut <= (int64_t)M - 1) { startf[cut] = 1; endf[cut - 1] = 1; }
        }
    }
}

// one workgroup: dst[0 .. n) = exclusive prefix sums of src, dst[n] = the total
__global__ __launch_bounds__(SK_SCAN_THREADS) void ap_scan_kernel(const int* src, int* dst, int n) {
    __shared__ int lds[SK_SCAN_THREADS / 64];
    int carry = 0;
    for (int at = 0; at < n; at += SK_SCAN_THREADS * SK_SCAN_ITEMS) {
        const int first = at + threadIdx.x * SK_SCAN_ITEMS;
        int v[SK_SCAN_ITEMS], sum = 0;
#pragma unroll
        for (int j = 0; j < SK_SCAN_ITEMS; ++j) { v[j] = first + j < n ? src[first + j] : 0; sum += v[j]; }
        int ex = wg_excl(sum, lds, carry);
#pragma unroll
        for (int j = 0; j < SK_SCAN_ITEMS; ++j) {
            if (first + j < n) dst[first + j] = ex;
            ex += v[j];
        }
    }
    if (threadIdx.x == 0) dst[n] = carry;
}

// sort: tiles of SK_SORT_TILE keys, ascending, in LDS
__global__ __launch_bounds__(SK_SORT_TILE / 2) void ap_sort_tile_kernel(const sk_u64* src, sk_u64* dst, int n) {
    __shared__ sk_u64 sm[SK_SORT_TILE];
    const int64_t base = (int64_t)blockIdx.x * SK_SORT_TILE;
    for (int i = threadIdx.x; i < SK_SORT_TILE; i += SK_SORT_TILE / 2) sm[i] = base + i < n ? src[base + i] : ~0ull;
    for (int k = 2; k <= SK_SORT_TILE; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int i = threadIdx.x; i < SK_SORT_TILE; i += SK_SORT_TILE / 2) {
                const int o = i ^ j;
                if (o > i) {
                    const sk_u64 a = sm[i], b = sm[o];
                    if ((a > b) == ((i & k) == 0)) { sm[i] = b; sm[o] = a; }
                }
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SK_SORT_TILE; i += SK_SORT_TILE / 2)
        if (base + i < n) dst[base + i] = sm[i];
}
// sort: sorted runs of `run` keys are merged in pairs; all keys differ, so a key's place is its index in its own run plus the keys below it in the partner run
__global__ __launch_bounds__(SK_THREADS) void ap_merge_kernel(const sk_u64* src, sk_u64* dst, int n, int64_t run) {
    for (int64_t g = blockIdx.x * (int64_t)SK_THREADS + threadIdx.x; g < n; g += (int64_t)gridDim.x * SK_THREADS) {
        const int64_t r = g / run, rs = r * run, ps = (r ^ 1) * run;
        const sk_u64 key = src[g];
        int64_t lo = ps < n ? ps : n, hi = ps + run < n ? ps + run : n;
        if (lo > hi) lo = hi;
        const int64_t first = lo;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (src[mid] < key) lo = mid + 1; else hi = mid;
        }
        dst[(rs < ps ? rs : ps) + (g - rs) + (lo - first)] = key;
    }
}
// sorts n keys; they start in a, b is as large; *sorted: where they end up
static int ap_sort(sk_u64* a, sk_u64* b, int n, hipStream_t s, const sk_u64** sorted) {
    *sorted = a;
    if (n <= 0) return P3_OK;
    P3_TRY(p3_launch<ap_sort_tile_kernel>(nullptr, p3_ceil_div(n, SK_SORT_TILE), SK_SORT_TILE / 2, 0, s, a, b, n));
    sk_u64 *src = b, *dst = a;
    const int grid = p3_ceil_div(n, SK_THREADS) < SK_MAX_GRID ? p3_ceil_div(n, SK_THREADS) : SK_MAX_GRID;
    for (int64_t run = SK_SORT_TILE; run < n; run <<= 1) {
        P3_TRY(p3_launch<ap_merge_kernel>(nullptr, grid, SK_THREADS, 0, s, src, dst, n, run));
        sk_u64* t = src; src = dst; dst = t;
    }
    *sorted = src;
    return P3_OK;
}

// 4: gstart (-1 before) / gend per node from run A
__global__ __launch_bounds__(SK_THREADS) void ap_groups_kernel(const sk_u64* sa, int M, int N, int* gstart, int* gend) {
    for (int j = blockIdx.x * SK_THREADS + threadIdx.x; j < M; j += gridDim.x * SK_THREADS) {
        const int v = ap_in(p3_hi32(sa[j]), N);
        if (j == 0 || p3_hi32(sa[j - 1]) != v) gstart[v] = j;
        if (j == M - 1 || p3_hi32(sa[j + 1]) != v) gend[v] = j + 1;
    }
}

__device__ __forceinline__ int ap_path(const int* pid_ex, const int* startf, int k) { return pid_ex[k] + startf[k] - 1; }          // startf[0] = 1: never negative

// 5: one workgroup (the header comment has the termination argument)
__global__ __launch_bounds__(SK_SCAN_THREADS) void ap_components_kernel(const sk_u64* sa, int M, const int* pid_ex, const int* startf, int* plab, int2* links) {
    __shared__ int lds[SK_SCAN_THREADS / 64];
    const int paths = pid_ex[M];
    for (int p = threadIdx.x; p < paths; p += SK_SCAN_THREADS) plab[p] = p;
    int nlinks = 0;
    for (int at = 0; at < M; at += SK_SCAN_THREADS) {
        const int j = at + threadIdx.x;
        int a = 0, b = 0, flag = 0;
        if (j >= 1 && j < M && p3_hi32(sa[j]) == p3_hi32(sa[j - 1])) {
            a = ap_in(ap_path(pid_ex, startf, ap_in(p3_lo32(sa[j - 1]), M)), paths);
            b = ap_in(ap_path(pid_ex, startf, ap_in(p3_lo32(sa[j]), M)), paths);
            flag = a != b ? 1 : 0;
        }
        const int ex = wg_excl(flag, lds, nlinks);
        if (flag) links[ex] = make_int2(a, b);
    }
    __syncthreads();
    for (;;) {
        int changed = 0;
        for (int l = threadIdx.x; l < nlinks; l += SK_SCAN_THREADS) {
            const int2 e = links[l];
            const int la = ap_load(plab + e.x), lb = ap_load(plab + e.y);
            if (la < lb) { atomicMin(plab + e.y, la); changed = 1; }
            else if (lb < la) { atomicMin(plab + e.x, lb); changed = 1; }
        }
        __syncthreads();
        for (int p = threadIdx.x; p < paths; p += SK_SCAN_THREADS) {
            const int l = ap_load(plab + p);
            const int ll = ap_load(plab + l);
            if (ll < l) { atomicMin(plab + p, ll); changed = 1; }
        }
        if (!__syncthreads_or(changed)) break;
    }
}

// 6: pmin (INT_MAX-like before) [paths]: the smallest node id of the component whose label is the path
__global__ __launch_bounds__(SK_THREADS) void ap_node_min_kernel(const sk_u64* sa, int N, int M, const int* gstart, const int* pid_ex, const int* startf, const int* plab, int* pmin) {
    for (int v = blockIdx.x * SK_THREADS + threadIdx.x; v < N; v += gridDim.x * SK_THREADS) {
        const int j = gstart[v];
        if (j >= 0 && j < M) atomicMin(pmin + ap_in(plab[ap_in(ap_path(pid_ex, startf, ap_in(p3_lo32(sa[j]), M)), M)], M), v);
    }
}
// keys of sort B
__global__ __launch_bounds__(SK_THREADS) void ap_node_key_kernel(const sk_u64* sa, int N, int M, const int* gstart, const int* pid_ex, const int* startf, const int* plab,
                                                                 const int* pmin, sk_u64* key) {
    for (int v = blockIdx.x * SK_THREADS + threadIdx.x; v < N; v += gridDim.x * SK_THREADS) {
        const int j = gstart[v];
        const int cmin = (j >= 0 && j < M) ? pmin[ap_in(plab[ap_in(ap_path(pid_ex, startf, ap_in(p3_lo32(sa[j]), M)), M)], M)] : v;
        key[v] = p3_pack2(cmin, v);
    }
}
// 8a: cn_node, its inverse, the first-of-component flags and the occurrence counts in cn order
__global__ __launch_bounds__(SK_THREADS) void ap_cn_kernel(const sk_u64* sb, int N, const int* gstart, const int* gend, int32_t* cn_node, int* cn_pos, int* first, int* occs) {
    for (int i = blockIdx.x * SK_THREADS + threadIdx.x; i < N; i += gridDim.x * SK_THREADS) {
        const int v = ap_in(p3_lo32(sb[i]), N);
        cn_node[i] = v;
        cn_pos[v] = i;
        first[i] = (i == 0 || p3_hi32(sb[i - 1]) != p3_hi32(sb[i])) ? 1 : 0;
        occs[i] = gstart[v] >= 0 ? gend[v] - gstart[v] : 0;
    }
}
// 8b: comp_ptr
__global__ __launch_bounds__(SK_THREADS) void ap_comp_ptr_kernel(int N, const int* first, const int* comp_ex, int32_t* comp_ptr, int32_t* counts) {
    for (int i = blockIdx.x * SK_THREADS + threadIdx.x; i < N; i += gridDim.x * SK_THREADS) {
        if (first[i]) comp_ptr[comp_ex[i]] = i;
        if (i == 0) { comp_ptr[comp_ex[N]] = N; counts[0] = comp_ex[N]; }
    }
}
// 8c: node_local; the largest component (counts[1], zero before)
__global__ __launch_bounds__(SK_THREADS) void ap_node_local_kernel(int N, const int* first, const int* comp_ex, const int32_t* comp_ptr, const int32_t* cn_node,
                                                                   int32_t* node_local, int32_t* counts) {
    for (int i = blockIdx.x * SK_THREADS + threadIdx.x; i < N; i += gridDim.x * SK_THREADS) {
        const int c = comp_ex[i] + first[i] - 1;          // first[0] = 1: never negative
        node_local[ap_in(cn_node[i], N)] = i - comp_ptr[c];
        if (first[i]) atomicMax(counts + 1, comp_ptr[c + 1] - comp_ptr[c]);
    }
}
// 9: every slot of run A to its place in cn order
__global__ __launch_bounds__(SK_THREADS) void ap_slots_kernel(const sk_u64* sa, int M, int N, const int64_t* idx, const int* gstart, const int* cn_pos, const int32_t* cn_occ,
                                                              const int* startf, const int* endf, const int32_t* node_local, int32_t* slot_k, int32_t* slot_nb) {
    for (int j = blockIdx.x * SK_THREADS + threadIdx.x; j < M; j += gridDim.x * SK_THREADS) {
        const int v = ap_in(p3_hi32(sa[j]), N), k = ap_in(p3_lo32(sa[j]), M);
        const int64_t t = (int64_t)cn_occ[ap_in(cn_pos[v], N)] + (j - gstart[v]);
        if (t < 0 || t >= M) continue;          // cannot happen: the runs partition the slots
        slot_k[t] = k;
        slot_nb[2 * t] = (startf[k] || k == 0) ? -1 : node_local[ap_node(idx, k - 1, N)];          // startf[0] = 1 and endf[M-1] = 1
        slot_nb[2 * t + 1] = (endf[k] || k == M - 1) ? -1 : node_local[ap_node(idx, k + 1, N)];
    }
}

struct ApWs {
    int *startf, *endf, *pid_ex;
    sk_u64 *keya, *keya2;
    int *gstart, *gend, *plab, *pmin;
    int2* links;
    sk_u64 *keyb, *keyb2;
    int *cn_pos, *first, *comp_ex, *occs;
};
static ApWs ap_carve(int64_t N, int64_t M, P3Carve& c) {
    ApWs l;
    if (N < 0) N = 0;
    if (M < 0) M = 0;
    l.startf = c.take<int>(M);
    l.endf = c.take<int>(M);
    l.pid_ex = c.take<int>(M + 1);
    l.keya = c.take<sk_u64>(M);
    l.keya2 = c.take<sk_u64>(M);
    l.gstart = c.take<int>(N);
    l.gend = c.take<int>(N);
    l.plab = c.take<int>(M);
    l.pmin = c.take<int>(M);
    l.links = c.take<int2>(M);
    l.keyb = c.take<sk_u64>(N);
    l.keyb2 = c.take<sk_u64>(N);
    l.cn_pos = c.take<int>(N);
    l.first = c.take<int>(N);
    l.comp_ex = c.take<int>(N + 1);
    l.occs = c.take<int>(N);
    return l;
}

extern "C" int64_t p3_asm_plan_workspace_bytes(int64_t N, int64_t M) {
    P3Carve c = {nullptr, 0};
    ap_carve(N, M, c);
    return c.at;
}

extern "C" int p3_asm_plan(const int64_t* path_index, int64_t M, const int64_t* path_delim, int64_t D, int64_t N, int32_t* comp_ptr, int32_t* cn_node, int32_t* cn_occ,
                           int32_t* slot_nb, int32_t* node_local, int32_t* slot_k, int32_t* counts, int32_t* status, void* workspace, void* stream) {
    P3_CHECK(N >= 0 && M >= 0 && D >= 0, P3_ESHAPE, "p3_asm_plan: bad sizes (N, M, D >= 0)");
    P3_CHECK(N < ((int64_t)1 << 31) - 1 && M < ((int64_t)1 << 31) - 1, P3_ESHAPE, "p3_asm_plan: N and M must stay below 2^31 - 1");
    P3_CHECK(comp_ptr && cn_occ && counts && status, P3_EINVAL, "p3_asm_plan: null pointer");
    P3_CHECK((M == 0 || (path_index && slot_nb && slot_k)) && (N == 0 || (cn_node && node_local)) && (D == 0 || path_delim), P3_EINVAL, "p3_asm_plan: null pointer");
    P3_CHECK(N == 0 || workspace, P3_EINVAL, "p3_asm_plan: null workspace (p3_asm_plan_workspace_bytes(N, M))");
    hipStream_t s = (hipStream_t)stream;
    P3_TRY(p3_memset(counts, 0, 2 * sizeof(int32_t), s));
    P3_TRY(p3_memset(status, 0, sizeof(int32_t), s));
    if (N == 0) {          // no node: every id there is lies outside [0, 0)
        P3_TRY(p3_memset(comp_ptr, 0, sizeof(int32_t), s));
        P3_TRY(p3_memset(cn_occ, 0, sizeof(int32_t), s));
        return M > 0 ? p3_hip_status(hipMemsetD32Async((hipDeviceptr_t)status, 2, 1, s)) : P3_OK;
    }
    P3Carve carve = {(char*)workspace, 0};
    const ApWs l = ap_carve(N, M, carve);
    const int n = (int)N, m = (int)M;
    const int64_t span = M > D ? M : D;
    const auto grid_of = [](int64_t items) { const int64_t g = (items + SK_THREADS - 1) / SK_THREADS; return (unsigned)(g < 1 ? 1 : (g < SK_MAX_GRID ? g : SK_MAX_GRID)); };
    const unsigned ngrid = grid_of(N), mgrid = grid_of(M);
    P3_TRY(p3_memset(l.gstart, 0xff, N * sizeof(int), s));
    const sk_u64* sa = l.keya;
    if (M > 0) {
        P3_TRY(p3_memset(l.startf, 0, M * sizeof(int), s));
        P3_TRY(p3_memset(l.endf, 0, M * sizeof(int), s));
        P3_TRY(p3_memset(l.pmin, 0x7f, M * sizeof(int), s));
        P3_TRY(p3_launch<ap_mark_kernel>(nullptr, grid_of(span), SK_THREADS, 0, s, path_index, m, path_delim, D, n, l.startf, l.endf, l.keya, status));
        P3_TRY(p3_launch<ap_scan_kernel>(nullptr, 1, SK_SCAN_THREADS, 0, s, l.startf, l.pid_ex, m));
        P3_TRY(ap_sort(l.keya, l.keya2, m, s, &sa));
        P3_TRY(p3_launch<ap_groups_kernel>(nullptr, mgrid, SK_THREADS, 0, s, sa, m, n, l.gstart, l.gend));
        P3_TRY(p3_launch<ap_components_kernel>(nullptr, 1, SK_SCAN_THREADS, 0, s, sa, m, l.pid_ex, l.startf, l.plab, l.links));
        P3_TRY(p3_launch<ap_node_min_kernel>(nullptr, ngrid, SK_THREADS, 0, s, sa, n, m, l.gstart, l.pid_ex, l.startf, l.plab, l.pmin));
    }
    P3_TRY(p3_launch<ap_node_key_kernel>(nullptr, ngrid, SK_THREADS, 0, s, sa, n, m, l.gstart, l.pid_ex, l.startf, l.plab, l.pmin, l.keyb));
    const sk_u64* sb;
    P3_TRY(ap_sort(l.keyb, l.keyb2, n, s, &sb));
    P3_TRY(p3_launch<ap_cn_kernel>(nullptr, ngrid, SK_THREADS, 0, s, sb, n, l.gstart, l.gend, cn_node, l.cn_pos, l.first, l.occs));
    P3_TRY(p3_launch<ap_scan_kernel>(nullptr, 1, SK_SCAN_THREADS, 0, s, l.first, l.comp_ex, n));
    P3_TRY(p3_launch<ap_scan_kernel>(nullptr, 1, SK_SCAN_THREADS, 0, s, l.occs, cn_occ, n));
    P3_TRY(p3_launch<ap_comp_ptr_kernel>(nullptr, ngrid, SK_THREADS, 0, s, n, l.first, l.comp_ex, comp_ptr, counts));
    P3_TRY(p3_launch<ap_node_local_kernel>(nullptr, ngrid, SK_THREADS, 0, s, n, l.first, l.comp_ex, comp_ptr, cn_node, node_local, counts));
    if (M > 0)
        P3_TRY(p3_launch<ap_slots_kernel>(nullptr, mgrid, SK_THREADS, 0, s, sa, m, n, path_index, l.gstart, l.cn_pos, cn_occ, l.startf, l.endf, node_local, slot_k,
                                          slot_nb));
    return P3_OK;
}
