// p3hip - FFL active-skeleton (ASM) optimiser (predict/ffl/polygonize_asm.py:133-421: AlignLoss + TensorSkeletonOptimizer, torch_lydorn tensorskeleton.py).
//   p3_asm_optimize   `steps` RMSprop iterations on every skeleton node with the analytic gradient of the reference's total_loss (:353: level, length and
//                     align; its curvature, corner and junction terms never enter the loss that is differentiated), no autograd graph.
//   p3_asm_schedule   host only: (data, length, crossfield, lr) of one iteration from the functions the kernel uses.
//
// Nodes interact only through shared paths, so the unit of work is a connected component of the skeleton graph (an isolated node is one of its own):
//   fast path  asm_lds_kernel: ONE launch for all steps, one workgroup per component.  The component's positions ping-pong between two halves of one LDS
//              array with one barrier per step; the maps are gathered from global memory as in acm.hip.  Gradients are owner-computed: a thread owns nodes, and
//              for each it walks the node's occurrences in path_index in ascending order, evaluating the incoming edge, the outgoing edge and the length term
//              of each.  Every edge is therefore evaluated by both of its ends, which is what saves the second barrier (and any atomic) an edge pass would need.
//              The RMSprop state `sq` is touched by the owning thread alone.
//   fallback   asm_global_kernel: components over ASM_LDS_CAP nodes (or all, when forced) ping-pong between `pos` and a workspace copy, one launch per step.
// Both call asm_node(), compiled with floating-point contraction off: the two paths give the same bits, and so do two runs and any split of the steps into
// calls (first_iter, sq).  No atomics, no host synchronisation.  The sampling of the two maps (pixel clamp, level term, align term of an edge) and the
// fixed-order sum of the loss terms are shared with acm.hip: ffl_field.h, which turns contraction off for itself.
//
// The plan (built once per skeleton by the host wrapper from path_index / path_delim) lists the nodes component by component ("cn order"):
//   comp_ptr [C+1]   component c holds cn entries comp_ptr[c] .. comp_ptr[c+1]
//   cn_node  [CN]    node id of a cn entry;  the entry's index inside its component is its "local" index
//   cn_occ   [CN+1]  the entry's occurrences in path_index are the slots cn_occ[i] .. cn_occ[i+1], ascending in k
//   slot_nb  [S,2]   per slot: local index of the node at k - 1 (-1 at a path start) and at k + 1 (-1 at a path end)
// Every index read from it is clamped, so no malformed plan can address outside pos, sq, the maps or the LDS buffers.
#include "p3_common.h"
#include "ffl_field.h"

#pragma clang fp contract(off)

#define ASM_THREADS 256
#define ASM_EPS 1e-6f             // z = e / (|e| + 1e-6) (polygonize_asm.py:182-201)
#define ASM_LDS_CAP 4096          // nodes: 2 buffers x 8 B x 4096 = 64 KiB, the most a workgroup gets without opting in to more dynamic LDS
#define ASM_MAX_KNOTS 8
static_assert(ASM_THREADS % 64 == 0, "whole waves");

struct AsmFields {
    const float* indicator;       // [B,H,W]
    const float* c0c2;            // [B,4,H,W]
    int B, H, W;
    float level;
};
struct AsmSched { int nk; double x[ASM_MAX_KNOTS], data[ASM_MAX_KNOTS], length[ASM_MAX_KNOTS], cross[ASM_MAX_KNOTS]; double lr, gamma; };
struct AsmCoefs { float wd, wl, wc, lr; };
struct AsmPlan {
    const int32_t* comp_ptr; const int32_t* cn_node; const int32_t* cn_occ; const int32_t* slot_nb;
    int C; int64_t CN, S;
    const uint8_t* is_tip; const int32_t* node_batch;
};
struct AsmNode { float r, c, sq_r, sq_c, g_r, g_c, align, level, length; };          // new position and state, the gradient, and the loss terms this node counts

// scipy.interpolate.interp1d(kind="linear") at x = it (polygonize_asm.py:151-156, 342-344), all in double: slope = (y_hi - y_lo) / (x_hi - x_lo), then
// slope * (it - x_lo) + y_lo.  For 1-d float tables scipy hands this to numpy.interp, whose segment has x_lo <= it < x_hi: at a knot the result is that knot's
// value exactly (interp1d's own searchsorted form takes the segment below and lands one ulp beside it), and so it is here.  Beyond the last knot, where
// the reference would raise, the last segment is extended.  The arrays are indexed by constants only (the schedule is a kernel argument: a run-time
// index would move it to scratch).
__host__ __device__ __forceinline__ double asm_interp(const double* x, const double* y, int nk, int it) {
    double xlo = x[0], xhi = x[1], ylo = y[0], yhi = y[1];
#pragma unroll
    for (int j = 1; j < ASM_MAX_KNOTS - 1; ++j)
        if (j < nk - 1 && x[j] <= (double)it) { xlo = x[j]; xhi = x[j + 1]; ylo = y[j]; yhi = y[j + 1]; }
    if ((double)it == xhi) return yhi;          // the last knot: every other one is the lower end of its segment
    const double slope = (yhi - ylo) / (xhi - xlo);
    return slope * ((double)it - xlo) + ylo;
}
// ExponentialLR(gamma) chains lr <- lr * gamma once per step (polygonize_asm.py:381, 411-412)
__host__ __device__ __forceinline__ double asm_lr(const AsmSched& s, int it) {
    double lr = s.lr;
    for (int i = 0; i < it; ++i) lr = lr * s.gamma;
    return lr;
}
__host__ __device__ __forceinline__ AsmCoefs asm_coefs(const AsmSched& s, int it, double lr) {
    AsmCoefs c;
    c.wd = (float)asm_interp(s.x, s.data, s.nk, it);
    c.wl = (float)asm_interp(s.x, s.length, s.nk, it);
    c.wc = (float)asm_interp(s.x, s.cross, s.nk, it);
    c.lr = (float)lr;
    return c;
}

// One RMSprop step of one node.  The only place the ASM's loss is put together, from the level and align terms of ffl_field.h: both kernels call it.
// `at(local)` is the position of the component's node `local` before the step; the node's occurrences are the slots s0 .. s1 (already clamped to the slot
// array), nb0 = asm_first_slot() the neighbours of the first of them (most nodes have one occurrence: the one-launch kernel keeps it in registers across
// the steps), n the nodes of its component.
template <class At>
__device__ __forceinline__ AsmNode asm_node(const AsmFields& f, const AsmCoefs& co, int img, bool tip, float2 cur, float2 sq, const int32_t* slot_nb, int64_t s0,
                                            int64_t s1, int2 nb0, int n, At at) {
    AsmNode o;
    const int64_t hw = (int64_t)f.H * f.W;
    const float* ind = f.indicator + (int64_t)img * hw;
    const float* cf = f.c0c2 + (int64_t)img * 4 * hw;
    const FflLevel lv = ffl_level(ind, f.H, f.W, f.level, cur);
    o.level = lv.dv * lv.dv;
    const float gI = co.wd * (2.f * lv.dv);
    float g_r = gI * lv.dIdy, g_c = gI * lv.dIdx;
    o.align = 0.f; o.length = 0.f;
    // the node's occurrences k in path_index, ascending: + the incoming edge's gradient (the node is its head), - the outgoing edge's (its tail), + the
    // length term's (both neighbours detached, :219-235), always in this order
    for (int64_t s = s0; s < s1; ++s) {
        const int lp = s == s0 ? nb0.x : slot_nb[2 * s], ln = s == s0 ? nb0.y : slot_nb[2 * s + 1];
        const bool has_p = lp >= 0, has_n = ln >= 0;
        float2 prev = cur, next = cur;
        if (has_p) {
            prev = at(min(lp, n - 1));
            const FflEdge e = ffl_edge(cf, f.H, f.W, ASM_EPS, prev, cur);
            g_r += co.wc * (e.mask * e.ge0); g_c += co.wc * (e.mask * e.ge1);
        }
        if (has_n) {
            next = at(min(ln, n - 1));
            const FflEdge e = ffl_edge(cf, f.H, f.W, ASM_EPS, cur, next);
            g_r -= co.wc * (e.mask * e.ge0); g_c -= co.wc * (e.mask * e.ge1);
            o.align += e.align;                                // an edge is counted once, by its tail
        }
        if (has_p && has_n) {
            const float p0 = cur.x - prev.x, p1 = cur.y - prev.y, n0 = next.x - cur.x, n1 = next.y - cur.y;
            g_r += co.wl * (2.f * p0 - 2.f * n0); g_c += co.wl * (2.f * p1 - 2.f * n1);
            o.length += (p0 * p0 + p1 * p1) + (n0 * n0 + n1 * n1);
        }
    }
    o.g_r = g_r; o.g_c = g_c;
    // torch.optim.RMSprop(alpha=0.9), eps 1e-8, no momentum, not centred (:380); a tip (degree 1) is put back after the step (:406-409), its state still updated
    o.sq_r = 0.9f * sq.x + 0.1f * (g_r * g_r);
    o.sq_c = 0.9f * sq.y + 0.1f * (g_c * g_c);
    o.r = tip ? cur.x : fmaf(-co.lr, g_r / (sqrtf(o.sq_r) + 1e-8f), cur.x);
    o.c = tip ? cur.y : fmaf(-co.lr, g_c / (sqrtf(o.sq_c) + 1e-8f), cur.y);
    return o;
}

// component c's clamped cn range
__device__ __forceinline__ void asm_comp(const AsmPlan& pl, int c, int64_t& start, int& n) {
    const int64_t s = min(max((int64_t)pl.comp_ptr[c], (int64_t)0), pl.CN), e = min(max((int64_t)pl.comp_ptr[c + 1], s), pl.CN);
    start = s;
    n = (int)(e - s);
}
// cn entry i: its node (clamped to pos), image, tip flag and clamped slot range
__device__ __forceinline__ void asm_entry(const AsmPlan& pl, int64_t i, int64_t N, int B, int& node, int& img, bool& tip, int64_t& s0, int64_t& s1) {
    node = (int)min(max((int64_t)pl.cn_node[i], (int64_t)0), N - 1);
    img = min(max(pl.node_batch[node], 0), B - 1);
    tip = pl.is_tip[node] != 0;
    s0 = min(max((int64_t)pl.cn_occ[i], (int64_t)0), pl.S);
    s1 = min(max((int64_t)pl.cn_occ[i + 1], s0), pl.S);
}

__device__ __forceinline__ int2 asm_first_slot(const AsmPlan& pl, int64_t s0, int64_t s1) {
    return s1 > s0 ? make_int2(pl.slot_nb[2 * s0], pl.slot_nb[2 * s0 + 1]) : make_int2(-1, -1);
}

// fast path.  Dynamic LDS: 2 * lds_len float2 (>= 64 B).  Components larger than lds_len are left to the fallback.
__global__ __launch_bounds__(ASM_THREADS) void asm_lds_kernel(float2* pos, float2* sqv, int64_t N, AsmPlan pl, AsmFields f, AsmSched sched, int first_iter, int steps,
                                                              int lds_len, float2* grad_out, float* comp_losses) {
    extern __shared__ __attribute__((aligned(16))) float2 asm_sm[];
    const int c = blockIdx.x, tid = threadIdx.x;
    int64_t start;
    int n;
    asm_comp(pl, c, start, n);
    if (n > lds_len) return;                                   // uniform over the workgroup
    for (int v = tid; v < n; v += ASM_THREADS) asm_sm[v] = pos[min(max((int64_t)pl.cn_node[start + v], (int64_t)0), N - 1)];
    __syncthreads();
    float s_al = 0.f, s_lv = 0.f, s_ln = 0.f;
    double lr = asm_lr(sched, first_iter);
    // this thread's first node (in a component of at most ASM_THREADS nodes its only one): what the plan says about it, read once.  Behind the barrier
    // of every step these would be three dependent global loads in front of the LDS read
    int node0 = 0, img0 = 0;
    bool tip0 = false;
    int64_t s00 = 0, s10 = 0;
    int2 nb00 = make_int2(-1, -1);
    if (tid < n) {
        asm_entry(pl, start + tid, N, f.B, node0, img0, tip0, s00, s10);
        nb00 = asm_first_slot(pl, s00, s10);
    }
    for (int k = 0; k < steps; ++k) {
        const int src = (k & 1) ? n : 0, dst = n - src;        // offsets into the one shared array, not pointers picked from an array: the accesses stay ds_
        const AsmCoefs co = asm_coefs(sched, first_iter + k, lr);
        lr = lr * sched.gamma;
        const bool last = k == steps - 1;
        for (int v = tid; v < n; v += ASM_THREADS) {
            int node = node0, img = img0;
            bool tip = tip0;
            int64_t s0 = s00, s1 = s10;
            int2 nb0 = nb00;
            if (v != tid) {
                asm_entry(pl, start + v, N, f.B, node, img, tip, s0, s1);
                nb0 = asm_first_slot(pl, s0, s1);
            }
            const AsmNode o = asm_node(f, co, img, tip, asm_sm[src + v], sqv[node], pl.slot_nb, s0, s1, nb0, n, [&](int i) { return asm_sm[src + i]; });
            asm_sm[dst + v] = make_float2(o.r, o.c);
            sqv[node] = make_float2(o.sq_r, o.sq_c);          // read and written by this thread alone
            if (last) {
                if (grad_out) grad_out[node] = make_float2(o.g_r, o.g_c);
                s_al += o.align; s_lv += o.level; s_ln += o.length;
            }
        }
        __syncthreads();          // the only barrier of the step: step k + 1 overwrites the half step k read, and every read of it lies before this
    }
    const int fin = (steps & 1) ? n : 0;
    for (int v = tid; v < n; v += ASM_THREADS) pos[min(max((int64_t)pl.cn_node[start + v], (int64_t)0), N - 1)] = asm_sm[fin + v];
    if (comp_losses) {
        __syncthreads();          // the position buffers are free now: their head holds the wave partials
        ffl_reduce3<ASM_THREADS>(s_al, s_lv, s_ln, (float*)asm_sm, comp_losses + 3 * (int64_t)c);
    }
}

// fallback, one launch per step: blockIdx.x = component, blockIdx.y = chunk of ASM_THREADS cn entries; src -> dst are `pos` and its workspace copy in turn.
// As in acm.hip the grid is C x ceil(largest / ASM_THREADS) and all workgroups but those of the large components return at once.
__global__ __launch_bounds__(ASM_THREADS) void asm_global_kernel(const float2* src, float2* dst, float2* sqv, int64_t N, AsmPlan pl, AsmFields f, AsmCoefs co,
                                                                 int lds_len, int force, float2* grad_out, float* node_losses) {
    int64_t start;
    int n;
    asm_comp(pl, blockIdx.x, start, n);
    if (!force && n <= lds_len) return;
    const int v = blockIdx.y * ASM_THREADS + threadIdx.x;
    if (v >= n) return;
    int node, img;
    bool tip;
    int64_t s0, s1;
    asm_entry(pl, start + v, N, f.B, node, img, tip, s0, s1);
    const AsmNode o = asm_node(f, co, img, tip, src[node], sqv[node], pl.slot_nb, s0, s1, asm_first_slot(pl, s0, s1), n,
                               [&](int i) { return src[min(max((int64_t)pl.cn_node[start + i], (int64_t)0), N - 1)]; });
    dst[node] = make_float2(o.r, o.c);
    sqv[node] = make_float2(o.sq_r, o.sq_c);
    if (grad_out) grad_out[node] = make_float2(o.g_r, o.g_c);
    if (node_losses) {
        float* w = node_losses + 3 * (start + v);
        w[0] = o.align; w[1] = o.level; w[2] = o.length;
    }
}

// fallback epilogue, one workgroup per component: copy the result home after an odd number of steps, and reduce the per-node loss terms in the fast path's order
__global__ __launch_bounds__(ASM_THREADS) void asm_global_finish_kernel(const float2* ws, float2* pos, int64_t N, AsmPlan pl, int lds_len, int force, int copy_home,
                                                                        const float* node_losses, float* comp_losses) {
    __shared__ float red[3 * (ASM_THREADS / 64)];
    int64_t start;
    int n;
    asm_comp(pl, blockIdx.x, start, n);
    if (!force && n <= lds_len) return;
    float s_al = 0.f, s_lv = 0.f, s_ln = 0.f;
    for (int v = threadIdx.x; v < n; v += ASM_THREADS) {
        if (copy_home) {
            const int64_t node = min(max((int64_t)pl.cn_node[start + v], (int64_t)0), N - 1);
            pos[node] = ws[node];
        }
        if (comp_losses) {
            const float* w = node_losses + 3 * (start + v);
            s_al += w[0]; s_lv += w[1]; s_ln += w[2];
        }
    }
    if (comp_losses) ffl_reduce3<ASM_THREADS>(s_al, s_lv, s_ln, red, comp_losses + 3 * (int64_t)blockIdx.x);
}

static bool asm_fill_sched(AsmSched& sc, const double* knots, int nk, double lr, double gamma) {
    if (!knots || nk < 2 || nk > ASM_MAX_KNOTS) return false;
    sc.nk = nk;
    for (int i = 0; i < ASM_MAX_KNOTS; ++i) {
        const int j = i < nk ? i : nk - 1;
        sc.x[i] = knots[j]; sc.data[i] = knots[nk + j]; sc.length[i] = knots[2 * nk + j]; sc.cross[i] = knots[3 * nk + j];
    }
    for (int i = 1; i < nk; ++i)
        if (!(sc.x[i] > sc.x[i - 1])) return false;
    sc.lr = lr; sc.gamma = gamma;
    return true;
}

// knots: double [4, nk] = step_thresholds, data, length, crossfield of loss_params.coefs.  out: (data, length, crossfield, lr) of iteration `iter` as the
// floats the kernel uses, widened to double
extern "C" int p3_asm_schedule(int iter, const double* knots, int nk, double lr, double gamma, double* out) {
    AsmSched sc;
    P3_CHECK(out && iter >= 0, P3_EINVAL, "p3_asm_schedule: null output or negative iteration");
    P3_CHECK(asm_fill_sched(sc, knots, nk, lr, gamma), P3_ESHAPE, "p3_asm_schedule: 2 .. 8 knots with increasing step_thresholds expected");
    const AsmCoefs co = asm_coefs(sc, iter, asm_lr(sc, iter));
    out[0] = co.wd; out[1] = co.wl; out[2] = co.wc; out[3] = co.lr;
    return P3_OK;
}

// workspace of the fallback: a copy of pos, and the per-node loss terms in cn order
extern "C" int64_t p3_asm_workspace_bytes(int64_t N, int64_t CN) {
    return N > 0 && CN >= 0 ? N * (int64_t)sizeof(float2) + CN * (int64_t)(3 * sizeof(float)) : 0;
}

extern "C" int p3_asm_optimize(float* pos, float* sq, int64_t N, const int32_t* comp_ptr, int C, const int32_t* cn_node, const int32_t* cn_occ, int64_t CN,
                               const int32_t* slot_nb, int64_t S, const uint8_t* is_tip, const int32_t* node_batch, const float* indicator, const float* c0c2,
                               int B, int H, int W, float data_level, const double* knots, int nk, double lr, double gamma, int first_iter, int steps,
                               int max_comp, int force_fallback, float* grad_out, float* comp_losses, void* workspace, void* stream) {
    P3_CHECK(C >= 0 && N >= 0 && N < ((int64_t)1 << 31) && CN >= 0 && CN < ((int64_t)1 << 31) && S >= 0 && S < ((int64_t)1 << 30) && steps >= 0 && first_iter >= 0,
             P3_ESHAPE, "p3_asm_optimize: bad sizes (0 <= N, CN < 2^31, 0 <= S < 2^30, C, steps, first_iter >= 0)");
    if (C == 0 || steps == 0 || N == 0 || CN == 0) return P3_OK;
    P3_CHECK(pos && sq && comp_ptr && cn_node && cn_occ && (slot_nb || S == 0) && is_tip && node_batch && indicator && c0c2, P3_EINVAL,
             "p3_asm_optimize: null pointer");
    P3_CHECK(B > 0 && H > 0 && W > 0, P3_ESHAPE, "p3_asm_optimize: bad map sizes");
    AsmSched sc;
    P3_CHECK(asm_fill_sched(sc, knots, nk, lr, gamma), P3_ESHAPE, "p3_asm_optimize: 2 .. 8 knots with increasing step_thresholds expected");
    const int64_t largest = max_comp > 0 ? (int64_t)max_comp : CN;               // no bound from the caller: one component may hold every node
    const bool fast = !force_fallback;
    const bool slow = force_fallback || largest > ASM_LDS_CAP;
    P3_CHECK(!slow || workspace, P3_EINVAL, "p3_asm_optimize: null workspace (components over the LDS cap, or the forced fallback, need p3_asm_workspace_bytes)");
    const int64_t chunks = (largest + ASM_THREADS - 1) / ASM_THREADS;
    P3_CHECK(!slow || chunks <= 65535, P3_ESHAPE, "p3_asm_optimize: a component of more than 65535 * 256 nodes");
    hipStream_t s = (hipStream_t)stream;
    AsmFields f;
    f.indicator = indicator; f.c0c2 = c0c2; f.B = B; f.H = H; f.W = W; f.level = data_level;
    AsmPlan pl;
    pl.comp_ptr = comp_ptr; pl.cn_node = cn_node; pl.cn_occ = cn_occ; pl.slot_nb = slot_nb; pl.C = C; pl.CN = CN; pl.S = S; pl.is_tip = is_tip;
    pl.node_batch = node_batch;
    const int lds_len = fast ? (int)(largest < ASM_LDS_CAP ? largest : ASM_LDS_CAP) : 0;
    if (fast) {
        size_t lds = (size_t)lds_len * 2 * sizeof(float2);
        if (lds < 64) lds = 64;
        P3_TRY(p3_launch<asm_lds_kernel>("asm_lds_kernel", C, ASM_THREADS, lds, s, (float2*)pos, (float2*)sq, N, pl, f, sc, first_iter, steps, lds_len, (float2*)grad_out,
                                         comp_losses));
    }
    if (slow) {
        float2* ws = (float2*)workspace;
        float* nloss = comp_losses ? (float*)(ws + N) : nullptr;
        double lr_k = asm_lr(sc, first_iter);
        for (int k = 0; k < steps; ++k) {
            const float2* src = (k & 1) ? ws : (const float2*)pos;
            float2* dst = (k & 1) ? (float2*)pos : ws;
            const AsmCoefs co = asm_coefs(sc, first_iter + k, lr_k);
            lr_k = lr_k * sc.gamma;
            const bool last = k == steps - 1;
            P3_TRY(p3_launch<asm_global_kernel>("asm_global_kernel", dim3(C, (unsigned)chunks), ASM_THREADS, 0, s, src, dst, (float2*)sq, N, pl, f, co, lds_len,
                                                force_fallback, last ? (float2*)grad_out : nullptr, last ? nloss : nullptr));
        }
        if ((steps & 1) || comp_losses)
            P3_TRY(p3_launch<asm_global_finish_kernel>(nullptr, C, ASM_THREADS, 0, s, ws, (float2*)pos, N, pl, lds_len, force_fallback, steps & 1, nloss, comp_losses));
    }
    return P3_OK;
}
