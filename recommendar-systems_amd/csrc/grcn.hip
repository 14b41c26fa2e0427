// grcn.hip — GRCN's learned-graph pieces on gfx950, forward and backward.  Reference:
// src/models/grcn.py (MM'20), restated in tests/grcn_ref.py.
//
// The graph is the user-item graph as a CSR by TARGET row (col = source), symmetric in
// structure, with rev[e] the slot of the reversed edge (rsx.grcn.target_csr).  Its VALUES are
// learned every step:
//
//  * attn_fwd: per row t the scores <x_t, x_s> of its in-edges, their softmax alpha (the row
//    max subtracted: x is general, not only unit rows) and rep_t = x_t + sum alpha x_s.
//    PyG's softmax adds 1e-16 to the denominator; the denominator here is a sum of exp(s - max)
//    that contains exp(0) = 1, so 1e-16 is far below its float32 rounding and is dropped.
//  * refine_fwd: w_e = relu(max_m alpha_m[e] conf[source(e), m]) into val[e] and valT[rev[e]]
//    (A_w and A_w^T share rowptr and col; both id-GCN products and their transposes run on
//    rsx_spmm over those two value arrays).
//  * edge_dots (SDDMM): dw_e = <G_t, h1_s> + <D_t, x_s>, one lane group an edge.
//  * refine_bwd: the winner recomputed by the forward's own arithmetic; a wave a SOURCE row,
//    its edges reached through rev, so dconf[s, :] has one writer.
//  * attn_bwd: the row-local part (da, the row's sum, ds, dx_t) and the gather through rev
//    (dx_s += ds_e x_t + alpha_e g_t), two launches.
//  * the loss on the three representation tables side by side (a wave a triplet: lane l the
//    columns 4 l .. 4 l + 3 of [id_rep | rep_v | rep_t], at most 256 wide) and `result`:
//    rsx_triplet.hpp's protocol at width 256 (one-score triplet, block partials, keys, walk,
//    workspace); its own: the concatenated row, the regularisers and their count gradients.
//
// Row kernels: a row is a lane group of d / 4 float4 lanes.  A row of more than kHubDegree
// in-edges is walked by its whole block instead: lane group g takes the edges g, g + RPB, ...
// with its own running state, the RPB states are merged in lane-group order.  Per-edge scalars
// that need the row's total (the score, da) are parked in the output array by the lane that
// later rewrites them.  No float atomics, every order fixed: two runs are bit-equal.
//
// kHubDegree is a tuning value nobody has measured: four SpMM chunks (the schedule's default
// chunk is 32), so that each of the 8 or 16 lane groups of a hub row's block still gets at
// least 8 edges to amortise the merge.
#include <cmath>

#include "rsx_triplet.hpp"

namespace rsx {
namespace grcn {

constexpr int kHubDegree = 128;

struct Graph {
    const int64_t* rowptr;
    const int32_t* col;
    const int32_t* rev;
    int64_t n, nnz;
};

__device__ __forceinline__ bool in_range(int32_t i, int64_t n) { return (uint32_t)i < (uint64_t)n; }

// ---------------------------------------------------------------------------
// the row kernel: light rows a lane group each, hub rows the whole block
// ---------------------------------------------------------------------------
// Task: State (clear / put / merge on a SLOT-float LDS slot), begin (the row's constants),
// load (an in-edge's operands) and edge (that edge into the state), finish (the row's outputs
// from the merged state; the lane group's own edges are first, first + stride, ...; `writer`:
// this lane group writes the row).
//
// A lane group's edges, in order; the operands of four edges are loaded before the first is
// consumed (a gather's latency is the walk's cost), the states take them in the same order.
template <class Task>
__device__ __forceinline__ void walk(const Task& task, typename Task::State& st, const Graph& gr, int64_t first,
                                     int64_t end, int64_t stride, int c) {
    int64_t j = first;
    for (; j + 3 * stride < end; j += 4 * stride) {
        const typename Task::Pre p0 = task.load(gr, j, c), p1 = task.load(gr, j + stride, c),
                                 p2 = task.load(gr, j + 2 * stride, c), p3 = task.load(gr, j + 3 * stride, c);
        task.edge(st, p0, j, c);
        task.edge(st, p1, j + stride, c);
        task.edge(st, p2, j + 2 * stride, c);
        task.edge(st, p3, j + 3 * stride, c);
    }
    for (; j < end; j += stride) task.edge(st, task.load(gr, j, c), j, c);
}

template <int D, class Task>
__global__ __launch_bounds__(256) void row_kernel(Task task, Graph gr) {
    constexpr int L = D / 4, RPB = 256 / L, SLOT = Task::kSlot;
    __shared__ __attribute__((aligned(16))) float sh[RPB * SLOT];
    const int grp = threadIdx.x / L, c = (threadIdx.x % L) * 4;
    const int64_t row0 = (int64_t)blockIdx.x * RPB;
    {
        const int64_t row = row0 + grp;
        if (row < gr.n) {  // uniform over the row's lane group, as every branch below
            const int64_t b = gr.rowptr[row], e = gr.rowptr[row + 1];
            if (e - b <= kHubDegree) {
                typename Task::State st;
                task.begin(st, row, c);
                st.clear();
                walk(task, st, gr, b, e, 1, c);
                task.finish(st, row, b, e, 1, true, c);
            }
        }
    }
#pragma unroll 1
    for (int r = 0; r < RPB; ++r) {  // block-uniform
        const int64_t row = row0 + r;
        if (row >= gr.n) break;
        const int64_t b = gr.rowptr[row], e = gr.rowptr[row + 1];
        if (e - b <= kHubDegree) continue;
        typename Task::State st;
        task.begin(st, row, c);
        st.clear();
        walk(task, st, gr, b + grp, e, RPB, c);
        st.put(sh + grp * SLOT, c);
        __syncthreads();
        st.clear();
        for (int g = 0; g < RPB; ++g) st.merge(sh + g * SLOT, c);  // lane-group order
        __syncthreads();  // the slots are free for the block's next hub row
        task.finish(st, row, b + grp, e, RPB, grp == 0, c);
    }
}

// attention forward: the running softmax (max m, sum l of exp(s - m), acc = sum exp(s - m) x_s)
template <int D>
struct AttnFwd {
    static constexpr int L = D / 4, kSlot = D + 4;
    const float* x;
    float* alpha;
    float* rep;
    struct State {
        float4 xt, acc;
        float m, l;
        __device__ __forceinline__ void clear() { acc = f4(0.f), m = -INFINITY, l = 0.f; }
        __device__ __forceinline__ void add(float s, float4 xs) {
            const float mn = fmaxf(m, s);
            const float sc = expf(m - mn), p = expf(s - mn);  // (m = -inf: sc = 0)
            l = l * sc + p;
            acc = fma4(p, xs, mul4(sc, acc));
            m = mn;
        }
        __device__ __forceinline__ void put(float* slot, int c) const {
            st4(slot + c, acc);
            if (c == 0) slot[D] = m, slot[D + 1] = l;
        }
        __device__ __forceinline__ void merge(const float* slot, int c) {
            const float om = slot[D], ol = slot[D + 1];
            if (!(ol > 0.f)) return;  // an empty share
            const float mn = fmaxf(m, om);
            const float sa = expf(m - mn), sb = expf(om - mn);
            l = l * sa + ol * sb;
            acc = fma4(sb, ld4(slot + c), mul4(sa, acc));
            m = mn;
        }
    };
    __device__ __forceinline__ void begin(State& st, int64_t row, int c) const { st.xt = ld4(x + row * D + c); }
    struct Pre {
        bool ok;
        float4 xs;
    };
    __device__ __forceinline__ Pre load(const Graph& gr, int64_t j, int c) const {
        const int32_t cj = gr.col[j];
        Pre p;
        p.ok = in_range(cj, gr.n);
        p.xs = p.ok ? ld4(x + (int64_t)cj * D + c) : f4(0.f);
        return p;
    }
    __device__ __forceinline__ void edge(State& st, const Pre& p, int64_t j, int c) const {
        if (!p.ok) {  // not an edge of this graph: alpha 0
            if (c == 0) alpha[j] = -INFINITY;
            return;
        }
        const float s = group_sum<L>(dot4(st.xt, p.xs));
        if (c == 0) alpha[j] = s;  // parked: finish rewrites it from the same lane
        st.add(s, p.xs);
    }
    __device__ __forceinline__ void finish(State& st, int64_t row, int64_t first, int64_t end, int stride, bool writer,
                                           int c) const {
        const bool any = st.l > 0.f;
        if (writer) st4(rep + row * D + c, any ? fma4(1.f / st.l, st.acc, st.xt) : st.xt);
        if (c == 0)
            for (int64_t j = first; j < end; j += stride) alpha[j] = any ? expf(alpha[j] - st.m) / st.l : 0.f;
    }
};

// attention backward, row-local: da_e = <g_t, x_s> + dext_e, dot = sum alpha da,
// ds_e = alpha_e (da_e - dot), dx_t = g_t + sum ds_e x_s = g_t + sum alpha da x_s - dot sum alpha x_s
template <int D>
struct AttnBwdRow {
    static constexpr int L = D / 4, kSlot = 2 * D + 4;
    const float *g, *x, *alpha, *dext;
    float *ds, *dx;
    struct State {
        float4 gt, a1, a2;
        float dot;
        __device__ __forceinline__ void clear() { a1 = a2 = f4(0.f), dot = 0.f; }
        __device__ __forceinline__ void put(float* slot, int c) const {
            st4(slot + c, a1);
            st4(slot + D + c, a2);
            if (c == 0) slot[2 * D] = dot;
        }
        __device__ __forceinline__ void merge(const float* slot, int c) {
            a1 = add4(a1, ld4(slot + c));
            a2 = add4(a2, ld4(slot + D + c));
            dot += slot[2 * D];
        }
    };
    __device__ __forceinline__ void begin(State& st, int64_t row, int c) const { st.gt = ld4(g + row * D + c); }
    struct Pre {
        bool ok;
        float4 xs;
        float a, de;
    };
    __device__ __forceinline__ Pre load(const Graph& gr, int64_t j, int c) const {
        const int32_t cj = gr.col[j];
        Pre p;
        p.ok = in_range(cj, gr.n);
        p.xs = p.ok ? ld4(x + (int64_t)cj * D + c) : f4(0.f);
        p.a = alpha[j];
        p.de = dext ? dext[j] : 0.f;
        return p;
    }
    __device__ __forceinline__ void edge(State& st, const Pre& p, int64_t j, int c) const {
        if (!p.ok) {
            if (c == 0) ds[j] = 0.f;
            return;
        }
        const float da = group_sum<L>(dot4(st.gt, p.xs)) + p.de;
        if (c == 0) ds[j] = da;  // parked
        st.a1 = fma4(p.a * da, p.xs, st.a1);
        st.a2 = fma4(p.a, p.xs, st.a2);
        st.dot = fmaf(p.a, da, st.dot);
    }
    __device__ __forceinline__ void finish(State& st, int64_t row, int64_t first, int64_t end, int stride, bool writer,
                                           int c) const {
        if (writer) st4(dx + row * D + c, add4(st.gt, fma4(-st.dot, st.a2, st.a1)));
        if (c == 0)
            for (int64_t j = first; j < end; j += stride) ds[j] = alpha[j] * (ds[j] - st.dot);
    }
};

// attention backward, the gather: row s as a SOURCE; slot j of row s is the edge s <- t = col[j],
// its reverse e = rev[j] the edge t <- s:  dx_s += ds_e x_t + alpha_e g_t
template <int D>
struct AttnBwdGather {
    static constexpr int L = D / 4, kSlot = D + 4;
    const float *g, *x, *alpha, *ds;
    float* dx;
    struct State {
        float4 acc;
        __device__ __forceinline__ void clear() { acc = f4(0.f); }
        __device__ __forceinline__ void put(float* slot, int c) const { st4(slot + c, acc); }
        __device__ __forceinline__ void merge(const float* slot, int c) { acc = add4(acc, ld4(slot + c)); }
    };
    __device__ __forceinline__ void begin(State&, int64_t, int) const {}
    struct Pre {
        float4 xt, gt;
        float dse, ae;
    };
    __device__ __forceinline__ Pre load(const Graph& gr, int64_t j, int c) const {
        const int32_t t = gr.col[j], e = gr.rev[j];
        Pre p;
        if (!in_range(t, gr.n) || !in_range(e, gr.nnz)) {  // not an edge of this graph: nothing to add
            p.xt = p.gt = f4(0.f), p.dse = p.ae = 0.f;
            return p;
        }
        p.xt = ld4(x + (int64_t)t * D + c), p.gt = ld4(g + (int64_t)t * D + c);
        p.dse = ds[e], p.ae = alpha[e];
        return p;
    }
    __device__ __forceinline__ void edge(State& st, const Pre& p, int64_t, int) const {
        st.acc = fma4(p.dse, p.xt, st.acc);
        st.acc = fma4(p.ae, p.gt, st.acc);
    }
    __device__ __forceinline__ void finish(State& st, int64_t row, int64_t, int64_t, int, bool writer, int c) const {
        if (writer) st4(dx + row * D + c, add4(ld4(dx + row * D + c), st.acc));
    }
};

// ---------------------------------------------------------------------------
// the refined edge weight
// ---------------------------------------------------------------------------
// The product of modality m on an edge and the winner: modality 1 wins only when strictly
// larger.  refine_fwd and refine_bwd both call this, so they agree on every edge.
__device__ __forceinline__ float winner(int M, float a0, float a1, const float* __restrict__ cs, int& win) {
    float p = a0 * cs[0];
    win = 0;
    if (M == 2) {
        const float p1 = a1 * cs[1];
        if (p1 > p) p = p1, win = 1;
    }
    return p;
}

__global__ __launch_bounds__(256) void refine_fwd(Graph gr, int M, const float* __restrict__ alpha0,
                                                  const float* __restrict__ alpha1, const float* __restrict__ conf,
                                                  float* __restrict__ val, float* __restrict__ valT) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= gr.nnz) return;
    const int32_t s = gr.col[e], re = gr.rev[e];
    float w = 0.f;
    if (in_range(s, gr.n)) {
        int win;
        w = fmaxf(winner(M, alpha0[e], M == 2 ? alpha1[e] : 0.f, conf + (int64_t)s * M, win), 0.f);
    }
    val[e] = w;
    if (in_range(re, gr.nnz)) valT[re] = w;
}

// dw_e = <G_t, h1_s> + <D_t, x_s>, t = row(e) = col[rev[e]], s = col[e]: a lane group an edge
template <int D>
__global__ __launch_bounds__(256) void edge_dots(Graph gr, const float* __restrict__ G, const float* __restrict__ h1,
                                                 const float* __restrict__ Dm, const float* __restrict__ x,
                                                 float* __restrict__ dw) {
    constexpr int L = D / 4, RPB = 256 / L;
    const int c = (threadIdx.x % L) * 4;
    const int64_t e = (int64_t)blockIdx.x * RPB + threadIdx.x / L;
    if (e >= gr.nnz) return;  // uniform over the lane group
    const int32_t s = gr.col[e], re = gr.rev[e];
    float p = 0.f;
    if (in_range(s, gr.n) && in_range(re, gr.nnz)) {
        const int32_t t = gr.col[re];
        if (in_range(t, gr.n)) {
            p = dot4(ld4(G + (int64_t)t * D + c), ld4(h1 + (int64_t)s * D + c)) +
                dot4(ld4(Dm + (int64_t)t * D + c), ld4(x + (int64_t)s * D + c));
            p = group_sum<L>(p);
        }
    }
    if (c == 0) dw[e] = p;
}

// A wave a source row s: lane l takes the slots b + l, b + l + 64, ... of row s, each the
// reverse of an edge e whose source is s.  dalpha_m[e] has one writer (rev is a permutation),
// dconf[s, :] is the wave's fixed tree over the lanes' sums.
__global__ __launch_bounds__(256) void refine_bwd(Graph gr, int M, const float* __restrict__ alpha0,
                                                  const float* __restrict__ alpha1, const float* __restrict__ conf,
                                                  const float* __restrict__ dw, float* __restrict__ dalpha0,
                                                  float* __restrict__ dalpha1, float* __restrict__ dconf) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // wave-uniform
    if (s >= gr.n) return;
    const int64_t b = gr.rowptr[s], en = gr.rowptr[s + 1];
    const float* cs = conf + s * M;
    float acc0 = 0.f, acc1 = 0.f;
    for (int64_t j = b + lane; j < en; j += kWave) {
        const int32_t e = gr.rev[j];
        if (!in_range(e, gr.nnz)) continue;
        const float a0 = alpha0[e], a1 = M == 2 ? alpha1[e] : 0.f;
        int win;
        const bool live = winner(M, a0, a1, cs, win) > 0.f;
        const float d = dw[e];
        dalpha0[e] = live && win == 0 ? d * cs[0] : 0.f;
        if (M == 2) dalpha1[e] = live && win == 1 ? d * cs[1] : 0.f;
        if (live && win == 0) acc0 = fmaf(d, a0, acc0);
        if (live && win == 1) acc1 = fmaf(d, a1, acc1);
    }
    acc0 = group_sum<kWave>(acc0);
    acc1 = group_sum<kWave>(acc1);
    if (lane == 0) {
        dconf[s * M] = acc0;
        if (M == 2) dconf[s * M + 1] = acc1;
    }
}

// ---------------------------------------------------------------------------
// the loss (grcn.py:300-333) on [id_rep | rep_v | rep_t], and `result`
// ---------------------------------------------------------------------------
constexpr int kTerms = 4, kSqBlocks = 256;

struct LossArgs {
    const float *id, *rv, *rt, *E, *pv, *pt;
    const int64_t* trip;
    int64_t nu, ni, B;
    int dx, dc, W;
    float reg_weight;
};

// the float4 at column col of a row of the concatenated representation (zero past its width)
__device__ __forceinline__ float4 rep4(const LossArgs& a, int64_t row, int col) {
    if (col < a.dx) return ld4(a.id + row * a.dx + col);
    col -= a.dx;
    if (col < a.dc) return ld4(a.rv + row * a.dc + col);
    col -= a.dc;
    if (a.rt && col < a.dc) return ld4(a.rt + row * a.dc + col);
    return f4(0.f);
}

__device__ __forceinline__ void load_trip(const LossArgs& a, int64_t b, int c, ScoreTrip& t) {
    load_score_trip<256>(
        a.trip, a.B, b, a.nu, a.ni, c, [&](int64_t u, int c) { return rep4(a, u, c); },
        [&](int64_t i, int c) { return rep4(a, a.nu + i, c); }, t);
}

// part[block] = sums over the block's four triplets of {softplus(-x), 2 |E_u|^2 + |E_p|^2 + |E_n|^2,
// |pref_v[u]|^2, |pref_t[u]|^2}
__global__ __launch_bounds__(256) void loss_rows(LossArgs a, float* __restrict__ part) {
    const RowGeom<256> r;  // a wave a triplet
    float v[kTerms] = {0.f, 0.f, 0.f, 0.f};
    if (r.b < a.B) {  // wave-uniform
        ScoreTrip t;
        load_trip(a, r.b, r.c, t);
        v[0] = softplus_neg(t.x);
        if (t.ok) {
            float e = 0.f, p0 = 0.f, p1 = 0.f;
            if (r.c < a.dx) {
                const float4 eu = ld4(a.E + t.u * a.dx + r.c), ep = ld4(a.E + (a.nu + t.p) * a.dx + r.c),
                             en = ld4(a.E + (a.nu + t.n) * a.dx + r.c);
                e = 2.f * dot4(eu, eu) + dot4(ep, ep) + dot4(en, en);  // users.repeat_interleave(2)
            }
            if (r.c < a.dc) {
                const float4 q = ld4(a.pv + t.u * a.dc + r.c);
                p0 = dot4(q, q);
                if (a.pt) {
                    const float4 q1 = ld4(a.pt + t.u * a.dc + r.c);
                    p1 = dot4(q1, q1);
                }
            }
            v[1] = group_sum<kWave>(e);
            v[2] = group_sum<kWave>(p0);
            v[3] = group_sum<kWave>(p1);
        }
    }
    block_partials<256, kTerms, kTerms>(r, v, part);
}

// partw[block] = the block's share of sum pref_v^2: block b the float4s b, b + kSqBlocks, ... in
// runs of 256; a thread's terms in index order, the block's 256 sums in a fixed tree
__global__ __launch_bounds__(256) void sq_partials(const float* __restrict__ p, int64_t n4, float* __restrict__ partw) {
    __shared__ float sh[4];
    float acc = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)kSqBlocks * 256) {
        const float4 v = ld4(p + 4 * i);
        acc += dot4(v, v);
    }
    acc = group_sum<kWave>(acc);
    if ((threadIdx.x & (kWave - 1)) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partw[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__global__ __launch_bounds__(64) void loss_finish(LossArgs a, const float* __restrict__ part, int nblk,
                                                  const float* __restrict__ partw, float* __restrict__ out) {
    float term[kTerms], whole[1];
    sum_partials<kTerms, kTerms>(part, nblk, term);
    sum_partials<1, 1>(partw, kSqBlocks, whole);
    if (threadIdx.x == 0) {
        const float B = (float)a.B;
        const float bpr = term[0] / B;
        float reg = term[1] / (2.f * B * (float)a.dx);
        reg += whole[0] / ((float)a.nu * (float)a.dc) + term[2] / (B * (float)a.dc);
        if (a.pt) reg += term[3] / (B * (float)a.dc);
        reg *= a.reg_weight;
        out[0] = bpr + reg;
        out[1] = bpr;
        out[2] = reg;
    }
}

// result[row, 0 : W] = [id_rep | rep_v | rep_t] at leading dimension ld (the columns past W stay)
__global__ __launch_bounds__(256) void write_result(LossArgs a, int64_t ld, float* __restrict__ out) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t n = a.nu + a.ni;
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < n; row += (int64_t)gridDim.x * 4)
        if (4 * lane < a.W) st4(out + row * ld + 4 * lane, rep4(a, row, 4 * lane));
}

// Per triplet b: coef[b] = d total / d x_b (upstream included), occU[b] = coef (rep_p - rep_n)
// (the user row's share), occR[b] = rep_u (what an item occurrence scales by +-coef), the keys.
__global__ __launch_bounds__(256) void loss_grad_rows(LossArgs a, const float* __restrict__ go,
                                                      float* __restrict__ occU, float* __restrict__ occR,
                                                      float* __restrict__ coef, int32_t* __restrict__ ku,
                                                      int32_t* __restrict__ ki) {
    const RowGeom<256> r;
    const int64_t b = r.b;
    if (b >= a.B) return;  // wave-uniform
    ScoreTrip t;
    load_trip(a, b, r.c, t);
    const float ck = bpr_coef(t, go, a.B);
    if (r.c < a.W) {
        st4(occU + b * a.W + r.c, mul4(ck, sub4(t.pr, t.nr)));
        st4(occR + b * a.W + r.c, t.ur);
    }
    if (r.c == 0) {
        coef[b] = ck;
        store_keys(t, a.B, b, ku, ki);
    }
}

struct LossGrads {
    float *g_id, *g_v, *g_t, *gE, *gpv, *gpt;
};

// gpv = the whole-table term's gradient on every row (the batch's users are rewritten after)
__global__ __launch_bounds__(256) void pref_whole_grad(LossArgs a, const float* __restrict__ go, float* __restrict__ gpv) {
    const int64_t n4 = a.nu * a.dc / 4;
    const float k = *go * a.reg_weight * 2.f / ((float)a.nu * (float)a.dc);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256)
        st4(gpv + 4 * i, mul4(k, ld4(a.pv + 4 * i)));
}

// The per-destination sums (rsx_triplet.hpp's walk, one lane group a wave).  The leader of a row
// also counts the row's occurrences: the regularisers' gradients are count times the row.
__global__ __launch_bounds__(256) void loss_sum_rows(LossArgs a, const float* __restrict__ go,
                                                     const float* __restrict__ occU, const float* __restrict__ occR,
                                                     const float* __restrict__ coef, const int32_t* __restrict__ ku,
                                                     const int32_t* __restrict__ ki, LossGrads G) {
    Walk<256> w;
    if (!w.begin(ku, ki, a.B)) return;
    const int c = w.c;
    const int64_t B = a.B;
    const bool user = w.user;
    float4 acc = f4(0.f);
    float cnt = 0.f;
    const bool mine_cols = c < a.W;
    w.each(
        [&](int64_t occ) {
            cnt += 1.f;
            if (mine_cols) acc = add4(acc, ld4(occU + occ * a.W + c));
        },
        [&](int64_t b, float sgn) {
            cnt += 1.f;
            if (mine_cols) acc = fma4(sgn * coef[b], ld4(occR + b * a.W + c), acc);
        });
    const int64_t row = user ? (int64_t)w.key : a.nu + w.key;
    int col = c;
    if (col < a.dx) {
        st4(G.g_id + row * a.dx + col, acc);
    } else if ((col -= a.dx) < a.dc) {
        st4(G.g_v + row * a.dc + col, acc);
    } else if ((col -= a.dc) < a.dc && a.rt) {
        st4(G.g_t + row * a.dc + col, acc);
    }
    const float kr = *go * a.reg_weight;
    if (c < a.dx) {  // d (2 |E_u|^2 or |E_i|^2) / (2 B dx), a term an occurrence
        const float k = kr * cnt * (user ? 4.f : 2.f) / (2.f * (float)B * (float)a.dx);
        st4(G.gE + row * a.dx + c, mul4(k, ld4(a.E + row * a.dx + c)));
    }
    if (user && c < a.dc) {
        const float kb = kr * cnt * 2.f / ((float)B * (float)a.dc);
        const float kw = kr * 2.f / ((float)a.nu * (float)a.dc);
        st4(G.gpv + row * a.dc + c, mul4(kb + kw, ld4(a.pv + row * a.dc + c)));
        if (a.pt) st4(G.gpt + row * a.dc + c, mul4(kb, ld4(a.pt + row * a.dc + c)));
    }
}

// the shared workspace for a wave a triplet and W-wide rows (occR is its extra row buffer, occX),
// then partw [kSqBlocks]
struct LossWs {
    TripletWs t;
    float* partw;
};
inline LossWs carve(void* ws, int64_t B, int W) {
    LossWs w{carve_triplet(ws, B, 256, kTerms, 1, 1, W), nullptr};
    w.partw = w.t.cv.take<float>((size_t)kSqBlocks * sizeof(float));
    return w;
}

inline bool width_ok(int d) { return d == 64 || d == 128; }

// (not check_triplet: two widths and their sum are judged before the pointers)
inline int loss_check(const rsx_grcn_loss_args* a, void* ws, size_t ws_bytes, LossArgs& k) {
    if (!a || a->batch < 1 || a->n_users < 1 || a->n_items < 1) return RSX_ERR_ARG;
    if (!width_ok(a->dx) || !width_ok(a->dc)) return RSX_ERR_UNSUPPORTED;
    const int W = a->dx + (a->rep_t ? 2 : 1) * a->dc;
    if (W > 256) return RSX_ERR_UNSUPPORTED;
    if (!a->id_rep || !a->rep_v || !a->E || !a->pref_v || !a->triplets || !ws) return RSX_ERR_ARG;
    if ((a->rep_t == nullptr) != (a->pref_t == nullptr)) return RSX_ERR_ARG;
    for (const void* p : {(const void*)a->id_rep, (const void*)a->rep_v, (const void*)a->rep_t, (const void*)a->E,
                          (const void*)a->pref_v, (const void*)a->pref_t, (const void*)ws})
        if (!aligned16(p)) return RSX_ERR_ARG;
    if (a->batch > kMaxBatch || a->n_users + a->n_items > 0x7fffffffll) return RSX_ERR_UNSUPPORTED;
    if (ws_bytes < rsx_grcn_loss_ws_bytes(a->batch, W)) return RSX_ERR_WORKSPACE;
    k.id = a->id_rep, k.rv = a->rep_v, k.rt = a->rep_t, k.E = a->E, k.pv = a->pref_v, k.pt = a->pref_t;
    k.trip = a->triplets;
    k.nu = a->n_users, k.ni = a->n_items, k.B = a->batch;
    k.dx = a->dx, k.dc = a->dc, k.W = W, k.reg_weight = a->reg_weight;
    return RSX_OK;
}

inline unsigned capped(int64_t nb, int64_t cap) { return (unsigned)(nb < 1 ? 1 : nb < cap ? nb : cap); }

inline int graph_check(const int64_t* rowptr, const int32_t* col, const int32_t* rev, int64_t n, int64_t nnz,
                       Graph& g) {
    if (n < 0 || nnz < 0 || !rowptr || (nnz > 0 && (!col || !rev))) return RSX_ERR_ARG;
    if (n > 0x7fffffffll || nnz > 0x7fffffffll) return RSX_ERR_UNSUPPORTED;  // int32 col / rev
    g.rowptr = rowptr, g.col = col, g.rev = rev, g.n = n, g.nnz = nnz;
    return RSX_OK;
}

template <int D, class Task>
int launch_rows(const Task& t, const Graph& g, hipStream_t s) {
    constexpr int RPB = 256 / (D / 4);
    hipLaunchKernelGGL((row_kernel<D, Task>), dim3((unsigned)((g.n + RPB - 1) / RPB)), dim3(256), 0, s, t, g);
    return last_rc();
}

}  // namespace grcn
}  // namespace rsx

using namespace rsx;

extern "C" {

int32_t rsx_grcn_hub_degree(void) { return grcn::kHubDegree; }

int rsx_grcn_attn_fwd(const float* x, const int64_t* rowptr, const int32_t* col, int64_t n, int64_t nnz, int32_t d,
                      float* alpha, float* rep, rsx_stream_t stream) {
    grcn::Graph g;
    const int rc = grcn::graph_check(rowptr, col, col, n, nnz, g);
    if (rc) return rc;
    if (!x || !rep || (nnz > 0 && !alpha) || !aligned16(x) || !aligned16(rep)) return RSX_ERR_ARG;
    if (!grcn::width_ok(d)) return RSX_ERR_UNSUPPORTED;
    if (n == 0) return RSX_OK;
    hipStream_t s = as_stream(stream);
    if (d == 64) return grcn::launch_rows<64>(grcn::AttnFwd<64>{x, alpha, rep}, g, s);
    return grcn::launch_rows<128>(grcn::AttnFwd<128>{x, alpha, rep}, g, s);
}

int rsx_grcn_attn_bwd(const float* g_rep, const float* dalpha_ext, const float* x, const float* alpha,
                      const int64_t* rowptr, const int32_t* col, const int32_t* rev, int64_t n, int64_t nnz, int32_t d,
                      float* ds, float* dx, rsx_stream_t stream) {
    grcn::Graph g;
    const int rc = grcn::graph_check(rowptr, col, rev, n, nnz, g);
    if (rc) return rc;
    if (!g_rep || !x || !dx || (nnz > 0 && (!alpha || !ds)) || !aligned16(g_rep) || !aligned16(x) || !aligned16(dx))
        return RSX_ERR_ARG;
    if (!grcn::width_ok(d)) return RSX_ERR_UNSUPPORTED;
    if (n == 0) return RSX_OK;
    hipStream_t s = as_stream(stream);
    int r;
    if (d == 64) {
        if ((r = grcn::launch_rows<64>(grcn::AttnBwdRow<64>{g_rep, x, alpha, dalpha_ext, ds, dx}, g, s))) return r;
        return grcn::launch_rows<64>(grcn::AttnBwdGather<64>{g_rep, x, alpha, ds, dx}, g, s);
    }
    if ((r = grcn::launch_rows<128>(grcn::AttnBwdRow<128>{g_rep, x, alpha, dalpha_ext, ds, dx}, g, s))) return r;
    return grcn::launch_rows<128>(grcn::AttnBwdGather<128>{g_rep, x, alpha, ds, dx}, g, s);
}

int rsx_grcn_refine_fwd(int32_t n_mod, const float* alpha0, const float* alpha1, const float* conf,
                        const int32_t* col, const int32_t* rev, int64_t n, int64_t nnz, float* val, float* valT,
                        rsx_stream_t stream) {
    if (n_mod != 1 && n_mod != 2) return RSX_ERR_UNSUPPORTED;
    if (n < 0 || nnz < 0 || !conf || (nnz > 0 && (!alpha0 || (n_mod == 2 && !alpha1) || !col || !rev || !val || !valT)))
        return RSX_ERR_ARG;
    if (n > 0x7fffffffll || nnz > 0x7fffffffll) return RSX_ERR_UNSUPPORTED;
    if (nnz == 0) return RSX_OK;
    const grcn::Graph g{nullptr, col, rev, n, nnz};
    hipLaunchKernelGGL(grcn::refine_fwd, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, as_stream(stream), g,
                       (int)n_mod, alpha0, alpha1, conf, val, valT);
    return last_rc();
}

int rsx_grcn_edge_dots(const float* G, const float* h1, const float* D, const float* x, const int32_t* col,
                       const int32_t* rev, int64_t n, int64_t nnz, int32_t d, float* dw, rsx_stream_t stream) {
    if (n < 0 || nnz < 0 || !G || !h1 || !D || !x || (nnz > 0 && (!col || !rev || !dw))) return RSX_ERR_ARG;
    if (!aligned16(G) || !aligned16(h1) || !aligned16(D) || !aligned16(x)) return RSX_ERR_ARG;
    if (!grcn::width_ok(d) || n > 0x7fffffffll || nnz > 0x7fffffffll) return RSX_ERR_UNSUPPORTED;
    if (nnz == 0) return RSX_OK;
    const grcn::Graph g{nullptr, col, rev, n, nnz};
    const int rpb = 256 / (d / 4);
    const dim3 grid((unsigned)((nnz + rpb - 1) / rpb));
    if (d == 64) hipLaunchKernelGGL(grcn::edge_dots<64>, grid, dim3(256), 0, as_stream(stream), g, G, h1, D, x, dw);
    else hipLaunchKernelGGL(grcn::edge_dots<128>, grid, dim3(256), 0, as_stream(stream), g, G, h1, D, x, dw);
    return last_rc();
}

int rsx_grcn_refine_bwd(int32_t n_mod, const float* alpha0, const float* alpha1, const float* conf, const float* dw,
                        const int64_t* rowptr, const int32_t* rev, int64_t n, int64_t nnz, float* dalpha0,
                        float* dalpha1, float* dconf, rsx_stream_t stream) {
    if (n_mod != 1 && n_mod != 2) return RSX_ERR_UNSUPPORTED;
    if (n < 0 || nnz < 0 || !conf || !dconf || !rowptr) return RSX_ERR_ARG;
    if (nnz > 0 && (!alpha0 || !dw || !rev || !dalpha0 || (n_mod == 2 && (!alpha1 || !dalpha1)))) return RSX_ERR_ARG;
    if (n > 0x7fffffffll || nnz > 0x7fffffffll) return RSX_ERR_UNSUPPORTED;
    if (n == 0) return RSX_OK;
    const grcn::Graph g{rowptr, nullptr, rev, n, nnz};
    hipLaunchKernelGGL(grcn::refine_bwd, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, as_stream(stream), g, (int)n_mod,
                       alpha0, alpha1, conf, dw, dalpha0, dalpha1, dconf);
    return last_rc();
}

size_t rsx_grcn_loss_ws_bytes(int64_t batch, int32_t width) {
    if (batch < 1 || batch > kMaxBatch || width < 128 || width > 256 || width % 64) return 0;
    return grcn::carve(nullptr, batch, width).t.cv.total();
}

int rsx_grcn_loss_fwd(const rsx_grcn_loss_args* a, float* out, float* result, int64_t ld, void* ws, size_t ws_bytes,
                      rsx_stream_t stream) {
    grcn::LossArgs k;
    const int rc = grcn::loss_check(a, ws, ws_bytes, k);
    if (rc) return rc;
    if (!out || !aligned16(result) || (result && (ld < k.W || ld % 4))) return RSX_ERR_ARG;
    hipStream_t s = as_stream(stream);
    const grcn::LossWs w = grcn::carve(ws, k.B, k.W);
    const int nblk = rows_blocks<256>(k.B);
    hipLaunchKernelGGL(grcn::loss_rows, dim3(nblk), dim3(256), 0, s, k, w.t.part);
    hipLaunchKernelGGL(grcn::sq_partials, dim3(grcn::kSqBlocks), dim3(256), 0, s, k.pv, k.nu * k.dc / 4, w.partw);
    hipLaunchKernelGGL(grcn::loss_finish, dim3(1), dim3(64), 0, s, k, (const float*)w.t.part, nblk,
                       (const float*)w.partw, out);
    if (result)
        hipLaunchKernelGGL(grcn::write_result, dim3(grcn::capped((k.nu + k.ni + 3) / 4, 4096)), dim3(256), 0, s, k, ld,
                           result);
    return last_rc();
}

int rsx_grcn_loss_bwd(const rsx_grcn_loss_args* a, const float* go, float* g_id, float* g_v, float* g_t, float* gE,
                      float* gpv, float* gpt, void* ws, size_t ws_bytes, rsx_stream_t stream) {
    grcn::LossArgs k;
    const int rc = grcn::loss_check(a, ws, ws_bytes, k);
    if (rc) return rc;
    if (!go || !g_id || !g_v || !gE || !gpv || (k.rt && (!g_t || !gpt))) return RSX_ERR_ARG;
    for (const void* p : {(const void*)g_id, (const void*)g_v, (const void*)g_t, (const void*)gE, (const void*)gpv,
                          (const void*)gpt})
        if (!aligned16(p)) return RSX_ERR_ARG;
    hipStream_t s = as_stream(stream);
    const TripletWs w = grcn::carve(ws, k.B, k.W).t;
    const size_t n = (size_t)(k.nu + k.ni);
    // (gpv: pref_whole_grad writes every row); the text tables only when the modality is present
    const int zrc = zero_tables({{g_id, n * k.dx}, {gE, n * k.dx}, {g_v, n * k.dc}, {k.rt ? g_t : nullptr, n * k.dc},
                                 {k.rt ? gpt : nullptr, (size_t)k.nu * k.dc}}, s);
    if (zrc) return zrc;
    hipLaunchKernelGGL(grcn::pref_whole_grad, dim3(grcn::capped((k.nu * k.dc / 4 + 255) / 256, 4096)), dim3(256), 0, s,
                       k, go, gpv);
    hipLaunchKernelGGL(grcn::loss_grad_rows, dim3(rows_blocks<256>(k.B)), dim3(256), 0, s, k, go, w.occU, w.occX,
                       w.coef, w.ku, w.ki);
    const grcn::LossGrads G{g_id, g_v, g_t, gE, gpv, gpt};
    launch_walk(grcn::loss_sum_rows, k.B, s, k, go, w.occU, w.occX, w.coef, w.ku, w.ki, G);
    return last_rc();
}

}  // extern "C"
