// lattice.hip — LATTICE on gfx950: the training loss, the learned item graph (build, propagation
// and the build batch's backward).
//
// Replaces (reference paths relative to its root):
//   src/models/lattice.py:199-227   the BPR loss with the L2 term on the propagated batch rows,
//                                   the item rows being E[nu + i] + F.normalize(h)[i], and their
//                                   autograd backward (index_put scatter-adds, normalize)
//   src/models/lattice.py:137-163   the learned item graph: build_sim + build_knn_neighbourhood
//                                   of the projected features, the modality mix, the degree
//                                   normalisation, the mix with the original graphs and
//                                   torch.mm(item_adj, h) on dense [n, n] matrices
// The dense matrix is never formed: item_adj is kept as 2 M lists of k edges a row (M
// modalities: the learned top-k lists and the original graphs' lists), in which it is linear.
//
// Layout: a d-wide row is one lane group of L = d / 4 float4 lanes (rsx_triplet.hpp's RowGeom).
//
// The loss.  The protocol (one-score triplet, block partials, keys, the first-occurrence walk,
//   workspace, argument checks) is rsx_triplet.hpp's; this file has the item row, the L2 term
//   and the walk's epilogue, which sends an item row's sum through the normalise Jacobian into gH.
// The graph.  One edge table [n, K], K = 2 M k: slots [m k, (m + 1) k) the learned list of
//   modality m, slots [(M + m) k, ...) its original list.  The transpose is an index: the edge
//   ids sorted by column (stable, built by the caller once per epoch) with a row pointer; the
//   values are read through it, so they exist once.  No float atomics anywhere: every sum is
//   a walk of a row's slots or of a column's index segment in a fixed order.
#include "rsx_triplet.hpp"

namespace rsx {
namespace lattice {

constexpr int kPartStride = 2, kCoef = 1;  // words a block partial, coefficients a triplet
constexpr int kMaxLayers = 4;
constexpr float kNormEps = 1e-12f;  // F.normalize's eps

struct Args {
    const float *E, *H;
    const int64_t* trip;
    int64_t nu, ni, B;
    float reg, bs;
};

// E[nu + i] + H[i] / max(|H[i]|, eps) as seen by one lane (its 4 columns)
template <int D>
__device__ __forceinline__ float4 item_row(const Args& a, int64_t i, int c) {
    const float4 h = ld4(a.H + i * D + c);
    const float nrm = sqrtf(group_sum<D / 4>(dot4(h, h)));
    return fma4(1.f / fmaxf(nrm, kNormEps), h, ld4(a.E + (a.nu + i) * D + c));
}

template <int D>
__device__ __forceinline__ void load_trip(const Args& a, int64_t b, int c, ScoreTrip& t) {
    load_score_trip<D>(
        a.trip, a.B, b, a.nu, a.ni, c, [&](int64_t u, int c) { return ld4(a.E + u * D + c); },
        [&](int64_t i, int c) { return item_row<D>(a, i, c); }, t);
}

// part[block] = {sum softplus(-x), sum 1/2 (|u|^2 + |p|^2 + |n|^2)} over the block's triplets, in row order
template <int D>
__global__ __launch_bounds__(256) void loss_rows(Args a, float* __restrict__ part) {
    constexpr int L = RowGeom<D>::L;
    const RowGeom<D> r;
    float v[2] = {0.f, 0.f};
    if (r.b < a.B) {  // uniform over a row's lane group
        ScoreTrip t;
        load_trip<D>(a, r.b, r.c, t);
        v[0] = softplus_neg(t.x);
        const float sq = group_sum<L>(dot4(t.ur, t.ur)) + group_sum<L>(dot4(t.pr, t.pr)) +
                         group_sum<L>(dot4(t.nr, t.nr));
        v[1] = t.ok ? 0.5f * sq : __builtin_nanf("");
    }
    block_partials<D, 2, kPartStride>(r, v, part);
}

// out = {total, mf, emb}: the block partials in index order
__global__ __launch_bounds__(64) void finish(const float* __restrict__ part, int nblk, int64_t B, float reg, float bs,
                                             float* __restrict__ out) {
    float term[2];
    sum_partials<2, kPartStride>(part, nblk, term);
    if (threadIdx.x == 0) {
        const float mf = term[0] / (float)B, emb = reg * (term[1] / bs);
        out[0] = mf + emb;
        out[1] = mf;
        out[2] = emb;
    }
}

// Per triplet b: coef[b] = d total / d x, occU[b] = its contribution to the user row
// coef (p - n) + s u with s = go reg / batch_size, and the keys (store_keys).
template <int D>
__global__ __launch_bounds__(256) void grad_rows(Args a, const float* __restrict__ go, float* __restrict__ occU,
                                                 float* __restrict__ coef, int32_t* __restrict__ ku,
                                                 int32_t* __restrict__ ki) {
    const RowGeom<D> r;
    const int64_t b = r.b;
    const int c = r.c;
    if (b >= a.B) return;  // uniform over a row's lane group
    ScoreTrip t;
    load_trip<D>(a, b, c, t);
    const float ck = bpr_coef(t, go, a.B), s = t.ok ? *go * a.reg / a.bs : 0.f;
    st4(occU + b * D + c, fma4(s, t.ur, mul4(ck, sub4(t.pr, t.nr))));
    if (c == 0) {
        coef[b] = ck;
        store_keys(t, a.B, b, ku, ki);
    }
}

// The per-destination sums (rsx_triplet.hpp's walk).  An item row's sum g = sum(+-coef E[user]) +
// count s row goes to gE[nu + key], and (g - hn <hn, g>) / max(|h|, eps), hn = h / max(|h|, eps),
// to gH[key].
template <int D>
__global__ __launch_bounds__(256) void sum_rows(Args a, const float* __restrict__ go, const float* __restrict__ occU,
                                                const float* __restrict__ coef, const int32_t* __restrict__ ku,
                                                const int32_t* __restrict__ ki, float* __restrict__ gE,
                                                float* __restrict__ gH) {
    constexpr int L = Walk<D>::L;
    Walk<D> w;
    if (!w.begin(ku, ki, a.B)) return;
    const int c = w.c;
    const int32_t key = w.key;
    float4 hn = f4(0.f), sp = f4(0.f);
    float inv = 0.f;
    if (!w.user) {  // the item's own row, scaled by s: added once an occurrence
        const float4 h = ld4(a.H + (int64_t)key * D + c);
        inv = 1.f / fmaxf(sqrtf(group_sum<L>(dot4(h, h))), kNormEps);
        hn = mul4(inv, h);
        sp = mul4(*go * a.reg / a.bs, add4(hn, ld4(a.E + (a.nu + key) * D + c)));
    }
    float4 acc = f4(0.f);
    w.each([&](int64_t occ) { acc = add4(acc, ld4(occU + occ * D + c)); },
           [&](int64_t b, float sgn) {
               acc = fma4(sgn * coef[b], ld4(a.E + (int64_t)ku[b] * D + c), acc);
               acc = add4(acc, sp);
           });
    tree_rows<L>(acc);
    const float hg = group_sum<L>(dot4(hn, acc));  // every lane group holds the same sum now
    if (w.g != 0) return;
    if (w.user) {
        st4(gE + (int64_t)key * D + c, acc);
    } else {
        st4(gE + (a.nu + key) * D + c, acc);
        st4(gH + (int64_t)key * D + c, mul4(inv, fma4(-hg, hn, acc)));
    }
}

inline TripletWs carve(void* ws, int64_t B, int d) { return carve_triplet(ws, B, d, kPartStride, kCoef); }

inline int check(const rsx_lattice_args* a, void* ws, size_t ws_bytes, Args& k) {
    if (!a) return RSX_ERR_ARG;
    const bool own_ok = a->E && a->H && a->triplets && ws && a->batch_size > 0.f && aligned16(a->E) &&
                        aligned16(a->H) && aligned16(ws);
    const int rc = check_triplet(a->batch, a->n_users, a->n_items, a->d, own_ok, ws_bytes,
                                 rsx_lattice_ws_bytes(a->batch, a->d));
    if (rc) return rc;
    k.E = a->E, k.H = a->H, k.trip = a->triplets;
    k.nu = a->n_users, k.ni = a->n_items, k.B = a->batch, k.reg = a->reg, k.bs = a->batch_size;
    return RSX_OK;
}

template <int D>
int fwd(const Args& k, float* out, void* ws, hipStream_t s) {
    const TripletWs w = carve(ws, k.B, D);
    const int nblk = rows_blocks<D>(k.B);
    hipLaunchKernelGGL(loss_rows<D>, dim3(nblk), dim3(256), 0, s, k, w.part);
    hipLaunchKernelGGL(finish, dim3(1), dim3(64), 0, s, (const float*)w.part, nblk, k.B, k.reg, k.bs, out);
    return last_rc();
}

template <int D>
int bwd(const Args& k, const float* go, float* gE, float* gH, void* ws, hipStream_t s) {
    const TripletWs w = carve(ws, k.B, D);
    const int rc = zero_tables({{gE, (size_t)(k.nu + k.ni) * D}, {gH, (size_t)k.ni * D}}, s);
    if (rc) return rc;
    hipLaunchKernelGGL(grad_rows<D>, dim3(rows_blocks<D>(k.B)), dim3(256), 0, s, k, go, w.occU, w.coef, w.ku, w.ki);
    launch_walk(sum_rows<D>, k.B, s, k, go, w.occU, w.coef, w.ku, w.ki, gE, gH);
    return last_rc();
}

// ---------------------------------------------------------------------------
// the learned item graph
// ---------------------------------------------------------------------------
struct Graph {
    int64_t n;
    int k, M, K;  // K = 2 M k
    float lam;
    const float* F[2];
    const int64_t *idx[2], *oidx[2];
    const float* oval[2];
    const float* mw;
    float *w, *invn[2], *a[2], *r, *dis, *val;
    int32_t* col;
    const int64_t* tptr;
    const int32_t* tedge;
};

// softmax(modal_weight) (one modality: its weight is 1)
__device__ __forceinline__ void modal_w(const Graph& g, float w[2]) {
    w[0] = 1.f, w[1] = 0.f;
    if (g.M == 2) {
        const float a = g.mw[0], b = g.mw[1], mx = fmaxf(a, b);
        const float ea = expf(a - mx), eb = expf(b - mx);
        w[0] = ea / (ea + eb), w[1] = eb / (ea + eb);
    }
}

// invn[m][i] = 1 / |F_m[i]|: a lane group a (modality, row)
template <int F>
__global__ __launch_bounds__(256) void norms(Graph g) {
    constexpr int L = F / 4, RPB = 256 / L;
    const int c = (threadIdx.x % L) * 4;
    const int64_t q = (int64_t)blockIdx.x * RPB + threadIdx.x / L;
    if (q >= g.M * g.n) return;  // uniform over the lane group
    const int m = (int)(q / g.n);
    const int64_t i = q % g.n;
    const float4 x = ld4(g.F[m] + i * F + c);
    const float s = group_sum<L>(dot4(x, x));
    if (c == 0) g.invn[m][i] = 1.f / sqrtf(s);
}

// a[m][i, j] = cos(F_m[i], F_m[idx_m[i, j]]) and the edge table's columns.  A column outside
// [0, n) becomes the row itself with similarity 0 (and weight 0 in `values`).
template <int F>
__global__ __launch_bounds__(256) void sims(Graph g) {
    constexpr int L = F / 4, RPB = 256 / L;
    const int c = (threadIdx.x % L) * 4;
    const int64_t q = (int64_t)blockIdx.x * RPB + threadIdx.x / L;
    if (q >= g.M * g.n) return;
    const int m = (int)(q / g.n);
    const int64_t i = q % g.n;
    const float* Fm = g.F[m];
    const float4 x = mul4(g.invn[m][i], ld4(Fm + i * F + c));
    for (int j = 0; j < g.k; ++j) {
        int64_t cj = g.idx[m][i * g.k + j], oj = g.oidx[m][i * g.k + j];
        const bool ok = cj >= 0 && cj < g.n;
        if (!ok) cj = i;
        if (oj < 0 || oj >= g.n) oj = -1;
        const float s = group_sum<L>(dot4(x, mul4(g.invn[m][cj], ld4(Fm + cj * F + c))));
        if (c == 0) {
            g.a[m][i * g.k + j] = ok ? s : 0.f;
            g.col[i * g.K + m * g.k + j] = (int32_t)cj;
            g.col[i * g.K + (g.M + m) * g.k + j] = (int32_t)(oj < 0 ? i : oj);
        }
    }
}

// r[i] = sum_m w_m sum_j a_m[i, j] (rank order), dis = r^-1/2 with inf -> 0: a thread a row
__global__ __launch_bounds__(256) void degrees(Graph g) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float w[2];
    modal_w(g, w);
    if (i == 0) g.w[0] = w[0], g.w[1] = w[1];
    if (i >= g.n) return;
    float r = 0.f;
    for (int m = 0; m < g.M; ++m) {
        float s = 0.f;
        for (int j = 0; j < g.k; ++j) s += g.a[m][i * g.k + j];
        r += w[m] * s;
    }
    float d = 1.f / sqrtf(r);
    if (isinf(d)) d = 0.f;
    g.r[i] = r;
    g.dis[i] = d;
}

// the edge values: (1 - lam) w_m dis_i a dis_c on a learned slot, lam w_m O_m on an original one
__global__ __launch_bounds__(256) void values(Graph g) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= g.n * g.K) return;
    const int64_t i = e / g.K;
    const int s = (int)(e % g.K), m = (s / g.k) % g.M, j = s % g.k;
    float w[2];
    modal_w(g, w);
    float v;
    if (s < g.M * g.k) {
        v = (1.f - g.lam) * w[m] * (g.dis[i] * g.a[m][i * g.k + j] * g.dis[g.col[e]]);
    } else {
        const int64_t oj = g.oidx[m][i * g.k + j];
        v = (oj >= 0 && oj < g.n) ? g.lam * w[m] * g.oval[m][i * g.k + j] : 0.f;
    }
    g.val[e] = v;
}

// y = item_adj x (T = false: a row's K slots in order) or item_adj^T x (T = true: the
// column's segment of the transpose index in order): a lane group a row
template <int D, bool T>
__global__ __launch_bounds__(256) void prop(Graph g, const float* __restrict__ x, float* __restrict__ y) {
    constexpr int L = D / 4, RPB = 256 / L;
    const int c = (threadIdx.x % L) * 4;
    const int64_t i = (int64_t)blockIdx.x * RPB + threadIdx.x / L;
    if (i >= g.n) return;
    float4 acc = f4(0.f);
    if (!T) {
        const int32_t* col = g.col + i * g.K;
        const float* val = g.val + i * g.K;
        for (int s = 0; s < g.K; ++s) acc = fma4(val[s], ld4(x + (int64_t)col[s] * D + c), acc);
    } else {
        for (int64_t t = g.tptr[i]; t < g.tptr[i + 1]; ++t) {
            const int64_t e = g.tedge[t];
            acc = fma4(g.val[e], ld4(x + (e / g.K) * D + c), acc);
        }
    }
    st4(y + i * D + c, acc);
}

struct Layers {
    int n;
    const float *G[kMaxLayers], *X[kMaxLayers];
};

// P[i, s] = sum_l <G_l[i], X_l[col[i, s]]>: a lane group a row
template <int D>
__global__ __launch_bounds__(256) void edge_dots(Graph g, Layers ly, float* __restrict__ P) {
    constexpr int L = D / 4, RPB = 256 / L;
    const int c = (threadIdx.x % L) * 4;
    const int64_t i = (int64_t)blockIdx.x * RPB + threadIdx.x / L;
    if (i >= g.n) return;
    float4 gr[kMaxLayers];
#pragma unroll
    for (int l = 0; l < kMaxLayers; ++l) gr[l] = l < ly.n ? ld4(ly.G[l] + i * D + c) : f4(0.f);
    for (int s = 0; s < g.K; ++s) {
        const int64_t cj = g.col[i * g.K + s];
        float p = 0.f;
#pragma unroll
        for (int l = 0; l < kMaxLayers; ++l)
            if (l < ly.n) p += dot4(gr[l], ld4(ly.X[l] + cj * D + c));
        p = group_sum<L>(p);
        if (c == 0) P[i * g.K + s] = p;
    }
}

// gr[i] = d loss / d r_i and the row's share pw[i, m] of d loss / d w_m: a thread a row
__global__ __launch_bounds__(256) void row_scalars(Graph g, const float* __restrict__ P, float* __restrict__ grr,
                                                   double* __restrict__ pw) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= g.n) return;
    float w[2];
    modal_w(g, w);
    const int KL = g.M * g.k;
    const double di = g.dis[i];
    double rowp = 0.0, wl[2] = {0.0, 0.0}, wo[2] = {0.0, 0.0}, sa[2] = {0.0, 0.0};
    for (int m = 0; m < g.M; ++m)
        for (int j = 0; j < g.k; ++j) {
            const int64_t e = i * g.K + m * g.k + j;
            const double a = g.a[m][i * g.k + j], t = a * (double)g.dis[g.col[e]] * (double)P[e];
            wl[m] += t;
            sa[m] += a;
            const int64_t oj = g.oidx[m][i * g.k + j];
            if (oj >= 0 && oj < g.n) wo[m] += (double)g.oval[m][i * g.k + j] * (double)P[e + KL];
        }
    for (int m = 0; m < g.M; ++m) rowp += w[m] * wl[m];
    double colp = 0.0;
    for (int64_t t = g.tptr[i]; t < g.tptr[i + 1]; ++t) {
        const int64_t e = g.tedge[t];
        const int s = (int)(e % g.K);
        if (s >= KL) continue;
        const int64_t r = e / g.K;
        colp += (double)w[s / g.k] * (double)g.a[s / g.k][r * g.k + s % g.k] * (double)g.dis[r] * (double)P[e];
    }
    const double gdis = (1.0 - g.lam) * (rowp + colp);
    const double gr = -0.5 * gdis * di * di * di;  // r^-3/2 = dis^3; 0 where dis was forced to 0
    grr[i] = (float)gr;
    for (int m = 0; m < g.M; ++m) pw[i * 2 + m] = (1.0 - g.lam) * di * wl[m] + (double)g.lam * wo[m] + gr * sa[m];
}

// g modal_weight = w (gw - <w, gw>), gw_m = sum_i pw[i, m] in a fixed order: one block
__global__ __launch_bounds__(256) void mw_grad(Graph g, const double* __restrict__ pw, float* __restrict__ gmw) {
    __shared__ double sh[256][2];
    double acc[2] = {0.0, 0.0};
    for (int64_t i = threadIdx.x; i < g.n; i += 256) acc[0] += pw[i * 2], acc[1] += pw[i * 2 + 1];
    sh[threadIdx.x][0] = acc[0], sh[threadIdx.x][1] = acc[1];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x][0] += sh[threadIdx.x + o][0], sh[threadIdx.x][1] += sh[threadIdx.x + o][1];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        float w[2];
        modal_w(g, w);
        const double dot = w[0] * sh[0][0] + w[1] * sh[0][1];
        gmw[0] = (float)(w[0] * (sh[0][0] - dot));
        gmw[1] = (float)(w[1] * (sh[0][1] - dot));
    }
}

// gF_m[i] = (gxn - xn <xn, gxn>) / |F_m[i]|, gxn = sum_j ga[i, j] xn_c + sum over the incoming
// learned edges (i', j) of modality m of ga[i', j] xn_i', ga = w_m ((1 - lam) dis_i dis_c P + gr_i):
// a lane group a (modality, row)
template <int F>
__global__ __launch_bounds__(256) void feat_grad(Graph g, const float* __restrict__ P, const float* __restrict__ grr,
                                                 float* __restrict__ gF0, float* __restrict__ gF1) {
    constexpr int L = F / 4, RPB = 256 / L;
    const int c = (threadIdx.x % L) * 4;
    const int64_t q = (int64_t)blockIdx.x * RPB + threadIdx.x / L;
    if (q >= g.M * g.n) return;
    const int m = (int)(q / g.n);
    const int64_t i = q % g.n;
    float w[2];
    modal_w(g, w);
    const float* Fm = g.F[m];
    const float* invn = g.invn[m];
    const float wm = w[m], one = 1.f - g.lam, di = g.dis[i], gri = grr[i];
    float4 acc = f4(0.f);
    for (int j = 0; j < g.k; ++j) {
        const int64_t e = i * g.K + m * g.k + j, cj = g.col[e];
        if (g.idx[m][i * g.k + j] != cj) continue;  // a column that was out of range: no edge
        const float ga = wm * (one * di * g.dis[cj] * P[e] + gri);
        acc = fma4(ga * invn[cj], ld4(Fm + cj * F + c), acc);
    }
    for (int64_t t = g.tptr[i]; t < g.tptr[i + 1]; ++t) {
        const int64_t e = g.tedge[t];
        const int s = (int)(e % g.K);
        if (s / g.k != m) continue;
        const int64_t r = e / g.K;
        if (g.idx[m][r * g.k + s % g.k] != i) continue;
        const float ga = wm * (one * g.dis[r] * di * P[e] + grr[r]);
        acc = fma4(ga * invn[r], ld4(Fm + r * F + c), acc);
    }
    const float4 xn = mul4(invn[i], ld4(Fm + i * F + c));
    const float d = group_sum<L>(dot4(xn, acc));
    st4((m ? gF1 : gF0) + i * F + c, mul4(invn[i], fma4(-d, xn, acc)));
}

inline int to_graph(const rsx_lattice_graph_args* a, Graph& g, bool need_t) {
    if (!a || a->n < 1 || a->k < 1 || (a->n_mod != 1 && a->n_mod != 2)) return RSX_ERR_ARG;
    if (a->k > 32 || a->k > a->n || a->n > 0x7fffffffll / (4 * a->k)) return RSX_ERR_UNSUPPORTED;
    if (a->f != 64 && a->f != 128) return RSX_ERR_UNSUPPORTED;
    g.n = a->n, g.k = a->k, g.M = a->n_mod, g.K = 2 * a->n_mod * a->k, g.lam = a->lambda;
    for (int m = 0; m < 2; ++m) {
        const bool on = m < a->n_mod;
        g.F[m] = on ? a->F[m] : nullptr, g.idx[m] = on ? a->idx[m] : nullptr, g.oidx[m] = on ? a->oidx[m] : nullptr;
        g.oval[m] = on ? a->oval[m] : nullptr, g.invn[m] = on ? a->invn[m] : nullptr, g.a[m] = on ? a->a[m] : nullptr;
        if (on && (!g.F[m] || !g.idx[m] || !g.oidx[m] || !g.oval[m] || !g.invn[m] || !g.a[m] || !aligned16(g.F[m])))
            return RSX_ERR_ARG;
    }
    g.mw = a->modal_weight, g.w = a->w, g.r = a->r, g.dis = a->dis, g.val = a->val, g.col = a->col;
    g.tptr = a->tptr, g.tedge = a->tedge;
    if ((g.M == 2 && !g.mw) || !g.w || !g.r || !g.dis || !g.val || !g.col) return RSX_ERR_ARG;
    if (need_t && (!g.tptr || !g.tedge)) return RSX_ERR_ARG;
    return RSX_OK;
}

template <int F>
int graph_fwd(const Graph& g, hipStream_t s) {
    constexpr int RPB = 256 / (F / 4);
    const unsigned nb = (unsigned)((g.M * g.n + RPB - 1) / RPB);
    hipLaunchKernelGGL(norms<F>, dim3(nb), dim3(256), 0, s, g);
    hipLaunchKernelGGL(sims<F>, dim3(nb), dim3(256), 0, s, g);
    hipLaunchKernelGGL(degrees, dim3((unsigned)((g.n + 255) / 256)), dim3(256), 0, s, g);
    hipLaunchKernelGGL(values, dim3((unsigned)((g.n * g.K + 255) / 256)), dim3(256), 0, s, g);
    return last_rc();
}

template <int D>
int run_prop(const Graph& g, const float* x, float* y, bool t, hipStream_t s) {
    constexpr int RPB = 256 / (D / 4);
    const unsigned nb = (unsigned)((g.n + RPB - 1) / RPB);
    if (t)
        hipLaunchKernelGGL((prop<D, true>), dim3(nb), dim3(256), 0, s, g, x, y);
    else
        hipLaunchKernelGGL((prop<D, false>), dim3(nb), dim3(256), 0, s, g, x, y);
    return last_rc();
}

struct BwdWs {
    float *P, *gr;
    double* pw;
    size_t total;
};
inline BwdWs carve_bwd(void* ws, int64_t n, int K) {
    BwdWs w;
    Carver cv(ws);
    w.P = cv.take<float>((size_t)n * K * sizeof(float));
    w.gr = cv.take<float>((size_t)n * sizeof(float));
    w.pw = cv.take<double>((size_t)n * 2 * sizeof(double));
    w.total = cv.total();
    return w;
}

}  // namespace lattice
}  // namespace rsx

using namespace rsx;

extern "C" size_t rsx_lattice_ws_bytes(int64_t batch, int32_t d) {
    return triplet_ws_bytes(batch, d, lattice::kPartStride, lattice::kCoef);
}

extern "C" int rsx_lattice_loss_fwd(const rsx_lattice_args* a, float* out, void* ws, size_t ws_bytes,
                                    rsx_stream_t stream) {
    lattice::Args k;
    const int rc = lattice::check(a, ws, ws_bytes, k);
    if (rc) return rc;
    if (!out) return RSX_ERR_ARG;
    hipStream_t s = as_stream(stream);
    return a->d == 64 ? lattice::fwd<64>(k, out, ws, s) : lattice::fwd<128>(k, out, ws, s);
}

extern "C" int rsx_lattice_loss_bwd(const rsx_lattice_args* a, const float* go, float* gE, float* gH, void* ws,
                                    size_t ws_bytes, rsx_stream_t stream) {
    lattice::Args k;
    const int rc = lattice::check(a, ws, ws_bytes, k);
    if (rc) return rc;
    if (!go || !gE || !gH || !aligned16(gE) || !aligned16(gH)) return RSX_ERR_ARG;
    hipStream_t s = as_stream(stream);
    return a->d == 64 ? lattice::bwd<64>(k, go, gE, gH, ws, s) : lattice::bwd<128>(k, go, gE, gH, ws, s);
}

extern "C" int rsx_lattice_graph(const rsx_lattice_graph_args* a, rsx_stream_t stream) {
    lattice::Graph g;
    const int rc = lattice::to_graph(a, g, false);
    if (rc) return rc;
    hipStream_t s = as_stream(stream);
    return a->f == 64 ? lattice::graph_fwd<64>(g, s) : lattice::graph_fwd<128>(g, s);
}

extern "C" int rsx_lattice_prop(const rsx_lattice_graph_args* a, const float* x, float* y, int32_t d, int32_t transpose,
                                rsx_stream_t stream) {
    lattice::Graph g;
    const int rc = lattice::to_graph(a, g, transpose != 0);
    if (rc) return rc;
    if (d != 64 && d != 128) return RSX_ERR_UNSUPPORTED;
    if (!x || !y || x == y || !aligned16(x) || !aligned16(y)) return RSX_ERR_ARG;
    hipStream_t s = as_stream(stream);
    return d == 64 ? lattice::run_prop<64>(g, x, y, transpose != 0, s)
                   : lattice::run_prop<128>(g, x, y, transpose != 0, s);
}

extern "C" size_t rsx_lattice_graph_bwd_ws_bytes(int64_t n, int32_t k, int32_t n_mod) {
    if (n < 1 || k < 1 || k > 32 || (n_mod != 1 && n_mod != 2)) return 0;
    return lattice::carve_bwd(nullptr, n, 2 * n_mod * k).total;
}

extern "C" int rsx_lattice_graph_bwd(const rsx_lattice_graph_args* a, int32_t n_layers, const float* const* G,
                                     const float* const* X, int32_t d, float* gF0, float* gF1, float* g_modal_weight,
                                     void* ws, size_t ws_bytes, rsx_stream_t stream) {
    lattice::Graph g;
    const int rc = lattice::to_graph(a, g, true);
    if (rc) return rc;
    if (d != 64 && d != 128) return RSX_ERR_UNSUPPORTED;
    if (n_layers < 1 || n_layers > lattice::kMaxLayers) return RSX_ERR_UNSUPPORTED;
    if (!G || !X || !gF0 || (g.M == 2 && (!gF1 || !g_modal_weight)) || !ws) return RSX_ERR_ARG;
    if (!aligned16(gF0) || !aligned16(gF1) || !aligned16(ws)) return RSX_ERR_ARG;
    if (ws_bytes < rsx_lattice_graph_bwd_ws_bytes(g.n, g.k, g.M)) return RSX_ERR_WORKSPACE;
    lattice::Layers ly;
    ly.n = n_layers;
    for (int l = 0; l < lattice::kMaxLayers; ++l) {
        ly.G[l] = l < n_layers ? G[l] : nullptr;
        ly.X[l] = l < n_layers ? X[l] : nullptr;
        if (l < n_layers && (!ly.G[l] || !ly.X[l] || !aligned16(ly.G[l]) || !aligned16(ly.X[l])))
            return RSX_ERR_ARG;
    }
    const lattice::BwdWs w = lattice::carve_bwd(ws, g.n, g.K);
    hipStream_t s = as_stream(stream);
    const unsigned nbd = (unsigned)((g.n + 256 / (d / 4) - 1) / (256 / (d / 4)));
    if (d == 64)
        hipLaunchKernelGGL(lattice::edge_dots<64>, dim3(nbd), dim3(256), 0, s, g, ly, w.P);
    else
        hipLaunchKernelGGL(lattice::edge_dots<128>, dim3(nbd), dim3(256), 0, s, g, ly, w.P);
    hipLaunchKernelGGL(lattice::row_scalars, dim3((unsigned)((g.n + 255) / 256)), dim3(256), 0, s, g,
                       (const float*)w.P, w.gr, w.pw);
    if (g.M == 2)
        hipLaunchKernelGGL(lattice::mw_grad, dim3(1), dim3(256), 0, s, g, (const double*)w.pw, g_modal_weight);
    const int rpf = 256 / (a->f / 4);
    const unsigned nbf = (unsigned)((g.M * g.n + rpf - 1) / rpf);
    if (a->f == 64)
        hipLaunchKernelGGL(lattice::feat_grad<64>, dim3(nbf), dim3(256), 0, s, g, (const float*)w.P,
                           (const float*)w.gr, gF0, gF1);
    else
        hipLaunchKernelGGL(lattice::feat_grad<128>, dim3(nbf), dim3(256), 0, s, g, (const float*)w.P,
                           (const float*)w.gr, gF0, gF1);
    return last_rc();
}
