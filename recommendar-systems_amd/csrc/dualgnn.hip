// dualgnn.hip — DualGNN's step past the two modality GCNs (reference src/models/dualgnn.py):
//   mix      the in-place alias of dualgnn.py:148-170 in one pass over the modality tables:
//            user_rep = w0 (v + t) + w1 t on the user rows, v + t on the item rows, written
//            straight into `result`; its backward with g_weight_u as lane-group row dots and
//            the weight_u^2 regulariser's gradient in the same pass.
//   ugraph   out[u] = user_rep[u] + sum_j W[u, j] user_rep[idx[u, j]] (:172-173, :259-266): a
//            lane group a user, the row's k indices and weights loaded once by the group and
//            broadcast; its backward is the transposed lists on rsx_spmm.
//   loss     -mean log2 sigmoid(x) on `result` plus the regularisers (:182-197), on
//            rsx_triplet.hpp's protocol; the backward's dense g_result, the preference term's
//            gradient with the batch's repeat counts, and g_weight_i.
// Everything is d = 64, f32, deterministic and free of atomics: a row is RowGeom<64>'s lane
// group (16 lanes x float4), 16 rows a block.
#include <cmath>

#include "rsx_triplet.hpp"

namespace rsx {
namespace dg {

constexpr int D = 64;
constexpr int kL = D / 4;            // lanes a row
constexpr int kMaxK = 64;            // the user graph's widest list: 4 entries a lane
constexpr float kInvLn2 = 1.4426950408889634f;

// ---------------------------------------------------------------------------
// the modality mix
// ---------------------------------------------------------------------------
// w [nu, 2] (weight_u [nu, 2, 1]).  One table null: its rows pass through.
__global__ __launch_bounds__(256) void mix_fwd(const float* __restrict__ xv, const float* __restrict__ xt,
                                               const float* __restrict__ w, int64_t nu, int64_t n,
                                               float* __restrict__ user_rep, float* __restrict__ result) {
    const RowGeom<D> r;
    if (r.b >= n) return;
    const int64_t o = r.b * D + r.c;
    if (!xv || !xt) {
        const float4 x = ld4((xv ? xv : xt) + o);
        st4(r.b < nu ? user_rep + o : result + o, x);
        return;
    }
    const float4 t = ld4(xt + o), s = add4(ld4(xv + o), t);  // s: v after `representation += t_rep`
    if (r.b < nu) {
        const float w0 = w[2 * r.b], w1 = w[2 * r.b + 1];
        st4(user_rep + o, fma4(w1, t, mul4(w0, s)));
    } else {
        st4(result + o, s);
    }
}

// g_user_rep [nu, D]; g_result [n, D], its item rows read; cw = 2 reg_weight / (2 nu), times *go
__global__ __launch_bounds__(256) void mix_bwd(const float* __restrict__ g_user_rep,
                                               const float* __restrict__ g_result, const float* __restrict__ xv,
                                               const float* __restrict__ xt, const float* __restrict__ w,
                                               const float* __restrict__ go, float cw, int64_t nu, int64_t n,
                                               float* __restrict__ g_v, float* __restrict__ g_t,
                                               float* __restrict__ g_w) {
    const RowGeom<D> r;
    if (r.b >= n) return;  // uniform over a row's lane group
    const int64_t o = r.b * D + r.c;
    const bool user = r.b < nu;
    const float4 g = ld4((user ? g_user_rep : g_result) + o);
    float w0 = 0.f, w1 = 0.f;
    if (user) w0 = w[2 * r.b], w1 = w[2 * r.b + 1];
    const float c = cw * *go;
    if (!xv || !xt) {
        st4((xv ? g_v : g_t) + o, g);
        if (user && r.c == 0) g_w[2 * r.b] = c * w0, g_w[2 * r.b + 1] = c * w1;
        return;
    }
    if (!user) {
        st4(g_v + o, g);
        st4(g_t + o, g);
        return;
    }
    st4(g_v + o, mul4(w0, g));
    st4(g_t + o, mul4(w0 + w1, g));
    const float4 t = ld4(xt + o), s = add4(ld4(xv + o), t);
    const float d0 = group_sum<kL>(dot4(g, s)), d1 = group_sum<kL>(dot4(g, t));
    if (r.c == 0) g_w[2 * r.b] = fmaf(c, w0, d0), g_w[2 * r.b + 1] = fmaf(c, w1, d1);
}

// ---------------------------------------------------------------------------
// the user graph
// ---------------------------------------------------------------------------
// Lane l of a row's group holds entries l, l + 16, l + 32, l + 48 of the row's list; entry j is
// broadcast from lane j % 16 of the group.  An index outside [0, nu) contributes nothing.
__global__ __launch_bounds__(256) void ugraph_fwd(const float* __restrict__ x, const int32_t* __restrict__ idx,
                                                  const float* __restrict__ W, int64_t nu, int k,
                                                  float* __restrict__ out) {
    const RowGeom<D> r;
    if (r.b >= nu) return;  // uniform over a row's lane group
    const int gl = threadIdx.x % kL;                             // this lane's place in its group
    const int g0 = (threadIdx.x & (kWave - 1)) - gl;             // the group's first lane in the wave
    int li[kMaxK / kL];
    float lw[kMaxK / kL];
#pragma unroll
    for (int q = 0; q < kMaxK / kL; ++q) {
        const int j = q * kL + gl;
        li[q] = j < k ? idx[r.b * k + j] : -1;
        lw[q] = j < k ? W[r.b * k + j] : 0.f;
    }
    float4 acc = f4(0.f);
#pragma unroll
    for (int q = 0; q < kMaxK / kL; ++q) {
        const int cnt = k - q * kL < kL ? k - q * kL : kL;  // uniform
#pragma unroll 4
        for (int jj = 0; jj < cnt; ++jj) {
            const int i = __shfl(li[q], g0 + jj, kWave);
            const float wj = __shfl(lw[q], g0 + jj, kWave);
            if (i >= 0 && (int64_t)i < nu) acc = fma4(wj, ld4(x + (int64_t)i * D + r.c), acc);
        }
    }
    st4(out + r.b * D + r.c, add4(ld4(x + r.b * D + r.c), acc));
}

// ---------------------------------------------------------------------------
// the loss (dualgnn.py:175-197)
// ---------------------------------------------------------------------------
constexpr int kPartStride = 4;  // {softplus(-x), |pref_v[u]|^2, |pref_t[u]|^2, -}

struct LossArgs {
    const float *result, *pv, *pt, *wu, *wi;
    const int64_t* trip;
    int64_t nu, ni, B;
    float reg_weight;
};

__device__ __forceinline__ void load_trip(const LossArgs& a, int64_t b, int c, ScoreTrip& t) {
    load_score_trip<D>(
        a.trip, a.B, b, a.nu, a.ni, c, [&](int64_t u, int c) { return ld4(a.result + u * D + c); },
        [&](int64_t i, int c) { return ld4(a.result + (a.nu + i) * D + c); }, t);
}

__global__ __launch_bounds__(256) void loss_rows(LossArgs a, float* __restrict__ part) {
    const RowGeom<D> r;
    float v[3] = {0.f, 0.f, 0.f};
    if (r.b < a.B) {  // uniform over a row's lane group
        ScoreTrip t;
        load_trip(a, r.b, r.c, t);
        v[0] = softplus_neg(t.x);
        if (t.ok) {
            if (a.pv) {
                const float4 p = ld4(a.pv + t.u * D + r.c);
                v[1] = group_sum<kL>(dot4(p, p));
            }
            if (a.pt) {
                const float4 p = ld4(a.pt + t.u * D + r.c);
                v[2] = group_sum<kL>(dot4(p, p));
            }
        }
    }
    block_partials<D, 3, kPartStride>(r, v, part);
}

// sum of squares of t[0, n): thread i adds elements i, i + 256, ... in index order, the 256
// thread sums are added in a fixed tree.  Every thread of the 256-thread block enters.
__device__ __forceinline__ float block_sumsq(const float* __restrict__ t, int64_t n, float* sh) {
    float acc = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += 256) acc = fmaf(t[i], t[i], acc);
    acc = group_sum<kWave>(acc);
    __syncthreads();  // sh may still be read from the previous call
    if ((threadIdx.x & (kWave - 1)) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// out = {total, bpr, reg}
__global__ __launch_bounds__(256) void loss_finish(LossArgs a, const float* __restrict__ part, int nblk,
                                                   float* __restrict__ out) {
    __shared__ float sh[4];
    const float su = block_sumsq(a.wu, 2 * a.nu, sh);
    const float si = block_sumsq(a.wi, 2 * a.ni, sh);
    if (threadIdx.x >= kWave) return;
    float term[3];
    sum_partials<3, kPartStride>(part, nblk, term);
    if (threadIdx.x == 0) {
        const float bpr = term[0] / (float)a.B * kInvLn2;
        const float rows = (float)a.B * (float)D;
        const float reg = a.reg_weight * (term[1] / rows + term[2] / rows) +
                          a.reg_weight * (su / (float)(2 * a.nu)) + a.reg_weight * (si / (float)(2 * a.ni));
        out[0] = bpr + reg;
        out[1] = bpr;
        out[2] = reg;
    }
}

// Per triplet b: coef[b] = d total / d x_b (upstream included), occU[b] = coef (p - n), the user
// row's share; occR[b] = the user row (what an item occurrence scales by +-coef[b]); the keys.
__global__ __launch_bounds__(256) void loss_grad_rows(LossArgs a, const float* __restrict__ go,
                                                      float* __restrict__ occU, float* __restrict__ occR,
                                                      float* __restrict__ coef, int32_t* __restrict__ ku,
                                                      int32_t* __restrict__ ki) {
    const RowGeom<D> r;
    const int64_t b = r.b;
    if (b >= a.B) return;  // uniform over a row's lane group
    ScoreTrip t;
    load_trip(a, b, r.c, t);
    const float ck = bpr_coef(t, go, a.B) * kInvLn2;
    st4(occU + b * D + r.c, mul4(ck, sub4(t.pr, t.nr)));
    st4(occR + b * D + r.c, t.ur);
    if (r.c == 0) {
        coef[b] = ck;
        store_keys(t, a.B, b, ku, ki);
    }
}

// The per-destination sums (rsx_triplet.hpp's walk).  G [nu + ni, D], gpv, gpt [nu, D], all
// zero-filled; a user's walk also counts its occurrences: gp_m[u] = cp count(u) pref_m[u].
__global__ __launch_bounds__(256) void loss_sum_rows(LossArgs a, const float* __restrict__ go,
                                                     const float* __restrict__ occU, const float* __restrict__ occR,
                                                     const float* __restrict__ coef, const int32_t* __restrict__ ku,
                                                     const int32_t* __restrict__ ki, float* __restrict__ G,
                                                     float* __restrict__ gpv, float* __restrict__ gpt) {
    Walk<D> w;
    if (!w.begin(ku, ki, a.B)) return;
    const int c = w.c;
    float4 acc = f4(0.f);
    float cnt = 0.f;
    w.each(
        [&](int64_t occ) {
            acc = add4(acc, ld4(occU + occ * D + c));
            cnt += 1.f;
        },
        [&](int64_t b, float sgn) { acc = fma4(sgn * coef[b], ld4(occR + b * D + c), acc); });
    tree_rows<kL>(acc);
#pragma unroll
    for (int o = kWave / 2; o >= kL; o >>= 1) cnt += __shfl_xor(cnt, o, kWave);  // counts are exact
    if (w.g != 0) return;
    st4(G + (w.user ? (int64_t)w.key : a.nu + w.key) * D + c, acc);
    if (!w.user) return;
    const float cp = 2.f * a.reg_weight * *go / ((float)a.B * (float)D) * cnt;
    const int64_t o = (int64_t)w.key * D + c;
    if (gpv) st4(gpv + o, mul4(cp, ld4(a.pv + o)));
    if (gpt) st4(gpt + o, mul4(cp, ld4(a.pt + o)));
}

// g_weight_i = 2 reg_weight / (2 ni) weight_i, times *go
__global__ __launch_bounds__(256) void weight_i_grad(const float* __restrict__ wi, const float* __restrict__ go,
                                                     float cw, int64_t n, float* __restrict__ g) {
    const float c = cw * *go;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) g[i] = c * wi[i];
}

inline TripletWs carve(void* ws, int64_t B) { return carve_triplet(ws, B, D, kPartStride, 1, 1); }

inline int loss_check(const rsx_dualgnn_loss_args* a, void* ws, size_t ws_bytes, LossArgs& k) {
    if (!a) return RSX_ERR_ARG;
    const bool own_ok = a->result && a->weight_u && a->weight_i && a->triplets && ws && (a->pref_v || a->pref_t) &&
                        aligned16(a->result) && aligned16(a->pref_v) && aligned16(a->pref_t) && aligned16(ws);
    if (a->d != D && a->batch >= 1 && a->n_users >= 1 && a->n_items >= 1) return RSX_ERR_UNSUPPORTED;
    const int rc = check_triplet(a->batch, a->n_users, a->n_items, a->d, own_ok, ws_bytes,
                                 rsx_dualgnn_loss_ws_bytes(a->batch, a->d));
    if (rc) return rc;
    if (a->n_users + a->n_items > 0x7fffffffll) return RSX_ERR_UNSUPPORTED;
    k.result = a->result, k.pv = a->pref_v, k.pt = a->pref_t, k.wu = a->weight_u, k.wi = a->weight_i;
    k.trip = a->triplets, k.nu = a->n_users, k.ni = a->n_items, k.B = a->batch, k.reg_weight = a->reg_weight;
    return RSX_OK;
}

inline unsigned row_grid(int64_t rows) { return (unsigned)rows_blocks<D>(rows); }

}  // namespace dg
}  // namespace rsx

using namespace rsx;

extern "C" {

int rsx_dualgnn_mix_fwd(const float* xv, const float* xt, const float* weight_u, int64_t n_users, int64_t n_items,
                        int32_t d, float* user_rep, float* result, rsx_stream_t stream) {
    if (n_users < 1 || n_items < 1 || (!xv && !xt) || !weight_u || !user_rep || !result) return RSX_ERR_ARG;
    if (d != dg::D || n_users + n_items > 0x7fffffffll) return RSX_ERR_UNSUPPORTED;
    if (!aligned16(xv) || !aligned16(xt) || !aligned16(user_rep) || !aligned16(result)) return RSX_ERR_ARG;
    const int64_t n = n_users + n_items;
    hipLaunchKernelGGL(dg::mix_fwd, dim3(dg::row_grid(n)), dim3(256), 0, as_stream(stream), xv, xt, weight_u, n_users, n,
                       user_rep, result);
    return last_rc();
}

int rsx_dualgnn_mix_bwd(const float* g_user_rep, const float* g_result, const float* xv, const float* xt,
                        const float* weight_u, const float* go, float reg_weight, int64_t n_users, int64_t n_items,
                        int32_t d, float* g_v, float* g_t, float* g_weight_u, rsx_stream_t stream) {
    if (n_users < 1 || n_items < 1 || (!xv && !xt) || !g_user_rep || !g_result || !weight_u || !go || !g_weight_u)
        return RSX_ERR_ARG;
    if ((xv && !g_v) || (xt && !g_t)) return RSX_ERR_ARG;
    if (d != dg::D || n_users + n_items > 0x7fffffffll) return RSX_ERR_UNSUPPORTED;
    for (const void* p : {(const void*)g_user_rep, (const void*)g_result, (const void*)xv, (const void*)xt,
                          (const void*)g_v, (const void*)g_t})
        if (!aligned16(p)) return RSX_ERR_ARG;
    const int64_t n = n_users + n_items;
    const float cw = 2.f * reg_weight / (float)(2 * n_users);
    hipLaunchKernelGGL(dg::mix_bwd, dim3(dg::row_grid(n)), dim3(256), 0, as_stream(stream), g_user_rep, g_result, xv, xt,
                       weight_u, go, cw, n_users, n, g_v, g_t, g_weight_u);
    return last_rc();
}

int rsx_dualgnn_ugraph_fwd(const float* user_rep, const int32_t* idx, const float* W, int64_t n_users, int32_t k,
                           int32_t d, float* out, rsx_stream_t stream) {
    if (n_users < 1 || !user_rep || !idx || !W || !out || !aligned16(user_rep) || !aligned16(out)) return RSX_ERR_ARG;
    if (d != dg::D || k < 1 || k > dg::kMaxK || n_users > 0x7fffffffll) return RSX_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(dg::ugraph_fwd, dim3(dg::row_grid(n_users)), dim3(256), 0, as_stream(stream), user_rep, idx, W,
                       n_users, (int)k, out);
    return last_rc();
}

size_t rsx_dualgnn_loss_ws_bytes(int64_t batch, int32_t d) {
    return d == dg::D ? triplet_ws_bytes(batch, d, dg::kPartStride, 1, 1) : 0;
}

int rsx_dualgnn_loss_fwd(const rsx_dualgnn_loss_args* a, float* out, void* ws, size_t ws_bytes, rsx_stream_t stream) {
    dg::LossArgs k;
    const int rc = dg::loss_check(a, ws, ws_bytes, k);
    if (rc) return rc;
    if (!out) return RSX_ERR_ARG;
    hipStream_t s = as_stream(stream);
    const TripletWs w = dg::carve(ws, k.B);
    const int nblk = rows_blocks<dg::D>(k.B);
    hipLaunchKernelGGL(dg::loss_rows, dim3(nblk), dim3(256), 0, s, k, w.part);
    hipLaunchKernelGGL(dg::loss_finish, dim3(1), dim3(256), 0, s, k, (const float*)w.part, nblk, out);
    return last_rc();
}

int rsx_dualgnn_loss_bwd(const rsx_dualgnn_loss_args* a, const float* go, float* g_result, float* g_pref_v,
                         float* g_pref_t, float* g_weight_i, void* ws, size_t ws_bytes, rsx_stream_t stream) {
    dg::LossArgs k;
    const int rc = dg::loss_check(a, ws, ws_bytes, k);
    if (rc) return rc;
    if (!go || !g_result || !g_weight_i || !aligned16(g_result) || !aligned16(g_pref_v) || !aligned16(g_pref_t))
        return RSX_ERR_ARG;
    if ((k.pv && !g_pref_v) || (k.pt && !g_pref_t)) return RSX_ERR_ARG;
    hipStream_t s = as_stream(stream);
    const TripletWs w = dg::carve(ws, k.B);
    float* gpv = k.pv ? g_pref_v : nullptr;
    float* gpt = k.pt ? g_pref_t : nullptr;
    const int zrc = zero_tables({{g_result, (size_t)(k.nu + k.ni) * dg::D},
                                 {gpv, (size_t)k.nu * dg::D},
                                 {gpt, (size_t)k.nu * dg::D}},
                                s);
    if (zrc) return zrc;
    hipLaunchKernelGGL(dg::loss_grad_rows, dim3(rows_blocks<dg::D>(k.B)), dim3(256), 0, s, k, go, w.occU, w.occX, w.coef,
                       w.ku, w.ki);
    launch_walk(dg::loss_sum_rows, k.B, s, k, go, w.occU, w.occX, w.coef, w.ku, w.ki, g_result, gpv, gpt);
    const int64_t nw = 2 * k.ni;
    const int64_t nb = (nw + 255) / 256;
    hipLaunchKernelGGL(dg::weight_i_grad, dim3((unsigned)(nb < 1024 ? nb : 1024)), dim3(256), 0, s, k.wi, go,
                       2.f * k.reg_weight / (float)(2 * k.ni), nw, g_weight_i);
    return last_rc();
}

}  // extern "C"
