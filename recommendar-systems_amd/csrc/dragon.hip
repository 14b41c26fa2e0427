// dragon.hip — DRAGON's step past the two modality GCNs (reference src/models/dragon.py):
//   cat      the concatenation of dragon.py:231-245 in one pass over the two 64-wide modality
//            tables: user_rep[u] = [w0 v[u] | w1 t[u]], item_rep = [v | t], both 128 wide; its
//            backward splits the 128-wide gradients again, g_weight_u as half-group row dots.
//   ugraph   out[u] = user_rep[u] + sum_j W[u, j] user_rep[idx[u, j]] (:251-252, :327-341):
//            DualGNN's list kernel as a template on the width; a lane group a user, the row's k
//            indices and weights loaded once by the group and broadcast; its backward is the
//            transposed lists on rsx_spmm.
//   loss     -mean log2 sigmoid(x) on `result` plus the regularisers (:262-277), on
//            rsx_triplet.hpp's protocol; the backward's dense g_result, the preference terms'
//            gradients with the batch's repeat counts, and g_weight_u.  No weight_i term.
// Everything is f32, deterministic and free of atomics: a row is RowGeom<D>'s lane group, at
// D = 128 32 lanes x float4 and 8 rows a block, at D = 64 16 lanes and 16 rows.  The item graph
// between the cat and the loss is rsx_spmm.
#include <cmath>

#include "rsx_triplet.hpp"

namespace rsx {
namespace dr {

constexpr int DM = 64;               // a modality table's and a preference table's width
constexpr int DC = 2 * DM;           // the concatenation's
constexpr int kHalf = DM / 4;        // the lanes of one modality's half of a 128-wide row
constexpr int kMaxK = 64;            // the user graph's widest list
constexpr float kInvLn2 = 1.4426950408889634f;

// ---------------------------------------------------------------------------
// the concatenation
// ---------------------------------------------------------------------------
// xv, xt [n, 64]; w [nu, 2] (weight_u [nu, 2, 1]).  Lanes with c < 64 read xv, the others xt.
__global__ __launch_bounds__(256) void cat_fwd(const float* __restrict__ xv, const float* __restrict__ xt,
                                               const float* __restrict__ w, int64_t nu, int64_t n,
                                               float* __restrict__ user_rep, float* __restrict__ item_rep) {
    const RowGeom<DC> r;
    if (r.b >= n) return;
    const int hi = r.c >= DM;
    const float4 x = ld4((hi ? xt : xv) + r.b * DM + (r.c - hi * DM));
    if (r.b < nu)
        st4(user_rep + r.b * DC + r.c, mul4(w[2 * r.b + hi], x));
    else
        st4(item_rep + (r.b - nu) * DC + r.c, x);
}

// g_user_rep [nu, 128], g_item_rep [ni, 128] -> g_v, g_t [n, 64]; g_w[u] = (<g[:64], v>, <g[64:], t>)
__global__ __launch_bounds__(256) void cat_bwd(const float* __restrict__ g_user_rep,
                                               const float* __restrict__ g_item_rep, const float* __restrict__ xv,
                                               const float* __restrict__ xt, const float* __restrict__ w, int64_t nu,
                                               int64_t n, float* __restrict__ g_v, float* __restrict__ g_t,
                                               float* __restrict__ g_w) {
    const RowGeom<DC> r;
    if (r.b >= n) return;  // uniform over a row's lane group
    const int hi = r.c >= DM;
    const int64_t o = r.b * DM + (r.c - hi * DM);
    float* dst = (hi ? g_t : g_v) + o;
    if (r.b >= nu) {
        st4(dst, ld4(g_item_rep + (r.b - nu) * DC + r.c));
        return;
    }
    const float4 g = ld4(g_user_rep + r.b * DC + r.c);
    st4(dst, mul4(w[2 * r.b + hi], g));
    const float dot = group_sum<kHalf>(dot4(g, ld4((hi ? xt : xv) + o)));  // a half of the 32-lane group
    if (r.c == hi * DM) g_w[2 * r.b + hi] = dot;
}

// ---------------------------------------------------------------------------
// the user graph
// ---------------------------------------------------------------------------
// Lane l of a row's group of L = D / 4 lanes holds entries l, l + L, ... of the row's list (4 a
// lane at D = 64, 2 at D = 128); entry j is broadcast from lane j % L of the group.  An index
// outside [0, nu) contributes nothing.
template <int D>
__global__ __launch_bounds__(256) void ugraph_fwd(const float* __restrict__ x, const int32_t* __restrict__ idx,
                                                  const float* __restrict__ W, int64_t nu, int k,
                                                  float* __restrict__ out) {
    constexpr int kL = D / 4, kPer = kMaxK / kL;
    const RowGeom<D> r;
    if (r.b >= nu) return;  // uniform over a row's lane group
    const int gl = threadIdx.x % kL;                  // this lane's place in its group
    const int g0 = (threadIdx.x & (kWave - 1)) - gl;  // the group's first lane in the wave
    int li[kPer];
    float lw[kPer];
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
        const int j = q * kL + gl;
        li[q] = j < k ? idx[r.b * k + j] : -1;
        lw[q] = j < k ? W[r.b * k + j] : 0.f;
    }
    float4 acc = f4(0.f);
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
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
// the loss (dragon.py:262-277)
// ---------------------------------------------------------------------------
constexpr int kPartStride = 4;  // {softplus(-x), |pref_v[u]|^2, |pref_t[u]|^2, -}

struct LossArgs {
    const float *result, *pv, *pt, *wu;
    const int64_t* trip;
    int64_t nu, ni, B;
    float reg_weight;
};

// The preference table a lane of a D-wide row answers for, and its first column there: at
// D = 128 pref_v under c < 64 and pref_t above; at D = 64 the one table given.  which: 0 v, 1 t.
template <int D>
__device__ __forceinline__ const float* pref_of(const LossArgs& a, int c, int& which, int& pc) {
    which = D == DC ? c >= DM : a.pv == nullptr;
    pc = D == DC ? c - which * DM : c;
    return which ? a.pt : a.pv;
}

template <int D>
__device__ __forceinline__ void load_trip(const LossArgs& a, int64_t b, int c, ScoreTrip& t) {
    load_score_trip<D>(
        a.trip, a.B, b, a.nu, a.ni, c, [&](int64_t u, int c) { return ld4(a.result + u * D + c); },
        [&](int64_t i, int c) { return ld4(a.result + (a.nu + i) * D + c); }, t);
}

template <int D>
__global__ __launch_bounds__(256) void loss_rows(LossArgs a, float* __restrict__ part) {
    const RowGeom<D> r;
    float v[3] = {0.f, 0.f, 0.f};
    if (r.b < a.B) {  // uniform over a row's lane group
        ScoreTrip t;
        load_trip<D>(a, r.b, r.c, t);
        v[0] = softplus_neg(t.x);
        if (t.ok) {
            int which, pc;
            const float* p = pref_of<D>(a, r.c, which, pc);
            float sq = 0.f;
            if (p) {
                const float4 x = ld4(p + t.u * DM + pc);
                sq = dot4(x, x);
            }
            // every lane of the group ends with both sums: the lanes of the other table add zeros
            v[1] = group_sum<D / 4>(which ? 0.f : sq);
            v[2] = group_sum<D / 4>(which ? sq : 0.f);
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
    if ((threadIdx.x & (kWave - 1)) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// out = {total, bpr, reg}
__global__ __launch_bounds__(256) void loss_finish(LossArgs a, const float* __restrict__ part, int nblk,
                                                   float* __restrict__ out) {
    __shared__ float sh[4];
    const float su = block_sumsq(a.wu, 2 * a.nu, sh);
    if (threadIdx.x >= kWave) return;
    float term[3];
    sum_partials<3, kPartStride>(part, nblk, term);
    if (threadIdx.x == 0) {
        const float bpr = term[0] / (float)a.B * kInvLn2;
        const float rows = (float)a.B * (float)DM;
        const float reg = a.reg_weight * (term[1] / rows + term[2] / rows) + a.reg_weight * (su / (float)(2 * a.nu));
        out[0] = bpr + reg;
        out[1] = bpr;
        out[2] = reg;
    }
}

// Per triplet b: coef[b] = d total / d x_b (upstream included), occU[b] = coef (p - n), the user
// row's share; occR[b] = the user row (what an item occurrence scales by +-coef[b]); the keys.
template <int D>
__global__ __launch_bounds__(256) void loss_grad_rows(LossArgs a, const float* __restrict__ go,
                                                      float* __restrict__ occU, float* __restrict__ occR,
                                                      float* __restrict__ coef, int32_t* __restrict__ ku,
                                                      int32_t* __restrict__ ki) {
    const RowGeom<D> r;
    const int64_t b = r.b;
    if (b >= a.B) return;  // uniform over a row's lane group
    ScoreTrip t;
    load_trip<D>(a, b, r.c, t);
    const float ck = bpr_coef(t, go, a.B) * kInvLn2;
    st4(occU + b * D + r.c, mul4(ck, sub4(t.pr, t.nr)));
    st4(occR + b * D + r.c, t.ur);
    if (r.c == 0) {
        coef[b] = ck;
        store_keys(t, a.B, b, ku, ki);
    }
}

// The per-destination sums (rsx_triplet.hpp's walk).  G [nu + ni, D], gpv, gpt [nu, 64], all
// zero-filled; a user's walk also counts its occurrences: gp_m[u] = cp count(u) pref_m[u], the
// lanes under c < 64 of a 128-wide walk writing pref_v's row and the others pref_t's.
template <int D>
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
    tree_rows<D / 4>(acc);
#pragma unroll
    for (int o = kWave / 2; o >= D / 4; o >>= 1) cnt += __shfl_xor(cnt, o, kWave);  // counts are exact
    if (w.g != 0) return;
    st4(G + (w.user ? (int64_t)w.key : a.nu + w.key) * D + c, acc);
    if (!w.user) return;
    int which, pc;
    const float* p = pref_of<D>(a, c, which, pc);
    if (!p) return;
    const float cp = 2.f * a.reg_weight * *go / ((float)a.B * (float)DM) * cnt;
    const int64_t o = (int64_t)w.key * DM + pc;
    st4((which ? gpt : gpv) + o, mul4(cp, ld4(p + o)));
}

// g_weight_u = 2 reg_weight / (2 nu) weight_u, times *go
__global__ __launch_bounds__(256) void weight_u_grad(const float* __restrict__ wu, const float* __restrict__ go,
                                                     float cw, int64_t n, float* __restrict__ g) {
    const float c = cw * *go;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) g[i] = c * wu[i];
}

inline TripletWs carve(void* ws, int64_t B, int d) { return carve_triplet(ws, B, d, kPartStride, 1, 1); }

inline int loss_check(const rsx_dragon_loss_args* a, void* ws, size_t ws_bytes, LossArgs& k) {
    if (!a) return RSX_ERR_ARG;
    // 128 wide: the concatenation, either table or both; 64 wide: one modality, its table alone
    const bool tables = a->d == DM ? (a->pref_v != nullptr) != (a->pref_t != nullptr) : (a->pref_v || a->pref_t);
    const bool own_ok = a->result && a->weight_u && a->triplets && ws && tables && aligned16(a->result) &&
                        aligned16(a->pref_v) && aligned16(a->pref_t) && aligned16(ws);
    const int rc = check_triplet(a->batch, a->n_users, a->n_items, a->d, own_ok, ws_bytes,
                                 rsx_dragon_loss_ws_bytes(a->batch, a->d));
    if (rc) return rc;
    if (a->n_users + a->n_items > 0x7fffffffll) return RSX_ERR_UNSUPPORTED;
    k.result = a->result, k.pv = a->pref_v, k.pt = a->pref_t, k.wu = a->weight_u;
    k.trip = a->triplets, k.nu = a->n_users, k.ni = a->n_items, k.B = a->batch, k.reg_weight = a->reg_weight;
    return RSX_OK;
}

template <int D>
void launch_loss_fwd(const LossArgs& k, float* out, void* ws, hipStream_t s) {
    const TripletWs w = carve(ws, k.B, D);
    const int nblk = rows_blocks<D>(k.B);
    hipLaunchKernelGGL(loss_rows<D>, dim3(nblk), dim3(256), 0, s, k, w.part);
    hipLaunchKernelGGL(loss_finish, dim3(1), dim3(256), 0, s, k, (const float*)w.part, nblk, out);
}

template <int D>
void launch_loss_bwd(const LossArgs& k, const float* go, float* G, float* gpv, float* gpt, void* ws, hipStream_t s) {
    const TripletWs w = carve(ws, k.B, D);
    hipLaunchKernelGGL(loss_grad_rows<D>, dim3(rows_blocks<D>(k.B)), dim3(256), 0, s, k, go, w.occU, w.occX, w.coef,
                       w.ku, w.ki);
    launch_walk(loss_sum_rows<D>, k.B, s, k, go, w.occU, w.occX, w.coef, w.ku, w.ki, G, gpv, gpt);
}

}  // namespace dr
}  // namespace rsx

using namespace rsx;

extern "C" {

int rsx_dragon_cat_fwd(const float* xv, const float* xt, const float* weight_u, int64_t n_users, int64_t n_items,
                       float* user_rep, float* item_rep, rsx_stream_t stream) {
    if (n_users < 1 || n_items < 1 || !xv || !xt || !weight_u || !user_rep || !item_rep) return RSX_ERR_ARG;
    if (n_users + n_items > 0x7fffffffll) return RSX_ERR_UNSUPPORTED;
    if (!aligned16(xv) || !aligned16(xt) || !aligned16(user_rep) || !aligned16(item_rep)) return RSX_ERR_ARG;
    const int64_t n = n_users + n_items;
    hipLaunchKernelGGL(dr::cat_fwd, dim3((unsigned)rows_blocks<dr::DC>(n)), dim3(256), 0, as_stream(stream), xv, xt,
                       weight_u, n_users, n, user_rep, item_rep);
    return last_rc();
}

int rsx_dragon_cat_bwd(const float* g_user_rep, const float* g_item_rep, const float* xv, const float* xt,
                       const float* weight_u, int64_t n_users, int64_t n_items, float* g_v, float* g_t,
                       float* g_weight_u, rsx_stream_t stream) {
    if (n_users < 1 || n_items < 1 || !xv || !xt || !g_user_rep || !g_item_rep || !weight_u || !g_v || !g_t ||
        !g_weight_u)
        return RSX_ERR_ARG;
    if (n_users + n_items > 0x7fffffffll) return RSX_ERR_UNSUPPORTED;
    for (const void* p : {(const void*)g_user_rep, (const void*)g_item_rep, (const void*)xv, (const void*)xt,
                          (const void*)g_v, (const void*)g_t})
        if (!aligned16(p)) return RSX_ERR_ARG;
    const int64_t n = n_users + n_items;
    hipLaunchKernelGGL(dr::cat_bwd, dim3((unsigned)rows_blocks<dr::DC>(n)), dim3(256), 0, as_stream(stream), g_user_rep,
                       g_item_rep, xv, xt, weight_u, n_users, n, g_v, g_t, g_weight_u);
    return last_rc();
}

int rsx_dragon_ugraph_fwd(const float* user_rep, const int32_t* idx, const float* W, int64_t n_users, int32_t k,
                          int32_t d, float* out, rsx_stream_t stream) {
    if (n_users < 1 || !user_rep || !idx || !W || !out || out == user_rep || !aligned16(user_rep) || !aligned16(out))
        return RSX_ERR_ARG;
    if ((d != dr::DM && d != dr::DC) || k < 1 || k > dr::kMaxK || n_users > 0x7fffffffll) return RSX_ERR_UNSUPPORTED;
    hipStream_t s = as_stream(stream);
    if (d == dr::DC)
        hipLaunchKernelGGL(dr::ugraph_fwd<dr::DC>, dim3((unsigned)rows_blocks<dr::DC>(n_users)), dim3(256), 0, s,
                           user_rep, idx, W, n_users, (int)k, out);
    else
        hipLaunchKernelGGL(dr::ugraph_fwd<dr::DM>, dim3((unsigned)rows_blocks<dr::DM>(n_users)), dim3(256), 0, s,
                           user_rep, idx, W, n_users, (int)k, out);
    return last_rc();
}

size_t rsx_dragon_loss_ws_bytes(int64_t batch, int32_t d) {
    return triplet_ws_bytes(batch, d, dr::kPartStride, 1, 1);
}

int rsx_dragon_loss_fwd(const rsx_dragon_loss_args* a, float* out, void* ws, size_t ws_bytes, rsx_stream_t stream) {
    dr::LossArgs k;
    const int rc = dr::loss_check(a, ws, ws_bytes, k);
    if (rc) return rc;
    if (!out) return RSX_ERR_ARG;
    if (a->d == dr::DC)
        dr::launch_loss_fwd<dr::DC>(k, out, ws, as_stream(stream));
    else
        dr::launch_loss_fwd<dr::DM>(k, out, ws, as_stream(stream));
    return last_rc();
}

int rsx_dragon_loss_bwd(const rsx_dragon_loss_args* a, const float* go, float* g_result, float* g_pref_v,
                        float* g_pref_t, float* g_weight_u, void* ws, size_t ws_bytes, rsx_stream_t stream) {
    dr::LossArgs k;
    const int rc = dr::loss_check(a, ws, ws_bytes, k);
    if (rc) return rc;
    if (!go || !g_result || !g_weight_u || !aligned16(g_result) || !aligned16(g_pref_v) || !aligned16(g_pref_t))
        return RSX_ERR_ARG;
    if ((k.pv && !g_pref_v) || (k.pt && !g_pref_t)) return RSX_ERR_ARG;
    hipStream_t s = as_stream(stream);
    float* gpv = k.pv ? g_pref_v : nullptr;
    float* gpt = k.pt ? g_pref_t : nullptr;
    const int zrc = zero_tables({{g_result, (size_t)(k.nu + k.ni) * a->d},
                                 {gpv, (size_t)k.nu * dr::DM},
                                 {gpt, (size_t)k.nu * dr::DM}},
                                s);
    if (zrc) return zrc;
    if (a->d == dr::DC)
        dr::launch_loss_bwd<dr::DC>(k, go, g_result, gpv, gpt, ws, s);
    else
        dr::launch_loss_bwd<dr::DM>(k, go, g_result, gpv, gpt, ws, s);
    const int64_t nw = 2 * k.nu;
    const int64_t nb = (nw + 255) / 256;
    hipLaunchKernelGGL(dr::weight_u_grad, dim3((unsigned)(nb < 1024 ? nb : 1024)), dim3(256), 0, s, k.wu, go,
                       2.f * k.reg_weight / (float)(2 * k.nu), nw, g_weight_u);
    return last_rc();
}

}  // extern "C"
