// freedom.hip — FREEDOM's training loss on gfx950, forward and backward.
//
// Replaces, per batch (reference paths relative to its root):
//   src/models/freedom.py:182-212   three BPR terms that share the user row: the id path on
//                                   E[u], E[nu + i] + H[i], and the text / image terms on the
//                                   projected feature tables, weighted by reg_weight
// and their autograd backward (the gathers' index_put scatter-adds).
//
// The protocol (lane-group layout, block partials, keys, the first-occurrence walk, workspace,
// argument checks) is rsx_triplet.hpp's; this file has the three-score triplet and what the
// walk adds: a user row adds the stored contribution rows; an item row adds coefficient *
// E[user] for the id, text and image coefficient of each occurrence in one walk, as all three
// tables share the item's occurrence list.
#include "rsx_triplet.hpp"

namespace rsx {
namespace freedom {

constexpr int kPartStride = 4, kCoef = 3;  // words a block partial, coefficients a triplet

struct Args {
    const float *E, *H, *T, *V;
    const int64_t* trip;
    int64_t nu, ni, B;
    float reg;
};

// One triplet as seen by one lane (its 4 columns): the rows and the three scores
// x_k = sum(u * pos_k) - sum(u * neg_k), k = id, text, image (0 where the table is absent).
// An index outside its table: ok = false, the scores NaN, the rows zero.
template <int D>
struct Trip : TripIdx {
    float4 ur, dp, dt, dv;  // the user row, pos - neg of the id / text / image rows
    float x[3];
};

template <int D>
__device__ __forceinline__ void load_trip(const Args& a, int64_t b, int c, Trip<D>& t) {
    constexpr int L = D / 4;
    load_idx(a.trip, a.B, b, a.nu, a.ni, t);
    t.ur = t.dp = t.dt = t.dv = f4(0.f);
    if (!t.ok) {  // uniform over the row's lane group
        t.x[0] = t.x[1] = t.x[2] = __builtin_nanf("");
        return;
    }
    t.ur = ld4(a.E + t.u * D + c);
    float4 pr = ld4(a.E + (a.nu + t.p) * D + c), nr = ld4(a.E + (a.nu + t.n) * D + c);
    if (a.H) {
        pr = add4(pr, ld4(a.H + t.p * D + c));
        nr = add4(nr, ld4(a.H + t.n * D + c));
    }
    t.x[0] = group_sum<L>(dot4(t.ur, pr)) - group_sum<L>(dot4(t.ur, nr));
    t.dp = sub4(pr, nr);
    t.x[1] = t.x[2] = 0.f;
    if (a.T) {
        pr = ld4(a.T + t.p * D + c), nr = ld4(a.T + t.n * D + c);
        t.x[1] = group_sum<L>(dot4(t.ur, pr)) - group_sum<L>(dot4(t.ur, nr));
        t.dt = sub4(pr, nr);
    }
    if (a.V) {
        pr = ld4(a.V + t.p * D + c), nr = ld4(a.V + t.n * D + c);
        t.x[2] = group_sum<L>(dot4(t.ur, pr)) - group_sum<L>(dot4(t.ur, nr));
        t.dv = sub4(pr, nr);
    }
}

// part[block][k] = sum over the block's triplets, in row order, of softplus(-x_k)
template <int D>
__global__ __launch_bounds__(256) void loss_rows(Args a, float* __restrict__ part) {
    const RowGeom<D> r;
    float v[3] = {0.f, 0.f, 0.f};
    if (r.b < a.B) {  // uniform over a row's lane group
        Trip<D> t;
        load_trip<D>(a, r.b, r.c, t);
        v[0] = softplus_neg(t.x[0]);
        if (a.T) v[1] = softplus_neg(t.x[1]);
        if (a.V) v[2] = softplus_neg(t.x[2]);
    }
    block_partials<D, 3, kPartStride>(r, v, part);
}

// out = {total, id, text, image}: the block partials in index order, then the mean
__global__ __launch_bounds__(64) void finish(const float* __restrict__ part, int nblk, int64_t B, float reg,
                                             float* __restrict__ out) {
    float term[3];
    sum_partials<3, kPartStride>(part, nblk, term);
#pragma unroll
    for (int k = 0; k < 3; ++k) term[k] /= (float)B;
    if (threadIdx.x == 0) {
        out[0] = term[0] + reg * (term[1] + term[2]);
        out[1] = term[0];
        out[2] = term[1];
        out[3] = term[2];
    }
}

// Per triplet b: coef[k B + b] = d total / d x_k (upstream *go included), occU[b] = its
// contribution to the user row, and the keys (store_keys).
template <int D>
__global__ __launch_bounds__(256) void grad_rows(Args a, const float* __restrict__ go, float* __restrict__ occU,
                                                 float* __restrict__ coef, int32_t* __restrict__ ku,
                                                 int32_t* __restrict__ ki) {
    const RowGeom<D> r;
    const int64_t b = r.b;
    const int c = r.c;
    if (b >= a.B) return;  // uniform over a row's lane group
    Trip<D> t;
    load_trip<D>(a, b, c, t);
    float ck[3] = {0.f, 0.f, 0.f};
    if (t.ok) {
        const float w = -*go / (float)a.B;
        ck[0] = w * sigmoid_neg(t.x[0]);
        if (a.T) ck[1] = w * a.reg * sigmoid_neg(t.x[1]);
        if (a.V) ck[2] = w * a.reg * sigmoid_neg(t.x[2]);
    }
    float4 g = mul4(ck[0], t.dp);
    g = fma4(ck[1], t.dt, g);
    g = fma4(ck[2], t.dv, g);
    st4(occU + b * D + c, g);
    if (c == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) coef[k * a.B + b] = ck[k];
        store_keys(t, a.B, b, ku, ki);
    }
}

// The per-destination sums (rsx_triplet.hpp's walk)
template <int D>
__global__ __launch_bounds__(256) void sum_rows(Args a, const float* __restrict__ occU, const float* __restrict__ coef,
                                                const int32_t* __restrict__ ku, const int32_t* __restrict__ ki,
                                                float* __restrict__ gE, float* __restrict__ gT,
                                                float* __restrict__ gV) {
    Walk<D> w;
    if (!w.begin(ku, ki, a.B)) return;
    const int c = w.c;
    const int32_t key = w.key;
    float4 acc[3] = {f4(0.f), f4(0.f), f4(0.f)};
    w.each([&](int64_t occ) { acc[0] = add4(acc[0], ld4(occU + occ * D + c)); },
           [&](int64_t b, float sgn) {
               const float4 u = ld4(a.E + (int64_t)ku[b] * D + c);
               acc[0] = fma4(sgn * coef[b], u, acc[0]);
               if (gT) acc[1] = fma4(sgn * coef[a.B + b], u, acc[1]);
               if (gV) acc[2] = fma4(sgn * coef[2 * a.B + b], u, acc[2]);
           });
#pragma unroll
    for (int k = 0; k < 3; ++k) tree_rows<Walk<D>::L>(acc[k]);
    if (w.g != 0) return;
    if (w.user) {
        st4(gE + (int64_t)key * D + c, acc[0]);
    } else {
        st4(gE + (a.nu + key) * D + c, acc[0]);
        if (gT) st4(gT + (int64_t)key * D + c, acc[1]);
        if (gV) st4(gV + (int64_t)key * D + c, acc[2]);
    }
}

inline TripletWs carve(void* ws, int64_t B, int d) { return carve_triplet(ws, B, d, kPartStride, kCoef); }

inline int check(const rsx_freedom_args* a, void* ws, size_t ws_bytes, Args& k) {
    if (!a) return RSX_ERR_ARG;
    const bool own_ok = a->E && a->triplets && ws && (a->T || a->V) && aligned16(a->E) && aligned16(a->H) &&
                        aligned16(a->T) && aligned16(a->V) && aligned16(ws);
    const int rc = check_triplet(a->batch, a->n_users, a->n_items, a->d, own_ok, ws_bytes,
                                 rsx_freedom_ws_bytes(a->batch, a->d));
    if (rc) return rc;
    k.E = a->E, k.H = a->H, k.T = a->T, k.V = a->V, k.trip = a->triplets;
    k.nu = a->n_users, k.ni = a->n_items, k.B = a->batch, k.reg = a->reg;
    return RSX_OK;
}

template <int D>
int fwd(const Args& k, float* out, void* ws, hipStream_t s) {
    const TripletWs w = carve(ws, k.B, D);
    const int nblk = rows_blocks<D>(k.B);
    hipLaunchKernelGGL(loss_rows<D>, dim3(nblk), dim3(256), 0, s, k, w.part);
    hipLaunchKernelGGL(finish, dim3(1), dim3(64), 0, s, (const float*)w.part, nblk, k.B, k.reg, out);
    return last_rc();
}

template <int D>
int bwd(const Args& k, const float* go, float* gE, float* gT, float* gV, void* ws, hipStream_t s) {
    const TripletWs w = carve(ws, k.B, D);
    const size_t items = (size_t)k.ni * D;
    // every row is written: zero off the batch
    const int rc = zero_tables({{gE, (size_t)(k.nu + k.ni) * D}, {gT, items}, {gV, items}}, s);
    if (rc) return rc;
    hipLaunchKernelGGL(grad_rows<D>, dim3(rows_blocks<D>(k.B)), dim3(256), 0, s, k, go, w.occU, w.coef, w.ku, w.ki);
    launch_walk(sum_rows<D>, k.B, s, k, w.occU, w.coef, w.ku, w.ki, gE, gT, gV);
    return last_rc();
}

}  // namespace freedom
}  // namespace rsx

using namespace rsx;

extern "C" size_t rsx_freedom_ws_bytes(int64_t batch, int32_t d) {
    return triplet_ws_bytes(batch, d, freedom::kPartStride, freedom::kCoef);
}

extern "C" int rsx_freedom_loss_fwd(const rsx_freedom_args* a, float* out, void* ws, size_t ws_bytes,
                                    rsx_stream_t stream) {
    freedom::Args k;
    const int rc = freedom::check(a, ws, ws_bytes, k);
    if (rc) return rc;
    if (!out) return RSX_ERR_ARG;
    hipStream_t s = as_stream(stream);
    return a->d == 64 ? freedom::fwd<64>(k, out, ws, s) : freedom::fwd<128>(k, out, ws, s);
}

extern "C" int rsx_freedom_loss_bwd(const rsx_freedom_args* a, const float* go, float* gE, float* gT, float* gV,
                                    void* ws, size_t ws_bytes, rsx_stream_t stream) {
    freedom::Args k;
    const int rc = freedom::check(a, ws, ws_bytes, k);
    if (rc) return rc;
    if (!go || !gE || (a->T && !gT) || (a->V && !gV)) return RSX_ERR_ARG;
    if (!aligned16(gE) || !aligned16(gT) || !aligned16(gV)) return RSX_ERR_ARG;
    hipStream_t s = as_stream(stream);
    gT = a->T ? gT : nullptr;
    gV = a->V ? gV : nullptr;
    return a->d == 64 ? freedom::bwd<64>(k, go, gE, gT, gV, ws, s) : freedom::bwd<128>(k, go, gE, gT, gV, ws, s);
}
