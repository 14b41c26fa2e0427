// selfcf.hip — SELFCFED_LGN (SelfCF with embedding dropout on a LightGCN encoder) on gfx950:
// the per-step dropped graph, the bootstrap loss forward and backward, the evaluation tables.
//
// Replaces, per batch (reference paths relative to its root):
//   src/common/encoders.py:80-96      sparse_dropout: a rate drawn uniformly in [0, 1), each of the
//                                     2 E directed entries kept independently, survivors * 1/(1 - rate)
//   src/models/selfcfed_lgn.py:41-69  F.dropout of the gathered batch rows (targets), the predictor,
//                                     the two halved cosine terms, L2Loss over the batch's rows
//   src/models/selfcfed_lgn.py:52-78  get_embedding / full_sort_predict's two-term score
// and their autograd backward.
//
// The dropped graph.  The structure (rowptr, col) never changes; one launch rewrites the two value
//   buffers of A and A^T: val[e] = keep(e) ? val0[e] * scale : 0 and valT[rev[e]] = val[e], rev the
//   reverse-slot permutation (every slot written exactly once: vector stores, no atomics).  keep(e)
//   and the rate are hashes of a device seed word (a captured step replays with a fresh draw), or an
//   explicit packed mask and scale word (tests replay a recorded draw).
// The loss.  Dropout is keyed on the BATCH POSITION (the reference drops the gathered [B, d] rows):
//   two occurrences of a table row see independent masks, unlike bm3.hip.  The online rows are read
//   from E through the index list (rsx_linear_rows_fwd's rows argument too: no gathered copy);
//   block partials in row order, one wave adds them in index order.  The backward sums, per
//   destination row, (G P)_b + reg_weight x_b over the row's occurrences with rsx_triplet.hpp's
//   first-occurrence walk: a pair batch is a triplet batch whose third key row is -1.
#include "rsx_triplet.hpp"

namespace rsx {
namespace selfcf {

constexpr float kCosEps = 1e-8f;  // torch.nn.functional.cosine_similarity's eps
constexpr int kPartStride = 4;    // words a block partial: cos ui, cos iu, l2
enum { S_USER = 0, S_ITEM = 1, S_EDGE = 2, S_RATE = 3 };  // hash streams

__device__ __forceinline__ uint32_t mix32(uint64_t x) {  // smore_fld.hpp's
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdULL;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ULL;
    x ^= x >> 33;
    return (uint32_t)x;
}
__device__ __forceinline__ uint32_t draw(uint64_t seed, int stream, uint64_t i) {
    return mix32(seed * 0x9E3779B97F4A7C15ULL + ((uint64_t)stream << 58) + i);
}

// ---------------------------------------------------------------------------
// the per-step dropped graph
// ---------------------------------------------------------------------------
// One lane a slot.  Hashed (mask == nullptr): rate = the top 24 bits of a draw over 2^24, so
// rate 2^32 is an integer threshold and 1 - rate is exact in f32.  info = {rate, scale}.
__global__ __launch_bounds__(256) void edge_drop(const float* __restrict__ val0, const int32_t* __restrict__ rev,
                                                 int64_t nnz, const int64_t* __restrict__ seed,
                                                 const uint32_t* __restrict__ mask, const float* __restrict__ scale_in,
                                                 float* __restrict__ val, float* __restrict__ valT,
                                                 float* __restrict__ info) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float rate, scale;
    bool keep = false;
    if (mask) {
        scale = *scale_in;
        rate = 1.f - 1.f / scale;
        if (e < nnz) keep = (mask[e >> 5] >> (e & 31)) & 1u;
    } else {
        const uint64_t s = (uint64_t)*seed;
        const uint32_t r24 = draw(s, S_RATE, 0) >> 8;
        rate = (float)r24 * (1.f / 16777216.f);
        scale = 1.f / (1.f - rate);
        if (e < nnz) keep = draw(s, S_EDGE, (uint64_t)e) >= (r24 << 8);
    }
    if (e == 0) {
        info[0] = rate;
        info[1] = scale;
    }
    if (e >= nnz) return;
    const float v = keep ? val0[e] * scale : 0.f;
    val[e] = v;
    const int64_t r = rev[e];
    if (r >= 0 && r < nnz) valT[r] = v;  // rev is a permutation of the slots (checked where it is built)
}

// ---------------------------------------------------------------------------
// the loss
// ---------------------------------------------------------------------------
struct Args {
    int64_t nu, ni, B;
    const float* E;
    const int64_t *users, *items;
    const int64_t* seed;
    const uint32_t* mask;  // [2, B, D / 32] or null
    float p_drop, scale, reg;
    // workspace pieces
    int64_t* rows;  // [2 B]: users, nu + items (0 for a pair with an index outside its table)
    int32_t *ku, *ki;  // the walk's keys: users [B], items [2 B] = [items; -1]
    float *Q, *G, *dX;  // [2 B, D]: predicted rows, their gradients, the online rows' gradients
};

__device__ __forceinline__ float4 mul44(float4 a, float4 b) {
    return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w);
}

// keep-scale (0 or 1 / (1 - p)) of columns c .. c + 3 of batch position b of stream s
template <int D>
__device__ __forceinline__ float4 keep4(const Args& a, int s, int64_t b, int c) {
    float k[4];
    if (a.mask) {
        const uint32_t w = a.mask[((int64_t)s * a.B + b) * (D / 32) + (c >> 5)] >> (c & 31);
#pragma unroll
        for (int r = 0; r < 4; ++r) k[r] = ((w >> r) & 1u) ? a.scale : 0.f;
    } else if (a.p_drop > 0.f) {
        const uint64_t seed = (uint64_t)*a.seed;
        const uint32_t thr = (uint32_t)fminf(a.p_drop * 4294967296.f, 4294967295.f);
#pragma unroll
        for (int r = 0; r < 4; ++r) k[r] = draw(seed, s, (uint64_t)b * D + (uint64_t)(c + r)) >= thr ? a.scale : 0.f;
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) k[r] = 1.f;
    }
    return make_float4(k[0], k[1], k[2], k[3]);
}

// the batch's row list and keys: a thread a pair
__global__ __launch_bounds__(256) void prep(Args a) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= a.B) return;
    const int64_t u = a.users[b], i = a.items[b];
    const bool ok = u >= 0 && u < a.nu && i >= 0 && i < a.ni;
    a.rows[b] = ok ? u : 0;
    a.rows[a.B + b] = ok ? a.nu + i : 0;
    a.ku[b] = ok ? (int32_t)u : -1;
    a.ki[b] = ok ? (int32_t)i : -1;
    a.ki[a.B + b] = -1;
}

// What one pair needs of both passes (the lane's 4 columns): online rows x, predicted rows q,
// targets t, and the squared norms over the row.
struct Pair {
    bool ok;
    float4 xu, xi, qu, qi, tu, ti;
    float quu, qii, tuu, tii;
};
template <int D>
__device__ __forceinline__ void load_pair(const Args& a, int64_t b, int c, Pair& p) {
    constexpr int L = D / 4;
    p.ok = a.ku[b] >= 0;
    p.xu = ld4(a.E + a.rows[b] * D + c);
    p.xi = ld4(a.E + a.rows[a.B + b] * D + c);
    p.qu = ld4(a.Q + b * D + c);
    p.qi = ld4(a.Q + (a.B + b) * D + c);
    p.tu = mul44(p.xu, keep4<D>(a, S_USER, b, c));
    p.ti = mul44(p.xi, keep4<D>(a, S_ITEM, b, c));
    p.quu = group_sum<L>(dot4(p.qu, p.qu));
    p.qii = group_sum<L>(dot4(p.qi, p.qi));
    p.tuu = group_sum<L>(dot4(p.tu, p.tu));
    p.tii = group_sum<L>(dot4(p.ti, p.ti));
}

// cos(q, t) = q . t / (max(|q|, eps) max(|t|, eps)): an all-dropped target gives 0
template <int L>
__device__ __forceinline__ float cosine(float4 q, float4 t, float qq, float tt) {
    return group_sum<L>(dot4(q, t)) / (fmaxf(sqrtf(qq), kCosEps) * fmaxf(sqrtf(tt), kCosEps));
}

// part[block] = {sum cos(q_u, t_i), sum cos(q_i, t_u), sum 1/2 (|x_u|^2 + |x_i|^2)} in row order
template <int D>
__global__ __launch_bounds__(256) void loss_rows(Args a, float* __restrict__ part) {
    constexpr int L = RowGeom<D>::L;
    const RowGeom<D> r;
    float v[3] = {0.f, 0.f, 0.f};
    if (r.b < a.B) {  // uniform over a row's lane group
        Pair p;
        load_pair<D>(a, r.b, r.c, p);
        v[0] = cosine<L>(p.qu, p.ti, p.quu, p.tii);
        v[1] = cosine<L>(p.qi, p.tu, p.qii, p.tuu);
        v[2] = 0.5f * (group_sum<L>(dot4(p.xu, p.xu)) + group_sum<L>(dot4(p.xi, p.xi)));
        if (!p.ok) v[0] = v[1] = v[2] = __builtin_nanf("");
    }
    block_partials<D, 3, kPartStride>(r, v, part);
}

// out = {total, ui, iu, reg}: ui = -mean cos(q_u, t_i) / 2, iu likewise, reg the batch L2 (unweighted)
__global__ __launch_bounds__(64) void finish(const float* __restrict__ part, int nblk, int64_t B, float reg_weight,
                                             float* __restrict__ out) {
    float term[3];
    sum_partials<3, kPartStride>(part, nblk, term);
    if (threadIdx.x == 0) {
        const float ui = -(term[0] / (float)B) / 2.f, iu = -(term[1] / (float)B) / 2.f;
        out[0] = (ui + iu) + reg_weight * term[2];
        out[1] = ui;
        out[2] = iu;
        out[3] = term[2];
    }
}

// out[s B + b] = the dropout target of stream s of batch position b
template <int D>
__global__ __launch_bounds__(256) void targets(Args a, float* __restrict__ out) {
    const RowGeom<D> r;
    if (r.b >= 2 * a.B) return;
    const int s = r.b >= a.B ? S_ITEM : S_USER;
    const int64_t b = r.b - (s ? a.B : 0);
    float4 x = ld4(a.E + a.rows[r.b] * D + r.c);
    if (a.ku[b] < 0) x = f4(__builtin_nanf(""));
    st4(out + r.b * D + r.c, mul44(x, keep4<D>(a, s, b, r.c)));
}

// w d cos(q, t) / dq: with n = max(|q|, eps), tn = max(|t|, eps), c = q . t / (n tn):
// t / (n tn) - (c / n) q / |q|  (the clamp is outside autograd, as torch's)
template <int L>
__device__ __forceinline__ float4 cos_grad(float4 q, float4 t, float qq, float tt, float w) {
    const float qn = sqrtf(qq), n = fmaxf(qn, kCosEps), tn = fmaxf(sqrtf(tt), kCosEps);
    const float c = group_sum<L>(dot4(q, t)) / (n * tn);
    const float wa = w / (n * tn), wb = qn > 0.f ? -w * c / (n * qn) : 0.f;
    return fma4(wb, q, mul4(wa, t));
}

// G[b], G[B + b] = d loss / d (predicted user / item row of pair b), upstream *go included;
// zero rows for a pair with an index outside its table
template <int D>
__global__ __launch_bounds__(256) void cos_bwd(Args a, const float* __restrict__ go) {
    constexpr int L = RowGeom<D>::L;
    const RowGeom<D> r;
    if (r.b >= a.B) return;  // uniform over a row's lane group
    Pair p;
    load_pair<D>(a, r.b, r.c, p);
    const float w = -*go / (2.f * (float)a.B);
    float4 gu = cos_grad<L>(p.qu, p.ti, p.quu, p.tii, w), gi = cos_grad<L>(p.qi, p.tu, p.qii, p.tuu, w);
    if (!p.ok) gu = gi = f4(0.f);
    st4(a.G + r.b * D + r.c, gu);
    st4(a.G + (a.B + r.b) * D + r.c, gi);
}

__global__ __launch_bounds__(256) void transpose_dd(const float* __restrict__ P, int d, float* __restrict__ PT) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < d * d) PT[(t % d) * d + t / d] = P[t];
}

// gE[row] = sum over the row's occurrences b of dX[b] + go reg_weight x (rsx_triplet.hpp's walk;
// the third key row is -1: its waves have nothing to sum)
template <int D>
__global__ __launch_bounds__(256) void sum_rows(Args a, const float* __restrict__ go, float* __restrict__ gE) {
    constexpr int L = Walk<D>::L;
    Walk<D> w;
    if (!w.begin(a.ku, a.ki, a.B)) return;
    const int c = w.c;
    float* dst = gE + ((w.user ? 0 : a.nu) + (int64_t)w.key) * D + c;
    const float4 sp = mul4(*go * a.reg, ld4(a.E + ((w.user ? 0 : a.nu) + (int64_t)w.key) * D + c));
    float4 acc = f4(0.f);
    w.each([&](int64_t occ) { acc = add4(acc, add4(ld4(a.dX + occ * D + c), sp)); },
           [&](int64_t b, float) { acc = add4(acc, add4(ld4(a.dX + (a.B + b) * D + c), sp)); });
    tree_rows<L>(acc);
    if (w.g == 0) st4(dst, acc);
}

// the workspace: the block partials, the keys, the row list, Q, G, dX [2 B, d], P^T [d, d],
// rsx_linear_rows_wgrad's workspace; every size grows with B
struct Ws {
    float *part, *Q, *G, *dX, *PT;
    int64_t* rows;
    int32_t *ku, *ki;
    void* wg;
    size_t wg_bytes, total;
};
inline Ws carve(void* ws, int64_t B, int d) {
    Ws w;
    Carver cv(ws);
    const int rpb = 256 / (d / 4);
    const size_t rows = (size_t)2 * (size_t)B * d * sizeof(float);
    w.part = cv.take<float>((size_t)((B + rpb - 1) / rpb) * kPartStride * sizeof(float));
    w.ku = cv.take<int32_t>((size_t)B * sizeof(int32_t));  // key lists: 256-byte aligned and padded (match256)
    w.ki = cv.take<int32_t>((size_t)2 * B * sizeof(int32_t));
    w.rows = cv.take<int64_t>((size_t)2 * B * sizeof(int64_t));
    w.Q = cv.take<float>(rows);
    w.G = cv.take<float>(rows);
    w.dX = cv.take<float>(rows);
    w.PT = cv.take<float>((size_t)d * d * sizeof(float));
    w.wg_bytes = rsx_linear_rows_wgrad_ws_bytes(2 * B, d, d);
    w.wg = cv.take<void>(w.wg_bytes);
    w.total = cv.total();
    return w;
}

inline int check(const rsx_selfcf_args* a, Args& k) {
    if (!a || a->batch < 1 || a->n_users < 1 || a->n_items < 1) return RSX_ERR_ARG;
    if (a->d != 64 && a->d != 128) return RSX_ERR_UNSUPPORTED;
    if (!a->E || !a->P || !a->pb || !a->users || !a->items || !a->ws) return RSX_ERR_ARG;
    if (!aligned16(a->E) || !aligned16(a->ws)) return RSX_ERR_ARG;
    if (!(a->p_drop >= 0.f && a->p_drop < 1.f)) return RSX_ERR_ARG;
    if (a->p_drop > 0.f && !a->seed && !a->mask) return RSX_ERR_ARG;  // a hashed stream needs the seed
    // the keys are int32; the walk over them is quadratic in the batch
    if (a->batch > kMaxBatch || a->n_users > 0x7fffffffll || a->n_items > 0x7fffffffll) return RSX_ERR_UNSUPPORTED;
    if (a->ws_bytes < rsx_selfcf_ws_bytes(a->batch, a->d)) return RSX_ERR_WORKSPACE;
    const Ws w = carve(a->ws, a->batch, a->d);
    k.nu = a->n_users, k.ni = a->n_items, k.B = a->batch;
    k.E = a->E, k.users = a->users, k.items = a->items, k.seed = a->seed, k.mask = a->mask;
    k.p_drop = a->p_drop, k.reg = a->reg_weight;
    k.scale = a->p_drop > 0.f ? (float)(1.0 / (1.0 - (double)a->p_drop)) : 1.f;
    k.rows = w.rows, k.ku = w.ku, k.ki = w.ki, k.Q = w.Q, k.G = w.G, k.dX = w.dX;
    return RSX_OK;
}

// the row list, the keys and the predicted rows: what the loss, the targets and the backward read
template <int D>
int predict(const rsx_selfcf_args* a, const Args& k, hipStream_t s) {
    hipLaunchKernelGGL(prep, dim3((unsigned)((k.B + 255) / 256)), dim3(256), 0, s, k);
    return rsx_linear_rows_fwd(k.E, a->P, a->pb, k.rows, 2 * k.B, D, D, k.Q, D, (rsx_stream_t)s);
}

template <int D>
int fwd(const rsx_selfcf_args* a, const Args& k, float* out, hipStream_t s) {
    const Ws w = carve(a->ws, k.B, D);
    const int rc = predict<D>(a, k, s);
    if (rc) return rc;
    const int nblk = rows_blocks<D>(k.B);
    hipLaunchKernelGGL(loss_rows<D>, dim3(nblk), dim3(256), 0, s, k, w.part);
    hipLaunchKernelGGL(finish, dim3(1), dim3(64), 0, s, (const float*)w.part, nblk, k.B, k.reg, out);
    return last_rc();
}

template <int D>
int tgt(const rsx_selfcf_args* a, const Args& k, float* out, hipStream_t s) {
    const int rc = predict<D>(a, k, s);
    if (rc) return rc;
    hipLaunchKernelGGL(targets<D>, dim3(rows_blocks<D>(2 * k.B)), dim3(256), 0, s, k, out);
    return last_rc();
}

template <int D>
int bwd(const rsx_selfcf_args* a, const Args& k, const float* go, float* gE, float* gP, float* gpb, hipStream_t s) {
    const Ws w = carve(a->ws, k.B, D);
    int rc = zero_tables({{gE, (size_t)(k.nu + k.ni) * D}}, s);
    if (rc) return rc;
    hipLaunchKernelGGL(cos_bwd<D>, dim3(rows_blocks<D>(k.B)), dim3(256), 0, s, k, go);
    hipLaunchKernelGGL(transpose_dd, dim3((D * D + 255) / 256), dim3(256), 0, s, a->P, D, w.PT);
    rc = rsx_linear_rows_fwd(w.G, w.PT, nullptr, nullptr, 2 * k.B, D, D, w.dX, D, (rsx_stream_t)s);
    if (rc) return rc;
    rc = rsx_linear_rows_wgrad(w.G, D, k.E, k.rows, 2 * k.B, D, D, gP, gpb, w.wg, w.wg_bytes, (rsx_stream_t)s);
    if (rc) return rc;
    launch_walk(sum_rows<D>, k.B, s, k, go, gE);
    return last_rc();
}

// UC[u] = [. | E[u]], IC[i] = [E[nu + i] | .]: the halves the predictor's product does not write
template <int D>
__global__ __launch_bounds__(256) void place(const float* __restrict__ E, int64_t nu, int64_t ni,
                                             float* __restrict__ UC, float* __restrict__ IC) {
    const RowGeom<D> r;
    if (r.b >= nu + ni) return;
    const float4 x = ld4(E + r.b * D + r.c);
    if (r.b < nu)
        st4(UC + r.b * 2 * D + D + r.c, x);
    else
        st4(IC + (r.b - nu) * 2 * D + r.c, x);
}

template <int D>
int eval_tables(const float* E, const float* P, const float* pb, int64_t nu, int64_t ni, float* UC, float* IC,
                hipStream_t s) {
    int rc = rsx_linear_rows_fwd(E, P, pb, nullptr, nu, D, D, UC, 2 * D, (rsx_stream_t)s);
    if (rc) return rc;
    rc = rsx_linear_rows_fwd(E + nu * D, P, pb, nullptr, ni, D, D, IC + D, 2 * D, (rsx_stream_t)s);
    if (rc) return rc;
    hipLaunchKernelGGL(place<D>, dim3(rows_blocks<D>(nu + ni)), dim3(256), 0, s, E, nu, ni, UC, IC);
    return last_rc();
}

}  // namespace selfcf
}  // namespace rsx

using namespace rsx;

extern "C" int rsx_selfcf_edge_drop(const float* val0, const int32_t* rev, int64_t nnz, const int64_t* seed,
                                    const uint32_t* keep_mask, const float* scale, float* val, float* valT,
                                    float* info, rsx_stream_t stream) {
    if (nnz < 0 || !val0 || !rev || !val || !valT || !info) return RSX_ERR_ARG;
    if (val == val0 || valT == val0 || val == valT) return RSX_ERR_ARG;
    if (keep_mask ? !scale : !seed) return RSX_ERR_ARG;  // a replayed mask comes with its scale; a hashed draw needs the seed
    if (nnz >= (int64_t)1 << 31) return RSX_ERR_UNSUPPORTED;  // the slots are int32
    if (nnz == 0) return RSX_OK;
    hipLaunchKernelGGL(selfcf::edge_drop, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, as_stream(stream), val0,
                       rev, nnz, seed, keep_mask, scale, val, valT, info);
    return last_rc();
}

extern "C" size_t rsx_selfcf_ws_bytes(int64_t batch, int32_t d) {
    if (batch < 1 || batch > kMaxBatch || (d != 64 && d != 128)) return 0;
    return selfcf::carve(nullptr, batch, d).total;
}

extern "C" int rsx_selfcf_loss_fwd(const rsx_selfcf_args* a, float* out, rsx_stream_t stream) {
    selfcf::Args k;
    const int rc = selfcf::check(a, k);
    if (rc) return rc;
    if (!out) return RSX_ERR_ARG;
    hipStream_t s = as_stream(stream);
    return a->d == 64 ? selfcf::fwd<64>(a, k, out, s) : selfcf::fwd<128>(a, k, out, s);
}

extern "C" int rsx_selfcf_targets(const rsx_selfcf_args* a, float* out, rsx_stream_t stream) {
    selfcf::Args k;
    const int rc = selfcf::check(a, k);
    if (rc) return rc;
    if (!out || !aligned16(out)) return RSX_ERR_ARG;
    hipStream_t s = as_stream(stream);
    return a->d == 64 ? selfcf::tgt<64>(a, k, out, s) : selfcf::tgt<128>(a, k, out, s);
}

extern "C" int rsx_selfcf_loss_bwd(const rsx_selfcf_args* a, const float* go, float* gE, float* gP, float* gpb,
                                   rsx_stream_t stream) {
    selfcf::Args k;
    const int rc = selfcf::check(a, k);
    if (rc) return rc;
    if (!go || !gE || !gP || !gpb || !aligned16(gE)) return RSX_ERR_ARG;
    hipStream_t s = as_stream(stream);
    return a->d == 64 ? selfcf::bwd<64>(a, k, go, gE, gP, gpb, s) : selfcf::bwd<128>(a, k, go, gE, gP, gpb, s);
}

extern "C" int rsx_selfcf_eval_tables(const float* E, const float* P, const float* pb, int64_t n_users,
                                      int64_t n_items, int32_t d, float* UC, float* IC, rsx_stream_t stream) {
    if (n_users < 1 || n_items < 1) return RSX_ERR_ARG;
    if (d != 64 && d != 128) return RSX_ERR_UNSUPPORTED;
    if (!E || !P || !pb || !UC || !IC || UC == IC || !aligned16(E) || !aligned16(UC) || !aligned16(IC))
        return RSX_ERR_ARG;
    hipStream_t s = as_stream(stream);
    return d == 64 ? selfcf::eval_tables<64>(E, P, pb, n_users, n_items, UC, IC, s)
                   : selfcf::eval_tables<128>(E, P, pb, n_users, n_items, UC, IC, s);
}
