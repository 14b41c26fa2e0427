// mmgcn.hip — MMGCN's own kernels on gfx950 (f32 MFMA: exact f32 products, f32 sums), forward
// and backward: the fused layer, the loss and `result`.  Reference: src/models/mmgcn.py, the
// concatenating branch, three layers.
//
// Per modality and layer, on a = A_hat x (the mean operator, an SpMM outside this file):
//   h = leaky(a Wc)   u = leaky(x Wl^T + bl)   x_hat = u + E   out = leaky([h | x_hat] Wg^T + bg)
// Layer 1 (width 256 or the text feature width), the image MLP, F.normalize and the bias
// gradients run on the shared dense blocks of dense.hip; leaky and its slope mask are
// smore_fld.hpp's.
//
//  * layer_fwd / layer_bwd (layers 2 and 3, width D = d in {64, 128}): the whole chain of a
//    16-row tile in a wave's registers, in the row-field layout of smore_fld.hpp, the four
//    D x D weights (Wc [in, out], Wl, and the two halves of Wg [D, 2 D]) staged in LDS.  At
//    D = 64 the four copies (70 KB) stay resident and a block strides over its 64-row blocks;
//    at D = 128 one copy fits beside a second block, so the weights are restaged per row block
//    (as mgcn.hip's fuser does).  The backward writes g_a, the direct part of g_x, and the
//    three pre-activation gradient rows and x_hat for the weight gradients (rsx_smore_wgrad).
//  * the loss (rsx_triplet.hpp's protocol: one-score triplet, block partials, keys, walk,
//    workspace, checks; its own: the rep row and the id regulariser) and the whole-table
//    `result` (write_result).
//
// Slopes are read off the sign of the saved f32 outputs (leaky(p) > 0 exactly when p > 0, the
// slope being positive): no mask tensors.  No float atomics anywhere: two runs are bit-equal.
#include <cmath>

#include "rsx_triplet.hpp"
#include "smore_fld.hpp"

namespace rsx {
namespace mm {

using namespace rsx::sf;

struct Add {
    __device__ float operator()(float a, float b) const { return a + b; }
};
constexpr Add add{};

// ---------------------------------------------------------------------------
// the fused layer (w = d)
// ---------------------------------------------------------------------------
struct LayerArgs {
    const float *Wc, *Wl, *bl, *Wg, *bg;  // Wc [D, D] (in, out); Wl [D, D]; Wg [D, 2 D]
    const float *a, *x, *E;               // forward inputs [n, D]
    float *h, *u, *out;                   // forward outputs (the backward reads them back)
    const float* g_out;                   // backward input
    float *go, *gh, *gu, *xh, *g_a, *g_x;  // backward outputs
    int64_t n, nbx;
};

__device__ __forceinline__ int64_t tile_row(int64_t bx, int64_t n) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (bx * 4 + (threadIdx.x >> 6)) * 16 + (lane & 15);
    return r < n ? r : (int64_t)-1;
}

// stage_w for a [D, D] block of a wider matrix (row stride ldw floats)
template <int D>
__device__ __forceinline__ const float* stage_ld(float* __restrict__ lds, const float* __restrict__ W, int64_t ldw) {
    static_assert(D % 64 == 0, "stage_ld: rows of whole 64-float pieces");
    __syncthreads();  // the previous weight's readers are done
    constexpr int PR = D / 64;
    const int lane = threadIdx.x & 63;
    const int nw = blockDim.x >> 6;
    for (int pc = threadIdx.x >> 6; pc < D * PR; pc += nw) {  // wave-uniform
        const int row = pc / PR, c0 = (pc - row * PR) * 64;
        __builtin_amdgcn_global_load_lds(W + (int64_t)row * ldw + c0 + lane, lds + row * kLd<D> + c0, 4, 0, 0);
    }
    __syncthreads();  // (waits for the DMA: vmcnt(0) before the barrier)
    return lds;
}

// The four weights of a layer: Wc, Wl, Wg[:, :D], Wg[:, D:].  kRes: all four resident in LDS
// (staged once by stage_all); else weight i is staged into the one copy when asked for.  Every
// thread of the block calls these in the same order.
template <int D>
struct Weights {
    static constexpr bool kRes = D == 64;
    static constexpr int kCopies = kRes ? 4 : 1;
    float* lds;
    const float* src[4];
    int64_t ld[4];
    __device__ __forceinline__ Weights(float* l, const LayerArgs& a) : lds(l) {
        src[0] = a.Wc, src[1] = a.Wl, src[2] = a.Wg, src[3] = a.Wg + D;
        ld[0] = ld[1] = D, ld[2] = ld[3] = 2 * D;
    }
    __device__ __forceinline__ void stage_all() {
        if (kRes)
#pragma unroll
            for (int i = 0; i < 4; ++i) stage_ld<D>(lds + i * D * kLd<D>, src[i], ld[i]);
    }
    __device__ __forceinline__ const float* get(int i) {
        if (kRes) return lds + i * D * kLd<D>;
        return stage_ld<D>(lds, src[i], ld[i]);
    }
};

template <int D>
__global__ __launch_bounds__(256) void layer_fwd(LayerArgs a) {
    __shared__ __attribute__((aligned(16))) float wl[Weights<D>::kCopies * D * kLd<D>];
    const int lane = threadIdx.x & 63, g = lane >> 4;
    Weights<D> W(wl, a);
    W.stage_all();
#pragma unroll 1
    for (int64_t bx = blockIdx.x; bx < a.nbx; bx += gridDim.x) {  // block-uniform
        const int64_t row = tile_row(bx, a.n);
        const Fld<D> h = fmap<D>(mvt_p<D, kLd<D>>(W.get(0), fload<D>(a.a, row, g), lane), leaky);
        fstore<D>(a.h, row, g, h);
        const Fld<D> u = fmap<D>(mv_p<D, kLd<D>>(W.get(1), a.bl, fload<D>(a.x, row, g), lane), leaky);
        fstore<D>(a.u, row, g, u);
        const Fld<D> xh = fmap2<D>(u, fload<D>(a.E, row, g), add);
        Fld<D> o = mv_p<D, kLd<D>>(W.get(2), a.bg, h, lane);
        o = fmap2<D>(o, mv_p<D, kLd<D>>(W.get(3), nullptr, xh, lane), add);
        fstore<D>(a.out, row, g, fmap<D>(o, leaky));
    }
}

// go = g_out .* slope(out);  [g_h | g_xh] = go Wg;  gh = g_h .* slope(h);  gu = g_xh .* slope(u);
// g_a = gh Wc^T;  g_x = gu Wl (the part through the Linear; the caller adds A_hat^T g_a)
template <int D>
__global__ __launch_bounds__(256) void layer_bwd(LayerArgs a) {
    __shared__ __attribute__((aligned(16))) float wl[Weights<D>::kCopies * D * kLd<D>];
    const int lane = threadIdx.x & 63, g = lane >> 4;
    Weights<D> W(wl, a);
    W.stage_all();
#pragma unroll 1
    for (int64_t bx = blockIdx.x; bx < a.nbx; bx += gridDim.x) {  // block-uniform
        const int64_t row = tile_row(bx, a.n);
        const Fld<D> go = fmap2<D>(fload<D>(a.g_out, row, g), fload<D>(a.out, row, g), mul_slope);
        fstore<D>(a.go, row, g, go);
        const Fld<D> gh = fmap2<D>(mvt_p<D, kLd<D>>(W.get(2), go, lane), fload<D>(a.h, row, g), mul_slope);
        fstore<D>(a.gh, row, g, gh);
        const Fld<D> u = fload<D>(a.u, row, g);
        const Fld<D> gu = fmap2<D>(mvt_p<D, kLd<D>>(W.get(3), go, lane), u, mul_slope);
        fstore<D>(a.gu, row, g, gu);
        fstore<D>(a.xh, row, g, fmap2<D>(u, fload<D>(a.E, row, g), add));
        fstore<D>(a.g_x, row, g, mvt_p<D, kLd<D>>(W.get(1), gu, lane));
        fstore<D>(a.g_a, row, g, mv_p<D, kLd<D>>(W.get(0), nullptr, gh, lane));
    }
}

// ---------------------------------------------------------------------------
// the loss (mmgcn.py:79-97) and `result`
// ---------------------------------------------------------------------------
constexpr int kPartStride = 2;

struct LossArgs {
    const float *xv, *xt, *E;
    const int64_t* trip;
    int64_t nu, ni, B;
    float inv_m, reg_weight, pref_term;
};

// rep row: (x_v + x_t) / num_modal (either table may be absent)
template <int D>
__device__ __forceinline__ float4 rep4(const LossArgs& a, int64_t row, int c) {
    float4 v = a.xv ? ld4(a.xv + row * D + c) : f4(0.f);
    if (a.xt) v = a.xv ? add4(v, ld4(a.xt + row * D + c)) : ld4(a.xt + row * D + c);
    return mul4(a.inv_m, v);
}

// the triplet on the rep rows of the user, the positive and the negative item
template <int D>
__device__ __forceinline__ void load_trip(const LossArgs& a, int64_t b, int c, ScoreTrip& t) {
    load_score_trip<D>(
        a.trip, a.B, b, a.nu, a.ni, c, [&](int64_t u, int c) { return rep4<D>(a, u, c); },
        [&](int64_t i, int c) { return rep4<D>(a, a.nu + i, c); }, t);
}

// part[block] = {sum softplus(-x), sum 2 |E_u|^2 + |E_p|^2 + |E_n|^2} over the block's triplets
template <int D>
__global__ __launch_bounds__(256) void loss_rows(LossArgs a, float* __restrict__ part) {
    constexpr int L = D / 4;
    const RowGeom<D> r;
    float v[2] = {0.f, 0.f};
    if (r.b < a.B) {  // uniform over a row's lane group
        ScoreTrip t;
        load_trip<D>(a, r.b, r.c, t);
        v[0] = softplus_neg(t.x);
        if (t.ok) {
            const float4 eu = ld4(a.E + t.u * D + r.c), ep = ld4(a.E + (a.nu + t.p) * D + r.c),
                         en = ld4(a.E + (a.nu + t.n) * D + r.c);
            // users.repeat_interleave(2): the user row is counted twice (mmgcn.py:84,93)
            v[1] = group_sum<L>(2.f * dot4(eu, eu) + dot4(ep, ep) + dot4(en, en));
        }
    }
    block_partials<D, 2, kPartStride>(r, v, part);
}

// out = {total, bpr, reg}: the block partials in index order
template <int D>
__global__ __launch_bounds__(64) void loss_finish(const float* __restrict__ part, int nblk, int64_t B, float reg_weight,
                                                  float pref_term, float* __restrict__ out) {
    float term[2];
    sum_partials<2, kPartStride>(part, nblk, term);
    if (threadIdx.x == 0) {
        const float bpr = term[0] / (float)B;
        const float reg = reg_weight * (term[1] / ((float)(2 * B) * (float)D) + pref_term);
        out[0] = bpr + reg;
        out[1] = bpr;
        out[2] = reg;
    }
}

// Per triplet b: coef[b] = d total / d x_b (upstream included), occU[b] = its contribution to
// the gradient of the user's row of either modality table, occR[b] = rep_u / num_modal (what an
// item occurrence scales by +-coef[b]), and the keys.
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
    const float ck = bpr_coef(t, go, a.B);
    st4(occU + b * D + r.c, mul4(ck * a.inv_m, sub4(t.pr, t.nr)));
    st4(occR + b * D + r.c, mul4(a.inv_m, t.ur));
    if (r.c == 0) {
        coef[b] = ck;
        store_keys(t, a.B, b, ku, ki);
    }
}

// The per-destination sums (rsx_triplet.hpp's walk).  G [n_users + n_items, D], zero-filled.
template <int D>
__global__ __launch_bounds__(256) void loss_sum_rows(LossArgs a, const float* __restrict__ occU,
                                                     const float* __restrict__ occR, const float* __restrict__ coef,
                                                     const int32_t* __restrict__ ku, const int32_t* __restrict__ ki,
                                                     float* __restrict__ G) {
    Walk<D> w;
    if (!w.begin(ku, ki, a.B)) return;
    const int c = w.c;
    float4 acc = f4(0.f);
    w.each([&](int64_t occ) { acc = add4(acc, ld4(occU + occ * D + c)); },
           [&](int64_t b, float sgn) { acc = fma4(sgn * coef[b], ld4(occR + b * D + c), acc); });
    tree_rows<Walk<D>::L>(acc);
    if (w.g != 0) return;
    st4(G + (w.user ? (int64_t)w.key : a.nu + w.key) * D + c, acc);
}

// result = (x_v + x_t) / num_modal over the whole table (n4 float4)
__global__ __launch_bounds__(256) void write_result(const float* __restrict__ xv, const float* __restrict__ xt,
                                                    float inv_m, int64_t n4, float* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        float4 v = xv ? ld4(xv + 4 * i) : f4(0.f);
        if (xt) v = xv ? add4(v, ld4(xt + 4 * i)) : ld4(xt + 4 * i);
        st4(out + 4 * i, mul4(inv_m, v));
    }
}

// one coefficient a triplet; occR is the workspace's extra row buffer (occX)
inline TripletWs carve(void* ws, int64_t B, int d) { return carve_triplet(ws, B, d, kPartStride, 1, 1); }

inline int loss_check(const rsx_mmgcn_loss_args* a, void* ws, size_t ws_bytes, LossArgs& k) {
    if (!a) return RSX_ERR_ARG;
    const bool own_ok = a->E && a->triplets && ws && (a->xv || a->xt) && aligned16(a->E) && aligned16(a->xv) &&
                        aligned16(a->xt) && aligned16(ws);
    const int rc = check_triplet(a->batch, a->n_users, a->n_items, a->d, own_ok, ws_bytes,
                                 rsx_mmgcn_loss_ws_bytes(a->batch, a->d));
    if (rc) return rc;
    if (a->n_users + a->n_items > 0x7fffffffll) return RSX_ERR_UNSUPPORTED;
    k.xv = a->xv, k.xt = a->xt, k.E = a->E, k.trip = a->triplets;
    k.nu = a->n_users, k.ni = a->n_items, k.B = a->batch;
    k.inv_m = 1.f / (float)((a->xv ? 1 : 0) + (a->xt ? 1 : 0));
    k.reg_weight = a->reg_weight, k.pref_term = a->pref_term;
    return RSX_OK;
}

template <int D>
int loss_fwd(const LossArgs& k, float* out, float* result, void* ws, hipStream_t s) {
    const TripletWs w = carve(ws, k.B, D);
    const int nblk = rows_blocks<D>(k.B);
    hipLaunchKernelGGL(loss_rows<D>, dim3(nblk), dim3(256), 0, s, k, w.part);
    hipLaunchKernelGGL(loss_finish<D>, dim3(1), dim3(64), 0, s, (const float*)w.part, nblk, k.B, k.reg_weight,
                       k.pref_term, out);
    if (result) {
        const int64_t n4 = (k.nu + k.ni) * (D / 4);
        const int64_t nb = (n4 + 255) / 256;
        hipLaunchKernelGGL(write_result, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(256), 0, s, k.xv, k.xt, k.inv_m,
                           n4, result);
    }
    return last_rc();
}

template <int D>
int loss_bwd(const LossArgs& k, const float* go, float* G, void* ws, hipStream_t s) {
    const TripletWs w = carve(ws, k.B, D);
    const int rc = zero_tables({{G, (size_t)(k.nu + k.ni) * D}}, s);
    if (rc) return rc;
    hipLaunchKernelGGL(loss_grad_rows<D>, dim3(rows_blocks<D>(k.B)), dim3(256), 0, s, k, go, w.occU, w.occX, w.coef,
                       w.ku, w.ki);
    launch_walk(loss_sum_rows<D>, k.B, s, k, w.occU, w.occX, w.coef, w.ku, w.ki, G);
    return last_rc();
}

template <int D>
int layer_launch(bool backward, LayerArgs& a, hipStream_t s) {
    a.nbx = ((a.n + 15) / 16 + 3) / 4;
    // two blocks a CU (the LDS weight copies allow two); each strides over its row blocks
    int64_t gx = a.nbx;
    const int64_t cap = 2 * (int64_t)device_cus();
    if (gx > cap) gx = cap;
    if (backward) hipLaunchKernelGGL(layer_bwd<D>, dim3((unsigned)gx), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(layer_fwd<D>, dim3((unsigned)gx), dim3(256), 0, s, a);
    return last_rc();
}

}  // namespace mm
}  // namespace rsx

using namespace rsx;

extern "C" {

int rsx_mmgcn_layer_fwd(const float* a, const float* x, const float* E, const float* Wc, const float* Wl,
                        const float* bl, const float* Wg, const float* bg, int64_t n, int32_t d, float* h, float* u,
                        float* out, rsx_stream_t stream) {
    if (n < 0 || !a || !x || !E || !Wc || !Wl || !bl || !Wg || !bg || !h || !u || !out) return RSX_ERR_ARG;
    if (d != 64 && d != 128) return RSX_ERR_UNSUPPORTED;
    for (const void* p : {(const void*)a, (const void*)x, (const void*)E, (const void*)Wc, (const void*)Wl,
                          (const void*)bl, (const void*)Wg, (const void*)bg, (const void*)h, (const void*)u,
                          (const void*)out})
        if (!aligned16(p)) return RSX_ERR_ARG;
    if (n == 0) return RSX_OK;
    mm::LayerArgs k{};
    k.Wc = Wc, k.Wl = Wl, k.bl = bl, k.Wg = Wg, k.bg = bg, k.a = a, k.x = x, k.E = E, k.h = h, k.u = u, k.out = out;
    k.n = n;
    hipStream_t s = as_stream(stream);
    return d == 64 ? mm::layer_launch<64>(false, k, s) : mm::layer_launch<128>(false, k, s);
}

int rsx_mmgcn_layer_bwd(const float* g_out, const float* out, const float* h, const float* u, const float* E,
                        const float* Wc, const float* Wl, const float* Wg, int64_t n, int32_t d, float* go, float* gh,
                        float* gu, float* xh, float* g_a, float* g_x, rsx_stream_t stream) {
    if (n < 0 || !g_out || !out || !h || !u || !E || !Wc || !Wl || !Wg || !go || !gh || !gu || !xh || !g_a || !g_x)
        return RSX_ERR_ARG;
    if (d != 64 && d != 128) return RSX_ERR_UNSUPPORTED;
    for (const void* p : {(const void*)g_out, (const void*)out, (const void*)h, (const void*)u, (const void*)E,
                          (const void*)Wc, (const void*)Wl, (const void*)Wg, (const void*)go, (const void*)gh,
                          (const void*)gu, (const void*)xh, (const void*)g_a, (const void*)g_x})
        if (!aligned16(p)) return RSX_ERR_ARG;
    if (n == 0) return RSX_OK;
    mm::LayerArgs k{};
    k.Wc = Wc, k.Wl = Wl, k.Wg = Wg, k.E = E, k.g_out = g_out;
    k.out = const_cast<float*>(out), k.h = const_cast<float*>(h), k.u = const_cast<float*>(u);  // (read only)
    k.go = go, k.gh = gh, k.gu = gu, k.xh = xh, k.g_a = g_a, k.g_x = g_x;
    k.n = n;
    hipStream_t s = as_stream(stream);
    return d == 64 ? mm::layer_launch<64>(true, k, s) : mm::layer_launch<128>(true, k, s);
}

size_t rsx_mmgcn_loss_ws_bytes(int64_t batch, int32_t d) {
    return triplet_ws_bytes(batch, d, mm::kPartStride, 1, 1);
}

int rsx_mmgcn_loss_fwd(const rsx_mmgcn_loss_args* a, float* out, float* result, void* ws, size_t ws_bytes,
                       rsx_stream_t stream) {
    mm::LossArgs k;
    const int rc = mm::loss_check(a, ws, ws_bytes, k);
    if (rc) return rc;
    if (!out || !aligned16(result)) return RSX_ERR_ARG;
    hipStream_t s = as_stream(stream);
    return a->d == 64 ? mm::loss_fwd<64>(k, out, result, ws, s) : mm::loss_fwd<128>(k, out, result, ws, s);
}

int rsx_mmgcn_loss_bwd(const rsx_mmgcn_loss_args* a, const float* go, float* g, void* ws, size_t ws_bytes,
                       rsx_stream_t stream) {
    mm::LossArgs k;
    const int rc = mm::loss_check(a, ws, ws_bytes, k);
    if (rc) return rc;
    if (!go || !g || !aligned16(g)) return RSX_ERR_ARG;
    hipStream_t s = as_stream(stream);
    return a->d == 64 ? mm::loss_bwd<64>(k, go, g, ws, s) : mm::loss_bwd<128>(k, go, g, ws, s);
}

}  // extern "C"
