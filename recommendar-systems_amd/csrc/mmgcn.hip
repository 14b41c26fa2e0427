// mmgcn.hip — MMGCN's dense part on gfx950 (f32 MFMA: exact f32 products, f32 sums), forward
// and backward.  Reference: src/models/mmgcn.py, the concatenating branch, three layers.
//
// Per modality and layer, on a = A_hat x (the mean operator, an SpMM outside this file):
//   h = leaky(a Wc)   u = leaky(x Wl^T + bl)   x_hat = u + E   out = leaky([h | x_hat] Wg^T + bg)
//
//  * layer_fwd / layer_bwd (layers 2 and 3, width D = d in {64, 128}): the whole chain of a
//    16-row tile in a wave's registers, in the row-field layout of smore_fld.hpp, the four
//    D x D weights (Wc [in, out], Wl, and the two halves of Wg [D, 2 D]) staged in LDS.  At
//    D = 64 the four copies (70 KB) stay resident and a block strides over its 64-row blocks;
//    at D = 128 one copy fits beside a second block, so the weights are restaged per row block
//    (as mgcn.hip's fuser does).  The backward writes g_a, the direct part of g_x, and the
//    three pre-activation gradient rows and x_hat for the weight gradients (rsx_smore_wgrad).
//  * gemm (layer 1, whose width is 256 or the text feature width, and the image MLP):
//    Y[n, N] = epilogue((X .* slope(Mx)) op(B) + bias), X optionally two column segments of
//    two tables (the [h | x_hat] operand is never concatenated), B given [K, N] or [N, K],
//    the epilogue leaky, a multiplication by slope(My) and a residual.  With Mx = the saved
//    output and the other layout of B it is the data gradient of the same product.
//    A 64 x 64 output tile a block, 16 x 64 a wave, K in 32-wide slabs staged in LDS with the
//    next slab's global loads in flight during the MFMAs.
//  * normalize (F.normalize over the image branch's item rows), colsum (the bias gradients:
//    block partial column sums, added in block order), the loss (rsx_triplet.hpp's protocol:
//    one-score triplet, block partials, keys, walk, workspace, checks; its own: the rep row
//    and the id regulariser) and the whole-table `result`.
//
// Slopes are read off the sign of the saved f32 outputs (leaky(p) > 0 exactly when p > 0, the
// slope being positive): no mask tensors.  No float atomics anywhere: two runs are bit-equal.
#include <cmath>

#include "rsx_triplet.hpp"
#include "smore_fld.hpp"

namespace rsx {
namespace mm {

using namespace rsx::sf;

constexpr float kSlope = 0.01f;  // F.leaky_relu's default

struct Leaky {
    __device__ float operator()(float v) const { return v > 0.f ? v : kSlope * v; }
};
struct MulSlope {  // g * slope(y): y a saved leaky output
    __device__ float operator()(float g, float y) const { return y > 0.f ? g : kSlope * g; }
};
struct Add {
    __device__ float operator()(float a, float b) const { return a + b; }
};
constexpr Leaky leaky{};
constexpr MulSlope mul_slope{};
constexpr Add add{};

__device__ __forceinline__ float4 mul_slope4(float4 g, float4 y) {
    return make_float4(mul_slope(g.x, y.x), mul_slope(g.y, y.y), mul_slope(g.z, y.z), mul_slope(g.w, y.w));
}

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
// the wide product
// ---------------------------------------------------------------------------
constexpr int kBM = 64, kBN = 64, kKS = 32, kLdT = kKS + 4;  // tile rows padded: conflict-free float4 reads

__global__ __launch_bounds__(256) void gemm(rsx_mmgcn_gemm_args a) {
    __shared__ __attribute__((aligned(16))) float Xs[kBM * kLdT];
    __shared__ __attribute__((aligned(16))) float Bs[kBN * kLdT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * kBM;
    const int col0 = (int)blockIdx.y * kBN;
    const int K = a.k0 + a.k1, N = a.n_out;
    const bool first_col_block = blockIdx.y == 0;

    // a slab's 64 x 32 tile of X: 512 float4, two a thread (8 along k, so a row is 128 B)
    auto load_x = [&](int ks, int j) __attribute__((always_inline)) {
        const int idx = tid + 256 * j;
        const int k = ks + ((idx & 7) << 2);
        const int64_t row = row0 + (idx >> 3);
        float4 v = f4(0.f);
        if (row < a.n && k < K) {
            if (k < a.k0) {
                v = ld4(a.x0 + row * a.ld0 + k);
                if (a.mx) v = mul_slope4(v, ld4(a.mx + row * a.ldmx + k));
                if (a.xm_out && first_col_block) st4(a.xm_out + row * (int64_t)a.k0 + k, v);
            } else {
                v = ld4(a.x1 + row * a.ld1 + (k - a.k0));
            }
        }
        return v;
    };
    // the slab's tile of B as [64 columns][32 k]: read along k ([N, K]) or along n ([K, N], transposed
    // on the way into LDS); columns past N and k past K are zero
    auto load_b = [&](int ks, int j) __attribute__((always_inline)) {
        const int idx = tid + 256 * j;
        float4 v = f4(0.f);
        if (a.b_kn) {
            const int k = ks + (idx >> 4), col = col0 + ((idx & 15) << 2);
            if (k < K && col < N) v = ld4(a.B + (int64_t)k * a.ldb + col);
        } else {
            const int k = ks + ((idx & 7) << 2), col = col0 + (idx >> 3);
            if (k < K && col < N) v = ld4(a.B + (int64_t)col * a.ldb + k);
        }
        return v;
    };
    auto store_tiles = [&](const float4 (&xr)[2], const float4 (&br)[2]) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int idx = tid + 256 * j;
            st4(Xs + (idx >> 3) * kLdT + ((idx & 7) << 2), xr[j]);
            if (a.b_kn) {
                const int kk = idx >> 4, nc = (idx & 15) << 2;
                Bs[(nc + 0) * kLdT + kk] = br[j].x;
                Bs[(nc + 1) * kLdT + kk] = br[j].y;
                Bs[(nc + 2) * kLdT + kk] = br[j].z;
                Bs[(nc + 3) * kLdT + kk] = br[j].w;
            } else {
                st4(Bs + (idx >> 3) * kLdT + ((idx & 7) << 2), br[j]);
            }
        }
    };

    // acc[tk][r]: row (row0 + 16 wave + c), column col0 + 16 tk + 4 g + r
    floatx4 acc[4];
#pragma unroll
    for (int tk = 0; tk < 4; ++tk) {
        const int col = col0 + 16 * tk + 4 * g;
        acc[tk] = floatx4{0.f, 0.f, 0.f, 0.f};
        if (a.bias && col < N) {
            const float4 b = ld4(a.bias + col);
            acc[tk] = floatx4{b.x, b.y, b.z, b.w};
        }
    }
    float4 xr[2], br[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) xr[j] = load_x(0, j), br[j] = load_b(0, j);
#pragma unroll 1
    for (int ks = 0; ks < K; ks += kKS) {
        __syncthreads();  // the previous slab's readers are done
        store_tiles(xr, br);
        __syncthreads();
        if (ks + kKS < K) {  // the next slab's loads fly during this slab's MFMAs
#pragma unroll
            for (int j = 0; j < 2; ++j) xr[j] = load_x(ks + kKS, j), br[j] = load_b(ks + kKS, j);
        }
        const float* xp = Xs + (16 * wave + c) * kLdT + 4 * g;
        const float* bp = Bs + c * kLdT + 4 * g;
#pragma unroll
        for (int t = 0; t < kKS / 16; ++t) {
            const float4 xv = ld4(xp + 16 * t);
            float4 w[4];
#pragma unroll
            for (int tk = 0; tk < 4; ++tk) w[tk] = ld4(bp + 16 * tk * kLdT + 16 * t);
#pragma unroll
            for (int tk = 0; tk < 4; ++tk) acc[tk] = mfma4(w[tk].x, xv.x, acc[tk]);
#pragma unroll
            for (int tk = 0; tk < 4; ++tk) acc[tk] = mfma4(w[tk].y, xv.y, acc[tk]);
#pragma unroll
            for (int tk = 0; tk < 4; ++tk) acc[tk] = mfma4(w[tk].z, xv.z, acc[tk]);
#pragma unroll
            for (int tk = 0; tk < 4; ++tk) acc[tk] = mfma4(w[tk].w, xv.w, acc[tk]);
        }
    }
    const int64_t row = row0 + 16 * wave + c;
    if (row >= a.n) return;
#pragma unroll
    for (int tk = 0; tk < 4; ++tk) {
        const int col = col0 + 16 * tk + 4 * g;
        if (col >= N) continue;
        float4 v = make_float4(acc[tk][0], acc[tk][1], acc[tk][2], acc[tk][3]);
        if (a.act) v = make_float4(leaky(v.x), leaky(v.y), leaky(v.z), leaky(v.w));
        const int64_t o = row * (int64_t)N + col;
        if (a.my) v = mul_slope4(v, ld4(a.my + o));
        if (a.y) st4(a.y + o, v);
        if (a.y2) st4(a.y2 + o, a.r ? add4(v, ld4(a.r + o)) : v);
    }
}

// ---------------------------------------------------------------------------
// F.normalize over rows (one wave a row), and its backward
// ---------------------------------------------------------------------------
constexpr float kNormEps = 1e-12f;

// y = x / max(|x|, eps); den[row] = max(|x|, eps).  y may alias x.
__global__ __launch_bounds__(256) void normalize_fwd(const float* x, int64_t n, int w, float* y, float* __restrict__ den) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // wave-uniform
    if (row >= n) return;
    float ss = 0.f;
    for (int k = 4 * lane; k < w; k += 256) {
        const float4 v = ld4(x + row * w + k);
        ss += dot4(v, v);
    }
    const float d = fmaxf(sqrtf(group_sum<kWave>(ss)), kNormEps);  // (every lane has read its chunks)
    for (int k = 4 * lane; k < w; k += 256) {
        const float4 v = ld4(x + row * w + k);
        st4(y + row * w + k, make_float4(v.x / d, v.y / d, v.z / d, v.w / d));
    }
    if (lane == 0) den[row] = d;
}

// torch's backward: g / den - y <g, y> / den where the norm was not clamped (den > eps; then
// x / |x| = y), g / den where it was (the clamp passes no gradient through the norm)
__global__ __launch_bounds__(256) void normalize_bwd(const float* __restrict__ gy, const float* __restrict__ y,
                                                     const float* __restrict__ den, int64_t n, int w,
                                                     float* __restrict__ gx) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // wave-uniform
    if (row >= n) return;
    float s = 0.f;
    for (int k = 4 * lane; k < w; k += 256) s += dot4(ld4(gy + row * w + k), ld4(y + row * w + k));
    const float d = den[row];
    const float dot = d > kNormEps ? group_sum<kWave>(s) : 0.f;
    for (int k = 4 * lane; k < w; k += 256) {
        const float4 gv = ld4(gy + row * w + k), yv = ld4(y + row * w + k);
        st4(gx + row * w + k, make_float4((gv.x - yv.x * dot) / d, (gv.y - yv.y * dot) / d, (gv.z - yv.z * dot) / d,
                                          (gv.w - yv.w * dot) / d));
    }
}

// ---------------------------------------------------------------------------
// column sums (bias gradients): block partials over kColRows rows each, then block order
// ---------------------------------------------------------------------------
constexpr int kColRows = 128;

__global__ __launch_bounds__(256) void colsum_part(const float* __restrict__ g, int64_t n, int N,
                                                   float* __restrict__ part) {
    const int col = (int)blockIdx.y * 256 + threadIdx.x;
    if (col >= N) return;
    const int64_t r0 = (int64_t)blockIdx.x * kColRows;
    const int64_t r1 = r0 + kColRows < n ? r0 + kColRows : n;
    float acc = 0.f;
    for (int64_t r = r0; r < r1; ++r) acc += g[r * N + col];
    part[(int64_t)blockIdx.x * N + col] = acc;
}

__global__ __launch_bounds__(256) void colsum_fin(const float* __restrict__ part, int64_t nblk, int N,
                                                  float* __restrict__ out) {
    const int col = (int)blockIdx.x * 256 + threadIdx.x;
    if (col >= N) return;
    float acc = 0.f;
    for (int64_t b = 0; b < nblk; ++b) acc += part[b * N + col];
    out[col] = acc;
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

int rsx_mmgcn_gemm(const rsx_mmgcn_gemm_args* a, rsx_stream_t stream) {
    if (!a || a->n < 0 || !a->x0 || !a->B || (!a->y && !a->y2) || (a->k1 > 0 && !a->x1)) return RSX_ERR_ARG;
    if (a->n_out <= 0 || a->k0 <= 0 || a->k1 < 0) return RSX_ERR_ARG;
    if ((a->n_out % 32) || (a->k0 % 4) || (a->k1 % 4) || a->n_out > 65535 * mm::kBN) return RSX_ERR_UNSUPPORTED;
    if (a->mx && a->k1 > 0) return RSX_ERR_UNSUPPORTED;  // the input mask covers a one-segment X
    if (a->xm_out && !a->mx) return RSX_ERR_ARG;
    const int K = a->k0 + a->k1;
    if (a->ld0 < a->k0 || (a->ld0 % 4) || (a->k1 > 0 && (a->ld1 < a->k1 || (a->ld1 % 4)))) return RSX_ERR_ARG;
    if (a->mx && (a->ldmx < a->k0 || (a->ldmx % 4))) return RSX_ERR_ARG;
    if (a->ldb < (a->b_kn ? a->n_out : K) || (a->ldb % 4)) return RSX_ERR_ARG;
    for (const void* p : {(const void*)a->x0, (const void*)a->x1, (const void*)a->mx, (const void*)a->xm_out,
                          (const void*)a->B, (const void*)a->bias, (const void*)a->my, (const void*)a->r,
                          (const void*)a->y, (const void*)a->y2})
        if (!aligned16(p)) return RSX_ERR_ARG;
    if (a->n == 0) return RSX_OK;
    const int64_t gx = (a->n + mm::kBM - 1) / mm::kBM;
    if (gx > 0x7fffffffll) return RSX_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)gx, (unsigned)((a->n_out + mm::kBN - 1) / mm::kBN));
    hipLaunchKernelGGL(mm::gemm, grid, dim3(256), 0, as_stream(stream), *a);
    return last_rc();
}

int rsx_mmgcn_normalize_fwd(const float* x, int64_t n, int32_t w, float* y, float* den, rsx_stream_t stream) {
    if (n < 0 || w <= 0 || !x || !y || !den || !aligned16(x) || !aligned16(y)) return RSX_ERR_ARG;
    if (w % 4) return RSX_ERR_UNSUPPORTED;
    if (n == 0) return RSX_OK;
    hipLaunchKernelGGL(mm::normalize_fwd, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, as_stream(stream), x, n, (int)w, y,
                       den);
    return last_rc();
}

int rsx_mmgcn_normalize_bwd(const float* gy, const float* y, const float* den, int64_t n, int32_t w, float* gx,
                            rsx_stream_t stream) {
    if (n < 0 || w <= 0 || !gy || !y || !den || !gx || !aligned16(gy) || !aligned16(y) || !aligned16(gx))
        return RSX_ERR_ARG;
    if (w % 4) return RSX_ERR_UNSUPPORTED;
    if (n == 0) return RSX_OK;
    hipLaunchKernelGGL(mm::normalize_bwd, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, as_stream(stream), gy, y, den, n,
                       (int)w, gx);
    return last_rc();
}

size_t rsx_mmgcn_colsum_ws_bytes(int64_t n, int32_t n_cols) {
    if (n <= 0 || n_cols <= 0) return 0;
    return (size_t)((n + mm::kColRows - 1) / mm::kColRows) * (size_t)n_cols * sizeof(float);
}

int rsx_mmgcn_colsum(const float* g, int64_t n, int32_t n_cols, float* out, void* ws, size_t ws_bytes,
                     rsx_stream_t stream) {
    if (n < 0 || n_cols <= 0 || !out || (n > 0 && !g)) return RSX_ERR_ARG;
    hipStream_t s = as_stream(stream);
    const unsigned gy = (unsigned)((n_cols + 255) / 256);
    const int64_t nblk = (n + mm::kColRows - 1) / mm::kColRows;
    if (n > 0 && (!ws || ws_bytes < rsx_mmgcn_colsum_ws_bytes(n, n_cols))) return RSX_ERR_WORKSPACE;
    if (nblk > 0x7fffffffll) return RSX_ERR_UNSUPPORTED;
    float* part = static_cast<float*>(ws);
    if (n > 0) hipLaunchKernelGGL(mm::colsum_part, dim3((unsigned)nblk, gy), dim3(256), 0, s, g, n, (int)n_cols, part);
    hipLaunchKernelGGL(mm::colsum_fin, dim3(gy), dim3(256), 0, s, (const float*)part, nblk, (int)n_cols, out);
    return last_rc();
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
