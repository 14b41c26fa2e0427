// bm3.hip — the bootstrap loss of BM3 on gfx950, forward and backward.
//
// Replaces, per batch (reference paths relative to its root):
//   src/models/bm3.py:99-149   predictor, four dropped-out targets, six cosine terms
//   src/common/loss.py:38-51   EmbLoss over the whole user and item tables
// and their autograd backward.
//
// The item row is E[NU + i] + H[i], formed where it is read (bm3.py:97's i_g_embeddings + h
// is never materialised), and the four dropout targets are rebuilt from the online rows and
// a per-element keep decision, so no [N, d] target table exists either.  The keep decision
// is a function of the TABLE row (an explicit bit mask, or the hash of smore_fld.hpp's
// drop_scale over (seed, stream, table row, column)): a row that occurs twice in a batch
// sees one mask, as in the reference, which drops out whole tables and gathers afterwards.
//
// Forward launches:  gather (the S B online rows, S = 2 + has_T + has_V, stacked by stream),
//   rsx_linear_rows_fwd (the predictor on the stacked rows: f32 MFMA, mf.hip's lin_rows_fwd),
//   the cosine terms (block partials), the two squared norms (block partials, f64), finish
//   (every partial added in index order: no float atomics on the loss).
// Backward launches: dense regulariser gradient into every row of gE (gT, gV zero-filled),
//   the cosine backward (gradient rows of the predicted rows), P^T, rsx_linear_rows_fwd (the
//   gradient of the online rows, g P), rsx_linear_rows_wgrad (gP, gpb: the fixed-order split
//   reduction), scatter of the online rows' gradients with f32 atomics (as bpr.hip's).
#include <algorithm>

#include "rsx_common.hpp"

namespace rsx {
namespace bm3 {

constexpr float kCosEps = 1e-8f;  // torch.nn.functional.cosine_similarity's eps
constexpr int kRegBlocks = 256;   // blocks (and partials) of the two squared norms
enum { S_USER = 0, S_ITEM = 1, S_TEXT = 2, S_IMAGE = 3 };

struct Args {
    int64_t nu, ni, B;
    const float *E, *H, *T, *V;
    const int64_t *users, *items;
    const int64_t* seed;
    const uint32_t* mask[4];
    float p_drop, scale;  // scale = 1 / (1 - p)
    int S;                // stacked streams: user, item, then text and / or image
    int slot_t, slot_v;   // the stacked slot of text / image, -1 when absent
};

__device__ __forceinline__ uint32_t mix32(uint64_t x) {  // smore_fld.hpp's
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdULL;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ULL;
    x ^= x >> 33;
    return (uint32_t)x;
}

// keep-scale (0 or 1 / (1 - p)) of columns c .. c + 3 of table row `row` of stream `s`
template <int D>
__device__ __forceinline__ float4 keep4(const Args& a, int s, int64_t row, int c) {
    float k[4];
    if (a.mask[s]) {
        const uint32_t w = a.mask[s][row * (D / 32) + (c >> 5)] >> (c & 31);
#pragma unroll
        for (int r = 0; r < 4; ++r) k[r] = ((w >> r) & 1u) ? a.scale : 0.f;
    } else if (a.p_drop > 0.f) {
        const uint64_t seed = (uint64_t)*a.seed;
        const uint32_t thr = (uint32_t)fminf(a.p_drop * 4294967296.f, 4294967295.f);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint64_t key = seed * 0x9E3779B97F4A7C15ULL + ((uint64_t)s << 58) + (uint64_t)row * D +
                                 (uint64_t)(c + r);
            k[r] = mix32(key) >= thr ? a.scale : 0.f;
        }
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) k[r] = 1.f;
    }
    return make_float4(k[0], k[1], k[2], k[3]);
}

__device__ __forceinline__ float4 mul44(float4 a, float4 b) {
    return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w);
}

// X[s B + b] = the online row of stream s of batch row b; a user or item index outside its
// table gives a NaN row (the loss is then NaN and the scatter skips the row).
template <int D>
__global__ __launch_bounds__(256) void gather(Args a, float* __restrict__ X) {
    constexpr int L = D / 4;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t r = t / L;
    const int c = (int)(t % L) * 4;
    if (r >= a.S * a.B) return;
    const int slot = (int)(r / a.B);
    const int64_t b = r % a.B;
    float4 v;
    if (slot == 0) {
        const int64_t u = a.users[b];
        v = (u >= 0 && u < a.nu) ? ld4(a.E + u * D + c) : f4(__builtin_nanf(""));
    } else {
        const int64_t i = a.items[b];
        if (i < 0 || i >= a.ni) v = f4(__builtin_nanf(""));
        else if (slot == 1) v = add4(ld4(a.E + (a.nu + i) * D + c), ld4(a.H + i * D + c));
        else v = ld4((slot == a.slot_t ? a.T : a.V) + i * D + c);
    }
    st4(X + r * D + c, v);
}

// out[s B + b] = the dropout target of stream s of batch row b (what the cosines compare with)
template <int D>
__global__ __launch_bounds__(256) void targets(Args a, const float* __restrict__ X, float* __restrict__ out) {
    constexpr int L = D / 4;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t r = t / L;
    const int c = (int)(t % L) * 4;
    if (r >= a.S * a.B) return;
    const int slot = (int)(r / a.B);
    const int64_t b = r % a.B;
    const int s = slot < 2 ? slot : (slot == a.slot_t ? S_TEXT : S_IMAGE);
    int64_t row = s == S_USER ? a.users[b] : a.items[b];
    if (row < 0 || row >= (s == S_USER ? a.nu : a.ni)) row = 0;  // the row is NaN (gather)
    st4(out + r * D + c, mul44(ld4(X + r * D + c), keep4<D>(a, s, row, c)));
}

// What one batch row needs of both passes: the four predicted rows q, the four targets t
// (lane's 4 columns), and the sums over the row (group_sum over the row's L lanes).
template <int D>
struct RowCtx {
    float4 q[4], t[4];
    float qq[4], tt[4];  // squared norms
    bool has[4];
};

template <int D>
__device__ __forceinline__ void load_row(const Args& a, const float* __restrict__ X, const float* __restrict__ Q,
                                         int64_t b, int c, RowCtx<D>& r) {
    constexpr int L = D / 4;
    int64_t u = a.users[b], i = a.items[b];
    const bool ok = u >= 0 && u < a.nu && i >= 0 && i < a.ni;
    if (!ok) u = i = 0;  // the rows are NaN (gather): only the mask address must be valid
    const int slot[4] = {0, 1, a.slot_t, a.slot_v};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        r.has[s] = slot[s] >= 0;
        if (!r.has[s]) {
            r.q[s] = r.t[s] = f4(0.f);
            r.qq[s] = r.tt[s] = 0.f;
            continue;
        }
        const int64_t off = ((int64_t)slot[s] * a.B + b) * D + c;
        r.q[s] = ld4(Q + off);
        r.t[s] = mul44(ld4(X + off), keep4<D>(a, s, s == S_USER ? u : i, c));
        r.qq[s] = group_sum<L>(dot4(r.q[s], r.q[s]));
        r.tt[s] = group_sum<L>(dot4(r.t[s], r.t[s]));
    }
}

// the six (online, target) pairs: ui, iu, t.i, v.i, t.t, v.v
__device__ constexpr int kOn[6] = {S_USER, S_ITEM, S_TEXT, S_IMAGE, S_TEXT, S_IMAGE};
__device__ constexpr int kTg[6] = {S_ITEM, S_USER, S_ITEM, S_ITEM, S_TEXT, S_IMAGE};

// cos(q, t) = (q / max(|q|, eps)) . (t / max(|t|, eps)): an all-dropped target gives 0
template <int D>
__device__ __forceinline__ float cos_pair(const RowCtx<D>& r, int k) {
    const int o = kOn[k], g = kTg[k];
    const float dot = group_sum<D / 4>(dot4(r.q[o], r.t[g]));
    return dot / (fmaxf(sqrtf(r.qq[o]), kCosEps) * fmaxf(sqrtf(r.tt[g]), kCosEps));
}

// part[block][k] = sum over the block's rows, in row order, of cosine term k
template <int D>
__global__ __launch_bounds__(256) void cos_fwd(Args a, const float* __restrict__ X, const float* __restrict__ Q,
                                               float* __restrict__ part) {
    constexpr int L = D / 4, RPB = 256 / L;
    __shared__ float sh[RPB][6];
    const int lr = threadIdx.x / L, c = (threadIdx.x % L) * 4;
    const int64_t b = (int64_t)blockIdx.x * RPB + lr;
    float cs[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (b < a.B) {  // uniform over a row's lane group
        RowCtx<D> r;
        load_row<D>(a, X, Q, b, c, r);
#pragma unroll
        for (int k = 0; k < 6; ++k)
            if (r.has[kOn[k]]) cs[k] = cos_pair<D>(r, k);
    }
    if (c == 0)
#pragma unroll
        for (int k = 0; k < 6; ++k) sh[lr][k] = cs[k];
    __syncthreads();
    if (threadIdx.x < 6) {
        float acc = 0.f;
        for (int j = 0; j < RPB; ++j) acc += sh[j][threadIdx.x];
        part[(int64_t)blockIdx.x * 8 + threadIdx.x] = acc;
    }
}

// rpart[block] = {sum x^2 over the block's user rows, over its item rows (E + H)} in f64;
// a block owns `rows` consecutive rows of [E_U ; E_I + H]
template <int D>
__global__ __launch_bounds__(256) void sqsum(Args a, int64_t rows, double* __restrict__ rpart) {
    constexpr int L = D / 4;
    __shared__ double sh[2][256];
    const int64_t n = a.nu + a.ni;
    const int64_t r0 = (int64_t)blockIdx.x * rows, r1 = min(n, r0 + rows);
    const int c = (threadIdx.x % L) * 4;
    double su = 0.0, si = 0.0;
    for (int64_t r = r0 + threadIdx.x / L; r < r1; r += 256 / L) {
        float4 v = ld4(a.E + r * D + c);
        if (r >= a.nu) {
            v = add4(v, ld4(a.H + (r - a.nu) * D + c));
            si += (double)dot4(v, v);
        } else {
            su += (double)dot4(v, v);
        }
    }
    sh[0][threadIdx.x] = su;
    sh[1][threadIdx.x] = si;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {  // a fixed tree
        if (threadIdx.x < s) {
            sh[0][threadIdx.x] += sh[0][threadIdx.x + s];
            sh[1][threadIdx.x] += sh[1][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        rpart[2 * blockIdx.x] = sh[0][0];
        rpart[2 * blockIdx.x + 1] = sh[1][0];
    }
}

// out[0] = total, out[1..7] = ui, iu, t, v, tv, vt, reg (the EmbLoss value, unweighted);
// norms[0..1] = |E_U|_F, |E_I + H|_F for the backward.  Every partial in index order.
__global__ __launch_bounds__(64) void finish(const float* __restrict__ part, int nblk, const double* __restrict__ rpart,
                                             int nreg, int64_t B, int64_t ni, int has_t, int has_v, float reg_weight,
                                             float cl_weight, float* __restrict__ norms, float* __restrict__ out) {
    __shared__ float term[8];
    const int k = threadIdx.x;
    if (k < 6) {
        float acc = 0.f;
        for (int j = 0; j < nblk; ++j) acc += part[(int64_t)j * 8 + k];
        const bool on = k < 2 || ((k == 2 || k == 4) ? has_t : has_v);
        term[k] = on ? 1.f - acc / (float)B : 0.f;
    } else if (k < 8) {
        double acc = 0.0;
        for (int j = 0; j < nreg; ++j) acc += rpart[2 * j + (k - 6)];
        term[k] = (float)sqrt(acc);
    }
    __syncthreads();
    if (k == 0) {
        const float reg = (term[6] + term[7]) / (float)ni;
        norms[0] = term[6];
        norms[1] = term[7];
        out[0] = (term[0] + term[1]) + reg_weight * reg + cl_weight * (((term[2] + term[3]) + term[4]) + term[5]);
#pragma unroll
        for (int j = 0; j < 6; ++j) out[1 + j] = term[j];
        out[7] = reg;
    }
}

// gE[r] = go reg_weight / NI * x / |X|_F over every row of [E_U ; E_I + H] (0 where the norm
// is 0, torch.norm's subgradient)
template <int D>
__global__ __launch_bounds__(256) void reg_fill(Args a, const float* __restrict__ norms, const float* __restrict__ go,
                                                float reg_weight, float* __restrict__ gE) {
    constexpr int L = D / 4;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t r = t / L;
    const int c = (int)(t % L) * 4;
    if (r >= a.nu + a.ni) return;
    const bool item = r >= a.nu;
    const float nrm = norms[item ? 1 : 0];
    const float coef = nrm > 0.f ? *go * reg_weight / (float)a.ni / nrm : 0.f;
    float4 v = ld4(a.E + r * D + c);
    if (item) v = add4(v, ld4(a.H + (r - a.nu) * D + c));
    st4(gE + r * D + c, mul4(coef, v));
}

// d cos(q, t) / dq, scaled by w, added to acc: with n = max(|q|, eps), th = t / max(|t|, eps)
// and c = q . th / n:  th / n - (c / n) q / |q|  (the clamp is outside autograd, as torch's)
template <int D>
__device__ __forceinline__ void cos_grad(const RowCtx<D>& r, int k, float w, float4& acc) {
    const int o = kOn[k], g = kTg[k];
    const float qn = sqrtf(r.qq[o]), n = fmaxf(qn, kCosEps), tn = fmaxf(sqrtf(r.tt[g]), kCosEps);
    const float dot = group_sum<D / 4>(dot4(r.q[o], r.t[g]));
    const float c = dot / (n * tn);
    const float wa = w / (n * tn), wb = qn > 0.f ? -w * c / (n * qn) : 0.f;
    acc = fma4(wa, r.t[g], acc);
    acc = fma4(wb, r.q[o], acc);
}

// G[s B + b] = d loss / d (predicted row of stream s of batch row b), upstream *go included
template <int D>
__global__ __launch_bounds__(256) void cos_bwd(Args a, const float* __restrict__ X, const float* __restrict__ Q,
                                               const float* __restrict__ go, float cl_weight, float* __restrict__ G) {
    constexpr int L = D / 4, RPB = 256 / L;
    const int lr = threadIdx.x / L, c = (threadIdx.x % L) * 4;
    const int64_t b = (int64_t)blockIdx.x * RPB + lr;
    if (b >= a.B) return;  // uniform over a row's lane group
    RowCtx<D> r;
    load_row<D>(a, X, Q, b, c, r);
    const float w1 = -*go / (float)a.B, w2 = w1 * cl_weight;
    float4 g[4] = {f4(0.f), f4(0.f), f4(0.f), f4(0.f)};
    cos_grad<D>(r, 0, w1, g[S_USER]);
    cos_grad<D>(r, 1, w1, g[S_ITEM]);
    if (r.has[S_TEXT]) {
        cos_grad<D>(r, 2, w2, g[S_TEXT]);
        cos_grad<D>(r, 4, w2, g[S_TEXT]);
    }
    if (r.has[S_IMAGE]) {
        cos_grad<D>(r, 3, w2, g[S_IMAGE]);
        cos_grad<D>(r, 5, w2, g[S_IMAGE]);
    }
    const int slot[4] = {0, 1, a.slot_t, a.slot_v};
#pragma unroll
    for (int s = 0; s < 4; ++s)
        if (slot[s] >= 0) st4(G + ((int64_t)slot[s] * a.B + b) * D + c, g[s]);
}

__global__ __launch_bounds__(256) void transpose_dd(const float* __restrict__ P, int d, float* __restrict__ PT) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < d * d) PT[(t % d) * d + t / d] = P[t];
}

// the online rows' gradients into their table rows (f32 atomics: a row occurs many times);
// one lane an element, so a wave's add covers 256 contiguous bytes of one row (two 128-byte
// row segments at d = 32)
template <int D>
__global__ __launch_bounds__(256) void scatter(Args a, const float* __restrict__ dX, float* __restrict__ gE,
                                               float* __restrict__ gT, float* __restrict__ gV) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t r = t / D;
    const int c = (int)(t % D);
    if (r >= a.S * a.B) return;
    const int slot = (int)(r / a.B);
    const int64_t b = r % a.B;
    const int64_t u = a.users[b], i = a.items[b];
    if (u < 0 || u >= a.nu || i < 0 || i >= a.ni) return;
    float* dst = slot == 0 ? gE + u * D : slot == 1 ? gE + (a.nu + i) * D : (slot == a.slot_t ? gT : gV) + i * D;
    atomicAdd(dst + c, dX[r * D + c]);
}

// the workspace: X, Q, G, dX [4 B, d], P^T [d, d], the loss partials, the norm partials, the
// two norms, rsx_linear_rows_wgrad's workspace; every size grows with B
struct Ws {
    float *X, *Q, *G, *dX, *PT, *part, *norms;
    double* rpart;
    void* wg;
    size_t wg_bytes, total;
};
inline Ws carve(void* ws, int64_t B, int d) {
    Ws w;
    Carver cv(ws);
    const size_t rows = (size_t)4 * (size_t)B * d * sizeof(float);
    w.X = cv.take<float>(rows);
    w.Q = cv.take<float>(rows);
    w.G = cv.take<float>(rows);
    w.dX = cv.take<float>(rows);
    w.PT = cv.take<float>((size_t)d * d * sizeof(float));
    w.part = cv.take<float>(((size_t)B / 8 + 1) * 8 * sizeof(float));
    w.rpart = cv.take<double>((size_t)kRegBlocks * 2 * sizeof(double));
    w.norms = cv.take<float>(4 * sizeof(float));
    w.wg_bytes = rsx_linear_rows_wgrad_ws_bytes(4 * B, d, d);
    w.wg = cv.take<void>(w.wg_bytes);
    w.total = cv.total();
    return w;
}

inline int check(const rsx_bm3_args* a, Args& k) {
    if (!a || a->batch < 1 || a->n_users < 1 || a->n_items < 1) return RSX_ERR_ARG;
    if (a->d != 32 && a->d != 64 && a->d != 128) return RSX_ERR_UNSUPPORTED;
    if (!a->E || !a->H || !a->P || !a->pb || !a->users || !a->items || !a->ws) return RSX_ERR_ARG;
    if (!(a->p_drop >= 0.f && a->p_drop < 1.f)) return RSX_ERR_ARG;
    if (a->batch > (int64_t)1 << 26) return RSX_ERR_UNSUPPORTED;  // 4 B d and the launch grids stay in 32 bits
    k.nu = a->n_users, k.ni = a->n_items, k.B = a->batch;
    k.E = a->E, k.H = a->H, k.T = a->T, k.V = a->V;
    k.users = a->users, k.items = a->items, k.seed = a->seed;
    for (int s = 0; s < 4; ++s) k.mask[s] = a->mask[s];
    k.p_drop = a->p_drop;
    k.scale = a->p_drop > 0.f ? (float)(1.0 / (1.0 - (double)a->p_drop)) : 1.f;
    k.slot_t = a->T ? 2 : -1;
    k.slot_v = a->V ? (a->T ? 3 : 2) : -1;
    k.S = 2 + (a->T != nullptr) + (a->V != nullptr);
    if (a->p_drop > 0.f && !a->seed) {  // a hashed stream needs the seed
        if (!a->mask[S_USER] || !a->mask[S_ITEM] || (a->T && !a->mask[S_TEXT]) || (a->V && !a->mask[S_IMAGE]))
            return RSX_ERR_ARG;
    }
    if (a->ws_bytes < rsx_bm3_ws_bytes(a->batch, a->d)) return RSX_ERR_WORKSPACE;
    return RSX_OK;
}

template <int D>
int fwd(const rsx_bm3_args* a, const Args& k, float* out, hipStream_t s) {
    constexpr int L = D / 4, RPB = 256 / L;
    const Ws w = carve(a->ws, k.B, D);
    const int64_t n = (int64_t)k.S * k.B;
    hipLaunchKernelGGL(gather<D>, dim3((unsigned)((n * L + 255) / 256)), dim3(256), 0, s, k, w.X);
    int rc = rsx_linear_rows_fwd(w.X, a->P, a->pb, nullptr, n, D, D, w.Q, D, (rsx_stream_t)s);
    if (rc) return rc;
    const int nblk = (int)((k.B + RPB - 1) / RPB);
    hipLaunchKernelGGL(cos_fwd<D>, dim3(nblk), dim3(256), 0, s, k, (const float*)w.X, (const float*)w.Q, w.part);
    const int64_t N = k.nu + k.ni;
    const int64_t rows = (N + kRegBlocks - 1) / kRegBlocks;
    const int nreg = (int)((N + rows - 1) / rows);
    hipLaunchKernelGGL(sqsum<D>, dim3(nreg), dim3(256), 0, s, k, rows, w.rpart);
    hipLaunchKernelGGL(finish, dim3(1), dim3(64), 0, s, (const float*)w.part, nblk, (const double*)w.rpart, nreg, k.B,
                       k.ni, (int)(a->T != nullptr), (int)(a->V != nullptr), a->reg_weight, a->cl_weight, w.norms, out);
    return last_rc();
}

template <int D>
int tgt(const Args& k, const Ws& w, float* out, hipStream_t s) {
    const int64_t n = (int64_t)k.S * k.B;
    const dim3 grid((unsigned)((n * (D / 4) + 255) / 256));
    hipLaunchKernelGGL(gather<D>, grid, dim3(256), 0, s, k, w.X);
    hipLaunchKernelGGL(targets<D>, grid, dim3(256), 0, s, k, (const float*)w.X, out);
    return last_rc();
}

template <int D>
int bwd(const rsx_bm3_args* a, const Args& k, const float* go, float* gE, float* gT, float* gV, float* gP, float* gpb,
        hipStream_t s) {
    constexpr int L = D / 4, RPB = 256 / L;
    const Ws w = carve(a->ws, k.B, D);
    const int64_t n = (int64_t)k.S * k.B, N = k.nu + k.ni;
    hipLaunchKernelGGL(reg_fill<D>, dim3((unsigned)((N * L + 255) / 256)), dim3(256), 0, s, k, (const float*)w.norms, go,
                       a->reg_weight, gE);
    hipError_t e;
    if (gT && (e = hipMemsetAsync(gT, 0, (size_t)k.ni * D * sizeof(float), s)) != hipSuccess) return hip_rc(e);
    if (gV && (e = hipMemsetAsync(gV, 0, (size_t)k.ni * D * sizeof(float), s)) != hipSuccess) return hip_rc(e);
    const int nblk = (int)((k.B + RPB - 1) / RPB);
    hipLaunchKernelGGL(cos_bwd<D>, dim3(nblk), dim3(256), 0, s, k, (const float*)w.X, (const float*)w.Q, go,
                       a->cl_weight, w.G);
    hipLaunchKernelGGL(transpose_dd, dim3((D * D + 255) / 256), dim3(256), 0, s, a->P, D, w.PT);
    int rc = rsx_linear_rows_fwd(w.G, w.PT, nullptr, nullptr, n, D, D, w.dX, D, (rsx_stream_t)s);
    if (rc) return rc;
    rc = rsx_linear_rows_wgrad(w.G, D, w.X, nullptr, n, D, D, gP, gpb, w.wg, w.wg_bytes, (rsx_stream_t)s);
    if (rc) return rc;
    hipLaunchKernelGGL(scatter<D>, dim3((unsigned)((n * D + 255) / 256)), dim3(256), 0, s, k, (const float*)w.dX, gE, gT,
                       gV);
    return last_rc();
}

}  // namespace bm3
}  // namespace rsx

using namespace rsx;

extern "C" size_t rsx_bm3_ws_bytes(int64_t batch, int32_t d) {
    if (batch < 1 || (d != 32 && d != 64 && d != 128)) return 0;
    return bm3::carve(nullptr, batch, d).total;
}

extern "C" int rsx_bm3_loss_fwd(const rsx_bm3_args* a, float* out, rsx_stream_t stream) {
    bm3::Args k;
    const int rc = bm3::check(a, k);
    if (rc) return rc;
    if (!out) return RSX_ERR_ARG;
    hipStream_t s = as_stream(stream);
    switch (a->d) {
        case 32: return bm3::fwd<32>(a, k, out, s);
        case 64: return bm3::fwd<64>(a, k, out, s);
        default: return bm3::fwd<128>(a, k, out, s);
    }
}

extern "C" int rsx_bm3_targets(const rsx_bm3_args* a, float* out, rsx_stream_t stream) {
    bm3::Args k;
    const int rc = bm3::check(a, k);
    if (rc) return rc;
    if (!out) return RSX_ERR_ARG;
    hipStream_t s = as_stream(stream);
    const bm3::Ws w = bm3::carve(a->ws, k.B, a->d);
    switch (a->d) {
        case 32: return bm3::tgt<32>(k, w, out, s);
        case 64: return bm3::tgt<64>(k, w, out, s);
        default: return bm3::tgt<128>(k, w, out, s);
    }
}

extern "C" int rsx_bm3_loss_bwd(const rsx_bm3_args* a, const float* go, float* gE, float* gT, float* gV, float* gP,
                                float* gpb, rsx_stream_t stream) {
    bm3::Args k;
    const int rc = bm3::check(a, k);
    if (rc) return rc;
    if (!go || !gE || !gP || !gpb || (a->T && !gT) || (a->V && !gV)) return RSX_ERR_ARG;
    hipStream_t s = as_stream(stream);
    switch (a->d) {
        case 32: return bm3::bwd<32>(a, k, go, gE, a->T ? gT : nullptr, a->V ? gV : nullptr, gP, gpb, s);
        case 64: return bm3::bwd<64>(a, k, go, gE, a->T ? gT : nullptr, a->V ? gV : nullptr, gP, gpb, s);
        default: return bm3::bwd<128>(a, k, go, gE, a->T ? gT : nullptr, a->V ? gV : nullptr, gP, gpb, s);
    }
}
