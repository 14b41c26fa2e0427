// freedom.hip — FREEDOM's training loss on gfx950, forward and backward.
//
// Replaces, per batch (reference paths relative to its root):
//   src/models/freedom.py:182-212   three BPR terms that share the user row: the id path on
//                                   E[u], E[nu + i] + H[i], and the text / image terms on the
//                                   projected feature tables, weighted by reg_weight
// and their autograd backward (the gathers' index_put scatter-adds).
//
// Layout: a d-wide row is one lane group of L = d / 4 float4 lanes, so a wave64 carries
// G = 64 / L rows (4 at d = 64, 2 at d = 128).
//
// Forward launches:  loss_rows (one lane group a triplet: the three scores, the stable
//   softplus, block partials in row order), finish (the partials in index order).  No atomics.
// Backward launches: memset of gE / gT / gV (every row is written: zero off the batch),
//   grad_rows (the scores again, the three coefficients of a triplet, its user-row
//   contribution stored ONCE in the workspace, and the batch's keys as int32), sum_rows.
//   sum_rows is the per-destination sum through the inverted index, the index being the
//   key lists themselves: one wave per occurrence; the wave of a destination's FIRST
//   occurrence (no equal key before it: a ballot scan) walks the keys after it 256 at a time
//   (an int4 of keys a lane), and the matches of a chunk, in a fixed order, are dealt
//   round-robin to the wave's G lane groups, which add their rows; the G partial rows are
//   then added in a fixed tree.
//   The order is a function of the keys alone, so the sums are bit-reproducible.  A user row
//   adds the stored contribution rows; an item row adds coefficient * E[user] for the id,
//   text and image coefficient of each occurrence (positives +, negatives -) in one walk, as
//   all three tables share the item's occurrence list.
// The walk costs (keys / 256) chunk loads a wave, 3 B waves: quadratic in the batch, which is
// why batch is capped (kMaxBatch); at B = 2048 it is 4096 waves of at most 16 chunk loads.
#include "rsx_common.hpp"

namespace rsx {
namespace freedom {

constexpr int64_t kMaxBatch = 65536;

struct Args {
    const float *E, *H, *T, *V;
    const int64_t* trip;
    int64_t nu, ni, B;
    float reg;
};

__device__ __forceinline__ float4 sub4(float4 a, float4 b) {
    return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w);
}
// softplus(-x) = -logsigmoid(x), the stable form of F.logsigmoid
__device__ __forceinline__ float softplus_neg(float x) { return fmaxf(-x, 0.f) + log1pf(expf(-fabsf(x))); }
// sigmoid(-x) without overflow
__device__ __forceinline__ float sigmoid_neg(float x) {
    const float e = expf(-fabsf(x));
    return x >= 0.f ? e / (1.f + e) : 1.f / (1.f + e);
}

// One triplet as seen by one lane (its 4 columns): the rows and the three scores
// x_k = sum(u * pos_k) - sum(u * neg_k), k = id, text, image (0 where the table is absent).
// An index outside its table: ok = false, the scores NaN, the rows zero.
template <int D>
struct Trip {
    bool ok;
    int64_t u, p, n;
    float4 ur, dp, dt, dv;  // the user row, pos - neg of the id / text / image rows
    float x[3];
};

template <int D>
__device__ __forceinline__ void load_trip(const Args& a, int64_t b, int c, Trip<D>& t) {
    constexpr int L = D / 4;
    t.u = a.trip[b], t.p = a.trip[a.B + b], t.n = a.trip[2 * a.B + b];
    t.ok = t.u >= 0 && t.u < a.nu && t.p >= 0 && t.p < a.ni && t.n >= 0 && t.n < a.ni;
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
    constexpr int L = D / 4, RPB = 256 / L;
    __shared__ float sh[RPB][3];
    const int lr = threadIdx.x / L, c = (threadIdx.x % L) * 4;
    const int64_t b = (int64_t)blockIdx.x * RPB + lr;
    float v[3] = {0.f, 0.f, 0.f};
    if (b < a.B) {  // uniform over a row's lane group
        Trip<D> t;
        load_trip<D>(a, b, c, t);
        v[0] = softplus_neg(t.x[0]);
        if (a.T) v[1] = softplus_neg(t.x[1]);
        if (a.V) v[2] = softplus_neg(t.x[2]);
    }
    if (c == 0)
#pragma unroll
        for (int k = 0; k < 3; ++k) sh[lr][k] = v[k];
    __syncthreads();
    if (threadIdx.x < 3) {
        float acc = 0.f;
        for (int j = 0; j < RPB; ++j) acc += sh[j][threadIdx.x];
        part[(int64_t)blockIdx.x * 4 + threadIdx.x] = acc;
    }
}

// out = {total, id, text, image}: lane l adds the block partials l, l + 64, ... in index order,
// the 64 lane sums are added in a fixed tree, then the mean
__global__ __launch_bounds__(64) void finish(const float* __restrict__ part, int nblk, int64_t B, float reg,
                                             float* __restrict__ out) {
    float term[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float acc = 0.f;
        for (int j = threadIdx.x; j < nblk; j += kWave) acc += part[(int64_t)j * 4 + k];
        term[k] = group_sum<kWave>(acc) / (float)B;
    }
    if (threadIdx.x == 0) {
        out[0] = term[0] + reg * (term[1] + term[2]);
        out[1] = term[0];
        out[2] = term[1];
        out[3] = term[2];
    }
}

// Per triplet b: coef[k B + b] = d total / d x_k (upstream *go included), occU[b] = its
// contribution to the user row, ku[b] / ki[b] / ki[B + b] = user / positive / negative as
// int32 (-1 for a triplet with an index outside its table: it contributes nothing).
template <int D>
__global__ __launch_bounds__(256) void grad_rows(Args a, const float* __restrict__ go, float* __restrict__ occU,
                                                 float* __restrict__ coef, int32_t* __restrict__ ku,
                                                 int32_t* __restrict__ ki) {
    constexpr int L = D / 4, RPB = 256 / L;
    const int lr = threadIdx.x / L, c = (threadIdx.x % L) * 4;
    const int64_t b = (int64_t)blockIdx.x * RPB + lr;
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
        ku[b] = t.ok ? (int32_t)t.u : -1;
        ki[b] = t.ok ? (int32_t)t.p : -1;
        ki[a.B + b] = t.ok ? (int32_t)t.n : -1;
    }
}

// Which of the 256 keys at `base` (a multiple of 256) equal `key`, among the indices in
// [lo, hi): lane l loads keys base + 4 l .. + 3 as one int4 (the key arrays are 256-byte
// aligned and padded to a multiple of 64 entries, so the load stays inside the array), and
// bit l of m[q] answers for index base + 4 l + q.
__device__ __forceinline__ void match256(const int32_t* __restrict__ keys, int64_t base, int lane, int64_t lo,
                                         int64_t hi, int32_t key, unsigned long long m[4]) {
    const int64_t i = base + 4 * lane;
    int4 k = make_int4(-1, -1, -1, -1);
    if (i < hi) k = *reinterpret_cast<const int4*>(keys + i);
    m[0] = __ballot(i >= lo && i < hi && k.x == key);
    m[1] = __ballot(i + 1 >= lo && i + 1 < hi && k.y == key);
    m[2] = __ballot(i + 2 >= lo && i + 2 < hi && k.z == key);
    m[3] = __ballot(i + 3 >= lo && i + 3 < hi && k.w == key);
}

// The per-destination sums (see the head of the file).  Wave w < B: user occurrence w;
// else item occurrence w - B of [positives; negatives].
template <int D>
__global__ __launch_bounds__(256) void sum_rows(Args a, const float* __restrict__ occU, const float* __restrict__ coef,
                                                const int32_t* __restrict__ ku, const int32_t* __restrict__ ki,
                                                float* __restrict__ gE, float* __restrict__ gT,
                                                float* __restrict__ gV) {
    constexpr int L = D / 4, G = kWave / L, kChunk = 4 * kWave;
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), B = a.B;
    if (w >= 3 * B) return;  // wave-uniform, as every branch on w, j, key and the ballots below
    const bool user = w < B;
    const int32_t* __restrict__ keys = user ? ku : ki;
    const int64_t n = user ? B : 2 * B, j = user ? w : w - B;
    const int32_t key = keys[j];
    if (key < 0) return;
    unsigned long long m[4];
    for (int64_t base = 0; base < j; base += kChunk) {  // an earlier occurrence leads
        match256(keys, base, lane, 0, j, key, m);
        if (m[0] | m[1] | m[2] | m[3]) return;
    }
    const int g = lane / L, c = (lane % L) * 4;
    float4 acc[3] = {f4(0.f), f4(0.f), f4(0.f)};
    for (int64_t base = j & ~(int64_t)(kChunk - 1); base < n; base += kChunk) {
        match256(keys, base, lane, j, n, key, m);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            unsigned long long mq = m[q];
            while (mq) {
                int64_t mine = -1;  // this lane group's occurrence of the next G matches
#pragma unroll
                for (int t = 0; t < G; ++t)
                    if (mq) {
                        const int bit = __ffsll(mq) - 1;
                        mq &= mq - 1;
                        if (t == g) mine = base + 4 * bit + q;
                    }
                if (mine < 0) continue;
                if (user) {
                    acc[0] = add4(acc[0], ld4(occU + mine * D + c));
                } else {
                    const int64_t b = mine < B ? mine : mine - B;
                    const float sgn = mine < B ? 1.f : -1.f;
                    const float4 u = ld4(a.E + (int64_t)ku[b] * D + c);
                    acc[0] = fma4(sgn * coef[b], u, acc[0]);
                    if (gT) acc[1] = fma4(sgn * coef[B + b], u, acc[1]);
                    if (gV) acc[2] = fma4(sgn * coef[2 * B + b], u, acc[2]);
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int o = kWave / 2; o >= L; o >>= 1) {  // the G partial rows, a fixed tree
            acc[k].x += __shfl_xor(acc[k].x, o, kWave);
            acc[k].y += __shfl_xor(acc[k].y, o, kWave);
            acc[k].z += __shfl_xor(acc[k].z, o, kWave);
            acc[k].w += __shfl_xor(acc[k].w, o, kWave);
        }
    if (g != 0) return;
    if (user) {
        st4(gE + (int64_t)key * D + c, acc[0]);
    } else {
        st4(gE + (a.nu + key) * D + c, acc[0]);
        if (gT) st4(gT + (int64_t)key * D + c, acc[1]);
        if (gV) st4(gV + (int64_t)key * D + c, acc[2]);
    }
}

inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

// the workspace: the forward's block partials; the backward's per-occurrence user rows
// [B, d], the coefficients [3, B] and the int32 keys (users [B], items [2 B])
struct Ws {
    float *part, *occU, *coef;
    int32_t *ku, *ki;
    size_t total;
};
inline Ws carve(void* ws, int64_t B, int d) {
    Ws w;
    char* p = static_cast<char*>(ws);
    size_t o = 0;
    auto take = [&](size_t n) {
        char* q = p ? p + o : nullptr;
        o += al(n);
        return q;
    };
    const int rpb = 256 / (d / 4);
    w.part = reinterpret_cast<float*>(take((size_t)((B + rpb - 1) / rpb) * 4 * sizeof(float)));
    w.occU = reinterpret_cast<float*>(take((size_t)B * d * sizeof(float)));
    w.coef = reinterpret_cast<float*>(take((size_t)3 * B * sizeof(float)));
    w.ku = reinterpret_cast<int32_t*>(take((size_t)B * sizeof(int32_t)));
    w.ki = reinterpret_cast<int32_t*>(take((size_t)2 * B * sizeof(int32_t)));
    w.total = o;
    return w;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline int check(const rsx_freedom_args* a, void* ws, size_t ws_bytes, Args& k) {
    if (!a || a->batch < 1 || a->n_users < 1 || a->n_items < 1) return RSX_ERR_ARG;
    if (a->d != 64 && a->d != 128) return RSX_ERR_UNSUPPORTED;
    if (!a->E || !a->triplets || !ws || (!a->T && !a->V)) return RSX_ERR_ARG;
    if (!aligned16(a->E) || !aligned16(a->H) || !aligned16(a->T) || !aligned16(a->V) || !aligned16(ws))
        return RSX_ERR_ARG;
    // keys are listed as int32; the walk over the keys is quadratic in the batch
    if (a->batch > kMaxBatch || a->n_users > 0x7fffffffll || a->n_items > 0x7fffffffll) return RSX_ERR_UNSUPPORTED;
    if (ws_bytes < rsx_freedom_ws_bytes(a->batch, a->d)) return RSX_ERR_WORKSPACE;
    k.E = a->E, k.H = a->H, k.T = a->T, k.V = a->V, k.trip = a->triplets;
    k.nu = a->n_users, k.ni = a->n_items, k.B = a->batch, k.reg = a->reg;
    return RSX_OK;
}

template <int D>
int fwd(const Args& k, float* out, void* ws, hipStream_t s) {
    constexpr int RPB = 256 / (D / 4);
    const Ws w = carve(ws, k.B, D);
    const int nblk = (int)((k.B + RPB - 1) / RPB);
    hipLaunchKernelGGL(loss_rows<D>, dim3(nblk), dim3(256), 0, s, k, w.part);
    hipLaunchKernelGGL(finish, dim3(1), dim3(64), 0, s, (const float*)w.part, nblk, k.B, k.reg, out);
    return last_rc();
}

template <int D>
int bwd(const Args& k, const float* go, float* gE, float* gT, float* gV, void* ws, hipStream_t s) {
    constexpr int RPB = 256 / (D / 4);
    const Ws w = carve(ws, k.B, D);
    hipError_t e;
    if ((e = hipMemsetAsync(gE, 0, (size_t)(k.nu + k.ni) * D * sizeof(float), s)) != hipSuccess) return hip_rc(e);
    if (gT && (e = hipMemsetAsync(gT, 0, (size_t)k.ni * D * sizeof(float), s)) != hipSuccess) return hip_rc(e);
    if (gV && (e = hipMemsetAsync(gV, 0, (size_t)k.ni * D * sizeof(float), s)) != hipSuccess) return hip_rc(e);
    const int nblk = (int)((k.B + RPB - 1) / RPB);
    hipLaunchKernelGGL(grad_rows<D>, dim3(nblk), dim3(256), 0, s, k, go, w.occU, w.coef, w.ku, w.ki);
    hipLaunchKernelGGL(sum_rows<D>, dim3((unsigned)((3 * k.B + 3) / 4)), dim3(256), 0, s, k, (const float*)w.occU,
                       (const float*)w.coef, (const int32_t*)w.ku, (const int32_t*)w.ki, gE, gT, gV);
    return last_rc();
}

}  // namespace freedom
}  // namespace rsx

using namespace rsx;

extern "C" size_t rsx_freedom_ws_bytes(int64_t batch, int32_t d) {
    if (batch < 1 || batch > freedom::kMaxBatch || (d != 64 && d != 128)) return 0;
    return freedom::carve(nullptr, batch, d).total;
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
    if (!freedom::aligned16(gE) || !freedom::aligned16(gT) || !freedom::aligned16(gV)) return RSX_ERR_ARG;
    hipStream_t s = as_stream(stream);
    gT = a->T ? gT : nullptr;
    gV = a->V ? gV : nullptr;
    return a->d == 64 ? freedom::bwd<64>(k, go, gE, gT, gV, ws, s) : freedom::bwd<128>(k, go, gE, gT, gV, ws, s);
}
