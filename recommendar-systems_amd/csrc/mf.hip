// mf.hip — BPR and VBPR matrix factorisation on gfx950: the row-gathered Linear forward,
// the fused triplet loss (forward + backward) and the dense Adam of one training batch.
//
// Replaces, per batch (reference paths relative to its root):
//   src/models/bpr.py:67-87     gather rows, dot, BPRLoss + EmbLoss
//   src/models/vbpr.py:69-98    item_linear over EVERY item's raw features, cat, gather, loss
//   src/common/loss.py:33-51    BPRLoss / EmbLoss
//   src/common/trainer.py:133,238  torch.optim.Adam on the dense gradients
//
// VBPR's projection only reaches the loss through the batch's positive and negative items,
// so it is computed for those 2 B rows (lin_rows_fwd, rows read in place through the index)
// and its weight gradient runs over the same 2 B rows (rsx_linear_rows_wgrad, linear.hip).
//
// lin_rows_fwd: a tall, skinny product (n = 2 B = 4096 rows, in_dim 1536..4480, out_dim 64).
// A block owns 32 output rows x out_dim; its waves split the K loop (wave w takes the
// 32-column steps w, w + NW, ...), each with OT = out_dim / 32 accumulators of
// v_mfma_f32_32x32x2_f32 (A = W[o][k], B = x[rows[r]][k], so a lane ends with 4 adjacent
// output columns of one row: float4 stores), and the partial strips are added in wave order
// through LDS.  Splitting K over the waves instead of sharing one staged W chunk among row
// tiles gives n / 32 blocks (128 at n = 4096) where 128-row blocks would give 32; W
// (out_dim x in_dim, at most 2.3 MB) is re-read by every block through L2.
#include <algorithm>
#include <type_traits>

#include "rsx_adam.hpp"
#include "rsx_common.hpp"

namespace rsx {

int sample_call(const rsx_sampler_args& s, int64_t batch, int64_t* out, hipStream_t st, int64_t bm, int64_t n_slices);

typedef float floatx16 __attribute__((ext_vector_type(16)));

// NW waves of a block split the K loop; each stages its own 32-column step of the block's
// 32 x rows and of W's out_dim rows in LDS.  Global loads are line-shaped (8 lanes x 16 B =
// one 128-B line of a row per instruction, every line fetched once); the MFMA operands are
// then read from LDS as float4 (lane (j, h): row j, columns 16 h .. 16 h + 15 of the step).
template <int OT, int NW>
__global__ __launch_bounds__(64 * NW) void lin_rows_fwd(const float* __restrict__ x, const float* __restrict__ W,
                                                        const float* __restrict__ b,
                                                        const int64_t* __restrict__ rows, int64_t n, int in_dim,
                                                        float* __restrict__ out, int64_t ld_out) {
    constexpr int LP = 36;  // padded LDS row: 32 columns + 4 (144 B, float4-aligned)
    __shared__ __attribute__((aligned(16))) float xs[NW][32 * LP];
    __shared__ __attribute__((aligned(16))) float wl[NW][32 * OT * LP];
    static_assert(NW * 32 * OT * LP >= (NW - 1) * OT * 16 * 64, "the strips' reduction reuses wl");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
    const int lr = lane >> 3, lc = (lane & 7) * 4;  // loader: rows lr + 8 i, columns lc .. lc + 3
    const int64_t r0 = (int64_t)blockIdx.x * 32;
    const int o0 = blockIdx.y * 32 * OT;  // the block's first output column (grid.y strips of 32 OT)
    W += (int64_t)o0 * in_dim;
    const float* xrow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t r = r0 + lr + 8 * i;
        xrow[i] = r < n ? x + (rows ? rows[r] : r) * in_dim : nullptr;
    }
    floatx16 acc[OT];
#pragma unroll
    for (int q = 0; q < OT; ++q)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[q][e] = 0.f;
    const int nsteps = (in_dim + 31) / 32;
    const int iters = (nsteps + NW - 1) / NW;  // block-uniform; a wave's steps past nsteps load zeros
    // two register sets: the loads of the next two steps are in flight while a step computes
    // (a wave has one block-step of loads per set; the loop is latency-bound without them)
    float4 xr[2][4], wr[2][4 * OT];
    auto gload = [&](int st, float4(&xv)[4], float4(&wv)[4 * OT]) __attribute__((always_inline)) {
        const int c = st * 32 + lc;
#pragma unroll
        for (int i = 0; i < 4; ++i) xv[i] = (xrow[i] && c < in_dim) ? ld4(xrow[i] + c) : f4(0.f);
#pragma unroll
        for (int i = 0; i < 4 * OT; ++i)
            wv[i] = c < in_dim ? ld4(W + (int64_t)(lr + 8 * i) * in_dim + c) : f4(0.f);
    };
    // one step from register set S: registers -> LDS, refill S with step it + 2, MFMAs from LDS
    auto step = [&](int it, auto sc) __attribute__((always_inline)) {
        constexpr int S = decltype(sc)::value;
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<float4*>(&xs[wave][(lr + 8 * i) * LP + lc]) = xr[S][i];
#pragma unroll
        for (int i = 0; i < 4 * OT; ++i) *reinterpret_cast<float4*>(&wl[wave][(lr + 8 * i) * LP + lc]) = wr[S][i];
        __syncthreads();
        if (it + 2 < iters) gload((it + 2) * NW + wave, xr[S], wr[S]);
        float4 xv[4];
#pragma unroll
        for (int f = 0; f < 4; ++f) xv[f] = *reinterpret_cast<const float4*>(&xs[wave][j * LP + 16 * h + 4 * f]);
#pragma unroll
        for (int q = 0; q < OT; ++q) {
            float4 wv[4];
#pragma unroll
            for (int f = 0; f < 4; ++f)
                wv[f] = *reinterpret_cast<const float4*>(&wl[wave][(32 * q + j) * LP + 16 * h + 4 * f]);
            // one MFMA sums the two halves' columns (k index = h), the same pairing for A and B
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[f].x, xv[f].x, acc[q], 0, 0, 0);
                acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[f].y, xv[f].y, acc[q], 0, 0, 0);
                acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[f].z, xv[f].z, acc[q], 0, 0, 0);
                acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[f].w, xv[f].w, acc[q], 0, 0, 0);
            }
        }
        __syncthreads();
    };
    gload(wave, xr[0], wr[0]);
    if (iters > 1) gload(NW + wave, xr[1], wr[1]);
    for (int it = 0; it < iters; it += 2) {  // block-uniform
        step(it, std::integral_constant<int, 0>{});
        if (it + 1 < iters) step(it + 1, std::integral_constant<int, 1>{});
    }
    // waves 1 .. NW-1 hand their strips to wave 0, which adds them in wave order
    float* red = &wl[0][0];
    if (wave > 0) {
#pragma unroll
        for (int q = 0; q < OT; ++q)
#pragma unroll
            for (int e = 0; e < 16; ++e) red[((wave - 1) * OT * 16 + q * 16 + e) * 64 + lane] = acc[q][e];
    }
    __syncthreads();
    const int64_t r = r0 + j;
    if (wave != 0 || r >= n) return;
    // C layout: lane holds row j, columns 32 q + 8 (e >> 2) + 4 h + (e & 3)
#pragma unroll
    for (int q = 0; q < OT; ++q) {
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int o = o0 + 32 * q + 8 * g4 + 4 * h;
            float v[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int e = 4 * g4 + t;
                v[t] = acc[q][e];
#pragma unroll
                for (int w = 0; w < NW - 1; ++w) v[t] += red[(w * OT * 16 + q * 16 + e) * 64 + lane];
                if (b) v[t] += b[o + t];
            }
            st4(out + r * ld_out + o, make_float4(v[0], v[1], v[2], v[3]));
        }
    }
}

// --------------------------------------------------------------------------------------
// loss: forward (scores, per-triplet coefficient, f64 partials) and backward (scatter)
// --------------------------------------------------------------------------------------
constexpr int kMfBlock = 256;

struct MfArgs {
    const float* U;
    const float* I;
    const float* proj;  // [2 batch, D]: positives then negatives (VB)
    const int64_t* trip;
    int64_t batch;
    float reg;
    float* gU;
    float* gI;
    float* gproj;
    float* loss_out;
    double* loss_acc;
    float* coef;   // [batch]
    double* part;  // [n_blocks][4]
    int32_t* halt;
    int32_t tag;
    int64_t* step_dev;  // optional: incremented once per step (read by the Adam launch)
};

template <int D, bool VB>
__global__ __launch_bounds__(kMfBlock) void mf_fwd(MfArgs a) {
    constexpr int G = D / 4, GPB = kMfBlock / G, DU = VB ? 2 * D : D;
    const int li = threadIdx.x % G;
    const int64_t t = (int64_t)blockIdx.x * GPB + threadIdx.x / G;
    double t_loss = 0.0, t_u = 0.0, t_p = 0.0, t_n = 0.0;
    if (t < a.batch) {
        const int64_t u = a.trip[t], p = a.trip[a.batch + t], n = a.trip[2 * a.batch + t];
        float sp = 0.f, sn = 0.f, qu = 0.f, qp = 0.f, qn = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int col = li + c * G;
            const float fu = a.U[u * DU + col], fp = a.I[p * D + col], fn = a.I[n * D + col];
            sp += fu * fp;
            sn += fu * fn;
            qu += fu * fu;
            qp += fp * fp;
            qn += fn * fn;
        }
        if constexpr (VB) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int col = li + c * G;
                const float fu = a.U[u * DU + D + col], fp = a.proj[t * D + col], fn = a.proj[(a.batch + t) * D + col];
                sp += fu * fp;
                sn += fu * fn;
                qu += fu * fu;
                qp += fp * fp;
                qn += fn * fn;
            }
        }
        sp = group_sum<G>(sp);
        sn = group_sum<G>(sn);
        const float delta = sp - sn;
        const float sg = 1.f / (1.f + expf(-delta));
        t_u = (double)qu;  // per-lane partials; summed across the block below
        t_p = (double)qp;
        t_n = (double)qn;
        if (li == 0) {
            // -log(1e-10 + sigmoid(delta)), mean over the batch (loss.py:33-35)
            a.coef[t] = -(sg * (1.f - sg)) / (1e-10f + sg) / (float)a.batch;
            t_loss = (double)(-logf(1e-10f + sg));
        }
    }
    // block reduction (fixed order: wave shuffles, then waves in order), as bpr_fwd
    __shared__ double red[kMfBlock / kWave][4];
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        t_loss += __shfl_xor(t_loss, o, kWave);
        t_u += __shfl_xor(t_u, o, kWave);
        t_p += __shfl_xor(t_p, o, kWave);
        t_n += __shfl_xor(t_n, o, kWave);
    }
    const int wv = threadIdx.x / kWave;
    if ((threadIdx.x % kWave) == 0) {
        red[wv][0] = t_loss;
        red[wv][1] = t_u;
        red[wv][2] = t_p;
        red[wv][3] = t_n;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        double s = 0.0;
        for (int w = 0; w < kMfBlock / kWave; ++w) s += red[w][threadIdx.x];
        a.part[(int64_t)blockIdx.x * 4 + threadIdx.x] = s;
    }
}

template <int D, bool VB>
__global__ __launch_bounds__(kMfBlock) void mf_bwd(MfArgs a, int n_part) {
    constexpr int G = D / 4, GPB = kMfBlock / G, DU = VB ? 2 * D : D;
    // every block reduces the per-block partials in the same fixed order (bpr_bwd's): the
    // regulariser's gradient needs the three global Frobenius norms before any row
    __shared__ double red[4][kMfBlock];
    __shared__ double tot[4];
    {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        for (int k = threadIdx.x; k < n_part; k += kMfBlock) {
            const double4 v = reinterpret_cast<const double4*>(a.part)[k];
            s0 += v.x;
            s1 += v.y;
            s2 += v.z;
            s3 += v.w;
        }
        red[0][threadIdx.x] = s0;
        red[1][threadIdx.x] = s1;
        red[2][threadIdx.x] = s2;
        red[3][threadIdx.x] = s3;
        __syncthreads();
        for (int w = kMfBlock / 2; w > 0; w >>= 1) {
            if (threadIdx.x < w) {
#pragma unroll
                for (int c = 0; c < 4; ++c) red[c][threadIdx.x] += red[c][threadIdx.x + w];
            }
            __syncthreads();
        }
        if (threadIdx.x < 4) tot[threadIdx.x] = red[threadIdx.x][0];
        __syncthreads();
    }
    const double B = (double)a.batch;
    const double nu = sqrt(tot[1]), np = sqrt(tot[2]), nn = sqrt(tot[3]);
    const double loss = tot[0] / B + (double)a.reg * (nu + np + nn) / B;
    const float ku = nu > 0 ? (float)((double)a.reg / (B * nu)) : 0.f;
    const float kp = np > 0 ? (float)((double)a.reg / (B * np)) : 0.f;
    const float kn = nn > 0 ? (float)((double)a.reg / (B * nn)) : 0.f;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (a.loss_out) a.loss_out[0] = (float)loss;
        if (a.loss_acc) a.loss_acc[0] += loss;
        if (a.halt && loss != loss && a.halt[0] == 0) {  // the first NaN batch: the Adam launch skips
            a.halt[1] = a.tag;
            a.halt[0] = 1;
        }
        if (a.step_dev) a.step_dev[0] += 1;
    }
    const int li = threadIdx.x % G;
    const int64_t t = (int64_t)blockIdx.x * GPB + threadIdx.x / G;
    if (t >= a.batch) return;
    const int64_t u = a.trip[t], p = a.trip[a.batch + t], n = a.trip[2 * a.batch + t];
    const float coef = a.coef[t];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int col = li + c * G;
        const float fu = a.U[u * DU + col], fp = a.I[p * D + col], fn = a.I[n * D + col];
        atomicAdd(a.gU + u * DU + col, coef * (fp - fn) + ku * fu);
        atomicAdd(a.gI + p * D + col, coef * fu + kp * fp);
        atomicAdd(a.gI + n * D + col, -coef * fu + kn * fn);
    }
    if constexpr (VB) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int col = li + c * G;
            const float fu = a.U[u * DU + D + col], fp = a.proj[t * D + col], fn = a.proj[(a.batch + t) * D + col];
            atomicAdd(a.gU + u * DU + D + col, coef * (fp - fn) + ku * fu);
            a.gproj[t * D + col] = coef * fu + kp * fp;  // one triplet per projected row: stored
            a.gproj[(a.batch + t) * D + col] = -coef * fu + kn * fn;
        }
    }
}

// --------------------------------------------------------------------------------------
// dense Adam over up to four tensors in one launch
// --------------------------------------------------------------------------------------
struct AdamSeg {
    float* p;
    float* m;
    float* v;
    float* g;
    int64_t n4;  // float4 groups
    int clear;   // g entries read as non-zero are cleared (the scatter scratch)
};

struct AdamJob {
    AdamSeg s[4];
    int nseg;
    rsx_adam adam;
    const int32_t* halt;
};

__global__ __launch_bounds__(256) void mf_adam(AdamJob j) {
    __shared__ AdamConst cs;
    if (threadIdx.x == 0) cs = adam_const(j.adam);
    __syncthreads();
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int k = 0;
    while (k < j.nseg && i >= j.s[k].n4) {
        i -= j.s[k].n4;
        ++k;
    }
    if (k >= j.nseg) return;
    const AdamSeg& sg = j.s[k];
    const AdamConst c = cs;
    const float4 g = ld4(sg.g + 4 * i);
    if (!(j.halt && j.halt[0])) {  // a NaN loss (this step's or an earlier one's): nothing moves
        float4 p = ld4(sg.p + 4 * i), m = ld4(sg.m + 4 * i), v = ld4(sg.v + 4 * i);
        adam_elem(c, p.x, m.x, v.x, g.x);
        adam_elem(c, p.y, m.y, v.y, g.y);
        adam_elem(c, p.z, m.z, v.z, g.z);
        adam_elem(c, p.w, m.w, v.w, g.w);
        st4(sg.p + 4 * i, p);
        st4(sg.m + 4 * i, m);
        st4(sg.v + 4 * i, v);
    }
    if (sg.clear && (g.x != 0.f || g.y != 0.f || g.z != 0.f || g.w != 0.f)) st4(sg.g + 4 * i, f4(0.f));
}

// --------------------------------------------------------------------------------------
// host side
// --------------------------------------------------------------------------------------
struct MfWs {
    size_t coef, part, proj, gproj, wg, total;
};

static MfWs mf_ws(int64_t batch, int d, int F) {
    MfWs w;
    const int64_t nb = (batch + 7) / 8 + 1;  // worst case d = 128: 8 triplets per block
    size_t off = 0;
    w.coef = off;
    off += al256((size_t)batch * sizeof(float));
    w.part = off;
    off += al256((size_t)nb * 4 * sizeof(double));
    w.proj = off;
    if (F > 0) off += al256((size_t)2 * batch * d * sizeof(float));
    w.gproj = off;
    if (F > 0) off += al256((size_t)2 * batch * d * sizeof(float));
    w.wg = off;
    if (F > 0) off += al256(rsx_linear_rows_wgrad_ws_bytes(2 * batch, d, F));
    w.total = off + 256;
    return w;
}

static bool mf_shape_ok(int d, int F) { return (d == 32 || d == 64 || d == 128) && F >= 0 && (F % 4) == 0; }

template <int D, bool VB>
static void launch_loss(const MfArgs& a, hipStream_t s) {
    constexpr int GPB = kMfBlock / (D / 4);
    const int nb = (int)((a.batch + GPB - 1) / GPB);
    hipLaunchKernelGGL((mf_fwd<D, VB>), dim3(nb), dim3(kMfBlock), 0, s, a);
    hipLaunchKernelGGL((mf_bwd<D, VB>), dim3(nb), dim3(kMfBlock), 0, s, a, nb);
}

// projection of the batch's item rows, loss forward + backward, weight gradient
static int mf_loss(const rsx_mf_step_args& st, int64_t batch, float* gU, float* gI, float* gW, float* gb,
                   int32_t* halt, int32_t tag, int64_t* step_dev, hipStream_t s) {
    const int d = st.d, F = st.F;
    const MfWs w = mf_ws(batch, d, F);
    if (!st.ws || st.ws_bytes < w.total) return RSX_ERR_WORKSPACE;
    char* base = static_cast<char*>(st.ws);
    float* proj = reinterpret_cast<float*>(base + w.proj);
    float* gproj = reinterpret_cast<float*>(base + w.gproj);
    const int64_t* item_rows = st.triplets + batch;  // positives then negatives: [2 batch]
    int rc;
    if (F > 0 && (rc = rsx_linear_rows_fwd(st.X, st.W, st.b, item_rows, 2 * batch, F, d, proj, d, s))) return rc;
    MfArgs a = {};
    a.U = st.U;
    a.I = st.I;
    a.proj = proj;
    a.trip = st.triplets;
    a.batch = batch;
    a.reg = st.reg;
    a.gU = gU;
    a.gI = gI;
    a.gproj = gproj;
    a.loss_out = st.loss_out;
    a.loss_acc = st.loss_acc;
    a.coef = reinterpret_cast<float*>(base + w.coef);
    a.part = reinterpret_cast<double*>(base + w.part);
    a.halt = halt;
    a.tag = tag;
    a.step_dev = step_dev;
    switch (d * 2 + (F > 0)) {
        case 32 * 2 + 0: launch_loss<32, false>(a, s); break;
        case 32 * 2 + 1: launch_loss<32, true>(a, s); break;
        case 64 * 2 + 0: launch_loss<64, false>(a, s); break;
        case 64 * 2 + 1: launch_loss<64, true>(a, s); break;
        case 128 * 2 + 0: launch_loss<128, false>(a, s); break;
        case 128 * 2 + 1: launch_loss<128, true>(a, s); break;
        default: return RSX_ERR_UNSUPPORTED;
    }
    if ((rc = last_rc())) return rc;
    if (F > 0)
        return rsx_linear_rows_wgrad(gproj, d, st.X, item_rows, 2 * batch, d, F, gW, gb, base + w.wg,
                                     rsx_linear_rows_wgrad_ws_bytes(2 * batch, d, F), s);
    return 0;
}

static int mf_check(const rsx_mf_step_args* st) {
    if (!st || !st->U || !st->I || !st->triplets || st->batch <= 0 || st->n_users <= 0 || st->n_items <= 0)
        return RSX_ERR_ARG;
    if (!mf_shape_ok(st->d, st->F)) return RSX_ERR_UNSUPPORTED;
    if (st->F > 0 && (!st->W || !st->b || !st->X)) return RSX_ERR_ARG;
    return 0;
}

}  // namespace rsx

using namespace rsx;

extern "C" int rsx_linear_rows_fwd(const float* x, const float* W, const float* b, const int64_t* rows, int64_t n,
                                   int32_t in_dim, int32_t out_dim, float* out, int64_t ld_out, rsx_stream_t stream) {
    if (n < 0 || in_dim <= 0 || out_dim <= 0) return RSX_ERR_ARG;
    if ((out_dim != 32 && out_dim != 64 && out_dim != 128) || (in_dim % 4)) return RSX_ERR_UNSUPPORTED;
    if (n == 0) return 0;
    if (!x || !W || !out || ld_out < out_dim || (ld_out % 4) || (reinterpret_cast<uintptr_t>(out) & 15)) return RSX_ERR_ARG;
    hipStream_t s = as_stream(stream);
    // a block takes 32 rows x (32 OT) columns: all of out_dim when the row tiles alone fill the
    // chip (x is then read once), else narrower strips over grid.y (f32 MFMA bounds the kernel at
    // n = 4096: 128 row tiles on 256 CUs would leave half of them idle).  The plan depends on
    // the shapes and the CU count only.
    const int64_t rb = (n + 31) / 32;
    int ot = out_dim / 32;
    while (ot > 1 && rb * (out_dim / 32 / ot) < device_cus()) ot /= 2;
    const dim3 grid((unsigned)rb, (unsigned)(out_dim / 32 / ot));
    switch (ot) {  // OT = 4: two waves a block (the W step alone is 18 KB of LDS a wave)
        case 1: hipLaunchKernelGGL((lin_rows_fwd<1, 4>), grid, dim3(256), 0, s, x, W, b, rows, n, (int)in_dim, out, ld_out); break;
        case 2: hipLaunchKernelGGL((lin_rows_fwd<2, 4>), grid, dim3(256), 0, s, x, W, b, rows, n, (int)in_dim, out, ld_out); break;
        default: hipLaunchKernelGGL((lin_rows_fwd<4, 2>), grid, dim3(128), 0, s, x, W, b, rows, n, (int)in_dim, out, ld_out); break;
    }
    return last_rc();
}

extern "C" size_t rsx_mf_ws_bytes(int64_t batch, int32_t d, int32_t F) {
    if (batch <= 0 || !mf_shape_ok(d, F)) return 0;
    return mf_ws(batch, d, F).total;
}

extern "C" int rsx_mf_loss_grad(const rsx_mf_step_args* st, float* gU, float* gI, float* gW, float* gb,
                                rsx_stream_t stream) {
    int rc = mf_check(st);
    if (rc) return rc;
    if (!gU || !gI || (st->F > 0 && (!gW || !gb))) return RSX_ERR_ARG;
    hipStream_t s = as_stream(stream);
    const int du = st->F > 0 ? 2 * st->d : st->d;
    hipError_t e = hipMemsetAsync(gU, 0, (size_t)st->n_users * du * sizeof(float), s);
    if (e != hipSuccess) return hip_rc(e);
    e = hipMemsetAsync(gI, 0, (size_t)st->n_items * st->d * sizeof(float), s);
    if (e != hipSuccess) return hip_rc(e);
    return mf_loss(*st, st->batch, gU, gI, gW, gb, nullptr, 0, nullptr, s);
}

extern "C" int rsx_mf_step(const rsx_mf_step_args* st, rsx_stream_t stream) {
    int rc = mf_check(st);
    if (rc) return rc;
    if (!st->mU || !st->vU || !st->mI || !st->vI || !st->gU || !st->gI) return RSX_ERR_ARG;
    if (st->F > 0 && (!st->mW || !st->vW || !st->mb || !st->vb || !st->gW || !st->gb)) return RSX_ERR_ARG;
    if (st->halt && (st->tag <= 0 || st->tag > INT32_MAX)) return RSX_ERR_ARG;
    hipStream_t s = as_stream(stream);
    int64_t batch = st->batch;
    if (st->sample) {
        const rsx_sampler_args& sa = *st->sample;
        if ((rc = sample_call(sa, st->batch, st->triplets, s, 0, 0))) return rc;
        batch = (sa.n_inter - sa.start) < st->batch ? (sa.n_inter - sa.start) : st->batch;
    }
    if ((rc = mf_loss(*st, batch, st->gU, st->gI, st->gW, st->gb, st->halt, (int32_t)st->tag, st->step_dev, s)))
        return rc;
    const int d = st->d, F = st->F, du = F > 0 ? 2 * d : d;
    AdamJob j = {};
    j.s[0] = {st->U, st->mU, st->vU, st->gU, st->n_users * du / 4, 1};
    j.s[1] = {st->I, st->mI, st->vI, st->gI, st->n_items * d / 4, 1};
    j.nseg = 2;
    if (F > 0) {
        j.s[2] = {st->W, st->mW, st->vW, st->gW, (int64_t)d * F / 4, 0};
        j.s[3] = {st->b, st->mb, st->vb, st->gb, d / 4, 0};
        j.nseg = 4;
    }
    j.adam = st->adam;
    if (st->step_dev) j.adam.step_dev = st->step_dev;
    j.halt = st->halt;
    int64_t tot = 0;
    for (int k = 0; k < j.nseg; ++k) tot += j.s[k].n4;
    hipLaunchKernelGGL(mf_adam, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, j);
    return last_rc();
}
