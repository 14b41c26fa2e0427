// dense.hip — the dense layer blocks the models share, on gfx950 (f32 MFMA: exact f32 products,
// f32 sums).  MMGCN's layer 1 and image MLP, GRCN's and DualGNN's content MLPs and their
// F.normalize run on these; no model's own kernels live here (rsx/dense.py is the Python side).
//
//  * gemm: Y[n, N] = epilogue((X .* slope(Mx)) op(B) + bias), X optionally two column segments
//    of two tables (a [h | x_hat] operand is never concatenated), B given [K, N] or [N, K], the
//    epilogue leaky, a multiplication by slope(My) and a residual.  With Mx = the saved output
//    and the other layout of B it is the data gradient of the same product.
//    A 64 x 64 output tile a block, 16 x 64 a wave, K in 32-wide slabs staged in LDS with the
//    next slab's global loads in flight during the MFMAs.
//  * normalize_fwd / normalize_bwd: F.normalize over rows, one wave a row, and torch's backward.
//  * colsum_part / colsum_fin (the bias gradients): block partial column sums, added in block
//    order.
//  * leaky_bwd: g .* slope(y), the masked gradient rows of leaky(X W^T + b) when no data-gradient
//    launch forms them.
//
// Slopes are read off the sign of the saved f32 outputs (leaky(p) > 0 exactly when p > 0, the
// slope being positive): no mask tensors.  No float atomics anywhere: two runs are bit-equal.
#include <cmath>

#include "smore_fld.hpp"

namespace rsx {
namespace dense {

using namespace rsx::sf;

// ---------------------------------------------------------------------------
// the wide product
// ---------------------------------------------------------------------------
constexpr int kBM = 64, kBN = 64, kKS = 32, kLdT = kKS + 4;  // tile rows padded: conflict-free float4 reads

__global__ __launch_bounds__(256) void gemm(rsx_dense_gemm_args a) {
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
// the leaky mask
// ---------------------------------------------------------------------------
// out = g .* slope(y), y a saved leaky_relu output (slope kSlope where y <= 0)
__global__ __launch_bounds__(256) void leaky_bwd(const float* __restrict__ g, const float* __restrict__ y, int64_t n4,
                                                 float* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 gv = ld4(g + 4 * i), yv = ld4(y + 4 * i);
        st4(out + 4 * i, make_float4(yv.x > 0.f ? gv.x : kSlope * gv.x, yv.y > 0.f ? gv.y : kSlope * gv.y,
                                     yv.z > 0.f ? gv.z : kSlope * gv.z, yv.w > 0.f ? gv.w : kSlope * gv.w));
    }
}

}  // namespace dense
}  // namespace rsx

using namespace rsx;

extern "C" {

int rsx_dense_gemm(const rsx_dense_gemm_args* a, rsx_stream_t stream) {
    if (!a || a->n < 0 || !a->x0 || !a->B || (!a->y && !a->y2) || (a->k1 > 0 && !a->x1)) return RSX_ERR_ARG;
    if (a->n_out <= 0 || a->k0 <= 0 || a->k1 < 0) return RSX_ERR_ARG;
    if ((a->n_out % 32) || (a->k0 % 4) || (a->k1 % 4) || a->n_out > 65535 * dense::kBN) return RSX_ERR_UNSUPPORTED;
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
    const int64_t gx = (a->n + dense::kBM - 1) / dense::kBM;
    if (gx > 0x7fffffffll) return RSX_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)gx, (unsigned)((a->n_out + dense::kBN - 1) / dense::kBN));
    hipLaunchKernelGGL(dense::gemm, grid, dim3(256), 0, as_stream(stream), *a);
    return last_rc();
}

int rsx_dense_normalize_fwd(const float* x, int64_t n, int32_t w, float* y, float* den, rsx_stream_t stream) {
    if (n < 0 || w <= 0 || !x || !y || !den || !aligned16(x) || !aligned16(y)) return RSX_ERR_ARG;
    if (w % 4) return RSX_ERR_UNSUPPORTED;
    if (n == 0) return RSX_OK;
    hipLaunchKernelGGL(dense::normalize_fwd, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, as_stream(stream), x, n, (int)w,
                       y, den);
    return last_rc();
}

int rsx_dense_normalize_bwd(const float* gy, const float* y, const float* den, int64_t n, int32_t w, float* gx,
                            rsx_stream_t stream) {
    if (n < 0 || w <= 0 || !gy || !y || !den || !gx || !aligned16(gy) || !aligned16(y) || !aligned16(gx))
        return RSX_ERR_ARG;
    if (w % 4) return RSX_ERR_UNSUPPORTED;
    if (n == 0) return RSX_OK;
    hipLaunchKernelGGL(dense::normalize_bwd, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, as_stream(stream), gy, y, den,
                       n, (int)w, gx);
    return last_rc();
}

size_t rsx_dense_colsum_ws_bytes(int64_t n, int32_t n_cols) {
    if (n <= 0 || n_cols <= 0) return 0;
    return (size_t)((n + dense::kColRows - 1) / dense::kColRows) * (size_t)n_cols * sizeof(float);
}

int rsx_dense_colsum(const float* g, int64_t n, int32_t n_cols, float* out, void* ws, size_t ws_bytes,
                     rsx_stream_t stream) {
    if (n < 0 || n_cols <= 0 || !out || (n > 0 && !g)) return RSX_ERR_ARG;
    hipStream_t s = as_stream(stream);
    const unsigned gy = (unsigned)((n_cols + 255) / 256);
    const int64_t nblk = (n + dense::kColRows - 1) / dense::kColRows;
    if (n > 0 && (!ws || ws_bytes < rsx_dense_colsum_ws_bytes(n, n_cols))) return RSX_ERR_WORKSPACE;
    if (nblk > 0x7fffffffll) return RSX_ERR_UNSUPPORTED;
    float* part = static_cast<float*>(ws);
    if (n > 0) hipLaunchKernelGGL(dense::colsum_part, dim3((unsigned)nblk, gy), dim3(256), 0, s, g, n, (int)n_cols, part);
    hipLaunchKernelGGL(dense::colsum_fin, dim3(gy), dim3(256), 0, s, (const float*)part, nblk, (int)n_cols, out);
    return last_rc();
}

int rsx_dense_leaky_bwd(const float* g, const float* y, int64_t n_elems, float* out, rsx_stream_t stream) {
    if (n_elems < 0 || !g || !y || !out || !aligned16(g) || !aligned16(y) || !aligned16(out)) return RSX_ERR_ARG;
    if (n_elems % 4) return RSX_ERR_UNSUPPORTED;
    if (n_elems == 0) return RSX_OK;
    const int64_t nb = (n_elems / 4 + 255) / 256;  // >= 1; grid-stride past 4096 blocks
    hipLaunchKernelGGL(dense::leaky_bwd, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(256), 0, as_stream(stream), g, y,
                       n_elems / 4, out);
    return last_rc();
}

}  // extern "C"
