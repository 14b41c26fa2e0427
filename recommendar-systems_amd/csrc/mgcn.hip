// mgcn.hip — MGCN's two per-row blocks (gfx950, f32 MFMA: exact f32 products, f32 sums),
// in the row-field layout of smore_fuse.hip (smore_fld.hpp: a 16-row tile of [rows x D]
// in a wave as the transposed accumulator layout of v_mfma_f32_16x16x4f32; a chain of
// Linears and activations stays in registers, weights staged in LDS per block).
//
// Replaces, per MGCN forward / backward (reference src/models/mgcn.py):
//  * the behaviour-guided purifier  item * sigmoid(Linear(feats_m)), m = image, text
//                                                                     (:152-154)
//  * the behaviour-aware fuser: the shared query MLP d -> d -> 1 on the image and the text
//    row, the two-way softmax, common / separated parts, the two preference gates on the
//    content row, side = (sep_i + sep_t + common) / 3, all = content + side
//                                                                     (:187-201)
// each one forward launch and one backward launch.  The Linear weight gradients come from
// rsx_smore_wgrad on the pre-activation gradient rows the backwards write; the [1, d]
// second query weight's gradient is reduced here (per-block partial rows, then one block
// summing them in a fixed order).
//
// The fuser's backward recomputes the forward's activations (four products) rather than
// reading saved ones: see DESIGN §3 for the byte and product count.  In the rows form the
// three table gradients are written per occurrence and summed per table row in ascending
// occurrence order (fuse_segsum): deterministic, no float atomics.
#include <cmath>

#include "rsx_common.hpp"
#include "smore_fld.hpp"

namespace rsx {
namespace mg {

using namespace rsx::sf;

// ---------------------------------------------------------------------------
// purifier (mgcn.py:152-154)
// ---------------------------------------------------------------------------
struct PurArgs {
    const float* feat[2];   // projected image / text features [n, D]
    const float* item;      // item-id embedding [n, D]
    const float* W[2];      // gate_v.0 / gate_t.0 weights [D, D]
    const float* b[2];
    int64_t n;
    int64_t nbx;            // 64-row blocks of n (grid.x may be fewer: blocks stride over them)
    float* out[2];          // forward
    const float* gout[2];   // backward: their gradients (NULL = zero)
    float* g_item;
    float* g_feat[2];
    float* dz[2];           // pre-activation gradients (wgrad rows)
};

__device__ __forceinline__ int64_t tile_row(int64_t bx, int64_t nbx, int64_t n) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (bx * 4 + (threadIdx.x >> 6)) * 16 + (lane & 15);
    return bx < nbx && r < n ? r : (int64_t)-1;
}

// one gate per block row (grid.y = 2): its weight staged once per block
template <int D>
__global__ __launch_bounds__(256) void purify_fwd(PurArgs a) {
    __shared__ __attribute__((aligned(16))) float wl[D * kLd<D>];
    const int lane = threadIdx.x & 63, g = lane >> 4;
    const int m = (int)blockIdx.y;
    const float* W = stage_w<D>(wl, a.W[m]);
#pragma unroll 1
    for (int64_t bx = blockIdx.x; bx < a.nbx; bx += gridDim.x) {  // block-uniform
        const int64_t row = tile_row(bx, a.nbx, a.n);
        const Fld<D> f = fload<D>(a.feat[m], row, g);
        const Fld<D> it = fload<D>(a.item, row, g);
        const Fld<D> s = fmap<D>(mv_p<D, kLd<D>>(W, a.b[m], f, lane), sigm);
        fstore<D>(a.out[m], row, g, fmap2<D>(it, s, [](float x, float y) { return x * y; }));
    }
}

// g_item needs both sigmoids of a row: one block runs the two gates of its row blocks
template <int D>
__global__ __launch_bounds__(256) void purify_bwd(PurArgs a) {
    __shared__ __attribute__((aligned(16))) float wl[D * kLd<D>];
    const int lane = threadIdx.x & 63, g = lane >> 4;
#pragma unroll 1
    for (int64_t bx = blockIdx.x; bx < a.nbx; bx += gridDim.x) {  // block-uniform
        const int64_t row = tile_row(bx, a.nbx, a.n);
        const Fld<D> it = fload<D>(a.item, row, g);
        Fld<D> gi = fzero<D>();
#pragma unroll 1
        for (int m = 0; m < 2; ++m) {
            const Fld<D> go = a.gout[m] ? fload<D>(a.gout[m], row, g) : fzero<D>();
            const Fld<D> f = fload<D>(a.feat[m], row, g);
            const float* W = stage_w<D>(wl, a.W[m]);
            const Fld<D> s = fmap<D>(mv_p<D, kLd<D>>(W, a.b[m], f, lane), sigm);
            gi = fmap3<D>(gi, go, s, [](float acc, float x, float y) { return acc + x * y; });
            const Fld<D> dz = fmap3<D>(go, it, s, [](float x, float y, float z) { return (x * y) * ((1.f - z) * z); });
            fstore<D>(a.dz[m], row, g, dz);
            fstore<D>(a.g_feat[m], row, g, mvt_p<D, kLd<D>>(W, dz, lane));
        }
        fstore<D>(a.g_item, row, g, gi);
    }
}

// ---------------------------------------------------------------------------
// fuser (mgcn.py:187-201)
// ---------------------------------------------------------------------------
enum { kW1 = 0, kW2, kWip, kWtp, kNW };
enum { kDz1I = 0, kDz1S, kDzIp, kDzTp, kNDz };

struct FuseArgs {
    const float* W[kNW];     // query_common.0 [D, D], query_common.2 [1, D], gate_{image,text}_prefer.0 [D, D]
    const float* b[kNW];     // biases (query_common.2 has none)
    const float* C;          // content / image-view / text-view tables
    const float* I;
    const float* T;
    const int64_t* rows;     // logical row r reads the tables at rows[r] (NULL: r)
    int64_t n;
    float* all;              // forward outputs (compact in the rows form)
    float* side;
    float* c_out;            // rows form: the gathered content / text rows (optional)
    float* t_out;
    const float* g_all;      // backward inputs (g_side, g_cin may be NULL)
    const float* g_side;
    const float* g_cin;
    float* gC;               // backward outputs: tables (full form) or [3][n][D] per-occurrence
    float* gI;               // rows (rows form: gC = slot 0, gI = 1, gT = 2, summed by fuse_segsum)
    float* gT;
    float* dz[kNDz];         // gradient rows: dz1I, dz1I + dz1T (W1's pre-activation on I, T), Wip, Wtp
    float* dif;              // the rows I - T (dW1 = dz1I^T (I - T) + (dz1I + dz1T)^T T)
    float* part;             // [grid.x][D] per-block partial rows of d w2
    int32_t* lead;           // rows form, [2][table rows], cleared before the launch: n - (the first
                             // occurrence of the table row), then the row's occurrence count
    int64_t n_table;
};

__device__ __forceinline__ int64_t src_row(const FuseArgs& a, int64_t r) { return (r >= 0 && a.rows) ? a.rows[r] : r; }

// softmax over the two scores
__device__ __forceinline__ void soft2(float aI, float aT, float& wI, float& wT) {
    const float mx = fmaxf(aI, aT);
    const float eI = expf(aI - mx), eT = expf(aT - mx);
    const float s = eI + eT;
    wI = eI / s;
    wT = eT / s;
}

template <int D>
__global__ __launch_bounds__(256) void fuse_fwd(FuseArgs a) {
    __shared__ __attribute__((aligned(16))) float wl[D * kLd<D>];
    const int lane = threadIdx.x & 63, g = lane >> 4;
    const int64_t n0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
    const int64_t out = n0 + (lane & 15) < a.n ? n0 + (lane & 15) : -1;
    const int64_t row = src_row(a, out);
    const auto mul = [](float x, float y) { return x * y; };
    const Fld<D> I = fload<D>(a.I, row, g);
    const Fld<D> T = fload<D>(a.T, row, g);
    fstore<D>(a.t_out, out, g, T);
    float wI, wT;
    {
        const float* W = stage_w<D>(wl, a.W[kW1]);
        const Fld<D> w2 = fvec<D>(a.W[kW2], g);
        const float aI = rsum<D>(fmap2<D>(fmap<D>(mv_p<D, kLd<D>>(W, a.b[kW1], I, lane), tanh_), w2, mul));
        const float aT = rsum<D>(fmap2<D>(fmap<D>(mv_p<D, kLd<D>>(W, a.b[kW1], T, lane), tanh_), w2, mul));
        soft2(aI, aT, wI, wT);
    }
    const Fld<D> cm = fmap2<D>(I, T, [&](float x, float y) { return wI * x + wT * y; });
    const Fld<D> C = fload<D>(a.C, row, g);
    fstore<D>(a.c_out, out, g, C);
    const Fld<D> pI = fmap<D>(mv_p<D, kLd<D>>(stage_w<D>(wl, a.W[kWip]), a.b[kWip], C, lane), sigm);
    Fld<D> sd = fmap3<D>(pI, I, cm, [](float p, float x, float c) { return p * (x - c); });
    const Fld<D> pT = fmap<D>(mv_p<D, kLd<D>>(stage_w<D>(wl, a.W[kWtp]), a.b[kWtp], C, lane), sigm);
    sd = fmap2<D>(sd, fmap3<D>(pT, T, cm, [](float p, float x, float c) { return p * (x - c); }),
                  [](float u, float v) { return u + v; });
    sd = fmap2<D>(sd, cm, [](float u, float c) { return (u + c) / 3.f; });
    fstore<D>(a.side, out, g, sd);
    fstore<D>(a.all, out, g, fmap2<D>(C, sd, [](float u, float v) { return u + v; }));
}

// Backward of one 16-row tile a wave.  With gs = (g_all + g_side) / 3:
//   d pI = gs (I - cm), d pT = gs (T - cm), d cm = gc = gs (1 - pI - pT),
//   d aI = wI wT <gc, I - T> = -d aT   (the two-way softmax: one is computed, the other
//   is its negation, so the nearly cancelling sums d W1 / d b1 / d w2 cancel exactly where
//   I = T),
//   d I = gs pI + wI gc + W1^T dz1I,  d T likewise,  d C = g_all (+ g_cin) + Wip^T dzip + Wtp^T dztp.
// W1 sees the image and the text row, dz1I = d aI w2 (1 - hI^2) and dz1T = -d aI w2 (1 - hT^2):
// where I ~ T the two row sets' weight-gradient sums cancel to a small fraction of their
// size, so the rows written are dz1I with the input I - T and
// dz1I + dz1T = d aI w2 (hT - hI)(hT + hI) with the input T (each formed without the
// cancellation): dW1 = dz1I^T (I - T) + (dz1I + dz1T)^T T, db1 = colsum (dz1I + dz1T).
template <int D>
__global__ __launch_bounds__(256) void fuse_bwd(FuseArgs a) {
    __shared__ __attribute__((aligned(16))) float wl[D * kLd<D>];
    __shared__ float red[4][D];
    const int lane = threadIdx.x & 63, g = lane >> 4, wave = threadIdx.x >> 6;
    const int64_t n0 = ((int64_t)blockIdx.x * 4 + wave) * 16;
    const int64_t out = n0 + (lane & 15) < a.n ? n0 + (lane & 15) : -1;
    const int64_t row = src_row(a, out);
    // rows form: per-occurrence rows (slot s of [3][n][D]); full form: the table rows
    const int64_t dst = a.rows ? out : row;
    const auto mul = [](float x, float y) { return x * y; };
    const auto add = [](float x, float y) { return x + y; };
    const auto sig_bwd = [](float gy, float y) { return gy * ((1.f - y) * y); };
    const Fld<D> I = fload<D>(a.I, row, g);
    const Fld<D> T = fload<D>(a.T, row, g);
    fstore<D>(a.dif, out, g, fmap2<D>(I, T, [](float x, float y) { return x - y; }));
    if (a.lead && out >= 0 && g == 0) {  // integer atomics: the same words whatever the order
        atomicMax(a.lead + row, (int32_t)(a.n - out));
        atomicAdd(a.lead + a.n_table + row, 1);
    }
    Fld<D> hI, hT;
    float wI, wT;
    {
        const float* W = stage_w<D>(wl, a.W[kW1]);
        const Fld<D> w2 = fvec<D>(a.W[kW2], g);
        hI = fmap<D>(mv_p<D, kLd<D>>(W, a.b[kW1], I, lane), tanh_);
        hT = fmap<D>(mv_p<D, kLd<D>>(W, a.b[kW1], T, lane), tanh_);
        soft2(rsum<D>(fmap2<D>(hI, w2, mul)), rsum<D>(fmap2<D>(hT, w2, mul)), wI, wT);
    }
    Fld<D> pI, pT;
    {
        const Fld<D> C = fload<D>(a.C, row, g);
        pI = fmap<D>(mv_p<D, kLd<D>>(stage_w<D>(wl, a.W[kWip]), a.b[kWip], C, lane), sigm);
        pT = fmap<D>(mv_p<D, kLd<D>>(stage_w<D>(wl, a.W[kWtp]), a.b[kWtp], C, lane), sigm);
    }
    Fld<D> gI, gT, dzt;
    float daI;
    {
        const Fld<D> gA = fload<D>(a.g_all, out, g);
        const Fld<D> gs = a.g_side ? fmap2<D>(gA, fload<D>(a.g_side, out, g), [](float u, float v) { return (u + v) / 3.f; })
                                   : fmap<D>(gA, [](float u) { return u / 3.f; });
        const Fld<D> cm = fmap2<D>(I, T, [&](float x, float y) { return wI * x + wT * y; });
        const Fld<D> gc = fmap3<D>(gs, pI, pT, [](float u, float p, float q) { return u * ((1.f - p) - q); });
        daI = (wI * wT) * rsum<D>(fmap3<D>(gc, I, T, [](float u, float x, float y) { return u * (x - y); }));
        fstore<D>(a.dz[kDzIp], out, g,
                  fmap2<D>(fmap3<D>(gs, I, cm, [](float u, float x, float c) { return u * (x - c); }), pI, sig_bwd));
        dzt = fmap2<D>(fmap3<D>(gs, T, cm, [](float u, float x, float c) { return u * (x - c); }), pT, sig_bwd);
        fstore<D>(a.dz[kDzTp], out, g, dzt);
        gI = fmap3<D>(gs, pI, gc, [&](float u, float p, float c) { return u * p + wI * c; });
        gT = fmap3<D>(gs, pT, gc, [&](float u, float p, float c) { return u * p + wT * c; });
    }
    // d C, first share: the text gate's weight is still staged
    Fld<D> gC = mvt_p<D, kLd<D>>(wl, dzt, lane);
    {
        // d w2: this block's 64 rows of d aI (hI - hT), summed over the tile's rows (lanes
        // n = 0..15 of each feature group), then over the four waves in wave order
        const Fld<D> q = fmap2<D>(hI, hT, [&](float x, float y) { return daI * (x - y); });
#pragma unroll
        for (int t = 0; t < D / 16; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = q.f[t][r];
                v += __shfl_xor(v, 1, kWave);
                v += __shfl_xor(v, 2, kWave);
                v += __shfl_xor(v, 4, kWave);
                v += __shfl_xor(v, 8, kWave);
                if ((lane & 15) == 0) red[wave][16 * t + 4 * g + r] = v;
            }
    }
    {
        const Fld<D> w2 = fvec<D>(a.W[kW2], g);
        fstore<D>(a.dz[kDz1S], out, g,
                  fmap3<D>(hI, hT, w2, [&](float x, float y, float w) { return (daI * w) * ((y - x) * (y + x)); }));
        hI = fmap2<D>(hI, w2, [&](float y, float w) { return (daI * w) * (1.f - y * y); });
        hT = fmap2<D>(hT, w2, [&](float y, float w) { return (-daI * w) * (1.f - y * y); });
        fstore<D>(a.dz[kDz1I], out, g, hI);
    }
    {
        const float* W = stage_w<D>(wl, a.W[kW1]);  // (its barriers also order the writes of `red`)
        if (threadIdx.x < D)
            a.part[(int64_t)blockIdx.x * D + threadIdx.x] =
                ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
        gI = fmap2<D>(gI, mvt_p<D, kLd<D>>(W, hI, lane), add);
        fstore<D>(a.gI, dst, g, gI);
        gT = fmap2<D>(gT, mvt_p<D, kLd<D>>(W, hT, lane), add);
        fstore<D>(a.gT, dst, g, gT);
    }
    {
        const float* W = stage_w<D>(wl, a.W[kWip]);
        const Fld<D> dzi = fload<D>(a.dz[kDzIp], out, g);  // this lane's own store above
        gC = fmap2<D>(mvt_p<D, kLd<D>>(W, dzi, lane), gC, add);
        Fld<D> gA = fload<D>(a.g_all, out, g);
        if (a.g_cin) gA = fmap2<D>(gA, fload<D>(a.g_cin, out, g), add);
        fstore<D>(a.gC, dst, g, fmap2<D>(gA, gC, add));
    }
}

// d w2 = the per-block partial rows summed in block order: 256 / D slices of the blocks,
// each in ascending order, then the slices in slice order (one block; deterministic)
template <int D>
__global__ __launch_bounds__(256) void fuse_dw2(const float* __restrict__ part, int64_t nblk, float* __restrict__ dw2) {
    constexpr int S = 256 / D;
    __shared__ float red[S][D];
    const int c = threadIdx.x % D, s = threadIdx.x / D;
    float acc = 0.f;
    for (int64_t p = s; p < nblk; p += S) acc += part[p * D + c];
    red[s][c] = acc;
    __syncthreads();
    if (s == 0) {
        float v = red[0][c];
#pragma unroll
        for (int k = 1; k < S; ++k) v += red[k][c];
        dw2[c] = v;
    }
}

// The rows form's per-occurrence rows summed per table row, deterministic: one wave per
// occurrence j; the first occurrence of its table row (fuse_bwd left n - j in lead[row] and
// the row's occurrence count beside it) adds the later occurrences in ascending order and
// stores the row of the three tables.  Table rows no occurrence names keep the zero fill.
// A row that occurs once is copied; otherwise the row ids after j are scanned, kSegU chunks
// of 64 a step (their loads in flight together), until the count is reached.  The matching
// occurrences are listed, ascending, in the wave's LDS list and then added kSegB at a time,
// their rows' loads issued together (a popular item's several hundred occurrences one by one
// would be the launch's tail).
constexpr int kSegU = 8, kSegList = 128;
template <int D>
__global__ __launch_bounds__(256) void fuse_segsum(const int64_t* __restrict__ rows, int64_t n,
                                                   const int32_t* __restrict__ lead, int64_t n_table,
                                                   const float* __restrict__ occ, float* __restrict__ gC,
                                                   float* __restrict__ gI, float* __restrict__ gT) {
    constexpr int F = D / 64, kSegB = D <= 64 ? 8 : 4;  // (32 at d = 64 measured 2.7x slower)
    __shared__ int32_t lists[4][kSegList];
    const int lane = threadIdx.x & 63;
    int32_t* lst = lists[threadIdx.x >> 6];  // this wave's own list: no block barrier involved
    const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // wave-uniform
    if (j >= n) return;
    const int64_t r = rows[j];
    if ((int64_t)lead[r] != n - j) return;  // an earlier occurrence leads
    int left = lead[n_table + r] - 1;       // later occurrences to find (wave-uniform)
    float acc[3][F];
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
        for (int f = 0; f < F; ++f) acc[s][f] = occ[((int64_t)s * n + j) * D + 64 * f + lane];
    int cnt = 0;  // wave-uniform
    auto flush = [&]() __attribute__((always_inline)) {
        for (int i0 = 0; i0 < cnt; i0 += kSegB) {
            float v[kSegB][3][F];
#pragma unroll
            for (int t = 0; t < kSegB; ++t) {
                const int64_t k = i0 + t < cnt ? (int64_t)lst[i0 + t] : j;  // (a padded slot reloads j, unused)
#pragma unroll
                for (int s = 0; s < 3; ++s)
#pragma unroll
                    for (int f = 0; f < F; ++f) v[t][s][f] = occ[((int64_t)s * n + k) * D + 64 * f + lane];
            }
#pragma unroll
            for (int t = 0; t < kSegB; ++t) {
                if (i0 + t >= cnt) break;  // wave-uniform
#pragma unroll
                for (int s = 0; s < 3; ++s)
#pragma unroll
                    for (int f = 0; f < F; ++f) acc[s][f] += v[t][s][f];
            }
        }
        cnt = 0;
    };
    for (int64_t base = j + 1; base < n && left > 0; base += 64 * kSegU) {
        unsigned long long m[kSegU];
#pragma unroll
        for (int u = 0; u < kSegU; ++u) {
            const int64_t i = base + 64 * u + lane;
            const int64_t v = rows[i < n ? i : j];
            m[u] = __ballot((i < n) & (v == r));
        }
#pragma unroll
        for (int u = 0; u < kSegU; ++u) {  // the chunks in order: occurrences ascending
            unsigned long long hit = m[u];
            while (hit) {
                const int b = __builtin_ctzll(hit);
                hit &= hit - 1;
                --left;
                if (lane == 0) lst[cnt] = (int32_t)(base + 64 * u + b);
                if (++cnt == kSegList) flush();
            }
        }
    }
    flush();
    float* const tab[3] = {gC, gI, gT};
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
        for (int f = 0; f < F; ++f) tab[s][r * D + 64 * f + lane] = acc[s][f];
}

}  // namespace mg
}  // namespace rsx

using namespace rsx;

extern "C" {

int rsx_mgcn_purify(int32_t backward, const float* const* feat, const float* item, const float* const* W,
                    const float* const* b, int64_t n, int32_t d, float* const* out, const float* const* gout,
                    float* g_item, float* const* g_feat, float* const* dz, rsx_stream_t stream) {
    if (n < 0 || !feat || !item || !W || !b) return RSX_ERR_ARG;
    if (d != 64 && d != 128) return RSX_ERR_UNSUPPORTED;
    if (n == 0) return RSX_OK;
    mg::PurArgs a{};
    for (int m = 0; m < 2; ++m) {
        if (!feat[m] || !W[m] || !b[m]) return RSX_ERR_ARG;
        a.feat[m] = feat[m];
        a.W[m] = W[m];
        a.b[m] = b[m];
        if (backward) {
            if (!g_feat || !dz || !g_feat[m] || !dz[m]) return RSX_ERR_ARG;
            a.gout[m] = gout ? gout[m] : nullptr;
            a.g_feat[m] = g_feat[m];
            a.dz[m] = dz[m];
        } else {
            if (!out || !out[m]) return RSX_ERR_ARG;
            a.out[m] = out[m];
        }
    }
    if (backward && !g_item) return RSX_ERR_ARG;
    a.item = item;
    a.n = n;
    a.g_item = g_item;
    a.nbx = ((n + 15) / 16 + 3) / 4;
    // at most two blocks a CU (the LDS weight copy allows two); each strides over its row blocks
    const unsigned gy = backward ? 1u : 2u;
    int64_t gx = a.nbx;
    const int64_t cap = (int64_t)(2 * device_cus()) / gy;
    if (gx > cap) gx = cap;
    const dim3 grid((unsigned)gx, gy);
    hipStream_t s = as_stream(stream);
    if (d == 64) {
        if (backward) hipLaunchKernelGGL(mg::purify_bwd<64>, grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL(mg::purify_fwd<64>, grid, dim3(256), 0, s, a);
    } else {
        if (backward) hipLaunchKernelGGL(mg::purify_bwd<128>, grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL(mg::purify_fwd<128>, grid, dim3(256), 0, s, a);
    }
    return last_rc();
}

// backward scratch: the d w2 partial rows, then (rows form) the [3][n][d] per-occurrence rows
// and the [2][n_table] first-occurrence / count words
size_t rsx_mgcn_fuse_ws_bytes(int64_t n, int64_t n_table, int32_t d, int32_t rows_form) {
    if (n <= 0 || n_table < 0 || d <= 0) return 0;
    const size_t nblk = (size_t)(((n + 15) / 16 + 3) / 4);
    return (nblk * (size_t)d + (rows_form ? (size_t)3 * (size_t)n * (size_t)d + 2 * (size_t)n_table : 0)) * 4;
}

int rsx_mgcn_fuse(int32_t backward, const float* const* W, const float* const* b, const float* content,
                  const float* image_emb, const float* text_emb, const int64_t* rows, int64_t n, int64_t n_table,
                  int32_t d, float* all_out, float* side_out, float* content_out, float* text_out,
                  const float* g_all, const float* g_side, const float* g_content_in, float* g_content,
                  float* g_image, float* g_text, float* const* dz, float* dif_out, float* dw2, void* ws,
                  size_t ws_bytes, rsx_stream_t stream) {
    if (n < 0 || n_table < 0 || !W || !b || !content || !image_emb || !text_emb) return RSX_ERR_ARG;
    if (!rows && n > n_table) return RSX_ERR_ARG;
    if (d != 64 && d != 128) return RSX_ERR_UNSUPPORTED;
    mg::FuseArgs a{};
    for (int i = 0; i < mg::kNW; ++i) {
        if (!W[i] || (i != mg::kW2 && !b[i])) return RSX_ERR_ARG;
        a.W[i] = W[i];
        a.b[i] = i == mg::kW2 ? nullptr : b[i];
    }
    if (backward) {
        if (!g_all || !g_content || !g_image || !g_text || !dz || !dif_out || !dw2) return RSX_ERR_ARG;
        for (int i = 0; i < mg::kNDz; ++i) {
            if (!dz[i]) return RSX_ERR_ARG;
            a.dz[i] = dz[i];
        }
    } else if (!all_out || !side_out) {
        return RSX_ERR_ARG;
    }
    hipStream_t s = as_stream(stream);
    const size_t tab = (size_t)n_table * (size_t)d * 4;
    if (backward && rows) {  // the table rows no occurrence names
        if (hipMemsetAsync(g_content, 0, tab, s) != hipSuccess || hipMemsetAsync(g_image, 0, tab, s) != hipSuccess ||
            hipMemsetAsync(g_text, 0, tab, s) != hipSuccess)
            return last_rc();
    }
    if (n == 0) {
        if (backward && hipMemsetAsync(dw2, 0, (size_t)d * 4, s) != hipSuccess) return last_rc();
        return RSX_OK;
    }
    const int64_t nblk = ((n + 15) / 16 + 3) / 4;
    if (n > 0x7fffffffll) return RSX_ERR_UNSUPPORTED;  // (occurrence indices are listed as int32)
    a.C = content;
    a.I = image_emb;
    a.T = text_emb;
    a.rows = rows;
    a.n = n;
    const dim3 grid((unsigned)nblk);
    if (!backward) {
        a.all = all_out;
        a.side = side_out;
        a.c_out = content_out;
        a.t_out = text_out;
        if (d == 64) hipLaunchKernelGGL(mg::fuse_fwd<64>, grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL(mg::fuse_fwd<128>, grid, dim3(256), 0, s, a);
        return last_rc();
    }
    if (!ws || ws_bytes < rsx_mgcn_fuse_ws_bytes(n, n_table, d, rows != nullptr)) return RSX_ERR_WORKSPACE;
    a.part = static_cast<float*>(ws);
    float* occ = a.part + nblk * d;
    int32_t* lead = reinterpret_cast<int32_t*>(occ + 3 * n * d);
    if (rows) {
        if (hipMemsetAsync(lead, 0, (size_t)2 * (size_t)n_table * 4, s) != hipSuccess) return last_rc();
        a.lead = lead;
        a.n_table = n_table;
    }
    a.g_all = g_all;
    a.g_side = g_side;
    a.g_cin = g_content_in;
    a.dif = dif_out;
    a.gC = rows ? occ : g_content;
    a.gI = rows ? occ + n * d : g_image;
    a.gT = rows ? occ + 2 * n * d : g_text;
    if (d == 64) {
        hipLaunchKernelGGL(mg::fuse_bwd<64>, grid, dim3(256), 0, s, a);
        hipLaunchKernelGGL(mg::fuse_dw2<64>, dim3(1), dim3(256), 0, s, a.part, nblk, dw2);
        if (rows)
            hipLaunchKernelGGL(mg::fuse_segsum<64>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, rows, n, lead,
                               n_table, occ, g_content, g_image, g_text);
    } else {
        hipLaunchKernelGGL(mg::fuse_bwd<128>, grid, dim3(256), 0, s, a);
        hipLaunchKernelGGL(mg::fuse_dw2<128>, dim3(1), dim3(256), 0, s, a.part, nblk, dw2);
        if (rows)
            hipLaunchKernelGGL(mg::fuse_segsum<128>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, rows, n, lead,
                               n_table, occ, g_content, g_image, g_text);
    }
    return last_rc();
}

}  // extern "C"
