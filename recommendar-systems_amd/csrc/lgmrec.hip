// lgmrec.hip — LGMRec on gfx950: the table-wide InfoNCE, the hyperedge assignments, the
// tall-skinny hypergraph products and the training loss.
//
// Replaces (reference paths relative to its root):
//   src/models/lgmrec.py:159-166   ssl_triple_loss: B normalised batch rows against every row of a
//                                  normalised table, with its autograd backward (a B x N matrix,
//                                  forward and backward, in the reference; never formed here)
//   src/models/lgmrec.py:118-126,139-140  F.gumbel_softmax on the hyperedge logits and the dropout
//   src/models/lgmrec.py:202-214   HGNNLayer: P^T X, P lat with P [n, H], H <= 64
//   src/models/lgmrec.py:175-194   BPR mean + Frobenius regulariser on the combined batch rows
//
// Everything is float32 and deterministic: no float atomics; sums over a split are written as
// partials and added in index order, sums over repeated batch rows go through rsx_triplet.hpp's
// first-occurrence walk.
//
// The InfoNCE.  The table is normalised once (M, ws), the batch rows gathered and normalised
// (n1, ws).  The B x N scores are tiled over the grid: a wave owns 16 "own" rows as a Fld (the
// accumulator layout of v_mfma_f32_16x16x4f32, smore_fld.hpp) and streams 16-row tiles of the
// "other" side: tile_dot gives the 16 x 16 scores, exp((s - 1) / tau - shift) the weights, and
// a second MFMA adds weight x other-row into the own rows' accumulators.  Forward: own = batch
// rows, other = a chunk of the table, only the row sums are kept (parts added in order, the
// shift 1 / tau goes back in the log domain).  Backward: the same tiles twice, own = batch rows
// over table chunks (d n1, parts added in order) and own = table rows over the whole batch
// (d m, no split), each sent through the normalisation's Jacobian.
#include <algorithm>

#include "rsx_triplet.hpp"
#include "smore_fld.hpp"

namespace rsx {
namespace lgm {

using sf::Fld;
using sf::floatx4;

constexpr float kNormEps = 1e-12f;  // F.normalize's eps
constexpr int64_t kSslChunk = 1024;  // table rows a forward / d n1 block streams, at least

// x / max(|x|, eps) of a row held by a lane group of L lanes; nrm: |x|
template <int L>
__device__ __forceinline__ float4 unit4(float4 x, float& nrm) {
    nrm = sqrtf(group_sum<L>(dot4(x, x)));
    return mul4(1.f / fmaxf(nrm, kNormEps), x);
}
// the Jacobian of x -> x / max(|x|, eps) applied to v, n the normalised row: (v - n <n, v>) / |x|
// above the clamp, v / eps below it (torch's clamp_min passes no gradient to the norm there)
template <int L>
__device__ __forceinline__ float4 unit_jac(float4 n, float nrm, float4 v) {
    const float dot = nrm >= kNormEps ? group_sum<L>(dot4(n, v)) : 0.f;
    return mul4(1.f / fmaxf(nrm, kNormEps), fma4(-dot, n, v));
}

// ------------------------------------------------------------------ a. InfoNCE
struct SslWs {
    float *M, *nrm2, *n1, *nrm1, *lt, *pos, *rowpart, *dpart, *occ, *part;
    int32_t* key;
    size_t total;
};
inline int64_t ssl_parts(int64_t N, int64_t B) {
    const int64_t cap = std::max<int64_t>(1, 131072 / ((B + 63) / 64 * 64));
    return std::max<int64_t>(1, std::min<int64_t>((N + kSslChunk - 1) / kSslChunk, cap));
}
inline int64_t ssl_chunk(int64_t N, int64_t B) {
    const int64_t ns = ssl_parts(N, B);
    return ((N + ns - 1) / ns + 15) / 16 * 16;
}
inline SslWs carve_ssl(void* ws, int64_t N, int64_t B, int d) {
    SslWs w;
    Carver cv(ws);
    const int64_t ns = ssl_parts(N, B);
    const int rpb = 256 / (d / 4);
    w.M = cv.take<float>((size_t)N * d * sizeof(float));
    w.nrm2 = cv.take<float>((size_t)N * sizeof(float));
    w.n1 = cv.take<float>((size_t)B * d * sizeof(float));
    w.nrm1 = cv.take<float>((size_t)B * sizeof(float));
    w.lt = cv.take<float>((size_t)B * sizeof(float));
    w.pos = cv.take<float>((size_t)B * sizeof(float));
    w.rowpart = cv.take<float>((size_t)ns * B * sizeof(float));
    w.dpart = cv.take<float>((size_t)ns * B * d * sizeof(float));
    w.occ = cv.take<float>((size_t)B * d * sizeof(float));
    w.part = cv.take<float>((size_t)((B + rpb - 1) / rpb) * sizeof(float));
    w.key = cv.take<int32_t>((size_t)B * sizeof(int32_t));
    w.total = cv.total();
    return w;
}

// M[j] = normalize(T[j]), nrm[j] = |T[j]|; with idx: row b is T[idx[b]] (zeros, key -1 and
// lt = +inf, which zeroes every weight of the row, for an index outside the table)
template <int D>
__global__ __launch_bounds__(256) void ssl_unit(const float* __restrict__ T, int64_t N, const int64_t* __restrict__ idx,
                                                int64_t rows, float* __restrict__ M, float* __restrict__ nrm,
                                                int32_t* __restrict__ key, float* __restrict__ lt) {
    const RowGeom<D> r;
    if (r.b >= rows) return;  // uniform over a row's lane group
    int64_t src = r.b;
    if (idx) {
        src = idx[r.b];
        const bool ok = src >= 0 && src < N;
        if (r.c == 0) key[r.b] = ok ? (int32_t)src : -1, lt[r.b] = ok ? 0.f : INFINITY;
        if (!ok) {
            st4(M + r.b * D + r.c, f4(0.f));
            if (r.c == 0) nrm[r.b] = 0.f;
            return;
        }
    }
    float n;
    st4(M + r.b * D + r.c, unit4<D / 4>(ld4(T + src * D + r.c), n));
    if (r.c == 0) nrm[r.b] = n;
}

// MODE 0: out[part][own] = sum over the part's other rows of exp((s - 1) / tau); pos[own] = the score
//         against other row key[own], the very number that went into the sum (the loss takes
//         the difference of the two: a separately rounded dot would leave 1e-7 / tau in each term)
// MODE 1: out[part][own][:] = sum of exp((s - 1) / tau - lt[own]) other[:]
// MODE 2: out[own][:] = Jacobian of own's normalisation on scale sum of exp((s - 1) / tau - lt[other]) other[:]
// MODE 1 / 2 with key (T1 == T2): the pairs of a batch row with its own table row are left out.  There
// n1_b is m_idx_b bit for bit, the normalisation's Jacobian maps it to zero, and P_bb n1_b - n1_b is the
// largest term of either sum: kept, it would cancel only up to rounding.
template <int D, int MODE>
__global__ __launch_bounds__(256) void ssl_tiles(const float* __restrict__ Own, int64_t n_own,
                                                 const float* __restrict__ Oth, int64_t n_oth, int64_t chunk,
                                                 const float* __restrict__ lt, float inv_tau,
                                                 const float* __restrict__ go, const float* __restrict__ own_nrm,
                                                 const int32_t* __restrict__ key, float* __restrict__ pos,
                                                 float* __restrict__ out) {
    constexpr int T = D / 16;
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int64_t own0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
    if (own0 >= n_own) return;  // wave-uniform
    const int64_t orow = own0 + c < n_own ? own0 + c : -1;
    const Fld<D> X = sf::fload<D>(Own, orow, g);
    const int64_t q_begin = (int64_t)blockIdx.y * chunk;
    const int64_t q_end = q_begin + chunk < n_oth ? q_begin + chunk : n_oth;
    const float lt_own = (MODE == 1 && orow >= 0) ? lt[orow] : 0.f;
    // (a row below the clamp is not annihilated: its pairs stay)
    const bool unit = MODE != 0 && orow >= 0 && own_nrm[orow] >= kNormEps;
    const int64_t k_own = (MODE != 2 && key && orow >= 0 && (MODE == 0 || unit)) ? key[orow] : -1;
    Fld<D> acc = sf::fzero<D>();
    float e = 0.f;
    for (int64_t q0 = q_begin; q0 < q_end; q0 += 16) {
        const Fld<D> Y = sf::fload<D>(Oth, q0 + c < q_end ? q0 + c : -1, g);
        const floatx4 s = sf::tile_dot<D>(Y, X);  // s[r] = <other q0 + 4 g + r, own c>
        float p[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t q = q0 + 4 * g + r;
            const bool valid = q < q_end;
            float sh = lt_own;
            if (MODE == 2) sh = valid ? lt[q] : 0.f;
            p[r] = valid ? expf((s[r] - 1.f) * inv_tau - sh) : 0.f;
            if (MODE == 0 && valid && q == k_own) pos[orow] = s[r];
            // one table: the pair (b, idx_b) is a row against itself, which its own Jacobian annihilates
            if (MODE == 1 && q == k_own) p[r] = 0.f;
            if (MODE == 2 && key && unit && valid && key[q] == orow) p[r] = 0.f;
        }
        if (MODE == 0) {
            e += (p[0] + p[1]) + (p[2] + p[3]);
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t q = q0 + 4 * g + r;
                const float* row = Oth + q * D + c;
#pragma unroll
                for (int t = 0; t < T; ++t) acc.f[t] = sf::mfma4(q < q_end ? row[16 * t] : 0.f, p[r], acc.f[t]);
            }
        }
    }
    if (MODE == 0) {
        e += __shfl_xor(e, 16, kWave);
        e += __shfl_xor(e, 32, kWave);
        if (g == 0 && orow >= 0) out[(int64_t)blockIdx.y * n_own + orow] = e;
    } else if (MODE == 1) {
        sf::fstore<D>(out + (int64_t)blockIdx.y * n_own * D, orow, g, acc);
    } else {
        const float sc = *go * inv_tau;
        const float nrm = orow >= 0 ? own_nrm[orow] : 1.f;
        const Fld<D> v = sf::fmap<D>(acc, [&](float a) { return sc * a; });
        const float dot = nrm >= kNormEps ? sf::rsum<D>(sf::fmap2<D>(X, v, [](float a, float b) { return a * b; })) : 0.f;
        const float inv = 1.f / fmaxf(nrm, kNormEps);
        sf::fstore<D>(out, orow, g, sf::fmap2<D>(X, v, [&](float m, float a) { return inv * (a - dot * m); }));
    }
}

// Per batch row: lt[b] = log of the parts' sum (in order), the row's loss term
// lt + (1 - pos[b]) / tau, block partials in row order
template <int D>
__global__ __launch_bounds__(256) void ssl_rows_fwd(const float* __restrict__ pos, const int32_t* __restrict__ key,
                                                    const float* __restrict__ rowpart,
                                                    int64_t ns, int64_t B, float inv_tau, float* __restrict__ lt,
                                                    float* __restrict__ part) {
    const RowGeom<D> r;
    float v[1] = {0.f};
    if (r.b < B) {
        const int32_t k = key[r.b];
        if (k >= 0) {
            float ttl = 0.f;
            for (int64_t p = 0; p < ns; ++p) ttl += rowpart[p * B + r.b];
            const float l = logf(ttl);
            v[0] = l + (1.f - pos[r.b]) * inv_tau;
            if (r.c == 0) lt[r.b] = l;
        }
    }
    block_partials<D, 1, 1>(r, v, part);
}

__global__ __launch_bounds__(64) void ssl_finish(const float* __restrict__ part, int nblk, float* __restrict__ out) {
    float term[1];
    sum_partials<1, 1>(part, nblk, term);
    if (threadIdx.x == 0) out[0] = term[0];
}

// occ[b] = Jacobian of n1_b's normalisation on go / tau (sum of the parts - m_idx)
template <int D>
__global__ __launch_bounds__(256) void ssl_rows_bwd(const float* __restrict__ n1, const float* __restrict__ nrm1,
                                                    const float* __restrict__ M, const int32_t* __restrict__ key,
                                                    const float* __restrict__ dpart, int64_t ns, int64_t B,
                                                    float inv_tau, const float* __restrict__ go, bool same,
                                                    float* __restrict__ occ) {
    const RowGeom<D> r;
    if (r.b >= B) return;
    const int32_t k = key[r.b];
    float4 out = f4(0.f);
    if (k >= 0) {
        float4 acc = f4(0.f);
        for (int64_t p = 0; p < ns; ++p) acc = add4(acc, ld4(dpart + (p * B + r.b) * D + r.c));
        const bool drop = same && nrm1[r.b] >= kNormEps;  // left out of dpart too
        const float4 dn = mul4(*go * inv_tau, drop ? acc : sub4(acc, ld4(M + (int64_t)k * D + r.c)));
        out = unit_jac<D / 4>(ld4(n1 + r.b * D + r.c), nrm1[r.b], dn);
    }
    st4(occ + r.b * D + r.c, out);
}

// The sums over a table row's occurrences in idx (the walk): gT1[key] += sum occ,
// gT2[key] += Jacobian of m_key's normalisation on -go / tau sum n1.  One wave an occurrence.
template <int D>
__global__ __launch_bounds__(256) void ssl_walk(const float* __restrict__ n1, const float* __restrict__ occ,
                                                const float* __restrict__ M, const float* __restrict__ nrm2,
                                                const int32_t* __restrict__ keys, int64_t B, float inv_tau,
                                                const float* __restrict__ go, float* gT1, float* gT2) {
    constexpr int L = D / 4;
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= B) return;  // wave-uniform, as every branch on j and key below
    const int32_t key = keys[j];
    if (key < 0 || !leads(keys, j, key, lane)) return;
    const int g = lane / L, c = (lane % L) * 4;
    float4 a1 = f4(0.f), a2 = f4(0.f);
    for_each_match<D>(keys, j, B, key, lane, [&](int64_t mine) {
        a1 = add4(a1, ld4(occ + mine * D + c));
        a2 = add4(a2, ld4(n1 + mine * D + c));
    });
    tree_rows<L>(a1);
    tree_rows<L>(a2);
    const float4 j2 = unit_jac<L>(ld4(M + (int64_t)key * D + c), nrm2[key], mul4(-*go * inv_tau, a2));
    if (g != 0) return;
    float* p1 = gT1 + (int64_t)key * D + c;
    st4(p1, add4(ld4(p1), a1));
    if (gT1 == gT2 && nrm2[key] >= kNormEps) return;  // one table: sum n1 is count m_key, annihilated
    float* p2 = gT2 + (int64_t)key * D + c;  // the same row when the tables are one: after p1's store
    st4(p2, add4(ld4(p2), j2));
}

inline int ssl_check(const rsx_lgm_ssl_args* a, void* ws, size_t ws_bytes) {
    if (!a || a->n < 1 || a->batch < 1) return RSX_ERR_ARG;
    if ((a->d != 64 && a->d != 128) || a->batch > kMaxBatch || a->n > 0x7fffffffll) return RSX_ERR_UNSUPPORTED;
    if (!a->T1 || !a->T2 || !a->idx || !ws || !(a->tau > 0.f) || !aligned16(a->T1) || !aligned16(a->T2) ||
        !aligned16(ws))
        return RSX_ERR_ARG;
    if (ws_bytes < rsx_lgm_ssl_ws_bytes(a->n, a->batch, a->d)) return RSX_ERR_WORKSPACE;
    return RSX_OK;
}

template <int D>
int ssl_fwd(const rsx_lgm_ssl_args* a, float* out, void* ws, hipStream_t s) {
    constexpr int RPB = RowGeom<D>::RPB;
    const int64_t N = a->n, B = a->batch, ns = ssl_parts(N, B), chunk = ssl_chunk(N, B);
    const SslWs w = carve_ssl(ws, N, B, D);
    const float it = 1.f / a->tau;
    const int nblk = (int)((B + RPB - 1) / RPB);
    hipLaunchKernelGGL(ssl_unit<D>, dim3((unsigned)((N + RPB - 1) / RPB)), dim3(256), 0, s, a->T2, N,
                       (const int64_t*)nullptr, N, w.M, w.nrm2, (int32_t*)nullptr, (float*)nullptr);
    hipLaunchKernelGGL(ssl_unit<D>, dim3(nblk), dim3(256), 0, s, a->T1, N, a->idx, B, w.n1, w.nrm1, w.key, w.lt);
    hipLaunchKernelGGL((ssl_tiles<D, 0>), dim3((unsigned)((B + 63) / 64), (unsigned)ns), dim3(256), 0, s,
                       (const float*)w.n1, B, (const float*)w.M, N, chunk, (const float*)w.lt, it,
                       (const float*)nullptr, (const float*)nullptr, (const int32_t*)w.key, w.pos, w.rowpart);
    hipLaunchKernelGGL(ssl_rows_fwd<D>, dim3(nblk), dim3(256), 0, s, (const float*)w.pos, (const int32_t*)w.key,
                       (const float*)w.rowpart, ns, B, it, w.lt, w.part);
    hipLaunchKernelGGL(ssl_finish, dim3(1), dim3(64), 0, s, (const float*)w.part, nblk, out);
    return last_rc();
}

template <int D>
int ssl_bwd(const rsx_lgm_ssl_args* a, const float* go, float* gT1, float* gT2, void* ws, hipStream_t s) {
    constexpr int RPB = RowGeom<D>::RPB;
    const int64_t N = a->n, B = a->batch, ns = ssl_parts(N, B), chunk = ssl_chunk(N, B);
    const SslWs w = carve_ssl(ws, N, B, D);
    const float it = 1.f / a->tau;
    const int nblk = (int)((B + RPB - 1) / RPB);
    const bool same = a->T1 == a->T2;
    hipLaunchKernelGGL((ssl_tiles<D, 1>), dim3((unsigned)((B + 63) / 64), (unsigned)ns), dim3(256), 0, s,
                       (const float*)w.n1, B, (const float*)w.M, N, chunk, (const float*)w.lt, it,
                       (const float*)nullptr, (const float*)w.nrm1, same ? (const int32_t*)w.key : nullptr, (float*)nullptr,
                       w.dpart);
    hipLaunchKernelGGL(ssl_rows_bwd<D>, dim3(nblk), dim3(256), 0, s, (const float*)w.n1, (const float*)w.nrm1,
                       (const float*)w.M, (const int32_t*)w.key, (const float*)w.dpart, ns, B, it, go, same, w.occ);
    // every row of gT2: the table side of the tiles, over the whole batch
    hipLaunchKernelGGL((ssl_tiles<D, 2>), dim3((unsigned)((N + 63) / 64), 1), dim3(256), 0, s, (const float*)w.M, N,
                       (const float*)w.n1, B, (B + 15) / 16 * 16, (const float*)w.lt, it, go, (const float*)w.nrm2,
                       same ? (const int32_t*)w.key : nullptr, (float*)nullptr, gT2);
    const int rc = gT1 != gT2 ? zero_tables({{gT1, (size_t)N * D}}, s) : RSX_OK;
    if (rc) return rc;
    hipLaunchKernelGGL(ssl_walk<D>, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, (const float*)w.n1,
                       (const float*)w.occ, (const float*)w.M, (const float*)w.nrm2, (const int32_t*)w.key, B, it, go,
                       gT1, gT2);
    return last_rc();
}

// ------------------------------------------------------------------ b. assignments
struct Assign {
    const float *x, *noise;
    const uint32_t* keep;
    const int64_t* seed;
    int64_t n;
    int H, ld, stream;
    float tau, inv_tau, keep_rate;
};
__device__ __forceinline__ uint32_t draw(uint64_t seed, int stream, int64_t row, int col) {
    return sf::mix32(seed * 0x9E3779B97F4A7C15ULL + ((uint64_t)stream << 56) + (uint64_t)row * 64 + (uint64_t)col);
}
// Gumbel noise -log(-log u) of a 32-bit draw: u = (k + 1/2) 2^-23 with k the draw's top 23 bits.
// k + 1/2 needs 24 significant bits, so it is exact in float32 (a 24-bit k would round up to 2^24
// at its largest value, u = 1 and g = +inf): u lies in [2^-24, 1 - 2^-24], g in [-2.82, 16.64].
__host__ __device__ __forceinline__ float gumbel_of_bits(uint32_t bits) {
    const float u = ((float)(bits >> 9) + 0.5f) * (1.f / 8388608.f);
    return -logf(-logf(u));
}
__device__ __forceinline__ float gumbel(const Assign& a, uint64_t seed, int64_t row, int h) {
    if (a.noise) return a.noise[row * a.H + h];
    return gumbel_of_bits(draw(seed, 2 * a.stream, row, h));
}
// keep / keep_rate of element (row, h)
__device__ __forceinline__ float keep_scale(const Assign& a, uint64_t seed, int64_t row, int h) {
    if (a.keep) return (a.keep[row * ((a.H + 31) / 32) + h / 32] >> (h % 32)) & 1u ? 1.f / a.keep_rate : 0.f;
    if (a.keep_rate >= 1.f) return 1.f;
    const uint32_t thr = (uint32_t)fminf((1.f - a.keep_rate) * 4294967296.f, 4294967295.f);
    return draw(seed, 2 * a.stream + 1, row, h) >= thr ? 1.f / a.keep_rate : 0.f;
}

// a thread a row: y = softmax((x + g) / tau) over the H columns, out = y keep / keep_rate.  The
// logits are formed and exponentiated in float64 (tau = 0.2 puts them near 50, where a float32
// exp argument loses 1e-6 of the result); the rows are small next to everything else in a step.
// Each element's noise is drawn once and its exponential taken once: the row of `out` holds the
// noise and the row of `y` the exponentials between the passes (y != out).
__global__ __launch_bounds__(256) void assign_fwd(Assign a, float* __restrict__ y, float* __restrict__ out,
                                                  float* __restrict__ noise_out) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= a.n) return;
    const uint64_t seed = a.seed ? (uint64_t)*a.seed : 0;
    const float* x = a.x + row * a.ld;
    float* yr = y + row * a.ld;
    float* outr = out + row * a.ld;
    const double it = 1.0 / (double)a.tau;
    double mx = -INFINITY, sum = 0.0;
    for (int h = 0; h < a.H; ++h) {
        const float gn = gumbel(a, seed, row, h);
        outr[h] = gn;
        if (noise_out) noise_out[row * a.H + h] = gn;
        mx = fmax(mx, ((double)x[h] + (double)gn) * it);
    }
    for (int h = 0; h < a.H; ++h) {
        const float e = (float)exp(((double)x[h] + (double)outr[h]) * it - mx);
        yr[h] = e;
        sum += (double)e;
    }
    for (int h = 0; h < a.H; ++h) {
        const float v = (float)((double)yr[h] / sum);
        yr[h] = v;
        outr[h] = v * keep_scale(a, seed, row, h);
    }
}

// dx = y (dy' - sum_h y_h dy'_h) / tau, dy' = dy keep / keep_rate
__global__ __launch_bounds__(256) void assign_bwd(Assign a, const float* __restrict__ y, const float* __restrict__ dy,
                                                  float* __restrict__ dx) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= a.n) return;
    const uint64_t seed = a.seed ? (uint64_t)*a.seed : 0;
    const float* yr = y + row * a.ld;
    float* dr = dx + row * a.ld;
    float dot = 0.f;
    for (int h = 0; h < a.H; ++h) {
        const float d = dy[row * a.ld + h] * keep_scale(a, seed, row, h);
        dr[h] = d;
        dot = fmaf(yr[h], d, dot);
    }
    for (int h = 0; h < a.H; ++h) dr[h] = yr[h] * (dr[h] - dot) * a.inv_tau;
}

// fwd: the forward draws noise; either pass draws keep bits when keep_rate < 1 and no mask is given
inline int to_assign(const rsx_lgm_assign_args* a, Assign& k, bool fwd) {
    if (!a || a->n < 1 || !a->x) return RSX_ERR_ARG;
    if (a->H < 4 || a->H > 64 || (a->H % 4)) return RSX_ERR_UNSUPPORTED;
    if (a->ld < a->H || !(a->tau > 0.f) || !(a->keep_rate > 0.f) || a->keep_rate > 1.f) return RSX_ERR_ARG;
    if (!a->seed && ((fwd && !a->noise) || (!a->keep && a->keep_rate < 1.f))) return RSX_ERR_ARG;
    k.x = a->x, k.noise = a->noise, k.keep = a->keep, k.seed = a->seed, k.n = a->n, k.H = a->H, k.ld = a->ld;
    k.stream = a->stream_id, k.tau = a->tau, k.inv_tau = 1.f / a->tau, k.keep_rate = a->keep_rate;
    return RSX_OK;
}

// ------------------------------------------------------------------ c. hypergraph products
constexpr int64_t kHgRows = 128;  // rows a reduce part takes, at least
constexpr int64_t kHgMaxParts = 512;
__host__ __device__ inline int64_t hg_rows_per(int64_t n) { return std::max<int64_t>(kHgRows, (n + kHgMaxParts - 1) / kHgMaxParts); }
inline int64_t hg_parts(int64_t n) { return n > 0 ? (n + hg_rows_per(n) - 1) / hg_rows_per(n) : 0; }

// part[blk][h][:] = sum over the part's rows, in row order, of P[r, h] X[r, :]; parts [0, s1) are
// of (P, X), the others of (P2, X2)
template <int D>
__global__ __launch_bounds__(256) void hg_reduce_part(const float* __restrict__ P, const float* __restrict__ X,
                                                      int64_t n, int s1, const float* __restrict__ P2,
                                                      const float* __restrict__ X2, int64_t n2, int ld, int H,
                                                      float* __restrict__ part) {
    constexpr int L = D / 4, NG = 256 / L, K = 64 / NG;
    const int c = (threadIdx.x % L) * 4, hg = threadIdx.x / L;
    const bool second = (int)blockIdx.x >= s1;
    const float* p = second ? P2 : P;
    const float* x = second ? X2 : X;
    const int64_t rows = second ? n2 : n, per = hg_rows_per(rows);
    const int64_t r0 = (int64_t)(second ? blockIdx.x - s1 : blockIdx.x) * per, r1 = r0 + per < rows ? r0 + per : rows;
    float4 acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = f4(0.f);
    for (int64_t r = r0; r < r1; ++r) {
        const float4 xv = ld4(x + r * D + c);
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (hg + k * NG < H) acc[k] = fma4(p[r * ld + hg + k * NG], xv, acc[k]);
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (hg + k * NG < H) st4(part + ((int64_t)blockIdx.x * H + hg + k * NG) * D + c, acc[k]);
}
// lat = the parts added in index order; a thread a float4
__global__ __launch_bounds__(256) void hg_reduce_sum(const float* __restrict__ part, int parts, int words,
                                                     float* __restrict__ lat) {
    const int i = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= words) return;
    float4 acc = f4(0.f);
    for (int s = 0; s < parts; ++s) acc = add4(acc, ld4(part + (int64_t)s * words + i));
    st4(lat + i, acc);
}

template <int D>
__device__ __forceinline__ void stage_lat(float* sh, const float* __restrict__ lat, int H) {
    for (int i = threadIdx.x * 4; i < H * D; i += 1024) st4(sh + i, ld4(lat + i));
    __syncthreads();
}
// Y[r, :] = sum_h P[r, h] lat[h, :], lat in LDS; a lane group a row
template <int D>
__global__ __launch_bounds__(256) void hg_expand(const float* __restrict__ P, int ld, int H,
                                                 const float* __restrict__ lat, int64_t n, float* __restrict__ Y) {
    __shared__ float sh[64 * D];
    stage_lat<D>(sh, lat, H);
    const RowGeom<D> r;
    if (r.b >= n) return;
    float4 acc = f4(0.f);
    for (int h = 0; h < H; ++h) acc = fma4(P[r.b * ld + h], ld4(sh + h * D + r.c), acc);
    st4(Y + r.b * D + r.c, acc);
}
// G[r, h] (+)= <X[r, :], lat[h, :]>
template <int D>
__global__ __launch_bounds__(256) void hg_rowdots(const float* __restrict__ X, const float* __restrict__ lat, int H,
                                                  int64_t n, float* __restrict__ G, int ld, int accumulate) {
    __shared__ float sh[64 * D];
    stage_lat<D>(sh, lat, H);
    const RowGeom<D> r;
    if (r.b >= n) return;
    const float4 x = ld4(X + r.b * D + r.c);
    for (int h = 0; h < H; ++h) {
        const float v = group_sum<D / 4>(dot4(x, ld4(sh + h * D + r.c)));
        if (r.c == 0) G[r.b * ld + h] = accumulate ? G[r.b * ld + h] + v : v;
    }
}

inline int hg_check(int32_t H, int32_t ld, int32_t d) {
    if (H < 1 || ld < H) return RSX_ERR_ARG;
    if (H > 64 || (d != 64 && d != 128)) return RSX_ERR_UNSUPPORTED;
    return RSX_OK;
}

// ------------------------------------------------------------------ d. the loss
// rsx_triplet.hpp's protocol (one-score triplet, block partials, keys, walk, workspace, checks)
// on the rows of `all`; its own: AllRow, the Frobenius terms and the walk's five Jacobians.
constexpr int kPartStride = 4, kCoef = 1;

struct Loss {
    const float *C, *Mv, *Mt, *Gv, *Gt;
    const int64_t* trip;
    int64_t nu, ni, B;
    float alpha, reg;
};
// row r of all = C + normalize(Mv) + normalize(Mt) + alpha normalize(Gv + Gt), with its pieces
template <int D>
struct AllRow {
    float4 all, nv, nt, ng;
    float rv, rt, rg;  // the three norms
    __device__ __forceinline__ void load(const Loss& a, int64_t r, int c) {
        constexpr int L = D / 4;
        nv = unit4<L>(ld4(a.Mv + r * D + c), rv);
        nt = unit4<L>(ld4(a.Mt + r * D + c), rt);
        ng = unit4<L>(add4(ld4(a.Gv + r * D + c), ld4(a.Gt + r * D + c)), rg);
        all = fma4(a.alpha, ng, add4(add4(ld4(a.C + r * D + c), nv), nt));
    }
};

template <int D>
__device__ __forceinline__ void load_trip(const Loss& a, int64_t b, int c, ScoreTrip& t) {
    const auto row = [&](int64_t r, int c) {
        AllRow<D> w;
        w.load(a, r, c);
        return w.all;
    };
    load_score_trip<D>(a.trip, a.B, b, a.nu, a.ni, c, row, [&](int64_t i, int c) { return row(a.nu + i, c); }, t);
}

// part[block] = {sum softplus(-x), sum |u|^2, sum |p|^2, sum |n|^2} over the block's triplets
template <int D>
__global__ __launch_bounds__(256) void loss_rows(Loss a, float* __restrict__ part) {
    constexpr int L = RowGeom<D>::L;
    const RowGeom<D> r;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (r.b < a.B) {
        ScoreTrip t;
        load_trip<D>(a, r.b, r.c, t);
        v[0] = softplus_neg(t.x);
        v[1] = group_sum<L>(dot4(t.ur, t.ur));
        v[2] = group_sum<L>(dot4(t.pr, t.pr));
        v[3] = group_sum<L>(dot4(t.nr, t.nr));
    }
    block_partials<D, 4, kPartStride>(r, v, part);
}
// out = {total, bpr, reg}; nrm [3]: the Frobenius norms of the batch matrices, for the backward
__global__ __launch_bounds__(64) void loss_finish(const float* __restrict__ part, int nblk, int64_t B, float reg,
                                                  float* __restrict__ out, float* __restrict__ nrm) {
    float term[4];
    sum_partials<4, kPartStride>(part, nblk, term);
    if (threadIdx.x == 0) {
        const float fu = sqrtf(term[1]), fp = sqrtf(term[2]), fn = sqrtf(term[3]);
        const float bpr = term[0] / (float)B, rg = reg * ((fu + fp + fn) / (float)B);
        out[0] = bpr + rg, out[1] = bpr, out[2] = rg;
        nrm[0] = fu, nrm[1] = fp, nrm[2] = fn;
    }
}

// d total / d |X|_F for the three batch matrices as row scales: go reg / (B |X|_F), 0 at |X|_F = 0
__device__ __forceinline__ float fro_scale(const float* go, float reg, int64_t B, float f) {
    return f > 0.f ? *go * reg / ((float)B * f) : 0.f;
}

// Per triplet b: coef[b] = d total / d x, allU[b] = its user row of all, occU[b] = the row's
// gradient coef (p - n) + s_u u, and the keys
template <int D>
__global__ __launch_bounds__(256) void loss_grad_rows(Loss a, const float* __restrict__ go,
                                                      const float* __restrict__ nrm, float* __restrict__ occU,
                                                      float* __restrict__ allU, float* __restrict__ coef,
                                                      int32_t* __restrict__ ku, int32_t* __restrict__ ki) {
    const RowGeom<D> r;
    if (r.b >= a.B) return;
    ScoreTrip t;
    load_trip<D>(a, r.b, r.c, t);
    const float ck = bpr_coef(t, go, a.B), s = t.ok ? fro_scale(go, a.reg, a.B, nrm[0]) : 0.f;
    st4(occU + r.b * D + r.c, fma4(s, t.ur, mul4(ck, sub4(t.pr, t.nr))));
    st4(allU + r.b * D + r.c, t.ur);
    if (r.c == 0) {
        coef[r.b] = ck;
        store_keys(t, a.B, r.b, ku, ki);
    }
}

// The per-destination sums (the walk), sent to the five tables: g to C, through the three
// normalisations' Jacobians to Mv, Mt and (alpha, both) Gv, Gt
template <int D>
__global__ __launch_bounds__(256) void loss_sum_rows(Loss a, const float* __restrict__ go,
                                                     const float* __restrict__ nrm, const float* __restrict__ occU,
                                                     const float* __restrict__ allU, const float* __restrict__ coef,
                                                     const int32_t* __restrict__ ku, const int32_t* __restrict__ ki,
                                                     float* __restrict__ gC, float* __restrict__ gMv,
                                                     float* __restrict__ gMt, float* __restrict__ gGv,
                                                     float* __restrict__ gGt) {
    constexpr int L = Walk<D>::L;
    Walk<D> w;
    if (!w.begin(ku, ki, a.B)) return;
    const int c = w.c;
    const int64_t row = w.user ? w.key : a.nu + w.key;
    AllRow<D> me;
    me.load(a, row, c);
    const float4 spp = mul4(fro_scale(go, a.reg, a.B, nrm[1]), me.all),
                 spn = mul4(fro_scale(go, a.reg, a.B, nrm[2]), me.all);
    float4 acc = f4(0.f);
    w.each([&](int64_t occ) { acc = add4(acc, ld4(occU + occ * D + c)); },
           [&](int64_t b, float sgn) {
               acc = fma4(sgn * coef[b], ld4(allU + b * D + c), acc);
               acc = add4(acc, sgn > 0.f ? spp : spn);
           });
    tree_rows<L>(acc);
    const float4 jv = unit_jac<L>(me.nv, me.rv, acc), jt = unit_jac<L>(me.nt, me.rt, acc);
    const float4 jg = mul4(a.alpha, unit_jac<L>(me.ng, me.rg, acc));
    if (w.g != 0) return;
    st4(gC + row * D + c, acc);
    st4(gMv + row * D + c, jv);
    st4(gMt + row * D + c, jt);
    st4(gGv + row * D + c, jg);
    st4(gGt + row * D + c, jg);
}

// the shared workspace with allU as its extra row buffer (occX), then nrm [3]: the one piece a
// backward reads from its forward
struct LossWs {
    TripletWs t;
    float* nrm;
};
inline LossWs carve_loss(void* ws, int64_t B, int d) {
    LossWs w{carve_triplet(ws, B, d, kPartStride, kCoef, 1), nullptr};
    w.nrm = w.t.cv.take<float>(4 * sizeof(float));
    return w;
}

inline int loss_check(const rsx_lgm_loss_args* a, void* ws, size_t ws_bytes, Loss& k) {
    if (!a) return RSX_ERR_ARG;
    const float* tabs[5] = {a->C, a->Mv, a->Mt, a->Gv, a->Gt};
    bool own_ok = a->triplets && ws && aligned16(ws);
    for (const float* t : tabs) own_ok = own_ok && t && aligned16(t);
    const int rc = check_triplet(a->batch, a->n_users, a->n_items, a->d, own_ok, ws_bytes,
                                 rsx_lgm_loss_ws_bytes(a->batch, a->d));
    if (rc) return rc;
    k.C = a->C, k.Mv = a->Mv, k.Mt = a->Mt, k.Gv = a->Gv, k.Gt = a->Gt, k.trip = a->triplets;
    k.nu = a->n_users, k.ni = a->n_items, k.B = a->batch, k.alpha = a->alpha, k.reg = a->reg;
    return RSX_OK;
}

template <int D>
int loss_fwd(const Loss& k, float* out, void* ws, hipStream_t s) {
    const LossWs w = carve_loss(ws, k.B, D);
    const int nblk = rows_blocks<D>(k.B);
    hipLaunchKernelGGL(loss_rows<D>, dim3(nblk), dim3(256), 0, s, k, w.t.part);
    hipLaunchKernelGGL(loss_finish, dim3(1), dim3(64), 0, s, (const float*)w.t.part, nblk, k.B, k.reg, out, w.nrm);
    return last_rc();
}

template <int D>
int loss_bwd(const Loss& k, const float* go, float* const (&gt)[5], void* ws, hipStream_t s) {
    const LossWs w = carve_loss(ws, k.B, D);
    const size_t n = (size_t)(k.nu + k.ni) * D;
    const int rc = zero_tables({{gt[0], n}, {gt[1], n}, {gt[2], n}, {gt[3], n}, {gt[4], n}}, s);
    if (rc) return rc;
    hipLaunchKernelGGL(loss_grad_rows<D>, dim3(rows_blocks<D>(k.B)), dim3(256), 0, s, k, go, (const float*)w.nrm,
                       w.t.occU, w.t.occX, w.t.coef, w.t.ku, w.t.ki);
    launch_walk(loss_sum_rows<D>, k.B, s, k, go, w.nrm, w.t.occU, w.t.occX, w.t.coef, w.t.ku, w.t.ki, gt[0], gt[1],
                gt[2], gt[3], gt[4]);
    return last_rc();
}

}  // namespace lgm
}  // namespace rsx

using namespace rsx;

extern "C" size_t rsx_lgm_ssl_ws_bytes(int64_t n, int64_t batch, int32_t d) {
    if (n < 1 || n > 0x7fffffffll || batch < 1 || batch > kMaxBatch || (d != 64 && d != 128)) return 0;
    return lgm::carve_ssl(nullptr, n, batch, d).total;
}

extern "C" int rsx_lgm_ssl_fwd(const rsx_lgm_ssl_args* a, float* out, void* ws, size_t ws_bytes, rsx_stream_t stream) {
    const int rc = lgm::ssl_check(a, ws, ws_bytes);
    if (rc) return rc;
    if (!out) return RSX_ERR_ARG;
    hipStream_t s = as_stream(stream);
    return a->d == 64 ? lgm::ssl_fwd<64>(a, out, ws, s) : lgm::ssl_fwd<128>(a, out, ws, s);
}

extern "C" int rsx_lgm_ssl_bwd(const rsx_lgm_ssl_args* a, const float* go, float* gT1, float* gT2, void* ws,
                               size_t ws_bytes, rsx_stream_t stream) {
    const int rc = lgm::ssl_check(a, ws, ws_bytes);
    if (rc) return rc;
    if (!go || !gT1 || !gT2 || !aligned16(gT1) || !aligned16(gT2) || (a->T1 == a->T2) != (gT1 == gT2))
        return RSX_ERR_ARG;
    hipStream_t s = as_stream(stream);
    return a->d == 64 ? lgm::ssl_bwd<64>(a, go, gT1, gT2, ws, s) : lgm::ssl_bwd<128>(a, go, gT1, gT2, ws, s);
}

extern "C" int rsx_lgm_assign_fwd(const rsx_lgm_assign_args* a, float* y, float* out, float* noise_out,
                                  rsx_stream_t stream) {
    lgm::Assign k;
    const int rc = lgm::to_assign(a, k, true);
    if (rc) return rc;
    if (!y || !out || y == out) return RSX_ERR_ARG;
    hipLaunchKernelGGL(lgm::assign_fwd, dim3((unsigned)((k.n + 255) / 256)), dim3(256), 0, as_stream(stream), k, y, out,
                       noise_out);
    return last_rc();
}

extern "C" float rsx_lgm_gumbel_of_bits(uint32_t bits) { return lgm::gumbel_of_bits(bits); }

extern "C" int rsx_lgm_assign_bwd(const rsx_lgm_assign_args* a, const float* y, const float* dy, float* dx,
                                  rsx_stream_t stream) {
    lgm::Assign k;
    const int rc = lgm::to_assign(a, k, false);
    if (rc) return rc;
    if (!y || !dy || !dx) return RSX_ERR_ARG;
    hipLaunchKernelGGL(lgm::assign_bwd, dim3((unsigned)((k.n + 255) / 256)), dim3(256), 0, as_stream(stream), k, y, dy,
                       dx);
    return last_rc();
}

extern "C" size_t rsx_lgm_hgnn_ws_bytes(int64_t n, int64_t n2, int32_t H, int32_t d) {
    if (n < 1 || n2 < 0 || H < 1 || H > 64 || (d != 64 && d != 128)) return 0;
    return al256((size_t)(lgm::hg_parts(n) + lgm::hg_parts(n2)) * H * d * sizeof(float));
}

extern "C" int rsx_lgm_hgnn_reduce(const float* P, const float* X, int64_t n, const float* P2, const float* X2,
                                   int64_t n2, int32_t ld, int32_t H, int32_t d, float* lat, void* ws, size_t ws_bytes,
                                   rsx_stream_t stream) {
    const int rc = lgm::hg_check(H, ld, d);
    if (rc) return rc;
    if (n < 1 || n2 < 0 || !P || !X || !lat || !ws || (n2 > 0 && (!P2 || !X2))) return RSX_ERR_ARG;
    if (!aligned16(X) || !aligned16(X2) || !aligned16(lat) || !aligned16(ws)) return RSX_ERR_ARG;
    if (ws_bytes < rsx_lgm_hgnn_ws_bytes(n, n2, H, d)) return RSX_ERR_WORKSPACE;
    hipStream_t s = as_stream(stream);
    const int s1 = (int)lgm::hg_parts(n), s2 = (int)lgm::hg_parts(n2);
    float* part = static_cast<float*>(ws);
    if (d == 64)
        hipLaunchKernelGGL(lgm::hg_reduce_part<64>, dim3(s1 + s2), dim3(256), 0, s, P, X, n, s1, P2, X2, n2, (int)ld,
                           (int)H, part);
    else
        hipLaunchKernelGGL(lgm::hg_reduce_part<128>, dim3(s1 + s2), dim3(256), 0, s, P, X, n, s1, P2, X2, n2, (int)ld,
                           (int)H, part);
    const int words = H * d;
    hipLaunchKernelGGL(lgm::hg_reduce_sum, dim3((words / 4 + 255) / 256), dim3(256), 0, s, (const float*)part, s1 + s2,
                       words, lat);
    return last_rc();
}

extern "C" int rsx_lgm_hgnn_expand(const float* P, int32_t ld, int32_t H, const float* lat, int64_t n, int32_t d,
                                   float* Y, rsx_stream_t stream) {
    const int rc = lgm::hg_check(H, ld, d);
    if (rc) return rc;
    if (n < 1 || !P || !lat || !Y || !aligned16(lat) || !aligned16(Y)) return RSX_ERR_ARG;
    const int rpb = 256 / (d / 4);
    const dim3 grid((unsigned)((n + rpb - 1) / rpb));
    if (d == 64)
        hipLaunchKernelGGL(lgm::hg_expand<64>, grid, dim3(256), 0, as_stream(stream), P, (int)ld, (int)H, lat, n, Y);
    else
        hipLaunchKernelGGL(lgm::hg_expand<128>, grid, dim3(256), 0, as_stream(stream), P, (int)ld, (int)H, lat, n, Y);
    return last_rc();
}

extern "C" int rsx_lgm_hgnn_rowdots(const float* X, const float* lat, int32_t H, int64_t n, int32_t d, float* G,
                                    int32_t ld, int32_t accumulate, rsx_stream_t stream) {
    const int rc = lgm::hg_check(H, ld, d);
    if (rc) return rc;
    if (n < 1 || !X || !lat || !G || !aligned16(lat) || !aligned16(X)) return RSX_ERR_ARG;
    const int rpb = 256 / (d / 4);
    const dim3 grid((unsigned)((n + rpb - 1) / rpb));
    if (d == 64)
        hipLaunchKernelGGL(lgm::hg_rowdots<64>, grid, dim3(256), 0, as_stream(stream), X, lat, (int)H, n, G, (int)ld,
                           (int)accumulate);
    else
        hipLaunchKernelGGL(lgm::hg_rowdots<128>, grid, dim3(256), 0, as_stream(stream), X, lat, (int)H, n, G, (int)ld,
                           (int)accumulate);
    return last_rc();
}

extern "C" size_t rsx_lgm_loss_ws_bytes(int64_t batch, int32_t d) {
    return triplet_shape_ok(batch, d) ? lgm::carve_loss(nullptr, batch, d).t.cv.total() : 0;
}

extern "C" int rsx_lgm_loss_fwd(const rsx_lgm_loss_args* a, float* out, void* ws, size_t ws_bytes,
                                rsx_stream_t stream) {
    lgm::Loss k;
    const int rc = lgm::loss_check(a, ws, ws_bytes, k);
    if (rc) return rc;
    if (!out) return RSX_ERR_ARG;
    hipStream_t s = as_stream(stream);
    return a->d == 64 ? lgm::loss_fwd<64>(k, out, ws, s) : lgm::loss_fwd<128>(k, out, ws, s);
}

extern "C" int rsx_lgm_loss_bwd(const rsx_lgm_loss_args* a, const float* go, float* gC, float* gMv, float* gMt,
                                float* gGv, float* gGt, void* ws, size_t ws_bytes, rsx_stream_t stream) {
    lgm::Loss k;
    const int rc = lgm::loss_check(a, ws, ws_bytes, k);
    if (rc) return rc;
    float* const gt[5] = {gC, gMv, gMt, gGv, gGt};
    for (float* t : gt)
        if (!t || !aligned16(t)) return RSX_ERR_ARG;
    if (!go) return RSX_ERR_ARG;
    hipStream_t s = as_stream(stream);
    return a->d == 64 ? lgm::loss_bwd<64>(k, go, gt, ws, s) : lgm::loss_bwd<128>(k, go, gt, ws, s);
}
