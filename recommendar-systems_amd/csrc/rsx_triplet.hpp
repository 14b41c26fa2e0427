// rsx_triplet.hpp — what the BPR-style losses on gathered rows share (freedom.hip, lattice.hip):
// the triplet's indices, the lane-group geometry of a d-wide row, the forward's fixed-order
// reductions, and the backward's first-occurrence walk.  Every device piece is inlined into
// the including file's own kernels; nothing here knows which model calls it.
//
// The walk.  The backward sums, per destination row, the contributions of the row's
// occurrences in the batch, without atomics and without a per-table-row list head: the
// inverted index is the batch's key list itself.  One wave an occurrence; the wave of a
// destination's FIRST occurrence (leads: no equal key before it, a ballot scan) walks the keys
// from its own position on, 256 at a time (an int4 of keys a lane); the matches of a chunk,
// in a fixed order, are dealt round-robin to the wave's G lane groups, which add their rows
// (for_each_match); the G partial rows are then added in a fixed tree (tree_rows).  Which
// wave leads, which lane group takes which occurrence and the order in which it adds them
// are functions of the keys alone, so the sums are bit-reproducible and a captured step
// equals the eager one.  The walk costs (keys / 256) chunk loads a wave: quadratic in the
// batch, which is why the batch is capped (kMaxBatch).
#pragma once
#include "rsx_common.hpp"

namespace rsx {

constexpr int64_t kMaxBatch = 65536;

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

// A d-wide row is one lane group of L = d / 4 float4 lanes: a 256-thread block carries RPB
// rows, a wave64 G of them (4 at d = 64, 2 at d = 128).  A thread of a block that owns RPB
// consecutive rows: its row b, that row's place lr in the block, its first column c.
template <int D>
struct RowGeom {
    static constexpr int L = D / 4, RPB = 256 / L, G = kWave / L;
    int lr, c;
    int64_t b;
    __device__ __forceinline__ RowGeom()
        : lr(threadIdx.x / L), c((threadIdx.x % L) * 4), b((int64_t)blockIdx.x * RPB + lr) {}
};

// Triplet b of trip [3, B] = [users; positives; negatives]; ok: every index is inside its table.
struct TripIdx {
    bool ok;
    int64_t u, p, n;
};
__device__ __forceinline__ void load_idx(const int64_t* __restrict__ trip, int64_t B, int64_t b, int64_t nu,
                                         int64_t ni, TripIdx& t) {
    t.u = trip[b], t.p = trip[B + b], t.n = trip[2 * B + b];
    t.ok = t.u >= 0 && t.u < nu && t.p >= 0 && t.p < ni && t.n >= 0 && t.n < ni;
}
// the batch's keys as int32: users ku [B], items ki [2 B] = [positives; negatives]; -1 for a
// triplet with an index outside its table (it contributes nothing)
__device__ __forceinline__ void store_keys(const TripIdx& t, int64_t B, int64_t b, int32_t* __restrict__ ku,
                                           int32_t* __restrict__ ki) {
    ku[b] = t.ok ? (int32_t)t.u : -1;
    ki[b] = t.ok ? (int32_t)t.p : -1;
    ki[B + b] = t.ok ? (int32_t)t.n : -1;
}

// part[block][k] = sum over the block's rows, in row order, of v[k] (the value of the row of
// this thread's lane group; NT terms, STRIDE words a block).  Every thread of the block enters.
template <int D, int NT, int STRIDE>
__device__ __forceinline__ void block_partials(const RowGeom<D>& r, const float (&v)[NT], float* __restrict__ part) {
    constexpr int RPB = RowGeom<D>::RPB;
    __shared__ float sh[RPB][NT];
    if (r.c == 0)
#pragma unroll
        for (int k = 0; k < NT; ++k) sh[r.lr][k] = v[k];
    __syncthreads();
    if (threadIdx.x < NT) {
        float acc = 0.f;
        for (int j = 0; j < RPB; ++j) acc += sh[j][threadIdx.x];
        part[(int64_t)blockIdx.x * STRIDE + threadIdx.x] = acc;
    }
}

// term[k] = the sum of the block partials of term k, by one wave: lane l adds the partials
// l, l + 64, ... in index order, the 64 lane sums are added in a fixed tree
template <int NT, int STRIDE>
__device__ __forceinline__ void sum_partials(const float* __restrict__ part, int nblk, float (&term)[NT]) {
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        float acc = 0.f;
        for (int j = threadIdx.x; j < nblk; j += kWave) acc += part[(int64_t)j * STRIDE + k];
        term[k] = group_sum<kWave>(acc);
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

// Whether occurrence j is the first of `key` (no equal key among keys[0, j)): its wave leads
// the key's sum.  Wave-uniform; the conditions of for_each_match hold here too.
__device__ __forceinline__ bool leads(const int32_t* __restrict__ keys, int64_t j, int32_t key, int lane) {
    unsigned long long m[4];
    for (int64_t base = 0; base < j; base += 4 * kWave) {
        match256(keys, base, lane, 0, j, key, m);
        if (m[0] | m[1] | m[2] | m[3]) return false;
    }
    return true;
}

// Calls f(i) for every index i in [j, n) with keys[i] == key: the matches of a 256-key chunk,
// in index order within each of the four int4 components, are dealt round-robin to the wave's
// G = 64 / (D / 4) lane groups, and lane group g's lanes call f on the group's share, in that
// order.  Conditions:
//   - keys is 256-byte aligned and padded to a multiple of 64 entries (match256's int4 load);
//   - every lane of the wave enters, with the same keys, j, n and key: the loops branch on the
//     ballots alone, so they are wave-uniform, and a lane whose group has no match in a round
//     skips f but stays with the wave (it must still reach the caller's tree_rows);
//   - f contains no cross-lane operation: it runs in the lanes that have a match only.
template <int D, class F>
__device__ __forceinline__ void for_each_match(const int32_t* __restrict__ keys, int64_t j, int64_t n, int32_t key,
                                               int lane, F f) {
    constexpr int L = D / 4, G = kWave / L, kChunk = 4 * kWave;
    const int g = lane / L;
    unsigned long long m[4];
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
                if (mine >= 0) f(mine);
            }
        }
    }
}

// The wave's 64 / L partial rows (lane groups of L lanes) added in a fixed tree: every lane
// group holds the whole sum afterwards.  Every lane of the wave enters.
template <int L>
__device__ __forceinline__ void tree_rows(float4& acc) {
#pragma unroll
    for (int o = kWave / 2; o >= L; o >>= 1) {
        acc.x += __shfl_xor(acc.x, o, kWave);
        acc.y += __shfl_xor(acc.y, o, kWave);
        acc.z += __shfl_xor(acc.z, o, kWave);
        acc.w += __shfl_xor(acc.w, o, kWave);
    }
}

// The workspace of such a loss: the forward's block partials (`stride` words a block of
// 256 / (d / 4) triplets); the backward's per-occurrence user rows [B, d], the coefficients
// [n_coef, B] and the int32 keys (users [B], items [2 B]).  A piece is padded to 256 bytes,
// which is the key lists' padding to 64 entries that match256 relies on.
struct TripletWs {
    float *part, *occU, *coef;
    int32_t *ku, *ki;
    size_t total;
};
inline TripletWs carve_triplet(void* ws, int64_t B, int d, int stride, int n_coef) {
    TripletWs w;
    Carver cv(ws);
    const int rpb = 256 / (d / 4);
    w.part = cv.take<float>((size_t)((B + rpb - 1) / rpb) * stride * sizeof(float));
    w.occU = cv.take<float>((size_t)B * d * sizeof(float));
    w.coef = cv.take<float>((size_t)n_coef * B * sizeof(float));
    w.ku = cv.take<int32_t>((size_t)B * sizeof(int32_t));
    w.ki = cv.take<int32_t>((size_t)2 * B * sizeof(int32_t));
    w.total = cv.total();
    return w;
}
// its size, 0 for a shape the losses do not take
inline size_t triplet_ws_bytes(int64_t batch, int d, int stride, int n_coef) {
    if (batch < 1 || batch > kMaxBatch || (d != 64 && d != 128)) return 0;
    return carve_triplet(nullptr, batch, d, stride, n_coef).total;
}

// The argument checks the losses share, in their precedence.  own_ok: the caller's own
// arguments hold (its pointers present and 16-byte aligned, its scalars in range).
inline int check_triplet(int64_t batch, int64_t nu, int64_t ni, int d, bool own_ok, size_t ws_bytes, size_t ws_need) {
    if (batch < 1 || nu < 1 || ni < 1) return RSX_ERR_ARG;
    if (d != 64 && d != 128) return RSX_ERR_UNSUPPORTED;
    if (!own_ok) return RSX_ERR_ARG;
    // keys are listed as int32; the walk over the keys is quadratic in the batch
    if (batch > kMaxBatch || nu > 0x7fffffffll || ni > 0x7fffffffll) return RSX_ERR_UNSUPPORTED;
    if (ws_bytes < ws_need) return RSX_ERR_WORKSPACE;
    return RSX_OK;
}

}  // namespace rsx
