// rsx_triplet.hpp — the protocol of the BPR-style losses on gathered rows, shared by freedom.hip,
// lattice.hip, lgmrec.hip, mmgcn.hip and grcn.hip.  A model's file holds its own mathematics
// (how a row is fetched, what a triplet contributes, where a summed row goes); everything else
// is here, inlined into the including file's kernels:
//   forward   a lane group a triplet of trip [3, B] (RowGeom, load_idx; ScoreTrip for a loss
//             with one score a triplet), block partials in row order (block_partials), one
//             wave adds them in index order (sum_partials).  Grid: rows_blocks.
//   backward  zero_tables; a rows kernel that stores, per triplet, its coefficients (bpr_coef),
//             its contribution to the user row, and the keys as int32 (store_keys); a walk
//             kernel (Walk, launch_walk) that sums per destination row.
//   workspace carve_triplet, triplet_ws_bytes; the argument checks: check_triplet.
//
// The walk.  The backward sums, per destination row, the contributions of the row's
// occurrences in the batch, without atomics and without a per-table-row list head: the
// inverted index is the batch's key list itself.  One wave an occurrence, 3 B waves: wave
// w < B is user occurrence w, the others item occurrence w - B of [positives; negatives].  The
// wave of a destination's FIRST occurrence (leads: no equal key before it, a ballot scan)
// walks the keys from its own position on, 256 at a time (an int4 of keys a lane); the matches
// of a chunk, in a fixed order, are dealt round-robin to the wave's G lane groups, which add
// their rows (for_each_match); the G partial rows are then added in a fixed tree (tree_rows).
// Which wave leads, which lane group takes which occurrence and the order in which it adds
// them are functions of the keys alone, so the sums are bit-reproducible and a captured step
// equals the eager one.  The walk costs (keys / 256) chunk loads a wave: quadratic in the
// batch, which is why the batch is capped (kMaxBatch).
#pragma once
#include <initializer_list>

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
// rows, a wave64 G of them (4 at d = 64, 2 at d = 128, 1 at d = 256: a wave a row).  A thread of
// a block that owns RPB consecutive rows: its row b, that row's place lr in the block, its
// first column c.
template <int D>
struct RowGeom {
    static constexpr int L = D / 4, RPB = 256 / L, G = kWave / L;
    int lr, c;
    int64_t b;
    __device__ __forceinline__ RowGeom()
        : lr(threadIdx.x / L), c((threadIdx.x % L) * 4), b((int64_t)blockIdx.x * RPB + lr) {}
};
// the blocks of a kernel with one lane group a triplet (the forward's block partials number as many)
template <int D>
inline int rows_blocks(int64_t B) {
    return (int)((B + RowGeom<D>::RPB - 1) / RowGeom<D>::RPB);
}

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

// A triplet with one score, as seen by one lane (its 4 columns): the three rows and
// x = <u, p> - <u, n>.  An index outside its table: ok = false, x NaN, the rows zero.
struct ScoreTrip : TripIdx {
    float4 ur, pr, nr;
    float x;
};
// user_row(u, c) / item_row(i, c): the lane's float4 at column c of user u's / item i's row.
// Every lane of the row's lane group (D / 4 lanes) enters; ok is uniform over it.
template <int D, class FU, class FI>
__device__ __forceinline__ void load_score_trip(const int64_t* __restrict__ trip, int64_t B, int64_t b, int64_t nu,
                                                int64_t ni, int c, FU user_row, FI item_row, ScoreTrip& t) {
    load_idx(trip, B, b, nu, ni, t);
    t.ur = t.pr = t.nr = f4(0.f);
    if (!t.ok) {
        t.x = __builtin_nanf("");
        return;
    }
    t.ur = user_row(t.u, c);
    t.pr = item_row(t.p, c);
    t.nr = item_row(t.n, c);
    t.x = group_sum<D / 4>(dot4(t.ur, t.pr)) - group_sum<D / 4>(dot4(t.ur, t.nr));
}
// d (mean softplus(-x)) / d x of the triplet, times the upstream *go; 0 for a bad triplet
__device__ __forceinline__ float bpr_coef(const ScoreTrip& t, const float* __restrict__ go, int64_t B) {
    return t.ok ? -*go / (float)B * sigmoid_neg(t.x) : 0.f;
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
// [lo, hi): lane l loads keys base + 4 l .. + 3 as one int4, and bit l of m[q] answers for
// index base + 4 l + q.  The load of a lane with 4 l < hi - base may reach 3 entries past hi:
// a key list is 256-byte aligned and padded to a multiple of 64 entries, which a piece of
// carve_triplet is (Carver pads every piece to 256 bytes).  Nothing else states this.
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
// order.  Conditions (Walk::each hands them on to its callbacks):
//   - keys is a key list as match256 needs it;
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

// A wave's place in the walk of a kernel started by launch_walk.  begin: false for a wave with
// nothing to sum (past the 3 B occurrences, a key of -1, or not its key's first occurrence);
// otherwise the wave sums the row `key` of the users' (user) or the items' table, this lane
// being lane (lane % L) of lane group g and holding the columns c .. c + 3.  All of it is
// wave-uniform but lane, g and c.  D = 256: one lane group a wave, no tree_rows needed.
template <int D>
struct Walk {
    static constexpr int L = D / 4;
    const int32_t* __restrict__ keys;
    int64_t B, j;
    int32_t key;
    int lane, g, c;
    bool user;
    __device__ __forceinline__ bool begin(const int32_t* __restrict__ ku, const int32_t* __restrict__ ki,
                                          int64_t batch) {
        lane = threadIdx.x & (kWave - 1);
        const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
        B = batch;
        if (w >= 3 * B) return false;
        user = w < B;
        keys = user ? ku : ki;
        j = user ? w : w - B;
        key = keys[j];
        if (key < 0 || !leads(keys, j, key, lane)) return false;
        g = lane / L, c = (lane % L) * 4;
        return true;
    }
    // The row's occurrences, in for_each_match's order and under its conditions (every lane
    // that passed begin enters; no cross-lane operation inside a callback): on_user(occ) for
    // a user row's occurrence in triplet occ; on_item(b, sgn) for an item row's occurrence in
    // triplet b, sgn +1.f as its positive and -1.f as its negative.
    template <class FU, class FI>
    __device__ __forceinline__ void each(FU on_user, FI on_item) const {
        for_each_match<D>(keys, j, user ? B : 2 * B, key, lane, [&](int64_t mine) {
            if (user) {
                on_user(mine);
            } else {
                const bool pos = mine < B;
                on_item(pos ? mine : mine - B, pos ? 1.f : -1.f);
            }
        });
    }
};
// starts a kernel that opens with Walk::begin: four waves a block, a wave an occurrence
template <class... P, class... A>
inline void launch_walk(void (*kernel)(P...), int64_t B, hipStream_t s, A... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((3 * B + 3) / 4)), dim3(256), 0, s, static_cast<P>(args)...);
}

// Zero-fills gradient tables (a null table is skipped); the first failure's code
struct Table {
    float* p;
    size_t n;  // floats
};
inline int zero_tables(std::initializer_list<Table> tables, hipStream_t s) {
    for (const Table& t : tables) {
        const hipError_t e = t.p ? hipMemsetAsync(t.p, 0, t.n * sizeof(float), s) : hipSuccess;
        if (e != hipSuccess) return hip_rc(e);
    }
    return RSX_OK;
}

// The workspace of such a loss: the forward's block partials (`stride` words a block of
// 256 / (d / 4) triplets, d the width a triplet's lane group spans); the backward's
// per-occurrence rows of `width` floats (d unless given: GRCN's rows are narrower than its
// wave), occU [B, width] and n_extra more of the model's own at occX [n_extra][B, width]; the
// coefficients [n_coef, B] and the int32 keys (users [B], items [2 B]).  A model's further
// pieces are taken from cv afterwards; cv.total() is the size.
struct TripletWs {
    float *part, *occU, *occX, *coef;
    int32_t *ku, *ki;
    Carver cv;
};
inline TripletWs carve_triplet(void* ws, int64_t B, int d, int stride, int n_coef, int n_extra = 0, int width = 0) {
    TripletWs w{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, Carver(ws)};
    const int rpb = 256 / (d / 4);
    const size_t rows = (size_t)B * (width ? width : d) * sizeof(float);
    w.part = w.cv.take<float>((size_t)((B + rpb - 1) / rpb) * stride * sizeof(float));
    w.occU = w.cv.take<float>(rows);
    w.occX = w.cv.take<float>(n_extra * rows);
    w.coef = w.cv.take<float>((size_t)n_coef * B * sizeof(float));
    w.ku = w.cv.take<int32_t>((size_t)B * sizeof(int32_t));
    w.ki = w.cv.take<int32_t>((size_t)2 * B * sizeof(int32_t));
    return w;
}
// the shapes the d-wide losses take
inline bool triplet_shape_ok(int64_t batch, int d) { return batch >= 1 && batch <= kMaxBatch && (d == 64 || d == 128); }
// the workspace's size without further pieces, 0 for a shape the losses do not take
inline size_t triplet_ws_bytes(int64_t batch, int d, int stride, int n_coef, int n_extra = 0) {
    return triplet_shape_ok(batch, d) ? carve_triplet(nullptr, batch, d, stride, n_coef, n_extra).cv.total() : 0;
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
