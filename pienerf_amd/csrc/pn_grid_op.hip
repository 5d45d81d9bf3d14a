// The stand-alone hash-grid encoder op for gfx950, input dimensions D = 2, 3, 4, 5: forward in fp32 (every D) and with a half table (D = 3, the
// `--fp16` / autocast form), dy_dx, backward in fp32 (every D) and half (D = 3), input backward, total-variation gradient.  One template family over
// (D, C); the render path's fused D = 3 encoder is pn_net_tile.h and does not come here.
//
// Reference: gridencoder/src/gridencoder.cu:50-245 (kernel_grid and its dy_dx branch), :248-340 (kernel_grid_backward), :343-369
// (kernel_input_backward), :506-611 (kernel_grad_tv), and the (D, C) dispatch at :376-399, :430-444, :629-634.
//
// Mapping: one lane per (sample, level) with blockIdx.y = level, so that a level's table slice (and its gradient slice) stays in the XCD L2s while
// that level is processed.  Index arithmetic and summation order are the reference kernel's (corner idx ascending, channels inside), and
// `inputs * scale + offset` is rounded once (nvcc's default contraction), so forward and dy_dx equal the reference's contracting build bit for bit.
// Scatter-adds are hardware atomics (global_atomic_add_f32 / global_atomic_pk_add_f16 at L2, no CAS loop); like the reference's atomicAdd their
// order is not fixed, so gradients are compared with the oracle to a tolerance.
#include <math.h>

#include <type_traits>

#include "pn_common.h"
#include "pn_encoders.h"

namespace {

// ------------------------------------------------------------------------------------------------ index
// get_grid_index<D, C> with ch = 0 (gridencoder.cu:65-84); `dense` = 0 -> fast_hash, else the number of strided dims (pn_fill_grid_levels).
struct LevelIdx { uint32_t dense, hs, mask, nomod, stride1; };
__device__ __forceinline__ LevelIdx level_idx(const PnGridLevels& lv, uint32_t level, int align_corners) {
    return LevelIdx{lv.dense[level], lv.hashmap_size[level], lv.mask[level], lv.nomod[level],
                    align_corners ? lv.resolution[level] : lv.resolution[level] + 1};
}
__device__ __forceinline__ uint32_t grid_index3(const LevelIdx& L, uint32_t g0, uint32_t g1, uint32_t g2) {
    if (L.dense == 0) {
        const uint32_t index = g0 ^ (g1 * 2654435761u) ^ (g2 * 805459861u);
        return L.mask ? (index & L.mask) : (index % L.hs);
    }
    const uint32_t index = g0 + (L.dense > 1 ? g1 * L.stride1 : 0u) + (L.dense > 2 ? g2 * L.stride1 * L.stride1 : 0u);
    return L.nomod ? index : (index % L.hs);
}
// D = 3 keeps grid_index3 as its body: the loop below yields the same integers there but not the same code (fewer, differently ordered VALU
// instructions in the forward kernel), and the D = 3 forward kernels are the ones bench.py times.
template <uint32_t D>
__device__ __forceinline__ uint32_t grid_index(const LevelIdx& L, const uint32_t (&p)[D]) {
    if constexpr (D == 3) {
        return grid_index3(L, p[0], p[1], p[2]);
    } else {
        constexpr uint32_t primes[7] = {1u, 2654435761u, 805459861u, 3674653429u, 2097192037u, 1434869437u, 2165219737u};
        uint32_t index = 0;
        if (L.dense == 0) {
#pragma unroll
            for (uint32_t d = 0; d < D; d++) index ^= p[d] * primes[d];
            return L.mask ? (index & L.mask) : (index % L.hs);
        }
        uint32_t stride = 1;
#pragma unroll
        for (uint32_t d = 0; d < D; d++) {
            if (d < L.dense) index += p[d] * stride;
            stride *= L.stride1;
        }
        return L.nomod ? index : (index % L.hs);
    }
}

// ------------------------------------------------------------------------------------------------ cell and corners
template <uint32_t D>
struct Cell { float pos[D], deriv[D]; uint32_t pg[D]; };

// sample b's coordinates (b < B)
template <uint32_t D>
__device__ __forceinline__ void load_point(const float* __restrict__ inputs, uint32_t b, float (&in)[D]) {
#pragma unroll
    for (uint32_t d = 0; d < D; d++) in[d] = inputs[b * D + d];   // B * D < 2^32: grid_levels
}
// for the kernels whose lanes past the end of the batch stay in the wave (LDS rows, the run fold): those get a point out of range, which writes
// nothing and adds nothing
template <uint32_t D>
__device__ __forceinline__ void load_point_or_outside(const float* __restrict__ inputs, uint32_t b, uint32_t B, float (&in)[D]) {
#pragma unroll
    for (uint32_t d = 0; d < D; d++) in[d] = -1.f;
    if (b < B) load_point<D>(inputs, b, in);
}

// gridencoder.cu:113-118: a sample outside [0, 1]^D encodes to zeros and takes no gradient
template <uint32_t D>
__device__ __forceinline__ bool in_range(const float (&in)[D]) {
    bool outside = false;
#pragma unroll
    for (uint32_t d = 0; d < D; d++) outside = outside | (in[d] < 0) | (in[d] > 1);   // no short circuit: the D loads stay independent
    return !outside;
}

// gridencoder.cu:136-157: the cell's integer corner pg, the (smoothstepped) fraction pos and its derivative
template <uint32_t D>
__device__ __forceinline__ Cell<D> locate(const float (&in)[D], float scale, int align_corners, uint32_t interp) {
    Cell<D> c;
#pragma unroll
    for (uint32_t d = 0; d < D; d++) {
        float p = fmaf(in[d], scale, align_corners ? 0.0f : 0.5f);  // explicit single rounding, as in the oracle
        c.pg[d] = (uint32_t)floorf(p);
        p -= (float)c.pg[d];
        if (interp == 1) { c.deriv[d] = 6 * p * (1 - p); p = p * p * (3.0f - 2.0f * p); }
        else c.deriv[d] = 1.0f;
        c.pos[d] = p;
    }
    return c;
}

// f(w, pl) for the 2^D corners of the cell in the reference's order: interpolation weight and integer position
template <uint32_t D, typename F>
__device__ __forceinline__ void for_each_corner(const Cell<D>& c, F&& f) {
#pragma unroll
    for (uint32_t idx = 0; idx < (1u << D); idx++) {
        float w = 1;
        uint32_t pl[D];
#pragma unroll
        for (uint32_t d = 0; d < D; d++) {
            if ((idx & (1u << d)) == 0) { w *= 1 - c.pos[d]; pl[d] = c.pg[d]; }
            else { w *= c.pos[d]; pl[d] = c.pg[d] + 1; }
        }
        f(w, pl);
    }
}

// the dy_dx variant (gridencoder.cu:204-243): f(w, left, right) for the 2^(D-1) edges along dimension gd, w = w0 * the other dims' weights
template <uint32_t D, typename F>
__device__ __forceinline__ void for_each_edge(const Cell<D>& c, uint32_t gd, float w0, F&& f) {
#pragma unroll
    for (uint32_t idx = 0; idx < (1u << (D - 1)); idx++) {
        float w = w0;
        uint32_t pl[D], pr[D];
#pragma unroll
        for (uint32_t nd = 0; nd < D - 1; nd++) {
            const uint32_t d = (nd >= gd) ? (nd + 1) : nd;
            if ((idx & (1u << nd)) == 0) { w *= 1 - c.pos[d]; pl[d] = c.pg[d]; }
            else { w *= c.pos[d]; pl[d] = c.pg[d] + 1; }
            pr[d] = pl[d];
        }
        pl[gd] = c.pg[gd];
        pr[gd] = c.pg[gd] + 1;
        f(w, pl, pr);
    }
}

// ------------------------------------------------------------------------------------------------ forward
// T = float: kernel_grid<float, D, C>.  T = _Float16: kernel_grid<at::Half, 3, C> — the table and the outputs are half, positions and weights
// stay float, and `results[ch] += w * grid[index + ch]` rounds the float product to half and adds half + half (c10::Half operators).
template <uint32_t D, uint32_t C, typename T>
__device__ __forceinline__ void grid_encode_one(const float (&in)[D], const T* __restrict__ emb, const PnGridLevels& lv, uint32_t level, int align_corners,
                                                uint32_t interp, T (&res)[C]) {
#pragma unroll
    for (uint32_t ch = 0; ch < C; ch++) res[ch] = (T)0.0f;
    if (!in_range<D>(in)) return;
    const Cell<D> c = locate<D>(in, lv.scale[level], align_corners, interp);
    const T* __restrict__ table = emb + (size_t)lv.offset[level] * C;
    const LevelIdx LI = level_idx(lv, level, align_corners);
    for_each_corner<D>(c, [&](float w, const uint32_t (&pl)[D]) {
        const uint32_t index = grid_index<D>(LI, pl) * C;
        if constexpr (sizeof(T) == 4 && C == 2) {
            const float2 v = *reinterpret_cast<const float2*>(table + index);
            res[0] += (T)(w * v.x);
            res[1] += (T)(w * v.y);
        } else {
#pragma unroll
            for (uint32_t ch = 0; ch < C; ch++) res[ch] = res[ch] + rounded_product<T>(w, table[index + ch]);
        }
    });
}

// [L,B,C] output (the reference kernel's own layout, gridencoder.cu:105): blockIdx.y = level, a thread per sample — the launch sweeps one level's
// table at a time (it stays in the XCD L2s), neighbouring lanes write neighbouring rows.
template <uint32_t D, uint32_t C, typename T>
__global__ void __launch_bounds__(256) k_grid_encode(const float* __restrict__ inputs, const T* __restrict__ emb, PnGridLevels lv, uint32_t B,
                                                     int align_corners, uint32_t interp, T* __restrict__ outputs) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const uint32_t level = blockIdx.y;
    float in[D];
    load_point<D>(inputs, b, in);
    T res[C];
    grid_encode_one<D, C, T>(in, emb, lv, level, align_corners, interp, res);
    T* out = outputs + ((size_t)level * B + b) * C;
#pragma unroll
    for (uint32_t ch = 0; ch < C; ch++) out[ch] = res[ch];
}

// [B,L*C] output (what gridencoder/grid.py:57 obtains with an extra permute pass).  A thread per sample that wrote its C values of every level
// straight to its row put neighbouring lanes' stores L*C*4 bytes apart (0.309 ms per 1.02 M samples against 0.172 for [L,B,C]); a thread per
// (sample, level) with the level varying fastest writes coalesced but gathers from all L tables at once (0.306 ms: the tables no longer take turns
// in L2).  Here a workgroup keeps its 256 samples, walks the levels like the [L,B,C] launch does — the workgroups of a launch move through the
// levels roughly together — collects the rows in LDS (row stride padded by one bank) and writes them out whole.
template <uint32_t D, uint32_t C, typename T>
__global__ void __launch_bounds__(256) k_grid_encode_rows(const float* __restrict__ inputs, const T* __restrict__ emb, PnGridLevels lv, uint32_t B,
                                                          int align_corners, uint32_t interp, T* __restrict__ outputs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rows_raw[];
    T* rows = reinterpret_cast<T*>(rows_raw);
    const uint32_t row = lv.L * C, stride = row + (sizeof(T) == 4 ? 1 : 2);
    const uint32_t b0 = blockIdx.x * 256u, b = b0 + threadIdx.x;
    float in[D];
    load_point_or_outside<D>(inputs, b, B, in);  // past the end: encoded as out of range, never written
    for (uint32_t level = 0; level < lv.L; level++) {
        T res[C];
        grid_encode_one<D, C, T>(in, emb, lv, level, align_corners, interp, res);
#pragma unroll
        for (uint32_t ch = 0; ch < C; ch++) rows[threadIdx.x * stride + level * C + ch] = res[ch];
    }
    __syncthreads();
    const uint32_t n_rows = min(256u, B - b0);
    for (uint32_t i = threadIdx.x; i < n_rows * row; i += 256) outputs[(size_t)b0 * row + i] = rows[(i / row) * stride + (i % row)];
}

// dy_dx [B, L, D, C] (gridencoder.cu:199-243)
template <uint32_t D, uint32_t C>
__global__ void __launch_bounds__(256) k_grid_dy_dx(const float* __restrict__ inputs, const float* __restrict__ emb, PnGridLevels lv, uint32_t B,
                                                    int align_corners, uint32_t interp, float* __restrict__ dy_dx) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const uint32_t level = blockIdx.y;
    float* out = dy_dx + ((size_t)b * lv.L + level) * D * C;
    float in[D];
    load_point<D>(inputs, b, in);
    if (!in_range<D>(in)) {
#pragma unroll
        for (uint32_t i = 0; i < D * C; i++) out[i] = 0;  // gridencoder.cu:115-125
        return;
    }
    const float scale = lv.scale[level];
    const Cell<D> c = locate<D>(in, scale, align_corners, interp);
    const float* __restrict__ table = emb + (size_t)lv.offset[level] * C;
    const LevelIdx LI = level_idx(lv, level, align_corners);
#pragma unroll
    for (uint32_t gd = 0; gd < D; gd++) {
        float rg[C];
#pragma unroll
        for (uint32_t ch = 0; ch < C; ch++) rg[ch] = 0;
        for_each_edge<D>(c, gd, scale, [&](float w, const uint32_t (&pl)[D], const uint32_t (&pr)[D]) {
            const uint32_t il = grid_index<D>(LI, pl) * C, ir = grid_index<D>(LI, pr) * C;
#pragma unroll
            for (uint32_t ch = 0; ch < C; ch++) rg[ch] += w * (table[ir + ch] - table[il + ch]) * c.deriv[gd];
        });
#pragma unroll
        for (uint32_t ch = 0; ch < C; ch++) out[gd * C + ch] = rg[ch];
    }
}

// ------------------------------------------------------------------------------------------------ backward
// The wave-level fold's two element types.  float: one channel per shuffle and per atomic.  _Float16 (kernel_grid_backward<at::Half>, the table is
// half under autocast, grid.py:43-44): every contribution is rounded to half — (__half)(w * grad), gridencoder.cu:327 — partial sums are half
// additions (each rounded to half, as an atomic would leave it), and channels travel and land two at a time (:324-331: atomicAdd on a __half2; here
// global_atomic_pk_add_f16).  C even there (the reference uses this path for N_C % 2 == 0; with one channel autocast keeps fp32).
typedef _Float16 pn_gh2 __attribute__((ext_vector_type(2)));
template <uint32_t C>
__device__ __forceinline__ void fold_from_below(float (&v)[C], int off, bool take) {
#pragma unroll
    for (uint32_t ch = 0; ch < C; ch++) {
        const float o = __shfl_down(v[ch], off, 64);
        if (take) v[ch] += o;
    }
}
template <uint32_t C>
__device__ __forceinline__ void fold_from_below(_Float16 (&v)[C], int off, bool take) {
    static_assert(C % 2 == 0, "channel pairs");
#pragma unroll
    for (uint32_t ch = 0; ch < C; ch += 2) {
        const pn_gh2 mine = {v[ch], v[ch + 1]};
        const pn_gh2 o = __builtin_bit_cast(pn_gh2, __shfl_down(__builtin_bit_cast(int, mine), off, 64));
        if (take) { v[ch] = v[ch] + o.x; v[ch + 1] = v[ch + 1] + o.y; }
    }
}
template <uint32_t C>
__device__ __forceinline__ void atomic_add_row(float* __restrict__ row, const float (&v)[C]) {
#pragma unroll
    for (uint32_t ch = 0; ch < C; ch++) unsafeAtomicAdd(row + ch, v[ch]);
}
template <uint32_t C>
__device__ __forceinline__ void atomic_add_row(_Float16* __restrict__ row, const _Float16 (&v)[C]) {
#pragma unroll
    for (uint32_t ch = 0; ch < C; ch += 2) {
        const pn_gh2 pk = {v[ch], v[ch + 1]};
        __builtin_amdgcn_global_atomic_fadd_v2f16(reinterpret_cast<pn_gh2*>(row + ch), pk);
    }
}

// grad_embeddings += w * grad (gridencoder.cu:248-340); grad [L, B, C], T = float or _Float16 for grad and the table's gradient.
// Device-scope atomics execute at the memory side on gfx950 (the per-XCD L2s are not coherent), ~10 ns each when they pile up on one address, and
// that is exactly what the coarse levels do: samples arrive in ray order (pn_march_rays_train keeps them so), so neighbouring lanes sit in the same
// cell of a 16..100-cell-wide level and hit the same 2^D corners.  Each wave therefore folds runs of equal target rows before touching memory: a lane
// starts a run when its row differs from the previous lane's, run ids come from a ballot + prefix popcount, a 6-step shuffle tree adds a lane's
// partial to the lane `off` below it while both carry the same run id (ids are monotonic, so equal ids = one contiguous run), and only run heads
// issue the atomic.  Fine hashed levels (no sharing) degenerate to one atomic per lane; coarse levels drop to one per cell crossing.
template <uint32_t D, uint32_t C, typename T>
__global__ void __launch_bounds__(256) k_grid_backward(const T* __restrict__ grad, const float* __restrict__ inputs, PnGridLevels lv, uint32_t B,
                                                       int align_corners, uint32_t interp, T* __restrict__ grad_emb) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t level = blockIdx.y;
    const uint32_t lane = threadIdx.x & 63;
    float in[D];
    load_point_or_outside<D>(inputs, b, B, in);
    const bool valid = in_range<D>(in);
    Cell<D> c = {};   // stays zero for a lane that is not valid: its row is no row and its value is 0
    if (valid) c = locate<D>(in, lv.scale[level], align_corners, interp);
    T* __restrict__ gt = grad_emb + (size_t)lv.offset[level] * C;
    const LevelIdx LI = level_idx(lv, level, align_corners);
    float g[C];
#pragma unroll
    for (uint32_t ch = 0; ch < C; ch++) g[ch] = valid ? (float)grad[((size_t)level * B + b) * C + ch] : 0.0f;
    for_each_corner<D>(c, [&](float w, const uint32_t (&pl)[D]) {
        const uint32_t row = valid ? grid_index<D>(LI, pl) : 0xFFFFFFFFu;
        T v[C];
#pragma unroll
        for (uint32_t ch = 0; ch < C; ch++) v[ch] = valid ? (T)(w * g[ch]) : (T)0.0f;
        const uint32_t prev = __shfl_up(row, 1, 64);
        const bool head = lane == 0 || prev != row;
        const unsigned long long heads = __ballot(head);
        const uint32_t run = __popcll(heads & ((2ull << lane) - 1ull));  // number of heads at or below this lane: monotonic run id
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t run2 = __shfl_down(run, off, 64);
            fold_from_below<C>(v, off, lane + off < 64 && run2 == run);
        }
        if (head && row != 0xFFFFFFFFu) atomic_add_row<C>(gt + (size_t)row * C, v);
    });
}

// grad_inputs[b, d] = sum_{l,c} grad[l,b,c] * dy_dx[b,l,d,c] (gridencoder.cu:343-369)
__global__ void __launch_bounds__(256) k_grid_input_backward(const float* __restrict__ grad, const float* __restrict__ dy_dx, float* __restrict__ grad_inputs,
                                                             uint32_t B, uint32_t L, uint32_t D, uint32_t C) {
    const uint32_t t = threadIdx.x + blockIdx.x * blockDim.x;
    if (t >= B * D) return;
    const uint32_t b = t / D, d = t - b * D;
    float result = 0;
    for (uint32_t l = 0; l < L; l++)
        for (uint32_t ch = 0; ch < C; ch++) result += grad[((size_t)l * B + b) * C + ch] * dy_dx[(((size_t)b * L + l) * D + d) * C + ch];
    grad_inputs[t] = result;
}

// kernel_grad_tv<float, D, C> (gridencoder.cu:506-611)
template <uint32_t D, uint32_t C>
__global__ void __launch_bounds__(256) k_grad_tv(const float* __restrict__ inputs, const float* __restrict__ emb, float* __restrict__ grad, PnGridLevels lv,
                                                 float weight, uint32_t B, int align_corners) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const uint32_t level = blockIdx.y;
    float in[D];
    load_point<D>(inputs, b, in);
    if (!in_range<D>(in)) return;
    const Cell<D> c = locate<D>(in, lv.scale[level], align_corners, 0);
    const float* __restrict__ table = emb + (size_t)lv.offset[level] * C;
    float* __restrict__ gt = grad + (size_t)lv.offset[level] * C;
    const LevelIdx LI = level_idx(lv, level, align_corners);
    const uint32_t resolution = lv.resolution[level];
    float results[C], idelta[C], here[C];
    const uint32_t index = grid_index<D>(LI, c.pg) * C;
#pragma unroll
    for (uint32_t ch = 0; ch < C; ch++) { results[ch] = 0; idelta[ch] = 0; here[ch] = table[index + ch]; }
    const float w = weight / (2 * D);
    const auto neighbour = [&](uint32_t d, uint32_t at) {
        uint32_t pn[D];
#pragma unroll
        for (uint32_t e = 0; e < D; e++) pn[e] = e == d ? at : c.pg[e];
        const uint32_t there = grid_index<D>(LI, pn) * C;
#pragma unroll
        for (uint32_t ch = 0; ch < C; ch++) { const float gv = here[ch] - table[there + ch]; results[ch] += gv; idelta[ch] += gv * gv; }
    };
#pragma unroll
    for (uint32_t d = 0; d < D; d++) {
        if (c.pg[d] < resolution) neighbour(d, c.pg[d] + 1);
        if (c.pg[d] > 0) neighbour(d, c.pg[d] - 1);
    }
#pragma unroll
    for (uint32_t ch = 0; ch < C; ch++) unsafeAtomicAdd(gt + index + ch, w * results[ch] * (1.0f / sqrtf(idelta[ch] + 1e-9f)));
}

// ------------------------------------------------------------------------------------------------ host side
template <uint32_t N>
using Const = std::integral_constant<uint32_t, N>;

// f(Const<D>, Const<C>) for the run-time (D, C): one switch for every kernel family of this file (gridencoder.cu:376-399)
template <uint32_t D, typename F>
int dispatch_c(uint32_t C, F&& f) {
    switch (C) {
        case 1: return f(Const<D>{}, Const<1>{});
        case 2: return f(Const<D>{}, Const<2>{});
        case 4: return f(Const<D>{}, Const<4>{});
        case 8: return f(Const<D>{}, Const<8>{});
        default: return PN_ERR_ARG;
    }
}
template <typename F>
int dispatch_dc(uint32_t D, uint32_t C, F&& f) {
    switch (D) {
        case 2: return dispatch_c<2>(C, f);
        case 3: return dispatch_c<3>(C, f);
        case 4: return dispatch_c<4>(C, f);
        case 5: return dispatch_c<5>(C, f);
        default: return PN_ERR_ARG;
    }
}

// what every entry point requires of its shape arguments, and the level table they determine
int grid_levels(PnGridLevels* lv, const int* offsets_host, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype,
                int align_corners, uint32_t interp) {
    PN_REQUIRE(D >= 2 && D <= 5);                         // "GridEncoding: D must be 2, 3, 4, 5" (gridencoder.cu:393-398)
    PN_REQUIRE(C == 1 || C == 2 || C == 4 || C == 8);     // gridencoder.cu:376-382
    PN_REQUIRE(gridtype <= 1 && interp <= 1);
    PN_REQUIRE((uint64_t)B * D < (1ull << 32));           // load_point indexes the inputs with 32 bits
    PN_REQUIRE(L >= 1 && L <= PN_MAX_LEVELS);
    PN_REQUIRE(pn_fill_grid_levels(lv, offsets_host, L, C, D, S, H, gridtype, align_corners) == PN_OK);
    return PN_OK;
}

template <typename T>
int grid_encode_launch(const float* inputs, const T* embeddings, const int* offsets_host, T* outputs, uint32_t B, uint32_t D, uint32_t C, uint32_t L,
                       float S, uint32_t H, float* dy_dx, uint32_t gridtype, int align_corners, uint32_t interp, int out_bl_major, hipStream_t st) {
    PN_REQUIRE(inputs && embeddings && offsets_host && outputs);
    PN_REQUIRE(sizeof(T) == 4 || D == 3);                 // the half table form is built for D = 3 only
    PnGridLevels lv;
    if (const int rc = grid_levels(&lv, offsets_host, B, D, C, L, S, H, gridtype, align_corners, interp)) return rc;
    return dispatch_dc(D, C, [&](auto d, auto c) -> int {
        if constexpr (sizeof(T) == 4 || d() == 3) {
            const dim3 grid(pn_div_up(B, 256), L, 1);
            if (out_bl_major) {
                const size_t lds = (size_t)256 * (L * c() + (sizeof(T) == 4 ? 1 : 2)) * sizeof(T);
                PN_REQUIRE(lds <= 150 * 1024);
                if (lds > 64 * 1024)  // opted into per call: rows this long (C = 8 with 16 levels) are not on any hot path
                    PN_HIP_CHECK(hipFuncSetAttribute((const void*)k_grid_encode_rows<d(), c(), T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                k_grid_encode_rows<d(), c(), T><<<dim3(grid.x, 1, 1), 256, lds, st>>>(inputs, embeddings, lv, B, align_corners, interp, outputs);
            } else {
                k_grid_encode<d(), c(), T><<<grid, 256, 0, st>>>(inputs, embeddings, lv, B, align_corners, interp, outputs);
            }
            if constexpr (sizeof(T) == 4) {
                if (dy_dx) k_grid_dy_dx<d(), c()><<<grid, 256, 0, st>>>(inputs, embeddings, lv, B, align_corners, interp, dy_dx);
            }
            PN_LAUNCH_CHECK();
            return PN_OK;
        }
        return PN_ERR_ARG;
    });
}

template <typename T>
int grid_backward_launch(const T* grad, const float* inputs, const int* offsets_host, T* grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L,
                         float S, uint32_t H, const float* dy_dx, float* grad_inputs, uint32_t gridtype, int align_corners, uint32_t interp, hipStream_t st) {
    PN_REQUIRE(grad && inputs && offsets_host && grad_embeddings);
    PN_REQUIRE(sizeof(T) == 4 || (D == 3 && C % 2 == 0));  // the half form: D = 3, channel pairs
    PN_REQUIRE((dy_dx == nullptr) == (grad_inputs == nullptr));
    PnGridLevels lv;
    if (const int rc = grid_levels(&lv, offsets_host, B, D, C, L, S, H, gridtype, align_corners, interp)) return rc;
    return dispatch_dc(D, C, [&](auto d, auto c) -> int {
        if constexpr (sizeof(T) == 4 || (d() == 3 && c() % 2 == 0)) {
            k_grid_backward<d(), c(), T><<<dim3(pn_div_up(B, 256), L, 1), 256, 0, st>>>(grad, inputs, lv, B, align_corners, interp, grad_embeddings);
            if constexpr (sizeof(T) == 4) {
                if (dy_dx) k_grid_input_backward<<<pn_div_up((uint64_t)B * D, 256), 256, 0, st>>>(grad, dy_dx, grad_inputs, B, L, D, C);
            }
            PN_LAUNCH_CHECK();
            return PN_OK;
        }
        return PN_ERR_ARG;
    });
}

}  // namespace

extern "C" int pn_grid_encode_forward(const float* inputs, const float* embeddings, const int* offsets_host, float* outputs, uint32_t B, uint32_t D,
                                      uint32_t C, uint32_t L, float S, uint32_t H, float* dy_dx, uint32_t gridtype, int align_corners,
                                      uint32_t interp, int out_bl_major, void* stream) {
    if (B == 0) return PN_OK;  // empty tensors have null data pointers
    return grid_encode_launch<float>(inputs, embeddings, offsets_host, outputs, B, D, C, L, S, H, dy_dx, gridtype, align_corners, interp, out_bl_major,
                                     (hipStream_t)stream);
}

extern "C" int pn_grid_encode_forward_half(const float* inputs, const uint16_t* embeddings, const int* offsets_host, uint16_t* outputs, uint32_t B,
                                           uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype, int align_corners,
                                           uint32_t interp, int out_bl_major, void* stream) {
    if (B == 0) return PN_OK;
    return grid_encode_launch<_Float16>(inputs, reinterpret_cast<const _Float16*>(embeddings), offsets_host, reinterpret_cast<_Float16*>(outputs), B, D,
                                        C, L, S, H, nullptr, gridtype, align_corners, interp, out_bl_major, (hipStream_t)stream);
}

extern "C" int pn_grid_encode_backward(const float* grad, const float* inputs, const float* embeddings, const int* offsets_host, float* grad_embeddings,
                                       uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, const float* dy_dx, float* grad_inputs,
                                       uint32_t gridtype, int align_corners, uint32_t interp, void* stream) {
    (void)embeddings;  // the fp32 path never reads the table in backward (the reference passes it for its dtype only)
    if (B == 0) return PN_OK;
    return grid_backward_launch<float>(grad, inputs, offsets_host, grad_embeddings, B, D, C, L, S, H, dy_dx, grad_inputs, gridtype, align_corners, interp,
                                       (hipStream_t)stream);
}

extern "C" int pn_grid_encode_backward_half(const uint16_t* grad, const float* inputs, const int* offsets_host, uint16_t* grad_embeddings, uint32_t B,
                                            uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype, int align_corners, uint32_t interp,
                                            void* stream) {
    if (B == 0) return PN_OK;
    return grid_backward_launch<_Float16>(reinterpret_cast<const _Float16*>(grad), inputs, offsets_host, reinterpret_cast<_Float16*>(grad_embeddings), B, D,
                                          C, L, S, H, nullptr, nullptr, gridtype, align_corners, interp, (hipStream_t)stream);
}

extern "C" int pn_grad_total_variation(const float* inputs, const float* embeddings, float* grad, const int* offsets_host, float weight, uint32_t B,
                                       uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype, int align_corners, void* stream) {
    if (B == 0) return PN_OK;
    PN_REQUIRE(inputs && embeddings && grad && offsets_host);
    PnGridLevels lv;
    if (const int rc = grid_levels(&lv, offsets_host, B, D, C, L, S, H, gridtype, align_corners, 0)) return rc;
    return dispatch_dc(D, C, [&](auto d, auto c) -> int {
        k_grad_tv<d(), c()><<<dim3(pn_div_up(B, 256), L, 1), 256, 0, (hipStream_t)stream>>>(inputs, embeddings, grad, lv, weight, B, align_corners);
        PN_LAUNCH_CHECK();
        return PN_OK;
    });
}
