// NeRFRenderer.run (nerf/renderer.py:137-265) — the hierarchical-sampling renderer of a model built WITHOUT a density grid — in ONE kernel per
// ray set, and NeRFNetwork.color (nerf/network.py:165-194), the masked colour query, as a launch of its own.  gfx950 only.
//
// k_render_hier: one wave per ray, persistent workgroups of PN_HIER_WAVES waves (the waves stride over the rays), the ray's whole sample set in LDS.
// Per ray, with T = num_steps coarse and t = upsample_steps fine samples (T + t <= PN_HIER_MAX_SAMPLES):
//   phase 0  near / far (the body of k_near_far); z[i] = near + (far - near) linspace(0, 1, T)[i] into LDS; sigma of the T samples as ceil(T / 32)
//            passes of the 32-sample network tile (pn_net_tile.h, two lanes per sample) stopped after the sigma layer; only the sigma logit is kept.
//   phase 1  (t > 0) deltas -> alpha -> transmittance (a wave-level multiplicative scan over the LDS array, 64 samples per step with a carry) ->
//            weights; sample_pdf with det = True: w[1:-1] + 1e-5, normalised, the cdf as an additive scan with a leading 0, every lane inverts the
//            cdf for its ceil(t / 64) values of u by binary search in LDS (searchsorted(right = True)); the new z into LDS behind the coarse ones,
//            made non-decreasing by a running maximum (the formula is monotone up to one rounding at a bin edge; the reference sorts); their sigma
//            as ceil(t / 32) more tiles.
//   phase 2  merge by rank (both lists are sorted: position = own index + number of elements of the other list before it, ties: coarse first, which
//            is one of the orders a sort may give — equal z means equal position and sigma, so the order among ties does not reach the outputs),
//            deltas (the last one is sample_dist) -> weights, weights_sum and depth over ALL samples, mask = w > 1e-4 by ballot, the masked samples'
//            indices compacted into a queue; the queue runs through the FULL tile (sigma layers again for geo_feat, then the colour net) 32 at a
//            time — recomputing the few masked samples' sigma layers is cheaper than parking 15 features for every sample;
//            image = sum w rgb by wave reduction, + (1 - weights_sum) * background (a scalar, a per-ray colour, or none = 0), three stores.
// The three phases share ONE inlined copy of the tile: a single pass loop whose prologue depends on the phase.
// Every sum has a fixed order (per-lane partial sums in index order, then an xor butterfly), so two runs give the same bits and a ray's result does
// not depend on which wave renders it or on how the caller batches the rays.
//
// LDS: the network's weight image (fp16 hi/lo form 41.7 KB, bf16 split 62.2 KB) + 512 B of level records + 8 KB per wave (four arrays of
// PN_HIER_MAX_SAMPLES floats: z | sigma of the unsorted lists, z | sigma -> weight of the merged one; the cdf and the queue reuse whichever pair is
// idle) = 74.8 KB per workgroup in the default form: two workgroups per CU.
//
// This unit is built with -ffp-contract=off: the ray-side arithmetic (z, positions, deltas, alpha, the cdf's interpolation, the blend) rounds once per
// operation like the torch op sequence it restates (NeRFRenderer.run_ops); the network tile contracts inside itself (pn_net_tile.h).  The results are
// tolerance work, not bit-exact work: the scans associate differently from torch.cumprod / cumsum.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#define PN_TU_FP_CONTRACT_OFF 1
#include "pn_common.h"
#include "pn_encoders.h"
#include "pn_net_tile.h"

#define PN_HIER_WAVES 4
#define PN_HIER_MAX_SAMPLES 512   // T + t held in LDS per wave; pn_hier_max_samples() tells the caller, who takes the op path beyond it
#define PN_HIER_WAVE_FLOATS (4 * PN_HIER_MAX_SAMPLES)
#define PN_COLOR_WAVES 4
#define PN_COLOR_QUEUE 128        // ring of masked rows per wave: < 32 left over + 64 new

namespace {

struct HierAabb { float v[6]; };

// orders this wave's LDS traffic: what other lanes stored before is visible to the loads after (a wave's DS operations execute in order; the fence keeps
// the compiler from moving them across)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ float wave_sum(float v) {   // xor butterfly: every lane ends with the same bits
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ float scan_mul(float v, int lane) {   // inclusive
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const float o = __shfl_up(v, d); if (lane >= d) v = o * v; }
    return v;
}
__device__ __forceinline__ float scan_add(float v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const float o = __shfl_up(v, d); if (lane >= d) v = o + v; }
    return v;
}
__device__ __forceinline__ float scan_max(float v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const float o = __shfl_up(v, d); if (lane >= d) v = fmaxf(o, v); }
    return v;
}
// number of elements of the non-decreasing a[0..n) that are <= v (OR_EQUAL) or < v
template <bool OR_EQUAL>
__device__ __forceinline__ int count_before(const float* a, int n, float v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const float m = a[mid];
        if (OR_EQUAL ? (m <= v) : (m < v)) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// torch.linspace(start, end, steps)[i] in fp32 (ATen RangeFactories: from the start in the first half, from the end in the second)
__device__ __forceinline__ float linspace_at(float start, float end, int steps, int i) {
    if (steps <= 1) return start;
    const float step = (end - start) / (float)(steps - 1);
    return i < steps / 2 ? start + step * (float)i : end - step * (float)(steps - i - 1);
}

// deltas -> alpha -> transmittance -> weights over zs / sg [0, n) (renderer.py:186-191, :217-221); w[i] may be sg[i].  FINAL: also the per-lane partial
// sums of w and w * clamp((z - near) / (far - near), 0, 1) (:234-238; the clamp keeps the NaN of a ray that misses the box) and the queue of the
// samples with w > 1e-4 (:227), whose length is returned.
template <bool FINAL>
__device__ __forceinline__ int hier_weights(const float* zs, const float* sg, float* w, int n, float sample_dist, float density_scale, int lane,
                                            float near, float span, int* queue, float& ws_part, float& depth_part) {
    float carry = 1.0f;
    int nq = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const bool valid = i < n;
        float alpha = 0.0f, z = 0.0f;
        if (valid) {
            z = zs[i];
            const float delta = (i + 1 < n) ? zs[i + 1] - z : sample_dist;
            alpha = 1.0f - pn_expf((-delta * density_scale) * sg[i]);
        }
        const float a = valid ? (1.0f - alpha) + 1e-15f : 1.0f;
        const float incl = scan_mul(a, lane);
        float excl = __shfl_up(incl, 1);
        if (lane == 0) excl = 1.0f;
        const float wi = alpha * (carry * excl);
        carry = carry * __shfl(incl, 63);
        if (FINAL) {
            const bool m = valid && wi > 1e-4f;
            const unsigned long long b = __ballot(m);
            if (m) queue[nq + __popcll(b & ((1ull << lane) - 1ull))] = i;
            nq += __popcll(b);
            if (valid) {
                float q = (z - near) / span;
                q = q < 0.0f ? 0.0f : (q > 1.0f ? 1.0f : q);   // NaN stays NaN, as torch.clamp leaves it
                ws_part += wi;
                depth_part += wi * q;
            }
        }
        if (valid) w[i] = wi;
    }
    return nq;
}

template <bool X>
__global__ void __launch_bounds__(PN_HIER_WAVES * 64, 2)
k_render_hier(const PnByteLevel* __restrict__ lv, const float* __restrict__ emb, const uint4* __restrict__ wimg_g, float bound,
              const float* __restrict__ x_scales, const float* __restrict__ rays_o, const float* __restrict__ rays_d, uint32_t N, HierAabb aabb,
              float min_near, int T, int t, float density_scale, float bg_scalar, const float* __restrict__ bg_rays, float* __restrict__ image,
              float* __restrict__ depth, float* __restrict__ weights_sum) {
    extern __shared__ __attribute__((aligned(16))) uint4 wimg[];   // the weight image, the 16 level records, then PN_HIER_WAVE_FLOATS floats per wave
    constexpr int IMG_BYTES = X ? PN_NET_X_BYTES : PN_NET_SPLIT_BYTES;
    const float sf = X ? x_scales[0] : 1.0f, rsf = X ? x_scales[1] : 1.0f;
    if (blockIdx.x * PN_HIER_WAVES >= N) return;   // no ray for any wave of this block (uniform: before the barrier)
    for (int i = threadIdx.x; i < IMG_BYTES / 16; i += PN_HIER_WAVES * 64) wimg[i] = wimg_g[i];
    if (threadIdx.x < 16 * sizeof(PnByteLevel) / 16) wimg[IMG_BYTES / 16 + threadIdx.x] = reinterpret_cast<const uint4*>(lv)[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int s = lane & 31, half = lane >> 5;
    const uint4* __restrict__ wl = wimg + lane;
    const PnByteLevel* lds_lv = reinterpret_cast<const PnByteLevel*>(wimg + IMG_BYTES / 16) + 8 * half;
    float* const A = reinterpret_cast<float*>(wimg + IMG_BYTES / 16 + 16 * sizeof(PnByteLevel) / 16) + wid * PN_HIER_WAVE_FLOATS;   // z, unsorted: coarse | fine
    float* const B = A + PN_HIER_MAX_SAMPLES;                                                                                     // sigma, unsorted
    float* const Cm = B + PN_HIER_MAX_SAMPLES;                                                                                    // cdf, then merged z
    float* const Dm = Cm + PN_HIER_MAX_SAMPLES;                                                                                   // coarse weights, then merged sigma -> weight
    const float inv2b = 1.0f / (2 * bound);
    const uint32_t waves_total = gridDim.x * PN_HIER_WAVES;

    for (uint32_t ray = blockIdx.x * PN_HIER_WAVES + wid; ray < N; ray += waves_total) {
        const float ox = rays_o[ray * 3], oy = rays_o[ray * 3 + 1], oz = rays_o[ray * 3 + 2];
        const float dx = rays_d[ray * 3], dy = rays_d[ray * 3 + 1], dz = rays_d[ray * 3 + 2];
        float near, far;
        {   // kernel_near_far_from_aabb (raymarching.cu:91-159; pn_near_far.h restates the same for k_near_far and the frame prologue)
            const float rdx = 1 / dx, rdy = 1 / dy, rdz = 1 / dz;
            near = (aabb.v[0] - ox) * rdx; far = (aabb.v[3] - ox) * rdx;
            if (near > far) { const float c = near; near = far; far = c; }
            float near_y = (aabb.v[1] - oy) * rdy, far_y = (aabb.v[4] - oy) * rdy;
            if (near_y > far_y) { const float c = near_y; near_y = far_y; far_y = c; }
            bool miss = (near > far_y || near_y > far);
            if (!miss) {
                if (near_y > near) near = near_y;
                if (far_y < far) far = far_y;
                float near_z = (aabb.v[2] - oz) * rdz, far_z = (aabb.v[5] - oz) * rdz;
                if (near_z > far_z) { const float c = near_z; near_z = far_z; far_z = c; }
                miss = (near > far_z || near_z > far);
                if (!miss) {
                    if (near_z > near) near = near_z;
                    if (far_z < far) far = far_z;
                    if (near < min_near) near = min_near;
                }
            }
            if (miss) near = far = FLT_MAX;
        }
        const float span = far - near;
        const float sample_dist = span / (float)T;
        // num_steps = 1: the reference's deltas are cat([N, 0], ones_like([N, 0])) = [N, 0] — no sample at all: weights_sum = depth = 0, image = background
        const int n_coarse = T == 1 ? 0 : T;
        const float* zm = A;      // the final sample list: z ...
        float* sm = B;            // ... and sigma, overwritten by the weights
        int* queue = reinterpret_cast<int*>(Cm);
        float ws_part = 0.0f, depth_part = 0.0f, acc[3] = {0.0f, 0.0f, 0.0f};

#pragma unroll 1
        for (int ph = 0; ph < 3; ph++) {
            int n_items = 0, first = 0;
            if (ph == 0) {
                for (int i = lane; i < T; i += 64) A[i] = near + span * linspace_at(0.0f, 1.0f, T, i);   // renderer.py:159-161
                n_items = n_coarse;
            } else if (ph == 1) {
                if (t == 0) continue;
                float dummy0 = 0.0f, dummy1 = 0.0f;
                hier_weights<false>(A, B, Dm, T, sample_dist, density_scale, lane, near, span, nullptr, dummy0, dummy1);
                wave_sync();
                // sample_pdf(z_mid [T - 1], w[1:-1] [T - 2], t, det = True) (renderer.py:19-53, :194-195)
                const int nw = T - 2;
                float part = 0.0f;
                for (int j = lane; j < nw; j += 64) part += Dm[j + 1] + 1e-5f;
                const float total = wave_sum(part);
                float carry = 0.0f;
                if (lane == 0) Cm[0] = 0.0f;
                for (int base = 0; base < nw; base += 64) {
                    const int j = base + lane;
                    const float p = j < nw ? (Dm[j + 1] + 1e-5f) / total : 0.0f;
                    const float incl = scan_add(p, lane);
                    if (j < nw) Cm[j + 1] = carry + incl;
                    carry = carry + __shfl(incl, 63);
                }
                wave_sync();
                const int n_cdf = T - 1;
                for (int k = lane; k < t; k += 64) {
                    const float u = linspace_at(0.5f / (float)t, 1.0f - 0.5f / (float)t, t, k);
                    const int inds = count_before<true>(Cm, n_cdf, u);   // searchsorted(cdf, u, right=True)
                    const int below = max(inds - 1, 0), above = min(inds, n_cdf - 1);
                    const float c0 = Cm[below], c1 = Cm[above];
                    // bins: z_mid[j] = z[j] + 0.5 (z[j + 1] - z[j]), j <= T - 2
                    const float zb0 = A[below], zb1 = A[above];
                    const float b0 = zb0 + 0.5f * (A[below + 1] - zb0), b1 = zb1 + 0.5f * (A[above + 1] - zb1);
                    float denom = c1 - c0;
                    if (denom < 1e-5f) denom = 1.0f;
                    const float tt = (u - c0) / denom;
                    A[T + k] = b0 + tt * (b1 - b0);
                }
                wave_sync();
                float cmax = -FLT_MAX;
                for (int base = 0; base < t; base += 64) {   // non-decreasing: see the head of the file
                    const int k = base + lane;
                    const float v = k < t ? A[T + k] : -FLT_MAX;
                    const float incl = fmaxf(cmax, scan_max(v, lane));
                    if (k < t) A[T + k] = incl;
                    cmax = __shfl(incl, 63);
                }
                first = T;
                n_items = t;
            } else {
                if (t > 0) {
                    for (int i = lane; i < T; i += 64) {
                        const float z = A[i];
                        const int pos = i + count_before<false>(A + T, t, z);
                        Cm[pos] = z; Dm[pos] = B[i];
                    }
                    for (int k = lane; k < t; k += 64) {
                        const float z = A[T + k];
                        const int pos = k + count_before<true>(A, T, z);
                        Cm[pos] = z; Dm[pos] = B[T + k];
                    }
                    zm = Cm; sm = Dm; queue = reinterpret_cast<int*>(A);
                    wave_sync();
                }
                n_items = hier_weights<true>(zm, sm, sm, n_coarse + t, sample_dist, density_scale, lane, near, span, queue, ws_part, depth_part);
            }
            wave_sync();
#pragma unroll 1
            for (int p0 = 0; p0 < n_items; p0 += 32) {
                const int j = p0 + s;
                const bool valid = j < n_items;
                const int idx = valid ? (ph < 2 ? first + j : queue[j]) : 0;
                const float z = valid ? (ph < 2 ? A[idx] : zm[idx]) : near;
                // xyzs = rays_o + rays_d * z, clipped to the box componentwise (renderer.py:170-171, :197-198)
                const float px = fminf(fmaxf(ox + dx * z, aabb.v[0]), aabb.v[3]);
                const float py = fminf(fmaxf(oy + dy * z, aabb.v[1]), aabb.v[4]);
                const float pz = fminf(fmaxf(oz + dz * z, aabb.v[2]), aabb.v[5]);
                f32x16 h2;
                if (X) h2 = tile_sigma_net_x<PN_BF_LU>(lds_lv, emb, wl, half, bound, inv2b, px, py, pz, sf);
                else h2 = tile_sigma_net<PN_BF_LU>(lds_lv, emb, wl, half, bound, inv2b, px, py, pz);
                if (ph < 2) {
                    if (valid && half == 0) B[idx] = tile_sigma_out(1.0f, X ? h2[0] * rsf : h2[0]);   // density(): sigma = trunc_exp(h[0])
                    continue;
                }
                __builtin_amdgcn_sched_barrier(0);
                float e[3];
                if (X) tile_color_net_x(wl, wimg, half, h2, dx, dy, dz, e);
                else tile_color_net(wl, wimg, half, h2, dx, dy, dz, e);
                if (valid && half == 0) {
                    const float w = sm[idx];
#pragma unroll
                    for (int o = 0; o < 3; o++) acc[o] += w * tile_rgb_out(e[o]);
                }
            }
            wave_sync();
        }
        const float ws = wave_sum(ws_part), dp = wave_sum(depth_part);
        float rgb[3];
#pragma unroll
        for (int o = 0; o < 3; o++) rgb[o] = wave_sum(acc[o]);
        if (lane == 0) {
            const float omw = 1.0f - ws;
#pragma unroll
            for (int o = 0; o < 3; o++) {
                const float bg = bg_rays ? bg_rays[ray * 3 + o] : bg_scalar;
                const float tb = omw * bg;   // image + (1 - weights_sum) * bg_color (renderer.py:251): two roundings (this unit does not contract)
                image[ray * 3 + o] = rgb[o] + tb;
            }
            depth[ray] = dp;
            weights_sum[ray] = ws;
        }
    }
}

// NeRFNetwork.color(x, d, mask, geo_feat): the colour tile on the rows whose mask byte is set (all rows without a mask), zeros elsewhere.  A wave walks
// its 64-row chunks, stores the zeros, collects the masked rows in a ring in LDS and runs a tile whenever 32 are waiting (and once more at the end), so
// the matrix work is proportional to the number of masked rows.  FORM 0: bf16 three-way split, 1: fp16 hi / lo (both fp32-accurate), 2: the autocast form.
template <int FORM>
__global__ void __launch_bounds__(PN_COLOR_WAVES * 64, 2)
k_nerf_color(const uint4* __restrict__ wimg_g, const float* __restrict__ x_scales, const float* __restrict__ dirs, const float* __restrict__ geo,
             const uint8_t* __restrict__ mask, uint32_t M, float* __restrict__ rgbs) {
    extern __shared__ __attribute__((aligned(16))) uint4 wimg[];   // the weight image, then PN_COLOR_QUEUE ints per wave
    constexpr int IMG_BYTES = FORM == 2 ? PN_NET_HALF_BYTES : (FORM == 1 ? PN_NET_X_BYTES : PN_NET_SPLIT_BYTES);
    const uint32_t n_chunks = (M + 63) / 64;
    if (blockIdx.x * PN_COLOR_WAVES >= n_chunks) return;
    for (int i = threadIdx.x; i < IMG_BYTES / 16; i += PN_COLOR_WAVES * 64) wimg[i] = wimg_g[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int s = lane & 31, half = lane >> 5;
    const uint4* __restrict__ wl = wimg + lane;
    uint32_t* const ring = reinterpret_cast<uint32_t*>(wimg + IMG_BYTES / 16) + wid * PN_COLOR_QUEUE;
    const float gscale = FORM == 1 ? 1.0f / x_scales[1] : 1.0f;   // the scale the density net's outputs leave the matrix pipe at (a power of two: exact)
    const uint32_t waves_total = gridDim.x * PN_COLOR_WAVES;
    uint32_t head = 0, tail = 0;
    uint32_t chunk = blockIdx.x * PN_COLOR_WAVES + wid;
    bool more = chunk < n_chunks;
    while (more || tail != head) {
        if (more) {
            const uint32_t row = chunk * 64 + lane;
            const bool in = row < M;
            const bool m = in && (mask ? mask[row] != 0 : true);
            if (in && !m) { rgbs[row * 3] = 0.0f; rgbs[row * 3 + 1] = 0.0f; rgbs[row * 3 + 2] = 0.0f; }
            const unsigned long long b = __ballot(m);
            if (m) ring[(tail + __popcll(b & ((1ull << lane) - 1ull))) & (PN_COLOR_QUEUE - 1)] = row;
            tail += __popcll(b);
            chunk += waves_total;
            more = chunk < n_chunks;
            wave_sync();
            if (more && tail - head < 32) continue;
        }
        while (tail - head >= 32 || (!more && tail != head)) {
            const uint32_t avail = min(tail - head, 32u);
            const bool valid = (uint32_t)s < avail;
            const uint32_t row = valid ? ring[(head + s) & (PN_COLOR_QUEUE - 1)] : 0u;
            float dx = 0.f, dy = 0.f, dz = 1.f;
            float g[8];
#pragma unroll
            for (int r = 0; r < 8; r++) g[r] = 0.0f;
            if (valid) {
                dx = dirs[row * 3]; dy = dirs[row * 3 + 1]; dz = dirs[row * 3 + 2];
                const float* __restrict__ gr = geo + (size_t)row * 15;
#pragma unroll
                for (int r = 0; r < 8; r++) {   // this lane's rows (r&3) + 8 (r>>2) + 4 half of the sigma net's 16 outputs; row 0 (sigma) is not an input
                    const int rw = (r & 3) + 8 * (r >> 2) + 4 * half;
                    if (rw >= 1) g[r] = gr[rw - 1] * gscale;
                }
            }
            float e[3];
            if (FORM == 2) {
                tile_color_net_h(wl, wimg, half, g, dx, dy, dz, e);
            } else {
                f32x16 h2 = {0};
#pragma unroll
                for (int r = 0; r < 8; r++) h2[r] = g[r];
                __builtin_amdgcn_sched_barrier(0);
                if (FORM == 1) tile_color_net_x(wl, wimg, half, h2, dx, dy, dz, e);
                else tile_color_net(wl, wimg, half, h2, dx, dy, dz, e);
            }
            if (valid && half == 0) {
#pragma unroll
                for (int o = 0; o < 3; o++) rgbs[row * 3 + o] = FORM == 2 ? tile_rgb_out_h(e[o]) : tile_rgb_out(e[o]);
            }
            head += avail;
            wave_sync();
        }
    }
}

int color_launch(const pn_net* net, const float* dirs, const float* geo, const uint8_t* mask, uint32_t M, float* rgbs, bool half, hipStream_t st) {
    if (M == 0) return PN_OK;
    PN_REQUIRE(net && dirs && geo && rgbs);
    PN_REQUIRE(M <= 0x7fffffffu / 15u);
    const uint32_t blocks = std::min(pn_div_up(pn_div_up(M, 64), PN_COLOR_WAVES), 1024u);
    const size_t ring = PN_COLOR_WAVES * PN_COLOR_QUEUE * sizeof(uint32_t);
    if (half) {
        PN_REQUIRE(net->emb_half && net->whalf);   // pn_net_enable_half first
        k_nerf_color<2><<<blocks, PN_COLOR_WAVES * 64, PN_NET_HALF_BYTES + ring, st>>>((const uint4*)net->whalf, nullptr, dirs, geo, mask, M, rgbs);
    } else if (net->x_ok) {
        k_nerf_color<1><<<blocks, PN_COLOR_WAVES * 64, PN_NET_X_BYTES + ring, st>>>((const uint4*)net->wx, net->x_scales, dirs, geo, mask, M, rgbs);
    } else {
        k_nerf_color<0><<<blocks, PN_COLOR_WAVES * 64, PN_NET_SPLIT_BYTES + ring, st>>>((const uint4*)net->wsplit, nullptr, dirs, geo, mask, M, rgbs);
    }
    PN_LAUNCH_CHECK();
    return PN_OK;
}

}  // namespace

extern "C" int pn_hier_max_samples(void) { return PN_HIER_MAX_SAMPLES; }

extern "C" int pn_render_hier(const pn_net* net, const float* rays_o, const float* rays_d, uint32_t N, const float* aabb_host, float min_near, int num_steps,
                              int upsample_steps, float density_scale, float bg_scalar, const float* bg_rays, float* image, float* depth, float* weights_sum,
                              int half, void* stream) {
    PN_REQUIRE(aabb_host && num_steps >= 1 && upsample_steps >= 0);
    PN_REQUIRE(upsample_steps == 0 || num_steps >= 3);                    // sample_pdf needs a weight between the first and the last sample
    PN_REQUIRE(num_steps + upsample_steps <= PN_HIER_MAX_SAMPLES);
    PN_REQUIRE(half == 0);                                                // the autocast form of run takes the op path (NeRFRenderer.run)
    if (N == 0) return PN_OK;
    PN_REQUIRE(net && rays_o && rays_d && image && depth && weights_sum);
    PN_REQUIRE(N <= 0x7fffffffu / 3u);
    HierAabb box;
    for (int i = 0; i < 6; i++) box.v[i] = aabb_host[i];
    hipStream_t st = (hipStream_t)stream;
    const uint32_t blocks = std::min(pn_div_up(N, PN_HIER_WAVES), 512u);   // two workgroups per CU x 256 CUs; the waves stride over the rays
    const size_t wave_bytes = (size_t)PN_HIER_WAVES * PN_HIER_WAVE_FLOATS * sizeof(float);
    // more than 64 KB of dynamic LDS needs the attribute, once per device and kernel
    static bool attr_set[PN_MAX_DEVICES][2];
    int dev = 0;
    PN_HIP_CHECK(hipGetDevice(&dev));
    PN_REQUIRE(dev >= 0 && dev < PN_MAX_DEVICES);
    if (net->x_ok) {
        const size_t lds = PN_NET_X_BYTES + 16 * sizeof(PnByteLevel) + wave_bytes;
        if (!attr_set[dev][1]) {
            PN_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_render_hier<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            attr_set[dev][1] = true;
        }
        k_render_hier<true><<<blocks, PN_HIER_WAVES * 64, lds, st>>>((const PnByteLevel*)net->byte_levels, net->embeddings, (const uint4*)net->wx, net->bound,
                                                                    net->x_scales, rays_o, rays_d, N, box, min_near, num_steps, upsample_steps, density_scale,
                                                                    bg_scalar, bg_rays, image, depth, weights_sum);
    } else {
        const size_t lds = PN_NET_SPLIT_BYTES + 16 * sizeof(PnByteLevel) + wave_bytes;
        if (!attr_set[dev][0]) {
            PN_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_render_hier<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            attr_set[dev][0] = true;
        }
        k_render_hier<false><<<blocks, PN_HIER_WAVES * 64, lds, st>>>((const PnByteLevel*)net->byte_levels, net->embeddings, (const uint4*)net->wsplit, net->bound,
                                                                     nullptr, rays_o, rays_d, N, box, min_near, num_steps, upsample_steps, density_scale,
                                                                     bg_scalar, bg_rays, image, depth, weights_sum);
    }
    PN_LAUNCH_CHECK();
    return PN_OK;
}

extern "C" int pn_nerf_color(const pn_net* net, const float* dirs, const float* geo_feat, const uint8_t* mask, uint32_t M, float* rgbs, void* stream) {
    return color_launch(net, dirs, geo_feat, mask, M, rgbs, false, (hipStream_t)stream);
}

extern "C" int pn_nerf_color_half(const pn_net* net, const float* dirs, const float* geo_feat, const uint8_t* mask, uint32_t M, float* rgbs, void* stream) {
    return color_launch(net, dirs, geo_feat, mask, M, rgbs, true, (hipStream_t)stream);
}
