// SSIM on channel-last images (pienerf_amd/metrics.py): the reference's SSIMMeter (nerf/utils.py:268-302) calls torchmetrics'
// structural_similarity_index_measure, which permutes to channel-first and runs five grouped 11 x 11 convolutions plus a dozen element-wise ops.
// Here: one launch over the [B, H, W, C] images the renderer produces (plus a B-block sum of the partials), and one launch for the gradient.
//
// Definition (include/pienerf_hip.h: pn_ssim_forward): Gaussian window of 11 taps, sigma 1.5, valid region only, S per position and channel from
// the five windowed moments, mean over positions and channels per image.
//
// Form, both kernels: ONE WORKGROUP PER 16 x 16 TILE, ALL CHANNELS.  The tile plus its 10-pixel halo is staged in LDS with the channel-last rows
// read as they lie in memory (consecutive lanes, consecutive floats), a horizontal pass writes the 11-tap row sums of every moment to a second LDS
// array, a vertical pass finishes them.  Channels go through in chunks of PN_SSIM_CH = 3 (RGB is one chunk): LDS per workgroup is
// 2 x 26 x 78 x 4 (images) + 5 x 26 x 48 x 4 (row sums) = 41,184 bytes, three workgroups = 12 waves per CU of the 160 KiB.  A 32 x 16 tile would
// read 2.1 instead of 2.6 input floats per output but needs 76 KiB: two workgroups per CU, and a 16 x 16 patch of the training loss (valid region
// 6 x 6) is one tile either way.
//
// Every operation rounds once, in source order (-ffp-contract=off), all sums run in a fixed order and nothing is accumulated with atomics: equal
// inputs give equal bits, whatever the grid does.  S is summed in fp64 (per thread, then a fixed shuffle tree, then the four waves in order); a
// second launch adds the workgroups' partials of an image in a fixed order.
#include <math.h>

#include "pn_common.h"

#define PN_SSIM_TAPS 11
#define PN_SSIM_HALO (PN_SSIM_TAPS - 1)
#define PN_SSIM_TILE 16
#define PN_SSIM_IN (PN_SSIM_TILE + PN_SSIM_HALO)   // 26 staged rows / columns
#define PN_SSIM_CH 3                               // channels per pass
#define PN_SSIM_THREADS 256
#define PN_SSIM_SW (PN_SSIM_IN * PN_SSIM_CH)       // floats per staged row
#define PN_SSIM_HW (PN_SSIM_TILE * PN_SSIM_CH)     // floats per row of row sums
#define PN_SSIM_RANGE_BLOCKS 256                   // partial (min, max) pairs of the range kernel
#define PN_SSIM_RANGE_BYTES (PN_SSIM_RANGE_BLOCKS * 4 * sizeof(float))

struct PnSsimTaps { float g[PN_SSIM_TAPS]; };

// g_i = exp(-((i - 5) / 1.5)^2 / 2) / sum, in double, rounded to fp32 once
static PnSsimTaps pn_ssim_taps() {
    PnSsimTaps t;
    double g[PN_SSIM_TAPS], s = 0.0;
    for (int i = 0; i < PN_SSIM_TAPS; i++) {
        const double d = (i - PN_SSIM_TAPS / 2) / 1.5;
        g[i] = exp(-d * d / 2.0);
        s += g[i];
    }
    for (int i = 0; i < PN_SSIM_TAPS; i++) t.g[i] = (float)(g[i] / s);
    return t;
}

__device__ __forceinline__ double pn_ssim_wave_sum(double v) {
#pragma unroll
    for (int o = PN_WAVE / 2; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;   // lane 0
}

// ------------------------------------------------------------------ data range -> c1, c2

// (min, max) of both images over a block's grid-stride share; min / max do not depend on the order they are taken in
__global__ void __launch_bounds__(PN_SSIM_THREADS) k_ssim_minmax(const float* __restrict__ pred, const float* __restrict__ truth, size_t n,
                                                                 float* __restrict__ part) {
    float pn = INFINITY, px = -INFINITY, tn = INFINITY, tx = -INFINITY;
    for (size_t i = (size_t)blockIdx.x * PN_SSIM_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * PN_SSIM_THREADS) {
        const float p = pred[i], t = truth[i];
        pn = fminf(pn, p);
        px = fmaxf(px, p);
        tn = fminf(tn, t);
        tx = fmaxf(tx, t);
    }
#pragma unroll
    for (int o = PN_WAVE / 2; o > 0; o >>= 1) {
        pn = fminf(pn, __shfl_down(pn, o));
        px = fmaxf(px, __shfl_down(px, o));
        tn = fminf(tn, __shfl_down(tn, o));
        tx = fmaxf(tx, __shfl_down(tx, o));
    }
    __shared__ float red[PN_SSIM_THREADS / PN_WAVE][4];
    const int wave = threadIdx.x / PN_WAVE;
    if (threadIdx.x % PN_WAVE == 0) {
        red[wave][0] = pn;
        red[wave][1] = px;
        red[wave][2] = tn;
        red[wave][3] = tx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < PN_SSIM_THREADS / PN_WAVE; w++) {
            pn = fminf(pn, red[w][0]);
            px = fmaxf(px, red[w][1]);
            tn = fminf(tn, red[w][2]);
            tx = fmaxf(tx, red[w][3]);
        }
        float* o = part + (size_t)blockIdx.x * 4;
        o[0] = pn;
        o[1] = px;
        o[2] = tn;
        o[3] = tx;
    }
}

// c12 = {(0.01 R)^2, (0.03 R)^2}; R = the host value, or with n_part > 0 max(pred.max - pred.min, truth.max - truth.min) of the partials.  One wave.
__global__ void __launch_bounds__(PN_WAVE) k_ssim_consts(const float* __restrict__ part, int n_part, float range, float* __restrict__ c12) {
    float R = range;
    if (n_part > 0) {
        float pn = INFINITY, px = -INFINITY, tn = INFINITY, tx = -INFINITY;
        for (int i = threadIdx.x; i < n_part; i += PN_WAVE) {
            pn = fminf(pn, part[i * 4]);
            px = fmaxf(px, part[i * 4 + 1]);
            tn = fminf(tn, part[i * 4 + 2]);
            tx = fmaxf(tx, part[i * 4 + 3]);
        }
#pragma unroll
        for (int o = PN_WAVE / 2; o > 0; o >>= 1) {
            pn = fminf(pn, __shfl_down(pn, o));
            px = fmaxf(px, __shfl_down(px, o));
            tn = fminf(tn, __shfl_down(tn, o));
            tx = fmaxf(tx, __shfl_down(tx, o));
        }
        R = fmaxf(px - pn, tx - tn);
    }
    if (threadIdx.x == 0) {
        const float k1 = 0.01f * R, k2 = 0.03f * R;
        c12[0] = k1 * k1;
        c12[1] = k2 * k2;
    }
}

// ------------------------------------------------------------------ forward

template <bool MAPS>
__global__ void __launch_bounds__(PN_SSIM_THREADS) k_ssim(const float* __restrict__ pred, const float* __restrict__ truth, int H, int W, int C,
                                                          PnSsimTaps taps, const float* __restrict__ c12, float* __restrict__ mapA,
                                                          float* __restrict__ mapB, float* __restrict__ mapD, double* __restrict__ partials) {
    __shared__ float sx[PN_SSIM_IN * PN_SSIM_SW], sy[PN_SSIM_IN * PN_SSIM_SW];
    __shared__ float hs[5][PN_SSIM_IN * PN_SSIM_HW];
    __shared__ double red[PN_SSIM_THREADS / PN_WAVE];
    const int tid = threadIdx.x, b = blockIdx.z;
    const int x0 = blockIdx.x * PN_SSIM_TILE, y0 = blockIdx.y * PN_SSIM_TILE;   // first output position = first staged pixel of the tile
    const int Hv = H - PN_SSIM_HALO, Wv = W - PN_SSIM_HALO;
    const float c1 = c12[0], c2 = c12[1];
    const float* g = taps.g;
    double acc = 0.0;

    for (int ch0 = 0; ch0 < C; ch0 += PN_SSIM_CH) {
        const int cn = min(PN_SSIM_CH, C - ch0);
        const int in_w = PN_SSIM_IN * cn, out_w = PN_SSIM_TILE * cn;
        if (ch0) __syncthreads();   // the previous chunk's vertical pass has read hs
        // stage: row r, then column, then channel: with cn == C a staged row is one contiguous run of the image
        for (int i = tid; i < PN_SSIM_IN * in_w; i += PN_SSIM_THREADS) {
            const int r = i / in_w, j = i - r * in_w, col = j / cn, ch = j - col * cn;
            const int y = y0 + r, x = x0 + col;
            float vx = 0.0f, vy = 0.0f;   // behind the image's edge: feeds only positions outside the valid region, which nothing reads
            if (y < H && x < W) {
                const size_t at = (((size_t)b * H + y) * W + x) * C + ch0 + ch;
                vx = pred[at];
                vy = truth[at];
            }
            sx[r * PN_SSIM_SW + j] = vx;
            sy[r * PN_SSIM_SW + j] = vy;
        }
        __syncthreads();
        // horizontal: the five moments' row sums, taps in ascending order
        for (int i = tid; i < PN_SSIM_IN * out_w; i += PN_SSIM_THREADS) {
            const int r = i / out_w, j = i - r * out_w;
            const float* px = sx + r * PN_SSIM_SW + j;
            const float* py = sy + r * PN_SSIM_SW + j;
            float m0 = 0.0f, m1 = 0.0f, m2 = 0.0f, m3 = 0.0f, m4 = 0.0f;
#pragma unroll
            for (int k = 0; k < PN_SSIM_TAPS; k++) {
                const float x = px[k * cn], y = py[k * cn], w = g[k];
                m0 += w * x;
                m1 += w * y;
                m2 += w * (x * x);
                m3 += w * (y * y);
                m4 += w * (x * y);
            }
            const int o = r * PN_SSIM_HW + j;
            hs[0][o] = m0;
            hs[1][o] = m1;
            hs[2][o] = m2;
            hs[3][o] = m3;
            hs[4][o] = m4;
        }
        __syncthreads();
        // vertical, then S and its derivatives
        for (int i = tid; i < PN_SSIM_TILE * out_w; i += PN_SSIM_THREADS) {
            const int r = i / out_w, j = i - r * out_w, col = j / cn, ch = j - col * cn;
            const int oy = y0 + r, ox = x0 + col;
            if (oy >= Hv || ox >= Wv) continue;
            float mx = 0.0f, my = 0.0f, exx = 0.0f, eyy = 0.0f, exy = 0.0f;
#pragma unroll
            for (int k = 0; k < PN_SSIM_TAPS; k++) {
                const int o = (r + k) * PN_SSIM_HW + j;
                const float w = g[k];
                mx += w * hs[0][o];
                my += w * hs[1][o];
                exx += w * hs[2][o];
                eyy += w * hs[3][o];
                exy += w * hs[4][o];
            }
            const float sxx = exx - mx * mx, syy = eyy - my * my, sxy = exy - mx * my;
            const float a1 = 2.0f * mx * my + c1, a2 = 2.0f * sxy + c2;
            const float b1 = mx * mx + my * my + c1, b2 = sxx + syy + c2;
            const float S = (a1 * a2) / (b1 * b2);
            acc += (double)S;
            if (MAPS) {
                // B = dS/dsxx = -S / b2;  D = dS/dsxy = 2 a1 / (b1 b2);  dS/dmx = a2 (2 my - 2 mx a1 / b1) / (b1 b2) with the sigmas held;
                // A = dS/dmx - 2 mx B - my D: the derivative with respect to mx of S written in the raw moments E[x], E[xx], E[xy]
                const float Bv = -S / b2;
                const float Dv = (2.0f * a1) / (b1 * b2);
                const float dmx = (a2 * (2.0f * my - (2.0f * mx) * (a1 / b1))) / (b1 * b2);
                const float Av = dmx - (2.0f * mx) * Bv - my * Dv;
                const size_t at = (((size_t)b * Hv + oy) * Wv + ox) * C + ch0 + ch;
                mapA[at] = Av;
                mapB[at] = Bv;
                mapD[at] = Dv;
            }
        }
    }
    acc = pn_ssim_wave_sum(acc);
    if (tid % PN_WAVE == 0) red[tid / PN_WAVE] = acc;
    __syncthreads();
    if (tid == 0) {
        double s = red[0];
        for (int w = 1; w < PN_SSIM_THREADS / PN_WAVE; w++) s += red[w];
        partials[((size_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = s;
    }
}

// out[b] = (sum of the image's n_tiles partials, in tile order per thread, then a fixed tree) / count.  One workgroup per image.
__global__ void __launch_bounds__(PN_SSIM_THREADS) k_ssim_finish(const double* __restrict__ partials, int n_tiles, double count,
                                                                 float* __restrict__ out) {
    __shared__ double red[PN_SSIM_THREADS / PN_WAVE];
    const double* p = partials + (size_t)blockIdx.x * n_tiles;
    double acc = 0.0;
    for (int i = threadIdx.x; i < n_tiles; i += PN_SSIM_THREADS) acc += p[i];
    acc = pn_ssim_wave_sum(acc);
    if (threadIdx.x % PN_WAVE == 0) red[threadIdx.x / PN_WAVE] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = red[0];
        for (int w = 1; w < PN_SSIM_THREADS / PN_WAVE; w++) s += red[w];
        out[blockIdx.x] = (float)(s / count);
    }
}

// ------------------------------------------------------------------ backward

// grad_pred[q] = grad_out[b] / count * ((w * A)_q + 2 x_q (w * B)_q + y_q (w * D)_q): the maps, zero outside the valid region, correlated with the
// window at every pixel.  Gather form: pixel q = (y, x) sums the positions (y - 10 .. y, x - 10 .. x); the taps are symmetric.
__global__ void __launch_bounds__(PN_SSIM_THREADS) k_ssim_backward(const float* __restrict__ pred, const float* __restrict__ truth, int H, int W, int C,
                                                                   PnSsimTaps taps, const float* __restrict__ mapA, const float* __restrict__ mapB,
                                                                   const float* __restrict__ mapD, const float* __restrict__ grad_out,
                                                                   float* __restrict__ grad_pred) {
    __shared__ float sm[3][PN_SSIM_IN * PN_SSIM_SW];
    __shared__ float hs[3][PN_SSIM_IN * PN_SSIM_HW];
    const int tid = threadIdx.x, b = blockIdx.z;
    const int x0 = blockIdx.x * PN_SSIM_TILE, y0 = blockIdx.y * PN_SSIM_TILE;   // first pixel of the tile; staged entry (r, col) = position (y0 - 10 + r, x0 - 10 + col)
    const int Hv = H - PN_SSIM_HALO, Wv = W - PN_SSIM_HALO;
    const float* g = taps.g;
    const float scale = grad_out[b] / (float)((double)Hv * (double)Wv * (double)C);

    for (int ch0 = 0; ch0 < C; ch0 += PN_SSIM_CH) {
        const int cn = min(PN_SSIM_CH, C - ch0);
        const int in_w = PN_SSIM_IN * cn, out_w = PN_SSIM_TILE * cn;
        if (ch0) __syncthreads();
        for (int i = tid; i < PN_SSIM_IN * in_w; i += PN_SSIM_THREADS) {
            const int r = i / in_w, j = i - r * in_w, col = j / cn, ch = j - col * cn;
            const int py = y0 - PN_SSIM_HALO + r, px = x0 - PN_SSIM_HALO + col;
            float a = 0.0f, bb = 0.0f, d = 0.0f;
            if (py >= 0 && py < Hv && px >= 0 && px < Wv) {
                const size_t at = (((size_t)b * Hv + py) * Wv + px) * C + ch0 + ch;
                a = mapA[at];
                bb = mapB[at];
                d = mapD[at];
            }
            sm[0][r * PN_SSIM_SW + j] = a;
            sm[1][r * PN_SSIM_SW + j] = bb;
            sm[2][r * PN_SSIM_SW + j] = d;
        }
        __syncthreads();
        for (int i = tid; i < PN_SSIM_IN * out_w; i += PN_SSIM_THREADS) {
            const int r = i / out_w, j = i - r * out_w;
            const int at = r * PN_SSIM_SW + j;
            float m0 = 0.0f, m1 = 0.0f, m2 = 0.0f;
#pragma unroll
            for (int k = 0; k < PN_SSIM_TAPS; k++) {
                const float w = g[k];
                m0 += w * sm[0][at + k * cn];
                m1 += w * sm[1][at + k * cn];
                m2 += w * sm[2][at + k * cn];
            }
            const int o = r * PN_SSIM_HW + j;
            hs[0][o] = m0;
            hs[1][o] = m1;
            hs[2][o] = m2;
        }
        __syncthreads();
        for (int i = tid; i < PN_SSIM_TILE * out_w; i += PN_SSIM_THREADS) {
            const int r = i / out_w, j = i - r * out_w, col = j / cn, ch = j - col * cn;
            const int y = y0 + r, x = x0 + col;
            if (y >= H || x >= W) continue;
            float cA = 0.0f, cB = 0.0f, cD = 0.0f;
#pragma unroll
            for (int k = 0; k < PN_SSIM_TAPS; k++) {
                const int o = (r + k) * PN_SSIM_HW + j;
                const float w = g[k];
                cA += w * hs[0][o];
                cB += w * hs[1][o];
                cD += w * hs[2][o];
            }
            const size_t at = (((size_t)b * H + y) * W + x) * C + ch0 + ch;
            grad_pred[at] = scale * (cA + (2.0f * pred[at]) * cB + truth[at] * cD);
        }
    }
}

// ------------------------------------------------------------------ C ABI

static bool pn_ssim_shape_ok(int B, int H, int W, int C) {
    // blockIdx.z carries the image and blockIdx.y the tile row; the tile counts and every per-image element count stay below 2^31
    return B > 0 && B <= 65535 && C > 0 && H >= PN_SSIM_TAPS && W >= PN_SSIM_TAPS && H <= 65535 * PN_SSIM_TILE &&
           (uint64_t)H * (uint64_t)W * (uint64_t)C < (1ull << 31);
}

extern "C" uint64_t pn_ssim_work_bytes(int B, int H, int W) {
    if (!pn_ssim_shape_ok(B, H, W, 1)) return 0;
    const uint64_t tiles = (uint64_t)pn_div_up(H - PN_SSIM_HALO, PN_SSIM_TILE) * pn_div_up(W - PN_SSIM_HALO, PN_SSIM_TILE);
    return PN_SSIM_RANGE_BYTES + (uint64_t)B * tiles * sizeof(double);
}

extern "C" int pn_ssim_range(const float* pred, const float* truth, uint64_t n, float data_range, void* work, float* c12, void* stream) {
    PN_REQUIRE(c12 != nullptr);
    hipStream_t s = (hipStream_t)stream;
    if (!pred && !truth) {
        PN_REQUIRE(data_range > 0.0f && isfinite(data_range));
        k_ssim_consts<<<1, PN_WAVE, 0, s>>>(nullptr, 0, data_range, c12);
        PN_LAUNCH_CHECK();
        return PN_OK;
    }
    PN_REQUIRE(pred && truth && work && n > 0);
    PN_REQUIRE((uintptr_t)work % 8 == 0);
    const uint32_t blocks = std::min<uint32_t>(PN_SSIM_RANGE_BLOCKS, pn_div_up(n, PN_SSIM_THREADS * 4));
    k_ssim_minmax<<<blocks, PN_SSIM_THREADS, 0, s>>>(pred, truth, (size_t)n, (float*)work);
    PN_LAUNCH_CHECK();
    k_ssim_consts<<<1, PN_WAVE, 0, s>>>((const float*)work, (int)blocks, 0.0f, c12);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

extern "C" int pn_ssim_forward(const float* pred, const float* truth, int B, int H, int W, int C, const float* c12, void* work, float* out,
                               float* mapA, float* mapB, float* mapD, void* stream) {
    PN_REQUIRE(pred && truth && c12 && work && out);
    PN_REQUIRE(pn_ssim_shape_ok(B, H, W, C));
    PN_REQUIRE((uintptr_t)work % 8 == 0);
    PN_REQUIRE((mapA && mapB && mapD) || (!mapA && !mapB && !mapD));
    const int Hv = H - PN_SSIM_HALO, Wv = W - PN_SSIM_HALO;
    const dim3 grid(pn_div_up(Wv, PN_SSIM_TILE), pn_div_up(Hv, PN_SSIM_TILE), B);
    double* partials = (double*)((char*)work + PN_SSIM_RANGE_BYTES);
    static const PnSsimTaps taps = pn_ssim_taps();
    hipStream_t s = (hipStream_t)stream;
    if (mapA)
        k_ssim<true><<<grid, PN_SSIM_THREADS, 0, s>>>(pred, truth, H, W, C, taps, c12, mapA, mapB, mapD, partials);
    else
        k_ssim<false><<<grid, PN_SSIM_THREADS, 0, s>>>(pred, truth, H, W, C, taps, c12, nullptr, nullptr, nullptr, partials);
    PN_LAUNCH_CHECK();
    k_ssim_finish<<<B, PN_SSIM_THREADS, 0, s>>>(partials, (int)(grid.x * grid.y), (double)Hv * (double)Wv * (double)C, out);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

extern "C" int pn_ssim_backward(const float* pred, const float* truth, int B, int H, int W, int C, const float* mapA, const float* mapB,
                                const float* mapD, const float* grad_out, float* grad_pred, void* stream) {
    PN_REQUIRE(pred && truth && mapA && mapB && mapD && grad_out && grad_pred);
    PN_REQUIRE(pn_ssim_shape_ok(B, H, W, C));
    const dim3 grid(pn_div_up(W, PN_SSIM_TILE), pn_div_up(H, PN_SSIM_TILE), B);
    static const PnSsimTaps taps = pn_ssim_taps();
    k_ssim_backward<<<grid, PN_SSIM_THREADS, 0, (hipStream_t)stream>>>(pred, truth, H, W, C, taps, mapA, mapB, mapD, grad_out, grad_pred);
    PN_LAUNCH_CHECK();
    return PN_OK;
}
