// The background model of NeRFNetwork (nerf/network.py:73-95,148-164; used at nerf/renderer.py:244-247, 283-286, 732-735, 799-801 with bg_radius > 0) in ONE
// kernel per frame, gfx950 only:
//   ray -> exit point on the sphere of `radius` as (theta, phi) in [-1, 1] (pn_sph.h: the very body of k_sph_from_ray)
//       -> GridEncoder(input_dim=2, 4 levels x 2 features, default bound 1: unit = (x + 1) / 2)              kernel_grid<float, 2, 2>, gridencoder.cu:87-197
//       -> cat([SH degree 4 of rays_d (16), grid features (8)])  — SH first —  -> Linear 24 -> 64, ReLU -> Linear 64 -> 3 -> sigmoid, no biases
//   and either rgb_out[N,3], or the renderer's blend in place: image = image + (1 - weights_sum) * rgb (renderer.py:288, :896), the multiply and the add
//   rounded separately, as torch's two ops round them.
//
// Wave layout (the render's network tile, pn_net_tile.h): a wave takes 64 consecutive rays as two tiles of 32; in a tile a ray has two lanes (lane & 31 = ray,
// lane >> 5 = half), which hold the two halves of every 16-wide K chunk of the first Linear's B operand on v_mfma_f32_32x32x16_f16:
//   chunk 0 = the 16 SH values (half 0: bands 0..7, half 1: 8..15); chunk 1 = the 8 grid features padded to 16 (half 0: levels 0, 1 + four zeros, half 1:
//   levels 2, 3 + four zeros) — so each lane gathers two levels' four corners, and the 24 -> 32 padding costs no gather.
// The coordinate and the SH basis are computed by both lanes of a pair (a few dozen instructions, against a cross-lane exchange of the B operands).
// Rays map to lanes in ray order: neighbouring pixels of an image row read neighbouring texels of the dense levels.
// fp32 form: every fp32 value as two fp16 pieces hi + lo, a product as hi*hi + hi*lo + lo*hi with the fp32 accumulator (pn_net_tile.h: split8x / split_mac_x),
// the SH values carried at 2^12 (|Y| < 4), the features at the power of two `sf` that puts the table's largest entry into (2^13, 2^14], the hidden layer at
// the power of two xs1 chosen the same way from the first Linear's row sums; the scales are folded into the weight image (bg_build_images) except `sf`, which
// the kernel reads from device memory beside the image so that launches captured into a HIP graph follow pn_bg_net_update.  A zero or non-finite bound takes
// the scale 1 (the result is then what the zero / non-finite weights make of it in any arithmetic): there is no second form.
// The 64 -> 3 Linear runs on the vector ALU in fp32 from the D layout (3 x 32 FMAs per lane + one cross-half add), as the colour net's last layer does.
// fp16 form (the reference under torch.cuda.amp.autocast): table entries rounded to half on load (= embeddings.to(torch.half), gridencoder/grid.py:43-44),
// kernel_grid<at::Half, 2, 2>'s half accumulation, half Linear layers with fp32 accumulation and one rounding per output, half sigmoid.
//
// This unit is built with -ffp-contract=off (the coordinate must equal pn_sph_from_ray's bit for bit, the blend must round twice); the network arithmetic of
// pn_net_tile.h contracts inside itself.  The 5.6 MB table is cache-resident: the kernel is bound by gather latency and instruction issue, not by HBM
// ("Background model").
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdint.h>

#define PN_TU_FP_CONTRACT_OFF 1
#include "pn_common.h"
#include "pn_net_tile.h"
#include "pn_sph.h"

#define PN_BG_LEVELS 4
#define PN_BG_IN 24      // 16 SH + 8 grid features
#define PN_BG_HIDDEN 64
#define PN_BG_GROUPS 4   // MFMA operand groups of the first Linear: (out tile t, K chunk kc) -> t * 2 + kc
// device image: [4 groups][hi, lo][64 lanes][8 fp16] | 192 fp32 (last Linear / xs1) | [4 groups][64 lanes][8 fp16] (half form) | 192 fp32 (half-rounded) | tail
#define PN_BG_X_W_BYTES (PN_BG_GROUPS * 2 * 64 * 16)
#define PN_BG_X_BYTES (PN_BG_X_W_BYTES + 192 * 4)
#define PN_BG_H_W_BYTES (PN_BG_GROUPS * 64 * 16)
#define PN_BG_H_BYTES (PN_BG_H_W_BYTES + 192 * 4)
#define PN_BG_TAIL_BYTES 16   // {table abs-max word, 0, sf, 0}
#define PN_BG_IMG_BYTES (PN_BG_X_BYTES + PN_BG_H_BYTES + PN_BG_TAIL_BYTES)
#define PN_BG_SH_SCALE 4096.0f
#define PN_BG_WAVES 4

struct PnBgLevel { float scale; uint32_t offset, stride, mask, hashed; };   // stride = resolution + 1 (dense: index g0 + g1 stride), mask = table size - 1 (hashed)
struct PnBgLevels { PnBgLevel l[PN_BG_LEVELS]; };

struct pn_bg_net {
    PnBgLevels levels;
    const float* embeddings;   // device, not owned
    uint32_t n_entries;
    unsigned char* img;        // device, owned: PN_BG_IMG_BYTES
    unsigned char* stage;      // host pinned: the same bytes, packed here and uploaded asynchronously
    hipEvent_t stage_done;     // the last upload that read `stage`
    float sf;                  // host copy of the features' scale
};

namespace {

// One level of kernel_grid<T, 2, 2> for one lane: corners in the reference's order (x, then y), weights (1 * wx) * wy.  `u0, u1` are already made safe for
// addressing (inside [0, 1]); the caller zeroes the result of an out-of-range input.  Dense level: index g0 + g1 stride < table size (pn_bg_net_create
// checks); hashed: (g0 ^ g1 * 2654435761) & mask.
template <bool HALF>
__device__ __forceinline__ void bg_encode_level(float scale, uint32_t offset, uint32_t stride, uint32_t mask, bool hashed, const float2* __restrict__ emb,
                                                float u0, float u1, float* out2) {
    float p0 = fmaf(u0, scale, 0.5f), p1 = fmaf(u1, scale, 0.5f);
    const float f0 = floorf(p0), f1 = floorf(p1);
    p0 -= f0; p1 -= f1;
    const uint32_t g0 = (uint32_t)f0, g1 = (uint32_t)f1;
    float2 e[4];
#pragma unroll
    for (int idx = 0; idx < 4; idx++) {
        const uint32_t a0 = g0 + (idx & 1), a1 = g1 + (idx >> 1);
        const uint32_t index = hashed ? ((a0 ^ (a1 * 2654435761u)) & mask) : (a0 + a1 * stride);
        e[idx] = emb[offset + index];
    }
    const float w0[2] = {1 - p0, p0}, w1[2] = {1 - p1, p1};
    if (HALF) {
        _Float16 r0 = (_Float16)0.0f, r1 = (_Float16)0.0f;
#pragma unroll
        for (int idx = 0; idx < 4; idx++) {
            const float w = (1 * w0[idx & 1]) * w1[idx >> 1];
            r0 = r0 + half_of_product(w, (_Float16)e[idx].x);   // Half(float * Half), then Half + Half (gridencoder.cu:184 with at::Half)
            r1 = r1 + half_of_product(w, (_Float16)e[idx].y);
        }
        out2[0] = (float)r0;
        out2[1] = (float)r1;
    } else {
        float r0 = 0.f, r1 = 0.f;
#pragma unroll
        for (int idx = 0; idx < 4; idx++) {
            const float w = (1 * w0[idx & 1]) * w1[idx >> 1];
            r0 = fmaf(w, e[idx].x, r0);   // results[ch] += w * grid[index + ch], contracted as nvcc contracts it (pn_grid_op.hip does the same)
            r1 = fmaf(w, e[idx].y, r1);
        }
        out2[0] = r0;
        out2[1] = r1;
    }
}

// the blend of renderer.py:288 / :896 for one channel: two roundings
__device__ __forceinline__ float bg_blend(float image, float one_minus_ws, float rgb) {
#pragma clang fp contract(off)
    const float t = one_minus_ws * rgb;
    return image + t;
}

template <bool HALF>
__global__ void __launch_bounds__(PN_BG_WAVES * 64) k_background(const unsigned char* __restrict__ img, const float2* __restrict__ emb, PnBgLevels lv,
                                                                const float* __restrict__ rays_o, const float* __restrict__ rays_d, uint32_t N, float radius,
                                                                float* __restrict__ rgb_out, const float* __restrict__ weights_sum,
                                                                float* __restrict__ image, float* __restrict__ coords_out,
                                                                const float* __restrict__ coords_in) {
    constexpr int IMG_BYTES = HALF ? PN_BG_H_BYTES : PN_BG_X_BYTES;
    constexpr int W_BYTES = HALF ? PN_BG_H_W_BYTES : PN_BG_X_W_BYTES;
    __shared__ __attribute__((aligned(16))) uint4 wimg[IMG_BYTES / 16];
    const uint32_t n_chunks = (N + 63) / 64;
    if (blockIdx.x * PN_BG_WAVES >= n_chunks) return;   // no chunk for any wave of this block (uniform: before the barrier)
    {
        const uint4* __restrict__ src = reinterpret_cast<const uint4*>(img + (HALF ? PN_BG_X_BYTES : 0));
        for (int i = threadIdx.x; i < IMG_BYTES / 16; i += PN_BG_WAVES * 64) wimg[i] = src[i];
    }
    __syncthreads();
    const float sf = reinterpret_cast<const float*>(img + PN_BG_X_BYTES + PN_BG_H_BYTES)[2];
    const int lane = threadIdx.x & 63;
    const int col = lane & 31, half = lane >> 5;
    const uint4* __restrict__ wl = wimg + lane;
    const float* __restrict__ wlast = reinterpret_cast<const float*>(wimg) + W_BYTES / 4 + half * 96;
    // this lane half's two levels: wave-uniform records (scalar registers), one select per constant
    const PnBgLevel A0 = lv.l[0], A1 = lv.l[1], B0 = lv.l[2], B1 = lv.l[3];
    const float sc[2] = {half ? B0.scale : A0.scale, half ? B1.scale : A1.scale};
    const uint32_t off[2] = {half ? B0.offset : A0.offset, half ? B1.offset : A1.offset};
    const uint32_t str[2] = {half ? B0.stride : A0.stride, half ? B1.stride : A1.stride};
    const uint32_t msk[2] = {half ? B0.mask : A0.mask, half ? B1.mask : A1.mask};
    const bool hsh[2] = {(half ? B0.hashed : A0.hashed) != 0, (half ? B1.hashed : A1.hashed) != 0};
    const uint32_t waves_total = gridDim.x * PN_BG_WAVES;

    for (uint32_t chunk = blockIdx.x * PN_BG_WAVES + (threadIdx.x >> 6); chunk < n_chunks; chunk += waves_total) {
#pragma unroll 1
        for (int t = 0; t < 2; t++) {
            const uint32_t ray = chunk * 64 + t * 32 + col;
            const bool valid = ray < N;
            float ox = 0.f, oy = 0.f, oz = 0.f, dx = 0.f, dy = 0.f, dz = 1.f;
            if (valid) {
                if (!coords_in) { ox = rays_o[ray * 3]; oy = rays_o[ray * 3 + 1]; oz = rays_o[ray * 3 + 2]; }
                dx = rays_d[ray * 3]; dy = rays_d[ray * 3 + 1]; dz = rays_d[ray * 3 + 2];
            }
            float cu = 0.f, cv = 0.f;
            if (coords_in) {   // NeRFNetwork.background(x, d) on coordinates the caller already has (kernel-uniform)
                if (valid) { cu = coords_in[ray * 2]; cv = coords_in[ray * 2 + 1]; }
            } else {
                pn_sph_coords(ox, oy, oz, dx, dy, dz, radius, cu, cv);
            }
            if (coords_out && valid && half == 0) { coords_out[ray * 2] = cu; coords_out[ray * 2 + 1] = cv; }
            // GridEncoder.forward with the default bound 1: (x + 1) / 2 (gridencoder/grid.py:149); out of [0, 1] -> zero features (gridencoder.cu:113-118).
            // A NaN coordinate (the ray never meets the sphere) is not "out of range" there and poisons the features; it does so here, but never an address.
            const float u0 = (cu + 1.0f) * 0.5f, u1 = (cv + 1.0f) * 0.5f;
            const bool inside = (u0 >= 0 && u0 <= 1 && u1 >= 0 && u1 <= 1);
            const bool isnan_in = (u0 != u0) || (u1 != u1);
            const float s0 = inside ? u0 : 0.f, s1 = inside ? u1 : 0.f;
            float feat[4];
            bg_encode_level<HALF>(sc[0], off[0], str[0], msk[0], hsh[0], emb, s0, s1, feat);
            bg_encode_level<HALF>(sc[1], off[1], str[1], msk[1], hsh[1], emb, s0, s1, feat + 2);
#pragma unroll
            for (int i = 0; i < 4; i++) feat[i] = inside ? feat[i] : (isnan_in ? __builtin_nanf("") : 0.f);
            float sh[16];
            sh16(dx, dy, dz, sh);
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {   // (an opaque copy keeps each select one v_cndmask: pn_net_tile.h, tile_color_net)
                float a = sh[k + 8], b = sh[k];
                asm volatile("" : "+v"(a), "+v"(b));
                v[k] = half ? a : b;
            }
            __builtin_amdgcn_sched_barrier(0);
            float e[3] = {0.f, 0.f, 0.f};
            if (HALF) {
                auto W = [&](int G) { return __builtin_bit_cast(f16x8, wl[G * 64]); };
                f16x8 b0, b1;
#pragma unroll
                for (int k = 0; k < 8; k++) b0[k] = (_Float16)v[k];
#pragma unroll
                for (int k = 0; k < 8; k++) b1[k] = k < 4 ? (_Float16)feat[k] : (_Float16)0.0f;
                f32x16 a0 = zero16(), a1 = zero16();
                a0 = PN_HMFMA(W(0), b0, a0);
                a0 = PN_HMFMA(W(1), b1, a0);
                a1 = PN_HMFMA(W(2), b0, a1);
                a1 = PN_HMFMA(W(3), b1, a1);
#pragma unroll
                for (int q = 0; q < 32; q++) {
                    const _Float16 h = (_Float16)(q < 16 ? a0[q] : a1[q - 16]);          // the Linear's half output
                    const float hv = (float)(h > (_Float16)0.0f ? h : (_Float16)0.0f);  // ReLU
#pragma unroll
                    for (int o = 0; o < 3; o++) e[o] = fmaf(wlast[q * 3 + o], hv, e[o]);
                }
            } else {
                const Split8x b0 = split8x(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], PN_BG_SH_SCALE);
                const Split8x b1 = split8x(feat[0], feat[1], feat[2], feat[3], 0.f, 0.f, 0.f, 0.f, sf);
                f32x16 a0 = {0}, a1 = {0};
                a0 = split_mac_x(wl, 0, b0, a0);
                a0 = split_mac_x(wl, 1, b1, a0);
                a1 = split_mac_x(wl, 2, b0, a1);
                a1 = split_mac_x(wl, 3, b1, a1);
                a0 = relu16(a0);
                a1 = relu16(a1);
#pragma unroll
                for (int q = 0; q < 32; q++) {
                    const float hv = q < 16 ? a0[q] : a1[q - 16];
#pragma unroll
                    for (int o = 0; o < 3; o++) e[o] = fmaf(wlast[q * 3 + o], hv, e[o]);
                }
            }
#pragma unroll
            for (int o = 0; o < 3; o++) e[o] += __shfl_xor(e[o], 32);   // the other 32 hidden units live in the partner lane
            if (valid && half == 0) {
                float rgb[3];
#pragma unroll
                for (int o = 0; o < 3; o++) rgb[o] = HALF ? tile_rgb_out_h(e[o]) : tile_rgb_out(e[o]);
                if (image) {
                    const float omw = 1 - weights_sum[ray];
#pragma unroll
                    for (int o = 0; o < 3; o++) image[ray * 3 + o] = bg_blend(image[ray * 3 + o], omw, rgb[o]);
                } else {
#pragma unroll
                    for (int o = 0; o < 3; o++) rgb_out[ray * 3 + o] = rgb[o];
                }
            }
        }
    }
}

// power of two that puts `bound` into (2^13, 2^14]; 1 when there is none to choose
double bg_scale_for(double bound) {
    if (!(bound > 0.0) || !std::isfinite(bound)) return 1.0;
    const int k = (int)floor(log2(16384.0 / bound));
    if (k < -100 || k > 100) return 1.0;
    return ldexp(1.0, k);
}

// `dst` <- the device image for W0 [64, 24] and W1 [3, 64] (row-major [out, in]) and the table's largest entry; returns the features' scale
float bg_build_images(const float* W0, const float* W1, float table_max, unsigned char* dst) {
    const double sf = bg_scale_for((double)table_max);
    double bb1 = 0.0;
    for (int i = 0; i < PN_BG_HIDDEN; i++) {
        double s = 0.0;
        for (int j = 0; j < PN_BG_IN; j++) s += fabs((double)W0[i * PN_BG_IN + j]) * (j < 16 ? 4.0 : (double)table_max);
        bb1 = std::max(bb1, s);
    }
    const double xs1 = bg_scale_for(bb1);
    // B-operand slot (K chunk kc, lane half h, element e) -> column of W0 (the network's input index), -1 = padding
    auto column = [](int kc, int h, int e) { return kc == 0 ? 8 * h + e : (e < 4 ? 16 + 4 * h + e : -1); };
    uint16_t* x16 = reinterpret_cast<uint16_t*>(dst);
    uint16_t* h16 = reinterpret_cast<uint16_t*>(dst + PN_BG_X_BYTES);
    for (int t = 0; t < 2; t++)
        for (int kc = 0; kc < 2; kc++) {
            const int G = t * 2 + kc;
            for (int l = 0; l < 64; l++)
                for (int e = 0; e < 8; e++) {
                    const int j = column(kc, l >> 5, e), row = t * 32 + (l & 31);
                    const float w = j < 0 ? 0.0f : W0[row * PN_BG_IN + j];
                    const float wx = j < 0 ? 0.0f : (float)((double)w * (xs1 / (j < 16 ? (double)PN_BG_SH_SCALE : sf)));
                    const uint16_t hi = pn_f2h_bits(wx);
                    x16[((size_t)(G * 2 + 0) * 64 + l) * 8 + e] = hi;
                    x16[((size_t)(G * 2 + 1) * 64 + l) * 8 + e] = pn_f2h_bits(wx - pn_h2f(hi));   // exact remainder (pn_nerf_forward.hip: build_weight_images)
                    h16[((size_t)G * 64 + l) * 8 + e] = pn_f2h_bits(w);
                }
        }
    // the vector-ALU Linear: wlast[h][q][o] = W1[o][row of D-layout register q = t * 16 + r of lane half h]
    float* wlast_x = reinterpret_cast<float*>(dst + PN_BG_X_W_BYTES);
    float* wlast_h = reinterpret_cast<float*>(dst + PN_BG_X_BYTES + PN_BG_H_W_BYTES);
    for (int h = 0; h < 2; h++)
        for (int q = 0; q < 32; q++)
            for (int o = 0; o < 3; o++) {
                const int t = q >> 4, r = q & 15;
                const float w = W1[o * PN_BG_HIDDEN + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * h];
                wlast_x[(h * 32 + q) * 3 + o] = (float)((double)w / xs1);
                wlast_h[(h * 32 + q) * 3 + o] = pn_h2f(pn_f2h_bits(w));
            }
    const float tail[4] = {0.0f, 0.0f, (float)sf, 0.0f};
    memcpy(dst + PN_BG_X_BYTES + PN_BG_H_BYTES, tail, sizeof(tail));
    return (float)sf;
}

// packs in pinned memory and uploads behind whatever `st` holds; one stream synchronisation (the table's abs-max), no allocation
int bg_upload(pn_bg_net* n, const float* W0, const float* W1, hipStream_t st) {
    unsigned* d_max = reinterpret_cast<unsigned*>(n->img + PN_BG_X_BYTES + PN_BG_H_BYTES);
    PN_HIP_CHECK(hipMemsetAsync(d_max, 0, 4, st));
    const int rc = pn_table_absmax_launch(n->embeddings, n->n_entries * 2u, d_max, st);
    if (rc) return rc;
    unsigned bits = 0;
    PN_HIP_CHECK(hipMemcpyAsync(&bits, d_max, 4, hipMemcpyDeviceToHost, st));
    PN_HIP_CHECK(hipStreamSynchronize(st));
    float table_max;
    memcpy(&table_max, &bits, 4);
    PN_HIP_CHECK(hipEventSynchronize(n->stage_done));   // the previous upload has finished reading the staging buffer
    n->sf = bg_build_images(W0, W1, table_max, n->stage);
    PN_HIP_CHECK(hipMemcpyAsync(n->img, n->stage, PN_BG_IMG_BYTES, hipMemcpyHostToDevice, st));
    PN_HIP_CHECK(hipEventRecord(n->stage_done, st));
    return PN_OK;
}

int bg_capturing(hipStream_t st, const char* who) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    PN_HIP_CHECK(hipStreamIsCapturing(st, &cs));
    if (cs != hipStreamCaptureStatusNone) {   // the packing runs on the host and reads host weights: it cannot be part of a captured graph
        snprintf(pn_err_buf, sizeof(pn_err_buf), "%s: called while the stream is being captured into a HIP graph; build / refresh the background weights before capture", who);
        return PN_ERR_ARG;
    }
    return PN_OK;
}

int bg_launch(const pn_bg_net* n, const float* rays_o, const float* rays_d, uint32_t N, float radius, float* rgb_out, const float* weights_sum, float* image,
              float* coords_out, const float* coords_in, bool half, hipStream_t st) {
    if (N == 0) return PN_OK;
    PN_REQUIRE(n && rays_d && (rays_o || coords_in));
    PN_REQUIRE((image != nullptr) == (weights_sum != nullptr));   // blend mode takes both
    PN_REQUIRE((image != nullptr) != (rgb_out != nullptr));       // one mode or the other
    PN_REQUIRE(N <= 0x7fffffffu / 3u);                            // ray * 3 + 2 in 32 bits
    const uint32_t blocks = std::min(pn_div_up(pn_div_up(N, 64), PN_BG_WAVES), 2048u);
    if (half)
        k_background<true><<<blocks, PN_BG_WAVES * 64, 0, st>>>(n->img, reinterpret_cast<const float2*>(n->embeddings), n->levels, rays_o, rays_d, N, radius, rgb_out,
                                                               weights_sum, image, coords_out, coords_in);
    else
        k_background<false><<<blocks, PN_BG_WAVES * 64, 0, st>>>(n->img, reinterpret_cast<const float2*>(n->embeddings), n->levels, rays_o, rays_d, N, radius, rgb_out,
                                                                weights_sum, image, coords_out, coords_in);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

}  // namespace

extern "C" int pn_bg_net_create(pn_bg_net** out, const float* embeddings, const int* offsets_host, uint32_t L, uint32_t C, float per_level_scale_log2,
                                uint32_t base_resolution, const float* W0_host, const float* W1_host, void* stream) {
    PN_REQUIRE(out && embeddings && offsets_host && W0_host && W1_host);
    PN_REQUIRE(L == PN_BG_LEVELS && C == 2);   // get_encoder(encoding_bg, input_dim=2, num_levels=4, ...), nerf/network.py:76
    hipStream_t st = (hipStream_t)stream;
    if (int rc = bg_capturing(st, "pn_bg_net_create")) return rc;
    PnBgLevels lv;
    for (uint32_t l = 0; l < L; l++) {
        const float scale = exp2f(l * per_level_scale_log2) * base_resolution - 1.0f;   // gridencoder.cu:133-134
        const uint32_t res = (uint32_t)ceilf(scale) + 1;
        PN_REQUIRE(offsets_host[l + 1] > offsets_host[l]);
        const uint32_t hs = (uint32_t)(offsets_host[l + 1] - offsets_host[l]), s1 = res + 1;
        const bool dense = (uint64_t)s1 * s1 <= hs;   // get_grid_index's stride loop for D = 2 (gridencoder.cu:65-84): both dimensions strided, index < s1^2 <= hs
        const bool hashed = !dense && s1 <= hs && (hs & (hs - 1)) == 0;
        if (!dense && !hashed) PN_REQUIRE(!"background level is neither fully dense nor hashed into a power-of-two table");
        lv.l[l] = PnBgLevel{scale, (uint32_t)offsets_host[l], s1, hashed ? hs - 1 : 0u, hashed ? 1u : 0u};
    }
    pn_bg_net* n = new pn_bg_net();
    memset(n, 0, sizeof(*n));
    n->levels = lv;
    n->embeddings = embeddings;
    n->n_entries = (uint32_t)offsets_host[L];
    hipError_t e = hipMalloc((void**)&n->img, PN_BG_IMG_BYTES);
    if (e == hipSuccess) e = hipHostMalloc((void**)&n->stage, PN_BG_IMG_BYTES);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&n->stage_done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(n->stage_done, st);
    if (e != hipSuccess) {
        snprintf(pn_err_buf, sizeof(pn_err_buf), "pn_bg_net_create: %s", hipGetErrorString(e));
        pn_bg_net_destroy(n);
        return PN_ERR_HIP;
    }
    if (int rc = bg_upload(n, W0_host, W1_host, st)) { pn_bg_net_destroy(n); return rc; }
    *out = n;
    return PN_OK;
}

extern "C" int pn_bg_net_update(pn_bg_net* n, const float* embeddings, const float* W0_host, const float* W1_host, void* stream) {
    PN_REQUIRE(n && embeddings && W0_host && W1_host);
    if (int rc = bg_capturing((hipStream_t)stream, "pn_bg_net_update")) return rc;
    n->embeddings = embeddings;
    return bg_upload(n, W0_host, W1_host, (hipStream_t)stream);
}

extern "C" void pn_bg_net_destroy(pn_bg_net* n) {
    if (!n) return;
    if (n->img) (void)hipFree(n->img);
    if (n->stage) (void)hipHostFree(n->stage);
    if (n->stage_done) (void)hipEventDestroy(n->stage_done);
    delete n;
}

extern "C" int pn_background_forward(const pn_bg_net* net, const float* rays_o, const float* rays_d, uint32_t N, float radius, float* rgb_out,
                                     const float* weights_sum, float* image, float* coords_out, void* stream) {
    return bg_launch(net, rays_o, rays_d, N, radius, rgb_out, weights_sum, image, coords_out, nullptr, false, (hipStream_t)stream);
}

extern "C" int pn_background_forward_half(const pn_bg_net* net, const float* rays_o, const float* rays_d, uint32_t N, float radius, float* rgb_out,
                                          const float* weights_sum, float* image, float* coords_out, void* stream) {
    return bg_launch(net, rays_o, rays_d, N, radius, rgb_out, weights_sum, image, coords_out, nullptr, true, (hipStream_t)stream);
}

extern "C" int pn_background_coords(const pn_bg_net* net, const float* coords, const float* dirs, uint32_t N, float* rgb_out, int half, void* stream) {
    PN_REQUIRE(coords && rgb_out);
    return bg_launch(net, nullptr, dirs, N, 0.0f, rgb_out, nullptr, nullptr, nullptr, coords, half != 0, (hipStream_t)stream);
}
