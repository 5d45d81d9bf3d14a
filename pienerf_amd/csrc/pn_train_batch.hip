// The data side of one training step (gfx950): which pixels a step trains on, their rays and their ground-truth colours, and the error map that
// steers the choice.  Built with -ffp-contract=off: the pixel index arithmetic restates separate torch ops (one rounding each) and the ray of a
// pixel is pn_ray_dir.h's, bit for bit what k_get_rays writes.  Reference citations are relative to /root/reference.
//
// Random numbers are inputs (drawn by torch on the device), so every kernel here is a pure function of its arguments.
#include "pn_ray_dir.h"

#define PN_SAMPLE_THREADS 1024
#define PN_SAMPLE_WAVES (PN_SAMPLE_THREADS / PN_WAVE)
#define PN_SAMPLE_PER 16                                        // keys per lane: cell 1024 k + thread, k < 16
#define PN_SAMPLE_MAX_CELLS (PN_SAMPLE_THREADS * PN_SAMPLE_PER)  // 16384 = 128 * 128, the error map's fixed resolution (provider.py:236)

// ------------------------------------------------------------------------------------------------ weighted sampling without replacement
// torch.multinomial(error_map, N, replacement=False) (nerf/utils.py:106) as exponential races: key_i = w_i / e_i with e_i ~ Exp(1); the N cells with
// the largest keys are a draw without replacement with probabilities proportional to w.  One workgroup; lane t holds the keys of cells 1024 k + t in
// registers (16 per lane, nothing to spill), LDS carries only per-wave counts.
//   1. Radix select, one key bit per pass from bit 30 down (positive floats order as unsigned integers): T = the largest value with
//      count(key >= T) >= N, i.e. the N-th largest key.  A pass counts with ballots + popcounts (no atomics) and costs one barrier.
//   2. Stable compaction: a cell is taken when key > T, or key == T and fewer than N - count(key > T) equal keys precede it (ties go to the lower
//      index).  The output slot is the number of taken cells before it — wave ballots inside a 64-cell run, an exclusive scan over the 256 runs — so
//      the cells come out in ascending index and two calls with equal inputs write equal bytes.
// A cell of weight zero has key 0 and is never taken: N > count(w > 0) sets *status = 1 and writes nothing else.  A positive weight whose quotient
// underflows to zero keeps the smallest positive key, so that it still counts as positive.
__global__ void __launch_bounds__(PN_SAMPLE_THREADS) k_sample_cells(const float* __restrict__ weights, const float* __restrict__ expo, int n_cells, int N,
                                                                    int64_t* __restrict__ cells_out, int* __restrict__ status) {
    __shared__ uint32_t s_cnt[2][PN_SAMPLE_WAVES];
    __shared__ uint32_t s_run[PN_SAMPLE_PER * PN_SAMPLE_WAVES];  // per 64-cell run: taken-for-sure count | equal count << 16, then their exclusive scan
    const int t = threadIdx.x, wave = t / PN_WAVE, lane = t % PN_WAVE;
    uint32_t key[PN_SAMPLE_PER];
    uint32_t pos = 0;
#pragma unroll
    for (int k = 0; k < PN_SAMPLE_PER; k++) {
        const int i = k * PN_SAMPLE_THREADS + t;
        uint32_t b = 0;
        if (i < n_cells) {
            const float w = weights[i];
            if (w > 0.0f) {
                b = __float_as_uint(w / expo[i]);  // IEEE division (-fhip-fp32-correctly-rounded-divide-sqrt)
                if (b == 0) b = 1;
            }
        }
        key[k] = b;
        pos += (uint32_t)__popcll(__ballot(b != 0));
    }
    if (lane == 0) s_cnt[0][wave] = pos;
    __syncthreads();
    uint32_t positive = 0;
#pragma unroll
    for (int w = 0; w < PN_SAMPLE_WAVES; w++) positive += s_cnt[0][w];
    if ((uint32_t)N > positive) {  // uniform: every lane read the same sum
        if (t == 0) *status = 1;
        return;
    }
    // 1. the N-th largest key
    uint32_t T = 0;
    for (int bit = 30; bit >= 0; bit--) {
        const uint32_t cand = T | (1u << bit);
        uint32_t c = 0;
#pragma unroll
        for (int k = 0; k < PN_SAMPLE_PER; k++) c += (uint32_t)__popcll(__ballot(key[k] >= cand));
        uint32_t* cnt = s_cnt[(bit + 1) & 1];  // the buffers alternate: a wave one pass ahead writes the other one
        if (lane == 0) cnt[wave] = c;
        __syncthreads();
        uint32_t total = 0;
#pragma unroll
        for (int w = 0; w < PN_SAMPLE_WAVES; w++) total += cnt[w];
        if (total >= (uint32_t)N) T = cand;
    }
    // 2. stable compaction
    const uint64_t below = (1ull << lane) - 1ull;
#pragma unroll
    for (int k = 0; k < PN_SAMPLE_PER; k++) {
        const uint32_t g = (uint32_t)__popcll(__ballot(key[k] > T)), e = (uint32_t)__popcll(__ballot(key[k] == T));
        if (lane == 0) s_run[k * PN_SAMPLE_WAVES + wave] = g | (e << 16);  // run r = 16 k + wave covers cells [64 r, 64 r + 64)
    }
    __syncthreads();
    if (wave == 0) {  // exclusive scan over the 256 runs: 4 per lane, then across the wave
        uint32_t v[4], sum = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            v[j] = s_run[lane * 4 + j];
            sum += v[j];
        }
        uint32_t incl = sum;
#pragma unroll
        for (int d = 1; d < PN_WAVE; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        uint32_t run = incl - sum;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            s_run[lane * 4 + j] = run;
            run += v[j];
        }
        if (lane == PN_WAVE - 1) s_cnt[0][0] = incl & 0xffffu;  // count(key > T); the select loop's last pass (bit 0) used s_cnt[1]
    }
    __syncthreads();
    const uint32_t take_equal = (uint32_t)N - s_cnt[0][0];  // >= 1: count(key >= T) >= N > count(key > T)
#pragma unroll
    for (int k = 0; k < PN_SAMPLE_PER; k++) {
        const uint64_t bg = __ballot(key[k] > T), be = __ballot(key[k] == T);
        const uint32_t base = s_run[k * PN_SAMPLE_WAVES + wave];
        const uint32_t g_before = (base & 0xffffu) + (uint32_t)__popcll(bg & below), e_before = (base >> 16) + (uint32_t)__popcll(be & below);
        const bool taken = key[k] > T || (key[k] == T && e_before < take_equal);
        const uint32_t slot = g_before + min(e_before, take_equal);
        if (taken && slot < (uint32_t)N) cells_out[slot] = (int64_t)(k * PN_SAMPLE_THREADS + t);
    }
    if (t == 0) *status = 0;
}

extern "C" int pn_sample_cells(const float* weights, const float* expo, int n_cells, int N, int64_t* cells_out, int* status, void* stream) {
    PN_REQUIRE(weights && expo && cells_out && status);
    PN_REQUIRE(n_cells > 0 && n_cells <= PN_SAMPLE_MAX_CELLS && N > 0 && N <= n_cells);
    k_sample_cells<<<1, PN_SAMPLE_THREADS, 0, (hipStream_t)stream>>>(weights, expo, n_cells, N, cells_out, status);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

// ------------------------------------------------------------------------------------------------ the rays and colours of one training step
// nerf/utils.py:77-136 for one pose, nerf/provider.py:311-316 (the gather of the ground truth).  One lane per ray.
//   mode 0 (:101)      a = the pixel indices as drawn
//   mode 1 (:106-115)  a = coarse cells (128 x 128), u = [2, N] uniforms: row = min(int64(float(cell / 128) * sx + u0 * sx), H - 1), sx = H / 128 (the
//                      reference's inds_x runs along H), column likewise with cell % 128, sy = W / 128 and u1; products and sum rounded one by one
//   mode 2 (:81-98)    a, b = top-left rows / columns of the patches; ray n is pixel (n % patch^2 / patch, n % patch) of patch n / patch^2
// An index outside the image (only possible with draws handed in from outside) reads nothing: its ray is NaN and its colour zero.
__global__ void __launch_bounds__(256) k_train_batch(const float* __restrict__ pose, float fx, float fy, float cx, float cy, int H, int W, int N, int mode,
                                                     const int64_t* __restrict__ a, const int64_t* __restrict__ b, const float* __restrict__ u, int patch,
                                                     const float* __restrict__ image, int C, int64_t* __restrict__ inds_out, float* __restrict__ rays_o,
                                                     float* __restrict__ rays_d, float* __restrict__ pixels_out) {
    const int n = threadIdx.x + blockIdx.x * blockDim.x;
    if (n >= N) return;
    int64_t row, col;
    if (mode == 0) {
        const int64_t ind = a[n];
        row = ind >= 0 ? ind / W : -1;
        col = ind >= 0 ? ind % W : -1;
    } else if (mode == 1) {
        const int64_t cell = a[n];
        const float sx = (float)H / 128.0f, sy = (float)W / 128.0f;  // exact: a division by a power of two
        const float rx = (float)(cell / 128) * sx, ry = (float)(cell % 128) * sy;
        const float jx = u[n] * sx, jy = u[N + n] * sy;
        row = (int64_t)(rx + jx);
        col = (int64_t)(ry + jy);
        if (row > H - 1) row = H - 1;
        if (col > W - 1) col = W - 1;
    } else {
        const int pp = patch * patch, p = n / pp, r = n % pp;
        row = a[p] + r / patch;
        col = b[p] + r % patch;
    }
    const int64_t ind = row * W + col;  // the reference's flattening (a corner outside the image keeps its wrapped index there; here it is refused)
    inds_out[n] = ind;
    const bool inside = row >= 0 && row < H && col >= 0 && col < W;
    if (inside) {
        pn_pixel_ray(pose, fx, fy, cx, cy, (int)col, (int)row, rays_o + (size_t)n * 3, rays_d + (size_t)n * 3);
    } else {
        const float nan = __uint_as_float(0x7fc00000u);
        for (int c = 0; c < 3; c++) rays_o[(size_t)n * 3 + c] = rays_d[(size_t)n * 3 + c] = nan;
    }
    if (pixels_out) {
        for (int c = 0; c < C; c++) pixels_out[(size_t)n * C + c] = inside ? image[(size_t)ind * C + c] : 0.0f;
    }
}

extern "C" int pn_train_batch(const float* pose, float fx, float fy, float cx, float cy, int H, int W, int N, int mode, const int64_t* a, const int64_t* b,
                              const float* u, int patch, const float* image, int C, int64_t* inds_out, float* rays_o, float* rays_d, float* pixels_out,
                              void* stream) {
    PN_REQUIRE(pose && a && inds_out && rays_o && rays_d && H > 0 && W > 0 && N > 0 && (int64_t)H * W < (1ll << 31));
    PN_REQUIRE(mode == 0 || (mode == 1 && u) || (mode == 2 && b && patch > 1 && N % (patch * patch) == 0));
    PN_REQUIRE((image == nullptr) == (pixels_out == nullptr) && (!image || C == 3 || C == 4));
    k_train_batch<<<pn_div_up(N, 256), 256, 0, (hipStream_t)stream>>>(pose, fx, fy, cx, cy, H, W, N, mode, a, b, u, patch, image, C, inds_out, rays_o, rays_d,
                                                                     pixels_out);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

// ------------------------------------------------------------------------------------------------ error map
// nerf/trainer.py:239-243: ema_error = 0.1 * error_map.gather(1, inds) + 0.9 * error, scattered back.  The cells of a batch are distinct (drawn without
// replacement), so the order of the lanes is free.  Two products and one sum, each rounded.
__global__ void __launch_bounds__(256) k_error_map_update(float* __restrict__ map_row, const int64_t* __restrict__ cells, const float* __restrict__ err, int N) {
    const int n = threadIdx.x + blockIdx.x * blockDim.x;
    if (n >= N) return;
    const int64_t c = cells[n];
    if (c < 0 || c >= PN_SAMPLE_MAX_CELLS) return;  // a row has 128 * 128 cells
    const float kept = 0.1f * map_row[c], fresh = 0.9f * err[n];
    map_row[c] = kept + fresh;
}

extern "C" int pn_error_map_update(float* map_row, const int64_t* cells, const float* err, int N, void* stream) {
    PN_REQUIRE(map_row && cells && err && N > 0);
    k_error_map_update<<<pn_div_up(N, 256), 256, 0, (hipStream_t)stream>>>(map_row, cells, err, N);
    PN_LAUNCH_CHECK();
    return PN_OK;
}
