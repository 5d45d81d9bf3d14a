// Spatial hash of the integration points (get_pnts_in_grids, nerf/utils.py:360-443) and the exclusive scans over its cells: kernels and their launchers.
// Part of the render unit (included by pn_render_ops.hip only).
#pragma once
#include "pn_common.h"

// ------------------------------------------------------------------------------------------------ spatial hash of IPs
// p2g, nerf/utils.py:389-407
__device__ __forceinline__ int p2g(const float* __restrict__ p, const float* __restrict__ bbmin, float hgs, const int* __restrict__ res, int n_grid) {
    const int g0 = (int)floorf((p[0] - bbmin[0]) / hgs);
    const int g1 = (int)floorf((p[1] - bbmin[1]) / hgs);
    const int g2 = (int)floorf((p[2] - bbmin[2]) / hgs);
    const int gid = g2 * res[1] * res[0] + g1 * res[0] + g0;
    return (gid < 0 || gid >= n_grid) ? -1 : gid;
}

__global__ void __launch_bounds__(256) k_pig_zero(int* __restrict__ cnt, int n_grid_max, const int* __restrict__ n_grid_dev) {
    const int n_grid = n_grid_dev ? min(*n_grid_dev, n_grid_max) : n_grid_max;
    for (int g = threadIdx.x + blockIdx.x * blockDim.x; g < n_grid; g += gridDim.x * blockDim.x) cnt[g] = 0;
}

// get_pig_cnt, nerf/utils.py:410-424
__global__ void __launch_bounds__(256) k_pig_count(int n_vtx, int n_grid_max, const int* __restrict__ n_grid_dev, const float* __restrict__ pnts,
                                                   const float* __restrict__ bbmin, float hgs, const int* __restrict__ res, int* cnt,
                                                   int* err_flag) {
    const int p = threadIdx.x + blockIdx.x * blockDim.x;
    if (p >= n_vtx) return;
    const int n_grid = n_grid_dev ? min(*n_grid_dev, n_grid_max) : n_grid_max;
    const int gid = p2g(pnts + p * 3, bbmin, hgs, res, n_grid);
    if (gid >= 0) atomicAdd(cnt + gid, 1);
    else if (err_flag) atomicOr(err_flag, 2);
}

// pig_bgn = cumsum(cnt) - cnt (nerf/utils.py:369), one workgroup of 1024 threads, 16 cells per thread per tile (16 384 cells per round: a 300 k-cell
// grid — --cut with bound 2 — is 19 rounds of one barrier each; with 4 cells per thread and three barriers per round it was 74 rounds, 0.23 ms per scan).
// The running carry lives in a register of every thread (each adds the same 16 wave totals), the wave totals alternate between two LDS rows.
__device__ __forceinline__ void block_scan_1024(int n_grid, const int* __restrict__ cnt, int* __restrict__ bgn, int* __restrict__ cursor) {
    __shared__ int wsum[2][16];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int carry = 0, buf = 0;
    for (int base = 0; base < n_grid; base += 16384, buf ^= 1) {
        const int i0 = base + threadIdx.x * 16;
        int v[16];
        if (i0 + 16 <= n_grid) {  // (cnt + i0 is 64-byte aligned: the tables come from hipMalloc and i0 is a multiple of 16)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int4 w = *reinterpret_cast<const int4*>(cnt + i0 + 4 * q);
                v[4 * q] = w.x; v[4 * q + 1] = w.y; v[4 * q + 2] = w.z; v[4 * q + 3] = w.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 16; k++) v[k] = (i0 + k < n_grid) ? cnt[i0 + k] : 0;
        }
        int tsum = 0;
#pragma unroll
        for (int k = 0; k < 16; k++) tsum += v[k];
        int inc = tsum;  // inclusive wave scan
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(inc, o);
            if (lane >= o) inc += u;
        }
        if (lane == 63) wsum[buf][wid] = inc;
        __syncthreads();
        int woff = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 16; w++) {
            const int x = wsum[buf][w];
            woff += (w < wid) ? x : 0;
            total += x;
        }
        int run = carry + woff + inc - tsum;
        if (i0 + 16 <= n_grid) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                int4 o4;
                o4.x = run; run += v[4 * q];
                o4.y = run; run += v[4 * q + 1];
                o4.z = run; run += v[4 * q + 2];
                o4.w = run; run += v[4 * q + 3];
                *reinterpret_cast<int4*>(bgn + i0 + 4 * q) = o4;
                *reinterpret_cast<int4*>(cursor + i0 + 4 * q) = o4;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 16; k++) {
                if (i0 + k < n_grid) { bgn[i0 + k] = run; cursor[i0 + k] = run; }
                run += v[k];
            }
        }
        carry += total;
    }
}
__global__ void __launch_bounds__(1024) k_pig_scan(int n_grid_max, const int* __restrict__ n_grid_dev, const int* __restrict__ cnt,
                                                   int* __restrict__ bgn, int* __restrict__ cursor) {
    const int n_grid = n_grid_dev ? min(*n_grid_dev, n_grid_max) : n_grid_max;
    block_scan_1024(n_grid, cnt, bgn, cursor);
}

// Large grids (--cut with bound 2: 300 k cells): the same exclusive scan in three launches over 4096-cell tiles — tile sums, one
// workgroup scanning the <= 1024 tile sums, per-tile scan + offset.  The tile's sum / offset travels in bgn[first cell of the tile],
// so no scratch buffer is needed.  (One workgroup walking 74 tiles one after the other took 0.23-0.30 ms per scan.)
__device__ __forceinline__ int block_sum_1024(int v, int* wsum) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0) wsum[wid] = v;
    __syncthreads();
    int total = 0;
    for (int w = 0; w < 16; w++) total += wsum[w];
    __syncthreads();
    return total;
}
__global__ void __launch_bounds__(1024) k_scan_tile_sum(int n_grid_max, const int* __restrict__ n_grid_dev, const int* __restrict__ cnt,
                                                        int* __restrict__ bgn) {
    __shared__ int wsum[16];
    const int n_grid = n_grid_dev ? min(*n_grid_dev, n_grid_max) : n_grid_max;
    const int base = (int)blockIdx.x * 4096;
    if (base >= n_grid) return;
    const int i0 = base + threadIdx.x * 4;
    int v = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) v += (i0 + k < n_grid) ? __hip_atomic_load(cnt + i0 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
    const int total = block_sum_1024(v, wsum);
    if (threadIdx.x == 0) bgn[base] = total;
}
__global__ void __launch_bounds__(1024) k_scan_tile_offsets(int n_grid_max, const int* __restrict__ n_grid_dev, int* __restrict__ bgn) {
    __shared__ int wsum[16];
    const int n_grid = n_grid_dev ? min(*n_grid_dev, n_grid_max) : n_grid_max;
    const int n_tiles = (n_grid + 4095) / 4096;  // <= 1024 (checked by the launcher)
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
    const int v = t < n_tiles ? __hip_atomic_load(bgn + (size_t)t * 4096, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    if (lane == 63) wsum[wid] = inc;
    __syncthreads();
    int woff = 0;
    for (int w = 0; w < wid; w++) woff += wsum[w];
    if (t < n_tiles) bgn[(size_t)t * 4096] = woff + inc - v;
}
__global__ void __launch_bounds__(1024) k_scan_tile_apply(int n_grid_max, const int* __restrict__ n_grid_dev, const int* __restrict__ cnt,
                                                          int* __restrict__ bgn, int* __restrict__ cursor) {
    __shared__ int wsum[16];
    __shared__ int off_s;
    const int n_grid = n_grid_dev ? min(*n_grid_dev, n_grid_max) : n_grid_max;
    const int base = (int)blockIdx.x * 4096;
    if (base >= n_grid) return;
    if (threadIdx.x == 0) off_s = __hip_atomic_load(bgn + base, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int i0 = base + threadIdx.x * 4;
    int v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = (i0 + k < n_grid) ? __hip_atomic_load(cnt + i0 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
    const int tsum = v[0] + v[1] + v[2] + v[3];
    int inc = tsum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    if (lane == 63) wsum[wid] = inc;
    __syncthreads();  // also orders thread 0's read of the tile offset before any write to bgn[base]
    int woff = 0;
    for (int w = 0; w < wid; w++) woff += wsum[w];
    int run = off_s + woff + inc - tsum;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (i0 + k < n_grid) { bgn[i0 + k] = run; cursor[i0 + k] = run; }
        run += v[k];
    }
}
// exclusive scan cnt -> bgn, cursor over up to n_grid_max cells (the live count may come from device memory)
static void launch_cell_scan(int n_grid_max, const int* n_grid_dev, const int* cnt, int* bgn, int* cursor, hipStream_t st) {
    const int tiles = (int)pn_div_up(n_grid_max, 4096);
    // the tiled form (three launches) over the one-workgroup scan on the trex option set (300 k cells): 1 464 -> 1 535 steps/s (profiles/r04_trex_scan.txt)
    if (tiles <= 16 || tiles > 1024) {  // small grids: one workgroup is faster than three launches
        k_pig_scan<<<1, 1024, 0, st>>>(n_grid_max, n_grid_dev, cnt, bgn, cursor);
        return;
    }
    k_scan_tile_sum<<<tiles, 1024, 0, st>>>(n_grid_max, n_grid_dev, cnt, bgn);
    k_scan_tile_offsets<<<1, 1024, 0, st>>>(n_grid_max, n_grid_dev, bgn);
    k_scan_tile_apply<<<tiles, 1024, 0, st>>>(n_grid_max, n_grid_dev, cnt, bgn, cursor);
}

// get_pig_idx, nerf/utils.py:427-443 — slots claimed through a per-cell cursor ...
__global__ void __launch_bounds__(256) k_pig_fill(int n_vtx, int n_grid_max, const int* __restrict__ n_grid_dev, const float* __restrict__ pnts,
                                                  const float* __restrict__ bbmin, float hgs, const int* __restrict__ res, int* cursor,
                                                  int* __restrict__ idx) {
    const int p = threadIdx.x + blockIdx.x * blockDim.x;
    if (p >= n_vtx) return;
    const int n_grid = n_grid_dev ? min(*n_grid_dev, n_grid_max) : n_grid_max;
    const int gid = p2g(pnts + p * 3, bbmin, hgs, res, n_grid);
    if (gid >= 0) idx[atomicAdd(cursor + gid, 1)] = p;
}
// ... then each cell's few entries are put in ascending point id, which makes the table independent of atomic order.
__global__ void __launch_bounds__(256) k_pig_sort(int n_grid_max, const int* __restrict__ n_grid_dev, const int* __restrict__ cnt,
                                                  const int* __restrict__ bgn, int* __restrict__ idx) {
    const int n_grid = n_grid_dev ? min(*n_grid_dev, n_grid_max) : n_grid_max;
    for (int g = threadIdx.x + blockIdx.x * blockDim.x; g < n_grid; g += gridDim.x * blockDim.x) {
        const int c = __hip_atomic_load(cnt + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c < 2) continue;
        int* a = idx + bgn[g];
        for (int i = 1; i < c; i++) {
            const int v = __hip_atomic_load(a + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            int j = i - 1;
            while (j >= 0) {
                const int u = __hip_atomic_load(a + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (u <= v) break;
                __hip_atomic_store(a + j + 1, u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                j--;
            }
            __hip_atomic_store(a + j + 1, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

static int pig_build(int n_vtx, int n_grid_max, const int* n_grid_dev, const float* pnts, const float* bbmin, float hgs, const int* res, int* cnt,
                     int* bgn, int* idx, int* cursor, int* err_flag, hipStream_t st) {
    const int gz = (int)pn_div_up(n_grid_max, 256) < 1024 ? (int)pn_div_up(n_grid_max, 256) : 1024;
    k_pig_zero<<<gz, 256, 0, st>>>(cnt, n_grid_max, n_grid_dev);
    k_pig_count<<<pn_div_up(n_vtx, 256), 256, 0, st>>>(n_vtx, n_grid_max, n_grid_dev, pnts, bbmin, hgs, res, cnt, err_flag);
    launch_cell_scan(n_grid_max, n_grid_dev, cnt, bgn, cursor, st);
    k_pig_fill<<<pn_div_up(n_vtx, 256), 256, 0, st>>>(n_vtx, n_grid_max, n_grid_dev, pnts, bbmin, hgs, res, cursor, idx);
    k_pig_sort<<<gz, 256, 0, st>>>(n_grid_max, n_grid_dev, cnt, bgn, idx);
    PN_LAUNCH_CHECK();
    return PN_OK;
}
