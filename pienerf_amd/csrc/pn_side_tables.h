// Side tables of the cooperative march, op-level build (count -> scan -> fill + packed IP records): kernels and their launcher.
// Part of the render unit (included by pn_render_ops.hip only); the frame driver builds the same tables in k_frame_prologue (pn_frame_kernels.h).
#pragma once
#include "pn_cell_hash.h"
#include "pn_march_tables.h"
#include "pn_render_records.h"

// ------------------------------------------------------------------------------------------------ march
// Side tables of the cooperative march (pn_march_tables.h): per-cell candidate lists and packed IP records.
__device__ __forceinline__ void nb_cell_coords(int c, int r0, int r1, int& g0, int& g1, int& g2) {
    g0 = c % r0;
    g1 = (c / r0) % r1;
    g2 = c / (r0 * r1);
}
// neighbour k of cell (g0,g1,g2) in the visiting order of find_closest_IPs (offset applied as (g0+a, g1+b, g2+c), raymarching.cu:1095-1102)
// or, for num_seek_IP == 1, of find_closest_IP (offset applied as (g2+a, g1+b, g0+c), :1018-1025).  Returns -1 when out of the grid.
__device__ __forceinline__ int nb_neighbour(int k, int swap, int g0, int g1, int g2, int r0, int r1, int r2) {
    const int a = pnm::NBR26[k][0], b = pnm::NBR26[k][1], c = pnm::NBR26[k][2];
    const int n0 = g0 + (swap ? c : a), n1 = g1 + b, n2 = g2 + (swap ? a : c);
    if (n0 < 0 || n0 >= r0 || n1 < 0 || n1 >= r1 || n2 < 0 || n2 >= r2) return -1;
    return n2 * r1 * r0 + n1 * r0 + n0;
}

__global__ void __launch_bounds__(256) k_nb_count(int n_grid_max, const int* __restrict__ n_grid_dev, const int* __restrict__ res,
                                                  const int* __restrict__ pig_cnt, int swap, int* __restrict__ nb_cnt) {
    const int n_grid = n_grid_dev ? min(*n_grid_dev, n_grid_max) : n_grid_max;
    const int r0 = res[0], r1 = res[1], r2 = res[2];
    for (int c = threadIdx.x + blockIdx.x * blockDim.x; c < n_grid; c += gridDim.x * blockDim.x) {
        int g0, g1, g2;
        nb_cell_coords(c, r0, r1, g0, g1, g2);
        int s = pig_cnt[c];
        for (int k = 0; k < 26; k++) {
            const int nbc = nb_neighbour(k, swap, g0, g1, g2, r0, r1, r2);
            if (nbc >= 0) s += pig_cnt[nbc];
        }
        nb_cnt[c] = s;
    }
}

__global__ void __launch_bounds__(256) k_nb_fill(int n_grid_max, const int* __restrict__ n_grid_dev, const int* __restrict__ res,
                                                 const int* __restrict__ pig_cnt, const int* __restrict__ pig_bgn, const int* __restrict__ pig_idx,
                                                 const float* __restrict__ p_def, int swap, const int* __restrict__ nb_cnt, const int* __restrict__ nb_bgn,
                                                 float4* __restrict__ nb, int nb_capacity, int* err_flag, int2* __restrict__ nb_rng) {
    const int n_grid = n_grid_dev ? min(*n_grid_dev, n_grid_max) : n_grid_max;
    const int r0 = res[0], r1 = res[1], r2 = res[2];
    for (int c = threadIdx.x + blockIdx.x * blockDim.x; c < n_grid; c += gridDim.x * blockDim.x) {
        int w = nb_bgn[c];
        const bool fits = w + nb_cnt[c] <= nb_capacity;
        nb_rng[c] = fits ? make_int2(w, w + nb_cnt[c]) : make_int2(0, 0);
        if (nb_cnt[c] == 0) continue;
        if (!fits) { if (err_flag) atomicOr(err_flag, 8); continue; }
        int g0, g1, g2;
        nb_cell_coords(c, r0, r1, g0, g1, g2);
        for (int k = -1; k < 26; k++) {
            const int cell = (k < 0) ? c : nb_neighbour(k, swap, g0, g1, g2, r0, r1, r2);
            if (cell < 0) continue;
            const int n = pig_cnt[cell], b = pig_bgn[cell];
            for (int i = 0; i < n; i++) {
                const int ip = pig_idx[b + i];
                nb[w++] = make_float4(p_def[ip * 3], p_def[ip * 3 + 1], p_def[ip * 3 + 2], __int_as_float(ip));
            }
        }
    }
}

// rec[ip]: see pn_march_tables.h (pack_ip_float)
__global__ void __launch_bounds__(256) k_pack_ip(int n_vtx, const float* __restrict__ p_ori, const float* __restrict__ p_def,
                                                 const float* __restrict__ F_IP, const float* __restrict__ dF_IP, float* __restrict__ rec) {
    const int t = threadIdx.x + blockIdx.x * blockDim.x;
    const int ip = t / PN_REC_FLOATS, j = t % PN_REC_FLOATS;
    if (ip >= n_vtx) return;
    rec[t] = pnm2::pack_ip_float(j, ip, p_ori, p_def, F_IP, dF_IP);
}

static int march_side_build(const MarchSide& s, int n_vtx, int n_grid_max, const int* n_grid_dev, const int* res, const int* pig_cnt,
                            const int* pig_bgn, const int* pig_idx, const float* p_def, const float* p_ori, const float* F_IP, const float* dF_IP,
                            int num_seek_IP, int* err_flag, hipStream_t st) {
    const int swap = (num_seek_IP == 1) ? 1 : 0;
    const int gz = (int)pn_div_up(n_grid_max, 256) < 1024 ? (int)pn_div_up(n_grid_max, 256) : 1024;
    k_nb_count<<<gz, 256, 0, st>>>(n_grid_max, n_grid_dev, res, pig_cnt, swap, s.nb_cnt);
    launch_cell_scan(n_grid_max, n_grid_dev, s.nb_cnt, s.nb_bgn, s.nb_cursor, st);
    k_nb_fill<<<gz, 256, 0, st>>>(n_grid_max, n_grid_dev, res, pig_cnt, pig_bgn, pig_idx, p_def, swap, s.nb_cnt, s.nb_bgn, s.nb, s.nb_capacity, err_flag, s.nb_rng);
    k_pack_ip<<<pn_div_up((uint64_t)n_vtx * PN_REC_FLOATS, 256), 256, 0, st>>>(n_vtx, p_ori, p_def, F_IP, dF_IP, s.rec);
    PN_LAUNCH_CHECK();
    return PN_OK;
}
