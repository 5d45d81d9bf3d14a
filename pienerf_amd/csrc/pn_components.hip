// Connected-component labelling of an occupancy lattice on the device: the floater filter of the point sampler and of the mesher.
//
// Input: a C-contiguous uint8 lattice [nx, ny, nz] (z fastest, pn_mc_count's layout), non-zero = occupied.  Output: int32 labels of the same shape,
// an occupied voxel's label = the smallest flat index of its component, an empty voxel's = -1.  Union-find with `labels` itself as the parent
// array: parent[v] <= v always, a root has parent[v] == v, and a hook is atomicMin(&parent[larger root], smaller root).  The smaller index always
// wins, so whatever order the hooks arrive in, a component's final root is its minimum index: the result is a pure function of the input.
// Three launches, the same three for every input (no host read-back, no "until nothing changes" loop: capturable):
//   tiles     k_ccl_tiles     one workgroup per PN_CCL_TX x TY x TZ tile: union-find over the tile's voxels in LDS, then every voxel writes its
//                             tile-local root as a global flat index (the local order is the global order restricted to the tile, so the local
//                             minimum is the global minimum of the tile-local component);
//   merge     k_ccl_merge     every occupied voxel unites itself with its occupied backward neighbours that lie in ANOTHER tile (faces, and at 26
//                             also edges and corners), with the global atomicMin union;
//   compress  k_ccl_compress  labels[v] = find(v).
// No workgroup waits on another: the only loops are find (strictly descending indices) and the union's retry, which repeats only after its atomicMin
// found that someone else had already hooked the node it meant to hook, and then continues from a strictly smaller index.
#include "pn_common.h"

#define PN_CCL_TX 4
#define PN_CCL_TY 8
#define PN_CCL_TZ 16  // 16 int32 labels = one 64-byte segment per tile row
#define PN_CCL_TILE (PN_CCL_TX * PN_CCL_TY * PN_CCL_TZ)
#define PN_CCL_BLOCK 256          // merge / compress: one lane per voxel, grid-stride
#define PN_CCL_MAX_BLOCKS (1u << 20)  // grids are capped (a 2^31-voxel line has 2^27 tiles); the workgroups stride over the rest
static_assert(PN_CCL_TX == 4 && PN_CCL_TY == 8 && PN_CCL_TZ == 16 && PN_CCL_TILE == 512, "the index shifts below are written for 4 x 8 x 16");

// The 13 backward neighbours (flat index below the voxel's own): c < 9: (-1, *, *); c < 12: (0, -1, *); c = 12: (0, 0, -1).  6-connectivity keeps the
// three with one non-zero component.
template <int CONN, class F>
__device__ __forceinline__ void ccl_backward(F f) {
#pragma unroll
    for (int c = 0; c < 13; c++) {
        const int di = c < 9 ? -1 : 0;
        const int dj = c < 9 ? c / 3 - 1 : (c < 12 ? -1 : 0);
        const int dk = c < 9 ? c % 3 - 1 : (c < 12 ? c - 10 : -1);
        if (CONN == 6 && (di != 0) + (dj != 0) + (dk != 0) != 1) continue;
        f(di, dj, dk);
    }
}

// ------------------------------------------------------------------------------------------------ union-find in LDS
// Other lanes of the workgroup hook concurrently: the parents are read with relaxed workgroup-scope atomic loads (ds_read, never kept in a register).
__device__ __forceinline__ int ccl_find_lds(int* s, int x) {
    for (;;) {
        const int p = __hip_atomic_load(s + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (p == x) return x;
        x = p;
    }
}

__device__ __forceinline__ void ccl_union_lds(int* s, int a, int b) {
    for (;;) {
        a = ccl_find_lds(s, a);
        b = ccl_find_lds(s, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(s + a, b);  // a > b: hook a under b if a is still a root
        if (old == a) return;
        a = old;  // a had a parent `old` < a already; parent[a] is now min(old, b), so old and b remain to be united
    }
}

// ------------------------------------------------------------------------------------------------ the global union-find
// The merge launch's find races with other workgroups' hooks.  Parents are read with relaxed AGENT-scope atomic loads (global_load sc1: past this
// CU's L1, which no other CU's atomic ever refreshes).  A plain load would be correct as well: a stale parent is an older parent, still a voxel of
// the same component with a smaller index, and whether a node is a root is decided by the atomicMin's returned value (executed at the memory side),
// never by a load; stale reads only cost retries.  The agent-scope load is chosen because it keeps those retries rare for the price of an L1 that the
// scattered 4-byte reads of a find use poorly anyway.
__device__ __forceinline__ int ccl_find_agent(int* L, int x) {
    for (;;) {
        const int p = __hip_atomic_load(L + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == x) return x;
        x = p;
    }
}

__device__ __forceinline__ void ccl_union_agent(int* L, int a, int b) {
    for (;;) {
        a = ccl_find_agent(L, a);
        b = ccl_find_agent(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(L + a, b);
        if (old == a) return;
        a = old;
    }
}

// ------------------------------------------------------------------------------------------------ tiles
template <int CONN>
__global__ void __launch_bounds__(PN_CCL_TILE) k_ccl_tiles(const uint8_t* __restrict__ occ, int nx, int ny, int nz, uint32_t tiles_y, uint32_t tiles_z,
                                                           uint32_t tiles, int* __restrict__ labels) {
    __shared__ int s_par[PN_CCL_TILE];
    const int t = threadIdx.x;
    const int li = t >> 7, lj = (t >> 4) & 7, lk = t & 15;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {  // uniform per workgroup: the barriers below are met by all lanes
        const uint32_t tk = tile % tiles_z, r = tile / tiles_z, tj = r % tiles_y, ti = r / tiles_y;
        const int i0 = (int)ti * PN_CCL_TX, j0 = (int)tj * PN_CCL_TY, k0 = (int)tk * PN_CCL_TZ;  // < nx, ny, nz
        const int i = i0 + li, j = j0 + lj, k = k0 + lk;
        const bool inside = i < nx && j < ny && k < nz;
        const int v = inside ? (i * ny + j) * nz + k : 0;  // < nx ny nz < 2^31
        const bool o = inside && occ[v] != 0;
        s_par[t] = o ? t : -1;
        __syncthreads();
        if (o) {
            ccl_backward<CONN>([&](int di, int dj, int dk) {
                const int a = li + di, b = lj + dj, c = lk + dk;
                if (a < 0 || b < 0 || b >= PN_CCL_TY || c < 0 || c >= PN_CCL_TZ) return;  // another tile's voxel: k_ccl_merge
                const int u = (a * PN_CCL_TY + b) * PN_CCL_TZ + c;
                if (__hip_atomic_load(s_par + u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= 0) ccl_union_lds(s_par, t, u);  // never turns -1
            });
        }
        __syncthreads();
        if (inside) {
            int lab = -1;
            if (o) {
                const int root = ccl_find_lds(s_par, t);  // an occupied voxel of this tile: inside the lattice
                lab = ((i0 + (root >> 7)) * ny + j0 + ((root >> 4) & 7)) * nz + k0 + (root & 15);
            }
            labels[v] = lab;
        }
        __syncthreads();  // s_par is rewritten by the next tile
    }
}

// ------------------------------------------------------------------------------------------------ merge
template <int CONN>
__global__ void __launch_bounds__(PN_CCL_BLOCK) k_ccl_merge(const uint8_t* __restrict__ occ, int nx, int ny, int nz, uint32_t n, int* labels) {
    const uint32_t nyz = (uint32_t)ny * nz;
    for (uint64_t x = (uint64_t)blockIdx.x * PN_CCL_BLOCK + threadIdx.x; x < n; x += (uint64_t)gridDim.x * PN_CCL_BLOCK) {
        const uint32_t v = (uint32_t)x;
        if (!occ[v]) continue;
        const int i = (int)(v / nyz), r = (int)(v - (uint32_t)i * nyz), j = r / nz, k = r - j * nz;
        ccl_backward<CONN>([&](int di, int dj, int dk) {
            const int a = i + di, b = j + dj, c = k + dk;
            if (a < 0 || b < 0 || b >= ny || c < 0 || c >= nz) return;
            if ((a >> 2) == (i >> 2) && (b >> 3) == (j >> 3) && (c >> 4) == (k >> 4)) return;  // the same tile: united in LDS already
            const int w = (a * ny + b) * nz + c;
            if (occ[w]) ccl_union_agent(labels, (int)v, w);
        });
    }
}

// ------------------------------------------------------------------------------------------------ compress
// After the merge launch has completed every parent is final except for what this launch writes itself, and it writes roots only: a lane that reads
// another lane's voxel sees its old parent or its root, both on the way to the same root.  Plain loads and stores.
__global__ void __launch_bounds__(PN_CCL_BLOCK) k_ccl_compress(uint32_t n, int* labels) {
    for (uint64_t x = (uint64_t)blockIdx.x * PN_CCL_BLOCK + threadIdx.x; x < n; x += (uint64_t)gridDim.x * PN_CCL_BLOCK) {
        const int p = labels[x];
        if (p < 0 || p == (int)x) continue;
        int root = p;
        for (;;) {
            const int q = labels[root];
            if (q == root) break;
            root = q;
        }
        if (root != p) labels[x] = root;
    }
}

// ------------------------------------------------------------------------------------------------ C ABI
static bool pn_ccl_dims_ok(int nx, int ny, int nz) {
    if (nx < 1 || ny < 1 || nz < 1) return false;
    const uint64_t lim = 1ull << 31;
    const uint64_t xy = (uint64_t)nx * ny;  // < 2^62
    return xy < lim && xy * nz < lim;
}

extern "C" int pn_ccl_label(const uint8_t* occ, int nx, int ny, int nz, int connectivity, int* labels, void* stream) {
    PN_REQUIRE(occ && labels);
    PN_REQUIRE(pn_ccl_dims_ok(nx, ny, nz));
    PN_REQUIRE(connectivity == 6 || connectivity == 26);
    const hipStream_t s = (hipStream_t)stream;
    const uint32_t n = (uint32_t)((uint64_t)nx * ny * nz);
    const uint32_t tiles_y = pn_div_up(ny, PN_CCL_TY), tiles_z = pn_div_up(nz, PN_CCL_TZ);
    const uint64_t tiles = (uint64_t)pn_div_up(nx, PN_CCL_TX) * tiles_y * tiles_z;  // <= n
    const uint32_t tile_blocks = (uint32_t)std::min<uint64_t>(tiles, PN_CCL_MAX_BLOCKS);
    const uint32_t voxel_blocks = std::min<uint32_t>(pn_div_up(n, PN_CCL_BLOCK), PN_CCL_MAX_BLOCKS);
    if (connectivity == 6) {
        k_ccl_tiles<6><<<tile_blocks, PN_CCL_TILE, 0, s>>>(occ, nx, ny, nz, tiles_y, tiles_z, (uint32_t)tiles, labels);
        PN_LAUNCH_CHECK();
        k_ccl_merge<6><<<voxel_blocks, PN_CCL_BLOCK, 0, s>>>(occ, nx, ny, nz, n, labels);
    } else {
        k_ccl_tiles<26><<<tile_blocks, PN_CCL_TILE, 0, s>>>(occ, nx, ny, nz, tiles_y, tiles_z, (uint32_t)tiles, labels);
        PN_LAUNCH_CHECK();
        k_ccl_merge<26><<<voxel_blocks, PN_CCL_BLOCK, 0, s>>>(occ, nx, ny, nz, n, labels);
    }
    PN_LAUNCH_CHECK();
    k_ccl_compress<<<voxel_blocks, PN_CCL_BLOCK, 0, s>>>(n, labels);
    PN_LAUNCH_CHECK();
    return PN_OK;
}
