// Marching cubes on a device lattice (nerf/utils.py:174-205 of the reference: extract_geometry's mcubes.marching_cubes, run on the GPU).
//
// Input: a C-contiguous fp32 field [nx, ny, nz] (z fastest) and an fp64 threshold.  Node (i,j,k) owns its lattice edges toward +x, +y, +z; a cell is
// named by its origin node.  Three stages, no atomics, so the output is a pure function of (field, threshold):
//   count  k_mc_count     one lane per node: the 3-bit mask of crossed owned edges and, at a cell origin, the cell's case; per tile of PN_MC_TILE
//                         nodes the sum of (vertices, triangles) packed into one 64-bit value (low / high 32 bits: V < 2^31 and T < 2^31 are checked
//                         on the host, so the halves never carry into each other);
//   scan   k_mc_scan_*    exclusive scan of the tile sums, PN_MC_SCAN entries per workgroup and level (levels until one workgroup holds the rest),
//                         then k_mc_offsets: every node's first vertex id;
//   emit   k_mc_emit      every node writes its vertices, every cell its triangles, at their offsets.
// Arithmetic contract ("Meshing"; tests/mc_reference.py restates it): above = (double)f > threshold (NaN is not above); an edge's
// vertex is lo_a + t, t = (threshold - f0) / (f1 - f0) in fp64 from the lower endpoint, the node's indices on the other axes; a NaN coordinate is
// written as the canonical quiet NaN.  Vertices in node order then axis, triangles in cell order then table order.
#include "pn_common.h"
#include "pn_mc_table.h"

#define PN_MC_TILE 256  // nodes per workgroup of k_mc_count / k_mc_offsets / k_mc_emit (one lane each)
#define PN_MC_SCAN 256  // tile sums per workgroup and level of the scan
static_assert(PN_MC_TILE == 4 * PN_WAVE && PN_MC_SCAN == 4 * PN_WAVE, "the block scan below is written for four waves");

__constant__ uint8_t d_mc_tri_count[256] = PN_MC_TRI_COUNT_INIT;
__constant__ __attribute__((aligned(16))) int8_t d_mc_tri_edges[256][PN_MC_SLOTS] = PN_MC_TRI_EDGES_INIT;
static const uint8_t h_mc_tri_count[256] = PN_MC_TRI_COUNT_INIT;
static const int8_t h_mc_tri_edges[256][PN_MC_SLOTS] = PN_MC_TRI_EDGES_INIT;

// Per Bourke edge: the owner node's offset from the cell origin (di, dj, dk) and the edge's axis.
__constant__ uint8_t d_mc_edge_owner[12][4] = {{0, 0, 0, 0}, {1, 0, 0, 1}, {0, 1, 0, 0}, {0, 0, 0, 1}, {0, 0, 1, 0}, {1, 0, 1, 1},
                                               {0, 1, 1, 0}, {0, 0, 1, 1}, {0, 0, 0, 2}, {1, 0, 0, 2}, {1, 1, 0, 2}, {0, 1, 0, 2}};

struct PnMcLayout {
    uint64_t n;            // nodes
    uint32_t tiles;        // PN_MC_TILE-node tiles
    int levels;            // scan levels below the single-workgroup top (0: the tile sums fit one workgroup)
    uint32_t len[8];       // entries of level l (len[0] = tiles)
    uint64_t off[8];       // byte offset of level l in the work buffer
    uint64_t code_off, voff_off, bytes;
};

static uint64_t pn_align256(uint64_t b) { return (b + 255) & ~(uint64_t)255; }

// work = [levels' 64-bit sums][uint16 code per node][uint32 first vertex id per node]
static PnMcLayout pn_mc_layout(int nx, int ny, int nz) {
    PnMcLayout L{};
    L.n = (uint64_t)nx * ny * nz;
    L.tiles = pn_div_up(L.n, PN_MC_TILE);
    uint64_t b = 0;
    uint32_t m = L.tiles;
    int l = 0;
    for (;;) {
        L.len[l] = m;
        L.off[l] = b;
        b = pn_align256(b + 8ull * m);
        if (m <= PN_MC_SCAN) break;
        m = pn_div_up(m, PN_MC_SCAN);
        l++;
    }
    L.levels = l;
    L.code_off = b;
    b = pn_align256(b + 2ull * L.n);
    L.voff_off = b;
    L.bytes = pn_align256(b + 4ull * L.n);
    return L;
}

// Every dimension >= 2, 3 nx ny nz < 2^31 (vertex ids) and 5 (nx-1)(ny-1)(nz-1) < 2^31 (triangle count).
static bool pn_mc_dims_ok(int nx, int ny, int nz) {
    if (nx < 2 || ny < 2 || nz < 2) return false;
    const uint64_t lim = 1ull << 31;
    const uint64_t xy = (uint64_t)nx * ny;  // < 2^62
    if (3 * xy >= lim) return false;
    const uint64_t n = xy * nz;             // < 2^62
    return 3 * n < lim && 5ull * (nx - 1) * (ny - 1) * (nz - 1) < lim;
}

// Exclusive scan of one 64-bit value per lane over a 256-lane workgroup; *total = the workgroup's sum.  Called once per kernel (s_w is not reset).
__device__ __forceinline__ uint64_t mc_block_scan(uint64_t v, uint64_t* s_w, uint64_t* total) {
    const int lane = threadIdx.x & (PN_WAVE - 1), w = threadIdx.x / PN_WAVE;
    uint64_t inc = v;
#pragma unroll
    for (int d = 1; d < PN_WAVE; d <<= 1) {
        const uint64_t y = __shfl_up(inc, d, PN_WAVE);
        if (lane >= d) inc += y;
    }
    if (lane == PN_WAVE - 1) s_w[w] = inc;
    __syncthreads();
    uint64_t before = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint64_t s = s_w[q];
        before += q < w ? s : 0;
        tot += s;
    }
    *total = tot;
    return before + inc - v;
}

__device__ __forceinline__ bool mc_above(float f, double thr) { return (double)f > thr; }

__device__ __forceinline__ uint64_t mc_packed(uint32_t code) {
    return (uint64_t)__popc((code >> 8) & 7u) | ((uint64_t)d_mc_tri_count[code & 255u] << 32);
}

// ------------------------------------------------------------------------------------------------ count
__global__ void __launch_bounds__(PN_MC_TILE) k_mc_count(const float* __restrict__ f, int nx, int ny, int nz, uint32_t n, double thr,
                                                         uint16_t* __restrict__ code, uint64_t* __restrict__ tile_sum) {
    __shared__ uint64_t s_w[4];
    const uint32_t v = blockIdx.x * PN_MC_TILE + threadIdx.x;
    uint32_t c = 0;
    if (v < n) {
        const uint32_t nyz = (uint32_t)ny * nz;
        const uint32_t i = v / nyz, r = v - i * nyz, j = r / nz, k = r - j * nz;
        const bool hx = i + 1 < (uint32_t)nx, hy = j + 1 < (uint32_t)ny, hz = k + 1 < (uint32_t)nz;
        const bool a0 = mc_above(f[v], thr);
        const bool a1 = hx && mc_above(f[v + nyz], thr);
        const bool a3 = hy && mc_above(f[v + nz], thr);
        const bool a4 = hz && mc_above(f[v + 1], thr);
        const uint32_t mask = (uint32_t)(hx && a1 != a0) | (uint32_t)(hy && a3 != a0) << 1 | (uint32_t)(hz && a4 != a0) << 2;
        uint32_t cs = 0;
        if (hx && hy && hz) {  // corners m = 0..7: bit m set when corner m is not above
            const bool a2 = mc_above(f[v + nyz + nz], thr), a5 = mc_above(f[v + nyz + 1], thr);
            const bool a6 = mc_above(f[v + nyz + nz + 1], thr), a7 = mc_above(f[v + nz + 1], thr);
            cs = (uint32_t)!a0 | (uint32_t)!a1 << 1 | (uint32_t)!a2 << 2 | (uint32_t)!a3 << 3 | (uint32_t)!a4 << 4 | (uint32_t)!a5 << 5 |
                 (uint32_t)!a6 << 6 | (uint32_t)!a7 << 7;
        }
        c = cs | mask << 8;
        code[v] = (uint16_t)c;
    }
    uint64_t total;
    mc_block_scan(mc_packed(c), s_w, &total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// ------------------------------------------------------------------------------------------------ scan
// sums[b] = sum of a[b PN_MC_SCAN .. (b+1) PN_MC_SCAN)
__global__ void __launch_bounds__(PN_MC_SCAN) k_mc_scan_reduce(const uint64_t* __restrict__ a, uint32_t n, uint64_t* __restrict__ sums) {
    __shared__ uint64_t s_w[4];
    const uint32_t x = blockIdx.x * PN_MC_SCAN + threadIdx.x;
    uint64_t total;
    mc_block_scan(x < n ? a[x] : 0, s_w, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// a = exclusive scan of a within each workgroup, plus base[b] (the level above, already scanned; NULL at the top).  The top level (one workgroup)
// also writes the grand total to totals = {V, T}.
__global__ void __launch_bounds__(PN_MC_SCAN) k_mc_scan_apply(uint64_t* __restrict__ a, uint32_t n, const uint64_t* __restrict__ base,
                                                              int64_t* __restrict__ totals) {
    __shared__ uint64_t s_w[4];
    const uint32_t x = blockIdx.x * PN_MC_SCAN + threadIdx.x;
    const uint64_t v = x < n ? a[x] : 0;
    uint64_t total;
    const uint64_t ex = mc_block_scan(v, s_w, &total) + (base ? base[blockIdx.x] : 0);
    if (x < n) a[x] = ex;
    if (totals && threadIdx.x == 0) {
        totals[0] = (int64_t)(total & 0xffffffffull);
        totals[1] = (int64_t)(total >> 32);
    }
}

// voff[v] = first vertex id of node v
__global__ void __launch_bounds__(PN_MC_TILE) k_mc_offsets(const uint16_t* __restrict__ code, uint32_t n, const uint64_t* __restrict__ tile_off,
                                                           uint32_t* __restrict__ voff) {
    __shared__ uint64_t s_w[4];
    const uint32_t v = blockIdx.x * PN_MC_TILE + threadIdx.x;
    const uint32_t c = v < n ? code[v] : 0;
    uint64_t total;
    const uint64_t ex = mc_block_scan((uint64_t)__popc((c >> 8) & 7u), s_w, &total);
    if (v < n) voff[v] = (uint32_t)(tile_off[blockIdx.x] + ex);
}

// ------------------------------------------------------------------------------------------------ emit
__device__ __forceinline__ double mc_coord(double lo, double t) {
    const double c = lo + t;
    return c == c ? c : __longlong_as_double(0x7FF8000000000000ll);  // canonical quiet NaN
}

__global__ void __launch_bounds__(PN_MC_TILE) k_mc_emit(const float* __restrict__ f, int ny, int nz, uint32_t n, double thr,
                                                        const uint16_t* __restrict__ code, const uint32_t* __restrict__ voff,
                                                        const uint64_t* __restrict__ tile_off, double* __restrict__ verts, int* __restrict__ tris) {
    __shared__ uint64_t s_w[4];
    const int8_t* tab = &d_mc_tri_edges[0][0];  // through the vector cache: an LDS copy per workgroup was slower ("Meshing")
    const uint32_t v = blockIdx.x * PN_MC_TILE + threadIdx.x;
    const uint32_t c = v < n ? code[v] : 0;
    uint64_t total;
    const uint64_t ex = mc_block_scan(mc_packed(c), s_w, &total) + tile_off[blockIdx.x];
    if (v >= n) return;
    const uint32_t mask = (c >> 8) & 7u, cs = c & 255u;
    const uint32_t nyz = (uint32_t)ny * nz;
    if (mask) {
        const uint32_t i = v / nyz, r = v - i * nyz, j = r / nz, k = r - j * nz;
        const double f0 = (double)f[v];
        const uint32_t stride[3] = {nyz, (uint32_t)nz, 1u};
        const double idx[3] = {(double)i, (double)j, (double)k};
        uint64_t o = (uint32_t)ex;  // this node's first vertex id
#pragma unroll
        for (int a = 0; a < 3; a++) {
            if (!((mask >> a) & 1u)) continue;
            const double f1 = (double)f[v + stride[a]];
            const double t = (thr - f0) / (f1 - f0);
            double* p = verts + 3 * o;
            p[0] = a == 0 ? mc_coord(idx[0], t) : idx[0];
            p[1] = a == 1 ? mc_coord(idx[1], t) : idx[1];
            p[2] = a == 2 ? mc_coord(idx[2], t) : idx[2];
            o++;
        }
    }
    const int nt = d_mc_tri_count[cs];
    if (nt) {
        int* out = tris + 3 * (uint64_t)(uint32_t)(ex >> 32);
        for (int s = 0; s < 3 * nt; s++) {
            const int e = tab[cs * PN_MC_SLOTS + s];
            const uint32_t w = v + d_mc_edge_owner[e][0] * nyz + d_mc_edge_owner[e][1] * (uint32_t)nz + d_mc_edge_owner[e][2];
            const uint32_t ax = d_mc_edge_owner[e][3];
            out[s] = (int)(voff[w] + __popc((code[w] >> 8) & ((1u << ax) - 1u)));
        }
    }
}

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" uint64_t pn_mc_work_bytes(int nx, int ny, int nz) { return pn_mc_dims_ok(nx, ny, nz) ? pn_mc_layout(nx, ny, nz).bytes : 0; }

extern "C" int pn_mc_count(const float* field, int nx, int ny, int nz, double threshold, void* work, int64_t* totals, void* stream) {
    PN_REQUIRE(pn_mc_dims_ok(nx, ny, nz));
    PN_REQUIRE(field && work && totals);
    const hipStream_t s = (hipStream_t)stream;
    const PnMcLayout L = pn_mc_layout(nx, ny, nz);
    char* w = (char*)work;
    uint64_t* lv[8];
    for (int l = 0; l <= L.levels; l++) lv[l] = (uint64_t*)(w + L.off[l]);
    uint16_t* code = (uint16_t*)(w + L.code_off);
    k_mc_count<<<L.tiles, PN_MC_TILE, 0, s>>>(field, nx, ny, nz, (uint32_t)L.n, threshold, code, lv[0]);
    PN_LAUNCH_CHECK();
    for (int l = 0; l < L.levels; l++) {
        k_mc_scan_reduce<<<L.len[l + 1], PN_MC_SCAN, 0, s>>>(lv[l], L.len[l], lv[l + 1]);
        PN_LAUNCH_CHECK();
    }
    k_mc_scan_apply<<<1, PN_MC_SCAN, 0, s>>>(lv[L.levels], L.len[L.levels], nullptr, totals);
    PN_LAUNCH_CHECK();
    for (int l = L.levels - 1; l >= 0; l--) {
        k_mc_scan_apply<<<L.len[l + 1], PN_MC_SCAN, 0, s>>>(lv[l], L.len[l], lv[l + 1], nullptr);
        PN_LAUNCH_CHECK();
    }
    k_mc_offsets<<<L.tiles, PN_MC_TILE, 0, s>>>(code, (uint32_t)L.n, lv[0], (uint32_t*)(w + L.voff_off));
    PN_LAUNCH_CHECK();
    return PN_OK;
}

extern "C" int pn_mc_emit(const float* field, int nx, int ny, int nz, double threshold, const void* work, double* vertices, int* triangles,
                          void* stream) {
    PN_REQUIRE(pn_mc_dims_ok(nx, ny, nz));
    PN_REQUIRE(field && work && vertices && triangles);
    const hipStream_t s = (hipStream_t)stream;
    const PnMcLayout L = pn_mc_layout(nx, ny, nz);
    const char* w = (const char*)work;
    k_mc_emit<<<L.tiles, PN_MC_TILE, 0, s>>>(field, ny, nz, (uint32_t)L.n, threshold, (const uint16_t*)(w + L.code_off),
                                            (const uint32_t*)(w + L.voff_off), (const uint64_t*)(w + L.off[0]), vertices, triangles);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

extern "C" int pn_mc_case_table(uint8_t* tri_count, int8_t* tri_edges) {
    PN_REQUIRE(tri_count && tri_edges);
    memcpy(tri_count, h_mc_tri_count, sizeof(h_mc_tri_count));
    memcpy(tri_edges, h_mc_tri_edges, sizeof(h_mc_tri_edges));
    return PN_OK;
}
