// Baseline JPEG of a rendered frame, encoded on the device (pienerf_amd/video.py; include/pienerf_hip.h: pn_jpeg_encode).  The frame is the
// renderer's fp32 [H, W, 3]; what leaves is the entropy-coded scan (everything between the SOS header and EOI, restart markers included) and its length,
// so tens of kilobytes cross to the host instead of 12 bytes per pixel.  The host prepends a header built once per run (video.jpeg_header).
//
// Three launches, nothing else: no allocation, no host synchronisation, no atomics whose order matters — equal inputs give equal bytes, and the launches
// are legal inside a stream capture.
//   k_jpeg_dct      a workgroup per 16 x 16 pixels (one 4:2:0 MCU, or four 4:4:4 MCUs): pixels -> 8 bits -> YCbCr in LDS, the two DCT passes through
//                   LDS, quantisation; int16 coef[block][64] in zigzag order, blocks in scan order.
//   k_jpeg_entropy  a workgroup per restart interval (one MCU row), a thread per block: a block's DC difference comes from coef (the previous block of
//                   its component), so its bit string is independent of every other block's.  Lengths, a workgroup scan for the bit offsets, then
//                   every block writes its bits at its offset into the interval's staging words (global memory: the worst case of a wide frame does
//                   not fit LDS, and the staging is sized from that worst case): whole words plainly, the words it shares with a neighbour by atomicOr
//                   onto zeros the sharers wrote before a barrier.  Then the 0xFF bytes are counted, a second scan, and the stuffed bytes go to the
//                   interval's segment.
//   k_jpeg_gather   a workgroup per interval sums the lengths in front of it (a fixed-order integer sum: nothing to look back at), copies its segment
//                   into the stream, appends RSTm, and the last one writes the byte count.
//
// The arithmetic is fixed operation by operation (-ffp-contract=off; tests/jpeg_reference.py restates it in numpy float32 and the bytes agree):
// products and sums round once each, sums run left to right, the quotient is IEEE, rintf rounds ties to even.
//
// LDS banks: both DCT passes read their tile by rows — the row pass has the lanes of a wave on 8 rows (one broadcast address each), the column pass on
// 8 consecutive floats of one row — so neither is a transposed read; rows are padded to 9 floats all the same, which keeps the 4 rows a 32-lane
// group touches on distinct banks whatever the block's base is.
#include <math.h>

#include "pn_common.h"
#include "pn_jpeg_tables.h"

#define PN_JPEG_THREADS 256
#define PN_JPEG_ROW 9                         // floats per padded tile row
#define PN_JPEG_TILE (8 * PN_JPEG_ROW)
#define PN_JPEG_BLOCK_BYTES 208               // a block's bits: at most 20 (DC: 9 + 11) + 63 * 26 (AC: 16 + 10) = 1658 < 1664
#define PN_JPEG_BLOCK_WORDS (PN_JPEG_BLOCK_BYTES / 4)

struct PnJpegQuant { uint8_t luma[64], chroma[64]; };   // natural order; by value in the launch: a captured launch keeps its tables

__constant__ float d_jpeg_dct[64] = PN_JPEG_DCT_INIT;
__constant__ uint8_t d_jpeg_zigzag[64] = PN_JPEG_ZIGZAG_INIT;
__constant__ uint32_t d_jpeg_dc[2][12] = {PN_JPEG_DC_LUMA_INIT, PN_JPEG_DC_CHROMA_INIT};
__constant__ uint32_t d_jpeg_ac[2][256] = {PN_JPEG_AC_LUMA_INIT, PN_JPEG_AC_CHROMA_INIT};

// ------------------------------------------------------------------ pass A: colour, DCT, quantisation

__device__ __forceinline__ float pn_jpeg_pixel(float v) {
    const float c = isnan(v) ? 0.0f : fminf(fmaxf(v, 0.0f), 1.0f);
    return floorf(c * 255.0f);   // io.save_image's truncation
}

// 4:2:0: the workgroup's 16 x 16 pixels are one MCU, tiles Y00 Y01 Y10 Y11 Cb Cr.  4:4:4: four MCUs (quadrant m = 2 row + column), tiles 3 m + {Y, Cb, Cr}.
template <int SUB>
__global__ void __launch_bounds__(PN_JPEG_THREADS) k_jpeg_dct(const float* __restrict__ image, uint32_t W, uint32_t H, uint32_t mcus_x, uint32_t mcus_y,
                                                              PnJpegQuant q, int16_t* __restrict__ coef) {
    constexpr int NT = SUB == 420 ? 6 : 12;
    __shared__ float s[12 * PN_JPEG_TILE], t[12 * PN_JPEG_TILE];
    __shared__ float full[2][16][17];   // 4:2:0: Cb, Cr at full resolution
    __shared__ float sC[64], sQ[2][64];
    __shared__ uint8_t sZ[64];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    if (tid < 64) {
        sC[tid] = d_jpeg_dct[tid];
        sQ[0][tid] = (float)q.luma[tid];
        sQ[1][tid] = (float)q.chroma[tid];
        sZ[tid] = d_jpeg_zigzag[tid];
    }
    {   // the last column and row are replicated into the padding
        const uint32_t px = min(blockIdx.x * 16u + tx, W - 1u), py = min(blockIdx.y * 16u + ty, H - 1u);
        const float* p = image + ((size_t)py * W + px) * 3;
        const float R = pn_jpeg_pixel(p[0]), G = pn_jpeg_pixel(p[1]), B = pn_jpeg_pixel(p[2]);
        const float Y = 0.299f * R + 0.587f * G + 0.114f * B - 128.0f;
        const float Cb = -0.168735892f * R - 0.331264108f * G + 0.5f * B;
        const float Cr = 0.5f * R - 0.418687589f * G - 0.081312411f * B;
        const int quad = (ty >> 3) * 2 + (tx >> 3), in = (ty & 7) * PN_JPEG_ROW + (tx & 7);
        if (SUB == 420) {
            s[quad * PN_JPEG_TILE + in] = Y;
            full[0][ty][tx] = Cb;
            full[1][ty][tx] = Cr;
        } else {
            s[(quad * 3 + 0) * PN_JPEG_TILE + in] = Y;
            s[(quad * 3 + 1) * PN_JPEG_TILE + in] = Cb;
            s[(quad * 3 + 2) * PN_JPEG_TILE + in] = Cr;
        }
    }
    __syncthreads();
    if (SUB == 420) {
        if (tid < 128) {
            const int c = tid >> 6, y = (tid >> 3) & 7, x = tid & 7;
            const float (*f)[17] = full[c];
            s[(4 + c) * PN_JPEG_TILE + y * PN_JPEG_ROW + x] = ((f[2 * y][2 * x] + f[2 * y][2 * x + 1]) + (f[2 * y + 1][2 * x] + f[2 * y + 1][2 * x + 1])) * 0.25f;
        }
        __syncthreads();
    }
    // rows: t[y][u] = sum_x s[y][x] C[u][x], x ascending
    for (int i = tid; i < NT * 64; i += PN_JPEG_THREADS) {
        const int b = i >> 6, y = (i >> 3) & 7, u = i & 7;
        const float* sr = s + b * PN_JPEG_TILE + y * PN_JPEG_ROW;
        float acc = sr[0] * sC[u * 8];
#pragma unroll
        for (int x = 1; x < 8; x++) acc = acc + sr[x] * sC[u * 8 + x];
        t[b * PN_JPEG_TILE + y * PN_JPEG_ROW + u] = acc;
    }
    __syncthreads();
    // columns: d[v][u] = sum_y C[v][y] t[y][u], y ascending; d replaces s
    for (int i = tid; i < NT * 64; i += PN_JPEG_THREADS) {
        const int b = i >> 6, v = (i >> 3) & 7, u = i & 7;
        const float* tc = t + b * PN_JPEG_TILE + u;
        float acc = sC[v * 8] * tc[0];
#pragma unroll
        for (int y = 1; y < 8; y++) acc = acc + sC[v * 8 + y] * tc[y * PN_JPEG_ROW];
        s[b * PN_JPEG_TILE + v * PN_JPEG_ROW + u] = acc;
    }
    __syncthreads();
    // quantise, zigzag order
    for (int i = tid; i < NT * 64; i += PN_JPEG_THREADS) {
        const int b = i >> 6, k = i & 63, n = sZ[k];
        uint32_t block;
        int chroma;
        if (SUB == 420) {
            chroma = b >= 4;
            block = (blockIdx.y * mcus_x + blockIdx.x) * 6u + b;
        } else {
            const int m = b / 3, c = b - 3 * m;
            const uint32_t my = blockIdx.y * 2u + (m >> 1), mx = blockIdx.x * 2u + (m & 1);
            if (my >= mcus_y || mx >= mcus_x) continue;   // a quadrant behind the last MCU column / row
            chroma = c > 0;
            block = (my * mcus_x + mx) * 3u + c;
        }
        float qv = rintf(s[b * PN_JPEG_TILE + (n >> 3) * PN_JPEG_ROW + (n & 7)] / sQ[chroma][n]);
        if (k > 0) qv = fminf(fmaxf(qv, -1023.0f), 1023.0f);   // baseline's largest AC category; rounding can pass it by one
        coef[(size_t)block * 64 + k] = (int16_t)(int)qv;
    }
}

// ------------------------------------------------------------------ pass B: entropy coding of one restart interval

struct PnJpegCount {   // a block's length in bits
    uint32_t n = 0;
    __device__ __forceinline__ void put(uint32_t, int len) { n += len; }
};

// A block's bits written at bit position p0 of the staging words; bit p of the interval is bit 31 - p % 32 of word p / 32.  A word this block fills
// alone is stored; its first word when it starts inside one, and its last when it ends inside one, are shared and OR-ed onto the zeros of phase 1.
struct PnJpegWriter {
    uint32_t* stage;
    uint32_t w;
    uint64_t acc = 0;
    int n;
    bool shared_first;
    __device__ __forceinline__ PnJpegWriter(uint32_t* stage_, uint32_t p0) : stage(stage_), w(p0 >> 5), n(p0 & 31), shared_first((p0 & 31) != 0) {}
    __device__ __forceinline__ void put(uint32_t bits, int len) {   // 0 < len <= 26, n < 32
        acc |= (uint64_t)bits << (64 - n - len);
        n += len;
        if (n >= 32) {
            const uint32_t word = (uint32_t)(acc >> 32);
            if (shared_first) {
                atomicOr(stage + w, word);
                shared_first = false;
            } else {
                stage[w] = word;
            }
            w++;
            acc <<= 32;
            n -= 32;
        }
    }
    __device__ __forceinline__ uint32_t position() const { return w * 32u + (uint32_t)n; }
    __device__ __forceinline__ void finish() {
        if (n > 0) atomicOr(stage + w, (uint32_t)(acc >> 32));
    }
};

// code of the symbol, then the value's `size` low bits (a negative value as value - 1: T.81 F.1.2.1)
template <class Sink>
__device__ __forceinline__ void pn_jpeg_put_value(Sink& sink, uint32_t entry, int value, int size) {
    const uint32_t bits = (uint32_t)(value < 0 ? value - 1 : value) & ((1u << size) - 1u);
    sink.put(((entry & 0xffffu) << size) | bits, (int)(entry >> 16) + size);
}

__device__ __forceinline__ int pn_jpeg_size(int value) { return value == 0 ? 0 : 32 - __clz(abs(value)); }

// Block i of the interval whose coefficients start at `coef`: the DC difference against the previous block of the same component in the interval, the
// AC run / size symbols with ZRL and EOB.
template <int SUB, class Sink>
__device__ __forceinline__ void pn_jpeg_walk(const int16_t* __restrict__ coef, uint32_t i, const uint32_t* s_dc, const uint32_t* s_ac, Sink& sink) {
    constexpr uint32_t BPM = SUB == 420 ? 6 : 3;
    const uint32_t k = i % BPM;
    int chroma, back;   // back: how many blocks before i its predecessor lies; 0: none
    if (SUB == 420) {
        chroma = k >= 4;
        back = (k >= 1 && k <= 3) ? 1 : (i < BPM ? 0 : (k == 0 ? 3 : 6));
    } else {
        chroma = k > 0;
        back = i < BPM ? 0 : 3;
    }
    const int16_t* c = coef + (size_t)i * 64;
    const int pred = back ? (int)coef[(size_t)(i - back) * 64] : 0;
    const int diff = min(max((int)c[0] - pred, -2047), 2047);
    const int dsize = pn_jpeg_size(diff);
    pn_jpeg_put_value(sink, s_dc[chroma * 12 + dsize], diff, dsize);
    const uint32_t* ac = s_ac + chroma * 256;
    const uint4* v = (const uint4*)c;
    int run = 0;
#pragma unroll
    for (int g = 0; g < 8; g++) {
        const uint4 q = v[g];
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int e = 0; e < 8; e++) {
            if (g == 0 && e == 0) continue;
            const int val = (int)(int16_t)(w[e >> 1] >> ((e & 1) * 16));
            if (val == 0) {
                run++;
                continue;
            }
            while (run > 15) {
                const uint32_t zrl = ac[0xf0];
                sink.put(zrl & 0xffffu, (int)(zrl >> 16));
                run -= 16;
            }
            const int size = pn_jpeg_size(val);
            pn_jpeg_put_value(sink, ac[(run << 4) | size], val, size);
            run = 0;
        }
    }
    if (run > 0) {
        const uint32_t eob = ac[0x00];
        sink.put(eob & 0xffffu, (int)(eob >> 16));
    }
}

// exclusive prefix of v over the workgroup's threads in thread order, and the total; red: one word per wave
__device__ __forceinline__ uint32_t pn_jpeg_scan(uint32_t v, uint32_t* red, uint32_t& total) {
    const int lane = threadIdx.x % PN_WAVE, wave = threadIdx.x / PN_WAVE;
    uint32_t incl = v;
#pragma unroll
    for (int o = 1; o < PN_WAVE; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    if (lane == PN_WAVE - 1) red[wave] = incl;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < PN_JPEG_THREADS / PN_WAVE; w++) {
        const uint32_t r = red[w];
        if (w < wave) base += r;
        tot += r;
    }
    __syncthreads();   // red is free for the next scan
    total = tot;
    return base + incl - v;
}

// Interval r = blockIdx.x: blocks [r nb, (r + 1) nb).  bitoff: nb words, stage: nb * 52 words, seg: nb * 416 bytes, all of this interval.
template <int SUB>
__global__ void __launch_bounds__(PN_JPEG_THREADS) k_jpeg_entropy(const int16_t* __restrict__ coef_all, uint32_t nb, uint32_t* __restrict__ bitoff_all,
                                                                  uint32_t* stage_all, uint8_t* __restrict__ seg_all, uint32_t* __restrict__ seglen) {
    __shared__ uint32_t s_dc[2 * 12], s_ac[2 * 256], red[PN_JPEG_THREADS / PN_WAVE];
    __shared__ uint32_t s_bits;
    const uint32_t tid = threadIdx.x, r = blockIdx.x;
    const int16_t* coef = coef_all + (size_t)r * nb * 64;
    uint32_t* bitoff = bitoff_all + (size_t)r * nb;
    uint32_t* stage = stage_all + (size_t)r * nb * PN_JPEG_BLOCK_WORDS;
    uint8_t* seg = seg_all + (size_t)r * nb * (2 * PN_JPEG_BLOCK_BYTES);
    for (uint32_t i = tid; i < 2 * 256; i += PN_JPEG_THREADS) s_ac[i] = (&d_jpeg_ac[0][0])[i];
    if (tid < 2 * 12) s_dc[tid] = (&d_jpeg_dc[0][0])[tid];
    __syncthreads();

    // phase 1: lengths -> bit offsets; the interval is padded to a byte (the last block carries the pad bits); every block zeroes the words it shares
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nb; base += PN_JPEG_THREADS) {
        const uint32_t i = base + tid;
        PnJpegCount count;
        if (i < nb) pn_jpeg_walk<SUB>(coef, i, s_dc, s_ac, count);
        uint32_t total;
        const uint32_t p0 = carry + pn_jpeg_scan(count.n, red, total);
        if (i < nb) {
            uint32_t end = p0 + count.n;
            if (i == nb - 1) {
                end = (end + 7u) & ~7u;
                s_bits = end;
            }
            bitoff[i] = p0;
            if (p0 & 31u) stage[p0 >> 5] = 0u;
            if (end & 31u) stage[end >> 5] = 0u;   // end <= nb * 1658 + 7 < nb * 1664: inside the interval's words
        }
        carry += total;
    }
    __threadfence();
    __syncthreads();

    // phase 2: the bits
    for (uint32_t i = tid; i < nb; i += PN_JPEG_THREADS) {
        PnJpegWriter wr(stage, bitoff[i]);
        pn_jpeg_walk<SUB>(coef, i, s_dc, s_ac, wr);
        if (i == nb - 1) {
            const int pad = (int)((0u - wr.position()) & 7u);
            if (pad) wr.put((1u << pad) - 1u, pad);
        }
        wr.finish();
    }
    __threadfence();
    __syncthreads();

    // phase 3: a 0x00 behind every 0xFF; a thread per staged word
    const uint32_t nbytes = s_bits >> 3, nwords = (nbytes + 3u) >> 2;
    uint32_t stuffed = 0;
    for (uint32_t base = 0; base < nwords; base += PN_JPEG_THREADS) {
        const uint32_t j = base + tid;
        uint32_t word = 0, have = 0, ff = 0;
        if (j < nwords) {
            word = __hip_atomic_load(stage + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // written by stores and atomics of other waves
            have = min(4u, nbytes - 4u * j);
            for (uint32_t e = 0; e < have; e++) ff += ((word >> (24 - 8 * e)) & 0xffu) == 0xffu;
        }
        uint32_t total;
        uint32_t at = 4u * j + stuffed + pn_jpeg_scan(ff, red, total);
        for (uint32_t e = 0; e < have; e++) {
            const uint32_t b = (word >> (24 - 8 * e)) & 0xffu;
            seg[at++] = (uint8_t)b;
            if (b == 0xffu) seg[at++] = 0;
        }
        stuffed += total;
    }
    if (tid == 0) seglen[r] = nbytes + stuffed;
}

// ------------------------------------------------------------------ pass C: the segments, contiguous, with RSTm between them

__global__ void __launch_bounds__(PN_JPEG_THREADS) k_jpeg_gather(const uint8_t* __restrict__ seg_all, const uint32_t* __restrict__ seglen, uint32_t nb,
                                                                 uint32_t rows, uint8_t* __restrict__ out, uint32_t* __restrict__ nbytes_out) {
    __shared__ uint32_t red[PN_JPEG_THREADS / PN_WAVE];
    const uint32_t tid = threadIdx.x, r = blockIdx.x;
    uint32_t before = 0;
    for (uint32_t i = tid; i < r; i += PN_JPEG_THREADS) before += seglen[i];
    uint32_t sum;
    pn_jpeg_scan(before, red, sum);
    const uint32_t off = sum + 2u * r, len = seglen[r];
    const uint8_t* seg = seg_all + (size_t)r * nb * (2 * PN_JPEG_BLOCK_BYTES);
    for (uint32_t j = tid; j < len; j += PN_JPEG_THREADS) out[off + j] = seg[j];
    if (tid == 0) {
        if (r + 1 < rows) {
            out[off + len] = 0xff;
            out[off + len + 1] = (uint8_t)(0xd0u + (r & 7u));
        } else {
            *nbytes_out = off + len;
        }
    }
}

// ------------------------------------------------------------------ C ABI

struct PnJpegGeometry { uint32_t mcus_x, mcus_y, bpm; uint64_t n_blocks, capacity; };

// false for what pn_jpeg_encode refuses by its size alone: a side of 0 or above 65535, another subsampling, a bound the 32-bit count cannot hold
static bool pn_jpeg_geometry(uint32_t W, uint32_t H, int subsampling, PnJpegGeometry* g) {
    if (W == 0 || H == 0 || W > 65535 || H > 65535 || (subsampling != 420 && subsampling != 444)) return false;
    const uint32_t m = subsampling == 420 ? 16 : 8;
    g->bpm = subsampling == 420 ? 6 : 3;
    g->mcus_x = (W + m - 1) / m;
    g->mcus_y = (H + m - 1) / m;
    g->n_blocks = (uint64_t)g->mcus_x * g->mcus_y * g->bpm;
    g->capacity = g->n_blocks * (2 * PN_JPEG_BLOCK_BYTES) + 2ull * (g->mcus_y - 1);
    return g->capacity <= 0xffffffffull;
}

extern "C" uint64_t pn_jpeg_stream_capacity(uint32_t W, uint32_t H, int subsampling) {
    PnJpegGeometry g;
    return pn_jpeg_geometry(W, H, subsampling, &g) ? g.capacity : 0;
}

// coef | stage | seg | bitoff | seglen
extern "C" uint64_t pn_jpeg_work_bytes(uint32_t W, uint32_t H, int subsampling) {
    PnJpegGeometry g;
    if (!pn_jpeg_geometry(W, H, subsampling, &g)) return 0;
    return g.n_blocks * (128 + PN_JPEG_BLOCK_BYTES + 2 * PN_JPEG_BLOCK_BYTES + 4) + 4ull * g.mcus_y;
}

static bool pn_jpeg_disjoint(const void* a, uint64_t na, const void* b, uint64_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa + na <= pb || pb + nb <= pa;
}

extern "C" int pn_jpeg_encode(const float* image, uint32_t W, uint32_t H, int subsampling, const uint8_t* qtab_luma_host64,
                              const uint8_t* qtab_chroma_host64, void* work, uint8_t* stream_out, uint64_t capacity, uint32_t* nbytes_out, void* stream) {
    PN_REQUIRE(image && qtab_luma_host64 && qtab_chroma_host64 && work && stream_out && nbytes_out);
    PnJpegGeometry g;
    PN_REQUIRE(pn_jpeg_geometry(W, H, subsampling, &g));
    PnJpegQuant q;
    for (int i = 0; i < 64; i++) {
        PN_REQUIRE(qtab_luma_host64[i] != 0 && qtab_chroma_host64[i] != 0);
        q.luma[i] = qtab_luma_host64[i];
        q.chroma[i] = qtab_chroma_host64[i];
    }
    PN_REQUIRE(capacity >= g.capacity);
    PN_REQUIRE((uintptr_t)work % 16 == 0);
    const uint64_t image_bytes = (uint64_t)W * H * 12, work_bytes = pn_jpeg_work_bytes(W, H, subsampling);
    PN_REQUIRE(pn_jpeg_disjoint(image, image_bytes, work, work_bytes) && pn_jpeg_disjoint(image, image_bytes, stream_out, capacity) &&
               pn_jpeg_disjoint(image, image_bytes, nbytes_out, 4) && pn_jpeg_disjoint(work, work_bytes, stream_out, capacity) &&
               pn_jpeg_disjoint(work, work_bytes, nbytes_out, 4) && pn_jpeg_disjoint(stream_out, capacity, nbytes_out, 4));

    char* at = (char*)work;
    int16_t* coef = (int16_t*)at;
    at += g.n_blocks * 128;
    uint32_t* stage = (uint32_t*)at;
    at += g.n_blocks * PN_JPEG_BLOCK_BYTES;
    uint8_t* seg = (uint8_t*)at;
    at += g.n_blocks * (2 * PN_JPEG_BLOCK_BYTES);
    uint32_t* bitoff = (uint32_t*)at;
    at += g.n_blocks * 4;
    uint32_t* seglen = (uint32_t*)at;
    const uint32_t nb = g.mcus_x * g.bpm;   // blocks per restart interval
    hipStream_t s = (hipStream_t)stream;
    if (subsampling == 420) {
        k_jpeg_dct<420><<<dim3(g.mcus_x, g.mcus_y), PN_JPEG_THREADS, 0, s>>>(image, W, H, g.mcus_x, g.mcus_y, q, coef);
        PN_LAUNCH_CHECK();
        k_jpeg_entropy<420><<<g.mcus_y, PN_JPEG_THREADS, 0, s>>>(coef, nb, bitoff, stage, seg, seglen);
    } else {
        k_jpeg_dct<444><<<dim3((g.mcus_x + 1) / 2, (g.mcus_y + 1) / 2), PN_JPEG_THREADS, 0, s>>>(image, W, H, g.mcus_x, g.mcus_y, q, coef);
        PN_LAUNCH_CHECK();
        k_jpeg_entropy<444><<<g.mcus_y, PN_JPEG_THREADS, 0, s>>>(coef, nb, bitoff, stage, seg, seglen);
    }
    PN_LAUNCH_CHECK();
    k_jpeg_gather<<<g.mcus_y, PN_JPEG_THREADS, 0, s>>>(seg, seglen, nb, g.mcus_y, stream_out, nbytes_out);
    PN_LAUNCH_CHECK();
    return PN_OK;
}
