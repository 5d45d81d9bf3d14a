// Stable compaction of the alive list, the end-of-trip bookkeeping, and composite + compaction in one launch: kernels of the render unit
// (included by pn_render_ops.hip only).
#pragma once
#include "pn_composite.h"
#include "pn_render_records.h"

// ------------------------------------------------------------------------------------------------ stable compaction
__global__ void __launch_bounds__(256) k_chunk_count(const int* __restrict__ rays_alive, uint32_t n, int* chunk_counts) {
    const uint32_t i = threadIdx.x + blockIdx.x * blockDim.x;
    const int c = __syncthreads_count(i < n && rays_alive[i] >= 0);
    if (threadIdx.x == 0) chunk_counts[blockIdx.x] = c;
}

// Packs the PN_SEGS segments of a list trip's sample list into the dense list the network kernel reads and publishes the total
// (workgroup s copies segment s behind the segments before it).  A dense trip has nothing to pack.
__global__ void __launch_bounds__(256) k_list_pack(PnTrip* trip, const int* __restrict__ samp_counts, const int* __restrict__ list_seg, int seg_cap,
                                                   int* __restrict__ list) {
    if (trip_is_dense(trip) || trip->n_alive <= 0) return;
    const int s = (int)blockIdx.x, lane = threadIdx.x & 63;
    __shared__ int before_s, total_s;
    if (threadIdx.x < 64) {
        const int c = samp_counts[lane * PN_SEG_STRIDE];
        int pre = lane < s ? c : 0, tot = c;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { pre += __shfl_xor(pre, o); tot += __shfl_xor(tot, o); }
        if (lane == 0) { before_s = pre; total_s = tot; }
    }
    __syncthreads();
    const int n = samp_counts[s * PN_SEG_STRIDE], off = before_s;
    const int* src = list_seg + (size_t)s * seg_cap;
    for (int i = threadIdx.x; i < n; i += 256) list[off + i] = src[i];
    if (s == 0 && threadIdx.x == 0) trip->n_samples = total_s;
}

// End of a trip of the frame driver, executed by ONE wave once every ray of the trip has been composited and `sum` of them survive: folds the
// march's segment counters into the records and clears them, and writes the next trip's record (renderer.py:839-846,891) — with ray groups
// (g_next != nullptr, see PnGroup) also the next trip's group records from this trip's and the per-group survivor counts of the composite:
// N_b // n_alive_b per group, exclusive sums for the first alive position and the first sample slot.
__device__ __forceinline__ void trip_epilogue(int lane, int sum, PnTrip* trip, PnTrip* next, uint32_t N_rays, uint32_t max_steps, int dense_trips,
                                              int* seg_counters, int* tail_diag, const PnGroup* __restrict__ g_cur, PnGroup* __restrict__ g_next,
                                              int* group_cnt, uint32_t group_rays, uint32_t n_groups) {
    if (seg_counters) {
        // this trip's march is over — fold its segment counters (seg_counters = [tail | sample | emitted | cursor | tail back] x PN_SEGS) into
        // the records and clear them for the next trip
        int* tail_c = seg_counters + lane * PN_SEG_STRIDE;
        int* samp_c = tail_c + PN_SEGS * PN_SEG_STRIDE;
        int* emit_c = samp_c + PN_SEGS * PN_SEG_STRIDE;
        int* curs_c = emit_c + PN_SEGS * PN_SEG_STRIDE;
        int* back_c = curs_c + PN_SEGS * PN_SEG_STRIDE;
        int tl = *tail_c + *back_c, em = *emit_c;
        *tail_c = 0; *samp_c = 0; *emit_c = 0; *curs_c = 0; *back_c = 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { tl += __shfl_xor(tl, o); em += __shfl_xor(em, o); }
        if (lane == 0) { if (tail_diag) *tail_diag = tl; if (trip) trip->n_emitted = em; }
    }
    if (!next) return;
    if (g_next) {
        // 64 groups per round, running sums carried in (uniform) registers
        int alive_run = 0, slot_run = 0, live = 0, step0 = 1;
        for (uint32_t b0 = 0; b0 < n_groups; b0 += 64) {
            const uint32_t b = b0 + (uint32_t)lane;
            int cnt = 0, nstep = 0, stepb = 0;
            if (b < n_groups) {
                const PnGroup g = g_cur[b];
                cnt = (n_groups == 1) ? sum : group_cnt[b];
                if (n_groups > 1) group_cnt[b] = 0;
                stepb = g.step_base + g.n_step;
                const uint32_t rays_b = min(group_rays, N_rays - b * group_rays);  // N_b
                const bool over = cnt <= 0 || (uint32_t)stepb >= max_steps || g.n_step == 0;
                nstep = over ? 0 : max(min((int)(rays_b / (uint32_t)cnt), 8), 1);
            }
            const int slots = cnt * nstep;
            int a_inc = cnt, s_inc = slots;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int ua = __shfl_up(a_inc, o), us = __shfl_up(s_inc, o);
                if (lane >= o) { a_inc += ua; s_inc += us; }
            }
            if (b < n_groups) g_next[b] = PnGroup{alive_run + a_inc - cnt, nstep, slot_run + s_inc - slots, stepb};
            if (b == 0) step0 = nstep;
            alive_run += __shfl(a_inc, 63);
            slot_run += __shfl(s_inc, 63);
            int lv = nstep > 0 ? cnt : 0;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) lv += __shfl_xor(lv, o);
            live += lv;
        }
        step0 = __shfl(step0, 0);
        if (lane == 0) {
            // rays of groups that ran into max_steps stay listed until the next composite retires them; the frame is over when no group marches on
            const bool done = live <= 0;
            next->n_alive = done ? 0 : sum;
            next->n_step = done ? 1 : max(step0, 1);  // informational with groups (every kernel reads the group records)
            next->step_base = trip->step_base + trip->n_step;
            next->dense = (dense_trips && !done) ? 1 : 0;
            next->n_samples = (dense_trips && !done) ? slot_run : 0;
            next->n_emitted = 0;
        }
    } else if (lane == 0) {
        const int step = trip->step_base + trip->n_step;
        const bool done = (sum <= 0) || ((uint32_t)step >= max_steps);
        next->n_alive = done ? 0 : sum;
        next->n_step = done ? 1 : max(min((int)(N_rays / (uint32_t)sum), 8), 1);
        next->step_base = step;
        // dense trip (see trip_is_dense): the list is the identity over all slots; n_emitted = -1 marks a list trip
        // every trip after the first is dense: its rays are the ones that found a sample before (n_step == 1 then means more than half of
        // all rays are still alive — they will mostly fill their single slot too)
        const bool dense = dense_trips && !done;
        next->dense = dense ? 1 : 0;
        next->n_samples = dense ? sum * next->n_step : 0;
        next->n_emitted = 0;
        // the rays max_steps ended the loop on (renderer.py:836 leaves them alive); an empty trip hands on what it found in its own record
        next->n_left = sum > 0 ? (done ? sum : 0) : trip->n_left;
    }
}

// Block c moves the survivors of chunk c to out[prefix(c) ...], keeping order (== rays_alive[rays_alive >= 0]).
// Block 0 also publishes the total and, in frame-driver mode, the next trip's record (renderer.py:839-846,891).
// Ray groups (g_next != nullptr, see PnGroup): chunk 0's first wave also writes the next trip's group records from this trip's records and the
// per-group survivor counts of k_composite — N_b // n_alive_b per group, exclusive sums for the first alive position and the first sample slot.
__global__ void __launch_bounds__(256) k_compact(const int* __restrict__ in, uint32_t n_arg, const int* __restrict__ chunk_counts,
                                                 int* __restrict__ out, int* n_out, PnTrip* trip, PnTrip* next, uint32_t N_rays,
                                                 uint32_t max_steps, int dense_trips, int* seg_counters, int* tail_diag,
                                                 const PnGroup* __restrict__ g_cur, PnGroup* __restrict__ g_next, int* group_cnt, uint32_t group_rays,
                                                 uint32_t n_groups) {
    __shared__ int red[4];
    __shared__ int woff[4];
    const uint32_t n = trip ? (uint32_t)trip->n_alive : n_arg;
    const uint32_t n_chunks = (n + 255) / 256;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    // bounded grid (see k_march): chunks are dealt round-robin; chunk 0 always runs once (it publishes the totals even when n == 0)
    for (uint32_t c = blockIdx.x; c == 0 || c * 256 < n; c += gridDim.x) {
        // prefix over earlier chunks (and, for chunk 0, the grand total)
        const uint32_t upto = (c == 0) ? n_chunks : c;
        int part = 0;
        for (uint32_t k = threadIdx.x; k < upto; k += 256) part += chunk_counts[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
        if (lane == 0) red[wid] = part;
        __syncthreads();
        const int sum = red[0] + red[1] + red[2] + red[3];
        const int offset = (c == 0) ? 0 : sum;
        if (c == 0 && wid == 0) {
            if (n_out && lane == 0) *n_out = sum;
            trip_epilogue(lane, sum, trip, next, N_rays, max_steps, dense_trips, seg_counters, tail_diag, g_cur, g_next, group_cnt, group_rays, n_groups);
        }
        const uint32_t i = c * 256 + threadIdx.x;
        const int v = (i < n) ? in[i] : -1;
        const bool keep = v >= 0;
        const unsigned long long m = __ballot(keep);
        const int rank = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) woff[wid] = __popcll(m);
        __syncthreads();
        int wbase = 0;
        for (int w = 0; w < wid; w++) wbase += woff[w];
        if (keep) out[offset + wbase + rank] = v;
        __syncthreads();  // red / woff are reused by the next chunk
    }
}

// ---- composite + stable compaction + end-of-trip bookkeeping in ONE launch (frame driver of the deformed render).
// kernel_composite_rays (raymarching.cu:827-923) followed by rays_alive = rays_alive[rays_alive >= 0] (renderer.py:887) is a scan: where a
// survivor goes depends on how many rays before it survive.  Two launches did that through per-chunk counts in memory (k_composite, k_compact);
// here workgroup b takes the chunks b, b + grid, ... of 256 * R consecutive alive positions, composites them, publishes each chunk's survivor
// count as (trip tag << 16 | count) and then sums the words of ALL chunks before its own, polling those that do not carry this trip's tag yet.
// No chain: a chunk waits for the composites of earlier chunks, never for their sums, so the launch lasts one composite plus one gather of at
// most n_chunks words.  (A decoupled look-back over 64 descriptors at a time was tried first: with every chunk of the trip in flight at once the
// prefixes have nothing to propagate from — 10 dependent steps on trip 0 — and 1 250 returning ticket / completion atomics on one address at
// 11.4 ns each: 174 us against 25 for the two launches.)  Progress: a chunk depends on lower-numbered chunks only and every workgroup takes its
// chunks in ascending order, so the launch finishes whenever ALL its workgroups can be resident at the same time — which is why the grid is bounded
// (PN_CC_GRID, 512 workgroups of 4 waves: three render lanes' composites together stay below the 8 192 wave slots of the part).  Rounds 2-3 launched
// one workgroup per chunk (2 500 on a frame's first trip) on the assumption that workgroups start in index order; the eight XCDs dispatch their shares
// independently, and two first-trip composites of different lanes could each fill an XCD with pollers waiting for a chunk whose workgroup had no slot
// on the other one: a deadlock, seen (as the poll guard's flag 16) in bench.py --config stress.  A workgroup's later chunks add only the words
// behind its previous chunk to the prefix it already has: 512 words per chunk instead of all before it.
// The tag makes last trip's words read as "not written yet"; the words are cleared once per frame (k_frame_prologue).  The workgroup of the
// trip's LAST chunk has the grand total and runs trip_epilogue: every earlier chunk has published its count, i.e. finished its composites and
// its per-group survivor atomics.  R = 1 alive position per thread (2 / 4 on a frame's first trip: 21.4 / 27.9 us against 20.0).
__global__ void __launch_bounds__(256) k_composite_compact(float T_thresh, const int* __restrict__ cur, int* __restrict__ nxt, float* rays_t,
                                                           const float* __restrict__ sigmas, const float* __restrict__ rgbs, const float* __restrict__ deltas,
                                                           float* weights_sum, float* depth, float* image, PnTrip* trip, PnTrip* next,
                                                           unsigned* words, uint32_t tag, uint32_t N_rays, uint32_t max_steps, int dense_trips,
                                                           int* seg_counters, int* tail_diag, const PnGroup* __restrict__ g_cur, PnGroup* __restrict__ g_next,
                                                           int* group_cnt, uint32_t group_rays, uint32_t n_groups, int* err_flag, uint32_t poll_cap) {
    constexpr int R = 1;  // alive positions per thread (the loops over them stay: the compiled kernel is the one measured)
    __shared__ int s_wcnt[4], s_part[4];
    const uint32_t n_alive = (uint32_t)trip->n_alive, n_step_trip = (uint32_t)trip->n_step;
    const uint32_t CH = 256u * R;
    const uint32_t n_chunks = max((n_alive + CH - 1) / CH, 1u);  // chunk 0 always runs: somebody has to write the next trip's record
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    bool have_prev = false;
    uint32_t c_prev = 0;
    int excl_prev = 0, count_prev = 0;
    for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        // ---- composite: R consecutive alive positions per thread
        int keep[R];
        int mine = 0;
#pragma unroll
        for (int r = 0; r < R; r++) {
            const uint32_t n = c * CH + threadIdx.x * R + r;
            bool alive = false;
            int grp = -1, index = -1;
            if (n < n_alive) {
                index = cur[n];
                uint32_t n_step = n_step_trip, slot0;
                ray_slots(g_cur, group_rays, index, n, n_step, slot0);
                if (g_cur) grp = (int)((uint32_t)index / group_rays);
                // n_step == 0: the ray's group has reached max_steps — the batch's loop is over (renderer.py:836), the ray is dropped
                if (n_step != 0) alive = composite_one(index, slot0, n_step, T_thresh, rays_t, sigmas, rgbs, deltas, weights_sum, depth, image);
            }
            keep[r] = alive ? index : -1;
            mine += alive ? 1 : 0;
            if (n_groups > 1) {  // survivors per group: one atomic per run of equal group ids (the positions of the 64 lanes are R apart, still sorted)
                const unsigned long long am = __ballot(alive);
                const int prev = __shfl_up(grp, 1);
                const bool head = lane == 0 || grp != prev;
                const unsigned long long hm = __ballot(head);
                if (head && grp >= 0) {
                    const unsigned long long above = lane == 63 ? 0ull : hm & ~((2ull << lane) - 1ull);
                    const unsigned long long upto = above ? ((1ull << (__ffsll((long long)above) - 1)) - 1ull) : ~0ull;
                    const int cc = (int)__popcll(am & upto & ~((1ull << lane) - 1ull));
                    // returning form: the value has to be back before this chunk's count is published below (the epilogue reads the counters once
                    // every count is out); a release fence would do the same by writing this XCD's whole L2 back
                    if (cc) { const int old = atomicAdd(group_cnt + grp, cc); asm volatile("" ::"v"(old)); }
                }
            }
        }
        // ---- this chunk's survivor count; exclusive prefix of the thread inside the chunk
        int inc = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(inc, o);
            if (lane >= o) inc += u;
        }
        if (lane == 63) s_wcnt[wid] = inc;
        __syncthreads();
        const int count = s_wcnt[0] + s_wcnt[1] + s_wcnt[2] + s_wcnt[3];
        int tbase = inc - mine;
        for (int w = 0; w < wid; w++) tbase += s_wcnt[w];
        // relaxed, device scope: the word IS the message (the XCDs' L2s are not coherent with each other: release / acquire at device scope
        // write back and invalidate whole caches — with them this kernel took 185 us on trip 0)
        if (threadIdx.x == 0) __hip_atomic_store(words + c, (tag << 16) | (unsigned)count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // ---- survivors of all chunks before this one: the words of the chunks behind this workgroup's previous chunk, on top of what it had there
        int part = 0;
        for (uint32_t k = (have_prev ? c_prev + 1 : 0u) + threadIdx.x; k < c; k += 256) {
            unsigned w;
            uint32_t polls = 0;
            do {
                w = __hip_atomic_load(words + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                // never seen: a word that stays unwritten would mean the dispatcher started this workgroup before a lower-numbered one that has
                // no slot yet.  Rather than hang the GPU, give up after ~a second, flag the frame (err bit 16) and carry on with garbage.
                if (++polls > poll_cap) { if (err_flag) atomicOr(err_flag, 16); w = tag << 16; }
            } while ((w >> 16) != tag);
            part += (int)(w & 0xFFFFu);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
        if (lane == 0) s_part[wid] = part;
        __syncthreads();
        const int excl = (have_prev ? excl_prev + count_prev : 0) + s_part[0] + s_part[1] + s_part[2] + s_part[3];
        have_prev = true; c_prev = c; excl_prev = excl; count_prev = count;
        // ---- survivors in order
        int w0 = excl + tbase;
#pragma unroll
        for (int r = 0; r < R; r++)
            if (keep[r] >= 0) nxt[w0++] = keep[r];
        if (c == n_chunks - 1 && wid == 0)
            trip_epilogue(lane, excl + count, trip, next, N_rays, max_steps, dense_trips, seg_counters, tail_diag, g_cur, g_next, group_cnt, group_rays, n_groups);
        __syncthreads();  // s_wcnt / s_part are rewritten by the next chunk
    }
}
