// Records shared by the trip kernels and the frame driver of the render unit (pn_render_ops.hip): the trip and ray-group records, the per-frame
// device record, the march's launch record and side-table buffers, the segmented append lists and the tail pass's hand-over entry.
#pragma once
#include "pn_common.h"

// Device-side record driving one loop trip of rund_cuda (nerf/renderer.py:836-891).
struct PnTrip {
    // written by the previous trip's compaction (trip 0: k_frame_prologue), read-only while this trip's kernels run
    int n_alive;    // rays entering this trip
    int n_step;     // max(min(N // n_alive, 8), 1)
    int step_base;  // renderer's `step` before this trip
    int dense;      // see below
    int n_left;     // rays the loop ended on: alive behind the trip that took `step` to max_steps (renderer.py:836), carried through the empty
                    // trips behind it; 0 while the loop goes on or when it ended because no ray was left (n_alive is 0 in both cases)
    int pad0[27];
    // counters the march updates with atomics: a cache line of their own, so that the waves reading the fields above (every wave's first
    // instruction) do not queue behind them
    int n_samples;  // entries of the sample list the network kernel reads (list trips: filled by atomics; dense trips: n_alive * n_step)
    int n_emitted;  // dense trips only: samples really emitted (statistics)
    int pad1[30];
};
static_assert(sizeof(PnTrip) == 256, "two cache lines");
// Dense trips (frame driver of the deformed render, every trip after the first): there nearly every alive ray fills all its n_step slots
// (measured on the chair: 98-99 %), so the sample list is the identity over the n_alive * n_step slots — written by the march without the
// returning atomic a compact list costs every wave (one more dependent memory round trip at the end of a latency-bound kernel: -24 % on
// trip 0's k_march without it) — and the few unfilled slots are zero-filled and run through the network as well; composite never reads
// them (their delta is 0).  The compaction kernel presets n_samples for such a trip.
__device__ __forceinline__ bool trip_is_dense(const PnTrip* t) { return t->dense != 0; }

// Ray groups (pn_render_opts::ray_batch > 0): the frame rendered "in ray batches of B" (max_ray_batch, get_opts.py:24; the staging loop of
// renderer.py:562-576) WITHOUT one launch chain per batch.  Rays are independent, so what a batch changes is only its own trip schedule: batch
// b = rays [b B, (b + 1) B) marches n_step_b = max(min(N_b // n_alive_b, 8), 1) samples per ray and trip, stops when none of ITS rays is alive or
// ITS step count reaches max_steps.  Stable compaction keeps the alive list sorted by ray id, so the batches are contiguous runs of it; every
// trip kernel handles all of them in one launch and looks up, per ray, its group's (first alive position, n_step, first sample slot).  One
// record per group and trip parity, written by the previous trip's compaction (trip 0: k_frame_prologue).  The sample slots of a trip stay dense:
// slot_base is the running sum of n_alive_b * n_step_b.  n_step == 0 marks a group that ran into max_steps: composite retires its rays.
struct PnGroup {
    int alive_base, n_step, slot_base, step_base;
};
// n_step / first sample slot of the ray at alive position n (ray id `index`); groups == nullptr: one schedule for all rays (slot0 = n * n_step)
__device__ __forceinline__ void ray_slots(const PnGroup* __restrict__ groups, uint32_t group_rays, int index, uint32_t n, uint32_t& n_step, uint32_t& slot0) {
    if (groups) {
        const PnGroup g = groups[(uint32_t)index / group_rays];
        n_step = (uint32_t)g.n_step;
        slot0 = (uint32_t)g.slot_base + (n - (uint32_t)g.alive_base) * (uint32_t)g.n_step;
    } else {
        slot0 = n * n_step;
    }
}

// Per-frame device record of the frame drivers (pn_render_deformed / pn_render_static).
struct PnFrameDev {
    float aabb[6];      // bbmin = aabb, bbmax = aabb + 3   (aabb = cat(bbmin, bbmax), renderer.py:796)
    int resolution[4];  // [3] = n_grid
    int err;
    int unfinished;     // rays left alive by fixed-trip renders since the last reset, summed (staged batches are checked once per frame)
    int trips_run;      // loop trips the last render (or continuation) on this workspace has enqueued: written by its epilogue, so that it is
                        // also right after a HIP-graph REPLAY, which the host-side bookkeeping never sees
    int nb_alloc;       // candidate-list entries handed out so far (k_frame_prologue bumps it once per 32 cells; cleared by k_frame_tables)
    int fused_trips;    // trips the last k_trips_fused launch ran (pn_trips_fused.h); k_frame_finish adds them to trips_run and clears the field
    // summary of the trip records, written by k_frame_finish (the host reads this record instead of every trip's):
    int stat_trips;     // trips that had rays
    int alive_at_exit;  // rays alive behind the last trip enqueued (the static render: + the rays max_steps ended the loop on, PnTrip::n_left)
    int pad0;
    long long stat_samples;  // samples marched (dense trips: emitted; list trips: listed)
    // cells [ip_lo, ip_hi] per axis hold every integration point (k_frame_tables); with --cut the search grid spans +-bound (67^3 cells on the trex option
    // set) while the points fill a fortieth of it: k_frame_prologue builds candidate lists for the cells within one cell of that box only
    int ip_lo[3], ip_hi[3];
    int pad1[2];
};

struct MarchSide {  // device buffers of the side tables
    int *nb_cnt, *nb_bgn, *nb_cursor;  // [n_grid_max + 1] op-level build only (count -> scan -> fill); the frame driver allocates list space by bumping a counter
    int2* nb_rng;                       // [n_grid_max]
    float4* nb;                         // [nb_capacity]
    float* rec;                         // [n_vtx * 44]
    int nb_capacity;
};

// A ray handed from k_march to k_march_tail, with everything the tail pass needs to go on: fetching the slot's ray through rays_alive ->
// rays_o / rays_d / fars again cost the tail three dependent memory round trips per ray — half of a typical tail ray's time (phase clocks).
struct __attribute__((aligned(16))) TailEntry {
    int n;            // alive slot
    float t, last_t;  // pnm3::RayState
    int step;
    float ox, oy, oz, dx;
    float dy, dz, rdx, rdy;
    float rdz, far;
    int slot0, n_step;  // first sample slot and sample budget of the ray in this trip (ray_slots)
};
static_assert(sizeof(TailEntry) == 64, "four 16-byte parts");

struct MarchIO {
    uint32_t n_alive, n_step;
    const int* rays_alive;
    float *xyzs, *dirs, *deltas;
    const float* noises;
    // frame-driver mode (trip != nullptr): counts come from device memory, valid sample slots are appended to `list`
    PnTrip* trip;
    int* list;
    float* t_resume;  // optional [n_alive]: written by k_march_skip, read by k_march (pn_march_skip.h: skip_empty_cells)
    // optional tail pass: rays unfinished after `max_rounds` windows in k_march are appended here (counters zeroed by the caller)
    struct TailEntry* tail;
    int* tail_counts;   // segmented (see PN_SEGS): rays with a long way to go, appended from the front of the segment's region
    int* tail_back;     // segmented: the others, appended from the back (the tail pass starts the long ones first)
    int* tail_cursors;  // segmented: next unprocessed entry (the tail pass hands its rays out dynamically)
    int tail_seg_cap;
    int max_rounds;
    // optional (trip 0 of the frame driver): k_march_skip lists the alive slots that still have something to march — nine rays in ten miss the
    // object's bounding box or run out of it inside the IP-free cells — and k_march walks that list instead of all n_alive slots
    int* active;
    int* active_counts;  // segmented
    int active_seg_cap;
    // frame-driver mode, list trips: the sample list is appended in segments (list_seg, samp_counts) and packed into `list` by k_list_pack;
    // dense trips: emit_parts collects the number of samples really emitted
    int* list_seg;
    int* samp_counts;
    int list_seg_cap;
    int* emit_parts;
    // optional: one bit per search cell, set when the cell has candidates (frame driver); k_march_skip keeps it in LDS when launched with
    // cell_bits_words * 4 bytes of dynamic shared memory
    const uint32_t* cell_bits;
    int cell_bits_words;
    // optional (with cell_bits): the cells within one cell of a cell with candidates, and where k_march_skip writes each ray's shortened end
    // (pn_march_skip.h: ray_end_of_candidates); the march kernels then run with MarchParams::fars = fars_eff
    const uint32_t* cell_bits2;
    float* fars_eff;
    // optional (frame driver with ray groups, see PnGroup): this trip's group records
    const PnGroup* groups;
    uint32_t group_rays;
    int lane_per_ray;           // k_march: one lane per ray instead of eight (the throughput form of a frame's first trip)
    int dda_start, hop_budget;  // k_march_skip: restart the hop chain just before the first cell with candidates; hops before a ray is handed on (pn_march_skip.h)
    // optional (--cut frames): the region map of pn_march_skip.h (region_dda) — one bit per 8^3-voxel block of the top cascade level, set when a point of
    // the region can meet an occupied voxel on any level or the cut box (k_frame_prologue); k_march_skip keeps it in LDS
    const uint32_t* grid_regions;
    int grid_regions_words;
    int grid_regions_R;   // regions per axis: H / 8 (8^3-voxel regions) or H / 4
};

// Append lists are SEGMENTED: PN_SEGS independent (counter, region) pairs, every counter on a cache line of its own, the producer picking
// its segment from its workgroup / wave id.  Atomics on ONE address are served one at a time by the memory side — measured 11.4 ns each on
// gfx950, returning or not, however many waves issue them (tools/calib_atomic.hip: 5 000 waves x 1 atomic = +50 us) — and the march used one
// per wave (sample list) or per ray (tail list): that serialisation, not ALU work or memory latency, was 50-120 us of every march launch.
// Consumers need no prefix over the segments: workgroup b (wave w) takes segment b % PN_SEGS (w % PN_SEGS) and strides over its entries.
#define PN_SEGS 64
#define PN_SEG_STRIDE 32  // ints between counters: 128 B
__device__ __forceinline__ int seg_count(const int* counts, int seg) {
    return __hip_atomic_load(counts + seg * PN_SEG_STRIDE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// entries a segment must hold when its producers are the workgroups (32 rays each) / waves (64 rays) with id % PN_SEGS == segment
// workers (workgroups or waves) whose id % PN_SEGS == seg, out of `total` (launches of segment consumers have at least PN_SEGS workers)
__device__ __forceinline__ int seg_workers(int total, int seg) { return max((total - seg + PN_SEGS - 1) / PN_SEGS, 1); }
// ... or, in the one-lane-per-ray form of k_march (G = 1), 256-ray chunks dealt by chunk % PN_SEGS: a segment then gets up to
// ceil(ceil(n / 256) / PN_SEGS) * 256 entries (640 000 rays: 10 240, more than the 64-ray form's 10 112 — round-3 advisor finding); the larger of the two
static uint32_t seg_cap_for(uint32_t n_rays) {
    const uint32_t by64 = (pn_div_up(pn_div_up(n_rays, 64), PN_SEGS) + 1) * 64, by256 = pn_div_up(pn_div_up(n_rays, 256), PN_SEGS) * 256 + 64;
    return std::max(by64, by256);
}
