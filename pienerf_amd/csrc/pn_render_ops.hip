// Ray-side kernels of the render path + the whole-frame driver (gfx950).
// Built with -ffp-contract=off (see pn_march_math.h).  Reference citations (raymarching.cu, nerf/...) name files of the reference implementation.
// The unit in the order it is included (every header below belongs to this translation unit alone):
//   pn_render_records.h   records shared by the trip kernels and the driver (PnTrip, PnGroup, PnFrameDev, MarchIO, MarchSide, PN_SEGS, TailEntry)
//   pn_cell_hash.h        spatial hash of the integration points and its scans
//   pn_side_tables.h      op-level build of the march's side tables
//   pn_march_kernels.h    k_march_skip, k_march, k_march_tail, k_march_static_trip (pn_march_skip.h and pn_march_window.h over pn_march_seq.h; pn_march_static.h)
//   pn_composite.h        composite_one, k_composite
//   pn_compact.h          k_compact, trip_epilogue, k_composite_compact, k_list_pack
//   pn_frame_kernels.h    pn_frame, k_frame_tables, k_frame_prologue, k_frame_finish (behind pn_trips_fused.h: the fused trip launch)
// then the op-level entry points that share these kernels with the driver, and the driver with the pn_render_* / pn_frame_* entry points.
// The ops the driver shares nothing with are a unit of their own (pn_ray_ops.hip).
#include <float.h>

#include <vector>

#include "pn_render_records.h"
#include "pn_cell_hash.h"
#include "pn_side_tables.h"
#include "pn_march_kernels.h"
#include "pn_composite.h"
#include "pn_compact.h"
#include "pn_frame_kernels.h"

thread_local char pn_err_buf[512] = {0};

// ------------------------------------------------------------------------------------------------ library-wide entries (beside the buffer they report)
extern "C" int pn_device_cu_count(void) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess) return -1;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return -1;
    return n;
}

extern "C" int pn_stream_create_cu_mask(uint32_t total_cu, uint32_t first_cu, uint32_t n_cu, int invert, void** stream_out) {
    PN_REQUIRE(stream_out && total_cu > 0 && total_cu <= 1024 && n_cu > 0 && first_cu + n_cu <= total_cu);
    uint32_t mask[32];
    const uint32_t words = (total_cu + 31) / 32;
    for (uint32_t w = 0; w < words; w++) mask[w] = 0;
    for (uint32_t i = 0; i < total_cu; i++) {
        const bool in = i >= first_cu && i < first_cu + n_cu;
        if (in != (invert != 0)) mask[i / 32] |= 1u << (i % 32);
    }
    hipStream_t s = nullptr;
    PN_HIP_CHECK(hipExtStreamCreateWithCUMask(&s, words, mask));
    *stream_out = (void*)s;
    return PN_OK;
}

extern "C" int pn_stream_destroy(void* stream) {
    PN_REQUIRE(stream);
    PN_HIP_CHECK(hipStreamDestroy((hipStream_t)stream));
    return PN_OK;
}

extern "C" const char* pn_version(void) { return "pienerf_hip 0.1.0 gfx950"; }
extern "C" const char* pn_last_error(void) { return pn_err_buf; }
extern "C" int pn_pnts_in_grids(int n_vtx, int n_grid, const float* pnts, const float* bbmin, float hgs, const int* resolution, int* pig_cnt,
                                int* pig_bgn, int* pig_idx, int* err_flag, void* stream) {
    PN_REQUIRE(n_vtx > 0 && n_grid > 0 && pnts && bbmin && resolution && pig_cnt && pig_bgn && pig_idx);
    int* cursor = nullptr;
    hipStream_t st = (hipStream_t)stream;
    PN_HIP_CHECK(hipMallocAsync((void**)&cursor, sizeof(int) * (size_t)n_grid, st));
    int rc = pig_build(n_vtx, n_grid, nullptr, pnts, bbmin, hgs, resolution, pig_cnt, pig_bgn, pig_idx, cursor, err_flag, st);
    PN_HIP_CHECK(hipFreeAsync(cursor, st));
    return rc;
}

extern "C" int pn_march_set_skip_dda(int on) {
    PN_REQUIRE(on >= -1 && on <= 1);
    g_skip_dda_override = on;
    return PN_OK;
}
extern "C" int pn_march_set_tail_rounds(int rounds) {
    PN_REQUIRE(rounds >= 0);
    g_tail_rounds_override = rounds;
    return PN_OK;
}

extern "C" int pn_march_rays_quadratic_bending(const int* pig_cnt, const int* pig_bgn, const int* pig_idx, int n_vtx, int n_grid,
                                               const float* p_def, const float* p_ori, const float* F_IP, const float* dF_IP, int max_iter_num,
                                               const float* bbmin, const float* bbmax, float hgs, const int* resolution, int num_seek_IP,
                                               float IP_dx, int cut, const float* cut_bounds, uint32_t n_alive, uint32_t n_step,
                                               const int* rays_alive, const float* rays_t, const float* rays_o, const float* rays_d, float bound,
                                               float dt_gamma, uint32_t max_steps, uint32_t C, uint32_t H, const uint8_t* grid, const float* nears,
                                               const float* fars, float* xyzs, float* dirs, float* deltas, const float* noises, int* err_flag,
                                               void* stream) {
    (void)nears;
    PN_REQUIRE(pig_cnt && pig_bgn && pig_idx && p_def && p_ori && F_IP && dF_IP && bbmin && bbmax && resolution);
    PN_REQUIRE(rays_alive && rays_t && rays_o && rays_d && grid && fars && xyzs && dirs && deltas);
    PN_REQUIRE(num_seek_IP >= 1 && num_seek_IP <= 3);
    PN_REQUIRE(!cut || cut_bounds);
    PN_REQUIRE(C >= 1 && C <= 8 && H > 0 && n_step >= 1 && n_vtx > 0 && n_grid > 0);
    if (n_alive == 0) return PN_OK;
    hipStream_t st = (hipStream_t)stream;
    // side tables are rebuilt from the caller's spatial hash on every call (stream-ordered pool allocations)
    MarchSide s;
    s.nb_capacity = 27 * n_vtx;
    char* pool = nullptr;
    const size_t ints = ((size_t)n_grid + 1) * 5 * sizeof(int), nbb = (size_t)s.nb_capacity * sizeof(float4), recb = (size_t)n_vtx * PN_REC_FLOATS * sizeof(float);
    const size_t off_nb = (ints + 255) & ~(size_t)255, off_rec = (off_nb + nbb + 255) & ~(size_t)255;
    const size_t off_res = (off_rec + recb + 255) & ~(size_t)255;
    const uint32_t tail_cap = seg_cap_for(n_alive);
    const size_t tail_ctr = (size_t)3 * PN_SEGS * PN_SEG_STRIDE * sizeof(int);  // front counters, back counters, cursors
    const size_t off_tail = (off_res + (size_t)n_alive * sizeof(float) + 255) & ~(size_t)255;  // [segment counters | tail entries]
    PN_HIP_CHECK(hipMallocAsync((void**)&pool, off_tail + tail_ctr + (size_t)PN_SEGS * tail_cap * sizeof(TailEntry), st));
    PN_HIP_CHECK(hipMemsetAsync(pool + off_tail, 0, tail_ctr, st));
    s.nb_cnt = (int*)pool; s.nb_bgn = s.nb_cnt + n_grid + 1; s.nb_cursor = s.nb_bgn + n_grid + 1; s.nb_rng = (int2*)(s.nb_cursor + n_grid + 1);
    s.nb = (float4*)(pool + off_nb); s.rec = (float*)(pool + off_rec);
    int rc = march_side_build(s, n_vtx, n_grid, nullptr, resolution, pig_cnt, pig_bgn, pig_idx, p_def, p_ori, F_IP, dF_IP, num_seek_IP, err_flag, st);
    if (rc == PN_OK) {
        pnm::MarchParams a = make_march_params(pig_cnt, pig_bgn, pig_idx, n_vtx, n_grid, p_def, p_ori, F_IP, dF_IP, max_iter_num, bbmin, bbmax, hgs,
                                               resolution, num_seek_IP, IP_dx, cut, cut_bounds, rays_t, rays_o, rays_d, bound, dt_gamma, max_steps,
                                               C, H, grid, fars, err_flag);
        pnm2::March2Tables tb{s.nb_rng, s.nb, (const float4*)s.rec};
        int* const tail_ctrs = (int*)(pool + off_tail);
        MarchIO io{};
        io.n_alive = n_alive; io.n_step = n_step; io.rays_alive = rays_alive;
        io.xyzs = xyzs; io.dirs = dirs; io.deltas = deltas; io.noises = noises;
        io.t_resume = (float*)(pool + off_res);
        io.tail = (TailEntry*)(pool + off_tail + tail_ctr);
        io.tail_counts = tail_ctrs; io.tail_back = tail_ctrs + PN_SEGS * PN_SEG_STRIDE; io.tail_cursors = tail_ctrs + 2 * PN_SEGS * PN_SEG_STRIDE;
        io.tail_seg_cap = (int)tail_cap;
        io.max_rounds = (int)march_tail_rounds();
        if (io.t_resume) k_march_skip<<<pn_div_up(n_alive, 256), 256, 0, st>>>(a, tb, io);
        launch_march(num_seek_IP, pn_div_up(n_alive, 32), std::max(std::min(pn_div_up(n_alive, 4), 2048u), (uint32_t)PN_SEGS / 4), st, a, tb, io);
    }
    PN_HIP_CHECK(hipFreeAsync(pool, st));
    if (rc) return rc;
    PN_LAUNCH_CHECK();
    return PN_OK;
}

extern "C" int pn_composite_rays(uint32_t n_alive, uint32_t n_step, float T_thresh, int* rays_alive, float* rays_t, const float* sigmas,
                                 const float* rgbs, const float* deltas, float* weights_sum, float* depth, float* image, void* stream) {
    if (n_alive == 0) return PN_OK;  // empty tensors have null data pointers
    PN_REQUIRE(rays_alive && rays_t && sigmas && rgbs && deltas && weights_sum && depth && image && n_step >= 1);
    k_composite<<<pn_div_up(n_alive, 256), 256, 0, (hipStream_t)stream>>>(n_alive, n_step, T_thresh, rays_alive, rays_t, sigmas, rgbs, deltas,
                                                                         weights_sum, depth, image, nullptr, nullptr, nullptr, 0, nullptr);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

extern "C" uint32_t pn_compact_scratch_ints(uint32_t n) { return pn_div_up(n, 256) + 1; }

extern "C" int pn_compact_rays(const int* rays_alive, uint32_t n, int* out, int* n_out, int* scratch, void* stream) {
    PN_REQUIRE(n_out);
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) { PN_HIP_CHECK(hipMemsetAsync(n_out, 0, sizeof(int), st)); return PN_OK; }  // empty tensors have null data pointers
    PN_REQUIRE(rays_alive && out && scratch);
    const uint32_t chunks = pn_div_up(n, 256);
    k_chunk_count<<<chunks, 256, 0, st>>>(rays_alive, n, scratch);
    k_compact<<<chunks, 256, 0, st>>>(rays_alive, n, scratch, out, n_out, nullptr, nullptr, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

// ------------------------------------------------------------------------------------------------ whole frame

extern "C" int pn_frame_create(pn_frame** out, uint32_t max_rays, uint32_t max_vtx, uint32_t max_grid_cells) {
    PN_REQUIRE(out && max_rays > 0 && max_vtx > 0 && max_grid_cells > 0);
    pn_frame* f = new pn_frame();
    memset(f, 0, sizeof(*f));
    f->max_rays = max_rays; f->max_vtx = max_vtx; f->max_cells = max_grid_cells;
    const size_t N = max_rays;
#define PN_ALLOC(ptr, bytes) PN_HIP_CHECK(hipMalloc((void**)&(ptr), (bytes)))
    PN_ALLOC(f->nears, N * 4); PN_ALLOC(f->fars, N * 4); PN_ALLOC(f->rays_t, N * 4);
    // sample slots: one per ray for the per-trip launches, 64 per wave of a fused launch (pn_trips_fused.h: one workgroup per CU) + one per position of a
    // whole-frame launch's first trip — the larger of the two
    {
        int dev_id = 0, cus = 0;
        PN_HIP_CHECK(hipGetDevice(&dev_id));
        PN_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev_id));
        f->fused_blocks = (uint32_t)std::min(std::max(cus, 1), 1024);
    }
    f->blist_cap = (uint32_t)(N / 8 + 64 + (size_t)(f->fused_blocks + 1) * 64);  // n_active <= N / 8, + one partial chunk per workgroup (pn_trips_fused.h)
    const size_t NS = N + (size_t)f->fused_blocks * PN_FUSED_WAVES * 64 + f->blist_cap;  // (per-ray slots | the fused launch's waves' slots | its first-trip positions)
    PN_ALLOC(f->xyzs, NS * 12); PN_ALLOC(f->dirs, NS * 12); PN_ALLOC(f->deltas, NS * 8); PN_ALLOC(f->sigmas, NS * 4); PN_ALLOC(f->rgbs, NS * 12);
    PN_ALLOC(f->fused_ctl, (size_t)PN_FUSED_CTL_INTS * 4);
    PN_HIP_CHECK(hipMemset(f->fused_ctl, 0, (size_t)PN_FUSED_CTL_INTS * 4));
    PN_ALLOC(f->fused_clocks, 16 * sizeof(unsigned long long));
    PN_HIP_CHECK(hipMemset(f->fused_clocks, 0, 16 * sizeof(unsigned long long)));
    f->fused_first = -1;
    PN_ALLOC(f->t_resume, N * 4);
    PN_ALLOC(f->blist, (size_t)f->blist_cap * 8);
    PN_ALLOC(f->strag, (size_t)f->blist_cap * 16);
    PN_ALLOC(f->acc_image, N * 12);
    PN_ALLOC(f->alive_a, N * 4); PN_ALLOC(f->alive_b, N * 4); PN_ALLOC(f->list, N * 4); PN_ALLOC(f->chunk_counts, (N / 256 + 4) * 4);
    PN_ALLOC(f->pig_cnt, (size_t)max_grid_cells * 4); PN_ALLOC(f->pig_bgn, (size_t)max_grid_cells * 4);
    PN_ALLOC(f->pig_cursor, (size_t)max_grid_cells * 4); PN_ALLOC(f->pig_idx, (size_t)max_vtx * 4);
    PN_ALLOC(f->side.nb_rng, ((size_t)max_grid_cells + 1) * sizeof(int2));
    f->side.nb_capacity = 27 * (int)max_vtx;
    PN_ALLOC(f->side.nb, (size_t)f->side.nb_capacity * sizeof(float4)); PN_ALLOC(f->side.rec, (size_t)max_vtx * PN_REC_FLOATS * 4);
    f->seg_cap = seg_cap_for(max_rays);
    PN_ALLOC(f->tail, (size_t)PN_SEGS * f->seg_cap * sizeof(TailEntry)); PN_ALLOC(f->tail_counts, sizeof(int) * (PN_MAX_TRIPS + 2));
    PN_ALLOC(f->list_seg, (size_t)PN_SEGS * f->seg_cap * 4); PN_ALLOC(f->active_seg, (size_t)PN_SEGS * f->seg_cap * 4);
    PN_ALLOC(f->seg_counters, (size_t)6 * PN_SEGS * PN_SEG_STRIDE * 4);
    PN_ALLOC(f->cell_bits, 2 * (((size_t)max_grid_cells + 31) / 32) * 4);
    PN_ALLOC(f->fars_eff, N * 4);
    PN_ALLOC(f->grid_regions, (size_t)PN_GRID_REGION_WORDS * 4);
    PN_ALLOC(f->trips, sizeof(PnTrip) * (PN_MAX_TRIPS + 2)); PN_ALLOC(f->dev, sizeof(PnFrameDev)); PN_ALLOC(f->cut_bounds, 6 * 4);
    f->max_groups = pn_div_up(max_rays, PN_MIN_RAY_BATCH) + 1;
    PN_ALLOC(f->groups, sizeof(PnGroup) * 2 * f->max_groups); PN_ALLOC(f->group_cnt, sizeof(int) * f->max_groups);
#undef PN_ALLOC
    PN_HIP_CHECK(hipMalloc((void**)&f->march_counters, 16 * sizeof(unsigned long long)));  // [4..15]: debug phase clocks (PN_DBG_PHASES builds)
    PN_HIP_CHECK(hipMalloc((void**)&f->stamps, sizeof(unsigned long long) * PN_TIMED_TRIPS * 3));
    PN_HIP_CHECK(hipHostMalloc((void**)&f->trips_pinned, sizeof(PnTrip) * (PN_MAX_TRIPS + 2)));
    PN_HIP_CHECK(hipHostMalloc((void**)&f->dev_pinned, sizeof(PnFrameDev)));
    PN_HIP_CHECK(hipMemset(f->dev, 0, sizeof(PnFrameDev)));
    memset(f->dev_pinned, 0, sizeof(PnFrameDev));
    *out = f;
    return PN_OK;
}

extern "C" void pn_frame_destroy(pn_frame* f) {
    if (!f) return;
    void* ptrs[] = {f->acc_image, f->nears, f->fars, f->rays_t, f->xyzs, f->dirs, f->deltas, f->sigmas, f->rgbs, f->alive_a, f->alive_b, f->list,
                    f->chunk_counts, f->pig_cnt, f->pig_bgn, f->pig_cursor, f->pig_idx, f->trips, f->dev, f->cut_bounds,
                    f->side.nb_rng, f->side.nb, f->side.rec, f->march_counters, f->tail, f->tail_counts, f->stamps,
                    f->list_seg, f->active_seg, f->seg_counters, f->cell_bits, f->fars_eff, f->grid_regions, f->groups, f->group_cnt, f->fused_ctl, f->fused_clocks, f->t_resume, f->blist, f->strag};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    for (int t = 0; t < PN_TIMED_TRIPS; t++)
        for (int e = 0; e < 3; e++) if (f->ev[t][e]) (void)hipEventDestroy(f->ev[t][e]);
    if (f->trips_pinned) (void)hipHostFree(f->trips_pinned);
    if (f->dev_pinned) (void)hipHostFree(f->dev_pinned);
    delete f;
}

static void frame_stats(pn_frame* f, int64_t* stats_host) {
    // the frame's own summary (k_frame_finish), as the render recorded it — right after graph replays too
    stats_host[0] = f->dev_pinned->stat_trips;
    stats_host[1] = f->dev_pinned->stat_samples;
    stats_host[2] = f->dev_pinned->err;
    stats_host[3] = f->dev_pinned->alive_at_exit;
    stats_host[4] = f->dev_pinned->unfinished;
}

// ---- the frame driver: one render call = argument checks, the plan, the prologue, then the trip loop of render_impl.

// What a render call decides before its first launch, filled once per call by make_frame_plan.  What a continuation has to know about the frame so far
// lives on pn_frame (skip_done, head_marched, fused_first, fused_mode, last_*), not here.
struct FramePlan {
    bool is_static;
    uint32_t nblk;  // 256-ray chunks of the frame
    // grids of the per-trip launches
    uint32_t march_grid, march_grid_first, march_grid_later, trip_grid, tail_grid;
    // the skip pre-pass (k_march_skip)
    int dda_start;
    uint32_t skip_hop_budget;
    size_t bit_words;       // words of one cell map
    bool short_rays;
    int skip_bits_words;
    uint32_t reg_R;         // regions per axis of the region map
    int grid_region_words_1, grid_region_words;  // one map / all of them (0: no region map)
    size_t skip_lds;
    // the throughput form of a frame's leading trips
    uint32_t lpr_rounds, lpr_trips;
    // ray groups
    uint32_t group_rays, n_groups;
    // the fused launch
    bool fused_ok, want_whole, want_fold, early_finish;
    int fuse_from;
};

static FramePlan make_frame_plan(const pn_frame* f, const pn_render_opts* o, uint32_t N, bool is_static, bool resume, int async_trips, const uint8_t* bitfield) {
    FramePlan p{};
    p.is_static = is_static;
    p.nblk = pn_div_up(N, 256);
    // per-trip launches use bounded grids with round-robin chunk loops (the alive count lives on the device): 32 march blocks and
    // 4 composite/compact blocks per CU (measured: 8192 march blocks is ~2 % faster than one block per 32 rays, 2048 is 6 % slower)
    p.march_grid = 8192;
    p.trip_grid = std::min(p.nblk, 1024u);
    p.march_grid_first = std::max(std::min(pn_div_up(N, 32), p.march_grid), (uint32_t)PN_SEGS);  // a frame's first trip: every ray
    // trips after the first find at most N / 8 rays in the typical frame (n_step = 8) = N / 256 chunks of 32: a grid of that size (the chunk loop takes
    // care of frames with more) instead of 8192 mostly empty workgroups per launch — what an empty captured trip costs is dispatch
    p.march_grid_later = std::max(std::min(pn_div_up(N, 256), p.march_grid), (uint32_t)PN_SEGS);
    p.tail_grid = std::max(std::min(pn_div_up(N, 4), 1024u), (uint32_t)PN_SEGS / 4);  // x4 waves, one unfinished ray per wave at a time; every tail segment needs a wave
    // k_march_skip: DDA start + hop budget (pn_march_skip.h: skip_empty_cells); pn_march_set_skip_dda(0) walks hop by hop like rounds 1-2 (same results bit for bit)
    p.dda_start = g_skip_dda_override >= 0 ? g_skip_dda_override : 1;
    p.skip_hop_budget = 8;
    // a frame's first trip with ONE lane per ray in pass 1 (k_march<.., 1>) for this many rounds = visited points before a ray goes to the windows
    p.lpr_rounds = o->throughput > 0 ? (uint32_t)o->throughput : 0u;
    p.lpr_trips = (uint32_t)std::max(o->throughput_trips, 1);  // leading trips in that form
    // the skip pre-pass keeps the cells' emptiness bits in LDS when they fit (48 KB = 393 k cells)
    p.bit_words = (f->max_cells + 31) / 32;
    p.short_rays = !is_static && !o->cut && p.bit_words * 8 <= 48 * 1024;  // both maps in LDS: rays end where their candidates end
    p.skip_bits_words = (p.short_rays || p.bit_words * 4 <= 48 * 1024) ? (int)p.bit_words : 0;
    // --cut: the region map for the skip pre-pass (MarchIO::grid_regions; pn_march_skip.h: region_dda) where its assumptions hold: the top cascade level
    // spans exactly +-bound (bound == 2^(C - 1)), regions are whole 64-byte lines of the bitfield and nest on every level, the map fits.
    // Regions of 8^3 voxels (a 64-byte line of the bitfield); 4^3-voxel regions measured 232 against 177 us on the trex option set (hop by hop 285)
    p.reg_R = o->grid_size / 8;
    const bool reg_ok = !is_static && o->cut && p.dda_start && bitfield && o->grid_size % 32 == 0 && o->cascade >= 1 && o->cascade <= 3 &&
                        o->bound == (float)(1u << (o->cascade - 1)) && (p.reg_R / 2) % (1u << (o->cascade - 1)) == 0 &&
                        (uint64_t)p.reg_R * p.reg_R * p.reg_R / 32 * o->cascade <= PN_GRID_REGION_WORDS && ((uintptr_t)bitfield & 15) == 0;
    p.grid_region_words_1 = reg_ok ? (int)((uint64_t)p.reg_R * p.reg_R * p.reg_R / 32) : 0;  // one map
    p.grid_region_words = p.grid_region_words_1 * (int)o->cascade;                            // one per minimum mip level (pn_march_skip.h)
    p.skip_lds = (size_t)p.skip_bits_words * 4 * (p.short_rays ? 2 : 1) + (size_t)p.grid_region_words * 4;
    // ray groups (ray_batch > 0): per-batch trip schedules inside the same launches
    p.group_rays = o->ray_batch > 0 ? (uint32_t)o->ray_batch : 0u;
    p.n_groups = p.group_rays ? pn_div_up(N, p.group_rays) : 0u;
    // The trips from `fuse_from` on as ONE launch (pn_trips_fused.h) where that form applies: a deformed frame with one trip schedule, max_steps within
    // the fused kernel's trip table.  pn_render_opts.fused_from: the first trip to run fused (0: 1 — right behind the frame's first trip; a scene whose
    // later trips still have more than N / 8 rays alive — the trex option set's second — names a later one; < 0: never).
    p.fused_ok = !is_static && !p.group_rays && o->fused_from >= 0 && o->max_steps <= 8u * PN_FUSED_MAX_TRIPS;
    p.fuse_from = p.fused_ok ? std::max(o->fused_from, 1) : PN_MAX_TRIPS + 1;
    // Forms of the fused launch that take the frame from its first trip on (see render_impl); they also write its epilogue, so the prologue has to know.
    // WHOLE (pn_render_opts.fused_whole with fused_from == 0): the whole frame behind the skip pre-pass as one launch.  The launch checks on the device that
    // at most N / 8 rays have anything to march (then every trip after the first marches 8 samples per ray whatever the first one finds) and does nothing
    // otherwise — the blocking driver then goes on trip by trip, a fixed-trip render is left to pn_render_continue.
    p.want_whole = p.fused_ok && o->fused_whole != 0 && o->fused_from == 0 && !resume;
    // FOLD (pn_render_opts.fused_fold with fused_from <= 1): the first trip's NETWORK, COMPOSITE and COMPACTION inside that launch.  The march of the first
    // trip stays what it is — skip pre-pass, one lane per ray / windows, tail pass, on every CU — and leaves the trip's segmented sample list; the launch runs
    // network tiles over it, composites, and takes the survivors on.  Four launches fewer on a frame's chain (k_list_pack, k_nerf_forward, k_composite,
    // k_compact).  Applies when at most N / 8 rays found a sample (checked on the device); otherwise as with fused_whole.
    p.want_fold = p.fused_ok && !p.want_whole && o->fused_fold != 0 && o->fused_from <= 1 && !resume;
    // the whole-frame form only (chair, profiles/r04_early_finish_ab.txt: 1 719 against 1 601 steps/s; with the folded first trip 1 983 / 1 950 against 2 002 / 1 981)
    p.early_finish = p.want_whole;
    return p;
}

// The arguments of one render call and the launch records that stay the same for all its trips.
struct RenderCall {
    pn_frame* f;
    const pn_net* net;
    const pn_render_opts* o;
    const float *rays_o, *rays_d;
    uint32_t N;
    const float *p_def, *p_ori, *F_IP, *dF_IP;
    int n_vtx;
    const uint8_t* bitfield;
    float *image, *depth, *depth_0, *weights_sum;
    const float* aabb_static;
    hipStream_t st;
    pnm::MarchParams mp, mq;  // mq: mp with the rays' ends where trip 0's k_march_skip shortened them to (FramePlan::short_rays), for the march launches
    pnm2::March2Tables tb;
};

// the alive list trip t reads (trip parity); trip t + 1's is the one its compaction writes
static int* alive_list(const pn_frame* f, int t) { return (t & 1) ? f->alive_b : f->alive_a; }
static PnGroup* group_records(const pn_frame* f, const FramePlan& pl, int t) { return pl.group_rays ? f->groups + (size_t)(t & 1) * f->max_groups : nullptr; }
// pn_frame::seg_counters: [tail | sample | emitted | tail cursor | tail back | active] x PN_SEGS
enum { SEG_TAIL, SEG_SAMP, SEG_EMIT, SEG_CURS, SEG_BACK, SEG_ACTIVE };
static int* seg_counter(const pn_frame* f, int which) { return f->seg_counters + which * PN_SEGS * PN_SEG_STRIDE; }

// The march's launch record of trip tt.  Trip 0 keeps its skip pre-pass state in f->t_resume and lists the slots worth marching in f->active_seg.
static MarchIO make_march_io(const RenderCall& c, const FramePlan& pl, int tt) {
    const pn_frame* f = c.f;
    const bool lpr = (uint32_t)tt < pl.lpr_trips && pl.lpr_rounds > 0;
    MarchIO io{};
    io.rays_alive = alive_list(f, tt);
    io.xyzs = f->xyzs; io.dirs = f->dirs; io.deltas = f->deltas;
    io.trip = f->trips + tt;
    io.list = f->list;
    io.t_resume = (tt == 0) ? f->t_resume : nullptr;
    io.tail = f->tail;
    io.tail_counts = seg_counter(f, SEG_TAIL); io.tail_back = seg_counter(f, SEG_BACK); io.tail_cursors = seg_counter(f, SEG_CURS);
    io.tail_seg_cap = (int)f->seg_cap;
    io.max_rounds = lpr ? (int)pl.lpr_rounds : (int)march_tail_rounds(tt);
    io.active = (tt == 0) ? f->active_seg : nullptr;
    io.active_counts = (tt == 0) ? seg_counter(f, SEG_ACTIVE) : nullptr;
    io.active_seg_cap = (int)f->seg_cap;
    io.list_seg = f->list_seg; io.samp_counts = seg_counter(f, SEG_SAMP); io.list_seg_cap = (int)f->seg_cap;
    io.emit_parts = seg_counter(f, SEG_EMIT);
    io.cell_bits = f->cell_bits; io.cell_bits_words = pl.skip_bits_words;
    io.cell_bits2 = pl.short_rays ? f->cell_bits + pl.bit_words : nullptr;
    io.fars_eff = pl.short_rays ? f->fars_eff : nullptr;
    io.groups = group_records(f, pl, tt); io.group_rays = pl.group_rays;
    io.lane_per_ray = lpr ? 1 : 0;
    io.dda_start = pl.dda_start; io.hop_budget = (int)pl.skip_hop_budget;
    io.grid_regions = pl.grid_region_words > 0 ? f->grid_regions : nullptr;
    io.grid_regions_words = pl.grid_region_words; io.grid_regions_R = (int)pl.reg_R;
    return io;
}

// Measurement mode (march_counters bit 1): point e (0 before the march, 1 behind it, 2 behind the network) of launch group `trip`.  Point 2 closes the
// group: the per-trip launches count the groups of this render, a fused launch (fused_group) never lowers the count.
static int time_mark(pn_frame* f, hipStream_t st, int trip, int e, bool fused_group) {
    if (!(f->march_counters_on & 2) || trip >= PN_TIMED_TRIPS) return PN_OK;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    PN_HIP_CHECK(hipStreamIsCapturing(st, &cs));
    const bool stamp = cs != hipStreamCaptureStatusNone;  // inside a capture: stamp kernels (events recorded in a graph cannot be timed)
    f->stamped = stamp ? 1 : 0;
    if (stamp) {
        k_stamp<<<1, 1, 0, st>>>(f->stamps + trip * 3 + e);
    } else {
        if (!f->ev[trip][e]) PN_HIP_CHECK(hipEventCreate(&f->ev[trip][e]));
        PN_HIP_CHECK(hipEventRecord(f->ev[trip][e], st));
    }
    if (e == 2) f->timed_trips = fused_group ? std::max(f->timed_trips, trip + 1) : trip + 1;
    return PN_OK;
}

// Bounding box, spatial hash and cell maps of a deformed frame (k_frame_tables, for large grids + the multi-workgroup build); the static render only
// sets its box.  keep_tables: those of the previous render on this workspace stay.
static int enqueue_tables(const RenderCall& c, bool is_static, bool keep_tables) {
    pn_frame* f = c.f;
    const pn_render_opts* o = c.o;
    // two 16-bit cell counters per LDS word + the staged point-index table
    const size_t tables_lds = ((size_t)f->max_cells + 1) / 2 * sizeof(unsigned) + (size_t)f->max_vtx * sizeof(int);
    const bool large = tables_lds > 150 * 1024;  // grid too large for the one-workgroup LDS build
    if (is_static) {
        const float* b = c.aabb_static;
        k_set_aabb<<<1, 1, 0, c.st>>>(f->dev, b[0], b[1], b[2], b[3], b[4], b[5]);
    } else if (keep_tables) {
        // nothing: bounding box, spatial hash, candidate lists and packed IP records of the previous render on this workspace stay
    } else if (!large) {
        // dynamic LDS above 64 KB has to be opted into (gfx950: 160 KB per workgroup); the attribute is per DEVICE, so the cache is too
        static size_t tables_lds_set[PN_MAX_DEVICES] = {0};
        int dev_id = 0;
        PN_HIP_CHECK(hipGetDevice(&dev_id));
        if (dev_id < 0 || dev_id >= PN_MAX_DEVICES || tables_lds > tables_lds_set[dev_id]) {
            PN_HIP_CHECK(hipFuncSetAttribute((const void*)k_frame_tables<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tables_lds));
            if (dev_id >= 0 && dev_id < PN_MAX_DEVICES) tables_lds_set[dev_id] = tables_lds;
        }
        k_frame_tables<false><<<1, 1024, tables_lds, c.st>>>(c.p_def, c.n_vtx, o->cut, o->bound, o->hash_grid_size, (int)f->max_cells, f->dev, f->pig_cnt,
                                                         f->pig_bgn, f->pig_idx, f->pig_cursor, f->cell_bits);
    } else {
        k_frame_tables<true><<<1, 1024, 0, c.st>>>(c.p_def, c.n_vtx, o->cut, o->bound, o->hash_grid_size, (int)f->max_cells, f->dev, f->pig_cnt, f->pig_bgn,
                                                   f->pig_idx, f->pig_cursor, f->cell_bits);
        return pig_build(c.n_vtx, (int)f->max_cells, f->dev->resolution + 3, c.p_def, f->dev->aabb, o->hash_grid_size, f->dev->resolution, f->pig_cnt, f->pig_bgn,
                         f->pig_idx, f->pig_cursor, &f->dev->err, c.st);  // (device addresses of members of the frame record)
    }
    return PN_OK;
}

// The prologue of a fresh frame: tables, candidate lists, packed IP records, region map, ray state (a continuation finds all of it in the workspace).
static int enqueue_prologue(const RenderCall& c, const FramePlan& pl) {
    pn_frame* f = c.f;
    const pn_render_opts* o = c.o;
    const bool keep_tables = !pl.is_static && o->reuse_tables && f->tables_n_vtx == c.n_vtx;  // staged batches of one frame: same IP state
    int rc = enqueue_tables(c, pl.is_static, keep_tables);
    if (rc) return rc;
    FramePrologue fp;
    memset(&fp, 0, sizeof(fp));
    if (!pl.is_static && !keep_tables) {
        f->tables_n_vtx = c.n_vtx;
        fp.n_grid_max = (int)f->max_cells; fp.n_grid_dev = f->dev->resolution + 3; fp.res = f->dev->resolution; fp.pig_cnt = f->pig_cnt; fp.pig_bgn = f->pig_bgn;
        fp.pig_idx = f->pig_idx; fp.p_def = c.p_def; fp.swap = (o->num_seek_IP == 1) ? 1 : 0; fp.nb_rng = f->side.nb_rng; fp.nb = f->side.nb;
        fp.nb_capacity = f->side.nb_capacity; fp.cell_bits = f->cell_bits;
        fp.list_blocks = (int)std::min(pn_div_up((uint64_t)f->max_cells, 32), 2048u);
        fp.pack_blocks = (int)pn_div_up((uint64_t)c.n_vtx * PN_REC_FLOATS, 256);
        fp.n_vtx = c.n_vtx; fp.p_ori = c.p_ori; fp.F_IP = c.F_IP; fp.dF_IP = c.dF_IP; fp.rec = f->side.rec;
    }
    fp.rays_o = c.rays_o; fp.rays_d = c.rays_d; fp.dev = f->dev; fp.N = c.N; fp.min_near = o->min_near; fp.nears = f->nears; fp.fars = f->fars; fp.rays_t = f->rays_t;
    fp.trips = f->trips; fp.tail_counts = f->tail_counts; fp.seg_counters = f->seg_counters; fp.n_trip_records = PN_MAX_TRIPS + 2; fp.alive = f->alive_a;
    fp.weights_sum = c.weights_sum; fp.depth_0 = c.depth_0; fp.image = f->acc_image; fp.groups = pl.group_rays ? f->groups : nullptr; fp.group_cnt = f->group_cnt;
    fp.group_rays = pl.group_rays; fp.n_groups = pl.n_groups; fp.chunk_words = f->chunk_counts;
    fp.early_finish = pl.early_finish ? 1 : 0; fp.bg = o->bg_color; fp.image_out = c.image; fp.depth_out = c.depth;
    {   // pn_render_opts.ray_tile_w: 16 x 4 pixel tiles
        const uint32_t lw = 4;
        const uint32_t tw = o->ray_tile_w > 0 ? (uint32_t)o->ray_tile_w : 0u;
        fp.tile_lw = lw;
        fp.tile_w = (!pl.is_static && !pl.group_rays && tw && tw % (1u << lw) == 0 && c.N % ((64u >> lw) * tw) == 0) ? tw : 0u;
    }
    // both cell maps of a workgroup in LDS while it builds its lists (up to 64 KB = 262 k cells; beyond that straight to global memory, where
    // the maps then span enough cache lines for the atomics not to queue)
    fp.lds_words = (fp.list_blocks > 0 && pl.bit_words * 8 <= 64 * 1024) ? (int)pl.bit_words : 0;
    if (pl.grid_region_words > 0) {
        fp.grid = c.bitfield; fp.grid_regions = f->grid_regions; fp.gr_R = (int)pl.reg_R; fp.gr_C = (int)o->cascade; fp.gr_H = o->grid_size;
        fp.gr_bound = o->bound; fp.cut_bounds = f->cut_bounds; fp.gr_blocks = (int)pn_div_up((uint64_t)pl.grid_region_words_1 * 32, 256);
    }
    k_frame_prologue<<<(uint32_t)(fp.list_blocks + fp.pack_blocks + fp.gr_blocks) + pl.nblk, 256, (size_t)fp.lds_words * 8, c.st>>>(fp);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

// The march launches of trip t.  Trip 0 (every ray, one sample each) is dominated by rays crossing IP-free cells: a one-lane-per-ray pre-pass fast-forwards
// them (its per-ray resume point: f->t_resume) and lists the slots that still have work (f->active_seg) — once per frame (pn_frame::skip_done), so a
// continuation from trip 0 does not run it again.
static void enqueue_skip(const RenderCall& c, const FramePlan& pl, const MarchIO& io0) {
    if (c.f->skip_done) return;
    k_march_skip<<<pl.nblk, 256, pl.skip_lds, c.st>>>(c.mp, c.tb, io0);
    c.f->skip_done = 1;
}
static void enqueue_march(const RenderCall& c, const FramePlan& pl, int t, bool margin) {
    const MarchIO io = make_march_io(c, pl, t);
    if (io.t_resume) enqueue_skip(c, pl, io);
    launch_march(c.o->num_seek_IP, t == 0 ? pl.march_grid_first : (margin ? 2u * PN_SEGS : pl.march_grid_later), margin ? (uint32_t)PN_SEGS : pl.tail_grid, c.st,
                 c.mq, c.tb, io);
}

// Composite + compaction of trip t in their two forms: one launch (k_composite_compact), or the pair k_composite, k_compact.
static void enqueue_composite(const RenderCall& c, const FramePlan& pl, int t, bool margin) {
    pn_frame* f = c.f;
    const pn_render_opts* o = c.o;
    int *cur = alive_list(f, t), *nxt = alive_list(f, t + 1);
    PnGroup *g_cur = group_records(f, pl, t), *g_nxt = group_records(f, pl, t + 1);
    // a frame's first trip has every ray alive (2 500 chunks at 800x800): five rounds of the bounded fused kernel (31 us) cost more than the two
    // launches (25 us), which poll nothing.  PN_CC_TRIP0=1 and PN_CC_GRID are test hooks (tests/test_gpu_edges.py): the fused form on trip 0, its grid
    static const bool cc_trip0 = pn_env_u32("PN_CC_TRIP0", 0) != 0;
    if (!pl.is_static && !margin && (t > 0 || cc_trip0)) {
        // a bounded grid with chunk loops: all of a launch's workgroups can be resident at once, whatever order the XCDs start them in (see the kernel)
        static const uint32_t cc_grid = pn_env_u32("PN_CC_GRID", 512);
        const uint32_t cc_poll_cap = 1u << 20;
        k_composite_compact<<<std::min(cc_grid, pn_div_up(c.N, 256)), 256, 0, c.st>>>(o->T_thresh, cur, nxt, f->rays_t, f->sigmas, f->rgbs, f->deltas, c.weights_sum,
                                                                                   c.depth_0, f->acc_image, f->trips + t, f->trips + t + 1, (unsigned*)f->chunk_counts,
                                                                                   (uint32_t)t + 1, c.N, o->max_steps, 1, f->seg_counters, f->tail_counts + t, g_cur,
                                                                                   g_nxt, f->group_cnt, pl.group_rays, pl.n_groups, &f->dev->err, cc_poll_cap);
        return;
    }
    // margin trips get a small grid (see enqueue_trips), and the two launches: the fused one needs a workgroup per chunk
    const uint32_t pair_grid = margin ? std::min(pl.trip_grid, 64u) : pl.trip_grid;
    k_composite<<<pair_grid, 256, 0, c.st>>>(0, 0, o->T_thresh, cur, f->rays_t, f->sigmas, f->rgbs, f->deltas, c.weights_sum, c.depth_0, f->acc_image, f->trips + t,
                                             f->chunk_counts, g_cur, pl.group_rays, pl.n_groups > 1 ? f->group_cnt : nullptr);
    k_compact<<<pair_grid, 256, 0, c.st>>>(cur, 0, f->chunk_counts, nxt, nullptr, f->trips + t, f->trips + t + 1, c.N, o->max_steps, pl.is_static ? 0 : 1,
                                           pl.is_static ? nullptr : f->seg_counters, f->tail_counts + t, g_cur, g_nxt, f->group_cnt, pl.group_rays, pl.n_groups);
}

// One loop trip as its own launches: march (or static march), list pack, network, composite + compaction.  The two heavy launch groups are bracketed
// on the launch stream in measurement mode.  margin: see enqueue_trips.
static int enqueue_trip(const RenderCall& c, const FramePlan& pl, int t, bool margin) {
    pn_frame* f = c.f;
    const pn_render_opts* o = c.o;
    int rc;
    if ((rc = time_mark(f, c.st, t, 0, false))) return rc;
    if (pl.is_static) {
        k_march_static_trip<<<pl.trip_grid, 256, 0, c.st>>>(f->trips + t, alive_list(f, t), f->rays_t, c.rays_o, c.rays_d, o->bound, o->dt_gamma, o->max_steps,
                                                            o->cascade, o->grid_size, c.bitfield, f->fars, f->xyzs, f->dirs, f->deltas, f->list);
    } else {
        // (a first trip whose march has already run — a fused launch that stepped aside — goes on with its sample list)
        if (!(t == 0 && f->head_marched)) enqueue_march(c, pl, t, margin);
        if (t == 0) k_list_pack<<<PN_SEGS, 256, 0, c.st>>>(f->trips + t, seg_counter(f, SEG_SAMP), f->list_seg, (int)f->seg_cap, f->list);  // the only list trip
    }
    if ((rc = time_mark(f, c.st, t, 1, false))) return rc;
    rc = pn_nerf_forward_launch(c.net, f->xyzs, f->dirs, f->list, &f->trips[t].n_samples, c.N, o->density_scale, f->sigmas, f->rgbs, o->fp16, c.st, margin ? 64u : 0u);
    if (rc) return rc;
    if ((rc = time_mark(f, c.st, t, 2, false))) return rc;
    enqueue_composite(c, pl, t, margin);
    return PN_OK;
}

// The fused launch (pn_trips_fused.h) from trip t on: form 0 the later trips, 1 (WHOLE) the frame from behind its skip pre-pass, which runs here, 2 (FOLD)
// from the first trip's network on — the first trip's march runs here as its per-trip launches would run it (no k_list_pack: the launch reads the
// segments).  finalize: the launch also writes the frame's epilogue.
static int enqueue_fused(const RenderCall& c, const FramePlan& pl, int t, int form, bool finalize) {
    pn_frame* f = c.f;
    const pn_net* net = c.net;
    const pn_render_opts* o = c.o;
    const bool whole = form == 1, fold = form == 2;
    int rc;
    if (fold) {
        if ((rc = time_mark(f, c.st, 0, 0, true))) return rc;
        enqueue_march(c, pl, 0, false);
        f->head_marched = 1;
        if ((rc = time_mark(f, c.st, 0, 1, true)) || (rc = time_mark(f, c.st, 0, 2, true))) return rc;
    }
    FusedArgs fa;
    memset(&fa, 0, sizeof(fa));
    fa.lv = (const PnFusedLevel*)(o->fp16 ? net->fused_levels : net->byte_levels); fa.emb = net->embeddings; fa.emb_h = (const uint32_t*)net->emb_half; fa.emb_bytes = net->n_entries * 4u;
    fa.wimg_g = (const uint4*)(o->fp16 ? net->whalf : (net->x_ok ? net->wx : net->wsplit)); fa.net_bound = net->bound; fa.net_inv2b = 1.0f / (2 * net->bound); fa.density_scale = o->density_scale;
    fa.x_scales = net->x_scales;
    fa.trips = f->trips + t; fa.N_rays = c.N; fa.max_steps = o->max_steps; fa.T_thresh = o->T_thresh;
    fa.alive = alive_list(f, t);
    fa.rays_t = f->rays_t; fa.weights_sum = c.weights_sum; fa.depth = c.depth_0; fa.image = f->acc_image;
    fa.xyzs = f->xyzs; fa.dirs = f->dirs; fa.deltas = f->deltas; fa.sigmas = f->sigmas; fa.rgbs = f->rgbs;
    fa.ctl = f->fused_ctl; fa.dev = f->dev; fa.tail_diag = f->tail_counts + t;
    fa.clocks = (f->march_counters_on & 4) ? f->fused_clocks : nullptr;
    fa.order = o->fused_order >= 0 ? 1 : 0;
    if (whole) {
        fa.active = f->active_seg; fa.active_counts = seg_counter(f, SEG_ACTIVE); fa.active_seg_cap = (int)f->seg_cap; fa.t_resume = f->t_resume;
        fa.blist = f->blist; fa.strag = f->strag; fa.blist_cap = f->blist_cap;
        fa.a_rounds = 24;
    }
    if (fold) {
        fa.list_seg = f->list_seg; fa.samp_counts = seg_counter(f, SEG_SAMP); fa.list_seg_cap = (int)f->seg_cap;
        fa.seg_tail = seg_counter(f, SEG_TAIL); fa.seg_back = seg_counter(f, SEG_BACK);
        fa.blist = f->blist; fa.strag = f->strag; fa.blist_cap = f->blist_cap;
    }
    if (finalize) {
        fa.finalize = 1; fa.bg = o->bg_color; fa.nears = f->nears; fa.fars_full = f->fars; fa.image_out = c.image; fa.depth_out = c.depth;
    }
    const int tb_idx = fold ? 1 : t;  // launch group the fused launch is timed as (fold: behind the first trip's march)
    if ((rc = time_mark(f, c.st, tb_idx, 0, true))) return rc;  // the whole launch is bracketed like a trip's march group (its network share comes from the phase clocks)
    if (whole) enqueue_skip(c, pl, make_march_io(c, pl, 0));  // per-ray resume points, shortened ends, the active list (one lane per ray)
    const uint32_t blocks = o->fused_grid > 0 ? std::min((uint32_t)o->fused_grid, f->fused_blocks) : f->fused_blocks;
    rc = launch_trips_fused(o->num_seek_IP, o->max_iter_num > 1, o->fp16 ? 1 : (net->x_ok ? 2 : 0), form, blocks, c.st, c.mq, c.tb, fa);
    if (rc) return rc;
    if ((rc = time_mark(f, c.st, tb_idx, 1, true)) || (rc = time_mark(f, c.st, tb_idx, 2, true))) return rc;
    f->fused_first = tb_idx;
    f->fused_mode = form;
    return PN_OK;
}

// What render_impl rejects: the argument checks of the four entry points.
static int check_render_call(const RenderCall& c, bool is_static, bool resume, int async_trips) {
    const pn_frame* f = c.f;
    const pn_render_opts* o = c.o;
    PN_REQUIRE(f && c.net && o && c.rays_o && c.rays_d && c.bitfield && c.image && c.depth && c.depth_0 && c.weights_sum);
    PN_REQUIRE(is_static || resume || (c.p_def && c.p_ori && c.F_IP && c.dF_IP && c.n_vtx > 0 && (uint32_t)c.n_vtx <= f->max_vtx));
    PN_REQUIRE(!resume || c.N == f->last_N);
    PN_REQUIRE(c.N > 0 && c.N <= f->max_rays);
    PN_REQUIRE(o->num_seek_IP >= 1 && o->num_seek_IP <= 3 && o->cascade >= 1 && o->cascade <= 8 && o->max_steps <= PN_MAX_TRIPS - PN_TRIP_BATCH);
    PN_REQUIRE(async_trips >= 0 && async_trips <= PN_MAX_TRIPS);
    PN_REQUIRE(!o->fp16 || c.net->emb_half);  // pn_net_enable_half before an fp16 render
    // ray groups: not for the static render (its trip kernel keeps one schedule); a continuation must use the frame's
    PN_REQUIRE(o->ray_batch == 0 || (o->ray_batch >= PN_MIN_RAY_BATCH && !is_static));
    PN_REQUIRE((o->ray_batch > 0 ? pn_div_up(c.N, (uint32_t)o->ray_batch) : 0u) <= f->max_groups);
    PN_REQUIRE(!resume || (o->ray_batch > 0 ? (uint32_t)o->ray_batch : 0u) == f->last_group_rays);
    return PN_OK;
}

// The trip loop, from trip `t` on; returns with t = the trips enqueued so far.
// async_trips == 0: blocking form.  Trips are enqueued in batches until a read-back shows no ray alive; a fused launch is followed by a read-back of how
//                   many trips it ran — none means it stepped aside: one trip of the per-trip launches, then the launch again.
// async_trips  > 0: exactly that many trips are enqueued and nothing blocks the host, so every call is legal inside a HIP-graph stream capture.
//                   Where the fused launch applies: the per-trip launches up to fuse_from, then the launch, and the loop ends there — how many trips it
//                   ran only the device knows (add_fused: k_frame_finish adds them; finished_in_launch: the launch itself wrote the frame's epilogue).
//                   If it steps aside the frame is an unfinished one, left to pn_render_continue.
// WHOLE and FOLD (FramePlan) are tried once, in front of a fresh frame's first trip.
static int enqueue_trips(const RenderCall& c, const FramePlan& pl, int async_trips, bool resume, int& t, int& add_fused, bool& finished_in_launch) {
    pn_frame* f = c.f;
    int rc;
    bool done = false;
    bool whole_try = pl.want_whole && t == 0, fold_try = pl.want_fold && t == 0;
    while (!done && t < PN_MAX_TRIPS) {
        const bool whole = whole_try;
        whole_try = false;
        const bool fold = !whole && fold_try && t == 0 && !f->head_marched;
        if (fold) fold_try = false;
        if (whole || fold || t >= pl.fuse_from) {
            const bool finalize = (whole || fold) && pl.early_finish;
            if ((rc = enqueue_fused(c, pl, t, whole ? 1 : (fold ? 2 : 0), finalize))) return rc;
            if (async_trips > 0) {
                add_fused = 1;
                finished_in_launch = finalize;
                break;
            }
            PN_HIP_CHECK(hipMemcpyAsync(f->dev_pinned, f->dev, sizeof(PnFrameDev), hipMemcpyDeviceToHost, c.st));
            PN_HIP_CHECK(hipMemcpyAsync(f->trips_pinned + t, f->trips + t, sizeof(PnTrip), hipMemcpyDeviceToHost, c.st));
            PN_HIP_CHECK(hipStreamSynchronize(c.st));
            if (f->dev_pinned->fused_trips > 0) {  // ran until no ray was alive (or max_steps)
                t += f->dev_pinned->fused_trips;
                finished_in_launch = finalize;
                break;
            }
            if (f->trips_pinned[t].n_alive <= 0) break;
            // not applicable at this trip (more than N / 8 rays alive: n_step < 8): one trip of the per-trip launches, then again
            f->fused_first = -1;
            f->fused_mode = 0;
        }
        const int batch = async_trips > 0 ? (pl.fused_ok ? pl.fuse_from - t : async_trips) : (pl.fused_ok ? std::max(pl.fuse_from - t, 1) : PN_TRIP_BATCH);
        for (int k = 0; k < batch; k++, t++) {
            // margin trips: a fixed-trip render (captured graphs) carries PN_TRIP_MARGIN more trips than the frame it was sized on needed, and they
            // find no ray (or a few hundred stragglers).  What they cost is the dispatch of their launches' workgroups, so they get small grids —
            // the chunk loops take care of whatever is alive — and the two-launch composite / compaction (the fused one needs a workgroup per chunk)
            const bool margin = !pl.fused_ok && async_trips > PN_TRIP_MARGIN && k >= async_trips - PN_TRIP_MARGIN && !resume;
            if ((rc = enqueue_trip(c, pl, t, margin))) return rc;
        }
        PN_LAUNCH_CHECK();
        if (async_trips > 0) {
            if (pl.fused_ok) continue;  // the fused launch follows
            break;
        }
        if (pl.fused_ok && t >= pl.fuse_from) continue;  // no read-back: the fused launch finds out by itself whether anything is alive
        // one small readback per batch decides whether more trips are needed (the reference syncs every trip)
        PN_HIP_CHECK(hipMemcpyAsync(f->trips_pinned + t, f->trips + t, sizeof(PnTrip), hipMemcpyDeviceToHost, c.st));
        PN_HIP_CHECK(hipStreamSynchronize(c.st));
        done = f->trips_pinned[t].n_alive <= 0;
    }
    return PN_OK;
}

// One render call: checks, plan, prologue (a fresh frame) or the workspace's state (a continuation), the trip loop, the epilogue.
// aabb_static != nullptr: the undeformed render (NeRFRenderer.run_cuda, eval branch, renderer.py:267-387): no IP state, near / far from the
// given box, kernel_march_rays instead of the bending march; everything else (trip records, network, composite, compaction, epilogue)
// is the same driver.
static int render_impl(pn_frame* f, const pn_net* net, const pn_render_opts* o, const float* rays_o, const float* rays_d, uint32_t N,
                       const float* p_def, const float* p_ori, const float* F_IP, const float* dF_IP, int n_vtx, const uint8_t* bitfield, float* image,
                       float* depth, float* depth_0, float* weights_sum, int64_t* stats_host, int async_trips, void* stream,
                       const float* aabb_static = nullptr, int mode = 0 /* 0: whole frame, 1: continue the deformed frame on f, 2: continue the static one */) {
    const bool is_static = aabb_static != nullptr || mode == 2;
    const bool resume = mode != 0;
    RenderCall c{};
    c.f = f; c.net = net; c.o = o; c.rays_o = rays_o; c.rays_d = rays_d; c.N = N;
    c.p_def = p_def; c.p_ori = p_ori; c.F_IP = F_IP; c.dF_IP = dF_IP; c.n_vtx = n_vtx; c.bitfield = bitfield;
    c.image = image; c.depth = depth; c.depth_0 = depth_0; c.weights_sum = weights_sum; c.aabb_static = aabb_static; c.st = (hipStream_t)stream;
    int rc = check_render_call(c, is_static, resume, async_trips);
    if (rc) return rc;
    const FramePlan pl = make_frame_plan(f, o, N, is_static, resume, async_trips, bitfield);
    // (bbmin, bbmax, resolution, err: device addresses of members of the frame record)
    c.mp = make_march_params(f->pig_cnt, f->pig_bgn, f->pig_idx, n_vtx, 0, p_def, p_ori, F_IP, dF_IP, o->max_iter_num, f->dev->aabb, f->dev->aabb + 3,
                             o->hash_grid_size, f->dev->resolution, o->num_seek_IP, o->IP_dx, o->cut, f->cut_bounds, f->rays_t, rays_o, rays_d, o->bound,
                             o->dt_gamma, o->max_steps, o->cascade, o->grid_size, bitfield, f->fars, &f->dev->err);
    c.mp.stats = (f->march_counters_on & 1) ? f->march_counters : nullptr;
    c.mq = c.mp;
    if (pl.short_rays) c.mq.fars = f->fars_eff;  // written by trip 0's k_march_skip
    c.tb = pnm2::March2Tables{f->side.nb_rng, f->side.nb, (const float4*)f->side.rec};

    if (!f->cut_bounds_valid || memcmp(f->cut_bounds_host, o->cut_bounds, sizeof(f->cut_bounds_host)) != 0) {  // uploaded only when it changes
        memcpy(f->cut_bounds_host, o->cut_bounds, sizeof(f->cut_bounds_host));
        PN_HIP_CHECK(hipMemcpyAsync(f->cut_bounds, f->cut_bounds_host, 6 * sizeof(float), hipMemcpyHostToDevice, c.st));
        f->cut_bounds_valid = 1;
    }
    if (!resume) {
        if ((rc = enqueue_prologue(c, pl))) return rc;
        f->skip_done = 0;
        f->head_marched = 0;
    }
    // a continuation picks up at the record the last compaction wrote; the trip count comes from the device (through the pinned copy the
    // previous render made at its end), not from host bookkeeping: the previous render may have been a graph replay
    int t = resume ? f->dev_pinned->trips_run : 0;
    PN_REQUIRE(t >= 0 && t <= PN_MAX_TRIPS);
    f->fused_first = -1;
    int add_fused = 0;
    bool finished_in_launch = false;
    if ((rc = enqueue_trips(c, pl, async_trips, resume, t, add_fused, finished_in_launch))) return rc;
    if (!finished_in_launch)
        k_frame_finish<<<pl.nblk, 256, 0, c.st>>>(N, o->bg_color, f->nears, f->fars, weights_sum, depth_0, f->acc_image, image, depth, f->trips, f->dev, t, add_fused,
                                                  pl.is_static ? 1 : 0);
    PN_LAUNCH_CHECK();
    f->last_trips = t;
    f->last_N = N;
    f->last_group_rays = pl.group_rays;
    // the frame record (trips run, summary of the trip records, flags: written by k_frame_finish) always travels to pinned host memory with one small
    // async copy: pn_render_status / pn_render_continue read it once the caller knows the render has completed
    PN_HIP_CHECK(hipMemcpyAsync(f->dev_pinned, f->dev, sizeof(PnFrameDev), hipMemcpyDeviceToHost, c.st));
    if (async_trips == 0 && stats_host) {
        PN_HIP_CHECK(hipStreamSynchronize(c.st));
        frame_stats(f, stats_host);
    }
    return PN_OK;
}

extern "C" int pn_render_deformed(pn_frame* f, const pn_net* net, const pn_render_opts* o, const float* rays_o, const float* rays_d, uint32_t N,
                                  const float* p_def, const float* p_ori, const float* F_IP, const float* dF_IP, int n_vtx,
                                  const uint8_t* bitfield, float* image, float* depth, float* depth_0, float* weights_sum, int64_t* stats_host,
                                  void* stream) {
    return render_impl(f, net, o, rays_o, rays_d, N, p_def, p_ori, F_IP, dF_IP, n_vtx, bitfield, image, depth, depth_0, weights_sum, stats_host, 0, stream);
}

extern "C" int pn_render_deformed_async(pn_frame* f, const pn_net* net, const pn_render_opts* o, const float* rays_o, const float* rays_d,
                                        uint32_t N, const float* p_def, const float* p_ori, const float* F_IP, const float* dF_IP, int n_vtx,
                                        const uint8_t* bitfield, float* image, float* depth, float* depth_0, float* weights_sum, int n_trips,
                                        void* stream) {
    PN_REQUIRE(n_trips > 0);
    return render_impl(f, net, o, rays_o, rays_d, N, p_def, p_ori, F_IP, dF_IP, n_vtx, bitfield, image, depth, depth_0, weights_sum, nullptr, n_trips,
                       stream);
}

extern "C" int pn_render_static(pn_frame* f, const pn_net* net, const pn_render_opts* o, const float* rays_o, const float* rays_d, uint32_t N,
                                const float* aabb_host, const uint8_t* bitfield, float* image, float* depth, float* depth_0, float* weights_sum,
                                int64_t* stats_host, int n_trips, void* stream) {
    PN_REQUIRE(aabb_host && n_trips >= 0);
    return render_impl(f, net, o, rays_o, rays_d, N, nullptr, nullptr, nullptr, nullptr, 0, bitfield, image, depth, depth_0, weights_sum, stats_host, n_trips,
                       stream, aabb_host);
}

extern "C" int pn_render_continue(pn_frame* f, const pn_net* net, const pn_render_opts* o, const float* rays_o, const float* rays_d, uint32_t N,
                                  const uint8_t* bitfield, float* image, float* depth, float* depth_0, float* weights_sum, int64_t* stats_host, int n_trips,
                                  int is_static, void* stream) {
    PN_REQUIRE(n_trips >= 0);
    return render_impl(f, net, o, rays_o, rays_d, N, nullptr, nullptr, nullptr, nullptr, 0, bitfield, image, depth, depth_0, weights_sum, stats_host, n_trips,
                       stream, nullptr, is_static ? 2 : 1);
}

extern "C" int pn_frame_march_counters(pn_frame* f, int enable, uint64_t* counters_host, void* stream) {
    PN_REQUIRE(f);
    hipStream_t st = (hipStream_t)stream;
    if (counters_host) {
        PN_HIP_CHECK(hipMemcpyAsync(counters_host, f->march_counters, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
#if PN_DBG_PHASES || PN_DBG_STATS   // (timing / counting builds only: tools/build_variant.py name -DPN_DBG_STATS=1 prints the debug slots [4..15])
        {
            unsigned long long ph[16];
            PN_HIP_CHECK(hipMemcpy(ph, f->march_counters, sizeof(ph), hipMemcpyDeviceToHost));
            fprintf(stderr, "phases:");
            for (int i = 4; i < 16; i++) fprintf(stderr, " %llu", ph[i]);
            fprintf(stderr, "\n");
        }
#endif
        PN_HIP_CHECK(hipStreamSynchronize(st));
    }
    if ((enable & 1) && !(f->march_counters_on & 1)) PN_HIP_CHECK(hipMemsetAsync(f->march_counters, 0, 16 * sizeof(unsigned long long), st));
    f->march_counters_on = enable & 7;  // bit 0: work counters, bit 1: per-trip event timing, bit 2: phase clocks of the fused launches
    return PN_OK;
}

// Phase clocks of the fused launches on `f` (march_counters bit 2): shader-clock cycles summed over waves for {refill, march window round, 64-lane
// windows, network, composite}, wave-rounds, waves; first_trip_out: the trip the last render started fusing at (-1: it did not).  reset != 0 zeroes them.
extern "C" int pn_frame_fused_clocks(pn_frame* f, uint64_t* clocks_host, int* first_trip_out, int reset, void* stream) {
    PN_REQUIRE(f);
    hipStream_t st = (hipStream_t)stream;
    if (clocks_host) {
        PN_HIP_CHECK(hipMemcpyAsync(clocks_host, f->fused_clocks, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        PN_HIP_CHECK(hipStreamSynchronize(st));
        clocks_host[15] = f->fused_first >= 0 ? (uint64_t)f->fused_mode : 0u;   // form of the last render's fused launch (host-side knowledge)
    }
    if (first_trip_out) *first_trip_out = f->fused_first;
    if (reset) PN_HIP_CHECK(hipMemsetAsync(f->fused_clocks, 0, 16 * sizeof(unsigned long long), st));
    return PN_OK;
}

// The drawing order of one share of the fused launch's plain form, on the host: the functions of pn_fused_order.h as the kernel runs them.  rays_t / fars
// [n_rays]: the share's rays in list order (packets of PN_ORDER_PACKET consecutive entries); perm_out [ceil(n_rays / PN_ORDER_PACKET)]: the packet drawn k-th.
extern "C" int pn_fused_order_host(const float* rays_t, const float* fars, int n_rays, int* perm_out) {
    PN_REQUIRE(n_rays >= 0 && (n_rays == 0 || (rays_t && fars && perm_out)));
    const int n_packets = (n_rays + PN_ORDER_PACKET - 1) / PN_ORDER_PACKET;
    const int n_ord = std::min(n_packets, PN_ORDER_CAP);
    std::vector<float> keys((size_t)n_ord, 0.0f);
    for (int k = 0; k < n_ord; k++)
        for (int s = 0; s < PN_ORDER_PACKET && k * PN_ORDER_PACKET + s < n_rays; s++)
            keys[k] = fmaxf(keys[k], pn_order_key(rays_t[k * PN_ORDER_PACKET + s], fars[k * PN_ORDER_PACKET + s]));
    for (int k = 0; k < n_ord; k++) perm_out[pn_order_rank(keys.data(), n_ord, k)] = k;
    for (int k = n_ord; k < n_packets; k++) perm_out[k] = k;
    return PN_OK;
}

extern "C" int pn_frame_trip_times(pn_frame* f, float* march_ms_host, float* network_ms_host, int max_trips, int* n_trips_out, void* stream) {
    PN_REQUIRE(f && march_ms_host && network_ms_host && n_trips_out && max_trips >= 0);
    PN_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    const int n = f->timed_trips < max_trips ? f->timed_trips : max_trips;
    if (f->stamped) {
        static unsigned long long host[PN_TIMED_TRIPS * 3];
        PN_HIP_CHECK(hipMemcpy(host, f->stamps, sizeof(unsigned long long) * (size_t)n * 3, hipMemcpyDeviceToHost));
        for (int t = 0; t < n; t++) {  // s_memrealtime ticks at 100 MHz: 1 tick = 1e-5 ms
            march_ms_host[t] = (float)((double)(host[t * 3 + 1] - host[t * 3]) * 1e-5);
            network_ms_host[t] = (float)((double)(host[t * 3 + 2] - host[t * 3 + 1]) * 1e-5);
        }
    } else {
        for (int t = 0; t < n; t++) {
            PN_HIP_CHECK(hipEventElapsedTime(march_ms_host + t, f->ev[t][0], f->ev[t][1]));
            PN_HIP_CHECK(hipEventElapsedTime(network_ms_host + t, f->ev[t][1], f->ev[t][2]));
        }
    }
    *n_trips_out = n;
    return PN_OK;
}

extern "C" int pn_frame_trip_records(pn_frame* f, int* records_host, int* tail_counts_host, int max_trips, void* stream) {
    PN_REQUIRE(f && records_host && tail_counts_host && max_trips >= 0);
    PN_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    const int n = max_trips < PN_MAX_TRIPS ? max_trips : PN_MAX_TRIPS;
    std::vector<PnTrip> rec((size_t)n);
    PN_HIP_CHECK(hipMemcpy(rec.data(), f->trips, sizeof(PnTrip) * (size_t)n, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) {
        int* r = records_host + 5 * i;
        r[0] = rec[i].n_alive; r[1] = rec[i].n_step; r[2] = rec[i].step_base; r[3] = rec[i].n_samples; r[4] = rec[i].dense ? rec[i].n_emitted : -1;
    }
    PN_HIP_CHECK(hipMemcpy(tail_counts_host, f->tail_counts, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
    return PN_OK;
}


extern "C" int pn_frame_reset_unfinished(pn_frame* f, void* stream) {
    PN_REQUIRE(f);
    k_reset_unfinished<<<1, 1, 0, (hipStream_t)stream>>>(f->dev);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

extern "C" int pn_render_status(pn_frame* f, int64_t* stats_host, int synchronize, void* stream) {
    PN_REQUIRE(f && stats_host);
    if (synchronize) PN_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    frame_stats(f, stats_host);
    return PN_OK;
}
