/* pienerf_hip.h — C ABI of libpienerf_hip.so: the MI355X (gfx950) kernels behind the
 * PIE-NeRF simulate-and-render hot path.
 *
 * Every entry point replaces one reference interface, cited as file:line relative to
 * /root/reference.  Conventions (SURVEY.md §8b "What a C-ABI replacement must export"):
 *   - plain device pointers + extents + scalars; no torch types;
 *   - the CALLER allocates every output (the reference's Python wrappers do, e.g.
 *     raymarching/raymarching.py:415-417) and zero-fills where stated;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); nothing blocks the
 *     host unless stated — the reference's per-call cudaEventSynchronize
 *     (raymarching/src/raymarching.cu:1481-1482) is deliberately not reproduced;
 *   - return value: 0 on success, a PN_ERR_* code otherwise (the pybind functions return void
 *     and TORCH_CHECK-throw; the Python mirror raises RuntimeError on non-zero).
 * Pointers are DEVICE pointers unless the parameter is marked [host].
 */
#ifndef PIENERF_HIP_H
#define PIENERF_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PN_OK 0
#define PN_ERR_ARG 1      /* unsupported D / C / degree / num_seek_IP, null pointer, ... */
#define PN_ERR_HIP 2      /* a HIP runtime call or kernel launch failed; see pn_last_error() */
#define PN_ERR_CAPACITY 3 /* a caller-provided scratch buffer is too small */

/* Library identity: "pienerf_hip <version> gfx950".  Never NULL. */
const char* pn_version(void);

/* Stream confined to a subset of the GPU's compute units (hipExtStreamCreateWithCUMask), for the pipelined harness: the
 * simulator's chain of small launches runs on `n_cu` CUs of its own, the render streams on the complement, so neither
 * waits for the other's waves to release registers.  Mask bits first_cu .. first_cu+n_cu-1 are set when invert == 0, all
 * the others (of total_cu) when invert != 0; consecutive mask bits fall on consecutive XCDs.  *stream_out is a hipStream_t
 * (wrap it with torch.cuda.ExternalStream); destroy with pn_stream_destroy.  No reference counterpart. */
int pn_stream_create_cu_mask(uint32_t total_cu, uint32_t first_cu, uint32_t n_cu, int invert, void** stream_out);
int pn_stream_destroy(void* stream);
/* Test / tuning hook: rounds (windows of 8 ray points) a ray gets in the first march launch before it is handed to the
 * wave-per-ray tail launch; 0 restores the default (4).  The samples do not depend on it (bit for bit) — tests use 1 and a
 * large value to push every ray through either launch.  Affects renders enqueued afterwards, process-wide. */
int pn_march_set_tail_rounds(int rounds);
/* Tests / experiments: 0 makes the frame driver's skip pre-pass walk hop by hop (rounds 1-2), 1 restarts the hop chain just before the first search cell
 * with candidates and hands stragglers to the windowed march, and — --cut frames — crosses the empty regions of the static background (8^3-voxel blocks of
 * the density bitfield without an occupied voxel on any level, outside the cut box) by walking the ray's t-sequence instead of visiting their voxels (the
 * default), -1 restores the default (1).  Same results bit for bit.  Takes effect for renders enqueued (or captured) afterwards,
 * process-wide. */
int pn_march_set_skip_dda(int on);
/* Number of compute units of the current device. */
int pn_device_cu_count(void);
/* Text of the last PN_ERR_HIP on the calling thread ("" if none). */
const char* pn_last_error(void);

/* ------------------------------------------------------------------ raymarching ---- */

/* raymarching/src/raymarching.h:8 sph_from_ray (kernel raymarching.cu:165-202): coords [N,2] in [-1,1] where each ray leaves the sphere. */
int pn_sph_from_ray(const float* rays_o, const float* rays_d, float radius, uint32_t N, float* coords, void* stream);
/* raymarching/src/raymarching.h:7 near_far_from_aabb (kernel raymarching.cu:91-159). */
int pn_near_far_from_aabb(const float* rays_o, const float* rays_d, const float* aabb, uint32_t N, float min_near, float* nears, float* fars,
                          void* stream);

/* raymarching/src/raymarching.h:20-36 march_rays_quadratic_bending (kernel raymarching.cu:1121-1434,
 * host :1436-1489).  Same argument order as the pybind function (p_def before p_ori).
 * xyzs [M,3], dirs [M,3], deltas [M,2] must be zero-filled, M >= n_alive*n_step.
 * num_seek_IP must be in [1,3] (get_opts.py:97,117-120).  err_flag (int[1], may be NULL) is OR-ed with
 * 1 when a sample's search cell falls outside the spatial-hash grid (reference: device printf "ERROR"). */
int pn_march_rays_quadratic_bending(const int* pig_cnt, const int* pig_bgn, const int* pig_idx, int n_vtx, int n_grid, const float* p_def,
                                    const float* p_ori, const float* F_IP, const float* dF_IP, int max_iter_num, const float* bbmin,
                                    const float* bbmax, float hgs, const int* resolution, int num_seek_IP, float IP_dx, int cut,
                                    const float* cut_bounds, uint32_t n_alive, uint32_t n_step, const int* rays_alive, const float* rays_t,
                                    const float* rays_o, const float* rays_d, float bound, float dt_gamma, uint32_t max_steps, uint32_t C,
                                    uint32_t H, const uint8_t* grid, const float* nears, const float* fars, float* xyzs, float* dirs,
                                    float* deltas, const float* noises, int* err_flag, void* stream);

/* raymarching/src/raymarching.h:18 composite_rays (kernel raymarching.cu:827-923).  In place on rays_alive,
 * rays_t, weights_sum, depth, image. */
int pn_composite_rays(uint32_t n_alive, uint32_t n_step, float T_thresh, int* rays_alive, float* rays_t, const float* sigmas, const float* rgbs,
                      const float* deltas, float* weights_sum, float* depth, float* image, void* stream);

/* nerf/renderer.py:887  rays_alive = rays_alive[rays_alive >= 0]  — stable stream compaction.
 * out [n] receives the survivors in order; *n_out (device int[1]) their count.  scratch: >= pn_compact_scratch_ints(n) ints. */
int pn_compact_rays(const int* rays_alive, uint32_t n, int* out, int* n_out, int* scratch, void* stream);
uint32_t pn_compact_scratch_ints(uint32_t n);

/* nerf/utils.py:355-443 get_pnts_in_grids (+ Warp kernels get_pig_cnt / get_pig_idx / p2g).  Slot order inside a
 * cell is ascending point id (the reference's is atomic-race order).  bbmin [3] and resolution [3] are device arrays,
 * as in the reference.  err_flag (may be NULL) is OR-ed with 2 when a point's cell id is outside [0,n_grid). */
int pn_pnts_in_grids(int n_vtx, int n_grid, const float* pnts, const float* bbmin, float hgs, const int* resolution, int* pig_cnt, int* pig_bgn,
                     int* pig_idx, int* err_flag, void* stream);

/* nerf/utils.py:54-138 get_rays, N=-1 path.  pose: device pointer to the row-major 4x4 cam2world (the reference's `poses[0]`).
 * rays_o/rays_d [H*W,3]. */
int pn_get_rays(const float* pose, float fx, float fy, float cx, float cy, int H, int W, float* rays_o, float* rays_d, void* stream);

/* ------------------------------------------------------------------ gridencoder ---- */

/* gridencoder/src/gridencoder.h:12 grid_encode_forward (kernel gridencoder.cu:87-245, D=3, C in {1,2,4,8}, fp32).
 * dy_dx: NULL, or [B, L, 3, C] (the `calc_grad_inputs` branch, :199-243; training side).  offsets_host [host]: the L+1 int32 level offsets (the reference passes a device tensor; the
 * launcher derives per-level scale / resolution / table size on the host with the reference's formulas :132-134 and
 * hands them to the kernel by value).  outputs [L,B,C] exactly like the reference kernel; with out_bl_major != 0 the
 * kernel writes [B, L*C] directly (what grid.py:57 produces by permute+reshape). */
int pn_grid_encode_forward(const float* inputs, const float* embeddings, const int* offsets_host, float* outputs, uint32_t B, uint32_t D,
                           uint32_t C, uint32_t L, float S, uint32_t H, float* dy_dx, uint32_t gridtype, int align_corners,
                           uint32_t interp, int out_bl_major, void* stream);

/* grid_encode_forward on a half table (AT_DISPATCH_FLOATING_TYPES_AND_HALF, gridencoder.cu:448-471 -> kernel_grid<at::Half,3,C>): embeddings
 * [sO,C] and outputs fp16 (bit patterns), inputs fp32; no dy_dx (inference).  What GridEncoder.forward launches under autocast. */
int pn_grid_encode_forward_half(const float* inputs, const uint16_t* embeddings, const int* offsets_host, uint16_t* outputs, uint32_t B, uint32_t D,
                                uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype, int align_corners, uint32_t interp,
                                int out_bl_major, void* stream);

/* ------------------------------------------------------------------ shencoder ---- */

/* shencoder/src/shencoder.h:9 sh_encode_forward (kernel shencoder.cu:27-123), D=3, degree C in [1,4]; dy_dx NULL or [B, 3, C*C]
 * (:125-355). */
int pn_sh_encode_forward(const float* inputs, float* outputs, uint32_t B, uint32_t D, uint32_t C, float* dy_dx, void* stream);

/* ------------------------------------------------------------------ static inference ops (off the hot path) */

/* march_rays (raymarching/src/raymarching.cu:703-824, wrapper raymarching.py:327-360): the undeformed march against the density
 * bitfield, up to n_step samples per alive ray.  xyzs/dirs [n_alive*n_step,3], deltas [..,2] zero-filled by the caller; noises
 * [n_alive] or NULL (= 0). */
int pn_march_rays(uint32_t n_alive, uint32_t n_step, const int* rays_alive, const float* rays_t, const float* rays_o, const float* rays_d,
                  float bound, float dt_gamma, uint32_t max_steps, uint32_t C, uint32_t H, const uint8_t* grid, const float* nears,
                  const float* fars, float* xyzs, float* dirs, float* deltas, const float* noises, void* stream);
/* packbits (raymarching.cu:270-303): bitfield[n] bit i = grid[8n+i] > density_thresh; N = number of bytes. */
int pn_packbits(const float* grid, uint32_t N, float density_thresh, uint8_t* bitfield, void* stream);
/* morton3D / morton3D_invert (raymarching.cu:217-263): coords [N,3] int32 <-> indices [N] int32. */
int pn_morton3D(const int* coords, uint32_t N, int* indices, void* stream);
int pn_morton3D_invert(const int* indices, uint32_t N, int* coords, void* stream);

/* ------------------------------------------------------------------ training ops (off the hot path) */

/* march_rays_train (raymarching/src/raymarching.h:13, kernel raymarching.cu:314-483, wrapper raymarching.py:163-236).  xyzs/dirs [M,3],
 * deltas [M,2] zero-filled by the caller; rays [N,3] = (ray id, point offset, point count); counter[2] += (points demanded, N).
 * DIFFERENCE (documented): the reference hands out offsets and ray rows with atomicAdd (race order); here row n is ray n
 * and offsets are the exclusive prefix sum of the counts (count -> single-workgroup scan -> write), so the output is reproducible.
 * Rays whose range passes M are dropped like the reference's (:415).  noises [N] or NULL. */
int pn_march_rays_train(const float* rays_o, const float* rays_d, const uint8_t* grid, float bound, float dt_gamma, uint32_t max_steps, uint32_t N,
                        uint32_t C, uint32_t H, uint32_t M, const float* nears, const float* fars, float* xyzs, float* dirs, float* deltas, int* rays,
                        int* counter, const float* noises, void* stream);
/* composite_rays_train_forward / _backward (raymarching.h:14-15, kernels raymarching.cu:503-581,604-686). */
int pn_composite_rays_train_forward(const float* sigmas, const float* rgbs, const float* deltas, const int* rays, uint32_t M, uint32_t N, float T_thresh,
                                    float* weights_sum, float* depth, float* image, void* stream);
int pn_composite_rays_train_backward(const float* grad_weights_sum, const float* grad_image, const float* sigmas, const float* rgbs,
                                     const float* deltas, const int* rays, const float* weights_sum, const float* image, uint32_t M, uint32_t N,
                                     float T_thresh, float* grad_sigmas, float* grad_rgbs, void* stream);
/* grid_encode_backward (gridencoder.h:13, kernels gridencoder.cu:248-369): grad [L,B,C]; grad_embeddings [sO,C] zero-filled by the
 * caller, accumulated with hardware fp32 atomics; dy_dx / grad_inputs [B,3] both NULL or both given. */
int pn_grid_encode_backward(const float* grad, const float* inputs, const float* embeddings, const int* offsets_host, float* grad_embeddings,
                            uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, const float* dy_dx, float* grad_inputs,
                            uint32_t gridtype, int align_corners, uint32_t interp, void* stream);
/* The same under autocast (kernel_grid_backward<at::Half>, gridencoder.cu:248-341 with the __half2 atomicAdd of :324-331; grid.py:43-44 casts the table to
 * half): grad [L,B,C] half, grad_embeddings [sO,C] HALF, zero-filled by the caller; every contribution is rounded to half and accumulated with packed
 * half atomics (global_atomic_pk_add_f16), C in {2, 4, 8}.  The sum of halves depends on the order the atomics meet in, here as in the reference: results
 * agree with the fp32 backward to the rounding of half sums.  No input gradients on this path. */
int pn_grid_encode_backward_half(const uint16_t* grad, const float* inputs, const int* offsets_host, uint16_t* grad_embeddings, uint32_t B, uint32_t D,
                                 uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype, int align_corners, uint32_t interp, void* stream);
/* grad_total_variation (gridencoder.h:15, kernel gridencoder.cu:506-611): grad [sO,C] += TV gradient at the cells of `inputs` [B,3] in [0,1]. */
int pn_grad_total_variation(const float* inputs, const float* embeddings, float* grad, const int* offsets_host, float weight, uint32_t B, uint32_t D,
                            uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype, int align_corners, void* stream);
/* sh_encode_backward (shencoder.h:10, kernel shencoder.cu:358-383): grad_inputs [B,3] += grad [B,C*C] . dy_dx [B,3,C*C]. */
int pn_sh_encode_backward(const float* grad, const float* inputs, uint32_t B, uint32_t D, uint32_t C, const float* dy_dx, float* grad_inputs,
                          void* stream);

/* ------------------------------------------------------------------ network -------- */

/* NeRFNetwork.forward (nerf/network.py:98-127): hash grid (16x2) -> 32->64->16 -> exp | SH(16)+15 -> 31->64->64->3 -> sigmoid,
 * no biases, fp32 in / fp32 out, fused in one kernel; the dense layers run on the bf16 matrix cores as a three-way split with fp32
 * accumulation (fp32-accurate: ~5e-6 relative on sigma).  Weights row-major [out,in] as in the state dict.
 * pn_net_create packs them (and the per-level table geometry) into a device-side context. */
typedef struct pn_net pn_net;
int pn_net_create(pn_net** out, const float* embeddings /*device, [n,2]*/, const int* offsets_host /*[L+1]*/, uint32_t L, uint32_t C,
                  float per_level_scale_log2, uint32_t base_resolution, float bound, const float* W0_host, const float* W1_host,
                  const float* W2_host, const float* W3_host, const float* W4_host, void* stream);
void pn_net_destroy(pn_net* net);
/* Refreshes the packed weights of an existing context in place after the parameters changed (training: every optimizer step invalidates
 * them): host-side packing into the context's pinned staging buffer + two asynchronous uploads on `stream`.  No allocation, no stream
 * synchronisation (it waits only for the previous refresh's own upload event).  `embeddings` replaces the table pointer; when the fp16
 * tables exist they are re-rounded from it.  PN_ERR_ARG while `stream` is being captured (the packing cannot be replayed). */
int pn_net_update(pn_net* net, const float* embeddings, const float* W0_host, const float* W1_host, const float* W2_host, const float* W3_host,
                  const float* W4_host, void* stream);
/* Form of the fp32 network's dense layers on `net` (chosen by pn_net_create / pn_net_update from the weights and the tables): 2 = fp16 hi/lo pieces on the
 * fp16 matrix pipe (every fp32 value as hi + lo, 22 significant bits; three products per K chunk; 4e-6 relative on sigma against the sequential fp32 oracle,
 * as the bf16 form), every layer's inputs carried at the power of two that puts their interval bound (tables' largest entry x row sums of |W|) into
 * [2^13, 2^14], the scales folded into the weight image — taken whenever those bounds are finite and positive; 0 = three bf16 pieces, six products (any
 * weights: an all-zero layer, a non-finite weight).  PN_NET_FORM=bf16 in the environment forces 0. */
int pn_net_form(const pn_net* net);
/* Number of times pn_net_update changed that form since pn_net_create.  The per-layer scales of form 2 live in device memory beside the weight image and are
 * read by the kernels, so launches captured into HIP graphs follow an in-place refresh; the FORM itself (kernel template + image) is fixed in a captured
 * launch: graphs captured under another epoch must be captured again (pienerf_amd/harness.py refuses to replay them). */
int pn_net_form_epoch(const pn_net* net);
/* Creates the fp16 copy of the hash tables (`embeddings.to(torch.half)`, gridencoder/grid.py:43-44; round to nearest even) once; the fp16
 * weight image always exists.  Call before the first *_half launch or fp16 render, outside stream capture. */
int pn_net_enable_half(pn_net* net, void* stream);
/* sigmas[M], rgbs[M,3] for xyzs[M,3] in [-bound,bound], dirs[M,3] unit.  density_scale multiplies sigma (renderer.py:875). */
int pn_nerf_forward(const pn_net* net, const float* xyzs, const float* dirs, uint32_t M, float density_scale, float* sigmas, float* rgbs,
                    void* stream);
/* The same under autocast (fp16 tables, half Linear layers on v_mfma_f32_32x32x16_f16, half activations): sigmas fp32 (trunc_exp casts to
 * float, nerf/activation.py:7), rgbs fp32 holding the half-rounded sigmoid outputs. */
int pn_nerf_forward_half(const pn_net* net, const float* xyzs, const float* dirs, uint32_t M, float density_scale, float* sigmas, float* rgbs,
                         void* stream);
/* NeRFNetwork.density (nerf/network.py:129-146): sigma = trunc_exp(h[0]) (no density_scale), geo_feat = h[1:16]; the same fused
 * kernel stopped after the sigma net.  Used off the hot path (point sampling, main_sample.py:164-168).  sigmas [M], geo_feat [M,15]. */
int pn_nerf_density(const pn_net* net, const float* xyzs, uint32_t M, float* sigmas, float* geo_feat, void* stream);
int pn_nerf_density_half(const pn_net* net, const float* xyzs, uint32_t M, float* sigmas, float* geo_feat, void* stream);
/* density_scale * sigma only (no geo_feat written): what update_extra_state needs from density() over 2-4 M cell samples
 * (nerf/renderer.py:493-495); half != 0 selects the fp16 form. */
int pn_nerf_sigma(const pn_net* net, const float* xyzs, uint32_t M, float density_scale, float* sigmas, int half, void* stream);
/* [host] fp32 -> fp16 bit patterns, round to nearest even: the rounding the host side of pn_net_create applies to the weights. */
int pn_host_float_to_half(const float* in_host, uint16_t* out_host, uint32_t n);

/* ------------------------------------------------------------------ background model -- */

/* The background model of NeRFNetwork with bg_radius > 0 (nerf/network.py:73-95,148-164; nerf/renderer.py:283-288, 799-801, 896), one launch per frame
 * (csrc/pn_background.hip): ray -> exit point on the sphere of `radius` as (theta, phi) in [-1, 1] (the arithmetic of pn_sph_from_ray, bit for bit)
 * -> 2-D grid encoder (4 levels x 2 features, inputs (x + 1) / 2) -> cat([SH degree 4 of rays_d, grid features]) -> Linear 24 -> 64, ReLU -> Linear 64 -> 3
 * -> sigmoid.  pn_bg_net_create packs W0 [64,24] and W1 [3,64] (row-major [out,in], host) and the level geometry; `embeddings` (device, [offsets[L], 2]
 * fp32) is read in place, not copied.  L must be 4 and C 2; every level either fully dense or hashed into a power-of-two table (else PN_ERR_ARG).
 * pn_bg_net_update refreshes the packed weights in place after the parameters changed: host packing into pinned staging + one asynchronous upload on
 * `stream`, one stream synchronisation (the table's largest entry chooses the fp16 pieces' scale), no allocation.  Both are PN_ERR_ARG while `stream` is
 * being captured. */
typedef struct pn_bg_net pn_bg_net;
int pn_bg_net_create(pn_bg_net** out, const float* embeddings, const int* offsets_host /*[L+1]*/, uint32_t L, uint32_t C, float per_level_scale_log2,
                     uint32_t base_resolution, const float* W0_host, const float* W1_host, void* stream);
int pn_bg_net_update(pn_bg_net* net, const float* embeddings, const float* W0_host, const float* W1_host, void* stream);
void pn_bg_net_destroy(pn_bg_net* net);
/* rays_o, rays_d [N,3].  Two modes: rgb_out [N,3] != NULL (weights_sum == image == NULL) receives the colour; or weights_sum [N] and image [N,3] != NULL
 * (rgb_out == NULL): image = image + (1 - weights_sum) * rgb IN PLACE, the multiply and the add rounded separately (torch's two ops, bit for bit given the
 * same rgb).  coords_out [N,2] (may be NULL): the (theta, phi) the kernel used, for tests.  fp32-accurate (fp16 hi + lo pieces on the matrix cores, 2e-6
 * on the colour against sequential fp32 sums).  No host synchronisation, no allocation: legal inside a HIP-graph capture; a captured launch follows
 * pn_bg_net_update.  N <= (2^31 - 1) / 3. */
int pn_background_forward(const pn_bg_net* net, const float* rays_o, const float* rays_d, uint32_t N, float radius, float* rgb_out,
                          const float* weights_sum, float* image, float* coords_out, void* stream);
/* The same as the reference computes it under autocast (half table entries, kernel_grid<at::Half>'s half accumulation, half Linear layers with fp32
 * accumulation, half sigmoid): the colours are half values held in fp32. */
int pn_background_forward_half(const pn_bg_net* net, const float* rays_o, const float* rays_d, uint32_t N, float radius, float* rgb_out,
                               const float* weights_sum, float* image, float* coords_out, void* stream);

/* NeRFNetwork.background(x, d) (nerf/network.py:148-164) on coordinates the caller already has: coords [N,2] in [-1,1], dirs [N,3] -> rgb_out [N,3]; the
 * same kernel with the coordinate read instead of derived.  half != 0: the autocast form. */
int pn_background_coords(const pn_bg_net* net, const float* coords, const float* dirs, uint32_t N, float* rgb_out, int half, void* stream);

/* NeRFNetwork.color(x, d, mask, geo_feat) (nerf/network.py:165-194; csrc/pn_hier.hip): rgbs [M,3] = sigmoid(colour net([SH16(dirs) | geo_feat])) on
 * the rows whose mask byte is non-zero (mask == NULL: every row) and exact zeros elsewhere.  dirs [M,3], geo_feat [M,15] fp32 as pn_nerf_density wrote
 * them, mask [M] bytes.  The matrix work is proportional to the number of masked rows (they are compacted into 32-row tiles per wave).  No host
 * synchronisation, no allocation.  M <= (2^31 - 1) / 15.  _half: the autocast form (geo_feat holds half values, rgbs the half-rounded sigmoid outputs;
 * needs pn_net_enable_half). */
int pn_nerf_color(const pn_net* net, const float* dirs, const float* geo_feat, const uint8_t* mask, uint32_t M, float* rgbs, void* stream);
int pn_nerf_color_half(const pn_net* net, const float* dirs, const float* geo_feat, const uint8_t* mask, uint32_t M, float* rgbs, void* stream);

/* NeRFRenderer.run (nerf/renderer.py:137-265), the hierarchical-sampling render of a model without a density grid, eval() mode (det = True, no perturb),
 * in one launch: per ray num_steps stratified samples between near and far of `aabb` ([host] six floats), their densities, upsample_steps samples drawn from
 * the resulting weights (sample_pdf), their densities, the merge, the colour of the samples whose weight exceeds 1e-4, and the sums
 *   weights_sum [N] = sum w,  depth [N] = sum w clamp((z - near) / (far - near), 0, 1)  (NaN for a ray that misses the box),
 *   image [N,3] = sum w rgb + (1 - weights_sum) * background,  background = bg_rays [N,3] when not NULL, else bg_scalar (0: composite over nothing).
 * One wave per ray, the sample set in LDS (csrc/pn_hier.hip): num_steps + upsample_steps <= pn_hier_max_samples(), num_steps >= 1, and >= 3 when
 * upsample_steps > 0 (else PN_ERR_ARG).  half must be 0: there is no autocast form of this launch.  Results are a pure function of the ray (fixed summation
 * order): they do not depend on N or on the order of the rays.  No host synchronisation, no allocation: legal inside a HIP-graph capture. */
int pn_render_hier(const pn_net* net, const float* rays_o, const float* rays_d, uint32_t N, const float* aabb_host, float min_near, int num_steps,
                   int upsample_steps, float density_scale, float bg_scalar, const float* bg_rays, float* image, float* depth, float* weights_sum, int half,
                   void* stream);
/* [host] largest num_steps + upsample_steps pn_render_hier takes. */
int pn_hier_max_samples(void);

/* ------------------------------------------------------------------ whole frame ---- */

/* NeRFRenderer.rund_cuda (nerf/renderer.py:755-907) for one frame with no host synchronisation inside the loop:
 * bbox/resolution of the deformed IPs, spatial hash, near/far, then trips of { march, network, composite,
 * stable compaction } driven by a device-side (n_alive, n_step) record that follows renderer.py:839-846,887-891.
 * Results are those of the op-by-op loop.  Workspace comes from pn_frame_create (sized for N rays, n_vtx IPs). */
typedef struct pn_frame pn_frame;
typedef struct {
    int max_iter_num;     /* --max_iter_num */
    float hash_grid_size; /* opt.hash_grid_size = 1.2*sim_dx (get_opts.py:96) */
    int num_seek_IP;
    float IP_dx;          /* model.IP_dx = 1.05*sim_dx (main_gui.py:56) */
    int cut;
    float cut_bounds[6];
    float bound;
    float min_near;
    float dt_gamma;
    uint32_t max_steps;
    float T_thresh;
    uint32_t cascade;     /* C */
    uint32_t grid_size;   /* H = 128 */
    float density_scale;
    float bg_color;       /* scalar background (renderer.py:803-804: bg_color = 1) */
    int fp16;             /* != 0: the network runs as under torch.cuda.amp.autocast (trainer.py:561, Trainer(fp16=True)): fp16 hash tables
                             (gridencoder/grid.py:43-44), fp16 MFMA layers with half-rounded activations; needs pn_net_enable_half */
    int reuse_tables;     /* != 0: the IP state (p_def, F, dF) is the one of the previous pn_render_deformed on this workspace — keep its bounding box,
                             spatial hash, candidate lists and packed records and only start new rays.  For a frame rendered in ray batches
                             (max_ray_batch, get_opts.py:24): the reference rebuilds get_pnts_in_grids for every rund_cuda call */
    int ray_batch;        /* > 0 (>= 64): the frame is rendered as ray batches of this many rays (opt.max_ray_batch = 4096, get_opts.py:24; the
                             staging loop of nerf/renderer.py:562-576) — every batch with its OWN trip schedule n_step = max(min(N_b // n_alive_b, 8), 1)
                             and its own max_steps count, exactly as if the batches were rendered one after the other, but all batches advance
                             inside the same launches (rays are independent; the alive list stays sorted by ray id, so a batch is a contiguous
                             run of it).  0: one schedule for the whole ray set (what the reference's render_deformed does, renderer.py:587-600).
                             Deformed render only. */
    int throughput;       /* > 0: the THROUGHPUT form of the frame's first trip — its first march pass walks every ray with ONE lane (one visited point of
                             the ray's chain per round, up to this many rounds; rays that outlast them go on in the wave-per-ray windows) instead of
                             evaluating windows of 8 / 64 consecutive lattice elements of which the chain visits one in 4.6: a quarter of the vector work
                             per visited point, bit-identical samples, a longer first trip (~7 us per round).  For pipelines that keep several frames in
                             flight (harness.capture_pipelined with more than one lane: +8 % steps/s on the chair, +13 % on configs[4]); 0: the latency
                             form.  Deformed render only. */
    int throughput_trips; /* with throughput > 0: how many leading trips of the frame march in that form (0 or 1: the first trip only).  Worth it for a
                             trip that still has rays enough to fill the GPU with one lane each (>= ~128 k alive: the second trip of the trex option
                             set, 246 k rays x 3 samples: +11 % steps/s); a trip of few rays with 8 samples each is faster in the windows.  The
                             results do not depend on it.  harness.capture_pipelined picks it from the trip records of its warm-up frame. */
    int ray_tile_w;       /* > 0: the N rays are the row-major pixels of an image this wide (get_rays, nerf/utils.py:65-147 with error_map None).  The
                             frame then walks them in 16 x 4 pixel tiles instead of runs of 64 pixels of a row: rays_alive starts as that permutation
                             of arange(N) (renderer.py:828) and every later list inherits the order, so the 64 rays that share a wave march about
                             equally long and fewer waves hold a silhouette ray (chair: skip pre-pass -17 %, tail pass -6 %, one-lane pass -10 %;
                             the network kernel's gathers share fewer lines, +2 %; +4 % steps/s).  Per-ray results do not depend on the order of
                             the alive list (each ray's samples, its composite and its pixel are its own); ignored unless ray_tile_w % 16 == 0 and
                             N % (4 * ray_tile_w) == 0, with ray_batch > 0 (whose batches are contiguous runs of a sorted alive list) and by
                             pn_render_static. */
    int fused_from;       /* the loop trips from this one on run as ONE persistent launch (csrc/pn_trips_fused.h): once n_alive <= N / 8 the reference's
                             n_step = max(min(N // n_alive, 8), 1) (renderer.py:839-846) is 8 for the rest of the frame, so every ray can loop
                             { march 8 samples; network; composite } on its own until it dies — the per-ray arithmetic, the samples, the pixels and the
                             per-trip counts of the trip-by-trip loop, without its 4-6 launches and its compaction per trip.
                             0: from trip 1 (right behind the frame's first trip; the chair);
                             k >= 1: the first k trips as per-trip launches (a scene whose second trip still has more than N / 8 rays alive: the trex
                             option set — harness.capture_pipelined reads k off its warm-up frame); < 0: never.  If the launch finds n_step < 8 at
                             its first trip it does nothing and the frame is continued like one that ran out of captured trips (pn_render_continue;
                             the blocking pn_render_deformed runs one per-trip trip and tries again).  Not with ray_batch > 0 (batches keep their own
                             n_step), not for pn_render_static, not for max_steps > 1024. */
    int fused_whole;      /* != 0 (with fused_from == 0): the WHOLE frame behind the skip pre-pass in that launch, first trip included, where that
                             applies — the first trip couples the rays only through the next trip's n_step, and n_alive there cannot exceed the rays the
                             skip pre-pass left anything to march for: the launch checks on the device that those are at most N / 8 (the chair: 10 % of the
                             rays meet the bounding box of the integration points) and does nothing otherwise; the blocking pn_render_deformed then runs
                             the first trip as per-trip launches and fuses from trip 1, a fixed-trip render is left unfinished at trip 0 and finished by
                             pn_render_continue.  Inside the launch the first trip is three kinds of work items per workgroup (one lane per ray for a
                             bounded number of rounds; 64-lane windows for the rays still searching; network tile + composite + hand-over per finished
                             chunk of 64 rays) that its waves take whenever they hold no ray of a later trip.  A frame is then prologue (2 launches), skip
                             pre-pass, this launch, epilogue.  Measured on the chair (MI355X): one frame at a time 0.90 ms against 0.86 ms, three frames in
                             flight 1 730 against 1 930 steps/s (the workgroups of the launch hold a CU each while their first trip's dependency chain
                             leaves most of its waves waiting), two frames in flight 1 700-1 740 against 1 560: harness.capture_pipelined switches it on for
                             pipelines of two render lanes (what every rank of a multi-GPU job runs).  Same samples, records and pixels either way. */
    int fused_fold;       /* != 0 (with fused_from <= 1, without fused_whole): the first trip's NETWORK, COMPOSITE and COMPACTION inside the fused launch — the
                             trip's march stays what it is (skip pre-pass, one lane per ray or windows, tail pass: launches that use every CU) and leaves
                             its segmented sample list; the launch runs network tiles of 32 list entries, composites (one sample per ray) and takes the
                             survivors on through a per-workgroup list.  Four launches fewer on a frame's chain (k_list_pack, k_nerf_forward, k_composite,
                             k_compact).  Applies when at most N / 8 rays found a sample on the first trip (checked on the device: then n_step is 8 from the
                             second trip on); otherwise the launch does nothing and the frame goes on as with fused_whole.  Same results bit for bit. */
    int fused_grid;       /* workgroups of the fused launch (0: one per CU, its upper bound — 12 waves and 157 KB of LDS each, so a workgroup has its CU to
                             itself).  A pipeline with several frames in flight gives each frame's launch a part of the GPU, so that the launches of
                             different frames run side by side instead of one after the other and the rest of the frame's kernels (prologue, skip
                             pre-pass, first trip, simulator) find CUs whose LDS is free: measured on the chair with three render lanes, 64 / 96 / 128 / 160 /
                             192 / 256 workgroups: 1 798 / 1 939 / 1 937 / 1 874 / 1 799 / 1 721 steps/s (profiles/r04_fused_grid_sweep.txt);
                             harness.capture_pipelined passes half the CUs when it runs more than one lane.  The results do not depend on it. */
    int fused_order;      /* >= 0 (0, the default): a workgroup of the fused launch draws the packets of its share LONGEST FIRST — a packet is 8 consecutive
                             entries of the alive list, its length the largest far - t of its rays (what the ray still has to march; the frame prologue has
                             shortened `fars` to where the ray's candidates end), equal lengths in list order (csrc/pn_fused_order.h).  The launch is as
                             long as its longest wave, and what decides a workgroup's end is the rounds its last rays need one after the other: a long ray
                             drawn last costs all of them behind everybody else's work.  The shares stay what they are — no ray moves between
                             workgroups, packets stay packets.  The first 512 packets of a share are ordered, the ones behind them follow in list order.
                             Acts on the form whose rays come from the alive list (neither fused_whole nor fused_fold took the frame); the other two
                             draw from lists that fill while the launch runs.  < 0: list order, what the launch did before.  The results do not depend on
                             it: every ray's march, network tiles and composite are a function of the ray alone. */
} pn_render_opts;
int pn_frame_create(pn_frame** out, uint32_t max_rays, uint32_t max_vtx, uint32_t max_grid_cells);
void pn_frame_destroy(pn_frame* f);
/* rays_o/rays_d [N,3]; p_def/p_ori [n_vtx,3], F_IP [n_vtx,9], dF_IP [n_vtx,27]; bitfield [C*H^3/8];
 * outputs image [N,3], depth [N], depth_0 [N], weights_sum [N].  stats_host (may be NULL) [host, int64[5]] =
 * {trips, emitted samples, error flags, rays alive at exit, rays left alive by fixed-trip renders on this workspace since
 * pn_frame_reset_unfinished}; reading it synchronises the stream. */
int pn_render_deformed(pn_frame* f, const pn_net* net, const pn_render_opts* opts, const float* rays_o, const float* rays_d, uint32_t N,
                       const float* p_def, const float* p_ori, const float* F_IP, const float* dF_IP, int n_vtx, const uint8_t* bitfield,
                       float* image, float* depth, float* depth_0, float* weights_sum, int64_t* stats_host, void* stream);

/* Non-blocking form of pn_render_deformed for HIP-graph capture / host run-ahead: enqueues exactly n_trips loop trips
 * (trips past the last alive ray cost ~20 us each), the epilogue and an asynchronous copy of the trip records to pinned host
 * memory.  Never synchronises.  The frame is complete iff pn_render_status reports 0 rays alive at exit; otherwise render again
 * with more trips. */
int pn_render_deformed_async(pn_frame* f, const pn_net* net, const pn_render_opts* opts, const float* rays_o, const float* rays_d, uint32_t N,
                             const float* p_def, const float* p_ori, const float* F_IP, const float* dF_IP, int n_vtx, const uint8_t* bitfield,
                             float* image, float* depth, float* depth_0, float* weights_sum, int n_trips, void* stream);
/* stats_host [host, int64[5]] = {trips with alive rays, emitted samples, error flags, rays alive at exit, unfinished total} of the last render on f.
 * synchronize != 0: waits for `stream` first; 0: the caller guarantees the render has completed (e.g. through an event). */
int pn_render_status(pn_frame* f, int64_t* stats_host, int synchronize, void* stream);
/* Zeroes the workspace's running total of rays left alive by fixed-trip renders (stats[4]): a frame rendered as many captured ray batches is
 * verified once, at its end, instead of once per batch. */
int pn_frame_reset_unfinished(pn_frame* f, void* stream);

/* Continues the last render on `f` where its trips stopped (a fixed-trip render that pn_render_status reports with rays alive at exit — the
 * reference's loop simply keeps going, renderer.py:836-891): n_trips more trips (0: blocking, until no ray is alive), then the epilogue again.
 * The workspace holds the frame's tables, ray state and colour accumulator, so only the rays, the bitfield and the SAME output buffers are
 * needed; results equal those of one render with enough trips, bit for bit.  is_static: the frame came from pn_render_static. */
int pn_render_continue(pn_frame* f, const pn_net* net, const pn_render_opts* opts, const float* rays_o, const float* rays_d, uint32_t N,
                       const uint8_t* bitfield, float* image, float* depth, float* depth_0, float* weights_sum, int64_t* stats_host, int n_trips,
                       int is_static, void* stream);

/* NeRFRenderer.run_cuda, eval branch (nerf/renderer.py:305-387): the undeformed render — near / far from `aabb_host` [host, 6 floats:
 * aabb_infer], trips of { march_rays, network, composite_rays, compaction } with the same device-side trip record as pn_render_deformed, then
 * image += (1 - weights_sum) * bg, depth = clamp(depth - nears, 0) / (fars - nears).  n_trips == 0: blocking form (batches of trips
 * until no ray is alive); n_trips > 0: exactly that many trips, no host synchronisation (pn_render_status afterwards).  depth_0 receives the
 * un-normalised depth (the reference discards it).  "Rays alive at exit" of a static frame (stats[3]) also counts the rays that max_steps ended the loop
 * on, as NeRFRenderer.run_cuda_ops reports them: more trips do nothing for those (pn_render_continue leaves the frame as it is) and they are not
 * added to the unfinished total.  The deformed forms report 0 there.  Off the simulate-and-render hot path. */
int pn_render_static(pn_frame* f, const pn_net* net, const pn_render_opts* opts, const float* rays_o, const float* rays_d, uint32_t N,
                     const float* aabb_host, const uint8_t* bitfield, float* image, float* depth, float* depth_0, float* weights_sum,
                     int64_t* stats_host, int n_trips, void* stream);

/* ------------------------------------------------------------------ frame copies to the host (nerf/trainer.py:589-592) ---- */

/* The reference's device->host boundary: image / depth / depth_0 .cpu().numpy() per frame.  A pn_copier performs such copies without a HIP
 * stream: a host thread waits for `after_event` (a hipEvent_t recorded behind the producing kernels; NULL: no wait), hands the copy to the
 * HSA runtime (SDMA engine) and waits for its completion signal, so the render streams never carry it (this part runs four hardware queues
 * concurrently; a copy on a fifth stream makes everything time-slice, a copy on a render stream holds that stream for the PCIe time).
 * dst_host: pinned host memory (hipHostMalloc / torch pin_memory); src_dev: device memory.  Copies complete in submission order.
 * pn_copier_wait blocks until the copy with that ticket (and every earlier one) has completed; returns PN_ERR_HIP if any copy failed. */
typedef struct pn_copier pn_copier;
int pn_copier_create(pn_copier** out);
void pn_copier_destroy(pn_copier* c);
int pn_copier_submit(pn_copier* c, void* dst_host, const void* src_dev, uint64_t bytes, void* after_event, uint64_t* ticket);
int pn_copier_wait(pn_copier* c, uint64_t ticket);

/* ------------------------------------------------------------------ density-grid state (off the hot path) */

/* NeRFRenderer.mark_untrained_grid (nerf/renderer.py:390-452): density_grid [cascade, H^3] (morton order) gets -1 in every cell that no
 * camera sees — cell centre (2c/(H-1) - 1)(bound_c - bound_c/H), cam = (centre - t) @ R, z > 0 and |x|, |y| inside the frustum padded by one
 * cell.  poses [B,4,4] row-major cam2world on the device; *n_unseen (device int[1]) receives the number of such cells. */
int pn_mark_untrained_grid(const float* poses, uint32_t B, float fx, float fy, float cx, float cy, uint32_t cascade, uint32_t H, float bound,
                           float* density_grid, int* n_unseen, void* stream);
/* update_extra_state, full sweep (renderer.py:466-497): xyzs [cascade*H^3, 3] = jittered centre of every cell, row = cascade*H^3 + morton
 * index; noise [cascade*H^3, 3] uniform in [0,1) (torch.rand_like).  The caller evaluates sigma there (pn_nerf_density) and hands the result
 * to pn_density_grid_update as tmp_grid. */
int pn_density_cells_full(uint32_t cascade, uint32_t H, float bound, const float* noise, float* xyzs, void* stream);
/* update_extra_state, partial sweep of one cascade (renderer.py:499-527): N cells from rand_coords [N,3] (torch.randint(0,H)) + N picks
 * occ[floor(rand_pick * n_occ)] from the cascade's occupied cells (density_grid_cas > 0, compacted on the device: no host round trip);
 * tmp_grid_cas [H^3] is set to -1; indices [2N] (-1 where the occupied list is empty) and jittered xyzs [2N,3] come back; noise [2N,3].
 * scratch: >= pn_density_partial_scratch_ints(H) ints. */
int pn_density_cells_partial(uint32_t cas, uint32_t H, float bound, uint32_t N, const int* rand_coords, const float* rand_pick, const float* noise,
                             const float* density_grid_cas, float* tmp_grid_cas, int* scratch, int* indices, float* xyzs, void* stream);
uint64_t pn_density_partial_scratch_ints(uint32_t H);
/* tmp_grid_cas[indices[m]] = sigmas[m] for indices >= 0 (renderer.py:527). */
int pn_density_scatter(uint32_t n, const int* indices, const float* sigmas, float* tmp_grid_cas, void* stream);
/* renderer.py:535-543: density_grid = where(grid >= 0 & tmp >= 0, max(grid * decay, tmp), grid) over n = cascade*H^3 cells; mean_thresh
 * (device float[2]) = { mean(clamp(grid, 0)), min(mean, density_thresh) } by a fixed-order reduction; bitfield = packbits(grid > threshold)
 * with the threshold read from the device.  partial: >= ceil(n / 256) doubles of scratch. */
int pn_density_grid_update(uint32_t n, float* density_grid, const float* tmp_grid, float decay, float density_thresh, uint8_t* bitfield,
                           double* partial, float* mean_thresh, void* stream);

/* Measurement hook (bench.py).  `enable` is a bitmask: bit 0 (1) — renders on f accumulate march work counters on the device,
 * {marching-loop iterations, candidate entries scanned, per-IP inverse warps, samples emitted}, the units behind the march
 * kernel's algorithmic-bytes figure (the counters add atomics, so never time with this bit set);
 * bit 1 (2) — blocking renders bracket each trip's march and network launches with HIP events (see pn_frame_trip_times);
 * bit 2 (4) — the fused launches of the later trips (pn_render_opts.fused_from) sum per-phase shader-clock cycles over their waves (see
 * pn_frame_fused_clocks; a drain of the memory counters at every phase boundary: never time `value` with it);
 * 0 switches all off.  counters_host (uint64[4], may be NULL): synchronises and reads the totals accumulated so far
 * (before any re-zeroing caused by enabling). */
int pn_frame_march_counters(pn_frame* f, int enable, uint64_t* counters_host, void* stream);
/* With bit 2: clocks_host (uint64[16], may be NULL; synchronises) = cycles summed over the waves of the fused launches on f since the last reset for
 * {hand-out of rays, march (8-lane window round), march (64-lane windows of the rays still going), network, composite}, then wave-rounds, waves,
 * wave lifetimes in 100 MHz ticks (sum), the largest round count and the longest lifetime of a wave; [10..14] (whole-frame form, fused_from = 0): the
 * first trip's one-lane march, its 64-lane windows, its network, its composite + hand-over, the wait at the workgroup barrier behind it; [15]: the form
 * of the last render's fused launch (0 later trips only, 1 whole frame, 2 first trip folded in);
 * *first_trip_out (may be NULL) = the trip at which the last render on f switched to the fused launch, -1 if it did not.  reset != 0: zero the sums. */
int pn_frame_fused_clocks(pn_frame* f, uint64_t* clocks_host, int* first_trip_out, int reset, void* stream);
/* The drawing order of pn_render_opts.fused_order for ONE share, computed on the host by the functions the kernel runs (csrc/pn_fused_order.h): rays_t /
 * fars [host, n_rays] are the share's rays in list order, perm_out [host, ceil(n_rays / 8)] receives the packet drawn k-th.  No GPU needed. */
int pn_fused_order_host(const float* rays_t, const float* fars, int n_rays, int* perm_out);
/* With bit 1 of `enable` set: the per-trip durations (ms, HIP events on the launch stream) of the last blocking render:
 * *n_trips_out entries in each array. */
/* Diagnostics: the device's per-trip records of the last render on `f` as int[max_trips][5] = (n_alive, n_step, step_base, n_samples, n_emitted; -1 on trips whose list is compacted)
 * and the number of rays each trip handed to the wave-per-ray tail pass.  Synchronises the stream. */
int pn_frame_trip_records(pn_frame* f, int* records_host, int* tail_counts_host, int max_trips, void* stream);
int pn_frame_trip_times(pn_frame* f, float* march_ms_host, float* network_ms_host, int max_trips, int* n_trips_out, void* stream);

/* ------------------------------------------------------------------ simulator ------ */

/* Simulator.get_IP_info (simulator/solver.py:402-424) = update_F_kernel (simulator/cuda_utils.py:206-233) + the
 * permute/cast: pos [n_IP,3], F [n_IP,9] (flat c*3+r), dF [n_IP,27] (flat c*9+r*3+j), fp32.
 * topo [n_IP,8] int32; dof [10 n_k,3]; Nx [n_IP,8,10]; dNx [n_IP,8,3,10]; ddNx [n_IP,8,3,3,10] fp64. */
int pn_sim_update_F(int n_IP, const int* topo, const double* dof, const double* Nx, const double* dNx, const double* ddNx, float* pos, float* F,
                    float* dF, void* stream);

/* calc_elastic (simulator/cuda_utils.py:83-121) + volume_invariant_project (simulator/func_utils.py:21-40).
 * RF, VF [n_IP,3,3] fp64 row-major; FF may be NULL.
 * mcadams_sweeps (here and in pn_sim_stepforward / pn_sim_stepforward_cells): which decomposition stands in for wp.svd3 (simulator/cuda_utils.py:107;
 * warp-lang is third-party and absent), for this call only:
 *   0            converged Jacobi — the contract: U, V proper rotations, the sign of det F on the last singular value;
 *   n in 1..64   the published algorithm wp.svd3 implements (McAdams et al., UW-Madison TR1690) with n fixed Jacobi sweeps, approximate Givens
 *                quaternions, negating-swap sort, Givens-quaternion QR, the paper's 10-digit constants (8 = double-precision setting, 4 = the paper's
 *                single-precision one).  oracle/sim_oracle.cpp: svd3_mcadams is the CPU restatement it is tested against;
 *   otherwise    PN_ERR_ARG.
 * pn_sim_stepforward_coop has the converged Jacobi only. */
int pn_sim_calc_elastic(int n_IP, const int* topo, const double* dNx, const double* dof, double* RF, double* VF, double* FF, int mcadams_sweeps,
                        void* stream);

/* collect_rhs_IP (simulator/cuda_utils.py:124-151) in its deterministic gather form (the reference ships the same
 * idea unused: collect_rhs_kernel :153-188, CSR built at solver.py:284-313).  csr_bg/csr_cnt [n_k], csr_buf [8 n_IP]
 * of (vid*8+dir) ascending per kernel.  rhs [10 n_k,3] is overwritten. */
int pn_sim_collect_rhs(int n_k, double dx, const int* csr_bg, const int* csr_cnt, const int* csr_buf, const double* mu, const double* lam,
                       const double* dNx, const double* RF, const double* VF, double* rhs, void* stream);

/* Y[n,3] = A[n,n] X[n,3]: the kron(A,I3) form of `global_matrix @ rhs` / `mass_matrix_invt2 @ dof_tilde`
 * (simulator/solver.py:493-496,532-538,576,600). */
int pn_sim_matvec3(int n, const double* A, const double* X, double* Y, void* stream);

/* Simulator.stepforward (simulator/solver.py:595-602) incl. compute_momentum (:574-576) and build_rhs (:541-571).
 * All vectors [10 n_k,3] fp64.  dof and dof_vel are updated in place.  work: >= pn_sim_work_doubles(n_k, n_IP) doubles.
 * prepared != 0: pn_sim_prepare has run on this `work` (the gather's chunk layout is there, and the per-IP rotations the local step's SVD is
 * warm-started from — they carry over from one local/global iteration and substep to the next); 0: the layout is rebuilt in this call and every
 * SVD starts from the identity.  mcadams_sweeps: the decomposition, see pn_sim_calc_elastic. */
int pn_sim_stepforward(int n_k, int n_IP, int iters, double dt, double dx, const int* topo, const int* csr_bg, const int* csr_cnt,
                       const int* csr_buf, const double* mu, const double* lam, const double* dNx, const double* dNx_csr, const int* csr_pos,
                       const double* Ainv,
                       const double* Mmat, const double* dof_rest, const double* rhs_rest, const double* rhs_gravity, const double* dof_f,
                       double* dof, double* dof_vel, double* work, int prepared, int mcadams_sweeps, void* stream);
/* dNx_csr (may be NULL): dNx rows gathered in CSR order, dNx_csr[e] = dNx[csr_buf[e]] (30 doubles each), built once at
 * initialisation; with it collect_rhs streams contiguous memory (one workgroup per kernel) instead of chasing csr_buf.
 * csr_pos (may be NULL; needs dNx_csr): inverse of csr_buf, csr_pos[csr_buf[e]] = e; calc_elastic then also writes P once per
 * neighbour slot in CSR order and the gather has no index left to follow. */
uint64_t pn_sim_work_doubles(int n_k, int n_IP);
/* Simulator.stepforward in its CELL form (csrc/pn_sim_cells.h: k_cells_elastic_gather): calc_elastic (cuda_utils.py:83-121) and collect_rhs_IP (:124-151)
 * of a local/global iteration as ONE launch, the dense product (solver.py:600-601) as the other — 1 + 2 iters launches per substep instead of 1 + 3 iters.
 * All integration points of one kernel-grid cell share their 8 neighbour kernels (solver.py:186-205); the caller sorts the points by cell and cuts the
 * cells into chunks of <= pn_sim_cells_chunk_ips() points:
 *   chunk_tab [n_chunks][12] int32: {points in the chunk, kernel of neighbour slot 0..7, 0, 0, 0};
 *   dNx_cell  [n_chunks][waves = chunk_ips / 8][15][64][2] fp64: lane l of wave w holds point w * 8 + l / 8, slot l % 8 of the chunk; its 30 gradients
 *             dNx[point, slot, c, x] (flat c * 10 + x) as 15 pairs; zeros for lanes behind the chunk's last point;
 *   mu_cell, lam_cell [n_chunks * chunk_ips] fp64 in chunk order;
 *   kp_bg [n_k + 1], kp_pos [8 n_chunks]: the (chunk * 8 + slot) pairs that refer to a kernel, in ascending order, are that kernel's run of partial sums
 *             [kp_bg[k], kp_bg[k + 1]); kp_pos[chunk * 8 + slot] = the pair's place in it (absolute) — where the chunk stores that partial sum.
 * Same results as pn_sim_stepforward up to the summation order of collect_rhs (1e-16 relative) AND the SVD's stopping rule: this form's warm-started
 * threshold Jacobi stops at off-diagonals <= 1e-11 of the diagonal (squares: 1e-22; pairs below 3e-12 are not rotated) where pn_sim_stepforward's stops at
 * 1e-12 — measured <= 8e-10 relative on the displacements between the forms (tests/test_gpu_persistent.py asserts 1e-8).  The warm start (each point's V of
 * the previous local/global iteration, kept in `work`) makes a substep's bits depend on the step HISTORY: bit-reproducible run to run for identical
 * histories; whoever restores dof / dof_vel to replay a trajectory bit for bit re-runs pn_sim_cells_prepare (Simulator.reset_warm_start) as well.
 * work >= pn_sim_cells_work_doubles doubles, initialised once by pn_sim_cells_prepare (identity rotations for the warm-started SVD, arrival counters). */
int pn_sim_cells_chunk_ips(void);
uint64_t pn_sim_cells_work_doubles(int n_k, int n_chunks);
int pn_sim_cells_prepare(int n_k, int n_chunks, double* work, void* stream);
int pn_sim_stepforward_cells(int n_k, int n_chunks, int iters, double dt, double dx, const int* chunk_tab, const double* dNx_cell, const double* mu_cell,
                             const double* lam_cell, const int* kp_bg, const int* kp_pos, const double* Ainv, const double* Mmat, const double* dof_rest,
                             const double* rhs_rest, const double* rhs_gravity, const double* dof_f, double* dof, double* dof_vel, double* work,
                             int mcadams_sweeps, void* stream);
/* The global step without a dense matrix (csrc/pn_sim_pcg.h).  The system block of simulator/solver.py:505-511,600 is kept in block-sparse rows over the
 * kernels: rowptr [n_k + 1], col [nnzb] int32 ascending inside a row, blocks [nnzb][10][10] fp64 row-major (simulator/gmls.py: bsr_pattern,
 * assemble_IP_bsr).  Y [10 n_k,3] = A X, the product simulator/solver.py:505-511,600 takes with the dense matrix; X != Y.  `blocks` and every vector the
 * three entries below gather from (X here; X, A and work of pn_sim_pcg_solve; A, M, dof, dof_vel, dof_rest and pcg_work of pn_sim_stepforward_cells_pcg) are
 * read 16 bytes at a time and must be 16-byte aligned: PN_ERR_ARG otherwise. */
int pn_sim_bsr_matvec3(int n_k, const int* rowptr, const int* col, const double* blocks, const double* X, double* Y, void* stream);
/* Solves A X = B (simulator/solver.py:505-511,600: `global_matrix @ rhs` without the inverse) for the three columns of B [10 n_k,3] together by conjugate
 * gradients preconditioned with Dinv [n_k][10][10], the inverted diagonal blocks (zeros for inactive kernels).  active [n_k] int32: rows and columns of
 * kernels with active == 0 are left out, their rows of X end as 0.  X holds the initial guess on entry and the solution on exit.  Per column: r = b - A x0;
 * |b| = 0 gives x = 0 in 0 iterations; a column stops when |r|_2 <= tol |b|_2 on the recurrence residual (tested before the first iteration too: a
 * converged x0 comes back bit for bit), and is then frozen — its x, r, p are not written again, so its bits do not depend on the other columns; p.Ap <= 0
 * or not finite freezes it as unconverged; after max_iters (>= 1) the current x stands and it counts as unconverged.  Plain launches only, 2 max_iters + 2
 * of them, which return at once when every column is frozen; every dot product is a sum of per-workgroup partials added in a fixed order (no
 * floating-point atomics): the same history gives the same bits.  work >= pn_sim_pcg_work_doubles(n_k) doubles, no initialisation needed: no value that a launch
 * of this solve has not written enters its arithmetic (an inactive kernel's and a frozen column's entries of p are never read into it), so the result does
 * not depend on what `work` held (tests/test_gpu_pcg.py fills it with NaN).
 * stats (int32, device, zeroed by the caller once): [0] solves and [1] unconverged columns, running totals; [2 + 6 s + c] iterations and [5 + 6 s + c]
 * flag (1 converged, 0 stopped by max_iters, 2 p.Ap breakdown) of column c in slot s — pn_sim_pcg_solve writes slot 0 (8 ints). */
uint64_t pn_sim_pcg_work_doubles(int n_k);
int pn_sim_pcg_solve(int n_k, const int* rowptr, const int* col, const double* A, const double* Dinv, const int* active, const double* B, double* X,
                     double tol, int max_iters, double* work, int* stats, void* stream);
/* pn_sim_stepforward_cells with the dense product of simulator/solver.py:505-511,600 replaced by that solve: A and M (the mass block, same pattern) instead
 * of Ainv and Mmat.  Momentum goes through the BSR product with M; every local/global iteration is k_cells_elastic_gather, a solve warm-started from
 * dof - dof_rest, dof = dof_rest + x, the last one also dof_vel.  `work` as pn_sim_stepforward_cells has it, pcg_work >= pn_sim_pcg_work_doubles(n_k);
 * stats >= 2 + 6 iters ints: slot s = local/global iteration s of this (the last) substep. */
int pn_sim_stepforward_cells_pcg(int n_k, int n_chunks, int iters, double dt, double dx, const int* chunk_tab, const double* dNx_cell, const double* mu_cell,
                                 const double* lam_cell, const int* kp_bg, const int* kp_pos, const int* rowptr, const int* col, const double* A,
                                 const double* M, const double* Dinv, const int* active, double tol, int max_iters, const double* dof_rest,
                                 const double* rhs_rest, const double* rhs_gravity, const double* dof_f, double* dof, double* dof_vel, double* work,
                                 double* pcg_work, int* stats, int mcadams_sweeps, void* stream);
/* The local/global iterations of a substep as ONE persistent kernel of n_wg workgroups (one per CU; csrc/pn_sim_coop.h: k_substep_coop) instead of four
 * launches per iteration: same arguments and results as pn_sim_stepforward (tolerance of the summation orders, ~1e-13 relative), `work` prepared by
 * pn_sim_prepare, `coop` >= pn_sim_coop_bytes(n_k, n_IP, n_wg) bytes prepared by pn_sim_coop_prepare, which also returns plan[3] = {pieces, entries
 * per slot, pieces per kernel at most} to pass on.  pn_sim_coop_bytes returns 0 and pn_sim_coop_prepare PN_ERR_ARG when the scene does not fit the persistent form (n_k > 204,
 * more integration points than 32 n_wg, kernel lists too long): callers keep pn_sim_stepforward then.  Every workgroup must become resident; one that
 * waits longer than ~2 s raises a flag and the launch ends with invalid results: pn_sim_coop_status (synchronous) reads the flag. */
uint64_t pn_sim_coop_bytes(int n_k, int n_IP, int n_wg);
int pn_sim_coop_prepare(int n_k, int n_IP, int n_wg, const int* csr_bg, const int* csr_cnt, void* coop, int* plan_out, void* stream);
int pn_sim_coop_status(const void* coop, int* timed_out);
int pn_sim_stepforward_coop(int n_k, int n_IP, int iters, double dt, double dx, const int* topo, const double* mu, const double* lam, const double* dNx,
                            const double* dNx_csr, const int* csr_pos, const double* Ainv, const double* Mmat, const double* dof_rest,
                            const double* rhs_rest, const double* rhs_gravity, const double* dof_f, double* dof, double* dof_vel, double* work,
                            void* coop, int n_wg, const int* plan, void* stream);
/* State-independent contents of `work` (once per simulator / per allocation of `work`), see pn_sim_stepforward. */
int pn_sim_prepare(int n_k, int n_IP, const int* csr_bg, const int* csr_cnt, double* work, void* stream);

/* Simulator.update_force (simulator/solver.py:578-588): dof_f [10 n_k,3] is overwritten, in ONE launch, with the pick force f3 of IP `vid`
 * (every other entry zero).  vid < 0: clear_force (:590-593), f3_host / topo / rho / Nx may then be NULL.  Enqueue it on the stream the
 * substeps run on: stream order then decides which substep sees the change. */
int pn_sim_update_force(int n_k, int vid, const double* f3_host, double dx, const int* topo, const double* rho, const double* Nx, double* dof_f,
                        void* stream);

/* The GUI's mouse drag on the device (nerf/gui.py:556-586, :833-841, :647-657; csrc/pn_drag.hip).  The state lives in device memory, so a substep
 * captured into a HIP graph follows the cursor without a recapture.  Layout (the host reads `vid` back after a pick): */
typedef struct pn_drag_state {
    int vid;           /* picked integration point */
    int active;        /* 0: no force (dof_f = 0, clear_force) */
    double target[3];  /* cursor point in world space */
    double scale;      /* the GUI's force_scale */
} pn_drag_state;
uint64_t pn_sim_drag_bytes(void);        /* sizeof(pn_drag_state) */
uint64_t pn_sim_drag_work_doubles(void); /* doubles of pn_sim_drag_unproject's `work` */
/* dof_f [10 n_k,3] = update_force(vid, f) with f = scale 1e5 (target - pos[vid]), pos[vid] = get_IP_info()'s fp32 position of the CURRENT dof, |f|
 * clamped to 5e5; all zero when !active.  One launch, enqueued in front of a substep on its stream. */
int pn_sim_drag_force(int n_k, int n_IP, const void* drag, const double* dof, double dx, const int* topo, const double* rho, const double* Nx,
                      double* dof_f, void* stream);
/* Writes the fields given: vid >= 0 (< n_IP), active >= 0 (0 or 1), scale > 0, target3_host != NULL; the others keep their value. */
int pn_sim_drag_set(void* drag, int n_IP, int vid, int active, double scale, const double* target3_host, void* stream);
/* screen_to_world: target = pose16 (c2w, row-major) @ [(x-cx)/fx d, (y-cy)/fy d, d, 1] with d = depth0[int(x) * 2 int(cy) + int(y)] (the reference's
 * depth.reshape(2cx, 2cy)[x, y]; W H must equal 2 int(cx) * 2 int(cy)), d == 0 -> the mean of the nonzero depths (fixed-order sum).  intr4 =
 * (fx, fy, cx, cy).  n_IP > 0 (a click): also vid = argmin |ip_pos [n_IP,3] fp32 - target|^2 (lowest index on ties), active = 1.  Two launches;
 * `work`: pn_sim_drag_work_doubles() doubles.  A pixel outside [0, 2cx) x [0, 2cy) is PN_ERR_ARG. */
int pn_sim_drag_unproject(const float* depth0, int W, int H, double x, double y, const double* intr4, const double* pose16, const float* ip_pos,
                          int n_IP, void* drag, double* work, void* stream);

/* Kinematic pins (csrc/pn_pins.hip; Simulator.enable_pin_motion): the pinned points follow a scripted motion.  The system matrix holds
 * stiff N N^T for every pinned point (build_pin_global), so a prescribed displacement u_p of pin p changes the right-hand side alone, by
 * stiff sum_p N_p^T u_p; a launch in front of every substep writes rhs_ext = rhs_gravity + that term, and the substep takes rhs_ext in its
 * rhs_gravity slot.  The motion is evaluated on the device from this state and its own substep clock, so a substep captured into a HIP graph, or
 * run frames ahead of the render, gets the displacement of ITS time:  substep k uses t = (k + 1) dt, and for a pin with rest position X
 *     u(t) = offset + T(t) + R(t)(X - c) - (X - c),   T(t) = A sin(2 pi f_T t + phi_T),
 *     R(t) = the Rodrigues rotation about the unit axis n by the angle theta sin(2 pi f_R t + phi_R)  (theta in radians). */
typedef struct pn_pin_motion {
    int64_t k;         /* substeps since the last pn_sim_pins_clock */
    int active;        /* 0: rhs_ext = rhs_gravity, bit for bit */
    int reserved;
    double A[3], f_T, phi_T;
    double n[3], theta, f_R, phi_R, c[3];
} pn_pin_motion;
uint64_t pn_sim_pins_bytes(void);        /* sizeof(pn_pin_motion) = 128 */
/* Writes `active` (>= 0; -1 keeps it) and the parameters given: translate5_host = (A[3], f_T, phi_T), rotate9_host = (n[3], theta, f_R, phi_R, c[3]);
 * NULL keeps that part.  Everything finite, |n| = 1 to 1e-9 when theta != 0.  A one-thread launch on `stream`; the clock is left alone. */
int pn_sim_pins_set(void* state, int n_pin, int active, const double* translate5_host, const double* rotate9_host, void* stream);
/* k = the clock's new value (>= 0), by a one-thread launch on `stream`. */
int pn_sim_pins_clock(void* state, int64_t k, void* stream);
/* rhs_ext [10 n_k,3] = rhs_gravity + stiff sum_p N_p^T u_p((k + 1) dt), then k += 1 (a one-thread launch BEHIND the first: no workgroup reads a
 * clock that its own launch advances).  Per-kernel CSR over the pins' (pin, neighbour slot) pairs, stably sorted by kernel: pin_bg [n_k + 1] run
 * starts, pin_of [8 n_pin] the entry's pin, pin_N [8 n_pin,10] its pts_Nx row, in CSR order; pin_X [n_pin,3] rest positions; offsets [n_pin,3] or
 * NULL.  One workgroup (one wave) per kernel: its lanes stride the run in ascending order and a fixed shuffle tree adds them, so the order of
 * the sum is a function of the run alone, not of the grid, the launch or the device; no atomics.  Rows of a kernel without an entry, and every row when !active, are copies of rhs_gravity. */
int pn_sim_pins_rhs(int n_k, int n_pin, void* state, double dt, double stiff, const double* rhs_gravity, const int* pin_bg, const int* pin_of,
                    const double* pin_N, const double* pin_X, const double* offsets, double* rhs_ext, void* stream);

/* Contact with planes and spheres (csrc/pn_contact.hip; Simulator.enable_contact): an explicit penalty on the right-hand side.  A
 * launch in front of every substep writes rhs_out = rhs_in + the contact term of the state that substep starts from, and the substep takes rhs_out in
 * its rhs_gravity slot; the matrix, Ainv and the substep's kernels stay as they are.  All fp64.  For integration point i with m_i = rho[i] dx^3,
 *     x_i = sum_{slot<8} sum_{c<10} Nx[i,slot,c] dof[topo[i,slot] 10 + c, :],  v_i the same over dof_vel   (pn_ip_row_acc's order, not rounded to fp32)
 * the colliders 0 .. n-1 are visited in index order, each giving a signed distance d and a unit normal nh out of the solid:
 *     plane (p, nh): d = nh.(x - p);  sphere (p, R): d = |x - p| - R, nh = (x - p)/|x - p|;  container (p, R): d = R - |x - p|, nh = -(x - p)/|x - p|
 *     (|x - p| = 0: nh = (0, 1, 0) before the container's sign), and with w = v_i - v (the collider's velocity), w_n = w.nh, w_t = w - w_n nh:
 *     delta = max(h - d, 0)                       delta = 0: this collider adds exactly nothing
 *     a_n = (kappa delta + beta min(max(-w_n, 0) dt, delta)) / dt^2,   a_t = min(mu a_n, |w_t| / dt)
 *     a_i += a_n nh - a_t w_t / |w_t|             (second term only when |w_t| > 0)
 *     rhs_out[k 30 + j 3 + r] = rhs_in[...] + sum_e m_i Nx[i,slot,j] a_i[r]  over the (i, slot) entries e of kernel k's run, ascending.
 * The system matrix is at least M / dt^2, so a point's response to its own term is at most dt^2 a_n <= (kappa + beta) delta.  Layout of the state: */
#define PN_CONTACT_SLOTS 8
enum { PN_CONTACT_EMPTY = 0, PN_CONTACT_PLANE = 1, PN_CONTACT_SPHERE = 2, PN_CONTACT_CONTAINER = 3, PN_CONTACT_BOX = 4, PN_CONTACT_CAPSULE = 5 };
/* The two solid primitives in the same slot, distance and normal as the law above takes them:
 *     box (axis-aligned; p the centre, n the three half-extents, each > 0, R exactly 0 — reserved):  r = x - p, q_i = |r_i| - n_i, sgn(r_i) = +1 for
 *         r_i >= 0, else -1.  max_i q_i > 0 (outside): e_i = max(q_i, 0), d = sqrt(e.e), nh_i = sgn(r_i) e_i / d — the Euclidean distance, with face,
 *         edge and corner regions.  Otherwise (inside or on the surface): k the axis of the largest q_i (lowest index on ties), d = q_k <= 0,
 *         nh = sgn(r_k) times unit axis k.
 *     capsule (p the end point A, n = B - A with n.n > 0, not normalised, R > 0):  s = clamp(((x - p).n) / (n.n), 0, 1), c = p + s n, then the sphere's
 *         rule with centre c and radius R (its fallback normal (0, 1, 0) when x == c). */
typedef struct pn_contact_collider {
    int type;          /* PN_CONTACT_*; 0: the slot is empty */
    int reserved;
    double p[3];       /* a point of the plane / the sphere's centre / the box's centre / the capsule's end point A */
    double n[3];       /* the plane's unit normal, out of the solid / the box's half-extents / the capsule's B - A */
    double R;          /* the sphere's or capsule's radius; a box: 0 */
    double v[3];       /* the collider's velocity */
} pn_contact_collider;
typedef struct pn_contact_state {
    int active;        /* 0: rhs_out = rhs_in, bit for bit */
    int n;             /* 1 + the highest slot in use (<= 8); 0: rhs_out = rhs_in, bit for bit */
    double kappa;      /* stiffness, in (0, 1] */
    double beta;       /* damping, in [0, 1] */
    double mu;         /* friction, >= 0 */
    double h;          /* thickness, >= 0: contact begins at d < h */
    pn_contact_collider c[PN_CONTACT_SLOTS];
} pn_contact_state;
uint64_t pn_sim_contact_bytes(void);     /* sizeof(pn_contact_state) = 744 */
/* Writes `active` (>= 0; -1 keeps it) and, with params4_host = (kappa, beta, mu, h) != NULL, the parameters: finite, kappa in (0, 1], beta in [0, 1],
 * mu >= 0, h >= 0, else PN_ERR_ARG.  A one-thread launch on `stream`. */
int pn_sim_contact_set_params(void* state, int active, const double* params4_host, void* stream);
/* Writes slot `index` (0 .. 7) and recomputes n.  geom10_host = (p[3], n[3], R, v[3]), finite; a plane's normal is a unit vector to 1e-9, a sphere's
 * or container's R > 0, a box's half-extents > 0 and its R exactly 0, a capsule's n.n > 0 and R > 0, else PN_ERR_ARG; type PN_CONTACT_EMPTY clears the slot (geom10_host may be NULL).  A one-thread launch on `stream`. */
int pn_sim_contact_set_collider(void* state, int index, int type, const double* geom10_host, void* stream);
/* rhs_out [10 n_k,3] = rhs_in + the contact term; rhs_in is left untouched and rhs_out is another buffer.  topo [n_IP,8], rho [n_IP], Nx [n_IP,8,10];
 * kernel_bg / kernel_cnt [n_k] and buffer [8 n_IP] (entry = point 8 + slot) the per-kernel CSR of pn_sim_stepforward, Nx_csr [8 n_IP,10] the Nx rows in
 * that order.  With accel_out [n_IP,3]: TWO launches, the measured faster form — a thread per point writes accel_out = a_i (zeros for a
 * point not in contact), then the per-kernel sum of pn_sim_accel_rhs (below) adds m_i Nx a_i.  accel_out NULL: ONE launch, the same workgroups with every entry evaluating
 * its point itself (8 x redundant across a point's kernels; every workgroup runs the same code on the same inputs, so all agree on a point to the
 * bit) — the same bits in rhs_out.  No atomics: the order of every sum is a function of the kernel's run alone.  A kernel none of whose points
 * is in contact, and every kernel when !active or n == 0, copies rhs_in bit for bit.  No allocation, no host synchronisation, capturable. */
int pn_sim_contact_rhs(int n_k, int n_IP, const void* state, double dt, double dx, const double* dof, const double* dof_vel, const int* topo,
                       const double* rho, const double* Nx, const int* kernel_bg, const int* kernel_cnt, const int* buffer, const double* Nx_csr,
                       const double* rhs_in, double* rhs_out, double* accel_out, void* stream);
/* The per-kernel sum that contact, the force fields and self-contact share (csrc/pn_sim_rhs.h: pn_kernel_accel_term), on its own: ONE launch,
 *     rhs_out[k 30 + j 3 + r] = rhs_in[...] + sum_e rho[i] dx^3 Nx_csr[e,j] accel[i,r]   over the entries e of kernel k's run, i = buffer[e] >> 3,
 * a workgroup of four waves per kernel, thread t taking the run's entries t, t + 256, ... in ascending order (an entry whose point has accel = 0 is
 * skipped), shuffle tree 32 ... 1 per wave, then the waves in the order ((w0 + w1) + w2) + w3 through LDS, no atomics.  A kernel none of whose points
 * has accel != 0 copies rhs_in bit for bit (-0.0 included).  This is the last launch of pn_sim_contact_rhs, pn_sim_fields_rhs and pn_sim_self_rhs with
 * their stage switched on: called on a stage's accel_out and rhs_in it returns that stage's rhs_out to the bit.  PN_ERR_ARG, before anything is
 * enqueued, for a NULL pointer, rhs_in == rhs_out, dx not finite and > 0, n_IP outside 1 .. 2^27.  No allocation, no host synchronisation, capturable. */
int pn_sim_accel_rhs(int n_k, int n_IP, double dx, const double* rho, const int* kernel_bg, const int* kernel_cnt, const int* buffer,
                     const double* Nx_csr, const double* accel, const double* rhs_in, double* rhs_out, void* stream);

/* Mesh colliders: signed-distance grids (csrc/pn_sdf.hip; pienerf_amd/sdf.py: SdfGrid; Simulator.add_mesh_collider).
 *
 * A grid holds fp32 values phi [nz, ny, nx] in device memory; node (i, j, k), i along x, is at lo + s (i, j, k) with cubic voxels of spacing s > 0;
 * 2 .. 512 nodes per axis, at most 2^27 nodes; lo and s are fp64.
 *
 * pn_sdf_build fills a grid from a triangle mesh in ONE launch.  tri9 [T, 9] fp32: the three corners of every triangle, gathered by the host, which
 * has dropped the triangles with a repeated index or zero area.  For node q = fp32(lo + s (i, j, k)) (the sum in fp64, rounded once per axis), over
 * the triangles 0 .. T-1 in ascending order, with a, b, c the corners minus q, all terms fp32:
 *     distance: the squared length of the point of the triangle closest to the origin, by the face / edge / vertex regions (in the order vertex a,
 *         vertex b, edge ab, vertex c, edge ac, edge bc, face; barycentric products d1 .. d6 as in Ericson, Real-Time Collision Detection 5.1.5);
 *         the minimum is kept squared and its square root is taken once at the end;
 *     sign: the generalised winding number w = (1 / 4 pi) sum_t 2 atan2(a.(b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|): the terms fp32,
 *         the sum fp64.  The node is inside iff |w| >= 0.5, and its value is then -dist: either orientation of a closed mesh works.
 * winding_out (NULL, or [nz, ny, nx] fp64) receives w.  The host wrapper (SdfGrid.from_mesh) derives from it closedness = max | |w| - round(|w|) |
 * over the nodes off the surface (value beyond 1e-5 s; a node on a face sees w = 1/2) and warns above 0.1: an open mesh has no inside.  One thread per node, 256-thread workgroups over bricks of 8 x 8 x 4 nodes, the triangles
 * staged through LDS in tiles of 128 that every lane reads at the same address; no atomics, so two builds are the same bits.  The cost is
 * nodes x triangles; there is no acceleration structure, so the one launch is capped at PN_SDF_MAX_PAIRS = 2^38 node-triangle pairs.  PN_ERR_ARG,
 * before anything is enqueued, for a NULL pointer, T outside 1 .. 2^24, a node count out of range, more pairs than the cap, lo or s not finite, s <= 0.  No allocation, no host synchronisation. */
#define PN_SDF_MAX_PAIRS (1ull << 38)
int pn_sdf_build(const float* tri9, int n_tris, int nx, int ny, int nz, const double* lo3_host, double spacing, float* grid, double* winding_out,
                 void* stream);
/* Contact against up to 4 placed grids: a second, optional state of the contact stage.  At integration point i (x_i, v_i as above, fp64), for the
 * slots 0 .. 3 in index order, a slot with grid != NULL:
 *     u = (x - lo) / s per axis; a point with u outside [0, n - 1) on any axis, or not finite, gets nothing from the slot;  i0 = floor(u), f = u - i0;
 *     d = the trilinear interpolant of the eight values about the point (each widened to fp64), lerp(a, b, f) = a + f (b - a) along x, then y, then z;
 *     g = the gradient of that interpolant in u (g_x = the y-then-z lerp of the four differences along x; g_y = the z lerp of the difference of the
 *         two y neighbours after the x lerp; g_z = the difference of the two z neighbours after the x and y lerps), nh = g / |g|, (0, 1, 0) for g = 0;
 *     then contact's own response with its kappa, beta, mu, h and the slot's velocity v: delta = max(h - d, 0), a_n, a_t and a_i += ... as above.
 * The slot's lo is the grid's lo plus the collider's offset: a placed grid is translated, never rotated or scaled. */
#define PN_SDF_SLOTS 4
typedef struct pn_sdf_slot {   /* 80 bytes */
    const float* grid;   /* device memory, [nz, ny, nx]; NULL: the slot is empty */
    int nx, ny, nz;      /* nodes per axis, 2 .. 512 */
    int reserved;
    double lo[3];        /* position of node (0, 0, 0) */
    double s;            /* spacing, > 0 */
    double v[3];         /* the collider's velocity */
} pn_sdf_slot;
typedef struct pn_sdf_state {  /* 328 bytes = 41 doubles */
    int n;               /* 1 + the highest slot in use (<= 4); 0: nothing is added */
    int reserved;
    pn_sdf_slot c[PN_SDF_SLOTS];
} pn_sdf_state;
uint64_t pn_sim_sdf_bytes(void);         /* sizeof(pn_sdf_state) = 328 */
/* Writes slot `index` (0 .. 3) and recomputes n.  grid NULL clears the slot (the other arguments are then ignored); else nx, ny, nz in 2 .. 512 with
 * at most 2^27 nodes and geom7_host = (lo[3], s, v[3]) finite with s > 0, else PN_ERR_ARG.  A one-thread launch on `stream`. */
int pn_sim_sdf_set_collider(void* state, int index, const float* grid, int nx, int ny, int nz, const double* geom7_host, void* stream);
/* pn_sim_contact_rhs's two-launch form with the grids between its launches, THREE launches: the analytic law at every point into accel_out
 * (k_contact_points, as pn_sim_contact_rhs enqueues it); a thread per point adds the grids' terms to accel_out[i] (a point no grid touches keeps
 * its bits; nothing is added while the contact state is inactive); the per-kernel sum of pn_sim_accel_rhs.  With an empty sdf_state rhs_out and
 * accel_out are pn_sim_contact_rhs's to the bit.  accel_out is required.  No atomics, no allocation, no host synchronisation, capturable. */
int pn_sim_contact_sdf_rhs(int n_k, int n_IP, const void* state, const void* sdf_state, double dt, double dx, const double* dof, const double* dof_vel,
                           const int* topo, const double* rho, const double* Nx, const int* kernel_bg, const int* kernel_cnt, const int* buffer,
                           const double* Nx_csr, const double* rhs_in, double* rhs_out, double* accel_out, void* stream);

/* Rigid balls (csrc/pn_bodies.hip; Simulator.enable_bodies / add_body): up to 8 dynamic spheres the object pushes back.  A dynamic
 * body b is bound to slot b of a pn_contact_state that holds a solid sphere (PN_CONTACT_SPHERE, radius R); it has a mass M > 0 and a linear damping
 * c >= 0 (1/s).  Its centre p and velocity u ARE the slot's p and v: there is no second copy, so contact, the drawn frame and the shadows follow a
 * moving ball without a change.  Two launches in front of every substep, behind contact's, evaluate everything from the state the substep starts from:
 *   1. object side: unchanged.  pn_sim_contact_rhs has evaluated its law against slot b with col->v = u.
 *   2. reaction: F_b = - sum_i m_i a_{i,b} over the integration points, m_i = rho[i] dx^3, a_{i,b} = a_n nh - a_t w_t / |w_t| slot b's own part of
 *      the contact law at point i (x_i, v_i as above; the contact state's kappa, beta, mu, h), and delta_max,b = the largest delta among the points
 *      slot b penetrates (0: none).  The sum's order is fixed: workgroups of 256 points in point order, in each a wave's shuffle tree 32, 16 ... 1 and
 *      then the waves as ((w0 + w1) + w2) + w3, the workgroups' partials added in ascending workgroup order.  No atomics; the bits do not depend on
 *      the device.
 *   3. clamp: s = min(1, M delta_max / (dt^2 |F_b|)) (s = 1 when F_b = 0), so the body's own response dt^2 s |F_b| / M to its reaction is at most
 *      its deepest penetration: the counterpart of dt^2 a_n <= (kappa + beta) delta for a point.  A (substep, body) pair with s < 1 is counted.
 *   4. static colliders: every other slot that is not a dynamic body (planes, solid spheres, the container, boxes, capsules) acts on the ball through the same law,
 *      applied at the point p with velocity u and the ball's radius in the thickness's place (kappa, beta, mu of the contact state; velocity relative
 *      to that collider's v): plane d = n.(p - p_c) - R, solid sphere d = |p - p_c| - R_c - R, container d = R_c - |p - p_c| - R, box and capsule d = (their distance at p) - R, delta = max(-d, 0),
 *      slots in index order, giving a_static.  Static colliders get no reaction; two dynamic balls pass through each other.
 *   5. integration, semi-implicit like the object's: u+ = (u + dt (g + s F_b / M + a_static)) / (1 + dt c), p+ = p + dt u+, both written into the
 *      slot; the substep clock k advances.
 * No rotation: the spheres have no spin and friction gives no torque.  With active = 0, or with the contact state inactive, no body moves (the clock
 * still counts).  Layout of the state: */
#define PN_BODIES_SLOTS 8          /* = PN_CONTACT_SLOTS: body b lives in collider slot b */
typedef struct pn_body {
    int dynamic;       /* 1: slot b of the contact state is a dynamic body (it acts only while that slot holds a PN_CONTACT_SPHERE) */
    int reserved;
    double M;          /* mass, > 0 */
    double c;          /* linear damping, 1/s, >= 0 */
    double F[3];       /* the last substep's raw reaction F_b */
    double s;          /* ... its clamp scale, in (0, 1] */
    double delta_max;  /* ... its deepest penetration */
    int64_t clamped;   /* substeps with s < 1 since the body was made dynamic */
} pn_body;
typedef struct pn_bodies_state {
    int64_t k;         /* substeps the stage has run */
    int active;        /* 0: no body moves */
    int reserved;
    double g[3];       /* gravity on the bodies */
    pn_body b[PN_BODIES_SLOTS];
} pn_bodies_state;
uint64_t pn_sim_bodies_bytes(void);      /* sizeof(pn_bodies_state) = 616 */
/* Bytes of pn_sim_bodies_step's `work` for n_IP points: 32 doubles (F[3], delta_max for 8 slots) per workgroup of 256 points, and 8 bytes behind
 * them for the one-launch form's arrival counter; 0 for n_IP outside 1 .. 2^27. */
uint64_t pn_sim_bodies_work_bytes(int n_IP);
/* Writes `active` (>= 0; -1 keeps it) and, with gravity3_host != NULL, g (finite, else PN_ERR_ARG).  A one-thread launch on `stream`. */
int pn_sim_bodies_set_params(void* state, int active, const double* gravity3_host, void* stream);
/* Slot `slot` (0 .. 7): dynamic 1 makes it a body of `mass` (finite, > 0) and `damping` (finite, >= 0), else PN_ERR_ARG; a slot that was not
 * dynamic before starts with F = 0, s = 1, delta_max = 0, clamped = 0, one that was keeps them.  dynamic 0 clears the record (mass and damping are
 * ignored).  A one-thread launch on `stream`. */
int pn_sim_bodies_set_body(void* state, int slot, int dynamic, double mass, double damping, void* stream);
/* Overwrites the centre (mask & 1) and / or the velocity (mask & 2) of slot `slot` in `contact_state` (a pn_contact_state) with pv6_host = (p[3],
 * v[3]), finite; mask in 1 .. 3, else PN_ERR_ARG.  What is not in the mask keeps the device's value.  A one-thread launch on `stream`. */
int pn_sim_bodies_set_motion(void* contact_state, int slot, int mask, const double* pv6_host, void* stream);
/* The next substep is substep k >= 0 of the stage's clock.  A one-thread launch on `stream`. */
int pn_sim_bodies_clock(void* state, int64_t k, void* stream);
/* One substep of every dynamic body.  one_launch 0, TWO launches, the measured faster form: k_body_reaction, a thread per
 * integration point in workgroups of 256, writes each workgroup's (F[3], delta_max) per slot into `work` (every word the second launch reads is
 * written by the first, zeros for a workgroup none of whose points touches a body); k_body_step, one workgroup, adds the partials in ascending order
 * and does steps 3 - 5 for the slots 0 .. 7.  one_launch 1: ONE launch, in which the workgroup that arrives last at a counter does k_body_step's work
 * behind an agent-scope release / acquire pair — the same sums in the same order, the same bits.  `work`: pn_sim_bodies_work_bytes(n_IP) bytes,
 * 8-byte aligned; the partials may hold anything on entry, the counter in its last 8 bytes is zero before the first call and left zero by every call.
 * `state` a pn_bodies_state and `contact_state` the pn_contact_state, both device memory; dof, dof_vel, topo, rho, Nx as pn_sim_contact_rhs's.
 * PN_ERR_ARG, before anything is enqueued, for a NULL pointer, dt or dx not finite and > 0, n_IP outside 1 .. 2^27, one_launch not 0 or 1.  No
 * allocation, no host synchronisation, capturable. */
int pn_sim_bodies_step(int n_k, int n_IP, void* state, void* contact_state, void* work, double dt, double dx, const double* dof, const double* dof_vel,
                       const int* topo, const double* rho, const double* Nx, int one_launch, void* stream);

/* Force fields (csrc/pn_fields.hip; Simulator.enable_fields): wind, vortex and blast on the whole body, with air drag.  A fourth
 * right-hand-side stage beside drag, pins and contact: launches in front of every substep write rhs_out = rhs_in + the field term of the state and the
 * time that substep starts from, and the substep takes rhs_out in its rhs_gravity slot; the matrix, Ainv and the substep's kernels stay as they are.
 * All fp64.  Substep k of the stage's own clock uses t = k dt.  x_i, v_i and m_i as for contact (above).  The fields 0 .. n-1 are visited in index
 * order, each acting only while t0 <= t < t1 (t1 may be +inf).  With c_eff = min(c, 1/dt), fall(q) = max(1 - q/R, 0)^2 and
 * s_eff = sign(s) min(|s|, R / (2 dt^2)):
 *     wind (origin p, velocity W = n, drag c, gust g, f, phi, wave vector kv):
 *         u = W (1 + g sin(2 pi (f t - kv.(x - p)) + phi)),   a_i += c_eff (u - v)          W = 0: still-air drag, mass-proportional damping
 *     vortex (point p, unit axis n, angular speed omega = s, drag c, R):
 *         r = x - p, rho = |r - (n.r) n|,   a_i += c_eff fall(rho) (omega (n x r) - v)      continuous at rho = R, exactly nothing at and beyond it
 *     radial (centre p, strength s in acceleration units, away for s > 0, R):
 *         L = |x - p|,   a_i += s_eff fall(L) (x - p) / L                                   only when L > 0; exactly nothing at and beyond R
 *     rhs_out[k 30 + j 3 + r] = rhs_in[...] + sum_e m_i Nx[i,slot,j] a_i[r]  over the (i, slot) entries e of kernel k's run, ascending.
 * The system matrix is at least M / dt^2, so a point's own response per step is at most dt c_eff |u - v| <= |u - v| in velocity, and at most R / 2 in
 * position for the radial field: the two clamps are the stability bounds.  Layout of the state: */
#define PN_FIELD_SLOTS 8
enum { PN_FIELD_EMPTY = 0, PN_FIELD_WIND = 1, PN_FIELD_VORTEX = 2, PN_FIELD_RADIAL = 3 };
typedef struct pn_force_field {        /* 144 bytes */
    int type;          /* PN_FIELD_*; 0: the slot is empty */
    int reserved;
    double p[3];       /* wind: origin of the gust's wave; vortex: a point of the axis; radial: the centre */
    double n[3];       /* wind: the velocity W; vortex: the unit axis */
    double c;          /* drag, 1/s, >= 0 (wind, vortex) */
    double s;          /* vortex: omega, rad/s; radial: strength, acceleration units */
    double R;          /* radius, > 0 (vortex, radial) */
    double g, f, phi;  /* wind: gust depth in [0, 1], frequency in Hz, phase */
    double kv[3];      /* wind: the gust's wave vector, cycles per unit length */
    double t0, t1;     /* acts while t0 <= t < t1; t1 may be +inf */
} pn_force_field;
typedef struct pn_field_state {        /* 1168 bytes = 146 doubles */
    int64_t k;         /* substeps since the last pn_sim_fields_clock */
    int active;        /* 0: rhs_out = rhs_in, bit for bit */
    int n;             /* 1 + the highest slot in use (<= 8); 0: rhs_out = rhs_in, bit for bit */
    pn_force_field f[PN_FIELD_SLOTS];
} pn_field_state;
uint64_t pn_sim_fields_bytes(void);      /* sizeof(pn_field_state) = 1168 */
/* active = 0 or 1, else PN_ERR_ARG.  A one-thread launch on `stream`; the clock and the slots are left alone. */
int pn_sim_fields_set_active(void* state, int active, void* stream);
/* Writes slot `index` (0 .. 7) and recomputes n.  geom17_host = (p[3], n[3], c, s, R, g, f, phi, kv[3], t0, t1).  PN_ERR_ARG, before anything is
 * enqueued, for an index outside 0 .. 7, an unknown type, a non-finite value (only t1 may be +inf), c < 0, g outside [0, 1], R <= 0 for a vortex or a
 * radial field, a vortex axis that is not a unit vector to 1e-9, t1 < t0.  Type PN_FIELD_EMPTY clears the slot (geom17_host may be NULL).  A
 * one-thread launch on `stream`. */
int pn_sim_fields_set_field(void* state, int index, int type, const double* geom17_host, void* stream);
/* k = the clock's new value (>= 0), by a one-thread launch on `stream`. */
int pn_sim_fields_clock(void* state, int64_t k, void* stream);
/* rhs_out [10 n_k,3] = rhs_in + the field term at t = k dt, then k += 1; rhs_in is left untouched and rhs_out is another buffer.  The tables are
 * pn_sim_contact_rhs's.  THREE launches: a thread per point writes accel_out [n_IP,3] = a_i (one wave per workgroup); the per-kernel sum of
 * pn_sim_accel_rhs (above) adds m_i Nx a_i, no atomics; and a one-thread launch BEHIND them advances the
 * clock (no workgroup reads a clock that its own launch advances).  A kernel none of whose points has a != 0, and every kernel when !active, n == 0 or
 * t is outside every window, copies rhs_in bit for bit (-0.0 included).  PN_ERR_ARG for a NULL pointer, rhs_in == rhs_out, dt or dx not > 0.  No
 * allocation, no host synchronisation, capturable. */
int pn_sim_fields_rhs(int n_k, int n_IP, void* state, double dt, double dx, const double* dof, const double* dof_vel, const int* topo,
                      const double* rho, const double* Nx, const int* kernel_bg, const int* kernel_cnt, const int* buffer, const double* Nx_csr,
                      const double* rhs_in, double* rhs_out, double* accel_out, void* stream);

/* Self-contact (csrc/pn_selfcontact.hip; Simulator.enable_self_contact): the body collides with itself and with its own pieces.  A
 * fifth right-hand-side stage, last in the chain rhs_gravity -> pins -> contact -> fields -> self: launches in front of every substep write
 * rhs_out = rhs_in + the self-contact term of the state that substep starts from; the matrix, Ainv and the substep's kernels stay as they are.  All
 * fp64.  x_i, v_i and m_i = rho[i] dx^3 as for contact (above); X_i is the point's rest position.  Parameters: kappa in (0, 1], beta in [0, 1],
 * mu >= 0, the contact distance h > 0 (default dx: two cell centres touch a cell apart) and the exclusion radius rho_x >= h (default 3 h).
 *   Eligible pairs: i != j with |X_i - X_j| >= rho_x (the squares summed as (q0 + q1) + q2, every operation rounded once).  Material adjacent at rest
 * never repels itself, however compressed; two disconnected pieces are always eligible.  For an eligible pair
 *     r = x_i - x_j,  L = |r|,  delta_ij = max(h - L, 0),  nh = r / L    (L = 0: nh = (0, 1, 0) for i < j, (0, -1, 0) for i > j: antisymmetric)
 *     delta_ij = 0: the pair adds exactly nothing
 *     S_i = sum_j delta_ij over the partners of i            w_ij = delta_ij / max(S_i, S_j)
 * w_ij is symmetric, continuous when a partner enters at delta = 0, and sum_j w_ij delta_ij <= max_j delta_ij however many partners a crushed
 * region gives a point.  With w = v_i - v_j, w_n = w.nh, w_t = w - w_n nh:
 *     g = w_ij (kappa delta_ij + beta min(max(-w_n, 0) dt, delta_ij)) / dt^2,   g_t = min(mu g, w_ij |w_t| / dt)
 *     a_i += (m_j / (m_i + m_j)) (g nh - g_t w_t / |w_t|)     (second term only when |w_t| > 0)
 *     rhs_out[k 30 + j 3 + r] = rhs_in[...] + sum_e m_i Nx[i,slot,j] a_i[r]  over the (i, slot) entries e of kernel k's run, ascending.
 * m_i a_i[from j] = -m_j a_j[from i]: the stage adds no net momentum.  A pair's relative response is at most (kappa + beta) delta_ij w_ij: contact's
 * stability argument.  There is no continuous collision detection: a piece moving more than h per substep can tunnel (|v| dt < h).
 *   Neighbour search, rebuilt on the device by every call.  A point's cell is floor(x / h) per axis in fp64, clamped to [-2^30, 2^30] as int32; a
 * point whose x or v is not finite takes no part (S = 0, nobody's partner).  Bucket = ((uint32)cx 73856093 ^ (uint32)cy 19349663 ^
 * (uint32)cz 83492791) & (T - 1), T the smallest power of two >= max(1024, 2 n_IP): hashed, so a falling or flying body needs no bounding box and no
 * host read-back.  Table: count, exclusive scan, fill (integer atomics on counters and cursors), then every bucket in ascending point id, which makes
 * the table independent of the atomics' order.  Point i visits the 27 cells c + (ox, oy, oz), oz outermost, each offset running -1, 0, 1; within a
 * bucket ascending j; j is accepted only if j's own cell EQUALS the visited cell, so two cells hashed to one bucket never count a partner twice.
 * Every floating-point sum (S_i, a_i) is taken in that order; none goes through an atomic.  Bounded cost: if any bucket holds more than
 * PN_SELF_BUCKET_CAP points the call adds exactly nothing (rhs_out = rhs_in bit for bit) and `overflowed` grows by one: more than 64 points in one
 * h^3 cell is a body that has already collapsed, and a blown-up run must not turn into an O(n^2) launch.  Layout of the state: */
#define PN_SELF_BUCKET_CAP 64
typedef struct pn_selfcontact_state {  /* 56 bytes = 7 doubles */
    int active;          /* 0: rhs_out = rhs_in, bit for bit */
    int reserved;
    int64_t overflowed;  /* calls switched off because a bucket held more than PN_SELF_BUCKET_CAP points */
    double kappa;        /* stiffness, in (0, 1] */
    double beta;         /* damping, in [0, 1] */
    double mu;           /* friction, >= 0 */
    double h;            /* contact distance, > 0 */
    double rho_x;        /* exclusion radius at rest, >= h */
} pn_selfcontact_state;
uint64_t pn_sim_self_bytes(void);        /* sizeof(pn_selfcontact_state) = 56 */
/* Bytes of the work area for n_IP points: positions and velocities [n_IP,6], S [n_IP], a [n_IP,3] (fp64), cells and buckets [n_IP,4], the buckets'
 * members twice [n_IP] (as placed, and sorted), and the table of T buckets: counts [T], starts [T + 1], two flag words.  0 for n_IP outside 1 .. 2^27. */
uint64_t pn_sim_self_work_bytes(int n_IP);
/* Kernel launches one pn_sim_self_rhs enqueues (8). */
int pn_sim_self_launches(void);
/* Writes `active` (0 or 1; -1 keeps it) and, with params5_host = (kappa, beta, mu, h, rho_x) != NULL, the parameters: finite, kappa in (0, 1], beta in
 * [0, 1], mu >= 0, h > 0, rho_x >= h, else PN_ERR_ARG before anything is enqueued.  `overflowed` is left alone.  A one-thread launch on `stream`. */
int pn_sim_self_set_params(void* state, int active, const double* params5_host, void* stream);
/* rhs_out [10 n_k,3] = rhs_in + the self-contact term; rhs_in is left untouched and rhs_out is another buffer.  X_rest [n_IP,3]; the other tables are
 * pn_sim_contact_rhs's; `work` has pn_sim_self_work_bytes(n_IP) bytes, 8-byte aligned, and may hold anything on entry.  accel_out [n_IP,3] = a_i
 * (NULL: kept in the work area).  EIGHT ordinary launches on `stream`, none waiting for another workgroup: points and cells (the counts zeroed); count;
 * scan and the overflow decision (one workgroup); fill; sort; S_i; a_i (a thread per point, one wave per workgroup); and the per-kernel sum of
 * pn_sim_accel_rhs (above), no atomics.  The same bits from every run on the same
 * inputs.  A kernel none of whose points has a != 0, and every kernel when !active or the call overflowed, copies rhs_in bit for bit (-0.0 included).
 * PN_ERR_ARG, before anything is enqueued, for a NULL pointer (accel_out excepted), rhs_in == rhs_out, dt or dx not > 0.  No allocation, no host
 * synchronisation, capturable. */
int pn_sim_self_rhs(int n_k, int n_IP, void* state, void* work, double dt, double dx, const double* dof, const double* dof_vel, const double* X_rest,
                    const int* topo, const double* rho, const double* Nx, const int* kernel_bg, const int* kernel_cnt, const int* buffer,
                    const double* Nx_csr, const double* rhs_in, double* rhs_out, double* accel_out, void* stream);

/* Simulator diagnostics (csrc/pn_diagnostics.hip; Simulator.diagnostics): what a state (dof, dof_vel) holds, as one row of
 * PN_DIAG_DOUBLES doubles.  A readout, not a stage: it writes `work`, `row_out` and `per_point` only, so a run with it and a run without it are the same
 * bits.  THE LAW, everything fp64.  Per integration point p with its 8 kernels, m = rho[p] dx^3 and j = rho[p] dx^5 / 12:
 *   x, v         position and velocity by pn_ip_state (csrc/pn_sim_rhs.h): what contact, the force fields and self-contact see;
 *   F, G         sum over the kernels of dof (x) dNx and dof_vel (x) dNx, a kernel's share as the substep's ip_F_partial forms it, the shares added over the
 *                point's eight lanes ^1, ^2, ^4;
 *   H            sum of dof (x) ddNx, the 27 components pn_sim_update_F calls dF;
 *   sig          the converged cold-start Jacobi svd3 of F (csrc/pn_sim_svd.h): |sig| descending, sig[2] carries the sign of det F.  Never the
 *                McAdams approximation, whatever decomposition the solver runs: this is a measurement;
 *   sp           volume_invariant_project(sig) (simulator/func_utils.py:21-40);  det = det F, from F directly.
 * The energies are the ones the solver's own matrix stands for (build_IP_global, simulator/cuda_utils.py:48-55: c0 = rho dx^3 / dt^2 on Nx, c1 =
 * dx^3 (rho dx^2 / 12 / dt^2 + mu + lam) on dNx, c2 = dx^5 (mu + lam) / 12 on ddNx):
 *   kinetic      ke = 1/2 m |v|^2 + 1/2 j |G|_F^2
 *   elastic      ee = dx^3 (mu/2 sum (sig_i - 1)^2 + lam/2 sum (sig_i - sp_i)^2) + (dx^5 / 12) (mu + lam)/2 |H|^2      (mu = mu[p], lam = lam[p];
 *                sum (sig_i - 1)^2 = |F - R|^2 and sum (sig_i - sp_i)^2 = |F - V|^2 of calc_elastic, so neither U nor V enters)
 *   gravity      ge = -m g.x
 *   momentum     P = m v;   L = m x cross v + j sum_c F[:,c] cross G[:,c]   (about the origin)
 *   strain       sqrt(sum (sig_i - 1)^2);   speed |v|.
 * A point is NON-FINITE when any of x, v, F, G, H is not finite, or one of its kernel ids is outside [0, n_k) (never with the tables solver.py builds):
 * it is counted and excluded from every sum and every extremum.  The row, PN_DIAG_DOUBLES doubles (Python: diagnostics.DIAG_FIELDS):
 *   [0] mass   [1..3] com = sum m x / mass   [4..6] P   [7..9] L   [10] kinetic   [11] gravity   [12] elastic
 *   [13,14] sig_min (over sig[2])   [15,16] sig_max (over sig[0])   [17,18] det_min   [19,20] strain_max   [21,22] speed_max: (value, point index as a double);
 *   on equal values the lowest index;  [23] nonfinite   [24] inverted (points with det <= 0).
 * With no finite point the sums are 0 and the extrema NaN with index -1.  The pin penalty's energy is NOT part of `elastic`: the pins act on cloud
 * points, not integration points, and kinematic pins move their targets.
 * per_point (may be NULL): [n_IP, 8] = (m, ke, ee, det, sig0, sig1, sig2, strain); NaN behind m for a non-finite point.
 * work >= pn_sim_diagnostics_work_doubles(n_IP) doubles: one partial record per 32 points.  g3_host: the gravity vector, read in the call.
 * TWO launches on `stream` (eight lanes per point and one record per workgroup, then one workgroup that folds the records in ascending order), no
 * atomics, fixed summation trees: the same bits from every run on the same inputs.  PN_ERR_ARG, before anything is enqueued, for a NULL pointer
 * (per_point excepted), n_k or n_IP <= 0, n_IP > 2^27, dx not finite or not > 0.  No allocation, no host synchronisation, capturable. */
#define PN_DIAG_DOUBLES 25
int pn_sim_diagnostics(int n_k, int n_IP, double dx, const double* g3_host, const double* dof, const double* dof_vel, const int* topo, const double* rho,
                       const double* mu, const double* lam, const double* Nx, const double* dNx, const double* ddNx, double* work, double* row_out,
                       double* per_point, void* stream);
/* PN_DIAG_DOUBLES, for the Python side to check its DIAG_FIELDS against (the row of pn_sim_diagnostics; energies of simulator/cuda_utils.py:48-55). */
int pn_sim_diagnostics_doubles(void);
/* Doubles of pn_sim_diagnostics's `work` for n_IP points (the partial records of its first launch; simulator/cuda_utils.py:48-55 has no counterpart:
 * the reference never sums its energies). */
uint64_t pn_sim_diagnostics_work_doubles(int n_IP);

/* The colliders drawn into a rendered frame (csrc/pn_colliders.hip; NeRFRenderer.set_collider_overlay): one launch behind the frame
 * driver, a thread per ray, composites the analytic surfaces of a pn_contact_state into `image` with a depth test against the object.  `contact_state`
 * is DEVICE memory with the pn_contact_state layout (the simulator's own buffer or a 744-byte copy), read at execution time: a captured launch follows
 * set_collider without a recapture.  The slots 0 .. n-1 that hold a valid type are drawn; `active` is ignored (it switches the force, not the picture).
 * The fp64 fields are rounded to fp32 once per workgroup; everything per ray is fp32, one rounding per operation, sums left to right.
 * t is in units of rays_d AS GIVEN (how depth_0 measures it); q = d.d, dh = d / sqrt(q).  Per ray (o, d), over the slots in index order — a later
 * slot wins only with a strictly smaller t:
 *     plane (p, nh):     nd = nh.d;  hit iff nd < 0 (front face only) and t = nh.(p - o) / nd lies in (t_min, t_max);  normal nh
 *     sphere (c, R):     oc = o - c, b = oc.d, disc = b b - q (oc.oc - R R);  hit iff disc > 0;  t = (-b - sqrt(disc)) / q if that is > t_min, else
 *                        (-b + sqrt(disc)) / q;  then t in (t_min, t_max);  normal (x - c) / R, x = o + t d
 *     container (c, R):  the larger root only (the inner wall seen through the front: a camera outside still sees the object);  normal -(x - c) / R
 *     box (c, h):        the three slabs in axis order.  d_i == 0: the ray misses unless |o_i - c_i| < h_i, and the axis bounds nothing.  Else
 *                        t1 = ((c_i - h_i) - o_i) / d_i, t2 = ((c_i + h_i) - o_i) / d_i;  t_enter = the largest min(t1, t2), t_exit = the smallest
 *                        max(t1, t2), each with the axis that gave it (the lowest index on ties);  hit iff t_enter < t_exit;  t = t_enter if that is
 *                        > t_min, else t_exit (the eye inside: the far face);  then t in (t_min, t_max);  normal: the chosen end's axis
 *     capsule (A, n, R): a = n / |n|, len = |n|, B = A + n, once per workgroup (|n| = 0 in fp32: the sphere (A, R)).  The convex union of three
 *                        parts, each an interval (near, far):  the spheres (A, R) and (B, R) with the sphere's roots, disc > 0;  the cylinder, with
 *                        oc = o - A, ad = a.d, ao = a.oc, dp = d - ad a, op = oc - ao a, A2 = dp.dp, b = op.dp, disc = b b - A2 (op.op - R R):  hit iff
 *                        A2 > 0 and disc > 0, (near, far) = ((-b - sqrt(disc)) / A2, (-b + sqrt(disc)) / A2) intersected with the slab between the
 *                        end planes — ad == 0: kept iff 0 < ao < len;  else s1 = (0 - ao) / ad, s2 = (len - ao) / ad, near = max(near, min(s1, s2)),
 *                        far = min(far, max(s1, s2)) — and kept iff near < far.  t_near = the smallest near, t_far = the largest far over the parts
 *                        that are hit;  t = t_near if that is > t_min, else t_far;  then t in (t_min, t_max);  normal (x - c) / R with
 *                        c = A + clamp(a.(x - A), 0, len) a, evaluated as ((x - A) - clamp(..) a) / R
 * Colour of the hit slot k:  shade = ambient + (1 - ambient) |normal.d| / sqrt(q);  for a plane with checker > 0: u = normalised nh x e, e the
 * coordinate axis on which |nh| is smallest (lowest index on ties), v = nh x u, parity = (floor(u.(x - p) / checker) + floor(v.(x - p) / checker)) & 1,
 * factor = checker_dim for parity 1, else 1;  c = (rgb[k] factor) shade.  A box's face carries the same checker over the two world axes other than
 * the face's, in index order (i < j): parity = (floor((x - c)_i / checker) + floor((x - c)_j / checker)) & 1.
 * Fade: a = clamp((t_max - t) / (0.5 t_max), 0, 1) — an endless floor dissolves into the background instead of ending at a line.
 * Composite, with s = weights_sum[i], acc = image[i] on entry (the frame composited over 0), t_obj = depth_0[i] / s when s > 1e-4, else +inf:
 *     no hit    : out = acc                    cov = s
 *     t < t_obj : out = a c + (1 - a) acc      cov = a + (1 - a) s        the collider in front of the object
 *     otherwise : out = acc + ((1 - s) a) c    cov = s + (1 - s) a        the collider behind it
 *     image[i] = out + (1 - cov) bg_scalar;  coverage_out[i] = cov;  collider_t_out[i] = t, or +inf without a hit
 * A ray without a hit gets the bits the frame's epilogue writes for the same background: acc + (1 - s) bg, multiply and add rounded separately.
 * A depth test, not a clamp of the march: exact where the object is opaque at the collider's depth; a collider inside a semi-transparent part of the
 * object is drawn wholly in front of it or wholly behind.  weights_sum and depth_0 are only read.  The style is a by-value kernel argument: a
 * captured launch keeps the style it was captured with (changing it needs a recapture). */
typedef struct pn_collider_style {
    float rgb[8][3];       /* one colour per slot (PN_CONTACT_SLOTS) */
    float checker;         /* cell size of a plane's checker pattern in world units; <= 0: no pattern */
    float checker_dim;     /* factor of the odd cells */
    float ambient;         /* in [0, 1]: the shade of a surface seen edge-on */
} pn_collider_style;
/* rays_o, rays_d [N,3], weights_sum, depth_0 [N], image [N,3] in place; coverage_out, collider_t_out [N] or NULL.  PN_ERR_ARG for a NULL required
 * pointer, an output overlapping an input, t_max <= t_min, a non-finite scalar or style entry, ambient outside [0, 1], N > (2^31 - 1) / 3.  N == 0:
 * success, nothing launched.  One launch, 256 threads per workgroup; no atomics, no allocation, no host synchronisation: legal in a stream capture. */
int pn_draw_colliders(const void* contact_state, const pn_collider_style* style, const float* rays_o, const float* rays_d, uint32_t N, float t_min,
                      float t_max, float bg_scalar, const float* weights_sum, const float* depth_0, float* image, float* coverage_out,
                      float* collider_t_out, void* stream);

/* The same launch with the object's shadow on the colliders (csrc/pn_colliders.hip; NeRFRenderer.set_collider_shadows).  The light is
 * directional: shadow_ws / shadow_depth_0 [S S] are weights_sum and depth_0 of a render of the object along the parallel rays of
 * pienerf_amd.colliders.shadow_rays — texel (i, j) at index j S + i, origin c + D L + ((i + 1/2) 2 / S - 1) half U + ((j + 1/2) 2 / S - 1) half V,
 * direction -L (a unit vector: the render's t is in world units).  L points from the scene towards the light; U, V are orthonormal to it.
 * Everything is fp32, one rounding per operation, sums left to right.  For a ray whose hit slot is k at t, x = o + t d as pn_draw_colliders
 * computes it, r = x - c:
 *     u = U.r, v = V.r, w = L.r, t_r = D - w                                 the receiver's t along its light ray
 *     fu = (u + half) (S / (2 half)) - 0.5, fv likewise;  i0 = floor(fu), j0 = floor(fv), a_u = fu - i0, a_v = fv - j0
 *     sum over the texels (i0 + di, j0 + dj), (di, dj) = (0,0), (1,0), (0,1), (1,1), starting from 0: a texel outside [0, S)^2 adds nothing; else with
 *     s_m = shadow_ws[idx], t_o = shadow_depth_0[idx] / s_m when s_m > 1e-4, else +inf: it adds (w_u w_v) s_m when t_r > t_o + bias, else nothing,
 *     w_u = 1 - a_u for di = 0 and a_u for di = 1, w_v likewise           (the object's mean depth along the light ray, as the camera-side test)
 *     occ_map = clamp(sum, 0, 1)
 *     with spheres != 0, every valid slot k' != k holding a solid sphere (c', R):  oc = x - c', b = oc.L, disc = b b - (oc.oc - R R);  it blocks the
 *     light iff disc > 0 and -b + sqrt(disc) > 0;  occ_sph = 1 if any blocks, else 0.  Planes and the container cast nothing.
 *     Likewise every valid slot k' != k holding a box or a capsule: with the intervals of pn_draw_colliders for the ray (o, d) = (x, L), q = L.L, a
 *     box blocks the light iff t_enter < t_exit and t_exit > 0, a capsule iff a part is hit and t_far > 0 (the ray x + s L, s > 0, passes through
 *     the solid);  a blocker sets occ_sph = 1.
 *     occ = max(occ_map, occ_sph);  the slot's colour c of pn_draw_colliders becomes c (1 - strength occ), per component;  shadow_out[i] = occ
 * The composite, coverage_out and collider_t_out are pn_draw_colliders' own, and so is a ray without a hit (shadow_out = 0).  Hence strength = 0, an
 * all-zero map without sphere casters, and every ray with occ = 0 give pn_draw_colliders' bits.  The maps are read at execution time (a captured
 * launch follows them); the light is a by-value kernel argument, baked into a captured launch like the style.
 * Limits: a collider between two parts of the object is judged against the middle of the column; the object receives no shadow from the colliders; a
 * sphere's, box's or capsule's own unlit side is not darkened; no penumbra beyond the bilinear footprint and the object's own soft opacity. */
typedef struct pn_shadow_light {
    float c[3];            /* the map's centre */
    float L[3];            /* unit vector from the scene towards the light */
    float U[3], V[3];      /* orthonormal to L: the map's axes */
    float half;            /* the map's half-extent in world units, > 0 */
    float D;               /* distance of the light rays' origins from c along L */
    int S;                 /* map resolution, 2 .. 4096 */
    float strength;        /* in [0, 1] */
    float bias;            /* world units */
    int spheres;           /* != 0: solid sphere, box and capsule colliders cast analytic shadows */
} pn_shadow_light;
/* pn_draw_colliders' arguments and checks, plus: shadow_ws, shadow_depth_0 [S S]; shadow_out [N] or NULL.  PN_ERR_ARG also for S outside 2 .. 4096, a
 * non-finite light entry, half <= 0, strength outside [0, 1], a NULL map, a map overlapping an output, shadow_out overlapping an input or another
 * output.  N == 0: success, nothing launched.  One launch, a thread per ray, 256 threads per workgroup; no atomics, no allocation, no host
 * synchronisation: legal in a stream capture. */
int pn_draw_colliders_shadowed(const void* contact_state, const pn_collider_style* style, const float* rays_o, const float* rays_d, uint32_t N,
                               float t_min, float t_max, float bg_scalar, const float* weights_sum, const float* depth_0, float* image,
                               float* coverage_out, float* collider_t_out, pn_shadow_light light, const float* shadow_ws, const float* shadow_depth_0,
                               float* shadow_out, void* stream);

/* The simulator's integration points and the drag handle drawn into a rendered frame (csrc/pn_points_overlay.hip; NeRFRenderer.set_point_overlay;
 * DESIGN.md 4.13): the reference's "render IPs" checkbox (nerf/gui.py:533-540, overlay_point_buffer) and the red and blue discs with the line between
 * them on a dragged point (gui.py:561-569).  TWO launches on `stream` with the per-frame key buffer `keys` between them, behind the frame driver, the
 * colliders' launch and the background's blend: they paint onto the finished picture.  pos, F, values, pose16 and drag are DEVICE memory read at
 * execution time: a captured pair follows the simulator, the camera and the cursor without a recapture.  Everything is fp32, one rounding per
 * operation, sums left to right.  pose16 is the c2w matrix, row-major: R[r][k] = pose16[4 r + k], c = (pose16[3], pose16[7], pose16[11]).
 * Projection of a world point x (the camera looks along +z, as gui.py:660-667 and get_rays have it):
 *     d = x - c;  xc = R[0][0] d0 + R[1][0] d1 + R[2][0] d2, yc and zc likewise with columns 1 and 2 (xc = R^T d);  t = sqrt(d0 d0 + d1 d1 + d2 d2)
 *     u = xc / zc fx + cx,  v = yc / zc fy + cy      (divide, multiply, add);  drawable iff x, t, u, v are finite and zc > 0
 * Splat, a thread per point i, 256 per workgroup: a point that is not drawable or has t <= t_min is dropped.  px = floor(u), py = floor(v): row py,
 * column px, index py W + px.  Every pixel (px + dx, py + dy) inside the image with dx dx + dy dy <= radius^2 (integers) takes an unsigned 64-bit
 * atomic min of (bits(t) << 32) | i into keys — t > 0, so its bits order as the floats do: per pixel the nearest point wins, the lowest index on
 * ties, in whatever order the hardware ran anything.  No other atomics.  (A plain load skips the atomic where the stored key is already smaller: min is
 * monotone, the result cannot change.)
 * Two deviations from the reference, both its defects: it projects a point BEHIND the camera mirrored through the centre onto the picture (zc < 0 is not
 * tested), here the point is dropped; and its int() truncates toward zero where this floors, which differs only for u or v in (-1, 0), where the
 * reference paints an off-screen point onto the border row or column.  Its double swap at gui.py:536-539 amounts to row py, column px.
 * Resolve, a thread per pixel p: reads keys[p] and, unless it is the empty value ~0, writes ~0 back — the buffer is all-empty between calls (fill it
 * once when it is allocated).  With a key, i = its low word, t = the float of its high word, s = weights_sum[p]:
 *     t_obj = depth_0[p] / s when s > 1e-4, else +inf;  t_front = min(t_obj, collider_t[p]) with collider_t, else t_obj      (the colliders' own test)
 *     visible iff xray != 0 or t <= t_front + bias;  a = alpha when visible, else alpha hidden_alpha;  hidden and hidden_alpha == 0: nothing is drawn
 *     colour c:  PN_POINT_FLAT: rgb.   Otherwise a scalar v of point i, F = F[i] row-major (F[r][k] = F[9 i + 3 r + k]):
 *         PN_POINT_STRAIN: C[a][b] = F[0][a] F[0][b] + F[1][a] F[1][b] + F[2][a] F[2][b], E[a][b] = 0.5 (C[a][b] - (a == b)),
 *                          v = sqrt(sum of E[a][b] E[a][b] over a, then b, starting from 0)                                    (|| 1/2 (F^T F - I) ||_F)
 *         PN_POINT_VOLUME: v = (F00 (F11 F22 - F12 F21) - F01 (F10 F22 - F12 F20) + F02 (F10 F21 - F11 F20)) - 1                (det F - 1)
 *         PN_POINT_VALUES: v = values[i]
 *         u = min(max((v - lo) / (hi - lo), 0), 1);  u < 0.5: w = 2 u, c = ramp[0] + w (ramp[1] - ramp[0]);  else w = 2 (u - 0.5),
 *         c = ramp[1] + w (ramp[2] - ramp[1]), per component
 *     image[p] = a c + (1 - a) image[p];  point_id_out[p] = i, point_t_out[p] = t       (else -1 and +inf)
 * Markers, with drag != NULL and drag->active != 0, in the same launch, per pixel centre q = (column + 1/2, row + 1/2), after the point, in the
 * reference's order: A = (u, v) of pos[drag->vid] (0 <= vid < n), B = (u, v) of drag->target rounded to fp32 once; an end that is not drawable drops
 * its disc and the line.  |q - A|^2 <= marker_radius^2: image[p] = (1, 0, 0);  then |q - B|^2 <= marker_radius^2: image[p] = (0, 0, 1);  then with
 * e = B - A, g = q - A, h = min(max((g.e) / (e.e), 0), 1) (0 when e.e == 0), f = g - h e:  f.f <= (0.5 marker_thickness)^2: image[p] = (1 - 100 / 255) image[p]
 * (black at alpha 100 / 255).  Squared lengths are x x + y y.  Markers ignore the depth test and t_min and do not write point_id_out.
 * A pixel with no key and no marker keeps its image bits.  weights_sum, depth_0 and collider_t are only read.
 * Limits: one point per pixel (the nearest; no blending of several), no anti-aliasing, and a depth test against the object's MEAN depth depth_0 / s: a
 * point inside a semi-transparent part is wholly in front of it or wholly behind. */
enum { PN_POINT_FLAT = 0, PN_POINT_STRAIN = 1, PN_POINT_VOLUME = 2, PN_POINT_VALUES = 3 };
typedef struct pn_point_style {
    int radius;              /* footprint radius in pixels, 0 .. 8 */
    int mode;                /* PN_POINT_* */
    int xray;                /* != 0: every point is visible (the reference's behaviour); 0: depth-tested ("occluded") */
    float rgb[3];            /* PN_POINT_FLAT's colour */
    float ramp[3][3];        /* the ramp modes' colours at u = 0, 1/2, 1 */
    float lo;                /* the ramp's range: u = 0 at lo ... */
    float hi;                /* ... and 1 at hi */
    float alpha;             /* in [0, 1] */
    float hidden_alpha;      /* in [0, 1]: factor on alpha for a point behind the object or a collider; 0: not drawn */
    float bias;              /* depth-test slack, in units of t */
    float marker_radius;     /* the drag handle's discs, in pixels (the reference: 10) */
    float marker_thickness;  /* ... and its line (the reference: 5) */
} pn_point_style;
uint64_t pn_points_keys_bytes(int W, int H);   /* 8 W H; 0 for W or H <= 0 */
/* pos [n,3]; F [n,9] or NULL; values [n] or NULL; pose16 [16] device; intr4_host = (fx, fy, cx, cy) on the HOST, baked into the launch like the style;
 * weights_sum, depth_0 [W H]; collider_t [W H] or NULL (pn_draw_colliders' collider_t_out); drag: a device pn_drag_state or NULL; keys [W H] uint64,
 * all ~0 on entry and on exit; image [W H,3] in place; point_id_out [W H] int32 and point_t_out [W H] or NULL.  PN_ERR_ARG for a NULL required
 * pointer, an output (image, keys, point_id_out, point_t_out) overlapping an input or another output, radius outside 0 .. 8, an unknown mode, a
 * non-finite style entry, intrinsic or t_min, alpha or hidden_alpha outside [0, 1], hi <= lo in a ramp mode, PN_POINT_STRAIN / PN_POINT_VOLUME
 * without F, PN_POINT_VALUES without values, n < 0, n or W H beyond int32, W or H <= 0.  n == 0 without a drag: success, nothing launched (with a
 * drag: the resolve launch alone).  No allocation, no host synchronisation: legal in a stream capture. */
int pn_draw_points(const float* pos, const float* F, const float* values, int64_t n, const float* pose16, const float* intr4_host, int W, int H,
                   float t_min, const float* weights_sum, const float* depth_0, const float* collider_t, const void* drag, uint64_t* keys,
                   pn_point_style style, float* image, int* point_id_out, float* point_t_out, void* stream);

/* Arbitrary rest-space points carried by the simulator's GMLS field (csrc/pn_warp_points.hip; simulator/binding.py: PointBinding.warp; INTEGRATION.md
 * "Deforming mesh").  Per point p, in fp64: pos = sum_{i<8} sum_{c<10} Nx[p,i,c] dof[topo[p,i] 10 + c, :], rounded to fp32 once.  With normals_out:
 * F[r][j] = sum_i sum_c dNx[p,i,j,c] dof[topo[p,i] 10 + c, r], n' = n0 (f1 x f2) + n1 (f2 x f0) + n2 (f0 x f1) with f_j = column j of F and
 * n = normals0[p] (cof(F) n: no division, no inverse), normalised in fp64 and rounded to fp32 once; |n'| zero or not finite: normals0[p] unchanged.
 * Tables, built once at bind time in groups of G = pn_sim_warp_points_group() = 8 points, n_g = ceil(n_pts / G) groups, lane l of a group's wave =
 * point l / 8, neighbour slot l % 8; rows behind the last point are zeros:
 *   topo_g [n_g][64] int32      = topo [n_g G, 8] row-major, entries in [0, n_k);
 *   Nx_g   [n_g][5][64][2] fp64: the lane's 10 weights Nx[p,i,:] as 5 pairs;
 *   dNx_g  [n_g][15][64][2] fp64: the lane's 30 gradients dNx[p,i,j,c] (flat j 10 + c) as 15 pairs (needed with normals_out only).
 * Nx_g, dNx_g and dof are read 16 bytes per lane and must be 16-byte aligned.  dof [10 n_k,3] fp64 is read from the pointer at execution time;
 * normals0 [n_pts,3] fp32; pos_out, normals_out [n_pts,3] fp32 (normals_out NULL: positions only; dNx_g and normals0 may then be NULL).
 * Each lane sums its slot over c = 0..9 in order, the 8 slots are added as ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)): a point's bits depend on
 * its own row only, not on the other points of the call.  One launch, no atomics, no allocation, no host synchronisation: legal inside a stream
 * capture.  PN_ERR_ARG for n_pts <= 0, n_k <= 0, a missing or misaligned pointer. */
int pn_sim_warp_points_group(void);
int pn_sim_warp_points(int n_pts, int n_k, const int* topo_g, const double* Nx_g, const double* dNx_g, const double* dof, const float* normals0,
                       float* pos_out, float* normals_out, void* stream);

/* ------------------------------------------------------------------ meshing ---- */

/* Marching cubes (nerf/utils.py:174-205 extract_geometry's mcubes.marching_cubes; csrc/pn_mesh.hip, INTEGRATION.md "Meshing").  `field` is a
 * C-contiguous fp32 lattice [nx, ny, nz] (z fastest), every dimension >= 2, 3 nx ny nz < 2^31 and 5 (nx-1)(ny-1)(nz-1) < 2^31 (else PN_ERR_ARG;
 * pn_mc_work_bytes returns 0).  A node is above when (double)f > threshold.  One vertex per crossed lattice edge, at lo + t on the edge's axis with
 * t = (threshold - f0) / (f1 - f0) in fp64 from the lower endpoint; vertices in node order then axis, triangles in cell order then case-table
 * order, pointing out of the above-threshold region.  No atomics: the output is a pure function of the field and the threshold.
 * pn_mc_count enqueues the count and the scan and writes totals [2] = {V, T} (device int64); the caller reads them to size vertices [V,3] fp64
 * (index space) and triangles [T,3] int32, then pn_mc_emit (V = 0 implies T = 0: nothing to emit).  `work`: pn_mc_work_bytes bytes, kept between
 * the two calls with the same field and threshold. */
uint64_t pn_mc_work_bytes(int nx, int ny, int nz);
int pn_mc_count(const float* field, int nx, int ny, int nz, double threshold, void* work, int64_t* totals, void* stream);
int pn_mc_emit(const float* field, int nx, int ny, int nz, double threshold, const void* work, double* vertices, int* triangles, void* stream);
/* [host] The case table the kernels use: tri_count [256], tri_edges [256*15] (Bourke edge ids, -1 padded).  No GPU needed. */
int pn_mc_case_table(uint8_t* tri_count, int8_t* tri_edges);

/* Connected-component labelling of an occupancy lattice (csrc/pn_components.hip, DESIGN.md 4.6, INTEGRATION.md "Connected components").  `occ` is a
 * C-contiguous uint8 lattice [nx, ny, nz] (z fastest, pn_mc_count's layout), non-zero = occupied; `labels` is int32 of the same shape.  An occupied
 * voxel receives the smallest flat index (i*ny + j)*nz + k of any voxel of its component, an empty voxel -1.  connectivity: 6 (faces) or 26 (faces,
 * edges and corners).  PN_ERR_ARG for a null pointer, a side < 1, nx*ny*nz >= 2^31 or any other connectivity (checked before anything is enqueued).
 * Three launches on `stream` whatever the data, no scratch memory (`labels` is the union-find's parent array), no allocation and no host
 * synchronisation: legal inside a stream capture.  Integer atomicMin union-find hooking the larger root under the smaller: the labels are a pure
 * function of `occ`. */
int pn_ccl_label(const uint8_t* occ, int nx, int ny, int nz, int connectivity, int* labels, void* stream);

/* ------------------------------------------------------------------ training data ---- */

/* The data side of a training step (csrc/pn_train_batch.hip, INTEGRATION.md "Training data").  Random numbers are inputs drawn by the caller, so each
 * entry is a pure function of its arguments. */

/* Weighted sampling without replacement, for torch.multinomial(error_map, N, replacement=False) (nerf/utils.py:106).  weights [n_cells] fp32 >= 0,
 * n_cells <= 16384; expo [n_cells]: Exp(1) draws.  cells_out [N] int64: the N cells with the largest keys weights[i] / expo[i] (IEEE division), in
 * ascending cell index; a tie at the N-th key goes to the lower index; a cell of weight zero is never returned.  *status (device int) = 0, or 1 when
 * fewer than N weights are positive (cells_out is then not written).  One workgroup, no atomics: equal inputs give equal bytes. */
int pn_sample_cells(const float* weights, const float* expo, int n_cells, int N, int64_t* cells_out, int* status, void* stream);
/* get_rays with N > 0 for one pose (nerf/utils.py:77-136) and the gather of the ground truth (nerf/provider.py:311-316), one launch.
 * pose: device, row-major 4x4 cam2world.  mode 0 (:101): a [N] = pixel indices.  mode 1 (:106-115): a [N] = coarse cells of the 128 x 128 error
 * map, u [2, N] uniforms in [0, 1).  mode 2 (:81-98): a, b [N / patch^2] = top-left rows / columns of the patches, pixels patch-major, then patch
 * row, then patch column.  Writes inds_out [N] int64 (row * W + col), rays_o / rays_d [N, 3] — a pixel's direction is bit for bit pn_get_rays' —
 * and, when `image` [H, W, C] fp32 (C = 3 or 4) is given, pixels_out [N, C] = image[inds].  a, b: int64. */
int pn_train_batch(const float* pose, float fx, float fy, float cx, float cy, int H, int W, int N, int mode, const int64_t* a, const int64_t* b,
                   const float* u, int patch, const float* image, int C, int64_t* inds_out, float* rays_o, float* rays_d, float* pixels_out,
                   void* stream);
/* The error map's moving average (nerf/trainer.py:239-243): map_row[cells[i]] = 0.1f * map_row[cells[i]] + 0.9f * err[i], i < N; map_row [128 * 128]
 * is the row of the batch's view, cells [N] int64 are distinct. */
int pn_error_map_update(float* map_row, const int64_t* cells, const float* err, int N, void* stream);

/* ------------------------------------------------------------------ image metrics ---- */

/* SSIM of channel-last images (csrc/pn_ssim.hip, pienerf_amd/metrics.py): what torchmetrics' structural_similarity_index_measure
 * computes for the reference's SSIMMeter (nerf/utils.py:268-302).  pred, truth [B, H, W, C] fp32 contiguous, H, W >= 11, C >= 1, B <= 65535,
 * H W C < 2^31.  Window: 11 taps g_i = exp(-((i - 5) / 1.5)^2 / 2) / sum (double on the host, rounded to fp32), weight g_i g_j.  Only the
 * (H - 10) x (W - 10) positions whose whole window lies inside the image exist.  Per position and channel, with w-weighted sums over the window:
 *     mx = E[x], my = E[y], sxx = E[xx] - mx^2, syy = E[yy] - my^2, sxy = E[xy] - mx my,
 *     S = ((2 mx my + c1)(2 sxy + c2)) / ((mx^2 + my^2 + c1)(sxx + syy + c2)),   c1 = (0.01 R)^2, c2 = (0.03 R)^2.
 * out [B] = the mean of S over positions and channels.  The kernels read {c1, c2} from the device buffer c12 [2], so no form of the data range makes
 * the host wait.  Every entry: no atomics, fixed summation order (equal inputs give equal bits), no allocation, no host synchronisation; PN_ERR_ARG
 * (nothing launched) for a null pointer or a shape outside the above. */
/* Bytes of `work` (8-byte aligned) for pn_ssim_range and pn_ssim_forward on [B, H, W, *]: the range kernel's partial extrema and one fp64 partial
 * per workgroup (16 x 16 output tile) and image.  0 for an illegal shape. */
uint64_t pn_ssim_work_bytes(int B, int H, int W);
/* c12 = {(0.01 R)^2, (0.03 R)^2} in fp32.  pred == truth == NULL: R = data_range (> 0, finite), one launch.  Otherwise R = max(pred.max() -
 * pred.min(), truth.max() - truth.min()) over the n floats of each, two launches (data_range is ignored; two constant images give R = 0 and S = 0/0,
 * as in the reference; a NaN pixel is skipped by the extrema, where torch's max would return it). */
int pn_ssim_range(const float* pred, const float* truth, uint64_t n, float data_range, void* work, float* c12, void* stream);
/* out [B]; with mapA, mapB, mapD (all three or none), each [B, H-10, W-10, C]: B = dS/dsxx, D = dS/dsxy, A = dS/dmx - 2 mx B - my D, the maps
 * pn_ssim_backward reads.  Two launches (tiles, then the fixed-order sum of their partials). */
int pn_ssim_forward(const float* pred, const float* truth, int B, int H, int W, int C, const float* c12, void* work, float* out, float* mapA,
                    float* mapB, float* mapD, void* stream);
/* grad_pred [B, H, W, C] = grad_out[b] / ((H-10)(W-10)C) * ((w * A)_q + 2 x_q (w * B)_q + y_q (w * D)_q): the gradient of sum_b grad_out[b] out[b]
 * with respect to pred (R constant; truth gets none).  `*` is the full correlation of a map, zero outside the valid region, with the window, at every
 * pixel q.  Gather form, one launch. */
int pn_ssim_backward(const float* pred, const float* truth, int B, int H, int W, int C, const float* mapA, const float* mapB, const float* mapD,
                     const float* grad_out, float* grad_pred, void* stream);

/* ------------------------------------------------------------------ video ---- */

/* A frame as a baseline sequential JPEG (SOF0, 8 bit, 3 components, interleaved), encoded on the device (csrc/pn_jpeg.hip, pienerf_amd/video.py,
 * DESIGN.md 4.14).  `image` [H, W, 3] fp32 on the device, as the renderer leaves it.  Written: the entropy-coded scan — everything between the SOS
 * header and EOI, restart markers included — to stream_out, and its length in bytes to *nbytes_out (both device memory); the host prepends the
 * header (video.jpeg_header) and appends EOI.  subsampling: 420 (MCU 16 x 16: Y00 Y01 Y10 Y11 Cb Cr) or 444 (MCU 8 x 8: Y Cb Cr).
 * The arithmetic, all fp32, one rounding per operation, sums left to right (tests/jpeg_reference.py restates it; the bytes agree):
 *   pixel     c = isnan(v) ? 0 : min(max(v, 0), 1), p = floorf(c * 255.0f) (io.save_image's truncation); a frame whose W or H is no multiple of the
 *             MCU is padded by replicating its last column and row;
 *   colour    Y = 0.299f R + 0.587f G + 0.114f B - 128.0f, Cb = -0.168735892f R - 0.331264108f G + 0.5f B,
 *             Cr = 0.5f R - 0.418687589f G - 0.081312411f B; a 4:2:0 chroma sample is ((tl + tr) + (bl + br)) * 0.25f of the converted values;
 *   DCT       t[y][u] = sum_x s[y][x] C[u][x], then d[v][u] = sum_y C[v][y] t[y][u], C[u][x] = (float)(c(u) / 2 cos((2x + 1) u pi / 16)) from fp64
 *             (csrc/pn_jpeg_tables.h);
 *   quantise  q = rintf(d / (float)Q[k]), ties to even; AC values clamped to +-1023, DC differences to +-2047 (baseline's categories);
 *   entropy   the typical Huffman tables of T.81 Annex K; one restart interval per MCU row (DRI = MCUs per row), the DC predictors reset at each;
 *             an interval is padded with 1-bits to a byte, a 0x00 follows every 0xFF byte, and FF D0+(r mod 8) follows interval r but the last.
 * The two quantisation tables (64 entries of 1 .. 255, natural order, HOST memory) are read during the call and travel by value in the launch.
 * Three launches on `stream`; no allocation, no host synchronisation, no host-visible side effect: legal inside a stream capture, and a captured launch
 * keeps the tables it was captured with.  Equal inputs give equal bytes.
 * PN_ERR_ARG before anything is enqueued for: a NULL pointer; W or H of 0 or above 65535; another subsampling; a frame whose bound below does not fit the
 * 32-bit count; a table entry of 0; capacity below pn_jpeg_stream_capacity; `work` not 16-byte aligned; stream_out, work or nbytes_out overlapping image
 * or each other. */
/* A proven bound on the scan's bytes: a block is at most 20 + 63 * 26 bits < 208 bytes, doubled by stuffing: n_blocks * 416 + 2 (mcu_rows - 1).  The
 * encoder requires this capacity and cannot pass it; there is no overflow flag.  0 for arguments pn_jpeg_encode refuses. */
uint64_t pn_jpeg_stream_capacity(uint32_t W, uint32_t H, int subsampling);
/* Bytes of `work` (16-byte aligned): the coefficients, the intervals' bit staging and stuffed segments (both sized from the worst case) and their
 * offsets.  Nothing in it outlives the call's launches.  0 for arguments pn_jpeg_encode refuses. */
uint64_t pn_jpeg_work_bytes(uint32_t W, uint32_t H, int subsampling);
int pn_jpeg_encode(const float* image, uint32_t W, uint32_t H, int subsampling, const uint8_t* qtab_luma_host64, const uint8_t* qtab_chroma_host64,
                   void* work, uint8_t* stream_out, uint64_t capacity, uint32_t* nbytes_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PIENERF_HIP_H */
