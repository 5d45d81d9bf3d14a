"""The static (undeformed) render of NeRFRenderer and the density-grid state it marches through (nerf/renderer.py:125-135, 267-549 of the reference;
csrc/pn_grid_state.hip): run_cuda with its one-call frame driver and its op-by-op loop, reset_extra_state / mark_untrained_grid /
update_extra_state, and aabb_infer on the host, which the hierarchical render (render_hier.py) reads as well."""
import ctypes as C

import torch

from .. import raymarching
from .._lib import check, lib, ptr, require_gpu, stream_ptr
from ._outputs import flat_rays, frame_outputs


class StaticRenderMixin:
    def reset_extra_state(self):
        """renderer.py:125-135."""
        if not self.cuda_ray:
            return
        self.density_grid.zero_()
        self.mean_density = 0
        self.iter_density = 0
        self.step_counter.zero_()
        self.mean_count = 0
        self.local_step = 0

    def run_cuda(self, rays_o, rays_d, dt_gamma=0, bg_color=None, perturb=False, force_all_rays=False, max_steps=1024, T_thresh=1e-2, **kwargs):
        """NeRFRenderer.run_cuda (nerf/renderer.py:267-387), the static / undeformed render.

        train():  march_rays_train -> network (differentiable) -> composite_rays_train, the step counter feeding ``mean_count`` (:293-341).
        eval():   ONE call of the frame driver pn_render_static — near / far from aabb_infer, then trips of march / network / composite /
                  stable compaction driven by a device-side trip record, with one 16-byte read-back per batch of 8 trips (the reference
                  synchronises the host on every trip, :351-380).  Per-ray background colours and ``perturb`` take the op-by-op loop
                  ``run_cuda_ops`` (same kernels, host-driven)."""
        self._refuse_overlays("the static render (run_cuda)")
        if not self.training and not perturb and (self.bg_radius > 0 or not torch.is_tensor(bg_color)):
            return self._run_static_fused(rays_o, rays_d, dt_gamma, 1 if bg_color is None else bg_color, max_steps, T_thresh, **kwargs)
        return self.run_cuda_ops(rays_o, rays_d, dt_gamma, bg_color, perturb, force_all_rays, max_steps, T_thresh, **kwargs)

    def _run_static_fused(self, rays_o, rays_d, dt_gamma, bg_color, max_steps, T_thresh, **kwargs):
        prefix = rays_o.shape[:-1]
        rays_o, rays_d = flat_rays(rays_o, rays_d)
        require_gpu(rays_o, rays_d)
        if self.bg_radius > 0:
            bg_color = 0   # renderer.py:283-288: the model's colour, blended in below
        N, device = rays_o.shape[0], rays_o.device
        o = self._static_opts(dt_gamma, bg_color, max_steps, T_thresh)
        aabb = (C.c_float * 6)(*self._aabb_infer_host())
        image, depth, depth_0, ws = frame_outputs(N, device)
        slot = int(kwargs.get("frame_slot") or 0)
        frame = self._frame_handle(N, 1, 1.0, slot, cells=1)
        self._static_depth_0[slot] = depth_0   # render_continue(static=True) composites on into it
        async_trips = int(kwargs.get("async_trips") or 0)
        stats = (C.c_int64 * 5)() if not async_trips else None
        check(lib().pn_render_static(frame, self._net_handle(half=bool(o.fp16)), C.byref(o), ptr(rays_o), ptr(rays_d), N, aabb, ptr(self.density_bitfield),
                                     ptr(image), ptr(depth), ptr(depth_0), ptr(ws), stats, async_trips, stream_ptr()), "render_static")
        if self.bg_radius > 0:
            self.blend_background(rays_o, rays_d, ws, image)
        if stats is not None:
            self._set_stats(stats)
        return {"depth": depth.view(*prefix), "image": image.view(*prefix, 3), "weights_sum": ws}

    def _aabb_infer_host(self):
        """aabb_infer as six Python floats, read back from the device only when the buffer changed (never inside a stream capture)."""
        key = (self.aabb_infer.data_ptr(), self.aabb_infer._version)
        if self._aabb_cache[0] != key:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("aabb_infer changed: render one frame outside stream capture first")
            self._aabb_cache = (key, [float(v) for v in self.aabb_infer.tolist()])
        return self._aabb_cache[1]

    def run_cuda_ops(self, rays_o, rays_d, dt_gamma=0, bg_color=None, perturb=False, force_all_rays=False, max_steps=1024, T_thresh=1e-2, **kwargs):
        """run_cuda op by op on the drop-in ops (the training branch; the eval branch with perturb / tensor backgrounds; parity tests)."""
        self._refuse_overlays("the static render (run_cuda_ops)")
        shape = rays_o.shape[:-1]
        o3, d3 = rays_o.contiguous().view(-1, 3), rays_d.contiguous().view(-1, 3)
        nears, fars = raymarching.near_far_from_aabb(o3, d3, self.aabb_train if self.training else self.aabb_infer, self.min_near)
        if self.bg_radius > 0:  # renderer.py:283-286: the model's colour; in train() mode through the differentiable ops
            bg_color = self.background(raymarching.sph_from_ray(o3, d3, self.bg_radius), d3)
        bg = 1 if bg_color is None else bg_color

        def shade(xyzs, dirs):
            sig, rgb = self(xyzs, dirs)
            return self.density_scale * sig, rgb

        if self.training:
            slot = self.step_counter[self.local_step % 16]
            slot.zero_()
            self.local_step += 1
            xyzs, dirs, deltas, rays = raymarching.march_rays_train(o3, d3, self.bound, self.density_bitfield, self.cascade, self.grid_size, nears, fars, slot,
                                                                    self.mean_count, perturb, 128, force_all_rays, dt_gamma, max_steps)
            ws, depth, image = raymarching.composite_rays_train(*shade(xyzs, dirs), deltas, rays, T_thresh)
            self.last_stats = dict(trips=1, samples=int(xyzs.shape[0]), err=0, alive_at_exit=0)
        else:
            with torch.no_grad():
                n_rays, dev = o3.shape[0], o3.device
                ws, depth, image = (torch.zeros(n_rays, device=dev), torch.zeros(n_rays, device=dev), torch.zeros(n_rays, 3, device=dev))
                alive, t_now = torch.arange(n_rays, dtype=torch.int32, device=dev), nears.clone()
                done_steps = trips = samples = 0
                while done_steps < max_steps and alive.shape[0] > 0:
                    k = alive.shape[0]
                    per_ray = max(min(n_rays // k, 8), 1)
                    xyzs, dirs, deltas = raymarching.march_rays(k, per_ray, alive, t_now, o3, d3, self.bound, self.density_bitfield, self.cascade,
                                                                self.grid_size, nears, fars, 128, perturb if done_steps == 0 else False, dt_gamma, max_steps)
                    raymarching.composite_rays(k, per_ray, alive, t_now, *shade(xyzs, dirs), deltas, ws, depth, image, T_thresh)
                    alive = raymarching.compact_rays(alive)
                    samples += int((deltas[:, 0] != 0).sum())
                    done_steps += per_ray
                    trips += 1
                self.last_stats = dict(trips=trips, samples=samples, err=0, alive_at_exit=int(alive.shape[0]))
        image = image + (1 - ws).unsqueeze(-1) * bg
        depth = torch.clamp(depth - nears, min=0) / (fars - nears)
        return {"depth": depth.view(*shape), "image": image.view(*shape, 3), "weights_sum": ws}

    # ------------------------------------------------------------------ density-grid state on the device (pn_grid_state.hip)
    @torch.no_grad()
    def mark_untrained_grid(self, poses, intrinsic, S=64):
        """renderer.py:390-452: cells of the density grid that no training camera sees get density -1 (never sampled, never updated).
        One launch — a lane per (cascade, cell) loops over the poses — instead of the reference's five nested Python loops; returns the
        number of unseen cells (the reference prints it).  ``S`` (the reference's block / pose-batch size) has no role here."""
        if not self.cuda_ray:
            return
        cams = torch.as_tensor(poses).to(device=self.density_grid.device, dtype=torch.float32).contiguous().view(-1, 4, 4)
        require_gpu(cams, self.density_grid)
        fx, fy, cx, cy = (float(v) for v in intrinsic)
        n_unseen = torch.zeros(1, dtype=torch.int32, device=cams.device)
        check(lib().pn_mark_untrained_grid(ptr(cams), cams.shape[0], fx, fy, cx, cy, self.cascade, self.grid_size, float(self.bound),
                                           ptr(self.density_grid), ptr(n_unseen), stream_ptr()), "mark_untrained_grid")
        return int(n_unseen.item())

    @torch.no_grad()
    def update_extra_state(self, decay=0.95, S=128):
        """renderer.py:454-549.  Density grid: sigma at one jittered sample per cell — every cell for the first 16 calls, afterwards H^3/4
        uniform cells + H^3/4 draws from the occupied cells per cascade — EMA-max into the grid, mean of the non-negative part, bitfield at
        min(mean, density_thresh); then ``mean_count`` from the step counters.  Everything runs on the device in a handful of launches
        (pn_density_cells_* -> pn_nerf_sigma -> pn_density_grid_update); the only host read-back is the final mean (the reference's
        ``.item()``), and the occupied-cell list of the partial sweep is compacted on the device instead of through torch.nonzero."""
        if not self.cuda_ray:
            return
        grid = self.density_grid
        dev, H, n_cas = grid.device, self.grid_size, self.cascade
        require_gpu(grid)
        cells = H ** 3
        net, half = self._net_handle(half=self._autocast_half()), int(self._autocast_half())
        tmp = torch.empty_like(grid)
        if self.iter_density < 16:
            pts = torch.empty(n_cas * cells, 3, dtype=torch.float32, device=dev)
            check(lib().pn_density_cells_full(n_cas, H, float(self.bound), ptr(torch.rand(n_cas * cells, 3, device=dev)), ptr(pts), stream_ptr()), "density_cells_full")
            check(lib().pn_nerf_sigma(net, ptr(pts), n_cas * cells, float(self.density_scale), ptr(tmp), half, stream_ptr()), "nerf_sigma")
        else:
            n = cells // 4
            scratch = torch.empty(int(lib().pn_density_partial_scratch_ints(H)), dtype=torch.int32, device=dev)
            pts = torch.empty(2 * n, 3, dtype=torch.float32, device=dev)
            idx = torch.empty(2 * n, dtype=torch.int32, device=dev)
            sig = torch.empty(2 * n, dtype=torch.float32, device=dev)
            for cas in range(n_cas):
                draws = torch.randint(0, H, (n, 3), device=dev, dtype=torch.int32)
                check(lib().pn_density_cells_partial(cas, H, float(self.bound), n, ptr(draws), ptr(torch.rand(n, device=dev)), ptr(torch.rand(2 * n, 3, device=dev)),
                                                     ptr(grid[cas]), ptr(tmp[cas]), ptr(scratch), ptr(idx), ptr(pts), stream_ptr()), "density_cells_partial")
                check(lib().pn_nerf_sigma(net, ptr(pts), 2 * n, float(self.density_scale), ptr(sig), half, stream_ptr()), "nerf_sigma")
                check(lib().pn_density_scatter(2 * n, ptr(idx), ptr(sig), ptr(tmp[cas]), stream_ptr()), "density_scatter")
        partial = torch.empty((n_cas * cells + 255) // 256, dtype=torch.float64, device=dev)
        mean_thresh = torch.empty(2, dtype=torch.float32, device=dev)
        check(lib().pn_density_grid_update(n_cas * cells, ptr(grid), ptr(tmp), float(decay), float(self.density_thresh), ptr(self.density_bitfield),
                                           ptr(partial), ptr(mean_thresh), stream_ptr()), "density_grid_update")
        self.mean_density = float(mean_thresh[0].item())
        self.iter_density += 1
        counted = min(16, self.local_step)
        if counted > 0:  # :545-547
            self.mean_count = int(self.step_counter[:counted, 0].sum().item() / counted)
        self.local_step = 0
