"""Deformed-space renderer with the reference's surface (nerf/renderer.py:74-113, 587-599, 755-907).

``NeRFRenderer.render_deformed(rays_o, rays_d, **vars(opt))`` is what ``Trainer.test_step`` calls
(nerf/trainer.py:316-318); the caller sets ``p_ori, p_def, IP_F, IP_dF, IP_dx`` on the model
(main_gui.py:52-56, trainer.py:303-306).  This file holds the class, the deformed frame driver and what it needs:

  * ``rund_cuda``        — one C call (pn_render_deformed): the whole loop runs on the GPU with a device-side
                           (n_alive, n_step) record; no per-trip host synchronisation.
  * ``render_continue``  — more trips of the same loop on a frame whose fixed trip count turned out too small.
  * ``_finish_frame``    — what both enqueue behind the driver: the colliders, the background, the points.
  * the option builders, the frame workspaces, ``render_status``.

The other render forms and the overlays are mixins of the class, a file each:

  * overlay_colliders.py    — the drawn colliders and the object's shadow on them
  * overlay_points.py       — the integration points and the drag handle
  * render_static.py        — ``run_cuda`` and the density-grid state
  * render_hier.py          — ``run`` (no density grid), ``sample_pdf`` and ``render``'s staging
  * render_deformed_ops.py  — ``rund_cuda_ops``: the reference's Python loop verbatim in structure, on the drop-in ops
  * frame_hooks.py          — the measurement hooks on a frame workspace
"""
import ctypes as C
import math

import torch
import torch.nn as nn

from .._lib import RenderOpts, check, lib, ptr, require_gpu, stream_ptr
from ._outputs import flat_rays, frame_outputs
from .frame_hooks import FrameHooksMixin
from .overlay_colliders import ColliderOverlayMixin
from .overlay_points import PointOverlayMixin
from .render_deformed_ops import DeformedOpsMixin
from .render_hier import HierRenderMixin, sample_pdf  # noqa: F401 — sample_pdf stays importable from here
from .render_static import StaticRenderMixin


def frame_background(bg_color, bg_radius, overlay):
    """What a deformed frame is composited over -> (the frame driver's scalar, the collider launch's scalar, the tensor blended in afterwards or None).
    With a background model (bg_radius > 0) its colour replaces whatever was passed (renderer.py:799-803): everything composites over 0 and
    blend_background follows.  None means 1.  A tensor ([3] or [N, 3], e.g. the GUI's bg_color tensor, gui.py:590): the driver composites over 0 and
    image + (1 - covered) * bg (renderer.py:896) is applied afterwards with the same two roundings.  With an `overlay` the driver composites over 0 as
    well: the scalar goes in behind the colliders, in the overlay's launch."""
    if bg_radius > 0:
        return 0.0, 0.0, None
    if bg_color is None:
        bg_color = 1
    if torch.is_tensor(bg_color):
        return 0.0, 0.0, bg_color
    return (0.0 if overlay else bg_color), bg_color, None


class NeRFRenderer(ColliderOverlayMixin, PointOverlayMixin, StaticRenderMixin, HierRenderMixin, DeformedOpsMixin, FrameHooksMixin, nn.Module):
    def __init__(self, bound=1, cuda_ray=False, density_scale=1, min_near=0.2, density_thresh=0.01, bg_radius=-1):
        super().__init__()
        self.bound = bound
        self.cascade = 1 + math.ceil(math.log2(bound))
        self.grid_size = 128
        self.density_scale = density_scale
        self.min_near = min_near
        self.density_thresh = density_thresh
        self.bg_radius = bg_radius
        aabb = torch.FloatTensor([-bound, -bound, -bound, bound, bound, bound])
        self.register_buffer("aabb_train", aabb)
        self.register_buffer("aabb_infer", aabb.clone())
        self.cuda_ray = cuda_ray
        if cuda_ray:  # same state-dict keys as renderer.py:94-111
            self.register_buffer("density_grid", torch.zeros([self.cascade, self.grid_size ** 3]))
            self.register_buffer("density_bitfield", torch.zeros(self.cascade * self.grid_size ** 3 // 8, dtype=torch.uint8))
            self.register_buffer("step_counter", torch.zeros(16, 2, dtype=torch.int32))
            self.mean_density = 0
            self.iter_density = 0
            self.mean_count = 0
            self.local_step = 0
        self._frames = {}              # frame workspaces: slot -> (pn_frame handle, what it was sized for)
        self._aabb_cache = (None, None)   # _aabb_infer_host: (the buffer's address and version, its six floats)
        self._static_depth_0 = {}      # slot -> the un-normalised depth of the static frame last rendered there: run_cuda returns the reference's three
                                       # tensors, and a continuation composites on into this fourth
        self.last_stats = None
        self._overlay = None   # set_collider_overlay: a ColliderOverlay
        self._shadows = None   # set_collider_shadows: a ColliderShadows
        self._points = None    # set_point_overlay: a PointOverlay
        self._point_keys = {}  # ... and its key buffers, one per frame workspace

    def forward(self, x, d):
        raise NotImplementedError()

    def density(self, x):
        raise NotImplementedError()

    def color(self, x, d, mask=None, **kwargs):
        raise NotImplementedError()

    def _net_handle(self, half=False):
        raise NotImplementedError()

    def background(self, x, d):
        raise NotImplementedError()

    def blend_background(self, rays_o, rays_d, weights_sum, image):
        raise NotImplementedError()

    @staticmethod
    def _autocast_half():
        return False

    def _refuse_overlays(self, what):
        """Every render form but the deformed frame driver raises while an overlay is set; with both, the colliders' message."""
        for rec, name, drawn in ((self._overlay, "collider", "colliders"), (self._points, "point", "points")):
            if rec is not None:
                raise RuntimeError(f"{name} overlay: {what} does not draw the {drawn} — only the deformed path does (render_deformed / rund_cuda without "
                                   f"perturb, and render_continue); clear_{name}_overlay() first")

    # ------------------------------------------------------------------ entry point (renderer.py:587-599)
    def render_deformed(self, rays_o, rays_d, staged=False, max_ray_batch=4096, **kwargs):
        """renderer.py:587-599.  `staged` / `max_ray_batch` are accepted and unused exactly as in the reference, whose render_deformed calls
        rund_cuda on the whole ray set whatever they say (only the non-cuda_ray `render` stages, :562-576)."""
        if not self.cuda_ray:
            # the reference's `rund` (:602-753) is run() with a host-synchronising print and positions handed over as view directions, and it applies no
            # deformation at all: a debugging stub, not a renderer to reproduce
            raise RuntimeError("render_deformed: only the cuda_ray path (main_gui.py / main_render.py with -O) is implemented")
        return self.rund_cuda(rays_o, rays_d, **kwargs)

    def _ip_state(self, device):
        return [t.to(device=device, dtype=torch.float32).contiguous() for t in (self.p_def, self.p_ori, self.IP_F, self.IP_dF)]

    def _frame_handle(self, N, n_vtx, hgs, slot=0, cells=None):
        """Per-frame workspace (pn_frame).  `slot` selects one of several independent workspaces so that frames can be in
        flight concurrently on different streams (harness.capture_pipelined)."""
        # spatial-hash capacity: the IP cloud lives inside the simulation box (2.04*bound per side, solver.py:24-32); x2 margin per axis
        side = int(math.ceil(2.2 * float(self.bound) / hgs)) + 2
        cells = side ** 3 if cells is None else int(cells)
        key = (N, n_vtx, cells)
        cur = self._frames.get(slot)
        if cur is None or cur[1] != key:
            if cur is not None:
                lib().pn_frame_destroy(cur[0])
            h = C.c_void_p()
            check(lib().pn_frame_create(C.byref(h), N, n_vtx, cells), "frame_create")
            self._frames[slot] = (h, key)
        return self._frames[slot][0]

    # ------------------------------------------------------------------ fused loop
    def _static_opts(self, dt_gamma, bg_scalar, max_steps, T_thresh):
        """The option set of the static render (pn_render_static, and pn_render_continue on a static frame): no IP state, no ray groups, no fused launch.
        _deformed_opts starts from it."""
        o = RenderOpts()
        o.max_iter_num, o.hash_grid_size, o.num_seek_IP, o.IP_dx, o.cut = 1, 1.0, 1, 0.0, 0
        o.bound, o.min_near, o.dt_gamma, o.max_steps, o.T_thresh = float(self.bound), float(self.min_near), float(dt_gamma), int(max_steps), float(T_thresh)
        o.cascade, o.grid_size, o.density_scale, o.bg_color = int(self.cascade), int(self.grid_size), float(self.density_scale), float(bg_scalar)
        o.fp16 = int(self._autocast_half())  # Trainer.test_gui renders under autocast(enabled=self.fp16) (trainer.py:561)
        return o

    def _deformed_opts(self, dt_gamma, bg_scalar, max_steps, T_thresh, kwargs, n_rays=0):
        o = self._static_opts(dt_gamma, bg_scalar, max_steps, T_thresh)
        o.max_iter_num = int(kwargs.get("max_iter_num"))
        o.hash_grid_size = float(kwargs.get("hash_grid_size"))
        o.num_seek_IP = int(kwargs.get("num_seek_IP"))
        o.IP_dx = float(self.IP_dx)
        o.cut = int(bool(kwargs.get("cut")))
        cb = kwargs.get("cut_bounds") or [0.0] * 6
        for i in range(6):
            o.cut_bounds[i] = float(cb[i])
        o.bound = float(kwargs.get("bound", self.bound))
        o.reuse_tables = int(bool(kwargs.get("reuse_tables")))  # extension: later ray batches of the same frame keep the first batch's tables
        o.ray_batch = int(kwargs.get("ray_batch") or 0)  # extension: per-batch trip schedules inside one set of launches (pn_render_opts.ray_batch)
        o.throughput = int(kwargs.get("march_throughput") or 0)  # extension: one lane per ray in the first trip's pass 1 (pn_render_opts.throughput)
        o.throughput_trips = int(kwargs.get("march_throughput_trips") or 0)  # ... and in this many leading trips (0: the first only)
        # extension: walk a whole image's rays in 16 x 4 pixel tiles (pn_render_opts.ray_tile_w; results do not depend on it).  The reference hands
        # **vars(opt) to the renderer (trainer.py:318), so W / H arrive by name; only a ray set of exactly W * H rays is taken for the image
        tw = kwargs.get("ray_tile_w")
        if tw is None and n_rays and kwargs.get("W") and kwargs.get("H") and int(kwargs["W"]) * int(kwargs["H"]) == n_rays:
            tw = kwargs["W"]
        o.ray_tile_w = int(tw or 0)
        o.fused_from = int(kwargs.get("fused_from") or 0)  # extension: first loop trip of the one-launch form (pn_render_opts.fused_from; 0: trip 1, < 0: never)
        o.fused_grid = int(kwargs.get("fused_grid") or 0)  # extension: workgroups of that launch (pn_render_opts.fused_grid; 0: one per CU)
        o.fused_fold = int(bool(kwargs.get("fused_fold")))  # extension: ... the first trip's network + composite + compaction folded in (pn_render_opts.fused_fold)
        o.fused_whole = int(bool(kwargs.get("fused_whole")))  # extension: ... the frame's first trip included, where it applies (pn_render_opts.fused_whole)
        fo = kwargs.get("fused_order")
        o.fused_order = 0 if (fo is None or fo) else -1  # extension: ... a workgroup draws its longest packets first (pn_render_opts.fused_order; False: list order)
        return o

    def rund_cuda(self, rays_o, rays_d, dt_gamma=0, bg_color=None, perturb=False, max_steps=1024, T_thresh=1e-2, _shadow_pass=False, **kwargs):
        """The deformed frame in one C call (see the module's docstring).  `_shadow_pass`: this call IS the shadow pass (overlay_colliders.py): the
        object alone over 0, no overlay, no background."""
        if perturb:
            self._refuse_overlays("the op-by-op loop (perturb=True)")
            return self.rund_cuda_ops(rays_o, rays_d, dt_gamma, bg_color, perturb, max_steps, T_thresh, **kwargs)
        prefix = rays_o.shape[:-1]
        rays_o, rays_d = flat_rays(rays_o, rays_d)
        require_gpu(rays_o, rays_d)
        N, device = rays_o.shape[0], rays_o.device
        overlay = self._overlay is not None and not _shadow_pass
        bg_driver, bg_colliders, bg_tensor = frame_background(bg_color, self.bg_radius, overlay)
        if bg_tensor is not None:
            bg_tensor = bg_tensor.to(device=device, dtype=torch.float32)
        p_def, p_ori, F_IP, dF_IP = self._ip_state(device)
        assert p_def.shape == p_ori.shape and p_ori.shape[0] > 0  # renderer.py:816-817
        n_vtx = p_ori.shape[0]
        if overlay and self._shadows is not None:
            self._render_shadow_map(dt_gamma, max_steps, T_thresh, kwargs)
        o = self._deformed_opts(dt_gamma, bg_driver, max_steps, T_thresh, kwargs, n_rays=N)
        ob = kwargs.get("out_buffers")  # extension: caller-owned outputs (the frame pipeline packs image | depth | depth_0 into one buffer -> one D2H)
        image, depth, depth_0, weights_sum = frame_outputs(N, device, ob)
        async_trips, slot = int(kwargs.get("async_trips") or 0), int(kwargs.get("frame_slot") or 0)
        frame, net = self._frame_handle(N, n_vtx, o.hash_grid_size, slot), self._net_handle(half=bool(o.fp16))
        args = (frame, net, C.byref(o), ptr(rays_o), ptr(rays_d), N, ptr(p_def), ptr(p_ori), ptr(F_IP), ptr(dF_IP), n_vtx, ptr(self.density_bitfield), ptr(image),
                ptr(depth), ptr(depth_0), ptr(weights_sum))
        if async_trips > 0:
            # non-blocking: a fixed number of trips, no host synchronisation (legal under HIP-graph capture); completion is
            # checked later with render_status(), a frame that ran out of trips is finished with render_continue()
            check(lib().pn_render_deformed_async(*args, async_trips, stream_ptr()), "render_deformed_async")
        else:
            stats = (C.c_int64 * 5)() if kwargs.get("collect_stats") else None
            check(lib().pn_render_deformed(*args, stats, stream_ptr()), "render_deformed")
            if stats is not None:
                self._set_stats(stats)
        res = {"depth": depth.view(*prefix), "depth_0": depth_0.view(*prefix), "weights_sum": weights_sum}
        image = self._finish_frame(rays_o, rays_d, (bg_colliders, bg_tensor), weights_sum, depth_0, image, res, ob, slot, kwargs.get("point_pose"),
                                   shadow_pass=_shadow_pass)
        res["image"] = image.view(*prefix, 3)
        return res

    def _finish_frame(self, rays_o, rays_d, bg, weights_sum, depth_0, image, res, ob, slot, point_pose, shadow_pass=False, static=False):
        """What stands behind the frame driver, enqueued on the current stream in this order: the colliders' launch, the background, the points' launch
        pair.  `bg`: frame_background's (collider launch's scalar, tensor or None); `image` holds the driver's frame, composited over 0 wherever a layer
        follows.  The layers' named outputs go to `res`, into its own tensors of those names, else the caller's `ob` (out_buffers or None), else new
        ones.  A shadow pass (`shadow_pass`) gets no layer; a `static` frame has no integration points to draw.  Returns the image: `image` itself,
        finished in place, except behind a tensor background."""
        bg_colliders, bg_tensor = bg
        covered, collider_t = weights_sum, None   # what the background is blended with: the object's own opacity, or with an overlay the object's and the colliders'
        if self._overlay is not None and not shadow_pass:
            covered, collider_t = self._draw_colliders(rays_o, rays_d, bg_colliders, weights_sum, depth_0, image, res, ob)
        if self.bg_radius > 0 and not shadow_pass:
            self.blend_background(rays_o, rays_d, covered, image)   # in place: `image` may be the caller's out_buffers
        elif bg_tensor is not None:
            image = image + (1 - covered).unsqueeze(-1) * bg_tensor
        if self._points is not None and not shadow_pass and not static:   # last: the points and the drag handle, painted onto the finished picture
            p_def, _, F_IP, _ = self._ip_state(image.device)
            self._draw_points(p_def, F_IP, weights_sum, depth_0, collider_t, image, res, ob, slot, point_pose)
        return image

    def render_continue(self, slot, rays_o, rays_d, out, n_trips=0, dt_gamma=0, bg_color=None, max_steps=1024, T_thresh=1e-2, static=False,
                        _shadow_pass=False, **kwargs):
        """Finishes the frame last rendered on workspace `slot` with a fixed trip count that turned out too small (render_status reports
        rays alive at exit): more trips of the same loop — n_trips of them, or (0) until no ray is alive — and the epilogue again, into the
        SAME output tensors `out` (the dict the render returned).  The reference's loop has no trip limit but max_steps (renderer.py:836-891);
        this is how the captured, fixed-length forms keep that semantics.  Blocking when n_trips == 0.  With a background model the epilogue
        composites over 0 again and the model's colour is blended in again, once.  `bg_color` is None or something float() takes: this entry
        has no tensor background."""
        rays_o, rays_d = flat_rays(rays_o, rays_d)
        N = rays_o.shape[0]
        if static:
            self._refuse_overlays("the static render (render_continue with static=True)")
        overlay = self._overlay is not None and not _shadow_pass
        if torch.is_tensor(bg_color) and not self.bg_radius > 0:
            bg_color = float(bg_color)
        bg_driver, bg_colliders, _ = frame_background(bg_color, self.bg_radius, overlay)
        if overlay and self._shadows is not None:
            self._continue_shadow_map(n_trips, dt_gamma, max_steps, T_thresh, kwargs)
        # with an overlay the epilogue rewrites `image` from the driver's accumulator over 0 and the layers are applied once more, below
        o = self._static_opts(dt_gamma, bg_driver, max_steps, T_thresh) if static else self._deformed_opts(dt_gamma, bg_driver, max_steps, T_thresh, kwargs, n_rays=N)
        image, depth, ws = out["image"].view(-1, 3), out["depth"].view(-1), out["weights_sum"].view(-1)
        if "depth_0" in out:
            depth_0 = out["depth_0"].view(-1)
        elif static:   # the accumulator the composite goes on adding to: the frame's own, never a new tensor
            depth_0 = self._static_depth_0.get(slot)
            if depth_0 is None or depth_0.shape != depth.shape or depth_0.device != depth.device:
                raise RuntimeError(f"render_continue: no static frame of {N} rays was rendered on frame workspace {slot}")
        else:
            depth_0 = torch.empty_like(depth)
        assert image.is_contiguous() and image.shape[0] == N
        stats = (C.c_int64 * 5)() if int(n_trips) == 0 else None
        check(lib().pn_render_continue(self._frames[slot][0], self._net_handle(half=bool(o.fp16)), C.byref(o), ptr(rays_o), ptr(rays_d), N,
                                       ptr(self.density_bitfield), ptr(image), ptr(depth), ptr(depth_0), ptr(ws), stats, int(n_trips), int(bool(static)),
                                       stream_ptr()), "render_continue")
        if "depth_0" not in out and not _shadow_pass:
            if overlay:
                raise RuntimeError("render_continue: the collider overlay composites against depth_0: pass the dict the deformed render returned")
            if self._points is not None and not static:
                raise RuntimeError("render_continue: the point overlay tests against depth_0: pass the dict the deformed render returned")
        # the points are painted from the state the frame was rendered from (the key buffer cleaned itself)
        self._finish_frame(rays_o, rays_d, (bg_colliders, None), ws, depth_0, image, out, None, slot, kwargs.get("point_pose"), shadow_pass=_shadow_pass, static=static)
        if stats is not None:
            self._set_stats(stats)
        return out

    def _set_stats(self, stats):
        self.last_stats = dict(trips=int(stats[0]), samples=int(stats[1]), err=int(stats[2]), alive_at_exit=int(stats[3]), unfinished=int(stats[4]))
        if stats[2]:
            raise RuntimeError(f"render_deformed: device error flags {int(stats[2])} (1: sample cell outside the spatial hash, "
                               "2: IP outside it, 4: spatial-hash capacity exceeded, 8: candidate-list capacity exceeded, "
                               "16: the fused composite/compaction gave up waiting for an earlier chunk, 32: the fused launch found its kernarg segment laid "
                               "out otherwise than csrc/pn_trips_fused.h: fused_karg_fresh assumes)")

    def render_status(self, synchronize=True, slot=0):
        """Outcome of the last render on frame workspace `slot`: dict(trips, samples, err, alive_at_exit).
        After an async render, alive_at_exit > 0 means the enqueued trips were not enough — or, on a static frame (run_cuda), that max_steps
        ended the loop with that many rays alive, as run_cuda_ops reports it; render_continue leaves such a frame as it is."""
        stats = (C.c_int64 * 5)()
        check(lib().pn_render_status(self._frames[slot][0], stats, int(bool(synchronize)), stream_ptr()), "render_status")
        self._set_stats(stats)
        return self.last_stats
