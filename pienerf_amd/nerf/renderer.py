"""Deformed-space renderer with the reference's surface (nerf/renderer.py:74-113, 587-599, 755-907).

``NeRFRenderer.render_deformed(rays_o, rays_d, **vars(opt))`` is what ``Trainer.test_step`` calls
(nerf/trainer.py:316-318); the caller sets ``p_ori, p_def, IP_F, IP_dF, IP_dx`` on the model
(main_gui.py:52-56, trainer.py:303-306).  Two implementations of ``rund_cuda`` are provided:

  * ``rund_cuda``      — one C call (pn_render_deformed): the whole loop runs on the GPU with a device-side
                         (n_alive, n_step) record; no per-trip host synchronisation.
  * ``rund_cuda_ops``  — the reference's Python loop verbatim in structure, on the drop-in ops
                         (near_far_from_aabb / get_pnts_in_grids / march_rays_quadratic_bending / network /
                         composite_rays / compaction).  Used by the parity tests and as documentation of semantics.
"""
import ctypes as C
import math

import torch
import torch.nn as nn

from .. import raymarching
from .._lib import ColliderStyle, PointStyle, RenderOpts, ShadowLight, check, lib, ptr, require_gpu, stream_ptr
from .utils import get_pnts_in_grids


def _flat_rays(rays_o, rays_d):
    """The rays as the frame drivers take them: [N, 3], fp32, contiguous."""
    return rays_o.to(torch.float32).contiguous().view(-1, 3), rays_d.to(torch.float32).contiguous().view(-1, 3)


def sample_pdf(bins, weights, n_samples, det=False):
    """nerf/renderer.py:19-53 (the original NeRF's inverse-CDF sampling), torch ops on whatever device the inputs live on.
    bins [B, T] (the old z values), weights [B, T - 1] (bin weights) -> [B, n_samples] new z values; det: the midpoints of n_samples equal
    slices of [0, 1] instead of uniform random numbers."""
    if weights.shape[-1] < 1:
        raise RuntimeError("sample_pdf: no bin weights (the hierarchical sampler needs num_steps >= 3: weights[:, 1:-1] is empty)")
    weights = weights + 1e-5  # prevent nans
    pdf = weights / torch.sum(weights, -1, keepdim=True)
    cdf = torch.cumsum(pdf, -1)
    cdf = torch.cat([torch.zeros_like(cdf[..., :1]), cdf], -1)
    if det:
        u = torch.linspace(0. + 0.5 / n_samples, 1. - 0.5 / n_samples, steps=n_samples).to(weights.device)
        u = u.expand(list(cdf.shape[:-1]) + [n_samples])
    else:
        u = torch.rand(list(cdf.shape[:-1]) + [n_samples]).to(weights.device)
    u = u.contiguous()
    inds = torch.searchsorted(cdf, u, right=True)
    below = torch.clamp(inds - 1, min=0)
    above = torch.clamp(inds, max=cdf.shape[-1] - 1)
    cdf_lo, cdf_hi = torch.gather(cdf, -1, below), torch.gather(cdf, -1, above)
    bins_lo, bins_hi = torch.gather(bins, -1, below), torch.gather(bins, -1, above)
    denom = cdf_hi - cdf_lo
    denom = torch.where(denom < 1e-5, torch.ones_like(denom), denom)
    t = (u - cdf_lo) / denom
    return bins_lo + t * (bins_hi - bins_lo)


class NeRFRenderer(nn.Module):
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
        self._frame = None
        self._frames = {}
        self.last_stats = None
        self._overlay = None   # set_collider_overlay: (contact state on the device, ColliderStyle, t_max)
        self._shadows = None   # set_collider_shadows: the light, its rays and the map buffers
        self._points = None    # set_point_overlay: the camera, the style and what else the point overlay's launch pair reads
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

    # ------------------------------------------------------------------ the contact colliders drawn into the frame (csrc/pn_colliders.hip)
    def set_collider_overlay(self, state, style=None, t_max=None):
        """From now on rund_cuda (render_deformed) and render_continue draw the colliders of `state` into the frame: one launch behind the frame driver
        (pn_draw_colliders; include/pienerf_hip.h has the law) composites them with a depth test against the object.  `state` is a device tensor of 93
        doubles with the pn_contact_state layout — Simulator.collider_state() or a copy — read on the device at execution time, so a captured render
        follows set_collider without a recapture.  `style`: a ColliderStyle (pienerf_amd.colliders.collider_style; None: its defaults), baked into a
        captured launch: changing it needs a recapture.  `t_max` (None: 8 * bound): the far end of the colliders, in units of rays_d; they fade into
        the background over its second half.  The returned dict gains 'coverage' and 'collider_t'; 'weights_sum', 'depth' and 'depth_0' stay the
        object's own.  The static and hierarchical renders and the op-by-op loop raise while an overlay is set."""
        from ..colliders import collider_style
        if not (torch.is_tensor(state) and state.dtype == torch.float64 and state.numel() == 93 and state.is_contiguous()):
            raise ValueError("set_collider_overlay: `state` is a contiguous tensor of 93 doubles (pn_contact_state; Simulator.collider_state())")
        require_gpu(state)
        style = collider_style() if style is None else style
        if not isinstance(style, ColliderStyle):
            raise ValueError("set_collider_overlay: `style` is a ColliderStyle (pienerf_amd.colliders.collider_style)")
        t_max = 8.0 * float(self.bound) if t_max is None else float(t_max)
        if not (math.isfinite(t_max) and t_max > float(self.min_near)):
            raise ValueError(f"set_collider_overlay: t_max must be a finite number above min_near = {self.min_near}, got {t_max!r}")
        self._overlay = (state, style, t_max)
        return self

    def clear_collider_overlay(self):
        self._overlay = None
        self._shadows = None

    def collider_overlay_key(self):
        """What a captured render bakes in of the overlay (None without one): the state's address, the style's bytes, t_max — and with shadows set the
        light's bytes and the map buffers' addresses."""
        if self._overlay is None:
            return None
        state, style, t_max = self._overlay
        key = (state.data_ptr(), bytes(style), t_max)
        if self._shadows is not None:
            sh = self._shadows
            key += (bytes(sh["light"]), sh["shadow_ws"].data_ptr(), sh["shadow_depth_0"].data_ptr())
        return key

    # ------------------------------------------------------------------ the object's shadow on the drawn colliders
    SHADOW_SLOT = 900   # the shadow pass's frame workspace: the pipeline's lanes use 0 .. lanes * depth - 1, the tile-parallel form 800

    def set_collider_shadows(self, light):
        """From now on the deformed render first renders the object along `light`'s parallel rays (a ShadowLight: pienerf_amd.colliders.shadow_light)
        into an opacity map — the existing render on the frame workspace SHADOW_SLOT, same IP state, options and async_trips, no overlay and no
        background — and the overlay's launch looks the map up while it draws (pn_draw_colliders_shadowed; include/pienerf_hip.h has the law).  The
        renderer owns the light rays and the map buffers `shadow_ws` / `shadow_depth_0` [S^2]; their addresses stay until the next call.  The returned
        dict gains 'shadow' [N]: the occlusion per camera ray, 0 where no collider is seen.  The light is baked into a captured launch like the style.
        RuntimeError without a collider overlay."""
        from ..colliders import shadow_rays
        if self._overlay is None:
            raise RuntimeError("set_collider_shadows: the shadows fall on the drawn colliders: set_collider_overlay() first")
        if not isinstance(light, ShadowLight):
            raise ValueError("set_collider_shadows: `light` is a ShadowLight (pienerf_amd.colliders.shadow_light)")
        dev = self._overlay[0].device
        rays_o, rays_d = shadow_rays(light, dev)
        n = rays_o.shape[0]
        buf = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)   # noqa: E731
        self._shadows = {"light": light, "rays_o": rays_o, "rays_d": rays_d, "shadow_ws": buf(n), "shadow_depth_0": buf(n), "image": buf(n, 3), "depth": buf(n)}
        return self

    def clear_collider_shadows(self):
        self._shadows = None

    @property
    def shadow_ws(self):
        return self._shadows["shadow_ws"] if self._shadows is not None else None

    @property
    def shadow_depth_0(self):
        return self._shadows["shadow_depth_0"] if self._shadows is not None else None

    def _shadow_out(self):
        sh = self._shadows
        return {"image": sh["image"], "depth": sh["depth"], "depth_0": sh["shadow_depth_0"], "weights_sum": sh["shadow_ws"]}

    def _render_shadow_map(self, dt_gamma, max_steps, T_thresh, kwargs):
        """The shadow pass, on the current stream in front of the camera's render.  ray_tile_w is set explicitly: S^2 == W H must not select the image
        tiling by accident (results do not depend on it).  last_stats stays the main frame's; the pass's own are read with render_status(slot=SHADOW_SLOT)."""
        sh = self._shadows
        kw = dict(kwargs, frame_slot=self.SHADOW_SLOT, out_buffers=self._shadow_out(), ray_tile_w=0, _shadow_pass=True)
        keep = self.last_stats
        try:
            self.rund_cuda(sh["rays_o"], sh["rays_d"], dt_gamma=dt_gamma, bg_color=0, perturb=False, max_steps=max_steps, T_thresh=T_thresh, **kw)
        finally:
            self.last_stats = keep

    def _refuse_overlay(self, what):
        if self._overlay is not None:
            raise RuntimeError(f"collider overlay: {what} does not draw the colliders — only the deformed path does (render_deformed / rund_cuda without "
                               "perturb, and render_continue); clear_collider_overlay() first")

    def _draw_colliders(self, rays_o, rays_d, bg_scalar, weights_sum, depth_0, image, out, ob=None):
        """Enqueues the overlay's launch on the current stream, in place in `image` (the frame composited over 0); 'coverage' and 'collider_t' of `out`
        (then of `ob`, else allocated) receive its other outputs, and with shadows 'shadow'.  Returns [coverage, collider_t] or [coverage, collider_t, shadow]."""
        state, style, t_max = self._overlay
        N = image.shape[0]
        res = []
        sh = self._shadows
        for name in ("coverage", "collider_t") + (("shadow",) if sh is not None else ()):
            t = out.get(name) if out is not None else None
            if t is None and ob is not None:
                t = ob.get(name)
            if t is None:
                t = torch.empty(N, dtype=torch.float32, device=image.device)
            assert t.shape == (N,) and t.dtype == torch.float32 and t.is_contiguous()
            res.append(t)
        if sh is not None:
            check(lib().pn_draw_colliders_shadowed(ptr(state), C.byref(style), ptr(rays_o), ptr(rays_d), N, float(self.min_near), t_max, float(bg_scalar),
                                                   ptr(weights_sum), ptr(depth_0), ptr(image), ptr(res[0]), ptr(res[1]), sh["light"], ptr(sh["shadow_ws"]),
                                                   ptr(sh["shadow_depth_0"]), ptr(res[2]), stream_ptr()), "draw_colliders_shadowed")
        else:
            check(lib().pn_draw_colliders(ptr(state), C.byref(style), ptr(rays_o), ptr(rays_d), N, float(self.min_near), t_max, float(bg_scalar),
                                          ptr(weights_sum), ptr(depth_0), ptr(image), ptr(res[0]), ptr(res[1]), stream_ptr()), "draw_colliders")
        return res

    # ------------------------------------------------------------------ the integration points and the drag handle drawn into the frame
    def set_point_overlay(self, pose_dev, intrinsics, W, H, style=None, source="ip", values=None, drag_state=None):
        """From now on rund_cuda (render_deformed) and render_continue draw the frame's integration points into the finished picture: a launch pair
        (pn_draw_points; include/pienerf_hip.h has the law) LAST on the deformed path, behind the colliders' launch and the background's blend, with the
        colliders' collider_t in its depth test when a collider overlay is set.  `source` 'ip': the positions and deformation gradients are the frame's
        own p_def / IP_F, so a pipelined frame draws the state it was rendered from.  `pose_dev`: the camera's c2w matrix as a device tensor of 16
        floats, read at execution time (a captured render follows it); None: every render passes its own as the keyword `point_pose` (the harness's
        forms do: each pipeline workspace keeps a pose of its own).  `intrinsics` = (fx, fy, cx, cy) and `W`, `H`: the frame's; a render needs
        N == W H rays.  `style`: a PointStyle (pienerf_amd.points_overlay.point_style; None: its defaults), baked into a captured launch like the
        intrinsics.  `values`: a device tensor [n] fp32 for the mode 'values'.  `drag_state`: the simulator's device pn_drag_state (5 doubles) — the
        launch then draws the drag handle while the drag is active.  The returned dict gains 'point_id' [N] int32 (the drawn point per pixel, -1:
        none) and 'point_t' [N].  The static, hierarchical and op-by-op renders raise while it is set."""
        from ..points_overlay import mode_name, point_style
        style = point_style() if style is None else style
        if not isinstance(style, PointStyle):
            raise ValueError("set_point_overlay: `style` is a PointStyle (pienerf_amd.points_overlay.point_style)")
        if source != "ip":
            raise ValueError(f"set_point_overlay: source must be 'ip' (the frame's integration points), got {source!r}")
        W, H = int(W), int(H)
        intr = tuple(float(v) for v in intrinsics)
        if W <= 0 or H <= 0 or len(intr) != 4 or not all(math.isfinite(v) for v in intr):
            raise ValueError("set_point_overlay: W, H > 0 and four finite intrinsics (fx, fy, cx, cy)")
        if pose_dev is not None:
            self._check_point_pose(pose_dev)
        if mode_name(style) == "values":
            if not (torch.is_tensor(values) and values.dtype == torch.float32 and values.dim() == 1 and values.is_contiguous()):
                raise ValueError("set_point_overlay: the mode 'values' needs `values`, a contiguous fp32 tensor [n] on the GPU")
            require_gpu(values)
        elif values is not None:
            raise ValueError("set_point_overlay: `values` goes with the mode 'values'")
        if drag_state is not None:
            if not (torch.is_tensor(drag_state) and drag_state.dtype == torch.float64 and drag_state.numel() == 5 and drag_state.is_contiguous()):
                raise ValueError("set_point_overlay: `drag_state` is a contiguous tensor of 5 doubles (pn_drag_state; the simulator's own)")
            require_gpu(drag_state)
        self._points = {"pose": pose_dev, "intr": intr, "intr_c": (C.c_float * 4)(*intr), "W": W, "H": H, "style": style, "values": values,
                        "drag": drag_state}
        return self

    @staticmethod
    def _check_point_pose(pose):
        if not (torch.is_tensor(pose) and pose.dtype == torch.float32 and pose.numel() == 16 and pose.is_contiguous()):
            raise ValueError("point overlay: the pose is a contiguous fp32 tensor of 16 values (c2w, row-major) on the GPU")
        require_gpu(pose)

    def clear_point_overlay(self):
        self._points = None

    def point_overlay_key(self):
        """What a captured render bakes in of the point overlay (None without one): the intrinsics, W, H, the style's bytes and the addresses of the
        default pose, the values and the drag state."""
        if self._points is None:
            return None
        p = self._points
        adr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        return (adr(p["pose"]), p["intr"], p["W"], p["H"], bytes(p["style"]), adr(p["values"]), adr(p["drag"]))

    def point_overlay_reads_drag(self):
        """Whether the launch pair reads a drag state: the caller then orders the render behind the stream that writes it."""
        return self._points is not None and self._points["drag"] is not None

    def _refuse_point_overlay(self, what):
        if self._points is not None:
            raise RuntimeError(f"point overlay: {what} does not draw the points — only the deformed path does (render_deformed / rund_cuda without "
                               "perturb, and render_continue); clear_point_overlay() first")

    def _point_key_buffer(self, slot, device):
        """The key buffer of frame workspace `slot` (lanes run concurrently: one each), allocated and filled outside any capture."""
        from ..points_overlay import key_buffer
        p = self._points
        cur = self._point_keys.get(slot)
        if cur is None or cur.numel() != p["W"] * p["H"] or cur.device != device:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"point overlay: the key buffer of frame workspace {slot} must exist before a capture: render one frame on it first")
            cur = self._point_keys[slot] = key_buffer(p["W"], p["H"], device)
        return cur

    def _draw_points(self, p_def, F_IP, weights_sum, depth_0, collider_t, image, out, ob, kwargs):
        """Enqueues the point overlay's launch pair on the current stream, in place in `image` (the finished picture); 'point_id' and 'point_t' of `out`
        (then of `ob`, else allocated) receive its other outputs.  Returns (point_id, point_t)."""
        p = self._points
        N = image.shape[0]
        if N != p["W"] * p["H"]:
            raise RuntimeError(f"point overlay: set for a {p['W']} x {p['H']} frame, this render has {N} rays (it needs N == W H: the whole image)")
        pose = kwargs.get("point_pose")
        pose = p["pose"] if pose is None else pose
        if pose is None:
            raise RuntimeError("point overlay: set_point_overlay() got no pose_dev: pass this render's camera as point_pose=")
        self._check_point_pose(pose)
        n = p_def.shape[0]
        if p["values"] is not None and p["values"].shape[0] != n:
            raise RuntimeError(f"point overlay: `values` has {p['values'].shape[0]} entries, the frame {n} integration points")
        assert F_IP.shape[0] == n and F_IP.is_contiguous() and image.is_contiguous()
        res = []
        for name, dtype in (("point_id", torch.int32), ("point_t", torch.float32)):
            t = out.get(name) if out is not None else None
            if t is None and ob is not None:
                t = ob.get(name)
            if t is None:
                t = torch.empty(N, dtype=dtype, device=image.device)
            assert t.shape == (N,) and t.dtype == dtype and t.is_contiguous()
            res.append(t)
        keys = self._point_key_buffer(int(kwargs.get("frame_slot") or 0), image.device)
        check(lib().pn_draw_points(ptr(p_def), ptr(F_IP), ptr(p["values"]), n, ptr(pose), p["intr_c"], p["W"], p["H"], float(self.min_near),
                                   ptr(weights_sum), ptr(depth_0), ptr(collider_t), ptr(p["drag"]), ptr(keys), p["style"], ptr(image), ptr(res[0]),
                                   ptr(res[1]), stream_ptr()), "draw_points")
        return res

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
        if slot == 0:
            self._frame = self._frames[0][0]
        return self._frames[slot][0]

    # ------------------------------------------------------------------ fused loop
    def _deformed_opts(self, dt_gamma, bg_scalar, max_steps, T_thresh, kwargs, n_rays=0):
        o = RenderOpts()
        o.max_iter_num = int(kwargs.get("max_iter_num"))
        o.hash_grid_size = float(kwargs.get("hash_grid_size"))
        o.num_seek_IP = int(kwargs.get("num_seek_IP"))
        o.IP_dx = float(self.IP_dx)
        o.cut = int(bool(kwargs.get("cut")))
        cb = kwargs.get("cut_bounds") or [0.0] * 6
        for i in range(6):
            o.cut_bounds[i] = float(cb[i])
        o.bound = float(kwargs.get("bound", self.bound))
        o.min_near = float(self.min_near)
        o.dt_gamma = float(dt_gamma)
        o.max_steps = int(max_steps)
        o.T_thresh = float(T_thresh)
        o.cascade = int(self.cascade)
        o.grid_size = int(self.grid_size)
        o.density_scale = float(self.density_scale)
        o.bg_color = float(bg_scalar)
        o.fp16 = int(self._autocast_half())  # Trainer.test_gui renders under autocast(enabled=self.fp16) (trainer.py:561)
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

    def _static_opts(self, dt_gamma, bg_scalar, max_steps, T_thresh):
        """The option set of the static render (pn_render_static, and pn_render_continue on a static frame): no IP state, no ray groups, no fused launch."""
        o = RenderOpts()
        o.max_iter_num, o.hash_grid_size, o.num_seek_IP, o.IP_dx, o.cut = 1, 1.0, 1, 0.0, 0
        o.bound, o.min_near, o.dt_gamma, o.max_steps, o.T_thresh = float(self.bound), float(self.min_near), float(dt_gamma), int(max_steps), float(T_thresh)
        o.cascade, o.grid_size, o.density_scale, o.bg_color = int(self.cascade), int(self.grid_size), float(self.density_scale), float(bg_scalar)
        o.fp16 = int(self._autocast_half())
        return o

    def rund_cuda(self, rays_o, rays_d, dt_gamma=0, bg_color=None, perturb=False, max_steps=1024, T_thresh=1e-2, **kwargs):
        if perturb:
            self._refuse_overlay("the op-by-op loop (perturb=True)")
            self._refuse_point_overlay("the op-by-op loop (perturb=True)")
            return self.rund_cuda_ops(rays_o, rays_d, dt_gamma, bg_color, perturb, max_steps, T_thresh, **kwargs)
        prefix = rays_o.shape[:-1]
        rays_o, rays_d = _flat_rays(rays_o, rays_d)
        require_gpu(rays_o, rays_d)
        N, device = rays_o.shape[0], rays_o.device
        if self.bg_radius > 0:
            bg_color = 0   # the model's colour replaces whatever was passed (renderer.py:799-803): composite over 0, blend below
        if bg_color is None:
            bg_color = 1
        # a tensor background ([3] or [N,3], e.g. the GUI's bg_color tensor, gui.py:590): the driver composites over 0 and the blend
        # image + (1 - weights_sum) * bg (renderer.py:896) is applied afterwards with the same two roundings
        bg_tensor = bg_color.to(device=device, dtype=torch.float32) if torch.is_tensor(bg_color) else None
        p_def, p_ori, F_IP, dF_IP = self._ip_state(device)
        assert p_def.shape == p_ori.shape and p_ori.shape[0] > 0  # renderer.py:816-817
        n_vtx = p_ori.shape[0]
        shadow_pass = bool(kwargs.get("_shadow_pass"))   # this call IS the shadow pass: the object alone over 0, no overlay, no background
        overlay = self._overlay is not None and not shadow_pass
        if overlay and self._shadows is not None:
            self._render_shadow_map(dt_gamma, max_steps, T_thresh, kwargs)
        # with an overlay the driver composites over 0 as well: the scalar background goes in behind the colliders, in the overlay's launch
        o = self._deformed_opts(dt_gamma, 0.0 if (bg_tensor is not None or overlay) else bg_color, max_steps, T_thresh, kwargs, n_rays=N)
        ob = kwargs.get("out_buffers")  # extension: caller-owned outputs (the frame pipeline packs image | depth | depth_0 into one buffer -> one D2H)
        if ob is not None:
            image, depth, depth_0, weights_sum = ob["image"], ob["depth"], ob["depth_0"], ob["weights_sum"]
            assert image.shape == (N, 3) and depth.shape == (N,) and all(t.is_contiguous() and t.dtype == torch.float32 for t in (image, depth, depth_0, weights_sum))
        else:
            image = torch.empty(N, 3, dtype=torch.float32, device=device)
            depth = torch.empty(N, dtype=torch.float32, device=device)
            depth_0 = torch.empty(N, dtype=torch.float32, device=device)
            weights_sum = torch.empty(N, dtype=torch.float32, device=device)
        async_trips = int(kwargs.get("async_trips") or 0)
        frame, net = self._frame_handle(N, n_vtx, o.hash_grid_size, int(kwargs.get("frame_slot") or 0)), self._net_handle(half=bool(o.fp16))
        if async_trips > 0:
            # non-blocking: a fixed number of trips, no host synchronisation (legal under HIP-graph capture); completion is
            # checked later with render_status(), a frame that ran out of trips is finished with render_continue()
            check(lib().pn_render_deformed_async(frame, net, C.byref(o), ptr(rays_o), ptr(rays_d), N, ptr(p_def), ptr(p_ori), ptr(F_IP), ptr(dF_IP),
                                                 n_vtx, ptr(self.density_bitfield), ptr(image), ptr(depth), ptr(depth_0), ptr(weights_sum),
                                                 async_trips, stream_ptr()), "render_deformed_async")
        else:
            stats = (C.c_int64 * 5)() if kwargs.get("collect_stats") else None
            check(lib().pn_render_deformed(frame, net, C.byref(o), ptr(rays_o), ptr(rays_d), N, ptr(p_def), ptr(p_ori), ptr(F_IP), ptr(dF_IP), n_vtx,
                                           ptr(self.density_bitfield), ptr(image), ptr(depth), ptr(depth_0), ptr(weights_sum), stats, stream_ptr()),
                  "render_deformed")
            if stats is not None:
                self._set_stats(stats)
        res = {"depth": depth.view(*prefix), "depth_0": depth_0.view(*prefix), "weights_sum": weights_sum}
        covered = weights_sum   # what the background is blended with: the object's own opacity, or with an overlay the object's and the colliders'
        if overlay:
            drawn = self._draw_colliders(rays_o, rays_d, 0.0 if (bg_tensor is not None or self.bg_radius > 0) else bg_color, weights_sum, depth_0, image,
                                         None, ob)
            covered, res["collider_t"] = drawn[0], drawn[1]
            res["coverage"] = covered
            if len(drawn) == 3:
                res["shadow"] = drawn[2]
        if self.bg_radius > 0 and not shadow_pass:
            self.blend_background(rays_o, rays_d, covered, image)   # in place: `image` may be the caller's out_buffers
        elif bg_tensor is not None:
            image = image + (1 - covered).unsqueeze(-1) * bg_tensor
        if self._points is not None and not shadow_pass:   # last: the points and the drag handle, painted onto the finished picture
            res["point_id"], res["point_t"] = self._draw_points(p_def, F_IP, weights_sum, depth_0, res.get("collider_t"), image, None, ob, kwargs)
        res["image"] = image.view(*prefix, 3)
        return res

    def render_continue(self, slot, rays_o, rays_d, out, n_trips=0, dt_gamma=0, bg_color=None, max_steps=1024, T_thresh=1e-2, static=False, **kwargs):
        """Finishes the frame last rendered on workspace `slot` with a fixed trip count that turned out too small (render_status reports
        rays alive at exit): more trips of the same loop — n_trips of them, or (0) until no ray is alive — and the epilogue again, into the
        SAME output tensors `out` (the dict the render returned).  The reference's loop has no trip limit but max_steps (renderer.py:836-891);
        this is how the captured, fixed-length forms keep that semantics.  Blocking when n_trips == 0.  With a background model the epilogue
        composites over 0 again and the model's colour is blended in again, once."""
        rays_o, rays_d = _flat_rays(rays_o, rays_d)
        N = rays_o.shape[0]
        if self.bg_radius > 0:
            bg_color = 0
        shadow_pass = bool(kwargs.get("_shadow_pass"))
        overlay = self._overlay is not None and not shadow_pass
        if overlay and self._shadows is not None and not static:
            # a shadow pass that ran out of its fixed trips is finished first, by this same continue on its own slot; the main frame's continue below
            # then rewrites `image` from the accumulator and applies the overlay again, over the finished map
            keep = self.last_stats
            try:
                if self.SHADOW_SLOT in self._frames and self.render_status(synchronize=True, slot=self.SHADOW_SLOT)["alive_at_exit"] > 0:
                    sh = self._shadows
                    self.render_continue(self.SHADOW_SLOT, sh["rays_o"], sh["rays_d"], self._shadow_out(), n_trips=n_trips, dt_gamma=dt_gamma, bg_color=0,
                                         max_steps=max_steps, T_thresh=T_thresh, **dict(kwargs, ray_tile_w=0, _shadow_pass=True))
            finally:
                self.last_stats = keep
        if static:
            self._refuse_overlay("the static render (render_continue with static=True)")
            self._refuse_point_overlay("the static render (render_continue with static=True)")
            o = self._static_opts(dt_gamma, 1 if bg_color is None else bg_color, max_steps, T_thresh)
        else:
            # with an overlay the epilogue rewrites `image` from the driver's accumulator over 0 and the overlay is applied once more, below
            o = self._deformed_opts(dt_gamma, 0.0 if overlay else (1 if bg_color is None else bg_color), max_steps, T_thresh, kwargs, n_rays=N)
        image, depth, ws = out["image"].view(-1, 3), out["depth"].view(-1), out["weights_sum"].view(-1)
        depth_0 = out["depth_0"].view(-1) if "depth_0" in out else torch.empty_like(depth)
        assert image.is_contiguous() and image.shape[0] == N
        stats = (C.c_int64 * 5)() if int(n_trips) == 0 else None
        check(lib().pn_render_continue(self._frames[slot][0], self._net_handle(half=bool(o.fp16)), C.byref(o), ptr(rays_o), ptr(rays_d), N,
                                       ptr(self.density_bitfield), ptr(image), ptr(depth), ptr(depth_0), ptr(ws), stats, int(n_trips), int(bool(static)),
                                       stream_ptr()), "render_continue")
        covered = ws
        if overlay:
            if "depth_0" not in out:
                raise RuntimeError("render_continue: the collider overlay composites against depth_0: pass the dict the deformed render returned")
            drawn = self._draw_colliders(rays_o, rays_d, 0.0 if self.bg_radius > 0 else (1 if bg_color is None else bg_color), ws, depth_0, image, out)
            covered = drawn[0]
            out["coverage"], out["collider_t"] = drawn[0], drawn[1]
            if len(drawn) == 3:
                out["shadow"] = drawn[2]
        if self.bg_radius > 0 and not shadow_pass:
            self.blend_background(rays_o, rays_d, covered, image)
        if self._points is not None and not shadow_pass and not static:
            # the epilogue rewrote `image`: the points are painted again, from the state the frame was rendered from (the key buffer cleaned itself)
            if "depth_0" not in out:
                raise RuntimeError("render_continue: the point overlay tests against depth_0: pass the dict the deformed render returned")
            p_def, _, F_IP, _ = self._ip_state(image.device)
            out["point_id"], out["point_t"] = self._draw_points(p_def, F_IP, ws, depth_0, out.get("collider_t") if overlay else None, image, out, None,
                                                                dict(kwargs, frame_slot=slot))
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

    def march_counters(self, enable, read=False, slot=0):
        """Measurement hook on workspace `slot`: 1 = device-side work counters of the march kernel (iterations, candidates, warps, samples);
        2 = HIP events around each trip's march and network launches (see trip_times)."""
        out = (C.c_uint64 * 4)() if read else None
        check(lib().pn_frame_march_counters(self._frames[slot][0], int(enable), out, stream_ptr()), "march_counters")
        return None if out is None else dict(iterations=int(out[0]), candidates=int(out[1]), warps=int(out[2]), samples=int(out[3]))

    def fused_clocks(self, slot=0, reset=False):
        """Phase clocks of the fused later-trips launches on `slot` (march_counters(4)): dict of cycles summed over waves + the trip the last render
        switched to the fused launch at (-1: it did not)."""
        out, first = (C.c_uint64 * 16)(), C.c_int(-1)
        check(lib().pn_frame_fused_clocks(self._frames[slot][0], out, C.byref(first), int(bool(reset)), stream_ptr()), "fused_clocks")
        return dict(refill=int(out[0]), march=int(out[1]), windows=int(out[2]), network=int(out[3]), composite=int(out[4]), wave_rounds=int(out[5]),
                    waves=int(out[6]), lifetime_ticks=int(out[7]), max_rounds=int(out[8]), max_lifetime_ticks=int(out[9]), first_trip=int(first.value),
                    # whole-frame form (fused_from = 0): the first trip's one-lane march, its 64-lane windows, its network, its composite + hand-over,
                    # the wait at the workgroup barrier behind it
                    a_march=int(out[10]), a_windows=int(out[11]), a_network=int(out[12]), a_composite=int(out[13]), a_barrier=int(out[14]),
                    mode=int(out[15]))   # 0: later trips only, 1: whole frame, 2: first trip's network / composite / compaction folded in

    def trip_records(self, slot=0, max_trips=16):
        """Diagnostics: [(n_alive, n_step, step_base, n_samples, n_emitted, n_tail)] per trip of the last render on `slot`."""
        rec, tail = (C.c_int * (5 * max_trips))(), (C.c_int * max_trips)()
        check(lib().pn_frame_trip_records(self._frames[slot][0], rec, tail, max_trips, stream_ptr()), "trip_records")
        return [tuple(rec[5 * i:5 * i + 5]) + (tail[i],) for i in range(max_trips) if rec[5 * i] > 0]

    def trip_times(self, slot=0):
        """Per-trip (march_ms, network_ms) of the last render on `slot` made while event timing was enabled (HIP events on the launch stream;
        for a captured render: the records of the last replay)."""
        a, b, n = (C.c_float * 64)(), (C.c_float * 64)(), C.c_int(0)
        check(lib().pn_frame_trip_times(self._frames[slot][0], a, b, 64, C.byref(n), stream_ptr()), "trip_times")
        return [float(a[i]) for i in range(n.value)], [float(b[i]) for i in range(n.value)]

    def render_status(self, synchronize=True, slot=0):
        """Outcome of the last render on frame workspace `slot`: dict(trips, samples, err, alive_at_exit).
        After an async render, alive_at_exit > 0 means the enqueued trips were not enough."""
        stats = (C.c_int64 * 5)()
        check(lib().pn_render_status(self._frames[slot][0], stats, int(bool(synchronize)), stream_ptr()), "render_status")
        self._set_stats(stats)
        return self.last_stats

    # ------------------------------------------------------------------ static render + training state
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
        self._refuse_overlay("the static render (run_cuda)")
        self._refuse_point_overlay("the static render (run_cuda)")
        if not self.training and not perturb and (self.bg_radius > 0 or not torch.is_tensor(bg_color)):
            return self._run_static_fused(rays_o, rays_d, dt_gamma, 1 if bg_color is None else bg_color, max_steps, T_thresh, **kwargs)
        return self.run_cuda_ops(rays_o, rays_d, dt_gamma, bg_color, perturb, force_all_rays, max_steps, T_thresh, **kwargs)

    def _run_static_fused(self, rays_o, rays_d, dt_gamma, bg_color, max_steps, T_thresh, **kwargs):
        prefix = rays_o.shape[:-1]
        rays_o, rays_d = _flat_rays(rays_o, rays_d)
        require_gpu(rays_o, rays_d)
        if self.bg_radius > 0:
            bg_color = 0   # renderer.py:283-288: the model's colour, blended in below
        N, device = rays_o.shape[0], rays_o.device
        o = self._static_opts(dt_gamma, bg_color, max_steps, T_thresh)
        aabb = (C.c_float * 6)(*self._aabb_infer_host())
        image, depth, depth_0, ws = (torch.empty(N, 3, dtype=torch.float32, device=device), torch.empty(N, dtype=torch.float32, device=device),
                                     torch.empty(N, dtype=torch.float32, device=device), torch.empty(N, dtype=torch.float32, device=device))
        frame = self._frame_handle(N, 1, 1.0, int(kwargs.get("frame_slot") or 0), cells=1)
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
        if getattr(self, "_aabb_cache", (None, None))[0] != key:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("aabb_infer changed: render one frame outside stream capture first")
            self._aabb_cache = (key, [float(v) for v in self.aabb_infer.tolist()])
        return self._aabb_cache[1]

    def run_cuda_ops(self, rays_o, rays_d, dt_gamma=0, bg_color=None, perturb=False, force_all_rays=False, max_steps=1024, T_thresh=1e-2, **kwargs):
        """run_cuda op by op on the drop-in ops (the training branch; the eval branch with perturb / tensor backgrounds; parity tests)."""
        self._refuse_overlay("the static render (run_cuda_ops)")
        self._refuse_point_overlay("the static render (run_cuda_ops)")
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

    def render(self, rays_o, rays_d, staged=False, max_ray_batch=4096, **kwargs):
        """renderer.py:552-585.  cuda_ray never stages.  Without cuda_ray the rays go through ``run``: staged, in batches of max_ray_batch with only
        depth and image returned (:565-580), otherwise in one call with weights_sum as well.  When ``run`` would take its fused form a staged call is
        served in one piece — that form has no [N, T, ...] intermediates to bound, and its per-ray results do not depend on how the rays are batched."""
        if self.cuda_ray:
            return self.run_cuda(rays_o, rays_d, **kwargs)
        if not staged:
            return self.run(rays_o, rays_d, **kwargs)
        if self._hier_fused_ok(rays_o, **kwargs):
            out = self.run(rays_o, rays_d, **kwargs)
            return {"depth": out["depth"], "image": out["image"]}
        B, N = rays_o.shape[:2]
        depth = torch.empty((B, N), device=rays_o.device)
        image = torch.empty((B, N, 3), device=rays_o.device)
        for b in range(B):
            for head in range(0, N, max_ray_batch):
                tail = min(head + max_ray_batch, N)
                part = self.run(rays_o[b:b + 1, head:tail], rays_d[b:b + 1, head:tail], **kwargs)
                depth[b:b + 1, head:tail] = part["depth"]
                image[b:b + 1, head:tail] = part["image"]
        return {"depth": depth, "image": image}

    # ------------------------------------------------------------------ hierarchical sampling without a density grid (renderer.py:137-265)
    @staticmethod
    def _check_hier_steps(num_steps, upsample_steps):
        if int(num_steps) < 1 or int(upsample_steps) < 0:
            raise RuntimeError(f"run: num_steps = {num_steps}, upsample_steps = {upsample_steps}")
        if int(upsample_steps) > 0 and int(num_steps) < 3:
            raise RuntimeError(f"run: upsample_steps = {upsample_steps} needs num_steps >= 3 (got {num_steps}): sample_pdf is handed weights[:, 1:-1], "
                               "which is empty, and the reference fails inside it")

    def _hier_fused_ok(self, rays_o, num_steps=128, upsample_steps=128, bg_color=None, perturb=False, **kwargs):
        """Whether ``run`` takes the fused launch for these arguments (see its docstring)."""
        if self.training or perturb or torch.is_grad_enabled() or self._autocast_half():
            return False
        if int(num_steps) + int(upsample_steps) > int(lib().pn_hier_max_samples()):
            return False
        if self.bg_radius > 0 or not torch.is_tensor(bg_color):
            return True
        n = rays_o.numel() // 3   # one colour [3] or one per ray [N, 3]; any other shape is left to torch's broadcasting in the op sequence
        return tuple(bg_color.shape) in ((3,), (n, 3))

    def run(self, rays_o, rays_d, num_steps=128, upsample_steps=128, bg_color=None, perturb=False, **kwargs):
        """NeRFRenderer.run (nerf/renderer.py:137-265) -> {'depth', 'image', 'weights_sum'}: num_steps stratified samples per ray, a density query,
        upsample_steps samples drawn from the resulting weights, a second density query, the merge, a colour query on the samples whose weight exceeds
        1e-4, and the sums.

        eval() under no_grad, without perturb:  ONE launch (pn_render_hier: a wave per ray, the sample set in LDS), then the background model's blend
                  when bg_radius > 0.  Takes a background of None / a scalar / one colour [3] / one colour per ray [N, 3].
        otherwise (train() mode, autograd recording, perturb, fp16 autocast — there is no half form of the launch —, or
                  num_steps + upsample_steps beyond the launch's LDS-resident limit, pn_hier_max_samples() = 512):  ``run_ops``."""
        self._refuse_overlay("the hierarchical render (run)")
        self._refuse_point_overlay("the hierarchical render (run)")
        self._check_hier_steps(num_steps, upsample_steps)
        if self._hier_fused_ok(rays_o, num_steps, upsample_steps, bg_color, perturb):
            return self._run_hier_fused(rays_o, rays_d, int(num_steps), int(upsample_steps), bg_color)
        return self.run_ops(rays_o, rays_d, num_steps, upsample_steps, bg_color, perturb, **kwargs)

    def _run_hier_fused(self, rays_o, rays_d, num_steps, upsample_steps, bg_color):
        prefix = rays_o.shape[:-1]
        rays_o, rays_d = _flat_rays(rays_o, rays_d)
        require_gpu(rays_o, rays_d)
        N, device = rays_o.shape[0], rays_o.device
        bg_rays, bg_scalar = None, 1.0
        if self.bg_radius > 0:
            bg_scalar = 0.0   # renderer.py:244-247: the model's colour, blended in below
        elif torch.is_tensor(bg_color):
            bg_rays = bg_color.to(device=device, dtype=torch.float32).expand(N, 3).contiguous()
        elif bg_color is not None:
            bg_scalar = float(bg_color)
        image = torch.empty(N, 3, dtype=torch.float32, device=device)
        depth = torch.empty(N, dtype=torch.float32, device=device)
        ws = torch.empty(N, dtype=torch.float32, device=device)
        aabb = (C.c_float * 6)(*self._aabb_infer_host())
        check(lib().pn_render_hier(self._net_handle(), ptr(rays_o), ptr(rays_d), N, aabb, float(self.min_near), num_steps, upsample_steps,
                                   float(self.density_scale), bg_scalar, ptr(bg_rays), ptr(image), ptr(depth), ptr(ws), 0, stream_ptr()), "render_hier")
        if self.bg_radius > 0 and N > 0:
            self.blend_background(rays_o, rays_d, ws, image)
        return {"depth": depth.view(*prefix), "image": image.view(*prefix, 3), "weights_sum": ws}

    def run_ops(self, rays_o, rays_d, num_steps=128, upsample_steps=128, bg_color=None, perturb=False, **kwargs):
        """``run`` as the reference's op sequence on near_far_from_aabb / density / color / sample_pdf and torch ops: differentiable (the training
        branch), with perturb, under autocast, with any background; the parity tests pin it against the reference's own run."""
        self._refuse_overlay("the hierarchical render (run_ops)")
        self._refuse_point_overlay("the hierarchical render (run_ops)")
        self._check_hier_steps(num_steps, upsample_steps)
        prefix = rays_o.shape[:-1]
        rays_o = rays_o.contiguous().view(-1, 3)
        rays_d = rays_d.contiguous().view(-1, 3)
        require_gpu(rays_o, rays_d)
        N, device = rays_o.shape[0], rays_o.device
        aabb = self.aabb_train if self.training else self.aabb_infer
        nears, fars = raymarching.near_far_from_aabb(rays_o, rays_d, aabb, self.min_near)
        nears, fars = nears.unsqueeze(-1), fars.unsqueeze(-1)
        z_vals = torch.linspace(0.0, 1.0, num_steps, device=device).unsqueeze(0).expand((N, num_steps))
        z_vals = nears + (fars - nears) * z_vals
        sample_dist = (fars - nears) / num_steps
        if perturb:
            z_vals = z_vals + (torch.rand(z_vals.shape, device=device) - 0.5) * sample_dist   # unclamped, as in the reference
        xyzs = rays_o.unsqueeze(-2) + rays_d.unsqueeze(-2) * z_vals.unsqueeze(-1)
        xyzs = torch.min(torch.max(xyzs, aabb[:3]), aabb[3:])

        def weights_of(z, sigma):
            deltas = z[..., 1:] - z[..., :-1]
            deltas = torch.cat([deltas, sample_dist * torch.ones_like(deltas[..., :1])], dim=-1)   # the last one is sample_dist, also after the merge
            alphas = 1 - torch.exp(-deltas * self.density_scale * sigma)
            shifted = torch.cat([torch.ones_like(alphas[..., :1]), 1 - alphas + 1e-15], dim=-1)
            return deltas, alphas * torch.cumprod(shifted, dim=-1)[..., :-1]

        dens = {k: v.view(N, num_steps, -1) for k, v in self.density(xyzs.reshape(-1, 3)).items()}
        if upsample_steps > 0:
            with torch.no_grad():
                deltas, weights = weights_of(z_vals, dens["sigma"].squeeze(-1))
                z_mid = z_vals[..., :-1] + 0.5 * deltas[..., :-1]
                new_z = sample_pdf(z_mid, weights[:, 1:-1], upsample_steps, det=not self.training).detach()
                new_xyzs = rays_o.unsqueeze(-2) + rays_d.unsqueeze(-2) * new_z.unsqueeze(-1)
                new_xyzs = torch.min(torch.max(new_xyzs, aabb[:3]), aabb[3:])
            new_dens = {k: v.view(N, upsample_steps, -1) for k, v in self.density(new_xyzs.reshape(-1, 3)).items()}   # only the new points
            z_vals, z_index = torch.sort(torch.cat([z_vals, new_z], dim=1), dim=1)
            xyzs = torch.cat([xyzs, new_xyzs], dim=1)
            xyzs = torch.gather(xyzs, dim=1, index=z_index.unsqueeze(-1).expand_as(xyzs))
            for k in dens:
                both = torch.cat([dens[k], new_dens[k]], dim=1)
                dens[k] = torch.gather(both, dim=1, index=z_index.unsqueeze(-1).expand_as(both))
        _, weights = weights_of(z_vals, dens["sigma"].squeeze(-1))
        dirs = rays_d.view(-1, 1, 3).expand_as(xyzs)
        dens = {k: v.reshape(-1, v.shape[-1]) for k, v in dens.items()}
        mask = weights > 1e-4  # hard coded in the reference
        rgbs = self.color(xyzs.reshape(-1, 3), dirs.reshape(-1, 3), mask=mask.reshape(-1), **dens).view(N, -1, 3)
        weights_sum = weights.sum(dim=-1)
        ori_z_vals = ((z_vals - nears) / (fars - nears)).clamp(0, 1)
        depth = torch.sum(weights * ori_z_vals, dim=-1)   # NaN for a ray that misses the box (near == far), like the reference
        image = torch.sum(weights.unsqueeze(-1) * rgbs, dim=-2)
        if self.bg_radius > 0:
            bg_color = self.background(raymarching.sph_from_ray(rays_o, rays_d, self.bg_radius), rays_d.reshape(-1, 3))
        elif bg_color is None:
            bg_color = 1
        image = image + (1 - weights_sum).unsqueeze(-1) * bg_color
        return {"depth": depth.view(*prefix), "image": image.view(*prefix, 3), "weights_sum": weights_sum}

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

    # ------------------------------------------------------------------ op-by-op loop (reference structure, renderer.py:755-907)
    def rund_cuda_ops(self, rays_o, rays_d, dt_gamma=0, bg_color=None, perturb=False, max_steps=1024, T_thresh=1e-2, **kwargs):
        self._refuse_overlay("the op-by-op loop (rund_cuda_ops)")
        self._refuse_point_overlay("the op-by-op loop (rund_cuda_ops)")
        dtype = torch.float32
        prefix = rays_o.shape[:-1]
        rays_o = rays_o.contiguous().view(-1, 3)
        rays_d = rays_d.contiguous().view(-1, 3)
        N, device = rays_o.shape[0], rays_o.device
        max_iter_num, hgs, bound = kwargs.get("max_iter_num"), kwargs.get("hash_grid_size"), kwargs.get("bound")
        cut = kwargs.get("cut")
        cut_bounds = torch.tensor(kwargs.get("cut_bounds") or [0.0] * 6, dtype=dtype, device=device)
        p_def, p_ori, F_IP, dF_IP = self._ip_state(device)
        bmin, bmax = p_def.min(axis=0).values, p_def.max(axis=0).values
        if cut:
            bmin = -bound * torch.ones(3, dtype=dtype, device=device)
            bmax = bound * torch.ones(3, dtype=dtype, device=device)
        marg = 1e-3
        bbmin = bmin - marg * torch.ones(3, dtype=dtype, device=device)
        bbmax = bmax + marg * torch.ones(3, dtype=dtype, device=device)
        resolution = torch.ceil((bbmax - bbmin) / hgs).to(torch.int32)
        aabb = torch.cat((bbmin, bbmax), dim=0)
        nears, fars = raymarching.near_far_from_aabb(rays_o, rays_d, aabb, self.min_near)
        if self.bg_radius > 0:  # renderer.py:799-801
            bg_color = self.background(raymarching.sph_from_ray(rays_o, rays_d, self.bg_radius), rays_d)
        elif bg_color is None:
            bg_color = 1
        weights_sum = torch.zeros(N, dtype=dtype, device=device)
        depth = torch.zeros(N, dtype=dtype, device=device)
        image = torch.zeros(N, 3, dtype=dtype, device=device)
        num_seek_IP = kwargs.get("num_seek_IP")
        n_vtx = p_ori.shape[0]
        n_grid = int(resolution[2] * resolution[1] * resolution[0])
        assert p_def.shape == p_ori.shape and n_vtx > 0
        pig_cnt, pig_bgn, pig_idx = get_pnts_in_grids(n_vtx, n_grid, p_def, bbmin, bbmax, hgs, resolution)
        rays_alive = torch.arange(N, dtype=torch.int32, device=device)
        rays_t = nears.clone()
        step, trips, samples = 0, 0, 0
        while step < max_steps:
            n_alive = rays_alive.shape[0]
            if n_alive <= 0:
                break
            n_step = max(min(N // n_alive, 8), 1)
            xyzs, dirs, deltas = raymarching.march_rays_quadratic_bending(
                pig_cnt, pig_bgn, pig_idx, n_vtx, n_grid, p_def, p_ori, F_IP, dF_IP, max_iter_num, bbmin, bbmax, hgs, resolution, num_seek_IP,
                self.IP_dx, cut, cut_bounds, n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, self.bound, self.density_bitfield, self.cascade,
                self.grid_size, nears, fars, 128, perturb if step == 0 else False, dt_gamma, max_steps)
            sigmas, rgbs = self(xyzs, dirs)
            sigmas = self.density_scale * sigmas
            raymarching.composite_rays(n_alive, n_step, rays_alive, rays_t, sigmas, rgbs, deltas, weights_sum, depth, image, T_thresh)
            rays_alive = raymarching.compact_rays(rays_alive)  # == rays_alive[rays_alive >= 0]
            samples += int((deltas[:, 0] != 0).sum())
            step += n_step
            trips += 1
        self.last_stats = dict(trips=trips, samples=samples, err=0, alive_at_exit=int(rays_alive.shape[0]))
        depth_0 = depth
        image = image + (1 - weights_sum).unsqueeze(-1) * bg_color
        depth = torch.clamp(depth - nears, min=0) / (fars - nears)
        return {"depth": depth.view(*prefix), "image": image.view(*prefix, 3), "depth_0": depth_0.view(*prefix), "weights_sum": weights_sum}
