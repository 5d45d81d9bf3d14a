"""The contact colliders drawn into the deformed frame, and the object's shadow on them (csrc/pn_colliders.hip): the overlay's
state as two records on NeRFRenderer, the shadow pass in front of the camera's render and the one launch behind the frame driver
(NeRFRenderer._finish_frame enqueues it first)."""
import ctypes as C
import math
from typing import NamedTuple

import torch

from .._lib import ColliderStyle, ShadowLight, check, lib, ptr, require_gpu, stream_ptr
from ._outputs import take_output


class ColliderOverlay(NamedTuple):
    """set_collider_overlay: what the overlay's launch reads."""
    state: torch.Tensor      # pn_contact_state, 93 doubles on the device
    style: ColliderStyle
    t_max: float


class ColliderShadows(NamedTuple):
    """set_collider_shadows: the light, its rays, the map buffers and the shadow pass's other outputs."""
    light: ShadowLight
    rays_o: torch.Tensor
    rays_d: torch.Tensor
    shadow_ws: torch.Tensor
    shadow_depth_0: torch.Tensor
    image: torch.Tensor
    depth: torch.Tensor

    def out(self):
        """The shadow pass's out_buffers: the map buffers are its weights_sum and depth_0."""
        return {"image": self.image, "depth": self.depth, "depth_0": self.shadow_depth_0, "weights_sum": self.shadow_ws}


class ColliderOverlayMixin:
    SHADOW_SLOT = 900   # the shadow pass's frame workspace: the pipeline's lanes use 0 .. lanes * depth - 1, the tile-parallel form 800

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
        self._overlay = ColliderOverlay(state, style, t_max)
        return self

    def clear_collider_overlay(self):
        self._overlay = None
        self._shadows = None

    def collider_overlay_key(self):
        """What a captured render bakes in of the overlay (None without one): the state's address, the style's bytes, t_max — and with shadows set the
        light's bytes and the map buffers' addresses."""
        ov, sh = self._overlay, self._shadows
        if ov is None:
            return None
        key = (ov.state.data_ptr(), bytes(ov.style), ov.t_max)
        if sh is not None:
            key += (bytes(sh.light), sh.shadow_ws.data_ptr(), sh.shadow_depth_0.data_ptr())
        return key

    # ------------------------------------------------------------------ the object's shadow on the drawn colliders
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
        dev = self._overlay.state.device
        rays_o, rays_d = shadow_rays(light, dev)
        n = rays_o.shape[0]
        buf = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)   # noqa: E731
        self._shadows = ColliderShadows(light, rays_o, rays_d, shadow_ws=buf(n), shadow_depth_0=buf(n), image=buf(n, 3), depth=buf(n))
        return self

    def clear_collider_shadows(self):
        self._shadows = None

    @property
    def shadow_ws(self):
        return self._shadows.shadow_ws if self._shadows is not None else None

    @property
    def shadow_depth_0(self):
        return self._shadows.shadow_depth_0 if self._shadows is not None else None

    def _render_shadow_map(self, dt_gamma, max_steps, T_thresh, kwargs):
        """The shadow pass, on the current stream in front of the camera's render.  ray_tile_w is set explicitly: S^2 == W H must not select the image
        tiling by accident (results do not depend on it).  last_stats stays the main frame's; the pass's own are read with render_status(slot=SHADOW_SLOT)."""
        sh = self._shadows
        keep = self.last_stats
        try:
            self.rund_cuda(sh.rays_o, sh.rays_d, dt_gamma=dt_gamma, bg_color=0, perturb=False, max_steps=max_steps, T_thresh=T_thresh, _shadow_pass=True,
                           **dict(kwargs, frame_slot=self.SHADOW_SLOT, out_buffers=sh.out(), ray_tile_w=0))
        finally:
            self.last_stats = keep

    def _continue_shadow_map(self, n_trips, dt_gamma, max_steps, T_thresh, kwargs):
        """A shadow pass that ran out of its fixed trips is finished first, by render_continue on its own slot; the main frame's continue then rewrites
        `image` from the accumulator and applies the overlay again, over the finished map."""
        sh = self._shadows
        keep = self.last_stats
        try:
            if self.SHADOW_SLOT in self._frames and self.render_status(synchronize=True, slot=self.SHADOW_SLOT)["alive_at_exit"] > 0:
                self.render_continue(self.SHADOW_SLOT, sh.rays_o, sh.rays_d, sh.out(), n_trips=n_trips, dt_gamma=dt_gamma, bg_color=0, max_steps=max_steps,
                                     T_thresh=T_thresh, _shadow_pass=True, **dict(kwargs, ray_tile_w=0))
        finally:
            self.last_stats = keep

    def _draw_colliders(self, rays_o, rays_d, bg_scalar, weights_sum, depth_0, image, res, ob):
        """Enqueues the overlay's launch on the current stream, in place in `image` (the frame composited over 0); 'coverage' and 'collider_t' of `res`
        (then of `ob`, else allocated) receive its other outputs, and with shadows 'shadow': `res` holds them afterwards.  Returns (coverage, collider_t)."""
        ov, sh = self._overlay, self._shadows
        N = image.shape[0]
        for name in ("coverage", "collider_t") + (("shadow",) if sh is not None else ()):
            res[name] = take_output(name, (N,), torch.float32, image.device, res, ob)
        cov, ct = res["coverage"], res["collider_t"]
        args = (ptr(ov.state), C.byref(ov.style), ptr(rays_o), ptr(rays_d), N, float(self.min_near), ov.t_max, float(bg_scalar), ptr(weights_sum), ptr(depth_0),
                ptr(image), ptr(cov), ptr(ct))
        if sh is not None:
            check(lib().pn_draw_colliders_shadowed(*args, sh.light, ptr(sh.shadow_ws), ptr(sh.shadow_depth_0), ptr(res["shadow"]), stream_ptr()),
                  "draw_colliders_shadowed")
        else:
            check(lib().pn_draw_colliders(*args, stream_ptr()), "draw_colliders")
        return cov, ct
