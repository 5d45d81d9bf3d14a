"""The GUI's mouse drag on the device (gui.py:556-586, :833-841, :857-865; csrc/pn_drag.hip): a pn_drag_state in device memory, read by a
k_drag_force launch in front of every substep.  The one stage that writes dof_f, not the right-hand side."""
import numpy as np
import torch

from .._lib import check, lib, ptr, stream_ptr
from ._stage import Stage, torchfloat

__all__ = ["DRAG_SCALE_MIN", "DRAG_SCALE_MAX", "wheel_force_scale", "DragMixin"]   # what solver.py re-exports

DRAG_SCALE_MIN, DRAG_SCALE_MAX = 1e-3, 5e1   # gui.py:865

STAGE = Stage(name="drag", flag="drag_enabled", state="_drag", subject="drag is", owner="the drag state", enable="enable_drag",
              struct="pn_drag_state", nbytes=40, sized_by="solver.py allocates", init="_init_drag", alloc="_alloc_drag", enqueue="_enqueue_drag_force",
              tables=None, writes="dof_f", clock=False)


def wheel_force_scale(scale, delta):
    """The GUI's mouse-wheel rule for the drag's force scale (gui.py:857-865): +-0.5 per notch above 1, +-0.1 at or below, clamped to [1e-3, 50]."""
    scale = float(scale)
    scale += delta * 0.5 if scale > 1.0 else delta * 0.1
    return max(DRAG_SCALE_MIN, min(scale, DRAG_SCALE_MAX))


def _check_scale(s):
    s = float(s)
    if not (np.isfinite(s) and s > 0.0):
        raise ValueError(f"drag force scale must be a positive finite number, got {s!r}")
    return s


class DragMixin:
    def _init_drag(self):
        self.drag_enabled = False
        self.drag_force_scale = 1.0
        self._drag = self._drag_work = None

    def enable_drag(self, scale=None):
        """From now on every stepforward() first writes dof_f with the GUI's spring force from the drag state (csrc/pn_drag.hip: k_drag_force):
        f = scale 1e5 (target - p0), |f| <= 5e5, p0 = the picked IP's get_IP_info() position of the state that substep starts from; all zero until
        drag_pick().  The state lives in device memory, so substeps captured into graphs after this call follow drag_to() without a recapture.
        While drag is enabled the drag state owns dof_f: update_force / clear_force raise.  May be called before initialize()."""
        if scale is not None:
            self.drag_force_scale = _check_scale(scale)
        self._switch_on(STAGE)
        return self

    def _alloc_drag(self):
        self._new_state(STAGE)          # vid, active = 0; target = 0
        self._drag_work = torch.zeros(int(lib().pn_sim_drag_work_doubles()), dtype=torchfloat, device=self.device)
        check(lib().pn_sim_drag_set(ptr(self._drag), self.n_IP, -1, -1, float(self.drag_force_scale), None, stream_ptr()), "sim_drag_set")
        self.dof_f.zero_()

    def _enqueue_drag_force(self):
        """dof_f = the spring force of THIS substep's state (gui.py:556-586), on the substep's stream, captured with it into graphs."""
        check(lib().pn_sim_drag_force(self.n_k, self.n_IP, ptr(self._drag), ptr(self.dof), float(self.dx), ptr(self.IP_kernel), ptr(self.IP_rho),
                                      ptr(self.IP_Nx), ptr(self.dof_f), stream_ptr()), "sim_drag_force")

    def _unproject(self, depth0, x, y, pose, intrinsics, ip_pos):
        drag = self._stage_state(STAGE)
        d = depth0.reshape(depth0.shape[-2], depth0.shape[-1]) if depth0.dim() >= 2 else depth0
        if d.dtype != torch.float32 or not d.is_cuda or not d.is_contiguous():
            raise ValueError("drag: depth0 must be a contiguous fp32 [H, W] tensor on the GPU (a frame's depth_0)")
        H, W = d.shape
        intr = np.ascontiguousarray(np.asarray(intrinsics, np.float64).reshape(4))
        pose16 = np.ascontiguousarray(np.asarray(pose, np.float64).reshape(-1)[-16:])
        n = 0
        if ip_pos is not None:
            if ip_pos.dtype != torch.float32 or not ip_pos.is_cuda or tuple(ip_pos.shape) != (self.n_IP, 3) or not ip_pos.is_contiguous():
                raise ValueError("drag_pick: ip_pos must be the contiguous fp32 [n_IP, 3] IP positions of a frame, on the GPU")
            n = self.n_IP
        with self._on_force_stream():
            check(lib().pn_sim_drag_unproject(ptr(d), W, H, float(x), float(y), intr.ctypes.data, pose16.ctypes.data, ptr(ip_pos), n, ptr(drag),
                                              ptr(self._drag_work), stream_ptr()), "sim_drag_unproject")

    def drag_pick(self, depth0, x, y, pose, intrinsics, ip_pos):
        """A ctrl-click at pixel (x, y) (gui.py:833-841): target = screen_to_world(x, y) against `depth0` ([H, W] fp32, the last frame's depth_0),
        the drag acts on the IP of `ip_pos` ([n_IP, 3] fp32, the IP positions that frame was rendered from) nearest to it.  Returns that IP's index:
        the drag's one read back to the host.  (x, y) are image pixels; a window's own offsets (dearpygui's +20 title bar, gui.py:809-812) are the
        caller's business."""
        self._unproject(depth0, x, y, pose, intrinsics, ip_pos)
        return int(self._host_read(lambda: self._drag[:1].view(torch.int32)[0].item()))

    def drag_to(self, depth0, x, y, pose, intrinsics):
        """The cursor moved to pixel (x, y): target = screen_to_world(x, y) against `depth0` (gui.py:647-657).  No host read."""
        self._unproject(depth0, x, y, pose, intrinsics, None)

    def drag_scale(self, s):
        """Sets the GUI's force_scale (f = s 1e5 (target - p0))."""
        self.drag_force_scale = _check_scale(s)
        if self._drag is not None:
            with self._on_force_stream():
                check(lib().pn_sim_drag_set(ptr(self._drag), self.n_IP, -1, -1, float(self.drag_force_scale), None, stream_ptr()), "sim_drag_set")
        return self.drag_force_scale

    def drag_wheel(self, delta):
        """The mouse wheel's rule (gui.py:857-865) applied to the force scale; returns the new scale."""
        return self.drag_scale(wheel_force_scale(self.drag_force_scale, delta))

    def drag_hold(self, vid, target):
        """Drags IP `vid` toward the world point `target` (no unprojection): scripted drags and tests."""
        t = np.ascontiguousarray(np.asarray(target, np.float64).reshape(3))
        drag = self._stage_state(STAGE)
        with self._on_force_stream():
            check(lib().pn_sim_drag_set(ptr(drag), self.n_IP, int(vid), 1, 0.0, t.ctypes.data, stream_ptr()), "sim_drag_set")

    def release(self):
        """Nothing picked (right click / Q, gui.py:821-826,843-849): every following substep gets dof_f = 0, as after clear_force()."""
        drag = self._stage_state(STAGE)
        with self._on_force_stream():
            check(lib().pn_sim_drag_set(ptr(drag), self.n_IP, -1, 0, 0.0, None, stream_ptr()), "sim_drag_set")
