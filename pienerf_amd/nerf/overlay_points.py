"""The simulator's integration points and the drag handle drawn into the deformed frame (csrc/pn_points_overlay.hip): the overlay's
state as one record on NeRFRenderer, its key buffers, and the launch pair that NeRFRenderer._finish_frame enqueues last."""
import ctypes as C
import math
from typing import NamedTuple, Optional

import torch

from .._lib import PointStyle, check, lib, ptr, require_gpu, stream_ptr
from ._outputs import take_output


class PointOverlay(NamedTuple):
    """set_point_overlay: the camera, the style and what else the launch pair reads."""
    pose: Optional[torch.Tensor]      # the default c2w on the device; None: every render passes point_pose
    intrinsics: tuple                 # (fx, fy, cx, cy)
    intrinsics_c: object              # ... as the launch takes them: float[4]
    W: int
    H: int
    style: PointStyle
    values: Optional[torch.Tensor]
    drag: Optional[torch.Tensor]      # pn_drag_state, 5 doubles on the device


class PointOverlayMixin:
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
        self._points = PointOverlay(pose_dev, intr, (C.c_float * 4)(*intr), W, H, style, values, drag_state)
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
        p = self._points
        if p is None:
            return None
        adr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        return (adr(p.pose), p.intrinsics, p.W, p.H, bytes(p.style), adr(p.values), adr(p.drag))

    def point_overlay_reads_drag(self):
        """Whether the launch pair reads a drag state: the caller then orders the render behind the stream that writes it."""
        return self._points is not None and self._points.drag is not None

    def _point_key_buffer(self, slot, device):
        """The key buffer of frame workspace `slot` (lanes run concurrently: one each), allocated and filled outside any capture."""
        from ..points_overlay import key_buffer
        p = self._points
        cur = self._point_keys.get(slot)
        if cur is None or cur.numel() != p.W * p.H or cur.device != device:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"point overlay: the key buffer of frame workspace {slot} must exist before a capture: render one frame on it first")
            cur = self._point_keys[slot] = key_buffer(p.W, p.H, device)
        return cur

    def _draw_points(self, p_def, F_IP, weights_sum, depth_0, collider_t, image, res, ob, slot, pose):
        """Enqueues the point overlay's launch pair on the current stream, in place in `image` (the finished picture); 'point_id' and 'point_t' of `res`
        (then of `ob`, else allocated) receive its other outputs: `res` holds them afterwards.  `pose`: this render's point_pose, None: the overlay's own."""
        p = self._points
        N = image.shape[0]
        if N != p.W * p.H:
            raise RuntimeError(f"point overlay: set for a {p.W} x {p.H} frame, this render has {N} rays (it needs N == W H: the whole image)")
        pose = p.pose if pose is None else pose
        if pose is None:
            raise RuntimeError("point overlay: set_point_overlay() got no pose_dev: pass this render's camera as point_pose=")
        self._check_point_pose(pose)
        n = p_def.shape[0]
        if p.values is not None and p.values.shape[0] != n:
            raise RuntimeError(f"point overlay: `values` has {p.values.shape[0]} entries, the frame {n} integration points")
        assert F_IP.shape[0] == n and F_IP.is_contiguous() and image.is_contiguous()
        pid = res["point_id"] = take_output("point_id", (N,), torch.int32, image.device, res, ob)
        pt = res["point_t"] = take_output("point_t", (N,), torch.float32, image.device, res, ob)
        keys = self._point_key_buffer(slot, image.device)
        check(lib().pn_draw_points(ptr(p_def), ptr(F_IP), ptr(p.values), n, ptr(pose), p.intrinsics_c, p.W, p.H, float(self.min_near), ptr(weights_sum),
                                   ptr(depth_0), ptr(collider_t), ptr(p.drag), ptr(keys), p.style, ptr(image), ptr(pid), ptr(pt), stream_ptr()), "draw_points")
