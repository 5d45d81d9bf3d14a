"""The simulator's integration points and the drag handle drawn into a rendered frame (csrc/pn_points_overlay.hip; include/pienerf_hip.h: pn_draw_points
has the law).

``point_style`` builds the launch pair's by-value style; ``key_buffer`` allocates the per-frame key buffer, filled once with the empty value.  The
renderer's side — the overlay's state, the key buffers per frame workspace, the launch pair — is nerf/overlay_points.py.
"""
import math

import torch

from ._lib import PointStyle

MODES = {"flat": 0, "strain": 1, "volume": 2, "values": 3}
MAX_RADIUS = 8
# the reference's point colour (gui.py:539) and a blue - white - red ramp for the scalar modes
POINT_RGB = (0.0, 0.0, 1.0)
RAMP = ((0.1, 0.2, 0.9), (0.95, 0.95, 0.95), (0.9, 0.15, 0.1))
RANGES = {"flat": (0.0, 1.0), "strain": (0.0, 0.25), "volume": (-0.25, 0.25), "values": (0.0, 1.0)}


def point_style(radius=1, mode="flat", rgb=POINT_RGB, ramp=RAMP, lo=None, hi=None, xray=False, alpha=1.0, hidden_alpha=0.0, bias=0.02,
                marker_radius=10.0, marker_thickness=5.0):
    """A PointStyle (pn_point_style).  `radius`: the footprint in pixels, an integer in 0 .. 8; `mode`: 'flat' (`rgb`), or a scalar per point mapped
    through `ramp` (three colours at u = 0, 1/2, 1) over [`lo`, `hi`] (None: RANGES[mode]): 'strain' = |1/2 (F^T F - I)|_F, 'volume' = det F - 1,
    'values' = the array given to set_point_overlay.  `xray`: every point is visible, as in the reference; otherwise a point is depth-tested against the
    object and the drawn colliders with the slack `bias` (units of t), and a hidden one is drawn with alpha * `hidden_alpha` (0: not at all).
    `marker_radius` / `marker_thickness`: the drag handle's discs and line in pixels (the reference's 10 and 5).  ValueError for a radius outside
    0 .. 8, an unknown mode, a non-finite value, alpha or hidden_alpha outside [0, 1], hi <= lo in a ramp mode, a negative marker size."""
    st = PointStyle()
    if isinstance(radius, bool) or int(radius) != radius or not 0 <= int(radius) <= MAX_RADIUS:
        raise ValueError(f"point_style: radius must be an integer in 0 .. {MAX_RADIUS}, got {radius!r}")
    if mode not in MODES:
        raise ValueError(f"point_style: mode must be one of {sorted(MODES)}, got {mode!r}")
    rgb = tuple(float(v) for v in rgb)
    ramp = tuple(tuple(float(v) for v in c) for c in ramp)
    if len(rgb) != 3 or len(ramp) != 3 or any(len(c) != 3 for c in ramp):
        raise ValueError("point_style: rgb is one colour and ramp three colours of 3 components")
    lo = RANGES[mode][0] if lo is None else float(lo)
    hi = RANGES[mode][1] if hi is None else float(hi)
    st.radius, st.mode, st.xray = int(radius), MODES[mode], int(bool(xray))
    for j in range(3):
        st.rgb[j] = rgb[j]
        for k in range(3):
            st.ramp[k][j] = ramp[k][j]
    st.lo, st.hi, st.alpha, st.hidden_alpha, st.bias = lo, hi, float(alpha), float(hidden_alpha), float(bias)
    st.marker_radius, st.marker_thickness = float(marker_radius), float(marker_thickness)
    vals = list(st.rgb) + [st.ramp[k][j] for k in range(3) for j in range(3)] + [st.lo, st.hi, st.alpha, st.hidden_alpha, st.bias, st.marker_radius,
                                                                                 st.marker_thickness]
    if not all(math.isfinite(v) for v in vals):
        raise ValueError("point_style: every value must be finite")
    if not 0.0 <= st.alpha <= 1.0:
        raise ValueError(f"point_style: alpha must be in [0, 1], got {alpha!r}")
    if not 0.0 <= st.hidden_alpha <= 1.0:
        raise ValueError(f"point_style: hidden_alpha must be in [0, 1], got {hidden_alpha!r}")
    if mode != "flat" and not st.hi > st.lo:
        raise ValueError(f"point_style: the ramp's range needs hi > lo, got lo = {lo!r}, hi = {hi!r}")
    if st.marker_radius < 0.0 or st.marker_thickness < 0.0:
        raise ValueError("point_style: marker_radius and marker_thickness must be >= 0")
    return st


def mode_name(style):
    return next(k for k, v in MODES.items() if v == int(style.mode))


def key_buffer(W, H, device):
    """The launch pair's key buffer for a W x H frame: W H 64-bit words, all the empty value ~0.  The resolve launch leaves it that way."""
    return torch.full((int(W) * int(H),), -1, dtype=torch.int64, device=device)
