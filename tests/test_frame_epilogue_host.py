"""The host side of the deformed frame's epilogue (pienerf_amd/nerf/renderer.py: frame_background, NeRFRenderer._finish_frame and _refuse_overlays;
nerf/_outputs.py; the overlay records of nerf/overlay_colliders.py and nerf/overlay_points.py).  No device: the records are built directly, in host memory."""
import ctypes as C
import re

import pytest
import torch

from pienerf_amd.colliders import collider_style, shadow_light
from pienerf_amd.nerf._outputs import frame_outputs, take_output
from pienerf_amd.nerf.overlay_colliders import ColliderOverlay, ColliderShadows
from pienerf_amd.nerf.overlay_points import PointOverlay
from pienerf_amd.nerf.renderer import NeRFRenderer, frame_background, sample_pdf  # noqa: F401 — both names stay exported
from pienerf_amd.points_overlay import point_style

COLOUR = torch.tensor([0.1, 0.5, 0.9])
# (bg_color, bg_radius, an overlay draws) -> (the driver's scalar, the collider launch's scalar, the tensor): the frame drivers' expressions, written out
TABLE = [
    (None, -1, False, (1, 1, None)), (None, -1, True, (0.0, 1, None)),
    (0, -1, False, (0, 0, None)), (0, -1, True, (0.0, 0, None)),
    (0.3, -1, False, (0.3, 0.3, None)), (0.3, -1, True, (0.0, 0.3, None)),
    (COLOUR, -1, False, (0.0, 0.0, COLOUR)), (COLOUR, -1, True, (0.0, 0.0, COLOUR)),
    (None, 32, False, (0.0, 0.0, None)), (None, 32, True, (0.0, 0.0, None)),
    (0, 32, False, (0.0, 0.0, None)), (0, 32, True, (0.0, 0.0, None)),
    (0.3, 32, False, (0.0, 0.0, None)), (0.3, 32, True, (0.0, 0.0, None)),
    (COLOUR, 32, False, (0.0, 0.0, None)), (COLOUR, 32, True, (0.0, 0.0, None)),
]


@pytest.mark.parametrize("bg_color, bg_radius, overlay, want", TABLE)
def test_frame_background_table(bg_color, bg_radius, overlay, want):
    driver, colliders, tensor = frame_background(bg_color, bg_radius, overlay)
    assert float(driver) == want[0] and float(colliders) == want[1]
    assert tensor is want[2]


def test_take_output_prefers_out_then_out_buffers_then_allocates():
    a, b = torch.zeros(5), torch.ones(5)
    assert take_output("coverage", (5,), torch.float32, "cpu", {"coverage": a}, {"coverage": b}) is a
    assert take_output("coverage", (5,), torch.float32, "cpu", {"depth": a}, {"coverage": b}) is b
    assert take_output("coverage", (5,), torch.float32, "cpu", None, {"coverage": b}) is b
    assert take_output("coverage", (5,), torch.float32, "cpu", {"coverage": None}, {"coverage": b}) is b
    new = take_output("point_id", (5,), torch.int32, "cpu", {"depth": a}, None)
    assert new.shape == (5,) and new.dtype == torch.int32 and new.is_contiguous()
    for wrong in (torch.zeros(5, dtype=torch.float64), torch.zeros(4), torch.zeros(5, 2)[:, 0]):     # dtype, shape, contiguity
        with pytest.raises(AssertionError):
            take_output("coverage", (5,), torch.float32, "cpu", {"coverage": wrong})
    ob = {"image": torch.zeros(5, 3), "depth": a}
    image, depth, depth_0, ws = frame_outputs(5, "cpu", ob)
    assert image is ob["image"] and depth is a and depth_0.shape == ws.shape == (5,) and depth_0.dtype == ws.dtype == torch.float32
    assert [t.shape for t in frame_outputs(4, "cpu")] == [(4, 3), (4,), (4,), (4,)]
    with pytest.raises(AssertionError):
        frame_outputs(5, "cpu", {"image": torch.zeros(5)})


def _colliders():
    return ColliderOverlay(torch.zeros(93, dtype=torch.float64), collider_style(), 8.0)


def _points(**kw):
    intr = (40.0, 41.0, 24.0, 23.0)
    args = dict(pose=None, intrinsics=intr, intrinsics_c=(C.c_float * 4)(*intr), W=48, H=47, style=point_style(radius=2), values=None, drag=None)
    return PointOverlay(**dict(args, **kw))


RAYS = torch.zeros(4, 3)
ENTRIES = {
    "the op-by-op loop (perturb=True)": lambda r: r.rund_cuda(RAYS, RAYS, perturb=True),
    "the op-by-op loop (rund_cuda_ops)": lambda r: r.rund_cuda_ops(RAYS, RAYS),
    "the static render (render_continue with static=True)": lambda r: r.render_continue(0, RAYS, RAYS, {}, static=True),
    "the static render (run_cuda)": lambda r: r.run_cuda(RAYS, RAYS),
    "the static render (run_cuda_ops)": lambda r: r.run_cuda_ops(RAYS, RAYS),
    "the hierarchical render (run)": lambda r: r.run(RAYS, RAYS),
    "the hierarchical render (run_ops)": lambda r: r.run_ops(RAYS, RAYS),
}
COLLIDER_TEXT = ("collider overlay: {} does not draw the colliders — only the deformed path does (render_deformed / rund_cuda without perturb, and "
                 "render_continue); clear_collider_overlay() first")
POINT_TEXT = ("point overlay: {} does not draw the points — only the deformed path does (render_deformed / rund_cuda without perturb, and "
              "render_continue); clear_point_overlay() first")


@pytest.mark.parametrize("what", list(ENTRIES))
@pytest.mark.parametrize("colliders, points", [(True, False), (False, True), (True, True)])
def test_every_other_entry_point_refuses_the_overlays(what, colliders, points):
    r = NeRFRenderer(bound=1, cuda_ray=True)
    r._overlay = _colliders() if colliders else None
    r._points = _points() if points else None
    text = (COLLIDER_TEXT if colliders else POINT_TEXT).format(what)      # both set: the colliders' message comes first
    with pytest.raises(RuntimeError, match="^" + re.escape(text) + "$"):
        ENTRIES[what](r)


def test_overlay_keys_are_the_records_addresses_and_bytes():
    r = NeRFRenderer(bound=1, cuda_ray=True)
    assert r.collider_overlay_key() is None and r.point_overlay_key() is None and not r.point_overlay_reads_drag()
    ov = r._overlay = _colliders()
    assert r.collider_overlay_key() == (ov.state.data_ptr(), bytes(ov.style), 8.0)
    light = shadow_light(resolution=8)
    buf = lambda *s: torch.zeros(*s)   # noqa: E731
    sh = r._shadows = ColliderShadows(light, buf(64, 3), buf(64, 3), shadow_ws=buf(64), shadow_depth_0=buf(64), image=buf(64, 3), depth=buf(64))
    assert r.collider_overlay_key() == (ov.state.data_ptr(), bytes(ov.style), 8.0, bytes(light), sh.shadow_ws.data_ptr(), sh.shadow_depth_0.data_ptr())
    assert r.shadow_ws is sh.shadow_ws and r.shadow_depth_0 is sh.shadow_depth_0
    assert sh.out() == {"image": sh.image, "depth": sh.depth, "depth_0": sh.shadow_depth_0, "weights_sum": sh.shadow_ws}
    p = r._points = _points()
    assert r.point_overlay_key() == (None, (40.0, 41.0, 24.0, 23.0), 48, 47, bytes(p.style), None, None) and not r.point_overlay_reads_drag()
    pose, values, drag = torch.zeros(16), torch.zeros(7), torch.zeros(5, dtype=torch.float64)
    p = r._points = _points(pose=pose, values=values, drag=drag)
    assert r.point_overlay_key() == (pose.data_ptr(), (40.0, 41.0, 24.0, 23.0), 48, 47, bytes(p.style), values.data_ptr(), drag.data_ptr())
    assert r.point_overlay_reads_drag()
    with pytest.raises(AttributeError):
        p.W = 3      # the records are immutable: a changed overlay is a new record
