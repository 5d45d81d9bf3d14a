"""Every layer of the deformed frame at once, on the 48 x 48 small chair: the background model (bg_radius = 32), the drawn colliders (floor + sphere), the
object's shadow on them, and the integration points with the drag handle of an active drag.  One blocking frame is the reference; the same frame as a
one-trip render finished by render_continue, rendered into caller-owned out_buffers, and as a captured step against the eager step all equal it bit for
bit, in every key: no arithmetic differs between the forms, only who enqueues the frame's epilogue (NeRFRenderer._finish_frame) and into which tensors.
"""
import pytest
import torch

import test_background_host as BH
import test_gpu_colliders as GC
import test_gpu_points_overlay as PO
from pienerf_amd.points_overlay import point_style
from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu
KEYS = {"image", "depth", "depth_0", "weights_sum", "coverage", "collider_t", "shadow", "point_id", "point_t"}
TARGET = (0.3, 0.4, 0.2)


def _harness(small_opt, small_cloud):
    h = GC._harness(small_opt, small_cloud, BH.bg_checkpoint(), W=48, draw=False, bg_radius=32.0)
    h.enable_drag()
    h.draw_colliders(h.style).cast_shadows(resolution=64).draw_points(point_style(radius=1, marker_radius=4, marker_thickness=2))
    return h


def _same(a, b):
    """Bit for bit (a depth is NaN where the ray misses the object's box; point_id is int32)."""
    return a.dtype == b.dtype and torch.equal(a.reshape(-1).contiguous().view(torch.int32), b.reshape(-1).contiguous().view(torch.int32))


@pytest.fixture(scope="module")
def frame(small_opt, small_cloud):
    """One harness, dragged for a few steps so that F is no identity and the handle is drawn, and its blocking frame."""
    h = _harness(small_opt, small_cloud)
    h.sim.drag_hold(h.sim.n_IP // 3, TARGET)
    for _ in range(3):
        h.step()
    h.synchronize()
    r, pose, drawn = PO._render(h)
    return h, r, pose, {k: v.clone() for k, v in drawn.items()}


def test_blocking_frame_has_every_layer(frame):
    h, r, pose, drawn = frame
    assert set(drawn) == KEYS
    image = drawn["image"].reshape(-1, 3)
    # every layer is in the picture (the sphere stands in front of a part of the chair and hides the points behind it)
    assert int(torch.isfinite(drawn["collider_t"]).sum()) > 300 and int((drawn["shadow"] > 0).sum()) > 0 and int((drawn["point_id"] >= 0).sum()) > 50
    assert int((image == torch.tensor([1.0, 0.0, 0.0], device=DEV)).all(dim=1).sum()) > 5      # the drag handle
    empty = (drawn["coverage"] == 0) & (drawn["point_id"].reshape(-1) < 0)
    assert int(empty.sum()) > 50 and len(torch.unique(image[empty], dim=0)) > 10               # the background model's colours, not one scalar


def test_one_trip_frame_finished_by_render_continue_equals_the_blocking_frame(frame):
    h, r, pose, drawn = frame
    _, _, part = PO._render(h, async_trips=1, fused_from=-1)      # one trip as launches of its own: the fused launch would run the frame to its end
    assert h.model.render_status(slot=0)["alive_at_exit"] > 0
    assert not _same(part["image"], drawn["image"])
    with torch.no_grad():
        done = h.model.render_continue(0, r["rays_o"], r["rays_d"], part, bg_color=None, **dict(h.render_kwargs(), fused_from=-1, point_pose=pose))
    torch.cuda.synchronize()
    assert h.model.last_stats["alive_at_exit"] == 0
    assert set(done) == KEYS
    for k in KEYS:
        assert _same(done[k], drawn[k]), k


def test_out_buffers_receive_every_output(frame):
    h, r, pose, drawn = frame
    N = h.opt["W"] * h.opt["H"]
    ob = {k: torch.empty((N, 3) if k == "image" else (N,), dtype=torch.int32 if k == "point_id" else torch.float32, device=DEV) for k in KEYS}
    _, _, out = PO._render(h, out_buffers=ob)
    assert set(out) == KEYS
    for k in KEYS:
        assert out[k].data_ptr() == ob[k].data_ptr(), k
        assert _same(ob[k], drawn[k]), k


def test_captured_step_equals_the_eager_step(small_opt, small_cloud):
    g = _harness(small_opt, small_cloud).capture(n_trips=8)
    g.sim.drag_hold(g.sim.n_IP // 3, TARGET)
    for _ in range(2):
        g.step_graph()
        g.finish_graph_frame()
    g.synchronize()
    dof = g.sim.dof.clone()
    out = g.step_graph()
    g.finish_graph_frame()
    g.synchronize()
    got = {k: v.clone() for k, v in out.items() if k != "_ip"}
    g.sim.dof.copy_(dof)      # an eager step() at the state that frame was rendered from
    m = g.model
    m.p_def, m.IP_F, m.IP_dF = g.sim.get_IP_info()
    want = g.step(simulate=False)
    g.synchronize()
    assert set(want) == (KEYS - {"weights_sum"}) | {"rays_o", "rays_d"} and set(want) <= set(got)
    for k in want:
        assert _same(got[k], want[k]), k
    assert int((want["image"].reshape(-1, 3) == torch.tensor([1.0, 0.0, 0.0], device=DEV)).all(dim=1).sum()) > 5
