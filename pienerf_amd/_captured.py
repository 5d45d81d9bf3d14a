"""What a capture of the harness bakes in (Captured), what each form of the frame leaves out (refuse_form) and the last returned frame the GUI's
drag and pick read (LastFrame).  Plain values only: imports and runs without a GPU."""
from collections import namedtuple
from typing import NamedTuple

# a stage enabled after the capture: its state is device memory and is followed without a recapture, its launches must be in the graph
STAGE_NOT_CAPTURED = {
    "pins": "pin motion: {what} was captured before enable_pin_motion(), its substep ignores the pin motion: {again} again",
    "contact": "contact: {what} was captured before enable_contact(), its substep ignores the colliders: {again} again",
    "bodies": "bodies: {what} was captured before enable_bodies(), its substep does not move the balls: {again} again",
    "fields": "fields: {what} was captured before enable_fields(), its substep ignores the force fields: {again} again",
    "self": "self-contact: {what} was captured before enable_self_contact(), its substep ignores self-contact: {again} again",
    # not one of Simulator.STAGES: the contact stage's second state, reported by enabled_stage_names() while a mesh collider exists
    "mesh_colliders": "mesh colliders: {what} was captured before add_mesh_collider(), its substep ignores the mesh colliders: {again} again",
}
# kind of capture: (what the network-form error calls it, what the others call it, the call that captures it again)
_WORDS = {"graph": ("the step", "the step graph", "capture()"), "pipe": ("the pipeline", "the pipeline", "capture_pipelined()")}


class Captured(NamedTuple):
    """What a captured step or pipeline holds and does not follow: compared with the record of the current state before every replay."""
    stages: frozenset     # Simulator.enabled_stage_names(): a stage's launches (Simulator.STAGES) are in the graph or they are not
    overlay: object       # NeRFRenderer.collider_overlay_key(): the render's collider overlay, with its style (draw_colliders) and shadows
    points: object        # NeRFRenderer.point_overlay_key(): the point overlay's launch pair (draw_points)
    form_epoch: int       # pn_net_form_epoch: the network's arithmetic form is baked into every captured launch

    def check_substep(self, now, kind):
        """The network's form, then the stages; `kind`: 'graph' (capture / step_graph) or 'pipe' (capture_pipelined / step_pipelined)."""
        net, what, again = _WORDS[kind]
        if now.form_epoch != self.form_epoch:
            raise RuntimeError(f"the network's weights were refreshed into another arithmetic form (pn_net_form) since {net} was captured: its graphs "
                               f"hold the old form's kernels — capture again")
        if not now.stages <= self.stages:   # (a captured stage that is off now is no error)
            for name, msg in STAGE_NOT_CAPTURED.items():
                if name in now.stages and name not in self.stages:
                    raise RuntimeError(msg.format(what=what, again=again))

    def check_render(self, now, kind):
        """The collider overlay, then the point overlay.  Their state (colliders, positions, pose, drag) is device memory and is followed without a
        recapture; the launches, their styles, t_max, the shadows' light and the intrinsics are in the graph."""
        _, what, again = _WORDS[kind]
        if now.overlay != self.overlay:
            if self.overlay is None:
                raise RuntimeError(f"colliders: {what} was captured before draw_colliders(), its frames do not draw the colliders: {again} again")
            if now.overlay is not None and len(now.overlay) > len(self.overlay):
                raise RuntimeError(f"colliders: {what} was captured before cast_shadows(), its frames cast no shadows: {again} again")
            raise RuntimeError(f"colliders: the overlay (its state buffer, style, t_max or the shadows' light) changed since {what} was captured: {again} again")
        if now.points != self.points:
            if self.points is None:
                raise RuntimeError(f"points: {what} was captured before draw_points(), its frames do not draw the points: {again} again")
            raise RuntimeError(f"points: the point overlay (its style, intrinsics, values or drag state) changed since {what} was captured: {again} again")


# form of the frame: (what a refusal calls it, whether it draws the colliders and the points, whether it is a pipeline)
_FORMS = {"pipelined": ("the pipeline", True, True), "frame_parallel": ("the frame-parallel pipeline", False, True), "staged": ("the staged form", False, True),
          "parallel_or_staged": ("the frame-parallel / staged pipeline", False, True), "tile_parallel": ("the tile-parallel form", False, False)}


def refuse_form(form, now, shadows, bodies):
    """RuntimeError where the form `form` of the frame does not draw what is set: `now` the Captured record of the current state, `shadows` whether
    cast_shadows() is set, `bodies` whether the rigid balls are enabled."""
    what, draws, pipelined = _FORMS[form]
    if not draws and now.overlay is not None:
        raise RuntimeError(f"colliders: {what} does not draw the colliders (the other ranks / ray batches would need the collider state sent with "
                           "the DOF snapshot): step(), capture() and the single-process capture_pipelined() do; hide_colliders() first")
    if not draws and now.points is not None:
        raise RuntimeError(f"points: {what} does not draw the points (the other ranks / ray batches hold only a part of the frame the launch pair "
                           "paints onto): step(), capture() and the single-process capture_pipelined() do; hide_points() first")
    if pipelined and shadows:
        raise RuntimeError("shadows: the pipelined form casts no shadows — each lane's workspace would need a shadow workspace and map of its own "
                           "(the follow-up); step() and capture() / step_graph() do; hide_shadows() first")
    if pipelined and bodies and now.overlay is not None:
        raise RuntimeError("bodies: the pipelined form draws the live collider state, which would show a ball sim_ahead frames in front of the object "
                           "it touches; step() and capture() / step_graph() draw the balls; hide_colliders() first")


# The last returned frame, as far as drag(), move() and pick_drawn() need it.  form: "eager", "graph" or "pipelined" (None: only the points' part is
# recorded); depth_0 [H, W], pose and intrinsics are held only while the drag is enabled, point_id only while the points are drawn, ip_pos (the positions
# the frame was rendered from) for either; nothing else is kept alive
LastFrame = namedtuple("LastFrame", "form depth_0 ip_pos pose intrinsics point_id", defaults=(None,) * 6)
