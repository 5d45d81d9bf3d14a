"""Headless counterpart of the reference's per-frame harness.

One ``step()`` = what ``NeRFSimGUI.test_step`` -> ``Trainer.test_gui`` -> ``Trainer.test_step`` do for one GUI frame
(nerf/gui.py:556-645, nerf/trainer.py:284-329,531-602), minus the window:

    rays = get_rays(pose, intrinsics, H, W)            # trainer.py:543
    IP_pos, IP_F, IP_dF = solver.get_IP_info()         # trainer.py:303   (state BEFORE the step: render lags sim by one frame)
    model.p_def / IP_F / IP_dF = ...                   # trainer.py:304-306
    solver.stepforward()                               # trainer.py:308
    model.render_deformed(rays_o, rays_d, **vars(opt)) # trainer.py:316-318

Start-up mirrors main_gui.py:26-56.
"""
import contextlib
import gc
import os

import numpy as np
import torch

from . import scene
from .nerf.network import NeRFNetwork
from .nerf.utils import get_rays
from .simulator.solver import Simulator


@contextlib.contextmanager
def _capture(graph, **kw):
    """torch.cuda.graph with the cyclic garbage collector held off: a collection that runs DURING a stream capture may free another harness
    (workspaces, streams, graphs of an earlier capture) — hipFree / hipGraphDestroy inside a capture abort the process."""
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(graph, capture_error_mode="thread_local", **kw):
            yield
    finally:
        if was:
            gc.enable()


# pn_render_opts.throughput_trips: a trip marches in the throughput form (one lane per ray) when it has at least this many alive rays — 2048 waves,
# two per SIMD (measured: trex option set, second trip of 246 k rays: 1 191 -> 1 321 steps/s; chair, second trip of 41 k rays: 1 650 -> 1 480)
THROUGHPUT_FORM_MIN_RAYS = 131072

class SimRenderHarness:
    def __init__(self, opt=None, cloud=None, ckpt=None, device="cuda", overlap_sim=True):
        self.opt = dict(opt or scene.default_opt())
        o = self.opt
        self.device = torch.device(device)
        self.cloud = cloud if cloud is not None else scene.make_chair_points(hgs=o["hash_grid_size"], bound=o["bound"])
        self.ckpt = ckpt if ckpt is not None else scene.make_checkpoint(bound=o["bound"], bg_radius=o["bg_radius"])
        # main_gui.py:26-34
        self.model = NeRFNetwork(encoding="hashgrid", bound=o["bound"], cuda_ray=True, density_scale=1, min_near=o["min_near"],
                                 density_thresh=o["density_thresh"], bg_radius=o["bg_radius"]).to(self.device)
        self.model.load_checkpoint_dict(self.ckpt)
        self.model.eval()
        # main_gui.py:39-48
        self.sim = Simulator(dt=o["sim_dt"], iters=o["sim_iters"], bbox=torch.tensor([2.0 * o["bound"]] * 3), dx=o["sim_dx"], stiff=o["sim_stiff"],
                             base=torch.tensor([-o["bound"]] * 3), device=self.device)
        c = self.cloud
        self.sim.InitializeFromArrays(c["pos"], c["mass"], c["mu"], c["lam"], c["pin"])
        # main_gui.py:50-56
        IP_pos, IP_F, IP_dF = self.sim.get_IP_info()
        m = self.model
        m.p_ori, m.p_def, m.IP_F, m.IP_dF = IP_pos, IP_pos, IP_F, IP_dF
        m.IP_dx = self.sim.dx * 1.05
        self.frame = 0
        self.pose = scene.orbit_pose(o["radius"])
        self.intrinsics = scene.orbit_intrinsics(o["W"], o["H"], o["fovy"])
        self._pose_dev = None
        self.overlap_sim = overlap_sim
        if overlap_sim:
            self._sim_stream = torch.cuda.Stream(self.device)
            self._ip_ready = torch.cuda.Event()
            self._sim_done = torch.cuda.Event()
            self._sim_done.record(torch.cuda.current_stream(self.device))
            self.sim.force_stream = self._sim_stream  # update_force / clear_force are ordered between two substeps (solver.py:578-593)

    def synchronize(self):
        torch.cuda.synchronize(self.device)
        self._check_persistent_substep()

    def _amp(self):
        """Trainer.test_gui renders inside ``torch.cuda.amp.autocast(enabled=self.fp16)`` (trainer.py:561).  main_gui.py builds its Trainer
        without fp16 (fp32 render, the default here); opt['fp16'] = True is main_train.py's Trainer(fp16=opt.fp16) and BASELINE configs[4]:
        fp16 hash tables + half Linear layers (renderer.rund_cuda reads the autocast state)."""
        return torch.autocast("cuda", dtype=torch.float16, enabled=bool(self.opt.get("fp16", False)))

    def render_kwargs(self):
        """**vars(opt) as the reference passes it (trainer.py:318); renderer reads these by name."""
        return dict(self.opt)

    @torch.no_grad()
    def step(self, pose=None, intrinsics=None, W=None, H=None, simulate=True, collect_stats=False, fused=True, render_kw=None):
        """render_kw: options of THIS render on top of self.opt (the pipeline's probes of a launch form pass theirs here instead of editing self.opt)."""
        o = self.opt
        W, H = W or o["W"], H or o["H"]
        pose = self.pose if pose is None else pose
        intrinsics = self.intrinsics if intrinsics is None else intrinsics
        key = np.asarray(pose, np.float32).tobytes()
        if self._pose_dev is None or self._pose_dev[0] != key:  # trainer.py:541 uploads the pose every frame; re-upload only when it changes
            self._pose_dev = (key, torch.from_numpy(np.asarray(pose, np.float32)).unsqueeze(0).to(self.device))
        rays = get_rays(self._pose_dev[1], intrinsics, H, W, -1)
        m = self.model
        self._order_overlay_behind_setters()   # before this frame's substep goes onto the simulator's stream: the render still overlaps it
        if simulate:
            main = torch.cuda.current_stream(self.device)
            if self.overlap_sim:
                main.wait_event(self._sim_done)            # the previous substep must have finished before dof is read
            IP_pos, IP_F, IP_dF = self.sim.get_IP_info()
            m.p_def, m.IP_F, m.IP_dF = IP_pos, IP_F, IP_dF
            self._snapshot_colliders()   # enable_bodies(): the balls this frame draws, as the substep below finds them
            if self.overlap_sim:
                # the substep only feeds the NEXT frame (render lags sim by one frame, trainer.py:300-318), so it runs on a
                # side stream concurrently with this frame's render
                self._ip_ready.record(main)
                self._sim_stream.wait_event(self._ip_ready)
                with torch.cuda.stream(self._sim_stream):
                    self.sim.stepforward()
                    self._sim_done.record(self._sim_stream)
            else:
                self.sim.stepforward()
            self.frame += 1
        kw = self.render_kwargs()
        kw.update(render_kw or {})
        kw["collect_stats"] = collect_stats
        if m.point_overlay_key() is not None:
            kw["point_pose"] = self._pose_dev[1]   # draw_points(): the camera this frame's rays come from
        with self._amp():
            if fused:
                out = m.render_deformed(rays["rays_o"], rays["rays_d"], staged=True, bg_color=None, perturb=False, **kw)
            else:
                out = m.rund_cuda_ops(rays["rays_o"], rays["rays_d"], bg_color=None, perturb=False, **kw)
        if self.sim.drag_enabled:   # what drag() / move() unproject against (only then: without the drag nothing else is kept alive)
            self._drag_frame = ("eager", out["depth_0"].reshape(H, W), m.p_def, pose, intrinsics)
        res = {"image": out["image"].reshape(-1, H, W, 3), "depth": out["depth"].reshape(-1, H, W), "depth_0": out["depth_0"].reshape(-1, H, W),
               "rays_o": rays["rays_o"], "rays_d": rays["rays_d"]}
        res.update({k: out[k] for k in ("coverage", "collider_t", "shadow") if k in out})   # draw_colliders() / cast_shadows(): the overlay's own outputs
        if "point_id" in out:   # draw_points(): the drawn point per pixel, what pick_drawn() reads
            res.update(point_id=out["point_id"].reshape(-1, H, W), point_t=out["point_t"].reshape(-1, H, W))
            self._points_frame = (res["point_id"], m.p_def)
        return res

    # ------------------------------------------------------------------ whole step as one HIP graph
    def _step_body(self, n_trips, W, H):
        """get_rays -> get_IP_info -> { stepforward || render_deformed } with fork/join on the current stream (capturable)."""
        m = self.model
        main = torch.cuda.current_stream(self.device)
        rays = get_rays(self._graph_pose, self.intrinsics, H, W, -1)
        IP_pos, IP_F, IP_dF = self.sim.get_IP_info()
        m.p_def, m.IP_F, m.IP_dF = IP_pos, IP_F, IP_dF
        self._snapshot_colliders()   # enable_bodies(): the balls this frame draws, as the substep below finds them
        self._sim_stream.wait_stream(main)
        with torch.cuda.stream(self._sim_stream):
            self.sim.stepforward()
        kw = self.render_kwargs()
        kw["async_trips"] = n_trips
        if m.point_overlay_key() is not None:
            kw["point_pose"] = self._graph_pose
        with self._amp():
            out = m.render_deformed(rays["rays_o"], rays["rays_d"], staged=True, bg_color=None, perturb=False, **kw)
        main.wait_stream(self._sim_stream)
        # every tensor the graph touches is returned (and so stays referenced): memory freed after capture would go back to the
        # graph's pool and could be handed out again
        res = {"image": out["image"].reshape(-1, H, W, 3), "depth": out["depth"].reshape(-1, H, W), "depth_0": out["depth_0"].reshape(-1, H, W),
               "weights_sum": out["weights_sum"], "rays_o": rays["rays_o"], "rays_d": rays["rays_d"], "_ip": (IP_pos, IP_F, IP_dF)}
        res.update({k: out[k] for k in ("coverage", "collider_t", "shadow") if k in out})   # draw_colliders() / cast_shadows(): render_continue writes them again
        res.update({k: out[k] for k in ("point_id", "point_t") if k in out})   # draw_points(): flat [N], render_continue writes them again
        return res

    @torch.no_grad()
    def capture(self, n_trips=8, W=None, H=None):
        """Captures one whole step (~85 kernel launches on two streams) into a HIP graph.  `n_trips` render-loop trips are
        baked in (the chair needs 5); step_graph() verifies afterwards that no ray was left alive."""
        o = self.opt
        W, H = W or o["W"], H or o["H"]
        if not hasattr(self, "_sim_stream"):
            self._sim_stream = torch.cuda.Stream(self.device)
        self._graph_pose = torch.from_numpy(np.asarray(self.pose, np.float32)).unsqueeze(0).to(self.device)
        self._graph_pose_host = self.pose
        keep = self.sim.keep_state()
        warm = torch.cuda.Stream(self.device)
        warm.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(warm):
            for _ in range(2):  # warm-up outside capture: lazily created handles, allocator pools
                self._step_body(n_trips, W, H)
        torch.cuda.current_stream(self.device).wait_stream(warm)
        torch.cuda.synchronize(self.device)
        self._graph = torch.cuda.CUDAGraph()
        with _capture(self._graph):
            self._graph_out = self._step_body(n_trips, W, H)
        self.sim.restore_state(keep)      # warm-up advanced the simulator and its stages' clocks (the k-th replayed frame sees the clock of the k-th eager step); capture itself executes nothing
        self.sim.reset_warm_start()       # ... and its SVD warm start: a replay from here has the bits of a simulator that never warmed up
        self._graph_trips = n_trips
        self._graph_done = None
        self._graph_stages = self.sim.enabled_stage_names()   # a stage's launches (Simulator.STAGES) are in the graph or they are not
        self._graph_overlay = self.model.collider_overlay_key()   # ... and the render's collider overlay, with its style (draw_colliders)
        self._graph_points = self.model.point_overlay_key()   # ... and the point overlay's launch pair (draw_points)
        self._graph_form_epoch = self._net_form_epoch()
        return self

    def _net_form_epoch(self):
        """How often the fp32 network switched between its fp16 hi/lo and bf16 forms (include/pienerf_hip.h: pn_net_form_epoch).  The per-layer scales
        live in device memory and follow an in-place weight refresh; the form is baked into every captured launch."""
        from ._lib import lib
        net = getattr(self.model, "_net", None)
        return int(lib().pn_net_form_epoch(net)) if net is not None else 0

    def _check_net_form(self, captured, what):
        if self._net_form_epoch() != captured:
            raise RuntimeError(f"the network's weights were refreshed into another arithmetic form (pn_net_form) since {what} was captured: its graphs "
                               f"hold the old form's kernels — capture again")

    # a stage enabled after the capture: its state is device memory and is followed without a recapture, its launches must be in the graph
    _STAGE_NOT_CAPTURED = {
        "pins": "pin motion: {what} was captured before enable_pin_motion(), its substep ignores the pin motion: {again} again",
        "contact": "contact: {what} was captured before enable_contact(), its substep ignores the colliders: {again} again",
        "bodies": "bodies: {what} was captured before enable_bodies(), its substep does not move the balls: {again} again",
        "fields": "fields: {what} was captured before enable_fields(), its substep ignores the force fields: {again} again",
        "self": "self-contact: {what} was captured before enable_self_contact(), its substep ignores self-contact: {again} again",
    }

    def _check_stages_captured(self, captured, what, again):
        now = self.sim.enabled_stage_names()
        for name, msg in self._STAGE_NOT_CAPTURED.items():
            if name in now and name not in captured:
                raise RuntimeError(msg.format(what=what, again=again))

    def _check_overlay_captured(self, captured, what, again):
        """The colliders' state is device memory and is followed without a recapture; the overlay's launch, its style and t_max are in the graph."""
        now = self.model.collider_overlay_key()
        if now is not None and captured is None:
            raise RuntimeError(f"colliders: {what} was captured before draw_colliders(), its frames do not draw the colliders: {again} again")
        if now is not None and captured is not None and len(now) > len(captured):
            raise RuntimeError(f"colliders: {what} was captured before cast_shadows(), its frames cast no shadows: {again} again")
        if now != captured:
            raise RuntimeError(f"colliders: the overlay (its state buffer, style, t_max or the shadows' light) changed since {what} was captured: {again} again")

    def _check_points_captured(self, captured, what, again):
        """Positions, pose and drag state are device memory and are followed without a recapture; the launch pair, its style and the intrinsics are in
        the graph."""
        now = self.model.point_overlay_key()
        if now is not None and captured is None:
            raise RuntimeError(f"points: {what} was captured before draw_points(), its frames do not draw the points: {again} again")
        if now != captured:
            raise RuntimeError(f"points: the point overlay (its style, intrinsics, values or drag state) changed since {what} was captured: {again} again")

    def draw_points(self, style=None, markers=True):
        """From the next frame on the renders draw the simulator's integration points into the finished picture — the reference's "render IPs"
        checkbox (gui.py:533-540) — and, with `markers`, the drag handle on a dragged point (gui.py:561-569): NeRFRenderer.set_point_overlay with this
        harness's intrinsics and frame size; DESIGN.md 4.13.  `style`: a PointStyle (None: pienerf_amd.points_overlay.point_style's defaults).  The
        handle reads the simulator's drag state, so enable_drag() comes first.  Call it BEFORE capture() / capture_pipelined(): a graph captured
        without the launch pair is refused.  step, capture / step_graph and the single-process capture_pipelined draw the points, every frame those
        of the state it was rendered from; the frame-parallel, tile-parallel and staged forms raise while it is set.  The returned frames gain
        'point_id' and 'point_t'."""
        o = self.opt
        drag = self.sim._drag if (markers and self.sim.drag_enabled) else None
        self.model.set_point_overlay(None, self.intrinsics, o["W"], o["H"], style, drag_state=drag)
        return self

    def hide_points(self):
        self.model.clear_point_overlay()
        self._points_frame = None
        return self

    def _refuse_points_form(self, what):
        if self.model.point_overlay_key() is not None:
            raise RuntimeError(f"points: {what} does not draw the points (the other ranks / ray batches hold only a part of the frame the launch pair "
                               "paints onto): step(), capture() and the single-process capture_pipelined() do; hide_points() first")

    def pick_drawn(self, x, y, point_id=None, ip_pos=None):
        """An exact pick through the picture: the integration point drawn at pixel (x, y) of the last frame (column x, row y) — that one value of the
        frame's 'point_id' is read back, no search for the point nearest to an unprojected cursor — is held by the drag (Simulator.drag_hold) with its
        own position as the target; move() then pulls it.  Returns its index, or -1 where no point was drawn (the drag is left as it was).  The
        pipelined form passes the retired frame's `point_id` and the positions `ip_pos` it was rendered from."""
        if not self.sim.drag_enabled:
            raise RuntimeError("pick_drawn: call enable_drag() first (before capture() / capture_pipelined())")
        if point_id is None:
            fr = getattr(self, "_points_frame", None)
            if fr is None:
                raise RuntimeError("pick_drawn: no frame with the points drawn has been rendered yet (draw_points(), then a step)")
            if getattr(self, "_drag_frame", ("",))[0] == "graph":
                self._check_previous_graph_frame()
            point_id, ip_pos = fr[0], (fr[1] if ip_pos is None else ip_pos)
        if ip_pos is None:
            raise ValueError("pick_drawn: pass ip_pos, the integration-point positions the frame was rendered from")
        W, H = self.opt["W"], self.opt["H"]
        x, y = int(x), int(y)
        if not (0 <= x < W and 0 <= y < H):
            raise ValueError(f"pick_drawn: pixel ({x}, {y}) is outside the {W} x {H} frame")
        vid = int(point_id.reshape(-1)[y * W + x].item())
        if vid < 0:
            return -1
        self.sim.drag_hold(vid, ip_pos[vid].detach().cpu().numpy().astype(np.float64))
        return vid

    def draw_colliders(self, style=None, t_max=None):
        """From the next frame on the renders draw the simulator's colliders (NeRFRenderer.set_collider_overlay on Simulator.collider_state(); DESIGN.md
        4.11).  `style`: a ColliderStyle (None: pienerf_amd.colliders.collider_style for the colliders present now, no checker).  Call it BEFORE
        capture() / capture_pipelined(): a graph captured without the launch is refused.  step, capture / step_graph and the single-process
        capture_pipelined draw them (the pipeline draws the LIVE state: a collider moved by the host can appear up to sim_ahead frames early); the
        frame-parallel, tile-parallel and staged forms raise while an overlay is set.  ValueError before Simulator.enable_contact().  With the rigid
        balls enabled (Simulator.enable_bodies) the substep itself moves collider slots while the frame renders beside it, so the overlay then reads a
        copy of the state taken with the frame's DOF snapshot (_snapshot_colliders): frame f shows ball and object at the same substep."""
        from .colliders import collider_style
        state = self.sim.collider_state()
        self._collider_snapshot = state.clone() if self.sim.bodies_enabled else None
        self.model.set_collider_overlay(state if self._collider_snapshot is None else self._collider_snapshot,
                                        collider_style(types=self.sim.collider_types()) if style is None else style, t_max)
        return self

    def _snapshot_colliders(self):
        """With balls and an overlay: the collider state this frame draws, copied on the current stream behind the previous substep and in front of
        this frame's (one 744-byte device copy, captured with the step).  An overlay set before enable_bodies() reads the live state: it is moved
        onto a copy here, which a graph captured with the live buffer refuses as a changed overlay.  Nothing is enqueued otherwise."""
        ov = getattr(self.model, "_overlay", None)
        if ov is None or not self.sim.bodies_enabled:
            return
        live = self.sim.collider_state()
        if getattr(self, "_collider_snapshot", None) is None or ov[0] is not self._collider_snapshot:
            self._collider_snapshot = live.clone()
            self.model.set_collider_overlay(self._collider_snapshot, ov[1], ov[2])
        self._collider_snapshot.copy_(live)

    def _refuse_bodies_overlay_pipelined(self):
        if self.sim.bodies_enabled and self.model.collider_overlay_key() is not None:
            raise RuntimeError("bodies: the pipelined form draws the live collider state, which would show a ball sim_ahead frames in front of the object "
                               "it touches; step() and capture() / step_graph() draw the balls; hide_colliders() first")

    def _order_overlay_behind_setters(self):
        """set_collider's one-thread launch runs on the simulator's force stream; a frame that draws the colliders reads the state on the render's
        stream, so with an overlay that stream first waits for what the force stream holds.  Nothing is enqueued without an overlay."""
        fs = self.sim.force_stream   # ... and the drag handle of draw_points() reads the drag state, written on the same stream
        if (self.model.collider_overlay_key() is not None or self.model.point_overlay_reads_drag()) and fs is not None:
            torch.cuda.current_stream(self.device).wait_stream(fs)

    def hide_colliders(self):
        self.model.clear_collider_overlay()
        return self

    def cast_shadows(self, direction=(0.4, 1.0, 0.3), strength=0.6, resolution=256, **light_kw):
        """From the next frame on the object casts a shadow onto the drawn colliders (NeRFRenderer.set_collider_shadows): every frame
        first renders the object along the light's parallel rays into a `resolution`^2 opacity map, on the render's stream in front of the camera's
        render.  `light_kw` goes to pienerf_amd.colliders.shadow_light, which takes `bound` and `min_near` from the options.  Call it AFTER
        draw_colliders() (RuntimeError otherwise) and BEFORE capture(): a graph captured without the shadows, or with another light, is refused.
        step() and capture() / step_graph() cast them; capture_pipelined() raises while they are set."""
        from .colliders import shadow_light
        if self.model.collider_overlay_key() is None:
            raise RuntimeError("cast_shadows: the shadows fall on the drawn colliders: draw_colliders() first")
        kw = dict(bound=self.opt["bound"], min_near=self.opt["min_near"])
        kw.update(light_kw)
        self.model.set_collider_shadows(shadow_light(direction=direction, strength=strength, resolution=resolution, **kw))
        return self

    def hide_shadows(self):
        self.model.clear_collider_shadows()
        return self

    def _shadows_set(self):
        return getattr(self.model, "_shadows", None) is not None

    def _refuse_overlay_form(self, what):
        if self.model.collider_overlay_key() is not None:
            raise RuntimeError(f"colliders: {what} does not draw the colliders (the other ranks / ray batches would need the collider state sent with "
                               "the DOF snapshot): step(), capture() and the single-process capture_pipelined() do; hide_colliders() first")

    def _refuse_shadows_pipelined(self):
        if self._shadows_set():
            raise RuntimeError("shadows: the pipelined form casts no shadows — each lane's workspace would need a shadow workspace and map of its own "
                               "(the follow-up); step() and capture() / step_graph() do; hide_shadows() first")

    @torch.no_grad()
    def step_graph(self, pose=None):
        """Replays the captured step.  Outputs are static tensors (overwritten by the next replay); they are complete — including frames
        that needed more trips than were captured — after the NEXT call or ``finish_graph_frame()``."""
        if getattr(self, "_graph", None) is None:
            self.capture()
        self._check_net_form(self._graph_form_epoch, "the step")
        self._check_stages_captured(self._graph_stages, "the step graph", "capture()")
        self._check_overlay_captured(self._graph_overlay, "the step graph", "capture()")
        self._check_points_captured(getattr(self, "_graph_points", None), "the step graph", "capture()")
        self._check_previous_graph_frame()
        if pose is not None:
            self._graph_pose.copy_(torch.from_numpy(np.asarray(pose, np.float32)).unsqueeze(0))
        self._order_overlay_behind_setters()
        self._graph.replay()
        self._graph_done = torch.cuda.Event()
        self._graph_done.record(torch.cuda.current_stream(self.device))
        self.frame += 1
        if pose is not None:
            self._graph_pose_host = pose
        if "drag" in self._graph_stages:
            g = self._graph_out
            self._drag_frame = ("graph", g["depth_0"][0], g["_ip"][0], self._graph_pose_host, self.intrinsics)
        else:
            self._drag_frame = ("graph",)
        if "point_id" in self._graph_out:
            self._points_frame = (self._graph_out["point_id"], self._graph_out["_ip"][0])
        return self._graph_out

    def finish_graph_frame(self):
        """Waits for the last replayed step and completes it; returns its outputs."""
        self._check_previous_graph_frame()
        return self._graph_out

    def _check_previous_graph_frame(self):
        """The captured step bakes in a trip count; a frame that still had rays alive after them is finished here with further trips (the
        reference's loop just keeps going, renderer.py:836-891) before its outputs are handed on."""
        if getattr(self, "_graph_done", None) is not None:
            self._graph_done.synchronize()  # normally long complete: the host only ever runs one frame ahead
            st = self.model.render_status(synchronize=False)
            alive = st["alive_at_exit"]
            if self._shadows_set():   # the shadow pass is in the graph too, on a workspace of its own: render_continue finishes it first, then the frame
                alive += self.model.render_status(synchronize=False, slot=self.model.SHADOW_SLOT)["alive_at_exit"]
                self.model.last_stats = st
            self._graph_done = None
            if alive > 0:
                g = self._graph_out
                if self.model.point_overlay_key() is not None:
                    self.model.p_def, self.model.IP_F, self.model.IP_dF = g["_ip"]   # the point overlay paints the state this frame was rendered from
                with self._amp():
                    self.model.render_continue(0, g["rays_o"], g["rays_d"], g, bg_color=None, **dict(self.render_kwargs(), point_pose=self._graph_pose))
                self.graph_continued = getattr(self, "graph_continued", 0) + 1

    # ------------------------------------------------------------------ several frames in flight (one GPU, or frame-parallel over a node)
    def _cu_masked_stream(self, first_cu, n_cu, invert):
        import ctypes

        from ._lib import check, lib
        total = lib().pn_device_cu_count()
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            check(lib().pn_stream_create_cu_mask(total, first_cu, n_cu, int(invert), ctypes.byref(h)), "stream_create_cu_mask")
        self._raw_streams = getattr(self, "_raw_streams", []) + [h.value]
        return torch.cuda.ExternalStream(h.value, device=self.device)

    @torch.no_grad()
    def capture_pipelined(self, lanes=2, n_trips=8, W=None, H=None, sim_ahead=None, depth=2, sim_priority=0, sim_cus=0, copy_out=True, group=None,
                          frame_parallel=False, sim_owner=0, dedicated_sim=None, on_retire=None, copy_on="host", _probe_no_substep=False, _time_trips=False,
                          render_kw=None, _force_collectives=False, sim_on_lanes=False):
        """Throughput mode (pienerf_amd/frames.py: FramePipeline): `lanes` render streams with `depth` workspaces each, the simulator running
        `sim_ahead` frames ahead on dof snapshots, every frame's image / depth / depth_0 copied to pinned host memory (the reference's
        device->host boundary, trainer.py:589-592; copy_out=False leaves the results on the device) — copy_on="host": by the library's copier
        thread through the HSA runtime's SDMA engine, no stream involved (csrc/pn_copier.hip; "lane" / "copy" / "sim": as a hipMemcpyAsync
        on the frame's render stream / a stream of its own / the simulator stream).  Everything a frame
        launches is captured in HIP graphs — one for the substep, one per workspace for get_rays + the render with `n_trips` loop trips
        (None: measured on one eager frame, + 2); a frame that still has rays alive after its trips is continued when it is retired
        (renderer.py:836-891).  frame_parallel=True (or ``capture_frame_parallel``): the same pipeline over the ranks of `group` — the sim
        owner broadcasts every snapshot (<= 82 KB) over RCCL, rank frames.frame_owner(f) renders frame f.

        ``step_pipelined(pose=None)`` enqueues the next frame (with its own camera pose, trainer.py:541) and returns the frames it retired:
        [(frame index, {'image','depth','depth_0': numpy views of the pinned buffers, 'device': the device tensors})]; a frame comes back
        lanes*depth steps after it went in, ``drain_pipeline()`` returns the rest.  The numpy arrays stay valid for another lanes*depth steps
        (two pinned sets per workspace alternate); the device tensors are the graph's static outputs and are overwritten by the workspace's
        next frame, i.e. any time after this call returns: a consumer of the device copy hooks in with on_retire(frame, result), which runs
        when the frame is complete and before its workspace is handed to the next frame.  Every frame is rendered from the state before its own
        substep (trainer.py:300-318); ``self.sim.dof`` is `sim_ahead + 1` substeps in front of the last enqueued frame, and a force set with
        update_force() acts from the next substep that is enqueued (it is ordered on the simulator's stream)."""
        import torch.distributed as dist

        from .frames import FramePipeline
        if frame_parallel:
            self._refuse_overlay_form("the frame-parallel pipeline")
            self._refuse_points_form("the frame-parallel pipeline")
        if (render_kw or {}).get("ray_batch"):
            self._refuse_overlay_form("the staged form")
            self._refuse_points_form("the staged form")
        self._refuse_shadows_pipelined()
        self._refuse_bodies_overlay_pipelined()
        o = self.opt
        W, H = W or o["W"], H or o["H"]
        on = bool(frame_parallel) and dist.is_available() and dist.is_initialized()
        world = dist.get_world_size(group) if on else 1
        rank = dist.get_rank(group) if on else 0
        if n_trips is None:  # calibrate: the trips one eager frame needs from the current state and pose, plus a margin
            self.step(simulate=False, collect_stats=True, W=W, H=H)
            n_trips = int(self.model.last_stats["trips"]) + 2  # every captured trip costs five launches whether it has rays or not
        from .frames import dedicated_sim_default
        if (world > 1 and (dedicated_sim_default(world) if dedicated_sim is None else bool(dedicated_sim)) and rank == sim_owner
                and dist.get_backend(group) == "nccl" and os.environ.get("PN_SIM_COOP", "") == "1"):
            # this GPU only simulates: with PN_SIM_COOP=1 the substep's local/global iterations run as one persistent kernel on (almost) every CU
            # (csrc/pn_sim_coop.h: k_substep_coop; 0.24 instead of 0.28 ms).  Opt-in: it has never run beside RCCL's kernels (one-GPU test box), and a
            # persistent kernel that cannot get all its CUs ends with a flag and an invalid state instead of a slower step.  Never beside renders:
            # its workgroups and those of the fused composite/compaction would wait for each other.  (A gloo group is the one-GPU dry run.)
            self.sim.enable_persistent()
        be = _HipBackend(self, lanes, depth, int(n_trips), W, H, sim_priority, sim_cus, copy_out, group if on else None,
                         (dist.get_global_rank(group, sim_owner) if (on and group is not None) else sim_owner), _probe_no_substep, _time_trips, copy_on,
                         render_kw=render_kw, distributed=on)
        self._pipe = FramePipeline(be, world=world, rank=rank, lanes=lanes, depth=depth, ahead=(lanes if sim_ahead is None and world == 1 else sim_ahead),
                                   sim_owner=sim_owner, dedicated_sim=dedicated_sim, copy_out=copy_out, on_retire=on_retire,
                                   force_collectives=bool(_force_collectives) and on, sim_on_lanes=sim_on_lanes)
        self.sim.force_hooks = (self._pipe.before_force, self._pipe.after_force) if self._pipe.sim_on_lanes else None
        self._pipe_stages = self.sim.enabled_stage_names()
        self._pipe_overlay = self.model.collider_overlay_key()
        self._pipe_points = self.model.point_overlay_key()
        self._pipe_single = not frame_parallel and not (render_kw or {}).get("ray_batch")
        self._drag_frame = ("pipelined",)
        self._pipe_backend = be
        self._pipe_form_epoch = self._net_form_epoch()
        self.model._in_flight = lambda pipe=self._pipe: sum(f is not None for f in pipe.pending)  # weight refreshes need a drained pipeline (network._net_handle)
        return self

    def capture_frame_parallel(self, lanes=2, n_trips=8, group=None, sim_owner=0, dedicated_sim=None, **kw):
        """Multi-GPU form (BASELINE.json configs[3]): every rank calls step_frame_parallel() once per GLOBAL frame."""
        return self.capture_pipelined(lanes=lanes, n_trips=n_trips, group=group, frame_parallel=True, sim_owner=sim_owner, dedicated_sim=dedicated_sim, **kw)

    @torch.no_grad()
    def step_pipelined(self, pose=None):
        self._check_net_form(self._pipe_form_epoch, "the pipeline")
        self._check_stages_captured(self._pipe_stages, "the pipeline", "capture_pipelined()")
        if not getattr(self, "_pipe_single", True):
            self._refuse_overlay_form("the frame-parallel / staged pipeline")
            self._refuse_points_form("the frame-parallel / staged pipeline")
        self._refuse_shadows_pipelined()
        self._refuse_bodies_overlay_pipelined()
        self._check_overlay_captured(getattr(self, "_pipe_overlay", None), "the pipeline", "capture_pipelined()")
        self._check_points_captured(getattr(self, "_pipe_points", None), "the pipeline", "capture_pipelined()")
        out = self._pipe.step(pose)
        self.frame = self._pipe.frame
        return out

    step_frame_parallel = step_pipelined

    @property
    def substeps_enqueued(self):
        """Simulator substeps enqueued so far in pipelined mode (= frames enqueued + sim_ahead once running)."""
        return self._pipe.substeps_enqueued

    @torch.no_grad()
    def drain_pipeline(self):
        """Retires every frame in flight (continuing any that ran out of trips) and returns them; the device is idle afterwards."""
        out = self._pipe.drain()
        torch.cuda.synchronize(self.device)
        self._check_persistent_substep()
        return out

    def wait_frame_copies(self):
        """Pipelined mode: host-waits for the device AND for the copier thread's frame copies (which are on no stream)."""
        torch.cuda.synchronize(self.device)
        be = getattr(self, "_pipe_backend", None)
        if be is not None and hasattr(be, "wait_copies"):
            be.wait_copies()

    @torch.no_grad()
    def verify_last_frame(self):
        """After drain_pipeline(): renders the LAST frame this rank's pipeline enqueued once more — a blocking render, launch by launch, from the
        integration-point state and pose its workspace still holds — and compares it bit for bit with what the pipeline delivered (the arrays in
        pinned host memory when the frames are copied out, else the workspace's device buffers).  Every form of the frame (captured graph, several
        frames in flight, fused launches, one lane per ray or windows) produces the same bits by construction; a difference means a race between the
        pipeline's streams, a frame copied before it was finished, or a broken kernel.  Returns dict(ok, frame, max_abs_diff)."""
        pipe, be, m = self._pipe, self._pipe_backend, self.model
        ws = pipe.last_ws
        if ws is None:
            return {"ok": False, "frame": None, "why": "no frame was enqueued"}
        torch.cuda.synchronize(self.device)
        res = be.result(ws)
        keep = (m.p_def, m.IP_F, m.IP_dF)
        try:
            m.p_def, m.IP_F, m.IP_dF = be.ip[ws]
            rays = get_rays(be.pose_dev[ws], self.intrinsics, be.H, be.W, -1)
            kw = dict(self.render_kwargs())
            kw.pop("ray_batch", None)
            if be.kw.get("ray_batch"):
                kw["ray_batch"] = be.kw["ray_batch"]   # batches keep their own trip schedules: part of what the frame IS, not of how it is launched
            if m.point_overlay_key() is not None:
                kw["point_pose"] = be.pose_dev[ws]
            with self._amp():
                out = m.render_deformed(rays["rays_o"], rays["rays_d"], staged=True, bg_color=None, perturb=False, **kw)
            torch.cuda.synchronize(self.device)
            worst, ok = 0.0, True
            for k in ("image", "depth_0"):
                want = out[k].reshape(-1).cpu().numpy()
                got = (res[k] if k in res else res["device"][k].cpu().numpy()).reshape(-1)
                ok = ok and bool(np.array_equal(want, got))
                worst = max(worst, float(np.abs(want - got).max()))
        finally:
            m.p_def, m.IP_F, m.IP_dF = keep
        return {"ok": ok, "frame": int(pipe.last_frame), "max_abs_diff": worst}

    def _check_persistent_substep(self):
        """A persistent substep whose workgroups could not all become resident ends with a flag instead of hanging (csrc/pn_sim_coop.h); its DOFs
        are garbage.  Checked where the host synchronises anyway."""
        if self.sim.persistent and self.sim.persistent_timed_out():
            raise RuntimeError("the persistent substep (pn_sim_stepforward_coop) timed out at a device-wide barrier: the simulator state is invalid "
                               "(another kernel held CUs for seconds, or two persistent substeps ran at once); use Simulator(persistent=False)")

    # ------------------------------------------------------------------ one frame split over the ranks (interactive latency)
    @torch.no_grad()
    def capture_tile_parallel(self, group=None, sim_owner=0, tile=8, W=None, H=None, _force_collectives=False):
        """Ray-tile-parallel form ("alternative for interactive latency"; frames.TileParallel): every rank renders an
        interleaved 1/world of the 8 x 8 pixel tiles of the SAME frame from the sim owner's broadcast DOF snapshot, and one all-gather
        (20 B x N / world per rank over RCCL) gives every rank the whole frame.  Unlike the frame-parallel pipeline, whose throughput is
        capped by the time-sequential simulator, this divides the render LATENCY of a frame by the rank count.  Launches are eager."""
        from .frames import TileParallel
        self._refuse_overlay_form("the tile-parallel form")
        self._refuse_points_form("the tile-parallel form")
        o, m, dev = self.opt, self.model, self.device
        W, H = W or o["W"], H or o["H"]
        ip = tuple(torch.empty((self.sim.n_IP, c), dtype=torch.float32, device=dev) for c in (3, 9, 27))
        self._tile_pose = torch.from_numpy(np.asarray(self.pose, np.float32)).unsqueeze(0).to(dev)

        def render_subset(idx):
            rays = get_rays(self._tile_pose, self.intrinsics, H, W, -1)
            sel = idx.clamp(min=0)
            self.sim.get_IP_info(out=ip)
            m.p_def, m.IP_F, m.IP_dF = ip
            with self._amp():
                out = m.render_deformed(rays["rays_o"][:, sel].contiguous(), rays["rays_d"][:, sel].contiguous(), bg_color=None, perturb=False, frame_slot=800,
                                        **self.render_kwargs())
            return torch.cat([out["image"].view(-1, 3), out["depth"].view(-1, 1), out["depth_0"].view(-1, 1)], dim=1)

        def set_dof(t):
            self.sim.dof.copy_(t)
        self._tile = TileParallel(W, H, render_subset, lambda: self.sim.dof, set_dof, self.sim.stepforward, sim_owner=sim_owner, group=group, tile=tile, device=dev,
                                  force_collectives=_force_collectives)
        self._tile_WH = (W, H)
        return self

    @torch.no_grad()
    def step_tile_parallel(self, pose=None):
        """One sim+render step; every rank gets the full frame: {'image' [1,H,W,3], 'depth' [1,H,W], 'depth_0' [1,H,W]} on the device."""
        self._refuse_overlay_form("the tile-parallel form")
        self._refuse_points_form("the tile-parallel form")
        if pose is not None:
            self._tile_pose.copy_(torch.from_numpy(np.asarray(pose, np.float32)).view(1, 4, 4).to(self.device))
        full = self._tile.step()
        W, H = self._tile_WH
        self.frame += 1
        return {"image": full[:, :3].reshape(1, H, W, 3), "depth": full[:, 3].reshape(1, H, W), "depth_0": full[:, 4].reshape(1, H, W)}

    # ------------------------------------------------------------------ a frame rendered in ray batches (BASELINE.json configs[4])
    def capture_staged(self, batch=None, **kw):
        """The frame rendered in ray batches of `batch` rays (opt max_ray_batch = 4096, get_opts.py:24; renderer.py:562-576's staging loop):
        every batch keeps its own trip schedule (n_step = max(min(N_b // n_alive_b, 8), 1), its own max_steps count), exactly as if the
        batches were rendered one after the other — but all batches advance inside the same launches (pn_render_opts.ray_batch: rays are
        independent, the alive list stays sorted by ray id, a batch is a contiguous run of it).  So the staged frame IS a pipelined frame:
        same graphs, same lanes, same D2H; `kw` goes to capture_pipelined, frames come back through step_pipelined() / drain_pipeline().
        (Rounds 1-2 replayed one captured launch chain per batch: ~10 000 launches per 800x800 frame, 20x slower than the frame in one piece.)"""
        rk = dict(kw.pop("render_kw", None) or {}, ray_batch=int(batch or self.opt.get("max_ray_batch", 4096)))  # this pipeline's renders only: self.opt stays as it was
        return self.capture_pipelined(render_kw=rk, **kw)

    # names of rounds 1-2 (one captured launch chain per batch), kept as aliases of the pipeline's calls
    def step_staged(self, pose=None):
        return self.step_pipelined(pose)

    def finish_staged(self):
        return self.drain_pipeline()

    # ------------------------------------------------------------------ the GUI's mouse drag (gui.py:556-586, :833-841)
    def enable_drag(self, scale=None):
        """Simulator.enable_drag: every substep from now on gets the GUI's spring force toward the cursor, computed on the device from the state that
        substep starts from.  Call it BEFORE capture() / capture_pipelined(): a graph captured without it has no drag launch and refuses drag()."""
        self.sim.enable_drag(scale)
        return self

    def _drag_check(self):
        if not self.sim.drag_enabled:
            raise RuntimeError("drag: call enable_drag() first (before capture() / capture_pipelined())")
        mode = getattr(self, "_drag_frame", None)
        if mode is None:
            raise RuntimeError("drag: no frame has been rendered yet (the cursor is unprojected against the last frame's depth_0)")
        if mode[0] == "graph" and not self._graph_drag:
            raise RuntimeError("drag: the step graph was captured before enable_drag(), its substep ignores the drag state: capture() again")
        if mode[0] == "pipelined" and not self._pipe_drag:
            raise RuntimeError("drag: the pipeline was captured before enable_drag(), its substep ignores the drag state: capture_pipelined() again")
        return mode

    def _drag_inputs(self, depth0, ip_pos, pick):
        mode = self._drag_check()
        if mode[0] == "pipelined":
            # the caller hands in the last RETIRED frame's depth_0: the cursor is then unprojected against an image `lanes * depth` frames older than
            # the state the next substep reads — inherent to the pipeline.  The pick searches the IPs of the simulator's newest state.
            if depth0 is None:
                raise ValueError("drag in the pipelined form: pass depth0, the depth_0 of the last frame step_pipelined() returned")
            depth0 = torch.as_tensor(depth0).to(self.device, torch.float32).contiguous()
            if pick and ip_pos is None:
                with self.sim._on_force_stream():
                    ip_pos = self.sim.get_IP_info()[0]
            return depth0, ip_pos, self.pose, self.intrinsics
        if mode[0] == "graph":
            self._check_previous_graph_frame()   # a frame left with rays alive is finished before its depth_0 is read
        return (mode[1] if depth0 is None else depth0), (mode[2] if ip_pos is None else ip_pos), mode[3], mode[4]

    def drag(self, x, y, depth0=None, ip_pos=None):
        """A ctrl-click at image pixel (x, y) (gui.py:833-841): picks the integration point nearest to the unprojected cursor among the IP positions
        the last returned frame was rendered from, against that frame's depth_0 and camera; the drag then acts from the next substep on.  Returns
        the picked IP.  (x, y) are image pixels: a window's own offsets, as dearpygui's +20 title bar (gui.py:809-812), are the caller's."""
        d, ip, pose, intr = self._drag_inputs(depth0, ip_pos, True)
        return self.sim.drag_pick(d, x, y, pose, intr, ip)

    def move(self, x, y, depth0=None):
        """The cursor moved to (x, y): the spring's target is unprojected against the last returned frame's depth_0 (gui.py:578).  No host read."""
        d, _, pose, intr = self._drag_inputs(depth0, None, False)
        self.sim.drag_to(d, x, y, pose, intr)

    def release(self):
        """Nothing picked any more: the following substeps run without force (the GUI's clear_force)."""
        self._drag_check()
        self.sim.release()

    def to_host(self, out):
        """The reference's device->host boundary (trainer.py:589-592)."""
        return {k: out[k][0].detach().cpu().numpy() for k in ("image", "depth", "depth_0")}


# h._graph_fields, h._pipe_drag, ...: whether the stage's launches are in the step graph / the pipeline's substep graph (False before a capture)
for _form in ("_graph", "_pipe"):
    for _st in Simulator.STAGES:
        setattr(SimRenderHarness, f"{_form}_{_st.name}", property(lambda self, _f=_form + "_stages", _n=_st.name: _n in getattr(self, _f, ())))


class _HipStream:
    def __init__(self, s):
        self.s = s

    def wait(self, ev):
        self.s.wait_event(ev.e)


class _HostCopyStream:
    """Stands where frames.FramePipeline expects the stream of the frame copies when they are done by the library's host-side copier
    (pn_copier, copy_on="host"): `wait(event)` names the event the next copy has to follow, `_HipBackend.copy_out` submits the copy behind it,
    an event `recorded` here carries the copy's ticket and can only be waited for by the host (which is all the pipeline does with it)."""

    def __init__(self, backend):
        self.backend, self.after, self.ticket = backend, None, None

    def wait(self, ev):
        self.after = ev


class _HipEvent:
    def __init__(self):
        self.e = torch.cuda.Event()
        self.copy = None  # (copier handle, ticket) when the event marks the end of a host-side frame copy

    def record(self, stream):
        if isinstance(stream, _HostCopyStream):
            self.copy = (stream.backend.copier, stream.ticket)
        else:
            self.copy = None
            self.e.record(stream.s)

    def host_wait(self):
        if self.copy is not None:
            from ._lib import check, lib
            check(lib().pn_copier_wait(self.copy[0], self.copy[1]), "copier_wait")
        else:
            self.e.synchronize()


class _HipBackend:
    """The device side of frames.FramePipeline on one MI355X: torch streams and events, the substep and one render per workspace captured
    as HIP graphs, RCCL broadcasts of the dof snapshots, D2H into pinned buffers."""

    def __init__(self, h, lanes, depth, n_trips, W, H, sim_priority, sim_cus, copy_out, group, src, probe_no_substep, time_trips=False, copy_on="host",
                 render_kw=None, distributed=False):
        # stream of the per-frame D2H.  gfx950 runs 4 hardware queues concurrently and time-slices beyond that: with 3 render lanes +
        # the simulator stream a copy stream of its own is a fifth busy queue (measured: 808 steps/s against 1016 with the copy on the frame's own
        # lane).  "copy": a stream of its own; "lane": the frame's render stream; "sim": the simulator stream; "host": no stream at all — the
        # library's copier thread waits for the render's event and hands the copy to the HSA runtime (SDMA), see csrc/pn_copier.hip
        self.copy_on = copy_on
        self.copier = None
        if copy_on == "host" and copy_out:
            import ctypes

            from ._lib import check, lib
            hc = ctypes.c_void_p()
            check(lib().pn_copier_create(ctypes.byref(hc)), "copier_create")
            self.copier = hc
        self.h, self.lanes, self.depth, self.trips, self.W, self.H, self.group, self.src = h, lanes, depth, n_trips, W, H, group, src
        dev, m, sim = h.device, h.model, h.sim
        self.continued = 0
        if sim_cus > 0:
            # compute-unit partition: the substep's chain of small dependent launches gets `sim_cus` CUs of its own (spread over the XCDs),
            # the render lanes the rest, so a substep never waits for a render wave to release registers
            self._streams = {"sim": h._cu_masked_stream(0, sim_cus, invert=False)}
            lane_streams = [h._cu_masked_stream(0, sim_cus, invert=True) for _ in range(lanes)]
        elif sim_cus < 0:
            # the converse: the render lanes stay off -sim_cus CUs, the simulator may use every CU — its launches always find those free, and whatever else is
            self._streams = {"sim": torch.cuda.Stream(dev, priority=sim_priority)}
            lane_streams = [h._cu_masked_stream(0, -sim_cus, invert=True) for _ in range(lanes)]
        else:
            self._streams = {"sim": torch.cuda.Stream(dev, priority=sim_priority)}
            lane_streams = [torch.cuda.Stream(dev) for _ in range(lanes)]
        for i, s in enumerate(lane_streams):
            self._streams[f"lane{i}"] = s
        self._streams["comm"], self._streams["copy"] = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
        sim.force_stream = self._streams["sim"]   # a force change is enqueued between two substeps of the simulator stream
        self.snap = {}
        n_ws, n_IP = lanes * depth, sim.n_IP
        self.consumer_done = [None] * n_ws   # per workspace: the event behind what on_retire enqueued on its stream (consumer_fence)
        kw = dict(h.render_kwargs(), async_trips=n_trips)
        kw.update(render_kw or {})  # options of THIS pipeline's renders (capture_staged: ray_batch)
        # several frames in flight: the first trip's march pass in its throughput form (pn_render_opts.throughput: one lane per ray, no speculative
        # evaluation; the same samples bit for bit, +8 % steps/s with three lanes) — with one lane the frame's own latency is what counts
        kw.setdefault("march_throughput", 64 if lanes > 1 else 0)
        # ... and each frame's fused launch (pn_render_opts.fused_from) on half of the CUs: the launches of the frames in flight run side by side and the
        # other kernels find CUs with free LDS (pn_render_opts.fused_grid; three lanes on the chair: 1 721 -> 1 937 steps/s)
        if lanes > 1:
            cus = torch.cuda.get_device_properties(dev).multi_processor_count
            kw.setdefault("fused_grid", max(cus * 5 // 8 if lanes == 2 else cus // 2, 1))   # (two lanes, whole-frame launches: 128 / 160 / 192 workgroups: 1 717 / 1 776 / 1 689 steps/s)
        self.kw = kw
        if "fused_from" not in kw:
            # pn_render_opts.fused_from: the loop trips from the first one with n_step == 8 on (n_alive <= N / 8: it stays 8 for the rest of the frame) run
            # as ONE persistent launch (csrc/pn_trips_fused.h) — read off the trip records of a blocking frame from the current state and pose.  A later
            # frame that still has more rays alive at that trip is finished when it is retired (frames.FramePipeline: continue), only slower
            h.step(simulate=False, collect_stats=True, W=W, H=H)
            recs = m.trip_records(slot=0, max_trips=64)
            kw["fused_from"] = next((i for i, r in enumerate(recs) if i >= 1 and r[1] == 8), -1) if not kw.get("ray_batch") else -1
        if "fused_whole" not in kw:
            # pn_render_opts.fused_whole: the frame's first trip in that launch too (where at most N / 8 rays have anything to march: the blocking frame
            # below tries it and reports the trip at which the fused launch took over).  Measured on the chair: better with two frames in flight
            # (1 700-1 740 against 1 560 steps/s), worse with three (1 730 against 1 930) or one at a time — include/pienerf_hip.h
            whole = lanes == 2 and kw["fused_from"] == 1
            if whole:
                h.step(simulate=False, collect_stats=True, W=W, H=H, render_kw=dict(kw, fused_whole=True, fused_from=0, async_trips=0))
                whole = m.fused_clocks(slot=0)["first_trip"] == 0
            kw["fused_whole"] = bool(whole)
            if whole:
                kw["fused_from"] = 0
        if "fused_fold" not in kw:
            # pn_render_opts.fused_fold: the first trip's network, composite and compaction inside the fused launch (its march stays launches of its own): four
            # launches fewer on a lane's chain.  Where the blocking frame below finds it applicable (at most N / 8 rays with a sample on the first trip)
            # (measured on the chair, alternating runs on one box: three lanes 1 960 against 1 925 steps/s, --steps 20: 1 801 against 1 790; one frame at a
            # time the launch with the first trip's tiles in front of its rounds is longer than what it replaces, 0.884 against 0.859 ms per step)
            # — that against the launch drawing its rays in list order.  Drawing each workgroup's longest packets first (pn_render_opts.fused_order, the
            # default) shortens the launch whose rays come from the alive list by 5-6 %, and does nothing for the folded one, whose rays are listed while it
            # runs: three lanes 1 503-1 508 against 1 483-1 486 steps/s on one box (EXPERIMENTS.md, "After round 6").  So: folded only in list order
            ordered = kw.get("fused_order") is None or bool(kw.get("fused_order"))
            fold = lanes >= 3 and (not kw.get("fused_whole")) and kw["fused_from"] == 1 and not ordered
            if fold:
                h.step(simulate=False, collect_stats=True, W=W, H=H, render_kw=dict(kw, fused_fold=True, async_trips=0))
                fold = m.fused_clocks(slot=0)["mode"] == 2
            kw["fused_fold"] = bool(fold)
        if distributed:
            # every rank of a frame-parallel job runs the launch form rank `src` picked (each probed its own warm-up frame: the same state and pose, but
            # nothing guarantees the same answer at a threshold) — round-4 advisor; gated on the job being distributed, NOT on `group`: the default
            # process group is group=None (round-5 advisor: with `if group is not None` this never ran in a real job)
            from .frames import agree_on_launch_form
            agree_on_launch_form(kw, src=src, group=group, device=dev)
        pose0 = torch.from_numpy(np.asarray(h.pose, np.float32)).unsqueeze(0)
        self.pose_dev = [pose0.to(dev) for _ in range(n_ws)]
        self.pose_pin = [pose0.clone().pin_memory() for _ in range(n_ws)]
        self.pose_key = [pose0.numpy().tobytes()] * n_ws
        self.ip = [tuple(torch.empty((n_IP, c), dtype=torch.float32, device=dev) for c in (3, 9, 27)) for _ in range(n_ws)]
        keep = sim.keep_state()
        main = torch.cuda.current_stream(dev)
        for ws in range(n_ws):  # warm-up of every workspace outside capture (creates the pn_frame workspaces, the fp16 tables, ...)
            s = self._streams[f"lane{ws // depth}"]
            s.wait_stream(main)
            with torch.cuda.stream(s):
                for _ in range(2):
                    sim.get_IP_info(out=self.ip[ws])
                    sim.stepforward()
                    m.p_def, m.IP_F, m.IP_dF = self.ip[ws]
                    rays = get_rays(self.pose_dev[ws], h.intrinsics, H, W, -1)
                    with h._amp():
                        m.render_deformed(rays["rays_o"], rays["rays_d"], staged=True, bg_color=None, perturb=False, **self._ws_kw(ws))
            torch.cuda.synchronize(dev)
            if ws == 0 and kw.get("march_throughput") and "march_throughput_trips" not in kw:
                # the throughput form for every leading trip that still has rays enough to fill the GPU with ONE lane per ray (the trex option set's
                # second trip: 246 k rays x 3 samples; the chair's: 41 k x 8, faster in the windows) — from this warm-up frame's trip records; the
                # samples do not depend on the form, so a scene that changes later only loses speed
                n_lpr = 1
                for rec in m.trip_records(slot=0)[1:]:
                    if rec[0] < THROUGHPUT_FORM_MIN_RAYS:
                        break
                    n_lpr += 1
                kw["march_throughput_trips"] = n_lpr
        # capture_error_mode="thread_local": with a process group alive, RCCL's watchdog thread queries events while we capture;
        # in the default "global" mode any HIP call from another thread invalidates the capture
        self.sim_graph = torch.cuda.CUDAGraph()
        with _capture(self.sim_graph, stream=self._streams["sim"]):
            if not probe_no_substep:
                sim.stepforward()
            else:
                sim.dof_vel.mul_(1.0)
        self.graph, self.rays, self.out, self.host, self.packed = [], [], [], [], []
        N = W * H
        for ws in range(n_ws):
            s = self._streams[f"lane{ws // depth}"]
            m.p_def, m.IP_F, m.IP_dF = self.ip[ws]  # the render graph of this workspace reads its own IP buffers
            if time_trips:  # measurement (bench.py): time stamps around each trip's march / network launches become nodes of the captured graph
                m.march_counters(2, slot=ws)
            # image | depth | depth_0 packed in one device buffer -> ONE device-to-host copy per frame (20 B per pixel, trainer.py:589-592)
            pk = torch.empty(N * 5, dtype=torch.float32, device=dev)
            ob = {"image": pk[:3 * N].view(N, 3), "depth": pk[3 * N:4 * N], "depth_0": pk[4 * N:], "weights_sum": torch.empty(N, dtype=torch.float32, device=dev)}
            g = torch.cuda.CUDAGraph()
            with _capture(g, stream=s):
                rays = get_rays(self.pose_dev[ws], h.intrinsics, H, W, -1)
                with h._amp():
                    out = m.render_deformed(rays["rays_o"], rays["rays_d"], staged=True, bg_color=None, perturb=False, out_buffers=ob, **self._ws_kw(ws))
            self.graph.append(g)
            # every tensor the graphs touch stays referenced: a tensor freed after capture goes back to the graph's memory pool
            self.rays.append(rays)
            self.out.append(out)
            self.packed.append(pk)
            # two pinned sets per workspace, used alternately: the arrays handed out when a frame is retired stay valid until the workspace has
            # been through another whole frame (the next frame's D2H goes into the other set)
            self.host.append([torch.empty(N * 5, dtype=torch.float32).pin_memory() for _ in range(2)] if copy_out else None)
        self.host_gen = [0] * n_ws
        torch.cuda.synchronize(dev)
        if self.copier is not None:
            # the first SDMA copy into a pinned buffer maps it for the engine (milliseconds): once per buffer here, not inside the pipeline's first frames
            import ctypes

            from ._lib import check, lib
            for ws in range(n_ws):
                for hb in self.host[ws]:
                    t = ctypes.c_uint64()
                    check(lib().pn_copier_submit(self.copier, ctypes.c_void_p(hb.data_ptr()), ctypes.c_void_p(self.packed[ws].data_ptr()),
                                                 hb.numel() * hb.element_size(), None, ctypes.byref(t)), "copier_submit")
                    check(lib().pn_copier_wait(self.copier, t.value), "copier_wait")
        sim.restore_state(keep)    # warm-up advanced the simulator and its stages' clocks; capture itself executes nothing
        sim.reset_warm_start()     # ... and its SVD warm start: a replay from here has the bits of a simulator that never warmed up
        torch.cuda.synchronize(dev)

    def _ws_kw(self, ws):
        """The render options of workspace `ws`: its frame workspace and, with draw_points(), its own camera for the point overlay."""
        kw = dict(self.kw, frame_slot=ws)
        if self.h.model.point_overlay_key() is not None:
            kw["point_pose"] = self.pose_dev[ws]
        return kw

    # ---- streams / events
    def stream(self, name):
        if name == "copy" and self.copier is not None:
            return _HostCopyStream(self)
        return _HipStream(self._streams[name])

    def __del__(self):
        if getattr(self, "copier", None) is not None:
            try:
                from ._lib import lib
                lib().pn_copier_destroy(self.copier)
            except Exception:  # noqa: BLE001 — interpreter shutdown: the import machinery is gone, the process is about to end anyway
                pass
            self.copier = None

    def event(self):
        return _HipEvent()

    def _snap(self, slot):
        if slot not in self.snap:
            self.snap[slot] = torch.empty_like(self.h.sim.dof)
        return self.snap[slot]

    # ---- device operations
    def snapshot(self, s, slot):
        with torch.cuda.stream(s.s):
            self._snap(slot).copy_(self.h.sim.dof)

    def substep(self, s):
        with torch.cuda.stream(s.s):
            self.sim_graph.replay()

    def broadcast(self, s, slot, src):
        import torch.distributed as dist
        with torch.cuda.stream(s.s):
            dist.broadcast(self._snap(slot), src=self.src, group=self.group)

    def consumer_fence(self, ws):
        """After on_retire(frame, result): whatever the consumer enqueued on its current stream (a copy of the device tensors) is ordered before
        the workspace's next render overwrites them."""
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.h.device))
        self.consumer_done[ws] = ev

    def render(self, s, frame, ws, slot, pose):
        with torch.cuda.stream(s.s):
            if self.consumer_done[ws] is not None:
                s.s.wait_event(self.consumer_done[ws])
                self.consumer_done[ws] = None
            # the camera of this frame (trainer.py:541): the given pose, else the harness's current one.  Every workspace keeps its own device
            # copy (the graph reads it), so it is uploaded whenever it differs from what THIS workspace last rendered — staged in pinned memory,
            # in stream order before the graph reads it
            p = np.ascontiguousarray(self.h.pose if pose is None else pose, dtype=np.float32).reshape(1, 4, 4)
            key = p.tobytes()
            if self.pose_key[ws] != key:
                self.pose_key[ws] = key
                self.pose_pin[ws].copy_(torch.from_numpy(p))
                self.pose_dev[ws].copy_(self.pose_pin[ws], non_blocking=True)
            self.h.sim.get_IP_info(dof=self._snap(slot), out=self.ip[ws])
            self.graph[ws].replay()

    def copy_out(self, s, ws, same_buffer=False):
        if not same_buffer:
            self.host_gen[ws] ^= 1
        dst, src = self.host[ws][self.host_gen[ws]], self.packed[ws]
        if isinstance(s, _HostCopyStream):
            import ctypes

            from ._lib import check, lib
            t = ctypes.c_uint64()
            after = ctypes.c_void_p(s.after.e.cuda_event) if s.after is not None else None
            check(lib().pn_copier_submit(self.copier, ctypes.c_void_p(dst.data_ptr()), ctypes.c_void_p(src.data_ptr()), src.numel() * src.element_size(), after,
                                         ctypes.byref(t)), "copier_submit")
            s.ticket = t.value
            self.last_ticket = t.value
            return
        with torch.cuda.stream(s.s):
            dst.copy_(src, non_blocking=True)

    def wait_copies(self):
        """[host] Blocks until every frame copy submitted so far has landed in host memory.  The copier thread's SDMA copies are on no stream:
        torch.cuda.synchronize() does not wait for them (bench.py stops its clock behind this)."""
        if self.copier is not None and getattr(self, "last_ticket", None) is not None:
            from ._lib import check, lib
            check(lib().pn_copier_wait(self.copier, self.last_ticket), "copier_wait")

    # ---- host side of a retired workspace
    def complete(self, ws):
        return self.h.model.render_status(synchronize=False, slot=ws)["alive_at_exit"] == 0

    def finish(self, ws):
        """The captured trips were not enough for this frame: keep going on the workspace's lane until no ray is alive (blocking), then copy
        the finished frame out again."""
        h, m = self.h, self.h.model
        s = self._streams[f"lane{ws // self.depth}"]
        with torch.cuda.stream(s):
            with h._amp():
                kw = self._ws_kw(ws)
                kw.pop("frame_slot")
                if "point_pose" in kw:
                    m.p_def, m.IP_F, m.IP_dF = self.ip[ws]   # the point overlay paints the state this frame was rendered from
                m.render_continue(ws, self.rays[ws]["rays_o"], self.rays[ws]["rays_d"], self.out[ws], bg_color=None, **kw)
            if self.host[ws] is not None:
                self.copy_out(_HipStream(s), ws, same_buffer=True)
        s.synchronize()
        self.continued += 1
        if self.continued == 8:
            # the launch form baked into the graphs (fused_from / fused_whole / fused_fold, the trip count) came from ONE warm-up frame; a scene or pose
            # that has moved away from it makes every frame end here, blocking — correct, only slow (round-4 advisor): say so once
            import warnings
            warnings.warn("8 frames of this pipeline had rays alive behind their captured trips and were finished by blocking renders: the launch form picked "
                          "at capture no longer fits the scene / pose — capture_pipelined() again from the current state", RuntimeWarning, stacklevel=2)

    def result(self, ws):
        o = self.out[ws]
        H, W, N = self.H, self.W, self.H * self.W
        dev = {"image": o["image"].view(-1, H, W, 3), "depth": o["depth"].view(-1, H, W), "depth_0": o["depth_0"].view(-1, H, W)}
        if "point_id" in o:   # draw_points(): on the device only (pick_drawn reads one value)
            dev.update(point_id=o["point_id"].view(-1, H, W), point_t=o["point_t"].view(-1, H, W), ip_pos=self.ip[ws][0])
        if self.host[ws] is None:
            return {"device": dev}
        hb = self.host[ws][self.host_gen[ws]].numpy()
        return {"image": hb[:3 * N].reshape(H, W, 3), "depth": hb[3 * N:4 * N].reshape(H, W), "depth_0": hb[4 * N:].reshape(H, W), "device": dev}
