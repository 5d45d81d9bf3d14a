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
from ._captured import Captured, LastFrame, refuse_form
from ._lib import lib
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
                             base=torch.tensor([-o["bound"]] * 3), device=self.device, kres=o.get("sim_kres", 7), solver=o.get("sim_solver", "dense"),
                             pcg_tol=o.get("pcg_tol", 1e-10), pcg_max_iters=o.get("pcg_max_iters", 576))
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
        self._graph = self._graph_done = None
        self._captured_graph = self._captured_pipe = None   # Captured: what the step graph / the pipeline baked in, None until captured
        self._pipe_form = None           # the pipeline's form by which step_pipelined() refuses (_captured.refuse_form)
        self._last = None                # LastFrame: what drag(), move() and pick_drawn() read
        self._collider_snapshot = None
        self.graph_continued = 0
        self._raw_streams = []
        # _pipe and _pipe_backend stay unset until capture_pipelined(): bench.py asks hasattr(h, "_pipe_backend")
        self.overlap_sim = overlap_sim
        self._sim_stream = None          # without overlap_sim: made by capture()
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

    @staticmethod
    def _pose_tensor(pose):
        """The [1, 4, 4] float32 host tensor of a camera pose (trainer.py:541)."""
        return torch.from_numpy(np.asarray(pose, np.float32)).unsqueeze(0)

    @staticmethod
    def _frame_views(out, H, W):
        """A render's flat image / depth / depth_0 as frames."""
        return {"image": out["image"].reshape(-1, H, W, 3), "depth": out["depth"].reshape(-1, H, W), "depth_0": out["depth_0"].reshape(-1, H, W)}

    def _render_frame(self, pose_dev, ip, kw, W, H, rays=None, out_buffers=None):
        """One frame of every form: the model renders from the integration-point triple `ip` (None: what it holds) along the rays of the camera
        `pose_dev` (`rays`: already built, where a step enqueues them in front of its substep), with the options `kw`.  Returns (rays, out)."""
        m = self.model
        if ip is not None:
            m.p_def, m.IP_F, m.IP_dF = ip
        if rays is None:
            rays = get_rays(pose_dev, self.intrinsics, H, W, -1)
        if m.point_overlay_key() is not None:
            kw = dict(kw, point_pose=pose_dev)   # draw_points(): the camera this frame's rays come from
        if out_buffers is not None:
            kw = dict(kw, out_buffers=out_buffers)
        with self._amp():
            return rays, m.render_deformed(rays["rays_o"], rays["rays_d"], staged=True, bg_color=None, perturb=False, **kw)

    def _now(self):
        """The Captured record of the current state: what a replay is checked against, and what a capture keeps."""
        return Captured(self.sim.enabled_stage_names(), self.model.collider_overlay_key(), self.model.point_overlay_key(), self._net_form_epoch())

    def _refuse(self, form, now=None):
        refuse_form(form, self._now() if now is None else now, self._shadows_set(), self.sim.bodies_enabled)

    @torch.no_grad()
    def step(self, pose=None, intrinsics=None, W=None, H=None, simulate=True, collect_stats=False, fused=True, render_kw=None):
        """render_kw: options of THIS render on top of self.opt (the pipeline's probes of a launch form pass theirs here instead of editing self.opt)."""
        o = self.opt
        W, H = W or o["W"], H or o["H"]
        pose = self.pose if pose is None else pose
        intrinsics = self.intrinsics if intrinsics is None else intrinsics
        key = np.asarray(pose, np.float32).tobytes()
        if self._pose_dev is None or self._pose_dev[0] != key:  # trainer.py:541 uploads the pose every frame; re-upload only when it changes
            self._pose_dev = (key, self._pose_tensor(pose).to(self.device))
        rays = get_rays(self._pose_dev[1], intrinsics, H, W, -1)
        m = self.model
        self._order_overlay_behind_setters()   # before this frame's substep goes onto the simulator's stream: the render still overlaps it
        if simulate:
            main = torch.cuda.current_stream(self.device)
            if self.overlap_sim:
                main.wait_event(self._sim_done)            # the previous substep must have finished before dof is read
            m.p_def, m.IP_F, m.IP_dF = self.sim.get_IP_info()
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
        if fused:
            _, out = self._render_frame(self._pose_dev[1], None, kw, W, H, rays=rays)   # (the state was installed with the substep, above)
        else:
            with self._amp():
                out = m.rund_cuda_ops(rays["rays_o"], rays["rays_d"], bg_color=None, perturb=False, **kw)
        res = dict(self._frame_views(out, H, W), rays_o=rays["rays_o"], rays_d=rays["rays_d"])
        res.update({k: out[k] for k in ("coverage", "collider_t", "shadow") if k in out})   # draw_colliders() / cast_shadows(): the overlay's own outputs
        if "point_id" in out:   # draw_points(): the drawn point per pixel, what pick_drawn() reads
            res.update(point_id=out["point_id"].reshape(-1, H, W), point_t=out["point_t"].reshape(-1, H, W))
        if self.sim.drag_enabled:   # what drag() / move() unproject against (only then: without the drag nothing else is kept alive)
            self._last = LastFrame("eager", out["depth_0"].reshape(H, W), m.p_def, pose, intrinsics, res.get("point_id"))
        elif "point_id" in out:
            self._last = (self._last or LastFrame())._replace(ip_pos=m.p_def, point_id=res["point_id"])
        return res

    # ------------------------------------------------------------------ whole step as one HIP graph
    def _step_body(self, n_trips, W, H):
        """get_rays -> get_IP_info -> { stepforward || render_deformed } with fork/join on the current stream (capturable)."""
        main = torch.cuda.current_stream(self.device)
        rays = get_rays(self._graph_pose, self.intrinsics, H, W, -1)
        ip = self.sim.get_IP_info()
        self._snapshot_colliders()   # enable_bodies(): the balls this frame draws, as the substep below finds them
        self._sim_stream.wait_stream(main)
        with torch.cuda.stream(self._sim_stream):
            self.sim.stepforward()
        _, out = self._render_frame(self._graph_pose, ip, dict(self.render_kwargs(), async_trips=n_trips), W, H, rays=rays)
        main.wait_stream(self._sim_stream)
        # every tensor the graph touches is returned (and so stays referenced): memory freed after capture would go back to the
        # graph's pool and could be handed out again
        res = dict(self._frame_views(out, H, W), weights_sum=out["weights_sum"], rays_o=rays["rays_o"], rays_d=rays["rays_d"], _ip=tuple(ip))
        res.update({k: out[k] for k in ("coverage", "collider_t", "shadow") if k in out})   # draw_colliders() / cast_shadows(): render_continue writes them again
        res.update({k: out[k] for k in ("point_id", "point_t") if k in out})   # draw_points(): flat [N], render_continue writes them again
        return res

    @torch.no_grad()
    def capture(self, n_trips=8, W=None, H=None):
        """Captures one whole step (~85 kernel launches on two streams) into a HIP graph.  `n_trips` render-loop trips are
        baked in (the chair needs 5); step_graph() verifies afterwards that no ray was left alive."""
        o = self.opt
        W, H = W or o["W"], H or o["H"]
        if self._sim_stream is None:
            self._sim_stream = torch.cuda.Stream(self.device)
        self._graph_pose = self._pose_tensor(self.pose).to(self.device)
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
        self._captured_graph = self._now()
        return self

    def _net_form_epoch(self):
        """How often the fp32 network switched between its fp16 hi/lo and bf16 forms (include/pienerf_hip.h: pn_net_form_epoch).  The per-layer scales
        live in device memory and follow an in-place weight refresh; the form is baked into every captured launch."""
        net = getattr(self.model, "_net", None)
        return int(lib().pn_net_form_epoch(net)) if net is not None else 0

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
        self._last = self._last and self._last._replace(point_id=None)
        return self

    def pick_drawn(self, x, y, point_id=None, ip_pos=None):
        """An exact pick through the picture: the integration point drawn at pixel (x, y) of the last frame (column x, row y) — that one value of the
        frame's 'point_id' is read back, no search for the point nearest to an unprojected cursor — is held by the drag (Simulator.drag_hold) with its
        own position as the target; move() then pulls it.  Returns its index, or -1 where no point was drawn (the drag is left as it was).  The
        pipelined form passes the retired frame's `point_id` and the positions `ip_pos` it was rendered from."""
        if not self.sim.drag_enabled:
            raise RuntimeError("pick_drawn: call enable_drag() first (before capture() / capture_pipelined())")
        if point_id is None:
            fr = self._last
            if fr is None or fr.point_id is None:
                raise RuntimeError("pick_drawn: no frame with the points drawn has been rendered yet (draw_points(), then a step)")
            if fr.form == "graph":
                self._check_previous_graph_frame()
            point_id, ip_pos = fr.point_id, (fr.ip_pos if ip_pos is None else ip_pos)
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
        if self._collider_snapshot is None or ov.state is not self._collider_snapshot:
            self._collider_snapshot = live.clone()
            self.model.set_collider_overlay(self._collider_snapshot, ov.style, ov.t_max)
        self._collider_snapshot.copy_(live)

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

    @torch.no_grad()
    def step_graph(self, pose=None):
        """Replays the captured step.  Outputs are static tensors (overwritten by the next replay); they are complete — including frames
        that needed more trips than were captured — after the NEXT call or ``finish_graph_frame()``."""
        if self._graph is None:
            self.capture()
        now, cap = self._now(), self._captured_graph
        cap.check_substep(now, "graph")
        cap.check_render(now, "graph")
        self._check_previous_graph_frame()
        if pose is not None:
            self._graph_pose.copy_(self._pose_tensor(pose))
        self._order_overlay_behind_setters()
        self._graph.replay()
        self._graph_done = torch.cuda.Event()
        self._graph_done.record(torch.cuda.current_stream(self.device))
        self.frame += 1
        if pose is not None:
            self._graph_pose_host = pose
        g, pid = self._graph_out, self._graph_out.get("point_id")
        if "drag" in cap.stages:
            self._last = LastFrame("graph", g["depth_0"][0], g["_ip"][0], self._graph_pose_host, self.intrinsics, pid)
        else:
            self._last = LastFrame("graph", ip_pos=None if pid is None else g["_ip"][0], point_id=pid)
        return g

    def finish_graph_frame(self):
        """Waits for the last replayed step and completes it; returns its outputs."""
        self._check_previous_graph_frame()
        return self._graph_out

    def _check_previous_graph_frame(self):
        """The captured step bakes in a trip count; a frame that still had rays alive after them is finished here with further trips (the
        reference's loop just keeps going, renderer.py:836-891) before its outputs are handed on."""
        if self._graph_done is not None:
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
                self.graph_continued += 1

    # ------------------------------------------------------------------ several frames in flight (one GPU, or frame-parallel over a node)
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

        from .frames import FramePipeline, dedicated_sim_default
        from .pipeline_hip import _HipBackend
        form = "frame_parallel" if frame_parallel else "staged" if (render_kw or {}).get("ray_batch") else "pipelined"
        self._refuse(form)
        o = self.opt
        W, H = W or o["W"], H or o["H"]
        on = bool(frame_parallel) and dist.is_available() and dist.is_initialized()
        world = dist.get_world_size(group) if on else 1
        rank = dist.get_rank(group) if on else 0
        if n_trips is None:  # calibrate: the trips one eager frame needs from the current state and pose, plus a margin
            self.step(simulate=False, collect_stats=True, W=W, H=H)
            n_trips = int(self.model.last_stats["trips"]) + 2  # every captured trip costs five launches whether it has rays or not
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
        self._captured_pipe = self._now()
        self._pipe_form = "pipelined" if form == "pipelined" else "parallel_or_staged"   # what step_pipelined() refuses by
        self._last = LastFrame("pipelined")   # drag() and pick_drawn() are handed the retired frame's depth_0 / point_id
        self._pipe_backend = be
        self.model._in_flight = lambda pipe=self._pipe: sum(f is not None for f in pipe.pending)  # weight refreshes need a drained pipeline (network._net_handle)
        return self

    def capture_frame_parallel(self, lanes=2, n_trips=8, group=None, sim_owner=0, dedicated_sim=None, **kw):
        """Multi-GPU form (BASELINE.json configs[3]): every rank calls step_frame_parallel() once per GLOBAL frame."""
        return self.capture_pipelined(lanes=lanes, n_trips=n_trips, group=group, frame_parallel=True, sim_owner=sim_owner, dedicated_sim=dedicated_sim, **kw)

    @torch.no_grad()
    def step_pipelined(self, pose=None):
        now, cap = self._now(), self._captured_pipe
        cap.check_substep(now, "pipe")
        self._refuse(self._pipe_form, now)
        cap.check_render(now, "pipe")
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
        if hasattr(self, "_pipe_backend"):   # unset until capture_pipelined(), see __init__: bench.py's barrier comes here in every form
            self._pipe_backend.wait_copies()

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
            kw = dict(self.render_kwargs())
            kw.pop("ray_batch", None)
            if be.kw.get("ray_batch"):
                kw["ray_batch"] = be.kw["ray_batch"]   # batches keep their own trip schedules: part of what the frame IS, not of how it is launched
            _, out = self._render_frame(be.pose_dev[ws], be.ip[ws], kw, be.W, be.H)
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
        self._refuse("tile_parallel")
        o, m, dev = self.opt, self.model, self.device
        W, H = W or o["W"], H or o["H"]
        ip = tuple(torch.empty((self.sim.n_IP, c), dtype=torch.float32, device=dev) for c in (3, 9, 27))
        self._tile_pose = self._pose_tensor(self.pose).to(dev)

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
        self._refuse("tile_parallel")
        if pose is not None:
            self._tile_pose.copy_(self._pose_tensor(pose).to(self.device))
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

    # ------------------------------------------------------------------ the GUI's mouse drag (gui.py:556-586, :833-841)
    def enable_drag(self, scale=None):
        """Simulator.enable_drag: every substep from now on gets the GUI's spring force toward the cursor, computed on the device from the state that
        substep starts from.  Call it BEFORE capture() / capture_pipelined(): a graph captured without it has no drag launch and refuses drag()."""
        self.sim.enable_drag(scale)
        return self

    def _drag_check(self):
        if not self.sim.drag_enabled:
            raise RuntimeError("drag: call enable_drag() first (before capture() / capture_pipelined())")
        fr = self._last
        if fr is None or fr.form is None:
            raise RuntimeError("drag: no frame has been rendered yet (the cursor is unprojected against the last frame's depth_0)")
        if fr.form == "graph" and "drag" not in self._captured_graph.stages:
            raise RuntimeError("drag: the step graph was captured before enable_drag(), its substep ignores the drag state: capture() again")
        if fr.form == "pipelined" and "drag" not in self._captured_pipe.stages:
            raise RuntimeError("drag: the pipeline was captured before enable_drag(), its substep ignores the drag state: capture_pipelined() again")
        return fr

    def _drag_inputs(self, depth0, ip_pos, pick):
        fr = self._drag_check()
        if fr.form == "pipelined":
            # the caller hands in the last RETIRED frame's depth_0: the cursor is then unprojected against an image `lanes * depth` frames older than
            # the state the next substep reads — inherent to the pipeline.  The pick searches the IPs of the simulator's newest state.
            if depth0 is None:
                raise ValueError("drag in the pipelined form: pass depth0, the depth_0 of the last frame step_pipelined() returned")
            depth0 = torch.as_tensor(depth0).to(self.device, torch.float32).contiguous()
            if pick and ip_pos is None:
                with self.sim._on_force_stream():
                    ip_pos = self.sim.get_IP_info()[0]
            return depth0, ip_pos, self.pose, self.intrinsics
        if fr.form == "graph":
            self._check_previous_graph_frame()   # a frame left with rays alive is finished before its depth_0 is read
        return (fr.depth_0 if depth0 is None else depth0), (fr.ip_pos if ip_pos is None else ip_pos), fr.pose, fr.intrinsics

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
