"""The device side of frames.FramePipeline on one MI355X (harness.SimRenderHarness.capture_pipelined builds it), and the launch form its frames
run in: pure functions of trip records and plain values, importable without a GPU, and the probes that feed them."""
import ctypes
import itertools

import numpy as np
import torch

from ._lib import check, lib

# pn_render_opts.throughput_trips: a trip marches in the throughput form (one lane per ray) when it has at least this many alive rays — 2048 waves,
# two per SIMD (measured: trex option set, second trip of 246 k rays: 1 191 -> 1 321 steps/s; chair, second trip of 41 k rays: 1 650 -> 1 480)
THROUGHPUT_FORM_MIN_RAYS = 131072


# ---- the launch form from plain values; a trip record is (n_alive, n_step, step_base, n_samples, n_emitted, n_tail)
def fused_from_of(recs, ray_batch):
    """pn_render_opts.fused_from: the first loop trip past the frame's first with n_step == 8, -1 without one and for a frame in ray batches."""
    return -1 if ray_batch else next((i for i, r in enumerate(recs) if i >= 1 and r[1] == 8), -1)


def throughput_trips_of(recs):
    """pn_render_opts.throughput_trips: the leading trips that still have rays enough to fill the GPU with ONE lane per ray."""
    return 1 + sum(1 for _ in itertools.takewhile(lambda rec: rec[0] >= THROUGHPUT_FORM_MIN_RAYS, recs[1:]))


def fused_grid_of(lanes, cus):
    """pn_render_opts.fused_grid with several frames in flight (two lanes, whole-frame launches: 128 / 160 / 192 workgroups: 1 717 / 1 776 / 1 689 steps/s)."""
    return max(cus * 5 // 8 if lanes == 2 else cus // 2, 1)


def try_fused_whole(lanes, fused_from):
    return lanes == 2 and fused_from == 1


def try_fused_fold(lanes, fused_whole, fused_from, fused_order):
    """Folded only in list order: `fused_order` given and false (None is the library's default, longest packets first)."""
    return lanes >= 3 and not fused_whole and fused_from == 1 and fused_order is not None and not fused_order


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
        self.copier = self.last_ticket = None
        if copy_on == "host" and copy_out:
            hc = ctypes.c_void_p()
            check(lib().pn_copier_create(ctypes.byref(hc)), "copier_create")
            self.copier = hc
        self.h, self.lanes, self.depth, self.trips, self.W, self.H, self.group, self.src = h, lanes, depth, n_trips, W, H, group, src
        dev, sim, n_ws = h.device, h.sim, lanes * depth
        self.continued = 0
        self._make_streams(sim_priority, sim_cus)
        self.snap = {}
        self.consumer_done = [None] * n_ws   # per workspace: the event behind what on_retire enqueued on its stream (consumer_fence)
        self.kw = dict(h.render_kwargs(), async_trips=n_trips)
        self.kw.update(render_kw or {})  # options of THIS pipeline's renders (capture_staged: ray_batch)
        self._choose_launch_form()
        if distributed:
            # every rank of a frame-parallel job runs the launch form rank `src` picked (each probed its own warm-up frame: the same state and pose, but
            # nothing guarantees the same answer at a threshold) — round-4 advisor; gated on the job being distributed, NOT on `group`: the default
            # process group is group=None (round-5 advisor: with `if group is not None` this never ran in a real job)
            from .frames import agree_on_launch_form
            agree_on_launch_form(self.kw, src=src, group=group, device=dev)
        pose0 = h._pose_tensor(h.pose)
        self.pose_dev = [pose0.to(dev) for _ in range(n_ws)]
        self.pose_pin = [pose0.clone().pin_memory() for _ in range(n_ws)]
        self.pose_key = [pose0.numpy().tobytes()] * n_ws
        self.ip = [tuple(torch.empty((sim.n_IP, c), dtype=torch.float32, device=dev) for c in (3, 9, 27)) for _ in range(n_ws)]
        keep = sim.keep_state()
        self._warm_up()
        self._capture_substep(probe_no_substep)
        self._capture_workspaces(time_trips, copy_out)
        torch.cuda.synchronize(dev)
        self._premap_host_buffers()
        sim.restore_state(keep)    # warm-up advanced the simulator and its stages' clocks; capture itself executes nothing
        sim.reset_warm_start()     # ... and its SVD warm start: a replay from here has the bits of a simulator that never warmed up
        torch.cuda.synchronize(dev)

    def _make_streams(self, sim_priority, sim_cus):
        h, dev = self.h, self.h.device
        # sim_cus > 0, a compute-unit partition: the substep's chain of small dependent launches gets `sim_cus` CUs of its own (spread over the XCDs),
        # the render lanes the rest, so a substep never waits for a render wave to release registers
        # sim_cus < 0, the converse: the render lanes stay off -sim_cus CUs, the simulator may use every CU — its launches always find those free, and whatever else is
        self._streams = {"sim": self._cu_masked_stream(sim_cus, invert=False) if sim_cus > 0 else torch.cuda.Stream(dev, priority=sim_priority)}
        for i in range(self.lanes):
            self._streams[f"lane{i}"] = self._cu_masked_stream(abs(sim_cus), invert=True) if sim_cus else torch.cuda.Stream(dev)
        self._streams["comm"], self._streams["copy"] = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
        h.sim.force_stream = self._streams["sim"]   # a force change is enqueued between two substeps of the simulator stream

    def _cu_masked_stream(self, n_cu, invert):
        """A stream confined to the first `n_cu` CUs, or with `invert` to all the others; its raw handle is kept on the harness."""
        raw = ctypes.c_void_p()
        with torch.cuda.device(self.h.device):
            check(lib().pn_stream_create_cu_mask(lib().pn_device_cu_count(), 0, n_cu, int(invert), ctypes.byref(raw)), "stream_create_cu_mask")
        self.h._raw_streams.append(raw.value)
        return torch.cuda.ExternalStream(raw.value, device=self.h.device)

    def _probe(self, **form):
        """A blocking frame from the current state and pose: in the harness's own options, or in the launch form `form` on top of the pipeline's."""
        self.h.step(simulate=False, collect_stats=True, W=self.W, H=self.H, render_kw=dict(self.kw, **form, async_trips=0) if form else None)

    def _choose_launch_form(self):
        """Fills self.kw with the launch form of this pipeline's frames; a key the caller passed in render_kw is never overwritten."""
        kw, lanes, m = self.kw, self.lanes, self.h.model
        # several frames in flight: the first trip's march pass in its throughput form (pn_render_opts.throughput: one lane per ray, no speculative
        # evaluation; the same samples bit for bit, +8 % steps/s with three lanes) — with one lane the frame's own latency is what counts
        kw.setdefault("march_throughput", 64 if lanes > 1 else 0)
        # ... and each frame's fused launch (pn_render_opts.fused_from) on half of the CUs: the launches of the frames in flight run side by side and the
        # other kernels find CUs with free LDS (pn_render_opts.fused_grid; three lanes on the chair: 1 721 -> 1 937 steps/s)
        if lanes > 1:
            kw.setdefault("fused_grid", fused_grid_of(lanes, torch.cuda.get_device_properties(self.h.device).multi_processor_count))
        if "fused_from" not in kw:
            # pn_render_opts.fused_from: the loop trips from the first one with n_step == 8 on (n_alive <= N / 8: it stays 8 for the rest of the frame) run
            # as ONE persistent launch (csrc/pn_trips_fused.h) — read off the trip records of a blocking frame from the current state and pose.  A later
            # frame that still has more rays alive at that trip is finished when it is retired (frames.FramePipeline: continue), only slower
            self._probe()
            kw["fused_from"] = fused_from_of(m.trip_records(slot=0, max_trips=64), kw.get("ray_batch"))
        if "fused_whole" not in kw:
            # pn_render_opts.fused_whole: the frame's first trip in that launch too (where at most N / 8 rays have anything to march: the blocking frame
            # below tries it and reports the trip at which the fused launch took over).  Measured on the chair: better with two frames in flight
            # (1 700-1 740 against 1 560 steps/s), worse with three (1 730 against 1 930) or one at a time — include/pienerf_hip.h
            whole = try_fused_whole(lanes, kw["fused_from"])
            if whole:
                self._probe(fused_whole=True, fused_from=0)
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
            fold = try_fused_fold(lanes, kw.get("fused_whole"), kw["fused_from"], kw.get("fused_order"))
            if fold:
                self._probe(fused_fold=True)
                fold = m.fused_clocks(slot=0)["mode"] == 2
            kw["fused_fold"] = bool(fold)

    def _warm_up(self):
        """Two frames on every workspace outside capture (creates the pn_frame workspaces, the fp16 tables, ...)."""
        h, sim, kw = self.h, self.h.sim, self.kw
        main = torch.cuda.current_stream(h.device)
        for ws in range(self.lanes * self.depth):
            s = self._streams[f"lane{ws // self.depth}"]
            s.wait_stream(main)
            with torch.cuda.stream(s):
                for _ in range(2):
                    sim.get_IP_info(out=self.ip[ws])
                    sim.stepforward()
                    h._render_frame(self.pose_dev[ws], self.ip[ws], self._ws_kw(ws), self.W, self.H)
            torch.cuda.synchronize(h.device)
            if ws == 0 and kw.get("march_throughput") and "march_throughput_trips" not in kw:
                # the throughput form for every leading trip that still has rays enough to fill the GPU with ONE lane per ray (the trex option set's
                # second trip: 246 k rays x 3 samples; the chair's: 41 k x 8, faster in the windows) — from this warm-up frame's trip records; the
                # samples do not depend on the form, so a scene that changes later only loses speed
                kw["march_throughput_trips"] = throughput_trips_of(h.model.trip_records(slot=0))

    def _capture_substep(self, probe_no_substep):
        from .harness import _capture
        # capture_error_mode="thread_local": with a process group alive, RCCL's watchdog thread queries events while we capture;
        # in the default "global" mode any HIP call from another thread invalidates the capture
        self.sim_graph = torch.cuda.CUDAGraph()
        with _capture(self.sim_graph, stream=self._streams["sim"]):
            if not probe_no_substep:
                self.h.sim.stepforward()
            else:
                self.h.sim.dof_vel.mul_(1.0)

    def _capture_workspaces(self, time_trips, copy_out):
        """One graph per workspace: get_rays + the render from the workspace's own IP buffers into its own output buffers."""
        from .harness import _capture
        h, dev, N = self.h, self.h.device, self.W * self.H
        self.graph, self.rays, self.out, self.host, self.packed = [], [], [], [], []
        for ws in range(self.lanes * self.depth):
            s = self._streams[f"lane{ws // self.depth}"]
            if time_trips:  # measurement (bench.py): time stamps around each trip's march / network launches become nodes of the captured graph
                h.model.march_counters(2, slot=ws)
            # image | depth | depth_0 packed in one device buffer -> ONE device-to-host copy per frame (20 B per pixel, trainer.py:589-592)
            pk = torch.empty(N * 5, dtype=torch.float32, device=dev)
            ob = {"image": pk[:3 * N].view(N, 3), "depth": pk[3 * N:4 * N], "depth_0": pk[4 * N:], "weights_sum": torch.empty(N, dtype=torch.float32, device=dev)}
            g = torch.cuda.CUDAGraph()
            with _capture(g, stream=s):
                rays, out = h._render_frame(self.pose_dev[ws], self.ip[ws], self._ws_kw(ws), self.W, self.H, out_buffers=ob)
            self.graph.append(g)
            # every tensor the graphs touch stays referenced: a tensor freed after capture goes back to the graph's memory pool
            self.rays.append(rays)
            self.out.append(out)
            self.packed.append(pk)
            # two pinned sets per workspace, used alternately: the arrays handed out when a frame is retired stay valid until the workspace has
            # been through another whole frame (the next frame's D2H goes into the other set)
            self.host.append([torch.empty(N * 5, dtype=torch.float32).pin_memory() for _ in range(2)] if copy_out else None)
        self.host_gen = [0] * len(self.graph)

    def _premap_host_buffers(self):
        """The first SDMA copy into a pinned buffer maps it for the engine (milliseconds): once per buffer here, not inside the pipeline's first frames."""
        for ws in range(len(self.packed) if self.copier is not None else 0):
            for _ in self.host[ws]:   # copy_out alternates between the workspace's two pinned sets
                self.copy_out(_HostCopyStream(self), ws)
                self.wait_copies()

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
                lib().pn_copier_destroy(self.copier)
            except Exception:  # noqa: BLE001 — interpreter shutdown: the module's globals are gone, the process is about to end anyway
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
        if self.copier is not None and self.last_ticket is not None:
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
        dev = self.h._frame_views(o, H, W)
        if "point_id" in o:   # draw_points(): on the device only (pick_drawn reads one value)
            dev.update(point_id=o["point_id"].view(-1, H, W), point_t=o["point_t"].view(-1, H, W), ip_pos=self.ip[ws][0])
        if self.host[ws] is None:
            return {"device": dev}
        hb = self.host[ws][self.host_gen[ws]].numpy()
        return {"image": hb[:3 * N].reshape(H, W, 3), "depth": hb[3 * N:4 * N].reshape(H, W), "depth_0": hb[4 * N:].reshape(H, W), "device": dev}
