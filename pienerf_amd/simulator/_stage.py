"""What the simulator's substep stages (drag.py, pins.py, contact.py, bodies.py, fields.py, selfcontact.py) have in common, written once.

A stage is a small state in device memory plus launches that ``Simulator.stepforward`` enqueues in front of the substep.  Each stage's module
describes it with a ``Stage`` record and holds a mixin with its methods; ``StageHost`` — a base of ``Simulator`` — holds the scaffold those mixins
share: the guards, the state allocator, the host read, the rule for the tables and keep_state / restore_state.
"""
from collections import namedtuple

import numpy as np
import torch

from .._lib import lib

torchfloat = torch.float64
npfloat = np.float64

# name: what the harness records as captured; flag / state: the Simulator attributes `X_enabled` and the device state (None until allocated);
# subject / owner: the words of the two guard errors; enable: the public method that switches the stage on; struct / nbytes / sized_by: the C struct,
# its size as Python lays it out and the words of the size error; init / alloc / enqueue: the mixin's methods, by name; tables: the method that builds
# the layout tables the stage reads (None: it reads none); writes: "dof_f" (enqueued in front of the substep's preparation) or "rhs" (a link of the
# right-hand-side chain, enqueue(rhs_in) -> rhs_out); clock: the state begins with an int64 substep clock that keep_state() saves
Stage = namedtuple("Stage", "name flag state subject owner enable struct nbytes sized_by init alloc enqueue tables writes clock")


def _vec3(v, what, who="contact"):
    a = np.asarray(v, npfloat)
    if a.size != 3 or not np.isfinite(a).all():
        raise ValueError(f"{who}: {what} is a finite 3-vector, got {v!r}")
    return a.reshape(3).copy()


class _null_ctx:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


class StageHost:
    STAGES = ()   # Simulator sets the order

    def enabled_stages(self):
        """The stages switched on, in the order stepforward() enqueues them."""
        return tuple(st for st in self.STAGES if getattr(self, st.flag))

    def enabled_stage_names(self):
        """What a capture records (_captured.Captured.stages): the enabled stages' names, and what an enabled stage adds to them while it enqueues
        launches that a graph captured earlier lacks (contact.py: "mesh_colliders")."""
        names = set()
        for st in self.enabled_stages():   # a stage's mixin may name more with a method _<stage>_capture_names()
            names.add(st.name)
            more = getattr(self, f"_{st.name}_capture_names", None)
            if more is not None:
                names.update(more())
        return frozenset(names)

    # ------------------------------------------------------------------ guards
    def _stage_state(self, st, gpu=True):
        """The stage's device state.  RuntimeError while the stage is not enabled and, with `gpu`, while the state is not allocated (None is returned
        for that without `gpu`: setters that only change the host mirror)."""
        if not getattr(self, st.flag):
            raise RuntimeError(f"Simulator: {st.subject} not enabled (call {st.enable}() first)")
        state = getattr(self, st.state)
        if gpu and state is None:
            raise RuntimeError(f"Simulator: {st.owner} lives on a GPU: initialize the simulator on a cuda device first")
        return state

    # ------------------------------------------------------------------ switching on, allocation
    def _switch_on(self, st):
        """The common part of enable_X(): with a layout in place build the stage's tables, set the flag, and on a GPU allocate the state.  Returns
        False when the stage was on already."""
        if getattr(self, st.flag):
            return False
        if self.dof is not None and st.tables:
            getattr(self, st.tables)()   # may raise (a cloud without pins): the stage then stays off
        setattr(self, st.flag, True)
        if self.dof is not None and self.device.type == "cuda":
            getattr(self, st.alloc)()
        return True

    def _build_stage_tables(self):
        """The tables of the enabled stages belong to the layout: precompute() builds them with it, _switch_on() for a stage enabled later."""
        self.n_pin, self.pin_bg = 0, None
        self.Nx_csr = None
        for st in self.enabled_stages():
            if st.tables:
                getattr(self, st.tables)()

    def _need_Nx_csr(self):
        """The Nx rows in CSR order (as dNx_csr is for the substep): the per-kernel sum of contact, force fields and self-contact reads a kernel's run
        as one contiguous stream.  The table exists only with one of the three enabled, and is built once for all of them; a new tensor after every
        precompute(), like the other tables of a layout."""
        if self.Nx_csr is None:
            self.Nx_csr = self.IP_Nx.reshape(self.n_IP * 8, 10)[self.buffer.long()].contiguous()

    def _new_state(self, st):
        """The stage's state as zeroed doubles, after checking that the library's struct has the size Python lays out."""
        nb = int(getattr(lib(), f"pn_sim_{st.name}_bytes")())
        if nb != st.nbytes:
            raise RuntimeError(f"libpienerf_hip.so's {st.struct} has {nb} bytes, {st.sized_by} {st.nbytes}")
        state = torch.zeros(st.nbytes // 8, dtype=torchfloat, device=self.device)
        setattr(self, st.state, state)
        return state

    # ------------------------------------------------------------------ host reads
    def _host_read(self, f):
        """f() — a read back to the host — on force_stream, or the current stream without one.  It waits for that stream only: where the substeps
        run on other streams (the pipelined harness, a caller's own side stream) the value is defined after those have been waited for."""
        s = self.force_stream if self.force_stream is not None else torch.cuda.current_stream(self.device)
        with torch.cuda.stream(s):
            return f()

    def _read_clock(self, st):
        state = self._stage_state(st)
        return self._host_read(lambda: int(state[:1].view(torch.int64)[0].item()))

    # ------------------------------------------------------------------ keep / restore
    def _clock_keep(self, st):
        state = getattr(self, st.state)
        return state[:1].clone() if state is not None else None

    def _clock_restore(self, st, keep):
        if keep is not None:
            getattr(self, st.state)[:1].copy_(keep)

    def keep_state(self):
        """dof, dof_vel and the substep clock of every stage that has one, as device copies: for whoever warms the substep up (a capture) or replays
        a trajectory, and then calls restore_state().  With the rigid balls enabled (bodies.py) their state and the contact state are kept too: a
        ball's position and velocity are part of the trajectory."""
        keep = dict(dof=self.dof.clone(), dof_vel=self.dof_vel.clone(), clocks=[(st, self._clock_keep(st)) for st in self.STAGES if st.clock])
        moved = [st for st in self.STAGES if st.name in ("contact", "bodies")]
        if getattr(self, "bodies_enabled", False) and all(getattr(self, st.state) is not None for st in moved):
            keep["bodies"] = [(st, getattr(self, st.state).clone()) for st in moved]
        return keep

    def restore_state(self, keep):
        """Back to keep_state()'s moment: dof, dof_vel, then the clocks in the stages' order, so the k-th step from here sees the clock of the k-th step
        from there.  The SVD warm start is not part of it: a replay that wants the same BITS calls reset_warm_start() as well."""
        self.dof.copy_(keep["dof"])
        self.dof_vel.copy_(keep["dof_vel"])
        for st, k in keep["clocks"]:
            self._clock_restore(st, k)
        for st, whole in keep.get("bodies", ()):
            getattr(self, st.state).copy_(whole)
