"""What a state of the simulator holds, measured on the device (csrc/pn_diagnostics.hip; the law: include/pienerf_hip.h, pn_sim_diagnostics, and
DESIGN.md 4.18): mass, centre of mass, linear and angular momentum, kinetic / gravitational / elastic energy, the extrema of the singular values, of
det F, of the strain and of the speed with the integration point that attains each, and the counts of non-finite and inverted points.

A readout, not a substep stage: it adds nothing to the right-hand-side chain and never writes simulator state, so a run with it and a run without it
are the same bits.  The energies are the ones the solver's own matrix stands for (build_IP_global, simulator/cuda_utils.py:48-55 of the reference).  The
integrator — Projective Dynamics with a few local/global iterations, a 1e-3 diagonal shift and pin penalties — conserves neither energy nor momentum
exactly, and the pin penalty's energy is not part of `elastic` (the pins act on cloud points, and kinematic pins move their targets)."""
import numpy as np
import torch

from .._lib import check, lib, ptr, stream_ptr
from ._stage import torchfloat

__all__ = ["DIAG_FIELDS", "DIAG_VECTORS", "DIAG_INDICES", "DIAG_COUNTS", "diagnostics_dict", "DiagnosticsLog", "DiagnosticsMixin"]   # what solver.py re-exports

# the row of pn_sim_diagnostics, one name per double (PN_DIAG_DOUBLES = pn_sim_diagnostics_doubles() of them); the CSV's header
DIAG_FIELDS = ("mass", "com_x", "com_y", "com_z", "P_x", "P_y", "P_z", "L_x", "L_y", "L_z", "kinetic", "gravity", "elastic",
               "sig_min", "sig_min_ip", "sig_max", "sig_max_ip", "det_min", "det_min_ip", "strain_max", "strain_max_ip", "speed_max", "speed_max_ip",
               "nonfinite", "inverted")
DIAG_VECTORS = ("com", "P", "L")                                                                  # read_diagnostics() gives these as arrays [3]
DIAG_INDICES = ("sig_min_ip", "sig_max_ip", "det_min_ip", "strain_max_ip", "speed_max_ip")        # ... these as ints (-1: no finite point)
DIAG_COUNTS = ("nonfinite", "inverted")                                                           # ... and these
PER_POINT_FIELDS = ("m", "ke", "ee", "det", "sig0", "sig1", "sig2", "strain")                     # the optional per-point record [n_IP, 8]


def diagnostics_dict(row):
    """One row (25 doubles, on the host) as a dict: scalars by their DIAG_FIELDS name, com / P / L as arrays [3], indices and counts as ints."""
    r = np.asarray(row, np.float64).reshape(-1)
    if r.size != len(DIAG_FIELDS):
        raise ValueError(f"a diagnostics row has {len(DIAG_FIELDS)} doubles, got {r.size}")
    d = {}
    for i, name in enumerate(DIAG_FIELDS):
        stem = name[:-2]
        if name.endswith("_x") and stem in DIAG_VECTORS:
            d[stem] = r[i:i + 3].copy()
        elif name[-2:] in ("_y", "_z") and stem in DIAG_VECTORS:
            continue
        elif name in DIAG_INDICES or name in DIAG_COUNTS:
            d[name] = int(r[i])
        else:
            d[name] = float(r[i])
    return d


class DiagnosticsLog:
    """Rows of diagnostics in device memory: Simulator.record_diagnostics(log) writes the next one, to_numpy() / write_csv() are the host's one read.
    Which row is written next is a HOST counter, so recording belongs outside a stream capture (a captured launch would write the same row on
    every replay)."""

    def __init__(self, capacity, device="cuda"):
        capacity = int(capacity)
        if capacity <= 0:
            raise ValueError(f"DiagnosticsLog: capacity is a positive number of rows, got {capacity}")
        self.capacity, self.count = capacity, 0
        self.rows = torch.zeros((capacity, len(DIAG_FIELDS)), dtype=torchfloat, device=device)

    def __len__(self):
        return self.count

    def next_row(self):
        """The row the next record writes; RuntimeError when the log is full."""
        if self.count >= self.capacity:
            raise RuntimeError(f"DiagnosticsLog: full ({self.capacity} rows)")
        row = self.rows[self.count]
        self.count += 1
        return row

    def to_numpy(self):
        """The recorded rows [count, 25] on the host, ordered behind the current stream (record_diagnostics makes it wait for each row)."""
        return self.rows[:self.count].cpu().numpy()

    def write_csv(self, path, rows=None):
        """The rows (default: to_numpy()) under a header of DIAG_FIELDS, 17 significant digits: a value reads back to the same double."""
        rows = self.to_numpy() if rows is None else np.asarray(rows, np.float64).reshape(-1, len(DIAG_FIELDS))
        with open(path, "w") as fh:
            fh.write(",".join(DIAG_FIELDS) + "\n")
            for r in rows:
                fh.write(",".join(repr(float(v)) for v in r) + "\n")
        return path


class DiagnosticsMixin:
    _diag_work = None   # the partial records of the first launch, made on first use (so: call diagnostics() once before capturing it into a graph)

    def _diag_state_arg(self, t, name):
        if t is None:
            return getattr(self, name)
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torchfloat and t.is_contiguous() and t.numel() == self.n_k * 30):
            raise ValueError(f"diagnostics: {name} is a contiguous fp64 snapshot of Simulator.{name} ([30 n_k] = {self.n_k * 30} doubles) on the GPU")
        return t

    def diagnostics(self, out=None, per_point=None, dof=None, dof_vel=None):
        """The diagnostics row of the live state — or of the snapshots `dof` / `dof_vel` — as a device tensor [25] (DIAG_FIELDS), written by two launches
        enqueued like update_force: on force_stream, between two substeps.  No host synchronisation; read_diagnostics() is the host read.
        out: the fp64 [25] device tensor to write (a row of a DiagnosticsLog); per_point: an fp64 [n_IP, 8] device tensor that receives
        (m, ke, ee, det, sig0, sig1, sig2, strain) of every point."""
        if self.dof is None or self.device.type != "cuda":
            raise RuntimeError("Simulator: diagnostics are measured on a GPU: initialize the simulator on a cuda device first")
        n = len(DIAG_FIELDS)
        if int(lib().pn_sim_diagnostics_doubles()) != n:
            raise RuntimeError(f"libpienerf_hip.so's diagnostics row has {lib().pn_sim_diagnostics_doubles()} doubles, diagnostics.py names {n}")
        if out is None:
            out = torch.empty(n, dtype=torchfloat, device=self.device)
        elif not (torch.is_tensor(out) and out.is_cuda and out.dtype == torchfloat and out.is_contiguous() and out.numel() == n):
            raise ValueError(f"diagnostics: out is a contiguous fp64 tensor of {n} doubles on the GPU")
        if per_point is not None and not (torch.is_tensor(per_point) and per_point.is_cuda and per_point.dtype == torchfloat
                                          and per_point.is_contiguous() and tuple(per_point.shape) == (self.n_IP, 8)):
            raise ValueError(f"diagnostics: per_point is a contiguous fp64 [n_IP, 8] = [{self.n_IP}, 8] tensor on the GPU")
        d, dv = self._diag_state_arg(dof, "dof"), self._diag_state_arg(dof_vel, "dof_vel")
        need = int(lib().pn_sim_diagnostics_work_doubles(self.n_IP))
        if self._diag_work is None or self._diag_work.numel() != need:
            self._diag_work = torch.empty(need, dtype=torchfloat, device=self.device)
        g = self.gravity_host   # the constructor's host copy: no device read here
        with self._on_force_stream():
            check(lib().pn_sim_diagnostics(self.n_k, self.n_IP, float(self.dx), g.ctypes.data, ptr(d), ptr(dv), ptr(self.IP_kernel), ptr(self.IP_rho),
                                           ptr(self.IP_mu), ptr(self.IP_lam), ptr(self.IP_Nx), ptr(self.IP_dNx), ptr(self.IP_ddNx), ptr(self._diag_work),
                                           ptr(out), ptr(per_point), stream_ptr()), "sim_diagnostics")
        return out

    def read_diagnostics(self, row=None):
        """A row (default: diagnostics() of the live state) as a dict on the host — diagnostics_dict: com / P / L as arrays, indices and counts as
        ints.  The one host read; like contact_count() it waits for force_stream (or the current stream) only."""
        if row is None:
            row = self.diagnostics()
        return diagnostics_dict(self._host_read(lambda: row.cpu().numpy()))

    def record_diagnostics(self, log):
        """Writes the live state's row into the next row of `log` (a DiagnosticsLog); RuntimeError when it is full.  The row index is a host counter:
        for use outside graph capture."""
        if log.count >= log.capacity:
            raise RuntimeError(f"DiagnosticsLog: full ({log.capacity} rows)")
        self.diagnostics(out=log.rows[log.count])   # may raise: the counter moves only behind it
        log.count += 1
        return log.count - 1
