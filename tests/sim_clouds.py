"""Named point clouds for the simulator tests beyond the chair: per-point materials, kernel-grid cells cut into several chunks of the substep's cell
form, and points that are no integration point's centre and name one kernel several times.  numpy + the CPU oracle only; a helper module, not a
conftest (fixtures live in the test modules, module-scoped: one oracle initialisation takes seconds).

Every cloud is built at the small scene's options (sim_dx = 0.1, sim_iters = 4, sub_res = 30: `opt()`), as the dict scene.make_chair_points returns.

  beam          a 1.4 x 0.5 x 0.5 bar along x, stiff and heavy at the pinned end (x < -0.6), soft and light at the tip, mu and lam crossing over
                between x = -0.2 and 0.2 (mu 4e6 -> 2e5, lam 1e6 -> 1.6e6), every point with seeded factors of its own on mu, lam and mass.  Its
                kernel-grid cells hold 4, 9, 27, 32 + 4 ... integration points: full chunks, cells of two chunks, ragged remainders.  Half of its
                pinned points repeat a kernel in their pts_kernel row.
  two_blocks    two disconnected pieces: a stiff dense block pinned at its base and a soft light block pinned on one face, with FREE points that
                repeat a kernel (update_pos, the mesh warp) beside pinned ones.
  beam_swapped  beam with mu and lam exchanged: what a kernel that reads the two the wrong way round would simulate.

`facts(sim)` measures what makes a cloud adversarial from a Simulator (any device) or an OracleSimulator, `check_facts` asserts it, so that a later
edit which quietly removes an edge fails the host tests.  `LOAD`, `run_schedule` and `rotate_in_cells` are what the trajectory tests and the guard
that their bar discriminates share.
"""
import numpy as np

from pienerf_amd import scene

NAMES = ("beam", "two_blocks")
SUB_RES, SIM_DX, SIM_ITERS = 30, 0.1, 4
CHUNK = 32                                 # solver.CELL_CHUNK_IPS, checked by test_sim_clouds_host
STEPS = 8                                  # substeps of a trajectory
LOAD = {"beam": ((300.0, -400.0, 200.0), (-150.0, 250.0, 350.0)),          # force from substep 2, force from substep 5 (cleared at 6)
        "two_blocks": ((200.0, 300.0, -250.0), (-300.0, 100.0, 150.0))}


def opt():
    return scene.default_opt(sim_dx=SIM_DX, sim_iters=SIM_ITERS, W=48, H=48)


def _jitter(rng, n):
    """Seeded per-point factors in [0.8, 1.25], log-uniform (so that 1 / factor has the same law)."""
    return np.exp(rng.uniform(np.log(0.8), np.log(1.25), n))


def beam():
    hgs = opt()["hash_grid_size"]
    c = scene.make_block_points((-0.7, -0.25, -0.25), (0.7, 0.25, 0.25), sub_res=SUB_RES, hgs=hgs)
    x = c["pos"][:, 0]
    n = len(x)
    rng = np.random.default_rng(20)
    t = np.clip((x + 0.2) / 0.4, 0.0, 1.0)
    c["mu"] = (4e6 * (1 - t) + 2e5 * t) * _jitter(rng, n)
    c["lam"] = (1e6 * (1 - t) + 1.6e6 * t) * _jitter(rng, n)
    c["mass"] = np.where(x < 0, 2000.0, 500.0) * _jitter(rng, n) * c["vp"]
    c["pin"] = (x < -0.6).astype(np.int32)
    return c


def two_blocks():
    hgs = opt()["hash_grid_size"]
    rng = np.random.default_rng(21)
    a = scene.make_block_points((-0.7, -0.75, -0.3), (-0.1, -0.1, 0.4), sub_res=SUB_RES, hgs=hgs)       # stiff and dense, pinned at its base
    n = len(a["pos"])
    h = np.clip((a["pos"][:, 1] + 0.75) / 0.65, 0.0, 1.0)
    a["mu"] = (6e6 * (1 - h) + 1.5e6 * h) * _jitter(rng, n)
    a["lam"] = (2e6 * (1 - h) + 4e6 * h) * _jitter(rng, n)
    a["mass"] = 3000.0 * _jitter(rng, n) * a["vp"]
    a["pin"] = (a["pos"][:, 1] < -0.68).astype(np.int32)
    b = scene.make_block_points((0.25, 0.1, -0.45), (0.8, 0.5, 0.1), sub_res=SUB_RES, hgs=hgs)          # soft and light, pinned on its +x face
    n = len(b["pos"])
    s = np.clip((0.8 - b["pos"][:, 0]) / 0.55, 0.0, 1.0)
    b["mu"] = (4e5 * (1 - s) + 1e5 * s) * _jitter(rng, n)
    b["lam"] = (1.5e5 * (1 - s) + 6e5 * s) * _jitter(rng, n)
    b["mass"] = 400.0 * _jitter(rng, n) * b["vp"]
    b["pin"] = (b["pos"][:, 0] > 0.72).astype(np.int32)
    return scene.concat_clouds(a, b)


def beam_swapped():
    c = beam()
    c["mu"], c["lam"] = c["lam"].copy(), c["mu"].copy()
    return c


BUILDERS = dict(beam=beam, two_blocks=two_blocks, beam_swapped=beam_swapped)


def make(name):
    return BUILDERS[name]()


# ------------------------------------------------------------------------------------------------ measuring a cloud
def _np(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def repeated_rows(topo):
    """[n] bool: the row of `topo` [n, 8] names some kernel more than once."""
    t = np.sort(_np(topo).astype(np.int64), axis=1)
    return (np.diff(t, axis=1) == 0).any(axis=1)


def cell_of_ip(sim):
    """The kernel-grid cell id of every integration point, by the expression precompute() uses (solver.py: IP2K)."""
    import torch
    base = sim.base if hasattr(sim.base, "dtype") else torch.as_tensor(sim.base)
    k = ((sim.IP_pos - base) // sim.kdx).to(dtype=torch.int32).long().cpu().numpy()
    return (k[:, 0] * sim.kres + k[:, 1]) * sim.kres + k[:, 2]


def facts(sim):
    """What the tests rely on, measured from a Simulator after precompute() or from an OracleSimulator."""
    cell = cell_of_ip(sim)
    _, per_cell = np.unique(cell, return_counts=True)
    chunks = []
    for n in per_cell:
        chunks += [CHUNK] * (n // CHUNK) + ([n % CHUNK] if n % CHUNK else [])
    rep = repeated_rows(sim.pts_kernel)
    pin = _np(sim.is_pin).astype(bool)
    mu, lam = _np(sim.IP_mu), _np(sim.IP_lam)
    fed = np.bincount(_np(sim.pts_IP).astype(np.int64), minlength=int(sim.n_IP))
    return dict(n_pts=len(pin), n_IP=int(sim.n_IP), n_k=int(sim.n_k), n_pin=int(pin.sum()), chunk_sizes=sorted(chunks), cells=len(per_cell),
                full_chunks=int(sum(c == CHUNK for c in chunks)), cells_of_several_chunks=int((per_cell > CHUNK).sum()),
                ragged_chunks=int(sum(c % 8 != 0 for c in chunks)), pinned_repeats=int((rep & pin).sum()), free_repeats=int((rep & ~pin).sum()),
                ip_repeats=int(repeated_rows(sim.IP_kernel).sum()), mu_ratio=float(mu.max() / mu.min()), min_mu_lam_gap=float(np.abs(mu / lam - 1.0).min()),
                fed_by=sorted(set(fed.tolist())))


def check_facts(name, f):
    assert f["full_chunks"] >= 1, (name, f["chunk_sizes"])                   # a chunk whose every lane is a point
    assert f["cells_of_several_chunks"] >= 1, (name, f["chunk_sizes"])       # a kernel collects partial sums of two chunks of one cell
    assert f["ragged_chunks"] >= 1, (name, f["chunk_sizes"])                 # lane < count inside a wave (8 points per wave)
    assert f["ip_repeats"] == 0, name                                       # an integration point's 8 kernels are distinct, always
    assert f["pinned_repeats"] >= 1, name
    if name == "two_blocks":
        assert f["free_repeats"] >= 1, name
    assert f["mu_ratio"] > 10.0 and f["min_mu_lam_gap"] > 0.0, (name, f["mu_ratio"], f["min_mu_lam_gap"])
    assert f["fed_by"][0] == 1 and f["fed_by"][-1] > 1, (name, f["fed_by"])  # means of one value and means of several


# ------------------------------------------------------------------------------------------------ trajectories
def load_point(sim, name):
    """The integration point the pick force acts on: the beam's tip, the soft block's free end."""
    p = _np(sim.IP_pos)
    return int(np.argmax(p[:, 0])) if name.startswith("beam") else int(np.argmin(np.where(p[:, 0] > 0, p[:, 0], np.inf) + 1e-3 * p[:, 1]))


def run_schedule(sim, name, steps=STEPS, after_step=None):
    """`steps` substeps of a Simulator or an OracleSimulator: force applied before substep 2, changed before 5, cleared before 6.  after_step(k, sim)
    runs behind every substep."""
    import torch
    f1, f2 = (np.array(f, np.float64) for f in LOAD["beam" if name.startswith("beam") else name])
    vid = load_point(sim, name)
    wrap = (lambda f: torch.from_numpy(f)) if hasattr(sim, "device") else (lambda f: f)
    for k in range(steps):
        if k == 2:
            sim.update_force(vid, wrap(f1))
        if k == 5:
            sim.update_force(vid, wrap(f2))
        if k == 6:
            sim.clear_force()
        sim.stepforward()
        if after_step is not None:
            after_step(k, sim)
    return sim


def rotate_in_cells(sim, values):
    """`values` [n_IP] moved on by one position inside every kernel-grid cell (the cell's points in ascending index order, cyclically): what a cell
    form whose `src` permutation is off by one would hand each lane."""
    cell = cell_of_ip(sim)
    out = np.array(values, np.float64, copy=True)
    for c in np.unique(cell):
        i = np.nonzero(cell == c)[0]
        out[i] = np.roll(np.asarray(values)[i], 1)
    return out
