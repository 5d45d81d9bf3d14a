"""The clouds of tests/sim_clouds.py on the CPU: that each keeps the edges it is there for, and everything Simulator.precompute() builds from per-point
materials, cells of several chunks and points with repeated kernels — collect_IP's means, the cell form's layout, the system matrices — against
explicit numpy and the fp64 oracle.  No kernel is launched; tests/test_gpu_sim_clouds.py runs the same clouds through the substep's three forms."""
import math

import numpy as np
import pytest
import torch

import sim_clouds as SC
from conftest import make_oracle_sim, rel_err


def cpu_simulator(cloud, opt):
    """A Simulator on the CPU up to precompute(), with the cell form's layout built whatever PN_SIM_FORM says."""
    from pienerf_amd.simulator.solver import Simulator
    s = Simulator(dt=opt["sim_dt"], iters=opt["sim_iters"], bbox=torch.tensor([2.0 * opt["bound"]] * 3), dx=opt["sim_dx"], stiff=opt["sim_stiff"],
                  base=torch.tensor([-opt["bound"]] * 3), device="cpu", persistent=False)
    s.cell_form = True
    s.initialize = s.precompute   # the tensor bookkeeping of initialize(): what runs without a GPU
    s.InitializeFromArrays(cloud["pos"], cloud["mass"], cloud["mu"], cloud["lam"], cloud["pin"])
    return s


@pytest.fixture(scope="module")
def built():
    """name -> (cloud, Simulator on the CPU after precompute(), OracleSimulator at rest), each built once."""
    opt = SC.opt()
    out = {}
    for name in SC.NAMES:
        c = SC.make(name)
        out[name] = (c, cpu_simulator(c, opt), make_oracle_sim(c, opt))
    return out


@pytest.mark.parametrize("name", SC.NAMES)
def test_clouds_keep_their_edges(built, name):
    from pienerf_amd.simulator import solver
    assert SC.CHUNK == solver.CELL_CHUNK_IPS
    c, s, ref = built[name]
    f = SC.facts(s)
    assert f == SC.facts(ref)
    print(name, {k: v for k, v in f.items() if k != "chunk_sizes"}, "chunks:", {n: f["chunk_sizes"].count(n) for n in sorted(set(f["chunk_sizes"]))})
    SC.check_facts(name, f)
    assert s._cells["n_chunks"] == len(f["chunk_sizes"]) and sorted(s._cells["tab"][:, 0].tolist()) == f["chunk_sizes"]
    if name == "beam":   # the recipe's measured shape: remainders of 4, 9 and 27 points, eight full chunks, eight cells of two chunks
        assert (f["n_pts"], f["n_IP"], f["n_k"], f["n_pin"], f["pinned_repeats"]) == (1408, 540, 54, 128, 64)
        assert {n: f["chunk_sizes"].count(n) for n in set(f["chunk_sizes"])} == {4: 8, 9: 4, 27: 8, 32: 8} and f["cells_of_several_chunks"] == 8
        assert f["fed_by"] == [1, 2, 4, 8]
        w = SC.make("beam_swapped")   # the same cloud with the two material arrays exchanged, nothing else
        assert np.array_equal(w["mu"], c["lam"]) and np.array_equal(w["lam"], c["mu"]) and all(np.array_equal(w[k], c[k]) for k in ("pos", "mass", "pin"))


@pytest.mark.parametrize("name", SC.NAMES)
def test_collect_IP_is_the_mass_weighted_mean_per_cell(built, name):
    """IP_mu = sum(m mu) / sum(m), IP_lam likewise and IP_rho = sum(m) / dx^3 over the points of each occupied cell, the cells found here from the
    positions alone and the sums taken exactly (math.fsum).  Bar 2^-48: a product (2^-53), a sum of at most 8 positive terms in any order (7 x 2^-53),
    for numerator and denominator, and a division — 17 x 2^-53 at the most, relative."""
    c, s, ref = built[name]
    pos, m, mu, lam = (np.asarray(c[k], np.float64) for k in ("pos", "mass", "mu", "lam"))
    g = np.floor((pos - s.base.numpy()[None, :]) / s.dx).astype(np.int64)
    r = [int(v) for v in s.res]
    assert (g >= 0).all() and (g < np.array(r)[None, :]).all()
    key = (g[:, 0] * r[1] + g[:, 1]) * r[2] + g[:, 2]
    cells = np.unique(key)                                    # ascending = the order IP_idx numbers the occupied cells in
    assert len(cells) == s.n_IP
    want = np.zeros((s.n_IP, 3))
    sizes = []
    for i, k in enumerate(cells):
        p = np.nonzero(key == k)[0]
        sizes.append(len(p))
        sm = math.fsum(m[p])
        want[i] = (math.fsum(m[p] * mu[p]) / sm, math.fsum(m[p] * lam[p]) / sm, sm / s.dx ** 3)
        assert np.array_equal(s.IP_grid[i].numpy(), g[p[0]])
    assert max(sizes) == 8 and min(sizes) == 1
    bar = 2.0 ** -48
    for got_sim, got_ref, col, label in ((s.IP_mu, ref.IP_mu, 0, "mu"), (s.IP_lam, ref.IP_lam, 1, "lam"), (s.IP_rho, ref.IP_rho, 2, "rho")):
        e_sim = np.abs(got_sim.numpy() / want[:, col] - 1.0).max()
        e_ref = np.abs(np.asarray(got_ref) / want[:, col] - 1.0).max()
        print(f"{name} IP_{label}: simulator {e_sim:.2e}, oracle {e_ref:.2e} relative, per cell")
        assert e_sim <= bar and e_ref <= bar
    # the means are means of DIFFERENT numbers: a cell's value is neither its first point's nor the plain average
    several = np.array(sizes) > 1
    first = np.array([mu[np.nonzero(key == k)[0][0]] for k in cells])
    plain = np.array([mu[key == k].mean() for k in cells])
    assert (np.abs(first / want[:, 0] - 1.0)[several] > 1e-3).any() and (np.abs(plain / want[:, 0] - 1.0)[several] > 1e-6).any()


@pytest.mark.parametrize("name", SC.NAMES)
def test_cell_form_layout(built, name):
    """Simulator._build_cells on cells of one and of two chunks, full and ragged: every table the cell form's kernel reads (csrc/pn_sim_cells.h)."""
    c, s, ref = built[name]
    cl = s._cells
    B, n_chunks, n_IP = cl["B"], cl["n_chunks"], s.n_IP
    src, valid, tab = cl["src"].numpy(), cl["valid"].numpy(), cl["tab"].numpy()
    assert B == SC.CHUNK and src.shape == valid.shape == (n_chunks, B) and tab.shape == (n_chunks, 12)
    # every integration point occupies exactly one valid (chunk, lane) slot; valid slots are the first tab[:, 0] of each chunk
    assert np.array_equal(np.sort(src[valid]), np.arange(n_IP))
    assert np.array_equal(valid, np.arange(B)[None, :] < tab[:, :1]) and int(tab[:, 0].sum()) == n_IP and (tab[:, 0] >= 1).all() and (tab[:, 9:] == 0).all()
    # a chunk's points lie in one kernel-grid cell, in ascending order, and the chunk's 8 kernels are theirs; chunks of one cell follow each other
    cell = SC.cell_of_ip(s)
    topo = s.IP_kernel.numpy()
    ch_cell = np.array([cell[src[b, 0]] for b in range(n_chunks)])
    for b in range(n_chunks):
        p = src[b, :tab[b, 0]]
        assert (cell[p] == ch_cell[b]).all() and (np.diff(p) > 0).all() and (topo[p] == tab[b, 1:9][None, :]).all()
    assert (np.diff(ch_cell) >= 0).all()
    for k in np.unique(ch_cell):
        counts = tab[ch_cell == k, 0]
        assert (counts[:-1] == B).all() and counts.sum() == (cell == k).sum()      # only a cell's last chunk is short
    assert (np.bincount(np.unique(ch_cell, return_inverse=True)[1]) > 1).any()
    # materials: the point's own on valid slots, 0 elsewhere
    mu_c, lam_c = cl["mu"].numpy().reshape(n_chunks, B), cl["lam"].numpy().reshape(n_chunks, B)
    assert np.array_equal(mu_c[valid], s.IP_mu.numpy()[src[valid]]) and np.array_equal(lam_c[valid], s.IP_lam.numpy()[src[valid]])
    assert (mu_c[~valid] == 0).all() and (lam_c[~valid] == 0).all() and (~valid).any()
    assert not np.array_equal(mu_c[valid], lam_c[valid]) and len(np.unique(mu_c[valid])) == n_IP     # no two points share a value: a wrong slot shows
    # shape-function gradients: [chunk][wave][15][64][2], lane l of wave w = point w * 8 + l // 8, slot l % 8, pair j = entries 2j, 2j + 1 of the 30
    g = cl["dNx"].numpy()
    assert g.shape == (n_chunks, B // 8, 15, 64, 2)
    dNx = s.IP_dNx.numpy().reshape(n_IP, 8, 30)
    for b in range(n_chunks):
        for pl in range(B):
            w, l0 = pl // 8, (pl % 8) * 8
            blk = g[b, w, :, l0:l0 + 8, :]                                           # [15, slot, 2]
            got = blk.transpose(1, 0, 2).reshape(8, 30)
            if valid[b, pl]:
                assert np.array_equal(got, dNx[src[b, pl]]), (b, pl)
            else:
                assert (got == 0).all(), (b, pl)
    # per kernel: its (chunk, slot) references, each exactly once, ascending; kp_pos is each reference's rank in that order
    kp_bg, kp_pos, kp_list = cl["kp_bg"].numpy(), cl["kp_pos"].numpy(), cl["kp_list"].numpy()
    keys = tab[:, 1:9].reshape(-1)
    assert len(kp_bg) == s.n_k + 1 and kp_bg[0] == 0 and kp_bg[-1] == 8 * n_chunks and np.array_equal(np.sort(kp_pos), np.arange(8 * n_chunks))
    for k in range(s.n_k):
        run = kp_list[kp_bg[k]:kp_bg[k + 1]]
        assert np.array_equal(run, np.nonzero(keys == k)[0])
        assert np.array_equal(kp_pos[run], np.arange(kp_bg[k], kp_bg[k + 1]))
    assert (np.diff(kp_bg) >= 2).any()   # kernels that collect from several chunks — of two-chunk cells among them:
    both = [k for k in range(s.n_k) if len(set(ch_cell[kp_list[kp_bg[k]:kp_bg[k + 1]] // 8])) < kp_bg[k + 1] - kp_bg[k]]
    assert both, "no kernel collects from two chunks of one cell"


@pytest.mark.parametrize("name", SC.NAMES)
def test_precompute_against_the_oracle(built, name):
    """The bars of test_host.test_simulator_precompute_matches_oracle_init and test_gpu_parity.test_sim_kernels_and_step."""
    c, s, ref = built[name]
    assert (s.n_IP, s.n_k) == (ref.n_IP, ref.n_k) and np.array_equal(s.IP_kernel.numpy(), ref.IP_kernel.numpy())
    assert np.array_equal(s.pts_kernel.numpy(), ref.pts_kernel.numpy()) and np.array_equal(s.pts_IP.numpy(), ref.pts_IP.numpy())
    assert np.array_equal(s.active_kernels.numpy(), ref.active)
    for a, b, label in ((s.IP_Nx, ref.IP_Nx, "IP_Nx"), (s.IP_dNx, ref.IP_dNx, "IP_dNx"), (s.IP_ddNx, ref.IP_ddNx, "IP_ddNx"), (s.pts_Nx, ref.pts_Nx, "pts_Nx"),
                        (s.Mmat, ref.Mmat, "Mmat")):
        e = rel_err(a.numpy(), b)
        print(f"{name} {label}: {e:.2e}")
        assert e < 1e-12, label
    e_A, e_g = rel_err(s.Ainv.numpy(), ref.Ainv), rel_err(s.rhs_gravity.numpy().reshape(-1, 3), ref.rhs_gravity)
    print(f"{name} Ainv: {e_A:.2e}, rhs_gravity: {e_g:.2e}")
    assert e_A < 1e-8 and e_g < 1e-12


def _oracle_run(cloud, name, change=None):
    ref = make_oracle_sim(cloud, SC.opt())
    if change is not None:
        change(ref)
    SC.run_schedule(ref, name)
    return ref.dof - ref.dof_rest


@pytest.fixture(scope="module")
def oracle_runs(built):
    return {name: _oracle_run(built[name][0], name) for name in SC.NAMES}


def test_the_bar_tells_swapped_materials_apart(oracle_runs):
    """The trajectory tests hold the kernels to 1e-4 of the oracle's displacements.  A kernel that reads mu for lam would compute the oracle's
    beam_swapped trajectory: more than 100 bars away."""
    d = rel_err(_oracle_run(SC.make("beam_swapped"), "beam_swapped"), oracle_runs["beam"])
    print(f"beam_swapped vs beam, oracle displacements after {SC.STEPS} substeps: {d:.3g} relative")
    assert d > 100 * 1e-4


@pytest.mark.parametrize("name", SC.NAMES)
def test_the_bar_tells_a_rotated_permutation_apart(built, oracle_runs, name):
    """... and so would one whose lanes take the material of the next point of their kernel-grid cell (a wrong `src` in _build_cells): the oracle with
    IP_mu / IP_lam moved on by one position inside every cell for the substeps (the system matrices and rhs_rest left as they are, as the simulator's
    would be: they are built from IP_mu itself, not from the cell form's copy)."""
    def rotate(ref):
        ref.IP_mu, ref.IP_lam = SC.rotate_in_cells(ref, ref.IP_mu), SC.rotate_in_cells(ref, ref.IP_lam)
    d = rel_err(_oracle_run(built[name][0], name, rotate), oracle_runs[name])
    print(f"{name}: rotated materials vs own, oracle displacements after {SC.STEPS} substeps: {d:.3g} relative")
    assert d > 100 * 1e-4

