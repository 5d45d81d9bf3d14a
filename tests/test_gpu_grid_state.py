"""The density-grid sweep, exact: every kernel of pn_grid_state.hip and the sigma-only launch of the fused network (pn_nerf_sigma) against the numpy
restatements of oracle/training.py, at grid sizes that leave ragged blocks — (cascade, H, bound) = (3, 4, 4.0): one block of 192 cells; (1, 8, 1.0):
two full blocks; (2, 32, 2.0): many blocks, two cascades — and NeRFRenderer.update_extra_state's partial sweep end to end at the renderer's own size
with its random draws replayed.  Integer and index work is bit-exact; the mean of the grid is held to 1e-6 relative (a sum in another order)."""
import numpy as np
import pytest
import torch

import oracle
from oracle import training as otr
from pienerf_amd import scene
from pienerf_amd._lib import check, lib, ptr, stream_ptr
from pienerf_amd.nerf.network import NeRFNetwork
from test_gpu_netform import _model
from test_gpu_parity import DEV, T

pytestmark = pytest.mark.gpu

GRIDS = ((3, 4, 4.0), (1, 8, 1.0), (2, 32, 2.0))
bits = lambda a: np.asarray(a, np.float32).view(np.uint32)


def _partial(cas, H, bound, coords, pick, noise, grid_cas):
    """pn_density_cells_partial on host arrays -> (indices, xyzs, tmp)."""
    N = len(coords)
    scratch = torch.empty(int(lib().pn_density_partial_scratch_ints(H)), dtype=torch.int32, device=DEV)
    idx = torch.full((2 * N,), -7, dtype=torch.int32, device=DEV)
    pts = torch.full((2 * N, 3), float("nan"), device=DEV)
    tmp = torch.zeros(H ** 3, device=DEV)
    tc, tp, tn, tg = T(coords.astype(np.int32)), T(pick), T(noise), T(grid_cas)
    check(lib().pn_density_cells_partial(cas, H, bound, N, ptr(tc), ptr(tp), ptr(tn), ptr(tg), ptr(tmp), ptr(scratch), ptr(idx), ptr(pts), stream_ptr()),
          "partial")
    return idx.cpu().numpy(), pts.cpu().numpy(), tmp.cpu().numpy()


@pytest.mark.parametrize("cascade,H,bound", GRIDS)
def test_mark_untrained_and_full_sweep_cells_bit_exact(cascade, H, bound):
    poses = np.stack([scene.orbit_pose(0.8 * bound, a, e) for a, e in ((0.0, -20.0), (35.0, -10.0), (200.0, -50.0))]).astype(np.float32)
    intr = scene.orbit_intrinsics(64, 48, 30.0)
    n = cascade * H ** 3
    grid, n_unseen = torch.zeros(n, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    cams = T(poses)
    check(lib().pn_mark_untrained_grid(ptr(cams), len(poses), *[float(v) for v in intr], cascade, H, bound, ptr(grid), ptr(n_unseen), stream_ptr()), "mark")
    want = otr.mark_untrained_grid(poses, intr, cascade, H, bound).reshape(-1)
    got = grid.cpu().numpy()
    assert 0 < want.sum() < n and int(n_unseen) == int(want.sum())
    assert np.array_equal(got == -1, want) and np.array_equal(got[~want], np.zeros(n - want.sum(), np.float32))
    noise = np.random.default_rng(H).random((n, 3)).astype(np.float32)
    pts = torch.full((n + 1, 3), float("nan"), device=DEV)
    tn = T(noise)
    check(lib().pn_density_cells_full(cascade, H, bound, ptr(tn), ptr(pts), stream_ptr()), "cells")
    ref = otr.density_cells_full(cascade, H, bound, noise)
    assert np.array_equal(bits(pts[:n].cpu().numpy()), bits(ref)) and bool(torch.isnan(pts[n]).all())   # nothing behind the last cell is written
    for cas in range(cascade):   # each cascade spans its own bound
        b = min(2.0 ** cas, bound)
        assert 0.5 * b < np.abs(ref[cas * H ** 3:(cas + 1) * H ** 3]).max() <= b


@pytest.mark.parametrize("cascade,H,bound", GRIDS)
@pytest.mark.parametrize("occupied", ["none", "one", "all", "random"])
def test_partial_sweep_cells_bit_exact(cascade, H, bound, occupied):
    """indices and xyzs of both halves bit for bit, tmp == -1 everywhere.  rand_pick carries 0, nextafter(1, 0) and values landing exactly on j / n_occ
    (where float32(u) * float32(n_occ) decides between two neighbours of the occupied list); every cascade of the grid uses its own bound."""
    rng = np.random.default_rng(1000 * H + len(occupied))
    cells = H ** 3
    N = max(cells // 4, 16) + 3   # ragged against the 256-lane block at every size
    for cas in range(cascade):
        g = {"none": np.zeros(cells), "one": np.zeros(cells), "all": rng.uniform(0.1, 9, cells), "random": rng.uniform(-1, 1, cells)}[occupied]
        g = g.astype(np.float32)
        if occupied == "one":
            g[cells - 3] = 2.0
        if occupied == "random":
            g[g < 0] = -1
            g[:2] = (0.0, -0.0)   # not occupied: > 0 is strict
        n_occ = int((g > 0).sum())
        pick = rng.random(N).astype(np.float32)
        pick[0], pick[1] = 0.0, np.nextafter(np.float32(1), np.float32(0))
        if n_occ > 1:
            js = rng.integers(0, n_occ, 8)
            pick[2:10] = (js / n_occ).astype(np.float32)   # rounds to either side of j / n_occ
            pick[10:12] = np.nextafter(pick[2:4], np.float32(0))
        coords = rng.integers(0, H, (N, 3))
        coords[0], coords[1] = 0, H - 1
        noise = rng.random((2 * N, 3)).astype(np.float32)
        noise[0], noise[N] = 0.0, np.nextafter(np.float32(1), np.float32(0))
        idx, pts, tmp = _partial(cas, H, bound, coords, pick, noise, g)
        ridx, rpts, rtmp = otr.density_cells_partial(cas, H, bound, coords, pick, noise, g)
        assert np.array_equal(idx, ridx), (cas, np.flatnonzero(idx != ridx)[:5])
        assert np.array_equal(bits(pts), bits(rpts)) and np.array_equal(tmp, rtmp) and (tmp == -1).all()
        if n_occ:
            assert (g[idx[N:]] > 0).all() and idx[N] == np.flatnonzero(g > 0)[0] and idx[N + 1] == np.flatnonzero(g > 0)[-1]
        else:
            assert (idx[N:] == -1).all() and not pts[N:].any()


@pytest.mark.parametrize("n", [0, 1, 255, 257])
def test_density_scatter(n):
    """A cell indexed more than once keeps whichever store lands last: every written cell holds one of the values sent to it; cells not indexed and
    indices of -1 leave the grid alone."""
    rng = np.random.default_rng(n)
    cells = 192
    idx = rng.integers(0, cells // 2, n).astype(np.int32)   # the upper half is never indexed; duplicates are many
    idx[1::5] = -1
    sig = rng.uniform(0, 50, n).astype(np.float32)
    before = rng.uniform(-1, 1, cells).astype(np.float32)
    tmp = T(before)
    ti, ts = (T(idx), T(sig)) if n else (None, None)
    check(lib().pn_density_scatter(n, ptr(ti), ptr(ts), ptr(tmp), stream_ptr()), "scatter")
    got = tmp.cpu().numpy()
    ref, ambiguous = otr.density_scatter(idx, sig, before)
    hit = np.zeros(cells, bool)
    hit[idx[idx >= 0]] = True
    assert np.array_equal(bits(got[~hit]), bits(before[~hit]))
    assert np.array_equal(bits(got[hit & ~ambiguous]), bits(ref[hit & ~ambiguous]))
    for c in np.flatnonzero(ambiguous):
        assert got[c] in sig[idx == c]
    if n:
        assert hit.any() and (n < 255 or ambiguous.any())


def _update(g0, t0, decay, thresh):
    n = g0.size
    grid, tmp = T(g0.reshape(-1)), T(t0.reshape(-1))
    bf = torch.full((n // 8 + 1,), 0xAA, dtype=torch.uint8, device=DEV)
    partial = torch.empty((n + 255) // 256, dtype=torch.float64, device=DEV)
    mt = torch.empty(2, device=DEV)
    check(lib().pn_density_grid_update(n, ptr(grid), ptr(tmp), decay, thresh, ptr(bf), ptr(partial), ptr(mt), stream_ptr()), "update")
    assert int(bf[-1]) == 0xAA   # nothing behind the last byte is written
    return grid.cpu().numpy(), bf[:-1].cpu().numpy(), mt.cpu().numpy()


@pytest.mark.parametrize("cascade,H,bound", GRIDS)
@pytest.mark.parametrize("side", ["thresh_below_mean", "thresh_above_mean", "inf"])
def test_density_grid_update_planted_cells(cascade, H, bound, side):
    rng = np.random.default_rng(H)
    n = cascade * H ** 3
    g0 = rng.uniform(-0.5, 30, n).astype(np.float32)
    g0[g0 < 0] = -1
    t0 = rng.uniform(-0.5, 30, n).astype(np.float32)
    t0[t0 < 0] = -1
    thresh = np.float32(10.0 if side != "thresh_above_mean" else 25.0)
    f, nan, inf = np.float32, np.float32(np.nan), np.float32(np.inf)
    # (g, t) planted into the last (ragged, where there is one) block and the first
    plant = [(-1, 5), (0, 5), (0, -1), (-0.0, 5), (-0.0, -1), (5, -1), (5, 0), (5, nan), (-1, nan), (thresh, -1), (np.nextafter(thresh, inf), -1),
             (thresh / f(0.95), 0), (1, thresh), (1, np.nextafter(thresh, inf))]
    if side == "inf":
        plant.append((3, inf))
    for k, (g, t) in enumerate(plant):
        for at in (k, n - 1 - k):
            g0[at], t0[at] = g, t
    grid, bf, mt = _update(g0, t0, 0.95, float(thresh))
    g_ref, mean_ref, bits_ref = otr.density_grid_update(g0, t0, 0.95, float(thresh))
    assert np.array_equal(bits(grid), bits(g_ref))
    if side == "inf":
        assert mt[0] == inf and mean_ref == np.inf and mt[1] == thresh
    else:
        assert abs(float(mt[0]) - mean_ref) < 1e-6 * mean_ref
        assert (mean_ref > thresh) == (side == "thresh_below_mean") and mt[1] == min(mt[0], thresh)
    if side != "thresh_above_mean":   # the threshold is density_thresh itself: the planted cells at it and one ulp above decide exactly
        assert np.array_equal(bf, bits_ref)
        cells = np.unpackbits(bf, bitorder="little")
        assert cells[9] == 0 and cells[10] == 1 and cells[12] == 0 and cells[13] == 1
    else:             # the threshold is the mean, a sum in another order: cells within its error may fall either way
        cells, want = np.unpackbits(bf, bitorder="little"), np.unpackbits(bits_ref, bitorder="little")
        differ = cells != want
        assert np.array_equal(bf, oracle.packbits(grid, float(mt[1]))) and (np.abs(g_ref[differ] - mean_ref) <= 1e-6 * mean_ref).all()


# ---------------------------------------------------------------------------------------------------------------- pn_nerf_sigma
SIGMA_SIZES = (1, 31, 32, 33, 4099, 65536 + 33, 131072 + 33)   # the last two: one ragged tile past one pass of the capped grid (fp32 / fp16 form)
_SIGMA_POINTS = {}


def _sigma_points(M):
    if M not in _SIGMA_POINTS:
        x = ((np.random.default_rng(M).random((M, 3)) * 2 - 1) * 0.95).astype(np.float32)
        x[M // 2] = (1.5, 0.0, 0.0)   # outside the bound: encodes to zero
        _SIGMA_POINTS[M] = x
    return _SIGMA_POINTS[M]


_NETS = {}


def _net(ckpt, form):
    if form not in _NETS:
        _NETS[form] = _model(ckpt, "bf16" if form == "bf16" else None)
    return _NETS[form]


def _sigma(net, x, scale, half):
    M = x.shape[0]
    out = torch.full((M + 70,), float("nan"), device=DEV)
    check(lib().pn_nerf_sigma(net._net_handle(half=bool(half)), ptr(x), M, float(scale), ptr(out), int(half), stream_ptr()), "nerf_sigma")
    assert bool(torch.isnan(out[M:]).all())           # nothing behind the last sample is written
    return out[:M].cpu().numpy()


@pytest.mark.parametrize("form", ["fp16_hilo", "bf16", "half"])
@pytest.mark.parametrize("M", SIGMA_SIZES)
def test_nerf_sigma(ckpt, form, M):
    """The sigma-only launch: bit for bit NeRFNetwork.density's sigma at density_scale 1, float32(scale) times it from one fp32 multiply otherwise
    (tile_sigma_out: density_scale * expf(logit)), no sample skipped (the buffer starts as NaN) and none written behind M."""
    half = form == "half"
    net = _net(ckpt, form)
    assert half or lib().pn_net_form(net._net) == (0 if form == "bf16" else 2)
    xh = _sigma_points(M)
    x = T(xh)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=half):
        want = net.density(x)["sigma"].cpu().numpy()
    one = _sigma(net, x, 1.0, half)
    assert not np.isnan(one).any() and np.array_equal(bits(one), bits(want))
    for scale in (0.5, 3.7):
        assert np.array_equal(bits(_sigma(net, x, scale, half)), bits(np.float32(scale) * want)), scale
    if half:
        with oracle.half_precision():
            ref, _ = oracle.nerf_forward(xh, np.tile(np.float32([0, 0, 1]), (M, 1)), ckpt, 1.0)
        rel = np.abs(one / ref - 1)
        assert rel.max() < 1.2e-2 and (M < 4099 or np.mean(rel < 1e-6) > 0.97)   # test_gpu_half.py's bars: <= 3 ulps of a half logit, the bulk equal
    else:
        ref, _ = oracle.nerf_forward(xh, np.tile(np.float32([0, 0, 1]), (M, 1)), ckpt, 1.0)
        assert np.abs(one / ref - 1).max() < 1e-4
    assert one[M // 2] == 1.0   # the point outside the bound: zero features, logit 0


# ---------------------------------------------------------------------------------------------------------------- update_extra_state, end to end
class _Replay:
    """torch.rand / torch.randint that record what they hand out."""

    def __init__(self, monkeypatch):
        self.rand, self.randint = [], []
        real_rand, real_randint = torch.rand, torch.randint

        def rand(*a, **k):
            t = real_rand(*a, **k)
            self.rand.append(t.clone())
            return t

        def randint(*a, **k):
            t = real_randint(*a, **k)
            self.randint.append(t.clone())
            return t

        monkeypatch.setattr(torch, "rand", rand)
        monkeypatch.setattr(torch, "randint", randint)


def test_update_extra_state_partial_sweep_equals_the_numpy_chain(monkeypatch):
    """Both cascades of the bound-2 model, H = 128: after a partial sweep the grid, the bitfield and the mean equal density_cells_partial -> the
    device's sigma at those points (an input) -> density_scatter -> density_grid_update on the recorded draws.  A cell drawn more than once keeps
    whichever store lands last: it must hold EXACTLY what one of its draws gives.  (The sweep makes H^3 / 2 draws per cascade over H^3 cells, all of
    them occupied in this model: by Poisson's law a quarter of the drawn cells are drawn twice or more — 401 054 of 1 605 033 here — so leaving such
    cells out, capped at a few percent, is not an option; they are checked against their candidates instead and nothing is left out.)"""
    ck = scene.make_checkpoint(bound=2.0, seed=3, shaped=True)
    net = NeRFNetwork(encoding="hashgrid", bound=2.0, cuda_ray=True, density_thresh=10, density_scale=1.5).to(DEV).load_checkpoint_dict(ck)
    H, cells, n = 128, 128 ** 3, 128 ** 3 // 4
    f = np.float32
    net.reset_extra_state()
    poses = np.stack([scene.orbit_pose(5.0, a, -20.0) for a in (0.0, 40.0)])
    assert net.mark_untrained_grid(poses, scene.orbit_intrinsics(64, 64, 25.0)) > 0   # some cells are -1 and must stay so
    torch.manual_seed(0)
    net.update_extra_state()
    g0 = net.density_grid.cpu().numpy().copy()
    assert ((g0 > 0).sum(1) > 1000).all() and (g0 == -1).any()
    net.iter_density = 16
    rec = _Replay(monkeypatch)
    net.update_extra_state(decay=0.9)
    monkeypatch.undo()
    assert net.iter_density == 17 and len(rec.randint) == 2 and len(rec.rand) == 4
    got = net.density_grid.cpu().numpy()
    tmp = np.empty_like(g0)
    ambiguous = np.zeros_like(g0, bool)
    for cas in range(2):
        coords, pick, noise = rec.randint[cas].cpu().numpy(), rec.rand[2 * cas].cpu().numpy(), rec.rand[2 * cas + 1].cpu().numpy()
        assert coords.shape == (n, 3) and pick.shape == (n,) and noise.shape == (2 * n, 3)
        idx, pts, fresh = otr.density_cells_partial(cas, H, 2.0, coords, pick, noise, g0[cas])
        assert (idx >= 0).all() and (g0[cas][idx[n:]] > 0).all() and (g0[cas][idx[:n]] == -1).any()
        sig = torch.empty(2 * n, device=DEV)
        tp = T(pts)
        check(lib().pn_nerf_sigma(net._net_handle(), ptr(tp), 2 * n, 1.5, ptr(sig), 0, stream_ptr()), "nerf_sigma")
        sig = sig.cpu().numpy()
        assert (sig > 0).all()
        tmp[cas], ambiguous[cas] = otr.density_scatter(idx, sig, fresh)
        # every drawn cell holds what ONE of its draws gives: max(decay * old, sigma) where the cell is seen, the old -1 where it is not
        old = g0[cas][idx]
        cand = np.where(old >= 0, np.maximum(old * f(0.9), sig), old)
        held, drawn = np.zeros(cells, bool), np.zeros(cells, bool)
        np.logical_or.at(held, idx, bits(cand) == bits(got[cas][idx]))
        drawn[idx] = True
        assert held[drawn].all(), (cas, int((drawn & ~held).sum()))
        assert np.array_equal(bits(got[cas][~drawn]), bits(g0[cas][~drawn]))     # a cell nobody drew is left alone (no decay either)
    share = ambiguous.sum() / ((tmp >= 0) | ambiguous).sum()
    print(f"\npartial sweep: {int(ambiguous.sum())} cells received different sigmas, {share:.3f} of the drawn cells")
    g_ref, _, _ = otr.density_grid_update(g0, tmp, 0.9, 10.0)
    keep = ~ambiguous
    assert np.array_equal(bits(got[keep]), bits(g_ref[keep]))                    # the chain itself, wherever it is single-valued
    # mean and bitfield of the chain, the many-valued cells at the value the device kept
    _, mean_ref, bits_ref = otr.density_grid_update(np.where(ambiguous, got, g0), np.where(ambiguous, f(-1), tmp), 0.9, 10.0)
    assert abs(net.mean_density - mean_ref) < 1e-6 * mean_ref
    assert np.array_equal(net.density_bitfield.cpu().numpy(), oracle.packbits(got, min(net.mean_density, net.density_thresh)))
    if mean_ref > 1.001 * net.density_thresh:   # the threshold is density_thresh itself, not a sum: the chain's own bitfield, bit for bit
        assert np.array_equal(net.density_bitfield.cpu().numpy(), bits_ref)
