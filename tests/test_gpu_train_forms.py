"""Both forms of the training ray ops (pienerf_amd/csrc/pn_train_ops.hip): the wave-per-ray kernels that N <= 131072 ray rows take and the lane-per-ray
kernels above it, on the same designed inputs (tests/train_forms_cases.py) — rays of up to 513 samples that leave at chosen samples, so that the
wave form's carry across 64-sample windows and both window edges are hit by many rays, embedded into batches on either side of the threshold.

Bars.  Composite: every ray and every sample within GPU_FACTOR x ORACLE_VS_F64 of the float64 autograd reference, in per-ray / per-sample units
(train_forms_cases.composite_errors), and within the suite's fp32-oracle bars (1e-5; 1e-4 for grad_sigmas) per ray; what the op does not write is
untouched, exactly.  March: bit for bit against the oracle and between the forms."""
import functools

import numpy as np
import pytest
import torch

import train_forms_cases as tfc
from oracle import training as otr
from pienerf_amd import scene
from pienerf_amd._lib import check, lib, ptr, stream_ptr
from test_gpu_parity import DEV, T
from test_gpu_training import _rays

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0     # finite, odd, nothing the op computes: plain equality tells written from untouched
N_WAVE, N_LANE = tfc.WAVE_FORM_MAX_N, tfc.WAVE_FORM_MAX_N + 77
OUTPUTS = ("weights_sum", "depth", "image", "grad_rgbs", "grad_sigmas")


# ------------------------------------------------------------------------------------------------ composite
@functools.lru_cache(maxsize=None)
def _case(T_thresh):
    """The designed batch, its float64 reference and the fp32 oracle's outputs — computed once per threshold, read-only afterwards."""
    b = tfc.composite_cases(T_thresh, np.random.default_rng(tfc.SEED))
    ref = tfc.composite_ref64(b["sigmas"], b["rgbs"], b["deltas"], b["rays"], T_thresh, b["grad_weights_sum"], b["grad_image"])
    ws, depth, image = otr.composite_rays_train_forward(b["sigmas"], b["rgbs"], b["deltas"], b["rays"], T_thresh)
    gs, gc = otr.composite_rays_train_backward(b["grad_weights_sum"], b["grad_image"], b["sigmas"], b["rgbs"], b["deltas"], b["rays"], ws, image, T_thresh)
    orc = dict(weights_sum=ws, depth=depth, image=image, grad_sigmas=gs, grad_rgbs=gc)
    for d in (b, ref, orc):
        for v in d.values():
            v.setflags(write=False)
    return b, ref, orc


def _composite_abi(b, rays, gws, gim, M, T_thresh):
    """Forward then backward through the C ABI on sentinel-filled outputs; the backward reads the forward's weights_sum / image like the autograd
    Function does.  Every buffer has its full size whatever M is passed, so a row the budget should drop shows as a lost sentinel."""
    N, M_full = len(rays), len(b["sigmas"])
    ts, tc, td = (torch.tensor(b[k], device=DEV) for k in ("sigmas", "rgbs", "deltas"))      # copies: the shared case is read-only
    tr, tgw, tgi = T(rays), T(gws), T(gim)
    ws, depth = (torch.full((N,), SENTINEL, device=DEV) for _ in range(2))
    image = torch.full((N, 3), SENTINEL, device=DEV)
    gs, gc = torch.full((M_full,), SENTINEL, device=DEV), torch.full((M_full, 3), SENTINEL, device=DEV)
    check(lib().pn_composite_rays_train_forward(ptr(ts), ptr(tc), ptr(td), ptr(tr), M, N, T_thresh, ptr(ws), ptr(depth), ptr(image), stream_ptr()))
    check(lib().pn_composite_rays_train_backward(ptr(tgw), ptr(tgi), ptr(ts), ptr(tc), ptr(td), ptr(tr), ptr(ws), ptr(image), M, N, T_thresh, ptr(gs),
                                                 ptr(gc), stream_ptr()))
    torch.cuda.synchronize()
    return dict(weights_sum=ws.cpu().numpy(), depth=depth.cpu().numpy(), image=image.cpu().numpy(), grad_sigmas=gs.cpu().numpy(),
                grad_rgbs=gc.cpu().numpy())


@functools.lru_cache(maxsize=None)
def _run(T_thresh, N_total):
    """The designed batch embedded into N_total rows, run in full and with the point budget cut at a mid-batch ray.
    -> (full, cut, M_cut, padded rays, pos); `full` / `cut` hold the raw outputs ("raw", indexed by the padded batch's ray index) and the designed
    rays' outputs moved back to the designed batch's ray indices."""
    b, _, _ = _case(T_thresh)
    rays = b["rays"]
    padded, pos = tfc.pad_rows(rays, N_total, np.random.default_rng(N_total))
    rng = np.random.default_rng(5)
    gws, gim = rng.standard_normal(N_total).astype(np.float32), rng.standard_normal((N_total, 3)).astype(np.float32)
    gws[padded[pos, 0]], gim[padded[pos, 0]] = b["grad_weights_sum"][rays[:, 0]], b["grad_image"][rays[:, 0]]
    M_cut = int(rays[len(rays) // 2, 1])

    def designed(raw):
        out = dict(raw=raw, grad_sigmas=raw["grad_sigmas"], grad_rgbs=raw["grad_rgbs"])
        for k in ("weights_sum", "depth", "image"):
            out[k] = np.empty_like(raw[k][:len(rays)])
            out[k][rays[:, 0]] = raw[k][padded[pos, 0]]
        return out

    full = designed(_composite_abi(b, padded, gws, gim, len(b["sigmas"]), T_thresh))
    cut = designed(_composite_abi(b, padded, gws, gim, M_cut, T_thresh))
    return full, cut, M_cut, padded, pos


@pytest.mark.parametrize("N_total", [None, N_WAVE, N_LANE], ids=["designed", "wave131072", "lane131149"])
@pytest.mark.parametrize("T_thresh", tfc.T_THRESHES)
def test_composite_train_against_float64_and_oracle(T_thresh, N_total):
    b, ref, orc = _case(T_thresh)
    rays = b["rays"]
    N = len(rays)
    full, cut, M_cut, padded, pos = _run(T_thresh, N if N_total is None else N_total)
    args = (rays, b["deltas"], b["grad_weights_sum"], b["grad_image"], ref["written"])
    # against the float64 reference: every ray, every sample
    e64 = {k: float(v.max()) for k, v in tfc.composite_errors(full, ref, *args).items()}
    e32 = {k: float(v.max()) for k, v in tfc.composite_errors(full, orc, *args, per_ray_max=True).items()}
    print(f"\nT_thresh {T_thresh:g}, N {len(padded)}: vs float64 " + ", ".join(f"{k} {e64[k]:.3e}" for k in OUTPUTS))
    print("    in units of ORACLE_VS_F64 " + ", ".join(f"{k} {e64[k] / tfc.ORACLE_VS_F64[T_thresh][k]:.2f}" for k in OUTPUTS))
    print("    vs the fp32 oracle, per ray " + ", ".join(f"{k} {e32[k]:.3e}" for k in OUTPUTS))
    for k in OUTPUTS:
        assert e64[k] <= tfc.GPU_FACTOR * tfc.ORACLE_VS_F64[T_thresh][k], (k, e64[k])
    for k in OUTPUTS:
        assert e32[k] < tfc.ORACLE_BARS[k], (k, e32[k])
    # exit semantics, exact: nothing after a ray's exit sample is written; empty rows write zeros at their index and touch no gradient
    raw = full["raw"]
    assert (raw["grad_sigmas"][~ref["written"]] == SENTINEL).all() and (raw["grad_rgbs"][~ref["written"]] == SENTINEL).all()
    assert (raw["grad_sigmas"][ref["written"]] != SENTINEL).all() and (raw["grad_rgbs"][ref["written"]] != SENTINEL).all()
    dead = np.ones(len(padded), bool)
    dead[pos] = False
    assert dead.sum() == len(padded) - N and not padded[dead, 2].any()
    for k in ("weights_sum", "depth", "image"):
        assert not raw[k][padded[dead, 0]].any(), k
        assert (raw[k][padded[pos, 0]] != SENTINEL).all(), k


@pytest.mark.parametrize("N_total", [None, N_WAVE, N_LANE], ids=["designed", "wave131072", "lane131149"])
@pytest.mark.parametrize("T_thresh", tfc.T_THRESHES)
def test_composite_train_point_budget(T_thresh, N_total):
    """M cut at the offset of a mid-batch ray: that ray and every later one are dropped whole (zeros, gradients untouched), the earlier ones do not change."""
    b, ref, _ = _case(T_thresh)
    rays = b["rays"]
    full, cut, M_cut, padded, pos = _run(T_thresh, len(rays) if N_total is None else N_total)
    kept = rays[:, 1] + rays[:, 2] <= M_cut
    assert 0 < M_cut < len(b["sigmas"]) and kept.sum() == len(rays) // 2 and (rays[~kept, 2] > 0).all()
    for k in ("weights_sum", "depth", "image"):
        assert not cut[k][rays[~kept, 0]].any(), k
        assert np.array_equal(cut[k][rays[kept, 0]], full[k][rays[kept, 0]]), k
        live = np.zeros(len(padded), bool)
        live[padded[pos[kept], 0]] = True
        assert not cut["raw"][k][~live].any(), k
    for k in ("grad_sigmas", "grad_rgbs"):
        assert (cut[k][M_cut:] == SENTINEL).all(), k
        assert np.array_equal(cut[k][:M_cut], full[k][:M_cut]), k


@pytest.mark.parametrize("T_thresh", tfc.T_THRESHES)
def test_composite_train_forms_agree(T_thresh):
    """The designed rows through the wave form (131072 rows) and through the lane form (131149 rows): same values within the per-ray fp32 bars, same
    set of written samples."""
    b, ref, _ = _case(T_thresh)
    wave, lane = _run(T_thresh, N_WAVE)[0], _run(T_thresh, N_LANE)[0]
    err = tfc.composite_errors(lane, wave, b["rays"], b["deltas"], b["grad_weights_sum"], b["grad_image"], ref["written"], per_ray_max=True)
    print(f"\nT_thresh {T_thresh:g}: lane form vs wave form, per ray " + ", ".join(f"{k} {float(err[k].max()):.3e}" for k in OUTPUTS))
    for k in OUTPUTS:
        assert float(err[k].max()) < tfc.ORACLE_BARS[k], k
    for k in ("grad_sigmas", "grad_rgbs"):
        assert np.array_equal(lane[k] == SENTINEL, wave[k] == SENTINEL), k


# ------------------------------------------------------------------------------------------------ march
def _march_abi(ck, o, d, nears, fars, noise, N, bound, dt_gamma, max_steps, M, rows):
    """pn_march_rays_train on the first N rays with point budget M; the sample buffers have `rows` rows and start zeroed like the oracle's."""
    to, td, tg, tn, tf, tz = T(o), T(d), T(ck["density_bitfield"]), T(nears), T(fars), T(noise)
    xyzs, dirs, deltas = (torch.zeros(rows, k, device=DEV) for k in (3, 3, 2))
    rays = torch.full((len(o), 3), -7, dtype=torch.int32, device=DEV)
    counter = torch.zeros(2, dtype=torch.int32, device=DEV)
    check(lib().pn_march_rays_train(ptr(to), ptr(td), ptr(tg), bound, dt_gamma, max_steps, N, ck["cascade"], ck["grid_size"], M, ptr(tn), ptr(tf), ptr(xyzs),
                                    ptr(dirs), ptr(deltas), ptr(rays), ptr(counter), ptr(tz), stream_ptr()))
    torch.cuda.synchronize()
    return tuple(a.cpu().numpy() for a in (xyzs, dirs, deltas, rays, counter))


@functools.lru_cache(maxsize=None)
def _march_case(bound, dt_gamma, max_steps, N_total):
    """The orbit view's rays that meet occupied cells, with a seeded noise vector, embedded into N_total rays that meet nothing (far = near)."""
    ck = scene.make_checkpoint(bound=bound, seed=1)
    o, d, nears, fars = _rays(bound, 64)
    noise = np.random.default_rng(11).random(len(o)).astype(np.float32)
    grid, C, H = ck["density_bitfield"], ck["cascade"], ck["grid_size"]
    first = otr.march_rays_train(o, d, bound, grid, C, H, nears, fars, None, -1, noise, -1, False, dt_gamma, max_steps)
    live = first[3][:, 2] > 0
    total = int(first[3][:, 2].sum())
    assert 200 < live.sum() < len(o) and total > 1000        # 846 rays / 15213 samples at bound 1, 231 / 1330 at bound 2
    lo, ld, ln, lf, lz = o[live], d[live], nears[live], fars[live], noise[live]
    po, pd, pn, pf, pz, pos = tfc.pad_march_rays(lo, ld, ln, lf, lz, N_total)
    return dict(ck=ck, live=(lo, ld, ln, lf, lz), padded=(po, pd, pn, pf, pz), pos=pos, total=total, counts=first[3][live, 2])


def _gather(rays_rows):
    """Sample indices of the given ray rows, in row order, through their own (offset, count)."""
    off, cnt = rays_rows[:, 1].astype(np.int64), rays_rows[:, 2].astype(np.int64)
    start = np.cumsum(cnt) - cnt
    return np.repeat(off - start, cnt) + np.arange(int(cnt.sum()))


@pytest.mark.parametrize("bound,dt_gamma,max_steps", [(1.0, 0.0, 256), (2.0, 1.0 / 128, 300)])
def test_march_rays_train_lane_form_bit_exact(bound, dt_gamma, max_steps):
    c = _march_case(bound, dt_gamma, max_steps, N_LANE)
    ck, total, pos = c["ck"], c["total"], c["pos"]
    grid, C, H = ck["density_bitfield"], ck["cascade"], ck["grid_size"]
    po, pd, pn, pf, pz = c["padded"]
    for M in (total, total // 3):
        cref = np.zeros(2, np.int32)
        ref = otr.march_rays_train(po, pd, bound, grid, C, H, pn, pf, cref, M, pz, -1, False, dt_gamma, max_steps)
        got = _march_abi(ck, po, pd, pn, pf, pz, N_LANE, bound, dt_gamma, max_steps, M, total)
        assert np.array_equal(got[4], cref) and tuple(cref) == (total, N_LANE)        # demand, not what fitted
        rays = got[3]
        assert np.array_equal(rays, ref[3])
        assert np.array_equal(rays[:, 0], np.arange(N_LANE)) and np.array_equal(rays[pos, 2], c["counts"])
        assert np.array_equal(rays[:, 1], np.cumsum(rays[:, 2]) - rays[:, 2])         # empty rows take their place in the prefix sum
        for a, r in zip(got[:3], ref[:3]):
            assert r.shape[0] == M and np.array_equal(a[:M], r)
            assert not a[M:].any()                                                     # nothing is written past the budget
        if M < total:                                                                  # later rays are dropped whole, not truncated
            fits = rays[:, 1] + rays[:, 2] <= M
            last = int((rays[fits, 1] + rays[fits, 2]).max())
            assert 0 < last <= M and not got[0][last:].any() and got[2][:last, 0].all()
    # cross-form: the live rays alone are a wave-form batch; same samples through each form's own (offset, count) rows
    lo, ld, ln, lf, lz = c["live"]
    full = _march_abi(ck, po, pd, pn, pf, pz, N_LANE, bound, dt_gamma, max_steps, total, total)
    wave = _march_abi(ck, lo, ld, ln, lf, lz, len(lo), bound, dt_gamma, max_steps, total, total)
    assert len(lo) <= N_WAVE and np.array_equal(wave[3][:, 2], full[3][pos, 2]) and wave[4][0] == full[4][0]
    iw, il = _gather(wave[3]), _gather(full[3][pos])
    assert len(iw) == len(il) == total
    for a, b in zip(wave[:3], full[:3]):
        assert np.array_equal(a[iw], b[il])


def test_march_rays_train_same_counts_on_both_sides_of_the_form_threshold():
    """N = 131072 (wave form) and N = 131073 (lane form) on the same arrays: identical counts for the shared rows."""
    c = _march_case(1.0, 0.0, 256, N_WAVE + 1)
    po, pd, pn, pf, pz = c["padded"]
    wave = _march_abi(c["ck"], po, pd, pn, pf, pz, N_WAVE, 1.0, 0.0, 256, c["total"], c["total"])
    lane = _march_abi(c["ck"], po, pd, pn, pf, pz, N_WAVE + 1, 1.0, 0.0, 256, c["total"], c["total"])
    assert np.array_equal(wave[3][:N_WAVE, 2], lane[3][:N_WAVE, 2]) and wave[3][:N_WAVE, 2].sum() > 10000
    assert (wave[3][N_WAVE] == -7).all() and lane[4][1] == N_WAVE + 1 and wave[4][1] == N_WAVE
