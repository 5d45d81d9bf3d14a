"""Shared inputs and yardsticks of the training ray ops' two-form tests (CPU: test_train_forms_host.py; GPU: test_gpu_train_forms.py).  The entry
points of pienerf_amd/csrc/pn_train_ops.hip take the wave-per-ray kernels up to WAVE_FORM_MAX_N ray rows and the lane-per-ray kernels above it.

  composite_cases  a designed batch: rays of 1 .. 513 samples whose transmittance crosses T_thresh at a chosen sample ("wall") or never, so that
                   every window of the wave-per-ray composite, its carry and both edges of a 64-sample window are exercised by many rays
  composite_ref64  the same operation in float64 with torch on the CPU, gradients from torch.autograd (not from the kernels' backward formula)
  pad_rows         the designed rows embedded into N_total rows of empty rays (front, middle across a multiple of 128, back)
  composite_errors the per-ray / per-sample error units both test files use

Data and torch / numpy only — no product code."""
import numpy as np
import torch

WAVE_FORM_MAX_N = 131072          # pn_train_ops.hip: N <= this takes the wave-per-ray kernels
T_THRESHES = (1e-4, 5e-2)
COPIES = 8
SEED = 20

# (length, wall index or None)
CASE_ROWS = ((1, None), (1, 0), (63, None), (64, None), (64, 63), (65, None), (65, 63), (65, 64), (127, None), (128, 127), (129, 128), (129, 64),
             (200, 130), (200, None), (320, None), (320, 255), (320, 256), (513, None), (513, 300), (513, 512))

# max error of the project's fp32 CPU oracle (oracle.training.composite_rays_train_forward / backward, a sequential restatement with libm's expf)
# against composite_ref64 on composite_cases(T_thresh, default_rng(SEED)), in the units of composite_errors.  Measured; test_train_forms_host.py
# asserts the oracle stays within them, test_gpu_train_forms.py allows the kernels GPU_FACTOR times as much.
ORACLE_VS_F64 = {
    1e-4: dict(weights_sum=9.68e-7, depth=9.02e-7, image=1.16e-6, grad_rgbs=1.80e-7, grad_sigmas=5.04e-7),
    5e-2: dict(weights_sum=1.21e-6, depth=1.10e-6, image=2.10e-6, grad_rgbs=6.45e-7, grad_sigmas=5.64e-7),
}
# __expf and expf may each be ~2 ulp off near 1, which enters alpha = 1 - exp(-x) as an absolute error, and the wave form sums by a scan tree
# where the oracle sums sample after sample
GPU_FACTOR = 4.0
# the bars the suite already holds the composite to against the fp32 oracle (test_gpu_training.py), here per ray instead of per batch
ORACLE_BARS = dict(weights_sum=1e-5, depth=1e-5, image=1e-5, grad_rgbs=1e-5, grad_sigmas=1e-4)
FLOOR = 1e-3                      # floor of the per-ray relative unit of weights_sum / depth / image


def composite_cases(T_thresh, rng):
    """-> dict(rays [N,3] int32 (index, offset, num_steps), sigmas [M], rgbs [M,3], deltas [M,2], walls [N] (wall sample or -1), grad_weights_sum [N],
    grad_image [N,3]); COPIES rays per row of CASE_ROWS, shuffled.  Optical depths x_i = sigma_i * delta_i[0]: the background of a ray sums to
    0.25 * (-ln T_thresh), so T stays e^(0.75 * -ln T_thresh) above the threshold without a wall; a wall sample has x = 3 * (-ln T_thresh) and puts T
    a factor T_thresh^2 below it.  The exit sample is therefore the same in fp32 and fp64 for every ray."""
    depth = -np.log(T_thresh)
    rows = [CASE_ROWS[i] for i in rng.permutation(np.repeat(np.arange(len(CASE_ROWS)), COPIES))]
    N = len(rows)
    lens = np.array([L for L, _ in rows], np.int64)
    walls = np.array([-1 if k is None else k for _, k in rows], np.int64)
    offs = np.cumsum(lens) - lens
    M = int(lens.sum())
    d0 = rng.uniform(0.004, 0.012, M)
    deltas = np.stack([d0, d0 * rng.uniform(1.0, 1.5, M)], 1).astype(np.float32)
    x = rng.uniform(0.1, 1.0, M)
    for n in range(N):
        seg = slice(offs[n], offs[n] + lens[n])
        bg = np.ones(lens[n], bool)
        if walls[n] >= 0:
            bg[walls[n]] = False
        xs = x[seg]
        if bg.any():
            xs[bg] *= 0.25 * depth / xs[bg].sum()
        xs[~bg] = 3.0 * depth
    sigmas = (x / deltas[:, 0].astype(np.float64)).astype(np.float32)
    rgbs = rng.uniform(0, 1, (M, 3)).astype(np.float32)
    rays = np.stack([rng.permutation(N), offs, lens], 1).astype(np.int32)
    gws, gim = rng.standard_normal(N).astype(np.float32), rng.standard_normal((N, 3)).astype(np.float32)
    return dict(rays=rays, sigmas=sigmas, rgbs=rgbs, deltas=deltas, walls=walls, grad_weights_sum=gws, grad_image=gim)


def composite_ref64(sigmas, rgbs, deltas, rays, T_thresh, grad_weights_sum, grad_image):
    """composite_rays_train forward + backward in float64.  Per ray: alpha = 1 - exp(-sigma * delta0), T by cumprod, the sample at which T drops below
    T_thresh is the last one accumulated (the mask is a constant of the graph).  Gradients of sum(weights_sum * grad_weights_sum) +
    sum(image * grad_image) by torch.autograd; depth gets none, like the op.  Rows with num_steps == 0 or offset + num_steps > M give zeros.
    -> dict(weights_sum, depth, image [by ray index]; grad_sigmas [M], grad_rgbs [M,3] (0 where the op writes nothing); written [M] bool (samples the
    backward writes); exit [N] (exit sample or -1, by row); margin [N] (min |ln(T / T_thresh)| over the row's samples, inf for dead rows))."""
    N, M = len(rays), len(sigmas)
    s = torch.tensor(np.asarray(sigmas, np.float64), requires_grad=True)
    c = torch.tensor(np.asarray(rgbs, np.float64).reshape(-1, 3), requires_grad=True)
    dl = torch.tensor(np.asarray(deltas, np.float64).reshape(-1, 2))
    gws, gim = torch.tensor(np.asarray(grad_weights_sum, np.float64)), torch.tensor(np.asarray(grad_image, np.float64).reshape(-1, 3))
    ws, depth, image = np.zeros(N), np.zeros(N), np.zeros((N, 3))
    written = np.zeros(M, bool)
    exits, margin = np.full(N, -1, np.int64), np.full(N, np.inf)
    loss = torch.zeros((), dtype=torch.float64)
    for row, (index, off, L) in enumerate(np.asarray(rays, np.int64)):
        if L == 0 or off + L > M:
            continue
        alpha = 1.0 - torch.exp(-s[off:off + L] * dl[off:off + L, 0])
        T_after = torch.cumprod(1.0 - alpha, 0)
        logs = np.log(np.maximum(T_after.detach().numpy(), 1e-300) / T_thresh)
        margin[row] = np.abs(logs).min()
        below = np.nonzero(logs < 0)[0]
        n_use = L if len(below) == 0 else int(below[0]) + 1
        exits[row] = -1 if len(below) == 0 else int(below[0])
        T_before = torch.cat([torch.ones(1, dtype=torch.float64), T_after[:n_use - 1]])
        w = alpha[:n_use] * T_before
        t = torch.cumsum(dl[off:off + n_use, 1], 0)
        ws_n, im_n = w.sum(), (w[:, None] * c[off:off + n_use]).sum(0)
        ws[index], depth[index], image[index] = ws_n.item(), (w * t).sum().item(), im_n.detach().numpy()
        written[off:off + n_use] = True
        loss = loss + ws_n * gws[index] + (im_n * gim[index]).sum()
    if loss.requires_grad:
        loss.backward()
    gs = np.zeros(M) if s.grad is None else s.grad.numpy()
    gc = np.zeros((M, 3)) if c.grad is None else c.grad.numpy()
    return dict(weights_sum=ws, depth=depth, image=image, grad_sigmas=gs, grad_rgbs=gc, written=written, exit=exits, margin=margin)


def sample_rows(rays, M):
    """[M] row of `rays` that owns each sample (-1: none; rows past the point budget own nothing)."""
    owner = np.full(M, -1, np.int64)
    for n, (_, off, L) in enumerate(np.asarray(rays, np.int64)):
        if L > 0 and off + L <= M:
            owner[off:off + L] = n
    return owner


def composite_errors(got, ref, rays, deltas, grad_weights_sum, grad_image, written, per_ray_max=False):
    """Error of `got` against `ref` (dicts with weights_sum, depth, image, grad_sigmas, grad_rgbs) in per-ray / per-sample units, one array per output:
      weights_sum, depth, image[c]   |err| / max(|ref|, FLOOR)                                                         per ray
      grad_rgbs[i, c]                |err| / |grad_image[ray, c]|                                                      (the weight's absolute error)
      grad_sigmas[i]                 |err| / (delta_i0 * (sum_c |grad_image[ray, c]| + |grad_weights_sum[ray]|))       (the terms before they cancel)
    per_ray_max: the gradients' denominator becomes max(unit, the ray's own largest |ref|) — the error relative to the ray's own maximum, floored at the
    unit, that the bars against the fp32 oracle use (for the three per-ray outputs that is the first line already).  All per-ray arrays are indexed by
    ray index.  Only the samples of `written` (composite_ref64) are compared: the op leaves the others alone and the caller checks them for its sentinel."""
    rays = np.asarray(rays, np.int64)
    M = len(ref["grad_sigmas"])
    owner = sample_rows(rays, M)
    live = np.asarray(written, bool)
    assert (owner[live] >= 0).all()
    idx = rays[owner[live], 0]
    f64 = lambda a: np.asarray(a, np.float64)
    gws, gim, d0 = f64(grad_weights_sum), f64(grad_image).reshape(-1, 3), f64(deltas).reshape(-1, 2)[:, 0]
    out = {}
    for k in ("weights_sum", "depth", "image"):
        out[k] = np.abs(f64(got[k]) - f64(ref[k])) / np.maximum(np.abs(f64(ref[k])), FLOOR)
    unit_c = np.abs(gim[idx])
    unit_s = d0[live] * (np.abs(gim[idx]).sum(1) + np.abs(gws[idx]))
    ref_c, ref_s = f64(ref["grad_rgbs"]).reshape(-1, 3)[live], f64(ref["grad_sigmas"])[live]
    if per_ray_max:
        top_c, top_s = np.zeros((len(rays), 3)), np.zeros(len(rays))
        np.maximum.at(top_c, owner[live], np.abs(ref_c))
        np.maximum.at(top_s, owner[live], np.abs(ref_s))
        unit_c, unit_s = np.maximum(unit_c, top_c[owner[live]]), np.maximum(unit_s, top_s[owner[live]])
    out["grad_rgbs"] = np.abs(f64(got["grad_rgbs"]).reshape(-1, 3)[live] - ref_c) / unit_c
    out["grad_sigmas"] = np.abs(f64(got["grad_sigmas"])[live] - ref_s) / unit_s
    return out


def pad_positions(n_designed, N_total):
    """Rows of the N_total-row batch that hold the designed rows, in their order: a third at the front, a third across a multiple of 128 in the middle,
    the rest at the very back (so the last live row is the batch's last row)."""
    if N_total == n_designed:
        return np.arange(n_designed)
    a = n_designed // 3
    b = n_designed - 2 * a
    mid = (N_total // 2) // 128 * 128 - a // 2
    assert a <= mid and mid + a <= N_total - b
    return np.concatenate([np.arange(a), mid + np.arange(a), N_total - b + np.arange(b)])


def pad_rows(rays, N_total, rng):
    """Composite rows embedded into N_total rows: -> (rays_padded [N_total,3], pos [N] rows of the designed rays).  Added rows have num_steps = 0 and
    the offset a prefix sum gives them; `index` becomes a random permutation of N_total in which the designed rays keep distinct slots.  M is unchanged."""
    rays = np.asarray(rays, np.int32)
    N = len(rays)
    pos = pad_positions(N, N_total)
    out = np.zeros((N_total, 3), np.int32)
    out[pos, 2] = rays[:, 2]
    # the designed rows stay in offset order, so the prefix sum of the padded counts reproduces their offsets
    assert np.array_equal(np.cumsum(rays[:, 2]) - rays[:, 2], rays[:, 1])
    out[:, 1] = np.cumsum(out[:, 2]) - out[:, 2]
    out[:, 0] = rng.permutation(N_total)
    return out, pos


def pad_march_rays(o, d, nears, fars, noise, N_total):
    """March inputs embedded into N_total rays: the added rays are copies of the first live ray with far = near, so t0 >= far and their count is 0.
    -> (o, d, nears, fars, noise, pos)."""
    N = len(o)
    pos = pad_positions(N, N_total)
    po, pd = np.repeat(o[:1], N_total, 0), np.repeat(d[:1], N_total, 0)
    pn = np.full(N_total, nears[0], np.float32)
    pf = pn.copy()
    pz = np.zeros(N_total, np.float32)
    po[pos], pd[pos], pn[pos], pf[pos], pz[pos] = o, d, nears, fars, noise
    return po, pd, pn, pf, pz, pos
