"""One training step of the cuda_ray renderer, restated in float64 (CPU: test_train_step_host.py; GPU: test_gpu_train_step.py).

NeRFRenderer.run_cuda_ops in train() mode chains march_rays_train -> forward_ops (hash grid, two bias-free MLPs, SH) -> density_scale ->
composite_rays_train -> image + (1 - weights_sum) * bg, and the trainer takes a per-ray MSE of it.  `train_step` below is that chain on GIVEN samples
(the march is integer / bit-exact work with a test of its own), with every gradient from torch.autograd:

  grid_cells      the hash grid's cell, fraction and table rows of every (sample, level) — the part of the operation that is DEFINED in fp32:
                  u = (x + bound) / (2 bound), pos = fmaf(u, scale, 0.5), floor, frac, all in fp32 exactly as the kernels take them.  Taking the
                  position in float64 instead would move the finest levels' weights by ~1e-4 and be mistaken for a kernel error.
  train_step      everything behind that in `dtype` (float64): corner weights, the gather embeddings[idx] * w summed over corners, relu(f W0^T) W1^T,
                  sigma = density_scale * exp(h0), [SH16(dirs) | h[1:]] through W2, W3, W4 and a sigmoid, the composite of tfc.composite_ref64 (a sample
                  is accumulated while T before it is >= T_thresh; the mask is a constant of the graph), the background blend and
                  loss = sum_n w_n mean_c (image_n - target_n)^2 / sum_n w_n.
  CASES / case_inputs   the ray sets both test files run, built from the oracle's march
  FP32_VS_F64     per case and parameter tensor: max|g32 - g64| / max|g64| of the same graph run in fp32 with the float64 run's mask — what fp32
                  arithmetic alone costs.  Measured; test_train_step_host.py asserts the fp32 run stays within them, test_gpu_train_step.py allows
                  the device GPU_FACTOR_STEP times as much (capped at GRAD_BAR_CAP).

torch / numpy and the project's CPU oracle (level parameters, SH values, the march) only — no product kernels."""
import numpy as np
import torch

import oracle
from oracle import training as otr

PARAMS = ("embeddings", "W0", "W1", "W2", "W3", "W4")
BG_PARAMS = ("bg_embeddings", "bg_W0", "bg_W1")
MARGIN = 1e-3          # rays whose min |ln(T / T_thresh)| is below this may end one sample apart on the device: loss weight 0 on both sides
MARGIN_SHARE = 0.02    # ... and no case may have more than this share of them (a condition on the poses, asserted on the CPU)

# max|g32 - g64| / max|g64| per case and tensor of the fp32 run with the float64 mask, measured with `PYTHONPATH=. python tests/train_step_reference.py` (torch
# on the CPU).  The figure is the top of rounding noise and moves with the BLAS summation order, so it is the largest of runs with 1, 4 and 8 threads,
# rounded up to two digits; `reference` pins its fp32 run to one thread so that the host test's own figure does not move.
FP32_VS_F64 = {
    "chair": dict(embeddings=1.5e-07, W0=3.3e-07, W1=2.4e-07, W2=2.3e-07, W3=2.7e-07, W4=2.9e-07),
    "tensor_bg": dict(embeddings=2.7e-07, W0=4.3e-07, W1=2.8e-07, W2=2.3e-07, W3=2.4e-07, W4=2.4e-07),
    "scaled": dict(embeddings=3.2e-07, W0=2.0e-07, W1=2.3e-07, W2=1.8e-07, W3=2.8e-07, W4=2.2e-07),
    "trex": dict(embeddings=4.4e-07, W0=2.8e-07, W1=4.1e-07, W2=3.1e-07, W3=2.6e-07, W4=2.3e-07),
    "budget": dict(embeddings=1.8e-07, W0=1.5e-07, W1=2.9e-07, W2=1.9e-07, W3=3.1e-07, W4=2.1e-07),
    "bg_model": dict(embeddings=6.9e-07, W0=6.3e-07, W1=2.8e-07, W2=3.3e-07, W3=2.6e-07, W4=2.0e-07, bg_embeddings=1.3e-07, bg_W0=2.5e-07, bg_W1=2.3e-07),
}
# The device step against float64 is allowed GPU_FACTOR_STEP times the fp32 floor of that tensor, at most GRAD_BAR_CAP (the 1e-4 the per-op tests
# already hold these gradients to).  32 rather than train_forms_cases.GPU_FACTOR's 4: the step stacks five rocBLAS GEMMs (each with its own summation
# order and, in the backward, two more per layer), __expf in the composite's forward and backward, and fp32 atomics that sum up to ~10^5 contributions
# into one table row in an order that changes from run to run.
GPU_FACTOR_STEP = 32.0
GRAD_BAR_CAP = 1e-4
# The device's own figures on an MI355X, max|g - g64| / max|g64| per tensor (test_gpu_train_step.py prints them; for the record, nothing asserts them).
# The largest is 17.9 floors (W0 in `scaled`), the table's gradient 2 .. 16 floors, the last colour layer about one: the allowance of 32 leaves a
# factor of two over the worst tensor, and the atomics' order moves the table's figure in the third digit from run to run.
DEVICE_VS_F64 = {
    "chair": dict(embeddings=1.8e-06, W0=5.2e-06, W1=2.1e-06, W2=1.7e-06, W3=1.4e-06, W4=2.8e-07),
    "tensor_bg": dict(embeddings=2.6e-06, W0=2.6e-06, W1=4.2e-07, W2=1.6e-06, W3=1.4e-06, W4=2.7e-07),
    "scaled": dict(embeddings=3.2e-06, W0=3.6e-06, W1=1.2e-06, W2=1.4e-06, W3=1.4e-06, W4=2.0e-07),
    "trex": dict(embeddings=8.6e-07, W0=1.8e-06, W1=1.0e-06, W2=7.1e-07, W3=1.0e-06, W4=1.5e-07),
    "budget": dict(embeddings=2.0e-06, W0=8.6e-07, W1=2.8e-07, W2=8.9e-07, W3=8.8e-07, W4=2.7e-07),
    "bg_model": dict(embeddings=1.1e-05, W0=5.9e-06, W1=6.0e-07, W2=1.3e-06, W3=1.2e-06, W4=2.3e-07, bg_embeddings=1.6e-07, bg_W0=4.3e-07, bg_W1=1.6e-07),
}
# fp16 (autocast): the sigma logit is a half value in [4, 8), one half ulp of it (2^-9) moves sigma by 0.2 % and a ray's ln T = -sum(sigma delta) by
# up to 0.4 % of |ln T_thresh| = 4.6, that is 2e-2: the rays within that of the threshold get loss weight 0 in the fp16 case.
MARGIN_HALF = 2e-2
HALF_BAR = 1e-2        # the suite's bar for the half scatter-add (test_gpu_half.py, test_gpu_training.py): 1e-2 of the tensor's largest entry


# ------------------------------------------------------------------------------------------------------------------ fp32 part: cells and fractions
def _fmaf(a, b, c):
    """fmaf(a, b, c) for float32 arrays: the product of two float32 is exact in float64; the sum is rounded once to float64 and once more to
    float32, and the (rare) case where the first rounding lands exactly on a float32 tie is put right with the sum's exact error (TwoSum)."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.float64(c)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    r = s.astype(np.float32)
    d = s - r.astype(np.float64)
    tie = (err != 0) & (np.abs(d) == 0.5 * np.spacing(np.abs(r)).astype(np.float64)) & (d != 0)
    if tie.any():
        away = tie & (np.sign(err) == np.sign(d))   # the exact sum lies beyond the tie, on the other neighbour's side
        r = np.where(away, np.nextafter(r, np.where(d > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)), r)
    return r


_PRIMES = (1, 2654435761, 805459861)


def grid_cells(x, bound, offsets, per_level_scale, base_resolution):
    """x [B, D] float32 (D = 2 or 3) in [-bound, bound] -> (idx [B, L, 2^D] int64 rows of the table, frac [B, L, D] float32, inside [B] bool).
    Index rule of gridencoder.cu:50-84 (oracle/render_oracle.cpp grid_index): stride while stride <= hashmap_size, else the prime hash, modulo
    the level's size.  Samples outside [0, 1] encode to zero (`inside` False)."""
    f = np.float32
    x = np.asarray(x, f)
    B, D = x.shape
    offsets = np.asarray(offsets, np.int64)
    L = len(offsets) - 1
    scales, ress = oracle.grid_level_params(L, per_level_scale, base_resolution)
    u = (x + f(bound)) / f(2 * bound)   # gridencoder/grid.py:152, a float32 tensor expression
    inside = ((u >= 0) & (u <= 1)).all(1)
    idx = np.zeros((B, L, 1 << D), np.int64)
    frac = np.zeros((B, L, D), f)
    for l in range(L):
        hs, res = int(offsets[l + 1] - offsets[l]), int(ress[l])
        pos = _fmaf(u, np.full_like(u, scales[l]), 0.5)
        pg = np.floor(pos)
        frac[:, l] = pos - pg
        pg = pg.astype(np.int64)
        for k in range(1 << D):
            pl = [pg[:, d] + ((k >> d) & 1) for d in range(D)]
            stride, index = 1, np.zeros(B, np.int64)
            for d in range(D):
                if stride > hs:
                    break
                index = (index + pl[d] * stride) & 0xFFFFFFFF
                stride *= res + 1
            if stride > hs:
                index = np.zeros(B, np.int64)
                for d in range(D):
                    index ^= (pl[d] * _PRIMES[d]) & 0xFFFFFFFF
            idx[:, l, k] = offsets[l] + index % hs
    idx[~inside] = 0
    return idx, frac, inside


def _encode(table, cells, dtype):
    """[B, L*C] features: sum over corners of table[idx] * w, w the product over axes of frac or 1 - frac (in `dtype`, from the fp32 fraction)."""
    idx, frac, inside = cells
    B, L, K = idx.shape
    D = frac.shape[2]
    fr = torch.as_tensor(frac).to(dtype)
    out = 0
    for k in range(K):
        w = torch.ones(B, L, dtype=dtype)
        for d in range(D):
            w = w * (fr[:, :, d] if (k >> d) & 1 else 1 - fr[:, :, d])
        out = out + table[torch.as_tensor(idx[:, :, k])] * w[:, :, None]
    out = out * torch.as_tensor(inside).to(dtype)[:, None, None]
    return out.reshape(B, -1)


class _Table:
    """The rows of an embedding table that a batch touches, as a leaf of the graph; `dense_grad` scatters their gradient into the full shape."""

    def __init__(self, emb, cells, dtype):
        self.shape = emb.shape
        idx, frac, inside = cells
        self.rows, inv = np.unique(idx, return_inverse=True)
        self.leaf = torch.tensor(np.asarray(emb)[self.rows], dtype=dtype, requires_grad=True)
        self.cells = (inv.reshape(idx.shape), frac, inside)
        self.dtype = dtype

    def encode(self):
        return _encode(self.leaf, self.cells, self.dtype)

    def dense_grad(self):
        g = np.zeros(self.shape, np.float64)
        if self.leaf.grad is not None:
            g[self.rows] = self.leaf.grad.numpy().astype(np.float64)
        return g


# ------------------------------------------------------------------------------------------------------------------ the step
def train_step(xyzs, dirs, deltas, rays, ck, bound, density_scale, T_thresh, bg, target, weights, rays_d=None, dtype=torch.float64, n_use=None,
               margin_min=MARGIN):
    """One step on the samples `xyzs, dirs, deltas, rays` of march_rays_train, checkpoint dict `ck` (scene.make_checkpoint).
    bg: a scalar, an [N,3] array, or dict(coords=[N,2] sphere coordinates) — then the checkpoint's background model shades them with `rays_d` [N,3].
    target [N,3], weights [N] (per-ray loss weights; None: loss_weights of this run's own margins at margin_min), both by ray index.  n_use: per-ROW accumulated sample counts of an earlier (float64) run, which
    replace this run's own exit decision (the mask is a constant of the graph).
    -> dict(sigma [M], rgb [M,3], weights_sum [N], image [N,3] (blended), loss, margin [N] by ray index (min |ln(T / T_thresh)|, inf for rows without
    samples), n_use [rows], grads {name: float64 array of the parameter's shape})."""
    f64 = np.float64
    tt = lambda a: torch.as_tensor(np.asarray(a, f64)).to(dtype)
    xyzs, dirs = np.asarray(xyzs, np.float32).reshape(-1, 3), np.asarray(dirs, np.float32).reshape(-1, 3)
    rays = np.asarray(rays, np.int64).reshape(-1, 3)
    M, N = xyzs.shape[0], rays.shape[0]
    W = {k: torch.tensor(np.asarray(ck[k], f64), dtype=dtype, requires_grad=True) for k in PARAMS[1:]}
    table = _Table(ck["embeddings"], grid_cells(xyzs, bound, ck["offsets"], ck["per_level_scale"], ck["base_resolution"]), dtype)
    h = torch.relu(table.encode() @ W["W0"].T) @ W["W1"].T
    sigma = density_scale * torch.exp(h[:, 0])
    sh = tt(oracle.sh_encode_forward(dirs, 4))   # no gradient: the directions are data
    c = torch.relu(torch.cat([sh, h[:, 1:]], 1) @ W["W2"].T)
    rgb = torch.sigmoid(torch.relu(c @ W["W3"].T) @ W["W4"].T)

    dl = tt(np.asarray(deltas).reshape(-1, 2))
    ws, image = [torch.zeros((), dtype=dtype)] * N, [torch.zeros(3, dtype=dtype)] * N
    margin, used = np.full(N, np.inf), np.zeros(N, np.int64)
    for row, (index, off, Ln) in enumerate(rays):
        if Ln == 0 or off + Ln > M:   # rows past the point budget composite to the background
            continue
        alpha = 1.0 - torch.exp(-sigma[off:off + Ln] * dl[off:off + Ln, 0])
        T_after = torch.cumprod(1.0 - alpha, 0)
        logs = np.log(np.maximum(T_after.detach().numpy().astype(f64), 1e-300) / T_thresh)
        margin[index] = np.abs(logs).min()
        if n_use is None:
            below = np.nonzero(logs < 0)[0]
            k = Ln if len(below) == 0 else int(below[0]) + 1
        else:
            k = int(n_use[row])
        used[row] = k
        w = alpha[:k] * torch.cat([torch.ones(1, dtype=dtype), T_after[:k - 1]])
        ws[index], image[index] = w.sum(), (w[:, None] * rgb[off:off + k]).sum(0)
    ws, image = torch.stack(ws), torch.stack(image)

    bg_leaves = {}
    if isinstance(bg, dict):
        bt = _Table(ck["bg_embeddings"], grid_cells(np.asarray(bg["coords"], np.float32).reshape(-1, 2), 1.0, ck["bg_offsets"], ck["bg_per_level_scale"],
                                                    ck["base_resolution"]), dtype)
        bg_leaves = {k: torch.tensor(np.asarray(ck[k], f64), dtype=dtype, requires_grad=True) for k in BG_PARAMS[1:]}
        hb = torch.cat([tt(oracle.sh_encode_forward(np.asarray(rays_d, np.float32).reshape(-1, 3), 4)), bt.encode()], 1)
        bg_rgb = torch.sigmoid(torch.relu(hb @ bg_leaves["bg_W0"].T) @ bg_leaves["bg_W1"].T)
    else:
        bt = None
        bg_rgb = tt(bg) if np.ndim(bg) else float(bg)
    blended = image + (1 - ws)[:, None] * bg_rgb
    if weights is None:
        weights = loss_weights(margin, margin_min)
    wn = tt(weights)
    loss = (wn * ((blended - tt(target)) ** 2).mean(1)).sum() / wn.sum()
    loss.backward()

    grads = {"embeddings": table.dense_grad()}
    for k, v in {**W, **bg_leaves}.items():
        grads[k] = np.zeros(v.shape) if v.grad is None else v.grad.numpy().astype(f64)
    if bt is not None:
        grads["bg_embeddings"] = bt.dense_grad()
    n64 = lambda t: t.detach().numpy().astype(f64)
    return dict(sigma=n64(sigma), rgb=n64(rgb), weights_sum=n64(ws), image=n64(blended), loss=float(loss.detach()), margin=margin, n_use=used, grads=grads,
                weights=np.asarray(weights, f64))


def loss_weights(margin, margin_min=MARGIN):
    """Per-ray loss weights shared by both sides: 0 for the rays within margin_min of the threshold, 1 elsewhere."""
    return (np.asarray(margin) >= margin_min).astype(np.float64)


def grad_errors(got, ref):
    """{name: max|got - ref| / max|ref|} over the tensors of `ref`."""
    return {k: float(np.abs(np.asarray(got[k], np.float64) - ref[k]).max() / np.abs(ref[k]).max()) for k in ref}


# ------------------------------------------------------------------------------------------------------------------ the cases
# name -> checkpoint (bound, seed, bg_radius), rays (W, pose = orbit_pose arguments), march (dt_gamma, max_steps), T_thresh, density_scale,
# background kind, budget (share of the needed samples that mean_count allows; None: every ray marches)
CASES = {
    "chair":     dict(bound=1.0, seed=0, W=24, pose=(4.0, 40.0, -20.0), dt_gamma=0.0, max_steps=1024, T_thresh=1e-2, density_scale=1.0, bg="white"),
    "tensor_bg": dict(bound=1.0, seed=0, W=24, pose=(4.0, 40.0, -20.0), dt_gamma=0.0, max_steps=1024, T_thresh=1e-2, density_scale=1.0, bg="tensor"),
    "scaled":    dict(bound=1.0, seed=0, W=24, pose=(4.0, 40.0, -20.0), dt_gamma=0.0, max_steps=1024, T_thresh=1e-2, density_scale=2.0, bg="white"),
    "trex":      dict(bound=2.0, seed=3, W=40, pose=(4.5, 25.0, -10.0), dt_gamma=1.0 / 128, max_steps=300, T_thresh=5e-2, density_scale=1.0, bg="white"),
    "budget":    dict(bound=1.0, seed=0, W=24, pose=(4.0, 40.0, -20.0), dt_gamma=0.0, max_steps=1024, T_thresh=1e-2, density_scale=1.0, bg="white",
                      budget=0.6),
    "bg_model":  dict(bound=1.0, seed=0, W=24, pose=(4.0, 40.0, -20.0), dt_gamma=0.0, max_steps=1024, T_thresh=1e-2, density_scale=1.0, bg="model",
                      bg_radius=3.0),
}
_cache = {}


def case_inputs(name):
    """The shared inputs of a case (cached, treat as read-only): dict(ck, o, d, nears, fars, xyzs, dirs, deltas, rays, mean_count, target [N,3],
    bg (scalar 1 / [N,3] / None for the model), plus the CASES entry)."""
    if name in _cache:
        return _cache[name]
    from pienerf_amd import scene   # data only: the synthetic checkpoint and the camera
    c = dict(CASES[name])
    ck = scene.make_checkpoint(bound=c["bound"], seed=c["seed"], shaped=True, **({"bg_radius": c["bg_radius"]} if "bg_radius" in c else {}))
    Wd, b = c["W"], c["bound"]
    o, d = oracle.get_rays(scene.orbit_pose(*c["pose"]), scene.orbit_intrinsics(Wd, Wd, 50.0), Wd, Wd)
    nears, fars = oracle.near_far_from_aabb(o, d, np.array([-b, -b, -b, b, b, b], np.float32), 0.2)
    march = lambda mean_count: otr.march_rays_train(o, d, b, ck["density_bitfield"], ck["cascade"], ck["grid_size"], nears, fars, None, mean_count, None,
                                                    128, False, c["dt_gamma"], c["max_steps"])
    mean_count = -1
    if c.get("budget"):
        mean_count = int(c["budget"] * int(march(-1)[3][:, 2].sum()))
    xyzs, dirs, deltas, rays = march(mean_count)
    rng = np.random.default_rng(len(name) + 7)
    N = len(o)
    target = rng.uniform(0, 1, (N, 3)).astype(np.float32)
    bg = {"white": 1.0, "tensor": rng.uniform(0, 1, (N, 3)).astype(np.float32), "model": None}[c["bg"]]
    c.update(ck=ck, o=o, d=d, nears=nears, fars=fars, xyzs=xyzs, dirs=dirs, deltas=deltas, rays=rays, mean_count=mean_count, target=target, bg=bg)
    _cache[name] = c
    return c


def host_sph_coords(o, d, radius):
    """The sphere coordinates from the CPU oracle (the GPU test reads them back from the device op instead, see test_gpu_train_step.py)."""
    return oracle.sph_from_ray(o, d, radius)


def reference(name, coords=None, dtype=torch.float64, first=None, margin_min=MARGIN):
    """train_step of a case; the float64 run's margins give the loss weights.  dtype=float32 needs `first`, that float64 result, and takes its mask
    and weights."""
    c = case_inputs(name)
    bg = c["bg"]
    if bg is None:
        bg = dict(coords=host_sph_coords(c["o"], c["d"], c["bg_radius"]) if coords is None else coords)
    run = lambda w, dt, n_use: train_step(c["xyzs"], c["dirs"], c["deltas"], c["rays"], c["ck"], c["bound"], c["density_scale"], c["T_thresh"], bg,
                                          c["target"], w, rays_d=c["d"], dtype=dt, n_use=n_use, margin_min=margin_min)
    if first is not None:
        threads = torch.get_num_threads()
        torch.set_num_threads(1)   # one summation order, see FP32_VS_F64
        try:
            return run(first["weights"], dtype, first["n_use"])
        finally:
            torch.set_num_threads(threads)
    return run(None, torch.float64, None)


if __name__ == "__main__":   # re-measure FP32_VS_F64 (one run; set OMP_NUM_THREADS to 1, 4, 8 and take the largest)
    import sys
    for name in (sys.argv[1:] or CASES):
        r64 = reference(name)
        r32 = reference(name, dtype=torch.float32, first=r64)
        m = r64["margin"]
        print(name, "samples", len(case_inputs(name)["xyzs"]), "margin<1e-3:", int((m < MARGIN).sum()), "of", len(m),
              {k: float(f"{v:.2e}") for k, v in grad_errors(r32["grads"], r64["grads"]).items()})
