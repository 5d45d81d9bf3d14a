"""SSIM on the device (pienerf_amd/metrics.py over csrc/pn_ssim.hip) against the torch restatement of tests/ssim_reference.py, and its use in
Trainer.evaluate_loader and Trainer.train_step.

Tolerances come from the restatement itself: the forward bar is 8 x |fp32 restatement - fp64 restatement| of the scalar on the same input (at least
5e-7, a few ulp of a mean near 1), the backward bar 8 x the fp32 restatement's max |grad - grad64| / max |grad64| (at least 1e-5).  The kernel sums
the same 121 products in another order (separably), so its error is an independent draw of the size of the fp32 restatement's.  Every case prints
its error as a fraction of its bar (``-s`` shows them; DESIGN.md 4.9 records one run)."""
import functools

import numpy as np
import pytest
import torch

import ssim_reference as ref
from pienerf_amd import metrics, scene
from pienerf_amd.nerf.network import NeRFNetwork
from pienerf_amd.nerf.utils import get_rays
from pienerf_amd.training import Trainer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [(1, 11, 11, 3),     # one output position: nothing but halo
          (2, 12, 27, 3),     # two images, ragged in both directions
          (1, 37, 70, 1),     # one channel
          (1, 80, 107, 3),    # valid region 70 x 97: several 16 x 16 tiles with a ragged last one
          (3, 16, 16, 3)]     # the patch shape of the loss
KINDS = {"noise": ref.noise_pair, "smooth": ref.smooth_pair}
CASES = [pytest.param(s, k, id=f"{'x'.join(map(str, s))}-{k}") for s in SHAPES for k in KINDS]


@functools.lru_cache(maxsize=None)
def _pair(shape, kind):
    """(pred, truth) on the host, seeded by the shape; shared by the tests and never written to."""
    return KINDS[kind](shape, seed=sum(shape))


@functools.lru_cache(maxsize=None)
def _forward_ref(shape, kind, data_range):
    return ref.forward_bar(*_pair(shape, kind), data_range)


@functools.lru_cache(maxsize=None)
def _grad_ref(shape, kind):
    return ref.grad_bar(*_pair(shape, kind), 1.0)


def _dev(shape, kind):
    p, t = _pair(shape, kind)
    return p.to(DEV), t.to(DEV)


def _check_forward(per, scalar, want_per, want, tol, what):
    err = max(float((per.double().cpu() - want_per).abs().max()), abs(float(scalar) - float(want)))
    print(f"{what}: ssim {float(want):.6f}, error {err:.2e} = {err / tol:.3f} of the bar {tol:.2e}")
    assert err <= tol, (what, err, tol)


@pytest.mark.parametrize("shape,kind", CASES)
@pytest.mark.parametrize("data_range", [None, 1.0], ids=["range_none", "range_1"])
def test_forward_matches_the_fp64_restatement(shape, kind, data_range):
    p, t = _dev(shape, kind)
    want_per, want, tol = _forward_ref(shape, kind, data_range)
    per = metrics.ssim(p, t, data_range, per_image=True)
    scalar = metrics.ssim(p, t, data_range)
    assert per.shape == (shape[0],) and scalar.dim() == 0 and per.dtype == torch.float32 and not per.requires_grad
    _check_forward(per, scalar, want_per, want, tol, f"forward {shape} {kind} range {data_range}")


def test_identical_images_give_one():
    p, _ = _dev((2, 12, 27, 3), "noise")
    assert bool((metrics.ssim(p, p, 1.0, per_image=True) == 1).all())


@pytest.mark.parametrize("shape,kind", CASES)
def test_data_range_none_is_the_range_computed_with_torch(shape, kind):
    p, t = _dev(shape, kind)
    R = float(torch.maximum(p.max() - p.min(), t.max() - t.min()))
    assert torch.equal(metrics.ssim(p, t, None, per_image=True), metrics.ssim(p, t, R, per_image=True))


@pytest.mark.parametrize("shape,kind", CASES)
def test_backward_matches_the_fp64_autograd(shape, kind):
    p, t = _dev(shape, kind)
    want, tol = _grad_ref(shape, kind)
    p.requires_grad_()
    t.requires_grad_()
    metrics.ssim(p, t, 1.0).backward()
    assert t.grad is None and p.grad.shape == p.shape and p.grad.dtype == torch.float32
    err = float((p.grad.double().cpu() - want).abs().max() / want.abs().max())
    print(f"backward {shape} {kind}: max|grad| {float(want.abs().max()):.3e}, error {err:.2e} = {err / tol:.3f} of the bar {tol:.2e}")
    assert err <= tol, (err, tol)


@pytest.mark.parametrize("shape,kind", CASES)
def test_two_runs_give_the_same_bits(shape, kind):
    p, t = _dev(shape, kind)
    runs = []
    for _ in range(2):
        x = p.clone().requires_grad_()
        per = metrics.ssim(x, t, None, per_image=True)
        per.sum().backward()
        runs.append((per.detach(), x.grad))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_upstream_gradients_scale_the_result():
    shape, kind = (3, 16, 16, 3), "noise"
    p, t = _dev(shape, kind)

    def grad(make_loss):
        x = p.clone().requires_grad_()
        make_loss(x).backward()
        return x.grad

    base = grad(lambda x: metrics.ssim(x, t, 1.0))
    assert torch.allclose(grad(lambda x: -2.5 * metrics.ssim(x, t, 1.0)), -2.5 * base, rtol=1e-6, atol=0)
    # per-image weights: each image's gradient is its own, scaled by its weight (the mean gives every image 1 / B)
    w = torch.tensor([0.5, -1.0, 3.0], device=DEV)
    got = grad(lambda x: (metrics.ssim(x, t, 1.0, per_image=True) * w).sum())
    assert torch.allclose(got, base * shape[0] * w[:, None, None, None], rtol=1e-6, atol=0)
    want = ref.grad_ref(*_pair(shape, kind), 1.0, weights=w.cpu())
    _, tol = _grad_ref(shape, kind)
    assert float((got.double().cpu() - want).abs().max() / want.abs().max()) <= tol
    # one image alone gives the same gradient as that image inside the batch: images do not mix
    x1 = p[1:2].clone().requires_grad_()
    metrics.ssim(x1, t[1:2], 1.0).backward()
    assert torch.allclose(x1.grad[0], base[1] * shape[0], rtol=1e-6, atol=0)


def test_half_input_is_its_float_value():
    p, t = _dev((2, 12, 27, 3), "noise")
    assert torch.equal(metrics.ssim(p.half(), t, 1.0, per_image=True), metrics.ssim(p.half().float(), t, 1.0, per_image=True))
    x = p.half().requires_grad_()
    with torch.autocast("cuda", dtype=torch.float16):
        loss = metrics.ssim(x, t, 1.0)
    assert loss.dtype == torch.float32
    loss.backward()
    y = p.half().float().requires_grad_()
    metrics.ssim(y, t, 1.0).backward()
    assert x.grad.dtype == torch.float16 and torch.equal(x.grad, y.grad.half())


def test_meter_is_the_mean_of_its_updates():
    views = [_dev(s, k) for s, k in (((1, 37, 70, 1), "noise"), ((2, 12, 27, 3), "smooth"), ((1, 80, 107, 3), "noise"))]
    meter = metrics.SSIMMeter(device=DEV)
    for p, t in views:
        meter.update(p, t)
    assert meter.N == 3 and torch.is_tensor(meter.V) and meter.V.is_cuda   # the running sum stays on the device
    want = float(sum(metrics.ssim(p, t) for p, t in views)) / 3
    assert meter.measure() == pytest.approx(want, abs=1e-6)
    assert meter.report() == "SSIM = %.6f" % meter.measure()
    meter.clear()
    assert meter.N == 0 and meter.V == 0
    meter.update(*views[0])
    assert meter.measure() == pytest.approx(float(metrics.ssim(*views[0])), abs=1e-7)
    psnr = metrics.PSNRMeter()
    psnr.update(*views[1])
    assert psnr.measure() == pytest.approx(-10 * np.log10(float(((views[1][0] - views[1][1]) ** 2).mean())), abs=1e-4)


# ---------------------------------------------------------------------------------------------------------------- trainer

RENDER = dict(dt_gamma=0, max_steps=512, T_thresh=1e-2)


@functools.lru_cache(maxsize=None)
def _chair():
    ck = scene.make_checkpoint(bound=1.0, seed=0, shaped=True)
    return NeRFNetwork(encoding="hashgrid", bound=1.0, cuda_ray=True).to(DEV).load_checkpoint_dict(ck)


def _views(model, size, angles, noise_seed):
    """What a validation loader yields ({'rays_o', 'rays_d', 'images' [1, H, W, 3]}) for views of ``size`` x ``size``: the ground truth is the
    model's own render plus seeded noise of 0.05, clamped.  Also returns the renders."""
    intr = scene.orbit_intrinsics(size, size, 50.0)
    g = torch.Generator().manual_seed(noise_seed)
    batches, preds = [], []
    model.eval()
    with torch.no_grad():
        for a in angles:
            pose = torch.from_numpy(scene.orbit_pose(4.0, a, -20.0).astype(np.float32))[None].to(DEV)
            rays = get_rays(pose, intr, size, size)
            pred = model.render(rays["rays_o"], rays["rays_d"], staged=True, bg_color=1, perturb=False, **RENDER)["image"].reshape(1, size, size, 3)
            gt = (pred + 0.05 * torch.randn(pred.shape, generator=g).to(DEV)).clamp(0, 1)
            batches.append({"rays_o": rays["rays_o"], "rays_d": rays["rays_d"], "images": gt, "H": size, "W": size})
            preds.append(pred.to(torch.float32))
    return batches, preds


def test_evaluate_loader_reports_ssim_beside_psnr():
    model = _chair()
    tr = Trainer(model, dict(RENDER), num_rays=1024)
    batches, preds = _views(model, 32, (0.0, 120.0), 5)
    res = tr.evaluate_loader(batches)
    mses = [float(torch.mean((p - b["images"]) ** 2)) for p, b in zip(preds, batches)]
    assert res["loss"] == pytest.approx(np.mean(mses), rel=1e-6)
    assert res["psnr"] == pytest.approx(np.mean([-10 * np.log10(m) for m in mses]), rel=1e-6)
    assert tr.stats["valid_loss"] == [res["loss"]] and tr.stats["results"] == [res["psnr"]]
    want = [ref.forward_bar(p.cpu(), b["images"].cpu(), None) for p, b in zip(preds, batches)]
    tol = float(np.mean([w[2] for w in want]))
    direct = float(sum(metrics.ssim(p, b["images"]) for p, b in zip(preds, batches))) / 2
    ref64 = float(np.mean([float(w[1]) for w in want]))
    print(f"evaluate_loader: ssim {res['ssim']:.6f}, restatement {ref64:.6f}, bar {tol:.2e}")
    assert abs(res["ssim"] - direct) <= tol and abs(res["ssim"] - ref64) <= tol
    assert 0.05 < res["ssim"] < 0.999
    # a view smaller than the window: no SSIM, and nothing else changes
    small, small_preds = _views(model, 10, (40.0,), 6)
    res = tr.evaluate_loader(small)
    mse = float(torch.mean((small_preds[0] - small[0]["images"]) ** 2))
    assert res["ssim"] is None and res["psnr"] == pytest.approx(-10 * np.log10(mse), rel=1e-6) and res["loss"] == pytest.approx(mse, rel=1e-6)
    assert len(tr.stats["results"]) == 2


def test_train_step_adds_the_ssim_term_on_patches():
    model = _chair()
    W = 64
    intr = scene.orbit_intrinsics(W, W, 50.0)
    pose = torch.from_numpy(scene.orbit_pose(4.0, 60.0, -20.0).astype(np.float32))[None].to(DEV)
    batches, _ = _views(model, W, (60.0,), 7)
    image = batches[0]["images"][0].contiguous()
    torch.manual_seed(11)
    data = get_rays(pose, intr, W, W, N=2048, patch_size=16, image=image)
    # the layout the loss relies on: patch-major, then patch row, then patch column
    inds = data["inds"].view(8, 16, 16).cpu()
    r, c = torch.arange(16)[None, :, None], torch.arange(16)[None, None, :]
    assert torch.equal(inds, inds[:, :1, :1] + r * W + c)
    assert torch.equal(data["images"].view(8, 16, 16, 3), torch.stack([image[int(i) // W:int(i) // W + 16, int(i) % W:int(i) % W + 16] for i in inds[:, 0, 0]]))

    def step(opt):
        tr = Trainer(model, dict(RENDER, patch_size=16, **opt), num_rays=2048)
        model.train()
        model.zero_grad(set_to_none=True)
        torch.manual_seed(12)   # the march's perturbation
        pred, gt, loss = tr.train_step(data)
        loss.backward()
        return pred.detach(), gt, loss.detach(), model.encoder.embeddings.grad.clone()

    lam = 0.2
    pred, gt, loss, grad = step(dict(ssim_lambda=lam))
    assert pred.shape == (1, 2048, 3) and torch.equal(gt, data["images"])
    pp, gp = pred.cpu().view(8, 16, 16, 3), gt.cpu().view(8, 16, 16, 3)
    _, s64, tol = ref.forward_bar(pp, gp, 1.0)
    want = (1 - lam) * float(((pp.double() - gp.double()) ** 2).mean()) + lam * (1 - float(s64))
    print(f"train_step: loss {float(loss):.6f}, restated {want:.6f}, ssim {float(s64):.4f}, bar {tol:.2e}")
    assert abs(float(loss) - want) <= tol
    for opt in (dict(), dict(ssim_lambda=0)):   # today's step: MSELoss per ray, then the mean over the rays
        pred0, gt0, loss0, grad0 = step(opt)
        assert torch.equal(loss0, torch.nn.MSELoss(reduction="none")(pred0, gt0).mean(-1).mean())
        assert torch.equal(pred0, pred)   # the same draws
    assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0 and not torch.equal(grad, grad0)
    model.zero_grad(set_to_none=True)
    model.eval()
