"""One training step on the device against its float64 restatement (tests/train_step_reference.py): NeRFRenderer.run_cuda in train() mode — the march,
forward_ops (HIP grid / SH encoders with their backward kernels, rocBLAS layers), density_scale, composite_rays_train and the background blend — a
weighted per-ray MSE, backward(), and EVERY parameter's .grad compared with autograd in float64 on the same samples.

Bars.  Per tensor max|g - g64| / max|g64| <= GPU_FACTOR_STEP x that tensor's FP32_VS_F64 (what fp32 arithmetic alone costs on this graph), at most 1e-4;
image and weights_sum within 1e-5 per ray (train_forms_cases.ORACLE_BARS; _forward_errors has the units); rows of the table the restatement leaves at zero are exactly zero.  The rays
within 1e-3 of the transmittance threshold (at most 2 % of a case, test_train_step_host.py) carry loss weight 0 on both sides and are left out of the image
comparison: they may end one sample apart on the device.

Measured on an MI355X: gradients 0.7 .. 17.9 floors (train_step_reference.DEVICE_VS_F64 has every tensor, EXPERIMENTS.md the table); image within
1.4e-6 and weights_sum within 2.7e-7 per ray; fp16: 1.2e-3 .. 9.6e-3 of the largest entry (W3 the largest)."""
import numpy as np
import pytest
import torch

import train_forms_cases as tfc
import train_step_reference as tsr
from pienerf_amd import raymarching
from pienerf_amd.nerf.network import NeRFNetwork
from test_gpu_parity import DEV, T

pytestmark = pytest.mark.gpu


def _net(c):
    kw = dict(bg_radius=c["bg_radius"]) if "bg_radius" in c else {}
    net = NeRFNetwork(encoding="hashgrid", bound=c["bound"], cuda_ray=True, density_scale=c["density_scale"], **kw).to(DEV).load_checkpoint_dict(c["ck"])
    net.mean_count = max(int(c["mean_count"]), 0)
    return net.train()


def _params(net):
    layers = list(net.sigma_net) + list(net.color_net)
    p = {"embeddings": net.encoder.embeddings, **{f"W{i}": l.weight for i, l in enumerate(layers)}}
    if net.bg_net is not None:
        p.update(bg_embeddings=net.encoder_bg.embeddings, bg_W0=net.bg_net[0].weight, bg_W1=net.bg_net[1].weight)
    return p


def _march_is_the_oracles(net, c):
    """The device march on the case's rays equals the oracle's samples bit for bit: the samples are an input both sides share."""
    o, d = T(c["o"]), T(c["d"])
    nears, fars = raymarching.near_far_from_aabb(o, d, net.aabb_train, net.min_near)
    counter = torch.zeros(2, dtype=torch.int32, device=DEV)
    got = raymarching.march_rays_train(o, d, net.bound, net.density_bitfield, net.cascade, net.grid_size, nears, fars, counter, net.mean_count, False, 128,
                                       False, c["dt_gamma"], c["max_steps"])
    for name, a, b in zip(("xyzs", "dirs", "deltas", "rays"), got, (c["xyzs"], c["dirs"], c["deltas"], c["rays"])):
        assert a.shape == b.shape and np.array_equal(a.cpu().numpy(), b), name
    assert int(counter[1]) == len(c["o"])


def _device_step(net, c, weights, half=False, scaler=None, optimizer=None):
    bg = T(c["bg"]) if isinstance(c["bg"], np.ndarray) else (1 if c["bg"] is None else c["bg"])
    with torch.autocast("cuda", dtype=torch.float16, enabled=half):
        out = net.run_cuda(T(c["o"])[None], T(c["d"])[None], dt_gamma=c["dt_gamma"], bg_color=bg, perturb=False, force_all_rays=False,
                           max_steps=c["max_steps"], T_thresh=c["T_thresh"])
        w = T(weights.astype(np.float32))
        loss = (w * ((out["image"][0] - T(c["target"])) ** 2).mean(-1)).sum() / w.sum()
    assert out["image"].requires_grad
    if scaler is None:
        loss.backward()
    else:
        scaler.scale(loss).backward()
        scaler.unscale_(optimizer)
    return out, float(loss.detach())


def _forward_errors(out, ref, far):
    """Per-ray errors against the restatement -> (image, weights_sum, weights_sum relative to the ray's own value).
    image: train_forms_cases' per-ray unit, |err| / max(|ref|, FLOOR).  weights_sum: |err| per ray, the value living in [0, 1].  Relative to the ray's
    own weights_sum no fp32 composite holds 1e-5 on an optically thin ray: there weights_sum = sum(sigma delta), so sigma's own distance from float64
    (4e-6 measured, held to 2e-5 by test_gpu_netform.py) is the ray's, and every alpha = 1 - expf(-x) carries half an ulp of 1.0 (3e-8) absolute
    whatever its size.  The project's fp32 oracle is 3.1e-5 from float64 in that unit on `chair` (a ray of 11 samples, weights_sum 1.1e-3, off by
    3.5e-8), the device 6.4e-5; the third figure is printed for the record."""
    im, ws = out["image"][0].detach().cpu().numpy().astype(np.float64), out["weights_sum"].detach().cpu().numpy().astype(np.float64)
    e_im = (np.abs(im - ref["image"]) / np.maximum(np.abs(ref["image"]), tfc.FLOOR))[far].max()
    e_ws = np.abs(ws - ref["weights_sum"])[far]
    return float(e_im), float(e_ws.max()), float((e_ws / np.maximum(np.abs(ref["weights_sum"][far]), tfc.FLOOR)).max())


@pytest.mark.parametrize("name", list(tsr.CASES))
def test_training_step_gradients_match_the_float64_restatement(name):
    c = tsr.case_inputs(name)
    net = _net(c)
    _march_is_the_oracles(net, c)
    coords = None
    if name == "bg_model":   # the sphere coordinates of the device op, for both sides (it is pinned to the reference kernel in test_gpu_background.py;
        # libm's atan2 one ulp away would move the finest 2-D level's weights by ~2e-3, which is not what this test is about)
        coords = raymarching.sph_from_ray(T(c["o"]), T(c["d"]), c["bg_radius"]).cpu().numpy()
    ref = tsr.reference(name, coords=coords)
    far = ref["weights"] > 0
    assert (~far).mean() <= tsr.MARGIN_SHARE
    out, loss = _device_step(net, c, ref["weights"])
    e_im, e_ws, e_ws_rel = _forward_errors(out, ref, far)
    params = _params(net)
    assert set(params) == set(ref["grads"])
    got = {k: p.grad.detach().cpu().numpy() for k, p in params.items()}
    err = tsr.grad_errors(got, ref["grads"])
    floors = tsr.FP32_VS_F64[name]
    print(f"\n{name}: per ray: image {e_im:.2e}, weights_sum {e_ws:.2e} (relative to its own value {e_ws_rel:.2e}), loss {loss:.6f} vs {ref['loss']:.6f}")
    print("    gradients vs float64: " + ", ".join(f"{k} {err[k]:.2e} ({err[k] / floors[k]:.1f} floors)" for k in err))
    assert e_im < tfc.ORACLE_BARS["image"] and e_ws < tfc.ORACLE_BARS["weights_sum"]
    for k in err:
        assert np.isfinite(got[k]).all() and err[k] <= min(tsr.GPU_FACTOR_STEP * floors[k], tsr.GRAD_BAR_CAP), (k, err[k], floors[k])
    for k in ("embeddings", "bg_embeddings"):
        if k in got:
            untouched = ~ref["grads"][k].any(1)
            assert untouched.any() and not got[k][untouched].any(), k
    if name == "budget":   # rows past the point budget: the background, exactly
        rays, M = c["rays"], len(c["xyzs"])
        dead = rays[rays[:, 1] + rays[:, 2] > M, 0]
        assert len(dead) > 50 and bool((out["weights_sum"][dead] == 0).all()) and bool((out["image"][0][dead] == 1).all())


def test_training_step_fp16_gradients():
    """`chair` under torch.autocast(float16) with a GradScaler: half tables and features, half nn.Linear, the half scatter-add of the grid's backward.
    Unscaled gradients finite and within 1e-2 of the largest entry per tensor (the suite's bar for the half scatter-add) of the float64 restatement.
    The rays within MARGIN_HALF of the threshold carry no loss weight (train_step_reference.py has the arithmetic)."""
    c = tsr.case_inputs("chair")
    net = _net(c)
    ref = tsr.reference("chair", margin_min=tsr.MARGIN_HALF)
    far = ref["weights"] > 0
    assert far.sum() > 0.95 * len(far)
    # GradScaler's default.  The loss is a mean: the largest gradient entry of this batch is 3e-3 (W0), 2e2 after scaling, far inside half's range
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 16)
    optimizer = torch.optim.Adam(net.get_params(1e-2))
    out, loss = _device_step(net, c, ref["weights"], half=True, scaler=scaler, optimizer=optimizer)
    got = {k: p.grad.detach().float().cpu().numpy() for k, p in _params(net).items()}
    err = tsr.grad_errors(got, ref["grads"])
    e_im, e_ws, _ = _forward_errors(out, ref, far)
    print(f"\nfp16 chair: image {e_im:.2e}, weights_sum {e_ws:.2e}, loss {loss:.6f} vs {ref['loss']:.6f}; gradients vs float64: "
          + ", ".join(f"{k} {v:.2e}" for k, v in err.items()))
    for k, v in err.items():
        assert np.isfinite(got[k]).all(), k
        assert v < tsr.HALF_BAR, (k, v)
    assert not got["embeddings"][~ref["grads"]["embeddings"].any(1)].any()
