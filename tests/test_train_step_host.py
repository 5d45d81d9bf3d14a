"""The yardstick of tests/test_gpu_train_step.py, proved on the CPU: the float64 restatement of one training step (train_step_reference.py) agrees in its
forward with the project's fp32 oracle (oracle.nerf_forward, oracle.training.composite_rays_train_forward), the same graph in fp32 stays within the
recorded FP32_VS_F64 of it, and no case has more than 2 % of its rays within 1e-3 of the transmittance threshold.  And ParamEMA (pienerf_amd/training.py),
which runs on any device."""
import numpy as np
import pytest
import torch

import oracle
import train_step_reference as tsr
from oracle import training as otr


@pytest.fixture(scope="module", params=list(tsr.CASES))
def case(request):
    name = request.param
    return name, tsr.case_inputs(name), tsr.reference(name)


def test_fmaf_and_cells_are_the_kernels_fp32_arithmetic():
    """_fmaf rounds once (against exact rational arithmetic); grid_cells's rows and fractions reproduce the oracle's grid forward bit for bit when the
    float64 gather is replaced by the kernel's sequential fp32 sum — for D = 3 and D = 2."""
    from fractions import Fraction
    rng = np.random.default_rng(0)
    a, b = rng.random(4000).astype(np.float32), (rng.random(4000) * 4095).astype(np.float32)
    a[:4], b[:4] = (0.5, 0.25, 1.0, 0.0), (3.0, 4094.0, 4095.0, 7.0)
    got = tsr._fmaf(a, b, 0.5)
    for x, y, g in zip(a, b, got):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(1, 2)
        lo = np.float32(float(exact))     # float(Fraction) and float32(double) round twice; compare distances instead
        cands = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
        best = min(abs(Fraction(float(c)) - exact) for c in cands)
        assert abs(Fraction(float(g)) - exact) == best
    from pienerf_amd import scene
    for D, ck in ((3, scene.make_checkpoint(bound=2.0, seed=3)), (2, scene.make_checkpoint(bound=1.0, seed=0, bg_radius=3.0))):
        emb, off, pls = (ck["embeddings"], ck["offsets"], ck["per_level_scale"]) if D == 3 else (ck["bg_embeddings"], ck["bg_offsets"], ck["bg_per_level_scale"])
        bound = 2.0 if D == 3 else 1.0
        x = ((rng.random((3000, D)) * 2 - 1) * bound).astype(np.float32)
        x[0], x[1] = bound, -bound
        idx, frac, inside = tsr.grid_cells(x, bound, off, pls, 16)
        assert inside.all()
        out = np.zeros((len(x), idx.shape[1], 2), np.float32)
        for k in range(1 << D):
            w = np.ones(frac.shape[:2], np.float32)
            for d in range(D):
                w = w * (frac[:, :, d] if (k >> d) & 1 else np.float32(1) - frac[:, :, d])
            out += w[:, :, None] * emb[idx[:, :, k]]
        u = (x + np.float32(bound)) / np.float32(2 * bound)
        want = oracle.grid_nd_forward(u, emb, off, pls, 16)
        assert np.array_equal(out.reshape(len(x), -1), want)


def test_forward_agrees_with_the_oracle(case):
    name, c, ref = case
    sig, rgb = oracle.nerf_forward(c["xyzs"], c["dirs"], c["ck"], c["bound"])
    sig = np.float32(c["density_scale"]) * sig
    ws, _, image = otr.composite_rays_train_forward(sig, rgb, c["deltas"], c["rays"], c["T_thresh"])
    e_sig = np.abs(sig / ref["sigma"] - 1).max()
    e_rgb = np.abs(rgb - ref["rgb"]).max()
    far = ref["margin"] >= tsr.MARGIN      # a ray at the threshold may end one sample apart in fp32
    e_ws = np.abs(ws - ref["weights_sum"])[far].max()
    print(f"{name}: oracle vs float64: sigma rel {e_sig:.2e}, rgb {e_rgb:.2e}, weights_sum {e_ws:.2e}")
    assert e_sig < 2e-5 and e_rgb < 2e-6 and e_ws < 1e-5     # the bars test_gpu_netform.py / train_forms_cases.ORACLE_BARS hold the kernels to
    if not isinstance(c["bg"], type(None)):
        blended = image + (1 - ws)[:, None] * c["bg"]
        assert np.abs(blended - ref["image"])[far].max() < 1e-5
    live = c["rays"][:, 1] + c["rays"][:, 2] <= len(c["xyzs"])
    if name == "budget":   # rows past the point budget composite to the background and their samples get exactly zero gradient
        dead = c["rays"][~live]
        assert 0.2 < (~live).mean() < 0.6 and (ref["weights_sum"][dead[:, 0]] == 0).all() and (ref["image"][dead[:, 0]] == 1).all()
    else:
        assert live.all()
    assert np.isfinite(ref["loss"]) and ref["loss"] > 0


def test_margin_cap(case):
    name, c, ref = case
    m = ref["margin"]
    share = float((m < tsr.MARGIN).mean())
    print(f"{name}: {int((m < tsr.MARGIN).sum())} of {len(m)} rays within {tsr.MARGIN:g} of the threshold, {int((m < 1e-4).sum())} within 1e-4")
    assert share <= tsr.MARGIN_SHARE
    assert np.array_equal(ref["weights"], (m >= tsr.MARGIN).astype(np.float64))
    assert np.isfinite(m).sum() >= 30              # the pose looks at the object


def test_fp32_run_stays_within_the_recorded_floors(case):
    name, c, ref = case
    r32 = tsr.reference(name, dtype=torch.float32, first=ref)
    err = tsr.grad_errors(r32["grads"], ref["grads"])
    print(f"{name}: fp32 vs float64: " + ", ".join(f"{k} {v:.2e}" for k, v in err.items()))
    assert set(err) == set(tsr.FP32_VS_F64[name]) == set(tsr.PARAMS + (tsr.BG_PARAMS if name == "bg_model" else ()))
    for k, v in err.items():
        assert np.abs(ref["grads"][k]).max() > 0
        assert v <= tsr.FP32_VS_F64[name][k], (k, v)
        assert v >= 0.2 * tsr.FP32_VS_F64[name][k], (k, v)   # the recorded figure is a measured one, not a loose cap


def test_gradient_is_the_loss_slope():
    """The restatement's gradient against a central difference of its own float64 loss, along a random direction per tensor (trex: the smallest case)."""
    c = tsr.case_inputs("trex")
    ref = tsr.reference("trex")
    rng = np.random.default_rng(5)
    for k in ("W1", "W4", "embeddings"):
        direction = rng.standard_normal(ref["grads"][k].shape)
        if k == "embeddings":
            direction *= ref["grads"][k] != 0      # rows no sample touches do not move the loss
            # the shaped checkpoint's occupancy entries (0 or 1 exactly) feed a ReLU that sits AT its kink outside the solid, where autograd's slope is
            # 0 and a central difference sees 1/2: they stay put
            direction *= ((c["ck"][k] != 0) & (c["ck"][k] != 1))
        eps = 1e-6
        vals = []
        for sgn in (1, -1):
            ck = dict(c["ck"])
            ck[k] = c["ck"][k].astype(np.float64) + sgn * eps * direction
            vals.append(tsr.train_step(c["xyzs"], c["dirs"], c["deltas"], c["rays"], ck, c["bound"], c["density_scale"], c["T_thresh"], c["bg"], c["target"],
                                       ref["weights"], n_use=ref["n_use"])["loss"])
        numeric, analytic = (vals[0] - vals[1]) / (2 * eps), float((ref["grads"][k] * direction).sum())
        assert abs(numeric - analytic) < 1e-6 * abs(analytic) + 1e-12, (k, numeric, analytic)


# ---------------------------------------------------------------------------------------------------------------- ParamEMA
def test_param_ema():
    """torch_ema's subset (pienerf_amd/training.py): the shadow follows s -= (1 - d_n)(s - p), d_n = min(decay, (1 + n) / (10 + n)), to fp32 rounding;
    store / copy_to / restore round-trip exactly; the state dict carries num_updates; frozen parameters are left out."""
    from pienerf_amd.training import ParamEMA
    rng = np.random.default_rng(0)
    a, b = torch.nn.Parameter(torch.tensor(rng.standard_normal((5, 3)), dtype=torch.float32)), torch.nn.Parameter(torch.tensor(rng.standard_normal(7), dtype=torch.float32))
    frozen = torch.nn.Parameter(torch.ones(4), requires_grad=False)
    ema = ParamEMA([a, frozen, b], decay=0.95)
    assert len(ema.params) == 2 and ema.params[0] is a and ema.params[1] is b
    shadow = [p.detach().numpy().astype(np.float64) for p in (a, b)]
    for n in range(1, 31):
        with torch.no_grad():
            for p in (a, b, frozen):
                p.add_(torch.tensor(rng.standard_normal(p.shape), dtype=torch.float32))
        ema.update()
        d = min(0.95, (1 + n) / (10 + n))
        for s, p in zip(shadow, (a, b)):
            s -= (1 - d) * (s - p.detach().numpy().astype(np.float64))
        for s, got in zip(shadow, ema.shadow):
            assert np.abs(got.numpy() - s).max() <= 8 * n * np.finfo(np.float32).eps * max(np.abs(s).max(), 1.0)
    assert ema.num_updates == 30
    assert np.abs(ema.shadow[0].numpy() - a.detach().numpy()).max() > 0.1      # an average, not a copy
    # store / copy_to / restore
    before = [p.detach().clone() for p in (a, b, frozen)]
    ema.store()
    ema.copy_to()
    assert torch.equal(a, ema.shadow[0]) and torch.equal(b, ema.shadow[1]) and torch.equal(frozen, before[2])
    ema.restore()
    assert all(torch.equal(p, q) for p, q in zip((a, b, frozen), before)) and ema.stored is None
    # state dict
    sd = ema.state_dict()
    assert sd["num_updates"] == 30 and sd["decay"] == 0.95 and len(sd["shadow_params"]) == 2
    other = ParamEMA([torch.nn.Parameter(torch.zeros(5, 3)), torch.nn.Parameter(torch.zeros(7))], decay=0.5)
    other.load_state_dict(sd)
    assert other.num_updates == 30 and other.decay == 0.95 and all(torch.equal(x, y) for x, y in zip(other.shadow, ema.shadow))
    sd["shadow_params"][0].add_(1.0)                                           # the state dict holds copies
    assert not torch.equal(sd["shadow_params"][0], ema.shadow[0])
    # the warm-up is what moves the first update: d_1 = 2 / 11, not 0.95
    p = torch.nn.Parameter(torch.zeros(1))
    e = ParamEMA([p], decay=0.95)
    with torch.no_grad():
        p.fill_(1.0)
    e.update()
    assert abs(float(e.shadow[0]) - (1 - 2 / 11)) < 1e-6
