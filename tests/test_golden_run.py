"""The hierarchical-sampling renderer (NeRFRenderer.run, a model without cuda_ray) on the CPU: sample_pdf against vectors the reference's own
sample_pdf produced, the self-consistency of tests/golden/run_kat.npz (made by tests/golden/make_golden_run.py from the reference's own run), and the
constructor / error surface of a model without a density grid.  The GPU side is tests/test_gpu_hier.py."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

KAT = os.path.join(ROOT, "tests", "golden", "run_kat.npz")
MAIN_CASES = {"t128_128": (128, 128, 1.0), "t512_0": (512, 0, 1.0), "t64_64": (64, 64, 1.0), "t64_64_ds2_bg": (64, 64, 2.0)}
EDGE_CASES = {"t1_0": (1, 0, 1.0), "t2_0": (2, 0, 1.0), "t3_1": (3, 1, 1.0)}


@pytest.fixture(scope="module")
def kat():
    return np.load(KAT)


def test_sample_pdf_matches_the_reference_vectors(kat):
    """The fixture's samples come from the reference's sample_pdf (det=True) on a CPU; the margin, 1e-6 of the bins' span (about 16 fp32 ulp of it), only
    admits a different association of the cumsum, to which the samples respond continuously away from the 1e-5 switch the generator keeps clear of."""
    from pienerf_amd.nerf.renderer import sample_pdf
    bins, wts, n = torch.from_numpy(kat["pdf_bins"]), torch.from_numpy(kat["pdf_weights"]), int(kat["pdf_n"])
    got = sample_pdf(bins, wts, n, det=True)
    assert got.shape == (bins.shape[0], n) and got.dtype == torch.float32
    span = (bins[:, -1] - bins[:, 0]).unsqueeze(-1)
    err = (got - torch.from_numpy(kat["pdf_samples"])).abs() / span
    assert float(err.max()) <= 1e-6, float(err.max())
    # the all-zero row is the uniform pdf: its samples are evenly spread over the bins' span; the single-peak row puts (nearly) all of them into one bin
    assert bool((got[:, 1:] >= got[:, :-1]).all())
    peak = got[2]
    assert int(((peak >= bins[2, 7]) & (peak <= bins[2, 8])).sum()) >= n - 1
    # det=False draws random numbers: two seeds differ, one seed repeats
    torch.manual_seed(3)
    a = sample_pdf(bins, wts, n)
    torch.manual_seed(3)
    b = sample_pdf(bins, wts, n)
    torch.manual_seed(4)
    c = sample_pdf(bins, wts, n)
    assert torch.equal(a, b) and not torch.equal(a, c)
    with pytest.raises(RuntimeError, match="num_steps >= 3"):
        sample_pdf(bins[:, :1], wts[:, :0], n, det=True)


def test_run_fixture_is_self_consistent(kat):
    """A regenerated file cannot silently weaken the GPU tests: shapes, the NaN depths exactly on the rays that miss the box, the 2 % condition on the
    doubtful rays, the expected option sets, and the size limit (no larger than the largest fixture that was here before)."""
    o, d, miss = kat["rays_o"], kat["rays_d"], kat["miss"]
    N = o.shape[0]
    assert N == len(range(0, 800 * 800, 311)) == 2058 and d.shape == (N, 3) and int(kat["ray_stride"]) == 311
    assert miss.dtype == bool and int(miss.sum()) == 94
    assert float(kat["band"]) == 1e-3
    assert sorted(kat["case_names"].tolist()) == sorted(list(MAIN_CASES) + list(EDGE_CASES))
    for name, (Tn, tn, ds) in {**MAIN_CASES, **EDGE_CASES}.items():
        opts = kat[f"{name}_opts"]
        assert (int(opts[0]), int(opts[1]), float(opts[2])) == (Tn, tn, ds)
        img, dep, ws, nd = kat[f"{name}_image"], kat[f"{name}_depth"], kat[f"{name}_weights_sum"], kat[f"{name}_n_doubt"]
        assert img.shape == (N, 3) and dep.shape == (N,) and ws.shape == (N,) and nd.shape == (N,)
        assert np.isfinite(img).all() and np.isfinite(ws).all()
        if Tn == 1:   # no sample at all (the reference's deltas are empty): depth 0 everywhere, the image is the background
            assert not np.isnan(dep).any() and (ws == 0).all() and (img == 1).all()
        else:
            assert np.array_equal(np.isnan(dep), miss)
            assert (ws[miss] == 0).all()
        assert (nd >= 0).all() and (nd > 0).mean() <= 0.02
        if bool(opts[3]):
            assert kat[f"{name}_bg"].shape == (N, 3)
            assert np.abs(img[miss] - kat[f"{name}_bg"][miss]).max() == 0
    for name in MAIN_CASES:
        assert int((kat[f"{name}_weights_sum"] > 0.5).sum()) > 500   # the object is in view
    assert os.path.getsize(KAT) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "train_kat.npz"))


def test_model_without_density_grid_constructs_and_refuses_cpu_tensors():
    from pienerf_amd.nerf.network import NeRFNetwork
    net = NeRFNetwork(encoding="hashgrid", bound=1.0, cuda_ray=False)
    keys = set(net.state_dict().keys())
    assert keys == {"aabb_train", "aabb_infer", "encoder.offsets", "encoder.embeddings", "sigma_net.0.weight", "sigma_net.1.weight",
                    "color_net.0.weight", "color_net.1.weight", "color_net.2.weight"}   # the reference's key set without cuda_ray
    o, d = torch.zeros(1, 4, 3), torch.tensor([0.0, 0.0, 1.0]).expand(1, 4, 3)
    for kw in (dict(), dict(staged=True), dict(num_steps=512, upsample_steps=0)):
        with pytest.raises(RuntimeError, match="GPU only"):
            net.eval().render(o, d, **kw)
    with pytest.raises(RuntimeError, match="GPU only"):
        net.train().render(o, d, perturb=True)
    # the smallest shape the reference rejects (its sample_pdf fails on the empty weights[:, 1:-1]) is refused before any launch
    with pytest.raises(RuntimeError, match="num_steps >= 3"):
        net.eval().render(o, d, num_steps=2, upsample_steps=1)
    with pytest.raises(RuntimeError, match="only the cuda_ray path"):
        net.render_deformed(o, d)


def test_trainer_passes_the_sampler_options_through():
    from pienerf_amd.nerf.network import NeRFNetwork
    from pienerf_amd.training import Trainer
    net = NeRFNetwork(encoding="hashgrid", bound=1.0, cuda_ray=False)
    tr = Trainer.__new__(Trainer)
    tr.opt = dict(num_steps=64, upsample_steps=32, dt_gamma=0, W=800)
    assert tr._render_opts() == dict(num_steps=64, upsample_steps=32, dt_gamma=0)
    tr.opt = dict(dt_gamma=0, max_steps=512, T_thresh=1e-2)
    assert tr._render_opts() == dict(dt_gamma=0, max_steps=512, T_thresh=1e-2)
    assert not hasattr(net, "density_bitfield")
