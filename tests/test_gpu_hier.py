"""NeRFRenderer.run — the hierarchical-sampling renderer of a model built without cuda_ray — on the GPU: the fused launch (pn_render_hier) and the op
sequence (run_ops) against tests/golden/run_kat.npz, which holds what the reference's own run returned on a CPU (tests/golden/make_golden_run.py), and
the masked colour query, batching, edge shapes, backgrounds, graph capture, training and autocast.

Bounds against the fixture: 1e-4 (the project's bar for tolerance work) on depth, weights_sum and image; the image bound grows by 1.001e-4
per sample of the ray whose weight the reference found within 1e-3 relative of the 1e-4 colour-mask threshold (`n_doubt`): the mask is the only
discontinuity of run in sigma, and a flipped sample moves a channel by at most w * rgb <= 1.001e-4."""
import os

import numpy as np
import pytest
import torch

import oracle
from conftest import ROOT
from pienerf_amd import scene
from pienerf_amd._lib import lib
from pienerf_amd.nerf.network import NeRFNetwork
from pienerf_amd.nerf.renderer import sample_pdf
from pienerf_amd.training import RayImageSet, Trainer
from test_gpu_parity import DEV, T

pytestmark = pytest.mark.gpu

BAR = 1e-4
FLIP = 1.001e-4
NET_BAR = 2e-6      # tests/test_gpu_background.py
MAIN_CASES = ("t128_128", "t512_0", "t64_64", "t64_64_ds2_bg")
EDGE_CASES = ("t1_0", "t2_0", "t3_1")


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(ROOT, "tests", "golden", "run_kat.npz"))


@pytest.fixture(scope="module")
def ck():
    return scene.make_checkpoint(shaped=True, sigma_outside=1e-3)


def _model(ck, **kw):
    return NeRFNetwork(encoding="hashgrid", bound=ck["bound"], cuda_ray=False, **kw).to(DEV).load_checkpoint_dict(ck)


@pytest.fixture(scope="module")
def net(ck):
    return _model(ck)


def _case(kat, name):
    Tn, tn, ds, per_ray = kat[f"{name}_opts"]
    bg = T(kat[f"{name}_bg"]) if per_ray else 1
    return int(Tn), int(tn), float(ds), bg


def _check_against_fixture(kat, name, out, what):
    img, dep, ws = (out[k].detach().cpu().numpy().reshape(s) for k, s in (("image", (-1, 3)), ("depth", (-1,)), ("weights_sum", (-1,))))
    w_img, w_dep, w_ws, nd = kat[f"{name}_image"], kat[f"{name}_depth"], kat[f"{name}_weights_sum"], kat[f"{name}_n_doubt"]
    assert np.array_equal(np.isnan(dep), np.isnan(w_dep)), (what, name, "NaN pattern of depth")
    ok = ~np.isnan(w_dep)
    e_dep = np.abs(dep[ok] - w_dep[ok]).max() if ok.any() else 0.0
    e_ws = np.abs(ws - w_ws).max()
    e_img = np.abs(img - w_img).max(-1)
    sure = nd == 0
    print(f"[hier] {what} {name}: max |d depth| {e_dep:.3e}  |d weights_sum| {e_ws:.3e}  |d image| {e_img[sure].max():.3e} on the {int(sure.sum())} rays with "
          f"n_doubt = 0, {e_img.max():.3e} on all; rays above 1e-5: {int((e_img > 1e-5).sum())}")
    assert e_dep <= BAR and e_ws <= BAR, (what, name, e_dep, e_ws)
    assert (e_img <= BAR + nd * FLIP).all(), (what, name, float(e_img.max()), int((e_img > BAR + nd * FLIP).sum()))


# ---------------------------------------------------------------------------------------------------- 1, 2: against the reference's own run
@pytest.mark.parametrize("name", MAIN_CASES + EDGE_CASES)
def test_fused_run_matches_the_reference_run(kat, ck, name):
    Tn, tn, ds, bg = _case(kat, name)
    m = _model(ck, density_scale=ds)
    with torch.no_grad():
        assert m._hier_fused_ok(T(kat["rays_o"])[None], Tn, tn, bg)
        out = m.run(T(kat["rays_o"])[None], T(kat["rays_d"])[None], num_steps=Tn, upsample_steps=tn, bg_color=bg)
    N = kat["rays_o"].shape[0]
    assert out["image"].shape == (1, N, 3) and out["depth"].shape == (1, N) and out["weights_sum"].shape == (N,)
    assert all(v.dtype == torch.float32 for v in out.values())
    _check_against_fixture(kat, name, out, "fused")


@pytest.mark.parametrize("name", MAIN_CASES + EDGE_CASES)
def test_run_ops_matches_the_reference_run(kat, ck, name):
    Tn, tn, ds, bg = _case(kat, name)
    m = _model(ck, density_scale=ds)
    with torch.no_grad():
        out = m.run_ops(T(kat["rays_o"])[None], T(kat["rays_d"])[None], num_steps=Tn, upsample_steps=tn, bg_color=bg)
    N = kat["rays_o"].shape[0]
    assert out["image"].shape == (1, N, 3) and out["depth"].shape == (1, N) and out["weights_sum"].shape == (N,)
    _check_against_fixture(kat, name, out, "ops")


def test_sample_pdf_on_the_gpu_matches_the_vectors(kat):
    bins, wts = T(kat["pdf_bins"]), T(kat["pdf_weights"])
    got = sample_pdf(bins, wts, int(kat["pdf_n"]), det=True)
    span = (bins[:, -1] - bins[:, 0]).unsqueeze(-1)
    assert float(((got - T(kat["pdf_samples"])).abs() / span).max()) <= 1e-6


# ---------------------------------------------------------------------------------------------------- 3: mask semantics
def test_color_masks_rows_exactly(ck, net):
    g = np.random.default_rng(0)
    M = 5000
    x = g.uniform(-0.9, 0.9, (M, 3)).astype(np.float32)
    d = g.standard_normal((M, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    mask = g.random(M) < 0.13
    mask[64:256] = False      # whole chunks without a masked row
    mask[1024:1100] = True    # and full ones
    with torch.no_grad():
        dens = net.density(T(x))
        rgb = net.color(T(x), T(d), mask=T(mask), geo_feat=dens["geo_feat"])
        _, full = net(T(x), T(d))
        every = net.color(T(x), T(d), geo_feat=dens["geo_feat"])
        none = net.color(T(x), T(d), mask=T(np.zeros(M, bool)), geo_feat=dens["geo_feat"])
        torch.cuda.synchronize()
    assert rgb.shape == (M, 3) and rgb.dtype == torch.float32
    tm = T(mask)
    assert bool((rgb[~tm] == 0).all())                                      # exact zeros, not small numbers
    assert float((rgb[tm] - full[tm]).abs().max()) <= 1e-4
    want = oracle.nerf_forward(x, d, ck, ck["bound"])[1]
    assert np.abs(rgb.cpu().numpy()[mask] - want[mask]).max() <= 1e-4
    assert np.abs(every.cpu().numpy() - want).max() <= 1e-4                 # mask=None colours every row
    assert none.shape == (M, 3) and bool((none == 0).all())                 # an all-false mask: zeros, no launch error
    assert float(rgb[tm].min()) > 0                                          # a sigmoid is never exactly 0: the masked rows were all written
    # a mask that is shorter than a tile, and a single row
    for n in (1, 31, 65):
        with torch.no_grad():
            r = net.color(T(x[:n]), T(d[:n]), mask=T(np.ones(n, bool)), geo_feat=dens["geo_feat"][:n].contiguous())
        assert np.abs(r.cpu().numpy() - want[:n]).max() <= 1e-4


# ---------------------------------------------------------------------------------------------------- 4: batching invariance
def test_results_do_not_depend_on_batching_or_ray_order(kat, net):
    o, d = T(kat["rays_o"]), T(kat["rays_d"])
    o, d = torch.cat([o, o + 0.01, o - 0.01]), torch.cat([d, d, d])        # 6174 rays: more than one batch of 4096
    N = o.shape[0]
    kw = dict(num_steps=64, upsample_steps=64, bg_color=1)
    with torch.no_grad():
        whole = net.render(o[None], d[None], staged=False, **kw)
        again = net.render(o[None], d[None], staged=False, **kw)
        staged = net.render(o[None], d[None], staged=True, max_ray_batch=4096, **kw)
        parts = [net.render(o[None, a:a + 1000], d[None, a:a + 1000], staged=False, **kw) for a in range(0, N, 1000)]
        perm = torch.randperm(N, generator=torch.Generator().manual_seed(0)).to(DEV)
        shuffled = net.render(o[perm][None], d[perm][None], staged=False, **kw)

    def same(a, b):   # bit for bit, NaN included
        return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    assert set(whole) == {"depth", "image", "weights_sum"} and set(staged) == {"depth", "image"}
    for k in ("depth", "image", "weights_sum"):
        assert same(whole[k], again[k]), k
    for k in ("depth", "image"):
        assert staged[k].shape == whole[k].shape and same(whole[k], staged[k]), k
        assert same(whole[k], torch.cat([p[k] for p in parts], dim=1)), k
        assert same(whole[k][0][perm], shuffled[k][0]), k
    assert same(whole["weights_sum"][perm], shuffled["weights_sum"])


# ---------------------------------------------------------------------------------------------------- 5: edge shapes
def test_edge_shapes(kat, ck, net):
    o, d = T(kat["rays_o"]), T(kat["rays_d"])
    with torch.no_grad():
        # the smallest shape the reference refuses: sample_pdf gets an empty weights[:, 1:-1]
        with pytest.raises(RuntimeError, match="num_steps >= 3"):
            net.run(o[None], d[None], num_steps=2, upsample_steps=1)
        with pytest.raises(RuntimeError, match="num_steps >= 3"):
            net.run_ops(o[None], d[None], num_steps=2, upsample_steps=1)
        # N = 1 and N = 0
        full = net.run(o[None], d[None], num_steps=64, upsample_steps=64)
        hit = int(torch.argmax(full["weights_sum"]))
        one = net.run(o[None, hit:hit + 1], d[None, hit:hit + 1], num_steps=64, upsample_steps=64)
        assert one["image"].shape == (1, 1, 3) and torch.equal(one["image"][0, 0], full["image"][0, hit]) and torch.equal(one["weights_sum"][0], full["weights_sum"][hit])
        empty = net.run(o[None, :0], d[None, :0], num_steps=64, upsample_steps=64)
        assert empty["image"].shape == (1, 0, 3) and empty["depth"].shape == (1, 0) and empty["weights_sum"].shape == (0,)
        empty = net.render(o[None, :0], d[None, :0], staged=True, num_steps=64, upsample_steps=0)
        assert empty["image"].shape == (1, 0, 3)
        # beyond the LDS-resident limit the op sequence runs: the same results as run_ops, within the bounds above (here: the same call)
        lim = int(lib().pn_hier_max_samples())
        assert lim >= 512
        sub = slice(0, 2058, 9)
        big = net.run(o[None, sub], d[None, sub], num_steps=lim - 100, upsample_steps=164)
        ref = net.run_ops(o[None, sub], d[None, sub], num_steps=lim - 100, upsample_steps=164)
        assert not net._hier_fused_ok(o[None, sub], lim - 100, 164) and net._hier_fused_ok(o[None, sub], lim - 100, 100)
        assert np.array_equal(np.isnan(big["depth"].cpu().numpy()), np.isnan(ref["depth"].cpu().numpy()))
        assert float((big["weights_sum"] - ref["weights_sum"]).abs().max()) <= BAR
        assert float((big["image"] - ref["image"]).abs().max()) <= BAR
        # T = 1024 + t = 1024 through the op sequence, on a few rays
        wide = net.run(o[None, hit:hit + 8], d[None, hit:hit + 8], num_steps=1024, upsample_steps=1024)
        assert wide["image"].shape == (1, 8, 3) and bool(torch.isfinite(wide["image"]).all())
        assert bool(torch.isfinite(wide["weights_sum"]).all()) and float(wide["weights_sum"].max()) <= 1 + 1e-5 and float(wide["weights_sum"][0]) > 0.5
        # rays that all miss the box
        om = torch.tensor([[0.0, 0.0, 5.0]], device=DEV).repeat(70, 1)
        dm = torch.tensor([[0.0, 0.6, 0.8]], device=DEV).repeat(70, 1)
        for tn in (0, 32):
            miss = net.run(om, dm, num_steps=32, upsample_steps=tn, bg_color=0.25)
            assert miss["image"].shape == (70, 3) and bool((miss["image"] == 0.25).all()) and bool((miss["weights_sum"] == 0).all())
            assert bool(torch.isnan(miss["depth"]).all())
    # bound = 2: two-cascade geometry (aabb +-2, 4096-resolution grid)
    ck2 = scene.make_checkpoint(bound=2.0, seed=3, shaped=True, sigma_outside=1e-3)
    m2 = _model(ck2)
    assert [float(v) for v in m2.aabb_infer.tolist()] == [-2, -2, -2, 2, 2, 2]
    o2, d2 = oracle.get_rays(scene.orbit_pose(5.0, 40.0, -20.0), scene.orbit_intrinsics(48, 48, 50.0), 48, 48)
    with torch.no_grad():
        f2 = m2.run(T(o2)[None], T(d2)[None], num_steps=96, upsample_steps=64)
        r2 = m2.run_ops(T(o2)[None], T(d2)[None], num_steps=96, upsample_steps=64)
    _close_to_ops(f2, r2)
    assert float(f2["weights_sum"].max()) > 0.9
    # aabb_infer narrowed in place is honoured on the next call
    m3 = _model(ck)
    with torch.no_grad():
        before = m3.run(o[None], d[None], num_steps=64, upsample_steps=32)
        m3.aabb_infer[3:] = torch.tensor([0.2, 0.6, 0.3], device=DEV)
        after = m3.run(o[None], d[None], num_steps=64, upsample_steps=32)
        after_ops = m3.run_ops(o[None], d[None], num_steps=64, upsample_steps=32)
    assert float((before["weights_sum"] - after["weights_sum"]).abs().max()) > 0.1
    _close_to_ops(after, after_ops)


def _close_to_ops(fused, ops):
    """Fused against the op sequence where no fixture knows the doubtful samples: depth and weights_sum (continuous in sigma) within 1e-4 everywhere, the image
    within 1e-4 except on the rays where a sample sits at the mask threshold — at most 2 % of them, the condition the fixture's generator enforces."""
    fd, od = fused["depth"].cpu().numpy().reshape(-1), ops["depth"].cpu().numpy().reshape(-1)
    assert np.array_equal(np.isnan(fd), np.isnan(od))
    ok = ~np.isnan(od)
    assert np.abs(fd[ok] - od[ok]).max() <= BAR
    assert float((fused["weights_sum"] - ops["weights_sum"]).abs().max()) <= BAR
    e = (fused["image"] - ops["image"]).abs().reshape(-1, 3).max(-1).values.cpu().numpy()
    assert (e > BAR).mean() <= 0.02, (float(e.max()), float((e > BAR).mean()))


# ---------------------------------------------------------------------------------------------------- 6: backgrounds
def test_backgrounds(kat, ck, net):
    o, d = T(kat["rays_o"]), T(kat["rays_d"])
    N = o.shape[0]
    kw = dict(num_steps=64, upsample_steps=64)
    per_ray = torch.rand(N, 3, generator=torch.Generator().manual_seed(5)).to(DEV)
    three = torch.tensor([0.1, 0.5, 0.9], device=DEV)
    with torch.no_grad():
        base = net.run(o, d, bg_color=0, **kw)
        omw = (1 - base["weights_sum"]).unsqueeze(-1)
        for bg, val in ((None, 1.0), (0.3, 0.3), (three, three), (per_ray, per_ray)):
            got = net.run(o, d, bg_color=bg, **kw)
            assert torch.equal(got["weights_sum"], base["weights_sum"])
            assert float((got["image"] - (base["image"] + omw * val)).abs().max()) <= NET_BAR
        # the model's own background (bg_radius > 0) replaces whatever is passed
        ckb = scene.make_checkpoint(shaped=True, sigma_outside=1e-3, bg_radius=32)
        mb = _model(ckb, bg_radius=32)
        for bg in (None, 0.3, per_ray):
            got = mb.run(o, d, bg_color=bg, **kw)
            assert torch.equal(got["weights_sum"], base["weights_sum"])    # the other tensors of the checkpoint are the same
            want = base["image"] + omw * mb.background_rays(o, d)
            assert float((got["image"] - want).abs().max()) <= NET_BAR
        assert float((got["image"] - base["image"]).abs().max()) > 0.05
        staged = mb.render(o[None], d[None], staged=True, **kw)
        assert torch.equal(staged["image"][0], got["image"])


# ---------------------------------------------------------------------------------------------------- 7: graph capture
def test_fused_run_can_be_captured_into_a_graph(kat, net):
    o, d = T(kat["rays_o"])[:1500].contiguous(), T(kat["rays_d"])[:1500].contiguous()
    kw = dict(num_steps=64, upsample_steps=64, bg_color=1)
    with torch.no_grad():
        eager = net.run(o, d, **kw)       # also builds the packed weights and reads aabb_infer, which a capture cannot
        torch.cuda.synchronize()
        graph, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.graph(graph, stream=s):
            out = net.run(o, d, **kw)
        for _ in range(2):
            for v in out.values():
                v.fill_(-7.0)
            graph.replay()
            torch.cuda.synchronize()
            for k in eager:
                assert torch.equal(out[k].view(torch.int32), eager[k].view(torch.int32)), k


# ---------------------------------------------------------------------------------------------------- 8: training branch
def test_training_branch_is_differentiable(ck):
    m = _model(ck).train()
    o, d = oracle.get_rays(scene.orbit_pose(4.0, 40.0, -20.0), scene.orbit_intrinsics(40, 40, 50.0), 40, 40)
    o, d = T(o)[None], T(d)[None]
    out = m.run(o, d, num_steps=64, upsample_steps=0, perturb=False)
    assert out["image"].requires_grad and out["weights_sum"].requires_grad and out["image"].shape == (1, 1600, 3)
    w = m.color_net[2].weight
    target = torch.rand_like(out["image"])
    ((out["image"] - target) ** 2).mean().backward()
    assert m.encoder.embeddings.grad is not None and float(m.encoder.embeddings.grad.abs().max()) > 0
    direction = torch.randn_like(w)
    analytic = float((w.grad * direction).sum())
    eps, vals = 1e-2, []
    for sgn in (1, -1):
        with torch.no_grad():
            w.add_(sgn * eps * direction)
        vals.append(float(((m.run(o, d, num_steps=64, upsample_steps=0, perturb=False)["image"].detach() - target) ** 2).mean()))
        with torch.no_grad():
            w.sub_(sgn * eps * direction)
    numeric = (vals[0] - vals[1]) / (2 * eps)
    assert abs(numeric - analytic) < 0.05 * abs(analytic) + 1e-6, (numeric, analytic)     # the rule of tests/test_gpu_trainloop.py:54
    # with upsampling the sampler draws random numbers in train() mode (det = not self.training)
    imgs = []
    for seed in (3, 3, 4):
        torch.manual_seed(seed)
        imgs.append(m.run(o, d, num_steps=32, upsample_steps=32, perturb=True)["image"].detach())
    assert torch.equal(imgs[0], imgs[1]) and not torch.equal(imgs[0], imgs[2])
    torch.manual_seed(3)
    a = m.run(o, d, num_steps=32, upsample_steps=32, perturb=False)["image"].detach()
    torch.manual_seed(4)
    b = m.run(o, d, num_steps=32, upsample_steps=32, perturb=False)["image"].detach()
    assert not torch.equal(a, b)                                                              # sample_pdf's rand alone


# ---------------------------------------------------------------------------------------------------- 9: training fits
def test_training_without_a_density_grid_fits_the_teacher_images():
    """Measured on an MI355X (400 steps, 2048 rays, num_steps 64 + upsample_steps 32): see DESIGN.md §7.  The cuda_ray test's factors (0.25 x, + 5 dB,
    > 20 dB) are not copied: this sampler's training behaviour had not been measured when the test was written."""
    ckt = scene.make_checkpoint(bound=1.0, seed=0, shaped=True)
    teacher = _model(ckt)
    Wd = 64
    intr = scene.orbit_intrinsics(Wd, Wd, 50.0)
    poses = np.stack([scene.orbit_pose(4.0, a, e) for a in (0.0, 60.0, 120.0, 180.0, 240.0, 300.0) for e in (-20.0, -50.0)]).astype(np.float32)
    from pienerf_amd.nerf.utils import get_rays
    opt = dict(num_steps=64, upsample_steps=32)
    images = []
    with torch.no_grad():
        for p in poses:
            r = get_rays(T(p[None]), intr, Wd, Wd)
            images.append(teacher.render(r["rays_o"], r["rays_d"], bg_color=1, **opt)["image"].view(Wd, Wd, 3))
    images = torch.stack(images)
    assert float(images.std()) > 0.05
    torch.manual_seed(1)
    student = NeRFNetwork(encoding="hashgrid", bound=1.0, cuda_ray=False).to(DEV)
    data = RayImageSet(T(poses), intr, images, generator=torch.Generator().manual_seed(2))
    tr = Trainer(student, opt, lr=1e-2, iters=400, num_rays=2048)
    psnr0, _ = tr.evaluate(data, 0)
    losses = tr.train(data, 400)
    psnr1, out = tr.evaluate(data, 0)
    msg = f"[hier] training: mean loss first 5 {np.mean(losses[:5]):.5f}, last 20 {np.mean(losses[-20:]):.5f}, PSNR of view 0 {psnr0:.2f} -> {psnr1:.2f} dB"
    print(msg)
    assert np.isfinite(losses).all(), msg
    assert np.mean(losses[-20:]) < np.mean(losses[:5]), msg
    assert psnr1 > psnr0, msg
    assert set(out) == {"depth", "image", "weights_sum"}


# ---------------------------------------------------------------------------------------------------- 10: autocast
def test_render_under_autocast(kat, net):
    o, d = T(kat["rays_o"])[None], T(kat["rays_d"])[None]
    N = o.shape[1]
    hit = T(~kat["miss"])
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        assert not net._hier_fused_ok(o, 64, 32)
        out = net.render(o, d, num_steps=64, upsample_steps=32, bg_color=1)
        staged = net.render(o, d, staged=True, max_ray_batch=1000, num_steps=64, upsample_steps=32, bg_color=1)
    assert out["image"].shape == (1, N, 3) and out["depth"].shape == (1, N) and out["weights_sum"].shape == (N,)
    assert all(v.dtype == torch.float32 for v in out.values()) and all(v.dtype == torch.float32 for v in staged.values())
    assert set(staged) == {"depth", "image"} and staged["image"].shape == (1, N, 3)
    for k in ("image", "depth"):
        assert bool(torch.isfinite(out[k][0][hit]).all()) and bool(torch.isfinite(staged[k][0][hit]).all())
    assert bool(torch.isfinite(out["weights_sum"]).all()) and float(out["weights_sum"].max()) > 0.9
