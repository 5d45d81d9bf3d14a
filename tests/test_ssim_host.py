"""SSIM without a GPU: the C ABI's new entries, main_train's --ssim_lambda, metrics.ssim's refusals, and the invariants of the torch restatement
(tests/ssim_reference.py) that tests/test_gpu_ssim.py measures the kernels against."""
import os
import re

import pytest
import torch

import ssim_reference as ref
from pienerf_amd import _lib, main_train, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pn_ssim_work_bytes", "pn_ssim_range", "pn_ssim_forward", "pn_ssim_backward")


def test_ssim_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pienerf_hip.h")).read(), flags=re.S)
    h = _lib.lib()
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} is not declared in include/pienerf_hip.h"
        assert name in _lib.SIGNATURES and hasattr(h, name)
    assert "pn_ssim.hip" in __import__("pienerf_amd.build", fromlist=["UNITS"]).UNITS


def test_ssim_entries_refuse_bad_arguments_without_launching():
    """PN_ERR_ARG (1) comes back before anything is enqueued, so this runs without a device."""
    import ctypes
    h, p = _lib.lib(), ctypes.c_void_p(64)
    assert h.pn_ssim_work_bytes(1, 10, 32) == 0 and h.pn_ssim_work_bytes(1, 32, 10) == 0 and h.pn_ssim_work_bytes(0, 32, 32) == 0
    assert h.pn_ssim_work_bytes(2, 11, 11) == 4096 + 2 * 8          # one tile per image
    assert h.pn_ssim_work_bytes(1, 80, 107) == 4096 + 5 * 7 * 8     # valid region 70 x 97 in 16 x 16 tiles
    assert h.pn_ssim_forward(p, p, 1, 10, 32, 3, p, p, p, None, None, None, None) == 1      # H < 11
    assert h.pn_ssim_forward(p, p, 1, 32, 10, 3, p, p, p, None, None, None, None) == 1      # W < 11
    assert h.pn_ssim_forward(None, p, 1, 32, 32, 3, p, p, p, None, None, None, None) == 1   # null image
    assert h.pn_ssim_forward(p, p, 1, 32, 32, 3, p, p, p, p, None, None, None) == 1         # one map of three
    assert h.pn_ssim_forward(p, p, 1, 32, 32, 0, p, p, p, None, None, None, None) == 1      # no channel
    assert h.pn_ssim_backward(p, p, 1, 10, 32, 3, p, p, p, p, p, None) == 1
    assert h.pn_ssim_backward(p, p, 1, 32, 32, 3, p, p, None, p, p, None) == 1
    assert h.pn_ssim_range(None, None, 0, 0.0, None, p, None) == 1                          # explicit range must be positive
    assert h.pn_ssim_range(p, None, 16, 1.0, p, p, None) == 1
    assert h.pn_ssim_range(None, None, 0, 1.0, None, None, None) == 1


def test_main_train_takes_ssim_lambda_with_patches_only():
    opt = main_train.parse(["--patch_size", "16", "--ssim_lambda", "0.2", "--num_rays", "2048"])
    assert opt.ssim_lambda == 0.2 and opt.patch_size == 16
    assert main_train.parse([]).ssim_lambda == 0.0
    with pytest.raises(SystemExit, match="patch_size"):
        main_train.parse(["--ssim_lambda", "0.2"])
    with pytest.raises(SystemExit, match="patch_size"):
        main_train.parse(["--ssim_lambda", "0.2", "--patch_size", "8", "--num_rays", "2048"])
    with pytest.raises(SystemExit, match="ssim_lambda"):
        main_train.parse(["--ssim_lambda", "1.5", "--patch_size", "16", "--num_rays", "2048"])
    with pytest.raises(SystemExit, match="ssim_lambda"):
        main_train.parse(["--ssim_lambda", "-0.1"])
    help_text = " ".join(main_train.parser().format_help().split())
    assert "--ssim_lambda" in help_text and "patches train with the MSE term alone, or with --ssim_lambda" in help_text


def test_ssim_refuses_cpu_tensors_and_small_images():
    a = torch.rand(1, 16, 16, 3)
    with pytest.raises(RuntimeError, match="GPU"):
        metrics.ssim(a, a)
    with pytest.raises(RuntimeError, match="window"):
        metrics.ssim(torch.rand(1, 10, 16, 3), torch.rand(1, 10, 16, 3))
    with pytest.raises(RuntimeError, match="window"):
        metrics.ssim(torch.rand(1, 16, 10, 3), torch.rand(1, 16, 10, 3))
    with pytest.raises(RuntimeError, match="differ"):
        metrics.ssim(a, torch.rand(1, 16, 17, 3))
    with pytest.raises(RuntimeError, match=r"\[B, H, W, C\]"):
        metrics.ssim(a[0], a[0])


def test_meters_have_the_reference_interface():
    for cls, word in ((metrics.PSNRMeter, "PSNR"), (metrics.SSIMMeter, "SSIM")):
        for name in ("clear", "update", "measure", "report", "write"):
            assert callable(getattr(cls, name))
    m = metrics.PSNRMeter()
    a = torch.full((1, 4, 4, 3), 0.5)
    m.update(a, a + 0.1)
    m.update(a, a + 0.01)
    assert m.N == 2 and m.measure() == pytest.approx((20.0 + 40.0) / 2, abs=1e-4)
    assert m.report() == "PSNR = %.6f" % m.measure()

    class Writer:
        def add_scalar(self, *a):
            self.got = a
    w = Writer()
    m.write(w, 7, prefix="val")
    assert w.got == (os.path.join("val", "PSNR"), m.measure(), 7)
    m.clear()
    assert m.N == 0 and m.V == 0


def test_taps_are_normalised_and_symmetric():
    g = ref.taps(torch.float64)
    assert g.shape == (11,) and abs(float(g.sum()) - 1) < 1e-7 and torch.equal(g, g.flip(0)) and int(g.argmax()) == 5
    assert torch.equal(g.to(torch.float32).to(torch.float64), g)   # fp32 values


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_restatement_invariants(dtype):
    g = torch.Generator().manual_seed(3)
    a = torch.rand(2, 20, 23, 3, generator=g)
    n = torch.randn(2, 20, 23, 3, generator=g)
    assert float(ref.ssim(a, a, None, dtype)) == 1.0                       # identical images: exactly 1
    assert torch.equal(ref.ssim_per_image(a, a, 1.0, dtype), torch.ones(2, dtype=dtype))
    b = (a + 0.1 * n).clamp(0, 1)
    tol = 0 if dtype == torch.float64 else 1e-6
    assert abs(float(ref.ssim(a, b, None, dtype) - ref.ssim(b, a, None, dtype))) <= tol + 1e-15   # symmetric in its arguments
    values = [float(ref.ssim((a + s * n).clamp(0, 1), a, 1.0, dtype)) for s in (0.0, 0.02, 0.05, 0.1, 0.3)]
    assert values[0] == 1.0 and all(x > y for x, y in zip(values, values[1:])), values   # falls as the noise grows
    assert ref.ssim_per_image(a, b, None, dtype).shape == (2,)
    assert float(ref.ssim(a, b, None, dtype)) == pytest.approx(float(ref.ssim_per_image(a, b, None, dtype).mean()))


def test_restatement_gradient_reaches_pred_only_through_the_formula():
    p, t = ref.noise_pair((1, 12, 13, 2), 0)
    g = ref.grad_ref(p, t, 1.0)
    assert g.shape == p.shape and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    # directional derivative against a central difference of the fp64 value
    d = torch.randn(p.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    eps = 1e-6
    num = float(ref.ssim(p.double() + eps * d, t, 1.0) - ref.ssim(p.double() - eps * d, t, 1.0)) / (2 * eps)
    assert num == pytest.approx(float((g * d).sum()), rel=1e-5)
