"""The training-data path on the host (no GPU): NeRFDataset against values the REFERENCE's own class returned for the two tiny data sets under
tests/golden (tests/golden/make_golden_data.py ran it; the PNG decoder is PIL on both sides, so the images pin layout, channel order and scaling),
the data-set writer, main_train's option set against the reference's namespace, and the C ABI of csrc/pn_train_batch.hip."""
import ctypes
import json
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import ROOT

G = os.path.join(ROOT, "tests", "golden")
BATCH_SYMBOLS = ("pn_sample_cells", "pn_train_batch", "pn_error_map_update")
SPLITS = {"blender": ("train", "val", "test", "trainval", "all"), "colmap": ("train", "val", "trainval")}


def _opt(k, name, **over):
    o = dict(path=os.path.join(G, "tiny_" + name), preload=False, scale=float(k[f"ds_{name}_scale"]), offset=[float(v) for v in k[f"ds_{name}_offset"]],
             bound=float(k[f"ds_{name}_bound"]), fp16=False, num_rays=64, rand_pose=-1, error_map=True, color_space="srgb", patch_size=1)
    o.update(over)
    return o


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(G, "data_kat.npz"))


@pytest.mark.parametrize("name,split", [(n, s) for n in SPLITS for s in SPLITS[n]])
def test_dataset_equals_the_reference_class(kat, name, split):
    from pienerf_amd.nerf.provider import NeRFDataset
    opt = _opt(kat, name)
    d = NeRFDataset(opt if split != "val" else types.SimpleNamespace(**opt), device="cpu", type=split)   # a mapping or a namespace
    k = f"ds_{name}_{split}_"
    poses, images = d.poses.numpy(), d.images.numpy()
    want_poses, want_images = kat[k + "poses"], kat[k + "images"]
    assert d.mode == str(kat[k + "mode"]) and len(d) == int(kat[k + "n"]) == len(images)
    if split == "all":   # the reference reads the JSON files in glob's order, which the file system decides: compare as sets of views
        order = np.lexsort(poses.reshape(len(poses), -1).T[::-1])
        want_order = np.lexsort(want_poses.reshape(len(want_poses), -1).T[::-1])
        poses, images, want_poses, want_images = poses[order], images[order], want_poses[want_order], want_images[want_order]
    assert poses.dtype == np.float32 and np.array_equal(poses.view(np.uint32), want_poses.view(np.uint32))
    assert [d.H, d.W] == list(kat[k + "HW"]) and np.array_equal(np.asarray(d.intrinsics, np.float64), kat[k + "intrinsics"])
    assert abs(d.radius - float(kat[k + "radius"])) <= 2.0 ** -23 * float(kat[k + "radius"])
    assert images.dtype == np.float32 and np.array_equal(images, want_images)
    if split in ("train", "trainval", "all"):
        assert list(d.error_map.shape) == list(kat[k + "error_map_shape"]) == [len(images), 128 * 128] and bool((d.error_map == 1).all())
        assert d.error_map.dtype == torch.float32 and d.training and d.num_rays == 64
    else:
        assert d.error_map is None and list(kat[k + "error_map_shape"]) == [0, 0] and not d.training and d.num_rays == -1
    loader = d.dataloader()
    assert loader._data is d and loader.has_gt and loader.batch_size == 1 and len(loader) == len(d)


def test_blender_rules(kat):
    from pienerf_amd.nerf.provider import NeRFDataset
    d = NeRFDataset(_opt(kat, "blender"), device="cpu", type="train")
    frames = json.load(open(os.path.join(G, "tiny_blender", "transforms_train.json")))["frames"]
    assert len(frames) == 4 and len(d) == 3                                    # the frame pointing at a missing file is skipped
    assert d.images.shape == (3, 6, 8, 4)                                      # RGBA; r_0 and r_2 are named without extension
    assert d.intrinsics[0] == d.intrinsics[1] and tuple(d.intrinsics[2:]) == (4.0, 3.0)   # a lone camera_angle_x: fl_y = fl_x; cx, cy = W/2, H/2
    v = NeRFDataset(_opt(kat, "blender"), device="cpu", type="val")
    assert not v.training and v.error_map is None and v.num_rays == -1 and not isinstance(v.dataloader().sampler, torch.utils.data.RandomSampler)
    assert isinstance(d.dataloader().sampler, torch.utils.data.RandomSampler)
    assert NeRFDataset(_opt(kat, "blender", error_map=False), device="cpu", type="train").error_map is None
    with pytest.raises(NotImplementedError, match="CLIP"):
        NeRFDataset(_opt(kat, "blender", rand_pose=0), device="cpu", type="train")
    with pytest.raises(NotImplementedError, match="transforms"):
        NeRFDataset(_opt(kat, "blender", path=G), device="cpu", type="train")


def test_linear_colour_space_converts_once_at_load(kat):
    from pienerf_amd import io
    from pienerf_amd.nerf.provider import NeRFDataset
    a = NeRFDataset(_opt(kat, "blender"), device="cpu", type="train").images
    b = NeRFDataset(_opt(kat, "blender", color_space="linear"), device="cpu", type="train").images
    assert torch.equal(b[..., :3], io.srgb_to_linear(a[..., :3])) and torch.equal(b[..., 3], a[..., 3])


@pytest.mark.parametrize("name", ["blender", "colmap"])
def test_downscale_halves_size_and_intrinsics(kat, name):
    """The 8-bit image is box-filtered: every pixel within half a level of the numpy block mean."""
    from PIL import Image
    from pienerf_amd.nerf.provider import NeRFDataset
    full = NeRFDataset(_opt(kat, name), device="cpu", type="train")
    half = NeRFDataset(_opt(kat, name), device="cpu", type="train", downscale=2)
    assert (half.H, half.W) == (full.H // 2, full.W // 2) and half.images.shape[1:3] == (half.H, half.W)
    if name == "colmap":
        assert np.array_equal(half.intrinsics, full.intrinsics / 2)
    else:   # from the halved W and the angle
        assert half.intrinsics[0] == half.W / (2 * np.tan(0.6911112070083618 / 2)) and tuple(half.intrinsics[2:]) == (half.W / 2, half.H / 2)
    src = "train/r_0.png" if name == "blender" else "images/0001.png"
    raw = np.asarray(Image.open(os.path.join(G, "tiny_" + name, src))).astype(np.float64)
    mean = raw.reshape(half.H, 2, half.W, 2, -1).mean(axis=(1, 3))
    levels = half.images[0].numpy().astype(np.float64) * 255
    assert np.abs(levels - np.round(levels)).max() < 1e-4            # 8-bit levels
    assert np.abs(np.round(levels) - mean).max() <= 0.5


def test_colmap_test_split_interpolates_between_two_poses(kat):
    from pienerf_amd.nerf.provider import NeRFDataset
    np.random.seed(3)
    d = NeRFDataset(_opt(kat, "colmap"), device="cpu", type="test", n_test=6)
    assert d.images is None and not d.dataloader().has_gt and d.poses.shape == (7, 4, 4) and d.poses.dtype == torch.float32
    R = d.poses[:, :3, :3].double()
    assert float((R @ R.transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-6
    assert bool((d.poses[:, 3] == torch.tensor([0.0, 0, 0, 1])).all())
    everything = NeRFDataset(_opt(kat, "colmap"), device="cpu", type="trainval").poses
    for end in (d.poses[0], d.poses[-1]):
        assert float((everything - end).abs().amax(dim=(1, 2)).min()) < 1e-6
    assert float((d.poses[0] - d.poses[-1]).abs().max()) > 1e-3


def test_written_dataset_loads_back_to_the_converted_matrices(tmp_path, kat):
    from pienerf_amd import io, scene
    from pienerf_amd.nerf.provider import NeRFDataset
    rng = np.random.default_rng(0)
    mats, imgs = {}, {}
    for s, n in (("train", 3), ("val", 1), ("test", 2)):
        m = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
        for i in range(n):
            m[i, :3, :3] = np.linalg.qr(rng.standard_normal((3, 3)))[0]
            m[i, :3, 3] = rng.uniform(-5, 5, 3)
        mats[s], imgs[s] = m, rng.integers(0, 256, (n, 10, 14, 4 if s == "train" else 3), dtype=np.uint8)
    out = scene.write_blender_dataset(str(tmp_path), W=14, H=10, fovy=40.0, scale=0.7, offset=(0.1, 0.0, -0.3), matrices=mats, images=imgs)
    for s in mats:
        d = NeRFDataset(_opt(kat, "blender", path=str(tmp_path), scale=0.7, offset=[0.1, 0.0, -0.3]), device="cpu", type=s)
        want = np.stack([io.nerf_matrix_to_ngp(m, scale=0.7, offset=(0.1, 0.0, -0.3)) for m in mats[s]])
        assert np.array_equal(d.poses.numpy().view(np.uint32), want.view(np.uint32)) and np.array_equal(out[s]["poses"], want)
        assert np.array_equal(d.images.numpy(), imgs[s].astype(np.float32) / 255)
        assert np.array_equal(d.intrinsics, out["intrinsics"]) and d.intrinsics[0] == d.intrinsics[1] and (d.H, d.W) == (10, 14)
    assert abs(out["intrinsics"][1] - 10 / (2 * np.tan(np.radians(40.0) / 2))) < 1e-9
    # the inverse conversion: an ngp pose survives the round trip through the blender convention up to the translation's rounding
    p = scene.orbit_pose(4.0, 60.0, -20.0)
    back = io.nerf_matrix_to_ngp(scene.ngp_matrix_to_nerf(p, 0.8), scale=0.8)
    assert np.array_equal(back[:3, :3], p[:3, :3]) and np.abs(back[:3, 3] - p[:3, 3]).max() < 1e-6
    assert np.array_equal(scene.dataset_orbit(12), np.stack([scene.orbit_pose(4.0, a, e) for a in (0.0, 60.0, 120.0, 180.0, 240.0, 300.0)
                                                             for e in (-20.0, -50.0)]).astype(np.float32))


def test_parser_agrees_with_the_reference_namespace():
    """opts_chair.json: the argv of the reference's chair command and the namespace its get_opts.py returned.  The argv also carries options of the
    simulate-and-render groups, which main_train does not have: those are left to parse_known_args."""
    from pienerf_amd import main_train
    ref = json.load(open(os.path.join(G, "opts_chair.json")))
    opt, rest = main_train.parser().parse_known_args(ref["argv"])
    opt = vars(main_train.derive(opt))
    assert all(a.startswith("--") for a in rest[::2])
    shared = sorted(set(opt) & set(ref["opt"]))
    assert len(shared) >= 30 and {"O", "fp16", "cuda_ray", "preload", "scale", "bound", "dt_gamma", "iters", "lr", "num_rays", "error_map", "patch_size",
                                  "rand_pose", "ckpt", "color_space", "max_steps", "T_thresh", "update_extra_interval"} <= set(shared)
    for key in shared:
        assert opt[key] == ref["opt"][key], key
    # the defaults, without the derived options
    ref2 = json.load(open(os.path.join(G, "opts_trex.json")))
    plain = vars(main_train.parser().parse_args(["--path", "x"]))
    for key in ("bound", "scale", "dt_gamma", "offset", "min_near", "density_thresh", "bg_radius", "iters", "lr", "num_rays", "seed"):
        assert plain[key] == ref2["opt"][key], key


def test_derived_option_rules():
    from pienerf_amd import main_train
    o = main_train.parse(["--path", "x"])
    assert not (o.fp16 or o.cuda_ray or o.preload) and (o.scale, o.bound, o.dt_gamma) == (0.33, 2.0, 1 / 128)
    o = main_train.parse(["--path", "x", "-O"])
    assert o.fp16 and o.cuda_ray and o.preload
    o = main_train.parse(["--path", "x", "--dataset_type", "synthetic", "--scale", "0.5"])
    assert (o.scale, o.bound, o.dt_gamma) == (0.8, 1.0, 0.0)
    o = main_train.parse(["--path", "x", "--patch_size", "16", "--error_map"])
    assert o.patch_size == 16 and o.error_map is False
    assert main_train.parse(["--path", "x", "--error_map"]).error_map is True
    with pytest.raises(SystemExit, match="divide"):
        main_train.parse(["--path", "x", "--patch_size", "24"])
    for argv in (["--ff"], ["--tcnn"], ["--gui"], ["--clip_text", "a chair"], ["--rand_pose", "0"]):
        with pytest.raises(SystemExit, match=argv[0]):
            main_train.parse(["--path", "x"] + argv)
    assert "MSE term alone" in " ".join(main_train.parser().format_help().split())   # the patch branch's LPIPS term is not built


def test_batch_symbols_in_library_header_and_signatures():
    from pienerf_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pienerf_hip.h")).read(), flags=re.S)
    so = ctypes.CDLL(_lib.LIB_PATH)
    for n in BATCH_SYMBOLS:
        assert re.search(r"\b" + n + r"\s*\(", text), n
        assert n in _lib.SIGNATURES, n
        assert hasattr(so, n), n
    h, d = _lib.lib(), ctypes.c_void_p(16)
    PN_ERR_ARG = 1
    assert h.pn_sample_cells(d, d, 16385, 4, d, d, None) == PN_ERR_ARG          # more cells than one workgroup holds
    assert h.pn_sample_cells(d, d, 128, 129, d, d, None) == PN_ERR_ARG          # more draws than cells
    assert h.pn_sample_cells(d, None, 128, 4, d, d, None) == PN_ERR_ARG
    assert h.pn_train_batch(d, 1.0, 1.0, 0.0, 0.0, 8, 8, 4, 1, d, None, None, 1, None, 0, d, d, d, None, None) == PN_ERR_ARG    # mode 1 without uniforms
    assert h.pn_train_batch(d, 1.0, 1.0, 0.0, 0.0, 8, 8, 6, 2, d, d, None, 2, None, 0, d, d, d, None, None) == PN_ERR_ARG       # 6 rays, patches of 4
    assert h.pn_train_batch(d, 1.0, 1.0, 0.0, 0.0, 8, 8, 4, 0, d, None, None, 1, d, 5, d, d, d, d, None) == PN_ERR_ARG          # 5 channels
    assert h.pn_train_batch(d, 1.0, 1.0, 0.0, 0.0, 8, 8, 4, 0, d, None, None, 1, d, 3, d, d, d, None, None) == PN_ERR_ARG       # image without pixels_out
    assert h.pn_error_map_update(d, d, None, 4, None) == PN_ERR_ARG


def test_training_forms_refuse_a_cpu_tensor(kat):
    from pienerf_amd.nerf.provider import NeRFDataset
    from pienerf_amd.nerf.utils import error_map_update, get_rays, sample_cells
    with pytest.raises(RuntimeError, match="GPU"):
        get_rays(torch.eye(4)[None], (10.0, 10.0, 4.0, 4.0), 8, 8, N=16)
    with pytest.raises(RuntimeError, match="GPU"):
        sample_cells(torch.ones(128), 4)
    with pytest.raises(RuntimeError, match="GPU"):
        error_map_update(torch.ones(128 * 128), torch.arange(4), torch.zeros(4))
    with pytest.raises(RuntimeError, match="GPU"):   # a batch is made on the device
        NeRFDataset(_opt(kat, "blender"), device="cpu", type="train").collate([0])
