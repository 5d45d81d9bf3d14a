#!/usr/bin/env python
"""Golden fixtures of the training-data path, produced by RUNNING THE REFERENCE ITSELF on the CPU (build container only; the reference tree does
not exist on the GPU box).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_data.py

Like make_golden_ref.py (whose ``extract`` it imports) this script compiles ORIGINAL definitions, unmodified, from the files under the reference
tree into a namespace that holds the libraries they need, and records what they return:

  * nerf/provider.py  NeRFDataset, nerf_matrix_to_ngp     -> data_kat.npz  ds_{set}_{split}_*  : poses, H, W, intrinsics, radius, images
  * nerf/utils.py     custom_meshgrid, get_rays (N > 0)   -> data_kat.npz  rays_{size}_m{mode}_* : the draws consumed and the results

``cv2`` is not installed.  The class makes three cv2 calls (imread, cvtColor, resize); they are served by a stand-in backed by PIL that returns
BGR(A) like cv2, so the reference's channel swap is exercised.  The decoder is therefore PIL on both sides: the recorded images pin layout,
channel order and scaling, not a PNG decoder.  ``get_rays`` is handed a ``torch`` namespace whose randint / rand / multinomial record what they
return, so the product can be replayed on the same draws.

Inputs are the two tiny data sets beside this file (written here when absent): tiny_blender/ (RGBA, camera_angle_x only, one frame without an
extension, one frame pointing at a missing file) and tiny_colmap/ (RGB, fl_x, cx, cy, h, w).  The colmap ``test`` split draws its two end frames
from numpy's global generator and is not pinned.  Nothing of the reference's text is written anywhere: the outputs are data.
"""
import json
import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_ref import extract  # noqa: E402

BLENDER_OPT = dict(scale=0.8, offset=[0, 0, 0], bound=1.0)
COLMAP_OPT = dict(scale=0.33, offset=[0.1, -0.2, 0.05], bound=2.0)
BLENDER_SPLITS = ("train", "val", "test", "trainval", "all")
COLMAP_SPLITS = ("train", "val", "trainval")


def _pose(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    m = np.eye(4)
    m[:3, :3] = q
    m[:3, 3] = rng.uniform(-4, 4, 3)
    return [[float(np.float32(v)) for v in row] for row in m]


def write_tiny_sets():
    """The two input data sets (deterministic; existing files are left alone)."""
    rng = np.random.default_rng(11)
    root = os.path.join(HERE, "tiny_blender")
    if not os.path.exists(os.path.join(root, "transforms_train.json")):
        H, W = 6, 8
        for split, names in (("train", ["train/r_0", "train/r_1.png", "train/r_gone", "train/r_2"]), ("val", ["val/r_0"]), ("test", ["test/r_0", "test/r_1"])):
            os.makedirs(os.path.join(root, split), exist_ok=True)
            frames = []
            for n in names:
                frames.append({"file_path": "./" + n, "transform_matrix": _pose(rng)})
                if "gone" in n:
                    continue
                img = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
                Image.fromarray(img, "RGBA").save(os.path.join(root, n if n.endswith(".png") else n + ".png"))
            with open(os.path.join(root, f"transforms_{split}.json"), "w") as f:
                json.dump({"camera_angle_x": 0.6911112070083618, "frames": frames}, f, indent=1)
                f.write("\n")
    root = os.path.join(HERE, "tiny_colmap")
    if not os.path.exists(os.path.join(root, "transforms.json")):
        H, W = 12, 16
        os.makedirs(os.path.join(root, "images"), exist_ok=True)
        frames = []
        for i in range(4):
            frames.append({"file_path": f"images/{i:04d}.png", "transform_matrix": _pose(rng)})
            Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8), "RGB").save(os.path.join(root, f"images/{i:04d}.png"))
        with open(os.path.join(root, "transforms.json"), "w") as f:
            json.dump({"fl_x": 17.25, "cx": 7.5, "cy": 6.25, "h": H, "w": W, "frames": frames}, f, indent=1)
            f.write("\n")


def cv2_stand_in():
    """The three cv2 calls of NeRFDataset.__init__ on PIL: imread returns BGR(A) uint8 like cv2."""
    cv2 = types.SimpleNamespace(IMREAD_UNCHANGED=-1, COLOR_BGR2RGB=4, COLOR_BGRA2RGBA=5, INTER_AREA=3)

    def imread(path, flag):
        img = Image.open(path)
        arr = np.asarray(img.convert("RGBA" if "A" in img.getbands() else "RGB"))
        return np.ascontiguousarray(arr[..., [2, 1, 0, 3][:arr.shape[-1]]])

    def cvtColor(image, code):
        return np.ascontiguousarray(image[..., [2, 1, 0, 3][:image.shape[-1]]])

    def resize(image, size, interpolation):
        chans = [np.asarray(Image.fromarray(np.ascontiguousarray(image[..., c])).resize(size, Image.BOX)) for c in range(image.shape[-1])]
        return np.stack(chans, -1)

    cv2.imread, cv2.cvtColor, cv2.resize = imread, cvtColor, resize
    return cv2


class RecordingTorch:
    """``torch`` with randint / rand / multinomial recording what they return."""

    def __init__(self):
        self.log = []

    def __getattr__(self, name):
        fn = getattr(torch, name)
        if name not in ("randint", "rand", "multinomial"):
            return fn

        def wrapped(*a, **k):
            out = fn(*a, **k)
            self.log.append((name, out.clone()))
            return out
        return wrapped


def main():
    write_tiny_sets()
    out = {}
    import packaging.version as pver
    from scipy.spatial.transform import Rotation, Slerp
    from torch.utils.data import DataLoader
    rec = RecordingTorch()
    u_ns = extract("nerf/utils.py", ["custom_meshgrid", "get_rays"], {"torch": rec, "pver": pver})
    tqdm = types.SimpleNamespace(tqdm=lambda it, desc=None: it)
    import glob
    p_ns = extract("nerf/provider.py", ["nerf_matrix_to_ngp", "NeRFDataset"],
                   {"os": os, "cv2": cv2_stand_in(), "glob": glob, "json": json, "tqdm": tqdm, "np": np, "Slerp": Slerp, "Rotation": Rotation,
                    "torch": torch, "DataLoader": DataLoader, "get_rays": u_ns["get_rays"]})
    # ---- 1. the data sets
    for name, o, splits in (("blender", BLENDER_OPT, BLENDER_SPLITS), ("colmap", COLMAP_OPT, COLMAP_SPLITS)):
        opt = types.SimpleNamespace(path=os.path.join(HERE, "tiny_" + name), preload=False, fp16=False, num_rays=64, rand_pose=-1, error_map=True,
                                    color_space="srgb", patch_size=1, **o)
        out[f"ds_{name}_scale"], out[f"ds_{name}_offset"], out[f"ds_{name}_bound"] = np.float64(o["scale"]), np.float64(o["offset"]), np.float64(o["bound"])
        for split in splits:
            d = p_ns["NeRFDataset"](opt, device="cpu", type=split)
            k = f"ds_{name}_{split}_"
            out.update({k + "poses": d.poses.numpy(), k + "HW": np.array([d.H, d.W]), k + "intrinsics": np.asarray(d.intrinsics, np.float64),
                        k + "radius": np.float64(d.radius), k + "n": np.int64(len(d.images)), k + "images": d.images.numpy(),
                        k + "mode": np.array(d.mode), k + "error_map_shape": np.array(d.error_map.shape if d.error_map is not None else [0, 0])})
    # ---- 2. get_rays, N > 0
    rng = np.random.default_rng(5)
    for tag, (H, W), N, intr in (("small", (75, 100), 1024, np.array([110.5, 108.25, 49.0, 38.5])), ("full", (800, 800), 4096, np.array([1111.1, 1111.1, 400.0, 400.0]))):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        pose = np.eye(4, dtype=np.float32)
        pose[:3, :3] = q
        pose[:3, 3] = rng.uniform(-3, 3, 3)
        emap = torch.from_numpy((rng.uniform(0, 1, (1, 128 * 128)) ** 2 * (rng.uniform(0, 1, (1, 128 * 128)) > 0.2)).astype(np.float32))
        k = f"rays_{tag}_"
        out.update({k + "pose": pose, k + "intr": intr, k + "HW": np.array([H, W]), k + "N": np.int64(N), k + "patch": np.int64(16), k + "error_map": emap.numpy()})
        torch.manual_seed(17)
        for mode in (0, 1, 2):
            rec.log.clear()
            r = u_ns["get_rays"](torch.from_numpy(pose).unsqueeze(0), intr, H, W, N, emap if mode == 1 else None, 16 if mode == 2 else 1)
            m = k + f"m{mode}_"
            names = [n for n, _ in rec.log]
            if mode == 0:
                assert names == ["randint"]
                out[m + "draw_inds"] = rec.log[0][1].numpy()
            elif mode == 1:
                assert names == ["multinomial", "rand", "rand"]
                out[m + "draw_cells"] = rec.log[0][1].numpy()[0]
                out[m + "draw_u"] = np.stack([rec.log[1][1].numpy()[0], rec.log[2][1].numpy()[0]])
                out[m + "inds_coarse"] = r["inds_coarse"].numpy()
            else:
                assert names == ["randint", "randint"]
                out[m + "draw_rows"], out[m + "draw_cols"] = rec.log[0][1].numpy(), rec.log[1][1].numpy()
            out.update({m + "inds": r["inds"].numpy(), m + "rays_o": r["rays_o"].numpy().copy(), m + "rays_d": r["rays_d"].numpy().copy()})
    np.savez_compressed(os.path.join(HERE, "data_kat.npz"), **out)
    print("wrote data_kat.npz:", len(out), "arrays,", os.path.getsize(os.path.join(HERE, "data_kat.npz")), "bytes")


if __name__ == "__main__":
    main()
