"""``NeRFDataset``: posed images of a ``transforms*.json`` data set (blender-synthetic or COLMAP layout) as training and evaluation batches, with the
reference's attributes and rules (nerf/provider.py:94-332).  The rays, the pixel choice and the gather of the ground truth of a training batch are
one HIP launch (``nerf.utils.get_rays`` with N > 0, csrc/pn_train_batch.hip).

Images are decoded with PIL (the reference uses cv2): RGB or RGBA, 8 bits, scaled by 1 / 255 to float32.  A size change (``downscale``, or a file
whose size differs from the JSON's) is a box filter on the 8-bit image, the area average that ``cv2.INTER_AREA`` computes.  For integer factors it is
the block mean of each channel rounded to the nearest level, computed in integers: PIL's own BOX resize rounds to 8 bits after each of its two
passes and lands up to a whole level from the block mean (measured), and its ``reduce`` is off by more than half a level at factor 3.  Other ratios
take PIL's BOX filter per channel.  That step is not pinned to cv2.

What differs from the reference, on purpose:
  * ``color_space == 'linear'``: the colour channels are converted once at load (``io.srgb_to_linear`` is elementwise, so this equals the reference's
    conversion of every batch, trainer.py:184-185 / :264-265);
  * preloaded images are float32 (the reference's half-precision preload is a memory saving);
  * the error map lives on ``device`` whether or not the images are preloaded: the kernels that read and update it run there;
  * ``type='all'`` reads the blender JSON files in sorted order (the reference: in glob's order);
  * ``rand_pose >= 0`` (CLIP-guided training on random poses) is refused: that package is not part of this project.
"""
import glob
import json
import os

import numpy as np
import torch
from torch.utils.data import DataLoader

from ..io import nerf_matrix_to_ngp, srgb_to_linear
from .utils import get_rays

OPT_FIELDS = ("path", "preload", "scale", "offset", "bound", "fp16", "num_rays", "rand_pose", "error_map", "color_space", "patch_size")


def _field(opt, name):
    return opt[name] if isinstance(opt, dict) or hasattr(opt, "keys") else getattr(opt, name)


def read_image(path, size=None):
    """uint8 [H, W, 3 or 4] (RGB order) of an image file; ``size`` = (W, H): box-filtered to that size when it differs (see the module's docstring)."""
    from PIL import Image
    with Image.open(path) as img:
        img = img.convert("RGBA" if "A" in img.getbands() else "RGB")
        if size is None or img.size == tuple(size):
            return np.asarray(img).copy()
        (W, H), (w, h) = size, img.size
        if w % W == 0 and h % H == 0:
            n = (w // W) * (h // H)
            total = np.asarray(img).astype(np.int64).reshape(H, h // H, W, w // W, -1).sum(axis=(1, 3))
            return ((2 * total + n) // (2 * n)).astype(np.uint8)   # the block mean, halves rounded up
        # per channel: PIL's own RGBA resize premultiplies alpha, cv2 does not
        return np.asarray(Image.merge(img.mode, [c.resize((W, H), Image.BOX) for c in img.split()])).copy()


class NeRFDataset:
    def __init__(self, opt, device, type="train", downscale=1, n_test=10):
        self.opt = opt
        self.device = device
        self.type = type  # train, val, test, trainval, all
        self.downscale = downscale
        for name in OPT_FIELDS:
            setattr(self, "root_path" if name == "path" else name, _field(opt, name))
        self.training = self.type in ["train", "all", "trainval"]
        self.num_rays = self.num_rays if self.training else -1
        if self.rand_pose >= 0:
            raise NotImplementedError("[NeRFDataset] rand_pose >= 0 is CLIP-guided training on random poses; the CLIP package is not part of this project")

        if os.path.exists(os.path.join(self.root_path, "transforms.json")):
            self.mode = "colmap"   # split by hand, view interpolation for test
        elif os.path.exists(os.path.join(self.root_path, "transforms_train.json")):
            self.mode = "blender"  # provided splits
        else:
            raise NotImplementedError(f"[NeRFDataset] Cannot find transforms*.json under {self.root_path}")

        def load(name):
            with open(os.path.join(self.root_path, name), "r") as f:
                return json.load(f)

        if self.mode == "colmap":
            transform = load("transforms.json")
        elif type == "all":
            transform = None
            for path in sorted(glob.glob(os.path.join(self.root_path, "*.json"))):
                tmp = load(os.path.basename(path))
                if transform is None:
                    transform = tmp
                else:
                    transform["frames"].extend(tmp["frames"])
        elif type == "trainval":
            transform = load("transforms_train.json")
            transform["frames"].extend(load("transforms_val.json")["frames"])
        else:
            transform = load(f"transforms_{type}.json")

        if "h" in transform and "w" in transform:
            self.H = int(transform["h"]) // downscale
            self.W = int(transform["w"]) // downscale
        else:
            self.H = self.W = None  # from the first image
        frames = transform["frames"]

        def ngp(frame):
            return nerf_matrix_to_ngp(np.array(frame["transform_matrix"], dtype=np.float32), scale=self.scale, offset=self.offset)

        if self.mode == "colmap" and type == "test":
            # two random frames and n_test + 1 poses interpolated between them (provider.py:166-182; numpy's global generator, like the reference)
            from scipy.spatial.transform import Rotation, Slerp
            f0, f1 = np.random.choice(frames, 2, replace=False)
            pose0, pose1 = ngp(f0), ngp(f1)
            slerp = Slerp([0, 1], Rotation.from_matrix(np.stack([pose0[:3, :3], pose1[:3, :3]])))
            self.poses, self.images = [], None
            for i in range(n_test + 1):
                ratio = np.sin(((i / n_test) - 0.5) * np.pi) * 0.5 + 0.5
                pose = np.eye(4, dtype=np.float32)
                pose[:3, :3] = slerp(ratio).as_matrix()
                pose[:3, 3] = (1 - ratio) * pose0[:3, 3] + ratio * pose1[:3, 3]
                self.poses.append(pose)
        else:
            if self.mode == "colmap":
                if type == "train":
                    frames = frames[1:]
                elif type == "val":
                    frames = frames[:1]
            self.poses, self.images = [], []
            for f in frames:
                f_path = os.path.join(self.root_path, f["file_path"])
                if self.mode == "blender" and "." not in os.path.basename(f_path):
                    f_path += ".png"
                if not os.path.exists(f_path):  # data sets in the wild list files they do not ship
                    continue
                image = read_image(f_path, None if self.H is None else (self.W, self.H))
                if self.H is None:
                    self.H, self.W = image.shape[0] // downscale, image.shape[1] // downscale
                    if image.shape[:2] != (self.H, self.W):
                        image = read_image(f_path, (self.W, self.H))
                self.poses.append(ngp(f))
                self.images.append(image.astype(np.float32) / 255)

        self.poses = torch.from_numpy(np.stack(self.poses, axis=0))  # [V, 4, 4]
        if self.images is not None:
            self.images = torch.from_numpy(np.stack(self.images, axis=0))  # [V, H, W, C]
            if self.color_space == "linear":
                self.images[..., :3] = srgb_to_linear(self.images[..., :3])
        self.radius = self.poses[:, :3, 3].norm(dim=-1).mean(0).item()

        if self.training and self.error_map:
            self.error_map = torch.ones([self.images.shape[0], 128 * 128], dtype=torch.float, device=self.device)  # fixed resolution (provider.py:236)
        else:
            self.error_map = None
        if self.preload:
            self.poses = self.poses.to(self.device)
            if self.images is not None:
                self.images = self.images.to(self.device)

        if "fl_x" in transform or "fl_y" in transform:
            fl_x = (transform["fl_x"] if "fl_x" in transform else transform["fl_y"]) / downscale
            fl_y = (transform["fl_y"] if "fl_y" in transform else transform["fl_x"]) / downscale
        elif "camera_angle_x" in transform or "camera_angle_y" in transform:  # radians; H / W are already downscaled
            fl_x = self.W / (2 * np.tan(transform["camera_angle_x"] / 2)) if "camera_angle_x" in transform else None
            fl_y = self.H / (2 * np.tan(transform["camera_angle_y"] / 2)) if "camera_angle_y" in transform else None
            if fl_x is None:
                fl_x = fl_y
            if fl_y is None:
                fl_y = fl_x   # a lone camera_angle_x: square pixels
        else:
            raise RuntimeError("Failed to load focal length, please check the transforms.json!")
        cx = (transform["cx"] / downscale) if "cx" in transform else (self.W / 2)
        cy = (transform["cy"] / downscale) if "cy" in transform else (self.H / 2)
        self.intrinsics = np.array([fl_x, fl_y, cx, cy])

    def __len__(self):
        return len(self.poses)

    def collate(self, index):
        """provider.py:277-323 for a list of one view index: {'H', 'W', 'rays_o', 'rays_d'} plus 'images' ([1, N, C] of the sampled pixels when
        training, else [1, H, W, C]) and, with an error map, 'index' and 'inds_coarse'."""
        if len(index) != 1:
            raise RuntimeError("NeRFDataset.collate: one view per batch (dataloader() uses batch_size=1)")
        poses = self.poses[index].to(self.device)  # [1, 4, 4]
        image = None if self.images is None else self.images[index[0]].to(self.device)  # [H, W, C]
        results = {"H": self.H, "W": self.W}
        if self.training:
            error_map = None if self.error_map is None else self.error_map[index]
            rays = get_rays(poses, self.intrinsics, self.H, self.W, self.num_rays, error_map, self.patch_size, image=image)
            if image is not None:
                results["images"] = rays["images"]
            if "inds_coarse" in rays:  # the trainer needs them to update the error map
                results["index"] = index
                results["inds_coarse"] = rays["inds_coarse"]
        else:
            rays = get_rays(poses, self.intrinsics, self.H, self.W, -1)
            if image is not None:
                results["images"] = image[None]
        results["rays_o"], results["rays_d"] = rays["rays_o"], rays["rays_d"]
        return results

    def dataloader(self):
        loader = DataLoader(list(range(len(self.poses))), batch_size=1, collate_fn=self.collate, shuffle=self.training, num_workers=0)
        loader._data = self  # the trainer reads error_map, poses and intrinsics through the loader, like the reference's
        loader.has_gt = self.images is not None
        return loader
