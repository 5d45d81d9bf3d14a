"""Headless training loop on the HIP ops — what ``main_train.py`` + ``Trainer.train_step / train_one_epoch`` do for
the ``-O`` (cuda_ray) configuration, without the dataset / GUI / tensorboard baggage.

Reference: main_train.py:60-80 (Adam(get_params(lr), betas=(0.9, 0.99), eps=1e-15), LambdaLR 0.1^(iter/iters), MSE), nerf/trainer.py:158-207
(train_step: render(..., perturb=True, force_all_rays=False), per-ray MSE), :604-667 (train_one_epoch: update_extra_state every
``update_extra_interval`` steps, zero_grad / backward / step / scheduler per step).  Data comes as posed images already on the device
(there is no dataset on the box): ``RayImageSet`` samples ``num_rays`` random pixels of a random view per step like
nerf/provider.py's training collate (one view per batch, rays drawn uniformly, :270-300).

Training from images on disk (``pienerf_amd.main_train``): ``Trainer.fit`` runs epochs over a ``NeRFDataset`` loader (nerf/provider.py), writes the
per-epoch checkpoints ``main_render --ckpt`` looks for and evaluates on a second loader; ``Trainer.evaluate_loader`` is the reference's
``evaluate_one_epoch``.  Reference: nerf/trainer.py:224-246 (error map), :382-406 (train), :689-792 (evaluate_one_epoch), :794-830 (save_checkpoint).
"""
import os

import numpy as np
import torch

from . import io, metrics
from .nerf.utils import error_map_update, extract_geometry, get_rays, write_to_ply


class RayImageSet:
    """Posed RGB(A) images [V, H, W, C] resident on the device; ``batch(num_rays)`` -> rays + target colours of one random view."""

    def __init__(self, poses, intrinsics, images, generator=None):
        self.poses = poses.to(torch.float32)                # [V, 4, 4] cam2world
        self.intrinsics = intrinsics                        # (fx, fy, cx, cy)
        self.images = images.to(torch.float32)              # [V, H, W, 3 or 4]
        self.V, self.H, self.W = images.shape[:3]
        self.gen = generator

    def batch(self, num_rays):
        dev = self.images.device
        v = int(torch.randint(0, self.V, (1,), generator=self.gen, device="cpu"))
        rays = get_rays(self.poses[v:v + 1], self.intrinsics, self.H, self.W)          # the full view, then a random subset of pixels
        inds = torch.randint(0, self.H * self.W, (num_rays,), generator=self.gen, device="cpu").to(dev)
        return {"rays_o": rays["rays_o"][:, inds], "rays_d": rays["rays_d"][:, inds], "images": self.images[v].reshape(1, -1, self.images.shape[-1])[:, inds],
                "index": v}


class ParamEMA:
    """Exponential moving average of the trainable parameters with torch_ema's interface subset the reference uses (trainer.py:86-89,
    643-644, 751-753, 789-790: update / store / copy_to / restore / state_dict), including torch_ema's warm-up of the decay,
    min(decay, (1 + n) / (10 + n))."""

    def __init__(self, parameters, decay=0.95):
        self.decay, self.num_updates = float(decay), 0
        self.params = [p for p in parameters if p.requires_grad]
        self.shadow = [p.detach().clone() for p in self.params]
        self.stored = None

    @torch.no_grad()
    def update(self):
        self.num_updates += 1
        d = min(self.decay, (1 + self.num_updates) / (10 + self.num_updates))
        for s, p in zip(self.shadow, self.params):
            s.sub_((1.0 - d) * (s - p))

    @torch.no_grad()
    def store(self):
        self.stored = [p.detach().clone() for p in self.params]

    @torch.no_grad()
    def copy_to(self):
        for s, p in zip(self.shadow, self.params):
            p.copy_(s)

    @torch.no_grad()
    def restore(self):
        for s, p in zip(self.stored, self.params):
            p.copy_(s)
        self.stored = None

    def state_dict(self):
        return {"decay": self.decay, "num_updates": self.num_updates, "shadow_params": [s.clone() for s in self.shadow], "collected_params": None}

    def load_state_dict(self, sd):
        self.decay, self.num_updates = float(sd["decay"]), int(sd["num_updates"])
        for s, v in zip(self.shadow, sd["shadow_params"]):
            s.copy_(v.to(s.device))


class _LoaderFeed:
    """One pass over a data loader behind ``RayImageSet``'s ``batch`` interface: Trainer.fit runs its epochs through Trainer.train."""

    def __init__(self, loader):
        self.batches = iter(loader)

    def batch(self, num_rays):  # the loader's data set has sampled its own num_rays
        return next(self.batches)


class Trainer:
    def __init__(self, model, opt, lr=1e-2, iters=30000, update_extra_interval=16, num_rays=4096, ema_decay=None, fp16=False, name="ngp",
                 eval_interval=50, max_keep_ckpt=2):
        """opt: the render options of a step (dt_gamma, max_steps, T_thresh, ...) and, for ``fit`` / ``evaluate_loader``, ``color_space``,
        ``patch_size`` and ``ssim_lambda`` (``train_step``).  name, eval_interval, max_keep_ckpt: trainer.py:17-31, used by ``fit``.
        ema_decay: main_train.py:78 passes 0.95; None (default) trains without an average, like Trainer's own default (trainer.py:19).
        fp16 (trainer.py:20,84: ``--fp16``): the steps run under autocast with a GradScaler — half hash tables, half nn.Linear, and the half
        scatter-add of the grid's backward (gridencoder.cu:324-331)."""
        self.model, self.opt = model, dict(opt)
        self.fp16 = bool(fp16)
        self.scaler = torch.amp.GradScaler("cuda", enabled=self.fp16)   # trainer.py:84
        self.optimizer = torch.optim.Adam(model.get_params(lr), betas=(0.9, 0.99), eps=1e-15)
        self.lr_scheduler = torch.optim.lr_scheduler.LambdaLR(self.optimizer, lambda it: 0.1 ** min(it / iters, 1))
        self.criterion = torch.nn.MSELoss(reduction="none")
        self.update_extra_interval, self.num_rays = update_extra_interval, num_rays
        self.global_step = 0
        self.ema = ParamEMA(model.parameters(), ema_decay) if ema_decay is not None else None
        self.name, self.eval_interval, self.max_keep_ckpt = name, int(eval_interval), int(max_keep_ckpt)
        self.epoch, self.workspace, self.error_map = 0, None, None   # error_map: the data set's, set by fit (trainer.py:391)
        self.stats = {"loss": [], "valid_loss": [], "results": [], "checkpoints": [], "best_result": None}   # trainer.py:92-98
        self.valid_result = None   # what fit's last validation returned (evaluate_loader)

    def _render_opts(self):
        keep = ("dt_gamma", "max_steps", "T_thresh", "num_steps", "upsample_steps")   # the last two: the sampler of a model without cuda_ray (get_opts.py:19-22)
        return {k: self.opt[k] for k in keep if k in self.opt}

    def train_step(self, data):
        """trainer.py:158-207 (the image-supervised branch).  opt['ssim_lambda'] = L > 0 with opt['patch_size'] >= 11: the loss is
        (1 - L) MSE + L (1 - ssim(patches, data_range=1)), the structural term standing where the reference's patch branch has its LPIPS term (:218)."""
        images = data["images"]
        C = images.shape[-1]
        if C == 4 and not self.model.bg_radius > 0:  # random per-pixel background under the alpha matte (trainer.py:186-196); not with a background model
            bg_color = torch.rand_like(images[..., :3])
            gt_rgb = images[..., :3] * images[..., 3:] + bg_color * (1 - images[..., 3:])
            bg = bg_color.view(-1, 3)
        elif C == 4:  # background model: the matte is composited over 1, the render's background is the model's whatever is passed (renderer.py:283-288)
            bg, gt_rgb = 1, images[..., :3] * images[..., 3:] + (1 - images[..., 3:])
        else:
            bg, gt_rgb = 1, images
        patch = int(self.opt.get("patch_size", 1))
        all_rays = patch != 1   # patches are rendered whole (trainer.py:201); their LPIPS term (:218) is not built
        outputs = self.model.render(data["rays_o"], data["rays_d"], staged=False, bg_color=bg, perturb=True, force_all_rays=all_rays, **self._render_opts())
        pred_rgb = outputs["image"]
        loss = self.criterion(pred_rgb, gt_rgb).mean(-1)   # per ray [1, N]
        if self.error_map is not None and "inds_coarse" in data:   # trainer.py:224-246: the sampled cells' moving average of the per-ray loss
            error_map_update(self.error_map[int(data["index"][0])], data["inds_coarse"], loss)
        loss = loss.mean()
        lam = float(self.opt.get("ssim_lambda", 0) or 0)
        if lam > 0 and patch >= metrics.WINDOW:
            # get_rays' patch batches are patch-major, then patch row, then patch column: [1, N, 3] is [N / p^2, p, p, 3]
            loss = (1 - lam) * loss + lam * (1 - metrics.ssim(pred_rgb.reshape(-1, patch, patch, 3), gt_rgb.reshape(-1, patch, patch, 3), data_range=1.0))
        return pred_rgb, gt_rgb, loss

    def train(self, dataset, steps):
        """``steps`` iterations of trainer.py:625-645; returns the per-step losses."""
        self.model.train()
        losses = []
        for _ in range(steps):
            if self.model.cuda_ray and self.global_step % self.update_extra_interval == 0:
                with torch.autocast("cuda", dtype=torch.float16, enabled=self.fp16):   # trainer.py:629
                    self.model.update_extra_state()
            self.global_step += 1
            self.optimizer.zero_grad()
            with torch.autocast("cuda", dtype=torch.float16, enabled=self.fp16):       # trainer.py:637
                _, _, loss = self.train_step(dataset.batch(self.num_rays))
            self.scaler.scale(loss).backward()                                         # trainer.py:640-642
            self.scaler.step(self.optimizer)
            self.scaler.update()
            self.lr_scheduler.step()
            if self.ema is not None:  # trainer.py:643-644
                self.ema.update()
            losses.append(float(loss.detach()))
        return losses

    @torch.no_grad()
    def evaluate(self, dataset, view):
        """Full-image PSNR of one view (eval() mode: the inference loop of run_cuda)."""
        self.model.eval()
        if self.ema is not None:  # evaluation runs on the averaged weights (trainer.py:751-753, 789-790)
            self.ema.store()
            self.ema.copy_to()
        rays = get_rays(dataset.poses[view:view + 1], dataset.intrinsics, dataset.H, dataset.W)
        out = self.model.render(rays["rays_o"], rays["rays_d"], bg_color=1, perturb=False, **self._render_opts())
        if self.ema is not None:
            self.ema.restore()
        img = dataset.images[view]
        gt = img[..., :3] * img[..., 3:] + (1 - img[..., 3:]) if img.shape[-1] == 4 else img
        mse = torch.mean((out["image"].view(dataset.H, dataset.W, 3) - gt) ** 2)
        return float(-10 * torch.log10(mse)), out

    # ------------------------------------------------------------------ epochs over a data loader (trainer.py:382-406)
    def checkpoint_dir(self, workspace=None):
        return os.path.join(workspace if workspace is not None else self.workspace, "checkpoints")

    def save_checkpoint(self, workspace=None):
        """trainer.py:794-830 (full=True, best=False, remove_old=True): ``checkpoints/{name}_ep%04d.pth`` with the optimiser, scheduler, scaler and
        EMA state; the oldest file beyond ``max_keep_ckpt`` is removed."""
        path = os.path.join(self.checkpoint_dir(workspace), f"{self.name}_ep{self.epoch:04d}.pth")
        self.stats["checkpoints"].append(path)
        if len(self.stats["checkpoints"]) > self.max_keep_ckpt:
            old = self.stats["checkpoints"].pop(0)
            if os.path.exists(old):
                os.remove(old)
        return io.save_checkpoint(self.model, path, epoch=self.epoch, global_step=self.global_step, stats=self.stats, optimizer=self.optimizer,
                                  lr_scheduler=self.lr_scheduler, full=True, ema=self.ema, scaler=self.scaler)

    def resume(self, path, allow_pickle=False):
        """trainer.py:856-916 (model_only=False): model, optimiser, scheduler, scaler, EMA, epoch, global_step and stats of a full checkpoint."""
        info = io.load_checkpoint(self.model, path, model_only=False, optimizer=self.optimizer, lr_scheduler=self.lr_scheduler, ema=self.ema,
                                  scaler=self.scaler, allow_pickle=allow_pickle)
        if info["epoch"] is not None:
            self.epoch = int(info["epoch"])
        if info["global_step"] is not None:
            self.global_step = int(info["global_step"])
        if isinstance(info.get("stats"), dict):
            self.stats.update(info["stats"])
        return info

    def fit(self, train_loader, valid_loader, max_epochs, workspace):
        """Trainer.train of the reference (trainer.py:382-406): the density cells no training camera sees are marked, then per epoch one pass over
        ``train_loader`` through ``train``'s step code, a full checkpoint, and every ``eval_interval`` epochs ``evaluate_loader(valid_loader)``.
        Starts behind ``self.epoch`` (``resume``).  Returns the per-step losses of the epochs it ran."""
        self.workspace = workspace
        data = train_loader._data
        if self.model.cuda_ray:
            self.model.mark_untrained_grid(data.poses, data.intrinsics)
        self.error_map = data.error_map
        losses = []
        for epoch in range(self.epoch + 1, int(max_epochs) + 1):
            self.epoch = epoch
            epoch_losses = self.train(_LoaderFeed(train_loader), len(train_loader))
            self.stats["loss"].append(sum(epoch_losses) / max(len(epoch_losses), 1))
            losses += epoch_losses
            self.save_checkpoint()
            if self.epoch % self.eval_interval == 0 and valid_loader is not None:
                self.valid_result = self.evaluate_loader(valid_loader)
        return losses

    @torch.no_grad()
    def evaluate_loader(self, loader, name=None):
        """evaluate_one_epoch (trainer.py:689-792) with the PSNR meter: every view of ``loader`` rendered in eval() mode on the averaged weights against
        its ground truth over white; the predictions go to ``{workspace}/validation/{name}_{i:04d}.png`` (through linear_to_srgb when the colour space
        is linear).  Returns {'loss': mean MSE, 'psnr': mean PSNR, 'ssim': mean SSIM} and records the first two in stats['valid_loss'] /
        stats['results'].  'ssim' is the SSIMMeter's (metrics.ssim with data_range=None per view, summed on the device and read once at the end);
        None when a view is smaller than the 11 x 11 window."""
        name = name if name is not None else f"{self.name}_ep{self.epoch:04d}"
        self.model.eval()
        if self.ema is not None:
            self.ema.store()
            self.ema.copy_to()
        total_loss, total_psnr, n = 0.0, 0.0, 0
        ssim_meter = metrics.SSIMMeter(device=next(self.model.parameters()).device)
        for data in loader:
            n += 1
            images = data["images"]   # [1, H, W, C]
            H, W = images.shape[1:3]
            gt = images[..., :3] * images[..., 3:] + (1 - images[..., 3:]) if images.shape[-1] == 4 else images
            with torch.autocast("cuda", dtype=torch.float16, enabled=self.fp16):   # trainer.py:716
                out = self.model.render(data["rays_o"], data["rays_d"], staged=True, bg_color=1, perturb=False, **self._render_opts())
            pred = out["image"].reshape(1, H, W, 3).to(torch.float32)
            mse = float(torch.mean((pred - gt) ** 2))
            total_loss += mse
            total_psnr += -10 * float(np.log10(mse))   # PSNRMeter (nerf/utils.py:249-256)
            if ssim_meter is not None and min(H, W) >= metrics.WINDOW:
                ssim_meter.update(pred, gt)
            else:
                ssim_meter = None
            if self.workspace is not None:
                shown = io.linear_to_srgb(pred) if self.opt.get("color_space", "srgb") == "linear" else pred
                io.save_image(shown[0], os.path.join(self.workspace, "validation", f"{name}_{n:04d}.png"), W, H)
        if self.ema is not None:
            self.ema.restore()
        result = {"loss": total_loss / max(n, 1), "psnr": total_psnr / max(n, 1), "ssim": ssim_meter.measure() if ssim_meter is not None and n else None}
        self.stats["valid_loss"].append(result["loss"])
        self.stats["results"].append(result["psnr"])
        return result

    def _geometry(self, resolution, threshold, components=0):
        from .mesh import density_query
        m = self.model
        return extract_geometry(m.aabb_infer[:3], m.aabb_infer[3:], resolution=resolution, threshold=threshold, query_func=density_query(m, self.fp16),
                                components=components)

    def save_mesh(self, save_path, resolution=256, threshold=10, components=0):
        """trainer.py:331-354: the `threshold` level set of model.density(pts)['sigma'] (no_grad, autocast(enabled=fp16)) on the resolution^3 lattice
        over aabb_infer, meshed on the device, written as a binary PLY (scene.write_mesh_ply).  `save_path` is required: this Trainer has no workspace
        or epoch to name a default file after.  components > 0: only that many largest connected components of the above-threshold nodes are meshed
        (extract_geometry); 0 meshes everything, floaters included."""
        from .scene import write_mesh_ply
        d = os.path.dirname(save_path)
        if d:
            os.makedirs(d, exist_ok=True)
        vertices, triangles = self._geometry(resolution, threshold, components)
        write_mesh_ply(save_path, vertices, triangles)
        return vertices, triangles

    def save_point_cloud(self, save_path, resolution=256, threshold=10, components=0):
        """trainer.py:356-378: the vertices of save_mesh's surface (`components` as there) as an ASCII PLY (write_to_ply).  `save_path` is required
        (no workspace / epoch)."""
        d = os.path.dirname(save_path)
        if d:
            os.makedirs(d, exist_ok=True)
        cloud, _ = self._geometry(resolution, threshold, components)
        write_to_ply(cloud, save_path)
        return cloud
