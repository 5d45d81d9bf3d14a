"""Train a NeRF from posed images on disk: the first step of the reference's workflow (``main_train.py``), for the ``nerf.network`` backbone.

    python -m pienerf_amd.main_train --path DATA --workspace WS -O [--iters 30000] [--error_map] [--patch_size 16] [--dataset_type synthetic]
    python -m pienerf_amd.main_train --path DATA --workspace WS -O --test

DATA holds ``transforms.json`` (COLMAP layout) or ``transforms_{train,val,test}.json`` (blender-synthetic layout) and the images they name
(pienerf_amd/nerf/provider.py); ``pienerf_amd.scene.write_blender_dataset`` renders such a directory from the synthetic chair.  Training writes
``WS/checkpoints/ngp_ep%04d.pth`` after every epoch (the last two are kept) — what ``python -m pienerf_amd.main_render --ckpt WS/checkpoints`` loads —
validation images under ``WS/validation`` and, at the end, the point cloud ``WS/points/ngp_{epoch}.ply``.  ``--ckpt latest`` (default) resumes from
the newest checkpoint of the workspace, ``--ckpt scratch`` starts fresh.  ``--test`` loads, evaluates the test split and writes ``WS/meshes``.

Reference: get_opts.py (the shared, training, backbone and data-set groups; defaults and the derived options -O, --dataset_type synthetic,
--patch_size), main_train.py:32-101 (flow).  Validation and test report the PSNR and the SSIM meter (pienerf_amd/metrics.py); ``--ssim_lambda`` puts
an SSIM term into the patch loss.  Not built: --ff, --tcnn, --gui, --clip_text and --rand_pose (refused by name), the LPIPS meter and the patch
branch's LPIPS term, tensorboard, video writing.
"""
import argparse
import os

import numpy as np
import torch

from . import io
from .nerf.provider import NeRFDataset


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--path", type=str)
    ap.add_argument("-O", action="store_true", help="equals --fp16 --cuda_ray --preload")
    ap.add_argument("--test", action="store_true", help="test mode: evaluate the test split and write a mesh")
    ap.add_argument("--workspace", type=str, default="workspace")
    ap.add_argument("--seed", type=int, default=0)
    # training options
    ap.add_argument("--iters", type=int, default=30000, help="training iters")
    ap.add_argument("--lr", type=float, default=1e-2, help="initial learning rate")
    ap.add_argument("--ckpt", type=str, default="latest", help="latest | scratch | a .pth to resume from")
    ap.add_argument("--num_rays", type=int, default=4096, help="rays sampled per image for each training step")
    ap.add_argument("--cuda_ray", action="store_true", help="ray marching on the density grid (the HIP march kernels) instead of the two-pass sampler")
    ap.add_argument("--max_steps", type=int, default=1024, help="max steps sampled per ray (with --cuda_ray)")
    ap.add_argument("--num_steps", type=int, default=512, help="steps sampled per ray (without --cuda_ray)")
    ap.add_argument("--upsample_steps", type=int, default=0, help="steps up-sampled per ray (without --cuda_ray)")
    ap.add_argument("--update_extra_interval", type=int, default=16, help="iter interval of the density-grid update (with --cuda_ray)")
    ap.add_argument("--max_ray_batch", type=int, default=4096, help="batch size of rays at inference (without --cuda_ray)")
    ap.add_argument("--patch_size", type=int, default=1,
                    help="train on square patches of this size (1: off; e.g. 64, 32, 16).  The reference adds an LPIPS term on the patches; its weights are "
                         "not available here: patches train with the MSE term alone, or with --ssim_lambda with a structural (SSIM) term beside it")
    ap.add_argument("--ssim_lambda", type=float, default=0.0,
                    help="weight L in [0, 1] of the patch loss (1 - L) MSE + L (1 - SSIM); needs --patch_size >= 11, the SSIM window.  0: off")
    ap.add_argument("--T_thresh", type=float, default=1e-2, help="stop marching a ray when its transmittance falls below this")
    # network backbone options
    ap.add_argument("--fp16", action="store_true", help="amp mixed precision training")
    ap.add_argument("--ff", action="store_true", help="[refused] fully-fused MLP backbone")
    ap.add_argument("--tcnn", action="store_true", help="[refused] TCNN backbone")
    # data-set options
    ap.add_argument("--color_space", type=str, default="srgb", help="linear | srgb")
    ap.add_argument("--preload", action="store_true", help="keep all images on the GPU")
    ap.add_argument("--bound", type=float, default=2.0, help="the scene lies in [-bound, bound]^3")
    ap.add_argument("--scale", type=float, default=0.33, help="scale of the camera positions into the box")
    ap.add_argument("--offset", type=float, nargs="*", default=[0, 0, 0], help="offset of the camera positions")
    ap.add_argument("--dt_gamma", type=float, default=1 / 128, help="adaptive ray marching step growth; 0 disables")
    ap.add_argument("--min_near", type=float, default=0.2, help="minimum near distance of a camera")
    ap.add_argument("--density_thresh", type=float, default=10, help="density above which a grid cell counts as occupied")
    ap.add_argument("--bg_radius", type=float, default=-1, help="> 0: a background model on the sphere of this radius")
    ap.add_argument("--dataset_type", type=str, default="", help="synthetic: scale 0.8, bound 1, dt_gamma 0 (the blender-synthetic scenes)")
    # experimental
    ap.add_argument("--error_map", action="store_true", help="sample the rays of a step by the training error (a 128 x 128 map per view)")
    ap.add_argument("--gui", action="store_true", help="[refused] the GUI's training mode")
    ap.add_argument("--clip_text", type=str, default="", help="[refused] CLIP guidance")
    ap.add_argument("--rand_pose", type=int, default=-1, help="[refused unless < 0] random poses for CLIP guidance")
    # this front end's own
    ap.add_argument("--eval_interval", type=int, default=50, help="validate every this many epochs (the reference's main_train.py fixes 50)")
    ap.add_argument("--resolution", type=int, default=256, help="lattice resolution of the final point cloud / the --test mesh")
    ap.add_argument("--con", dest="components", type=int, default=0, help="keep this many largest connected components of the density field in the final point cloud / the "
                    "--test mesh; 0 (default) keeps all.  The reference declares --con with default 1 and never reads it, so off is the faithful default")
    ap.add_argument("--trust-ckpt", dest="trust_ckpt", action="store_true", help="allow a checkpoint that needs arbitrary pickle globals")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--quiet", action="store_true")
    return ap


def derive(opt):
    """The derived options of get_opts.py:100-115, and the refusals."""
    if opt.dataset_type == "synthetic":
        opt.scale, opt.bound, opt.dt_gamma = 0.8, 1.0, 0.0
    if opt.O:
        opt.fp16 = opt.cuda_ray = opt.preload = True
    if opt.patch_size > 1:
        opt.error_map = False  # patches ignore the error map
        if opt.num_rays % (opt.patch_size ** 2) != 0:
            raise SystemExit("--patch_size: its square must divide --num_rays")
    if not 0.0 <= opt.ssim_lambda <= 1.0:
        raise SystemExit("--ssim_lambda: a weight in [0, 1]")
    if opt.ssim_lambda > 0 and opt.patch_size < 11:
        raise SystemExit("--ssim_lambda > 0 needs --patch_size >= 11: SSIM's 11 x 11 window has to fit into a patch")
    for flag, what in (("ff", "--ff (fully-fused MLP backbone)"), ("tcnn", "--tcnn (TCNN backbone)"), ("gui", "--gui (training inside the GUI)")):
        if getattr(opt, flag):
            raise SystemExit(f"{what} is not part of this project: the nerf.network backbone trains headless")
    if opt.clip_text:
        raise SystemExit("--clip_text (CLIP guidance) is not part of this project")
    if opt.rand_pose >= 0:
        raise SystemExit("--rand_pose >= 0 (random poses for CLIP guidance) is not part of this project")
    return opt


def parse(argv=None):
    return derive(parser().parse_args(argv))


def build(opt):
    """main_train.py:32-42,69-79: seed, model and trainer of an option namespace (``parse``); ``--ckpt`` is applied."""
    from .nerf.network import NeRFNetwork
    from .training import Trainer
    torch.manual_seed(opt.seed)   # seed_everything (nerf/utils.py:141-145)
    np.random.seed(opt.seed)
    model = NeRFNetwork(encoding="hashgrid", bound=opt.bound, cuda_ray=opt.cuda_ray, density_scale=1, min_near=opt.min_near,
                        density_thresh=opt.density_thresh, bg_radius=opt.bg_radius).to(opt.device)
    trainer = Trainer(model, vars(opt), lr=opt.lr, iters=opt.iters, update_extra_interval=opt.update_extra_interval, num_rays=opt.num_rays,
                      ema_decay=None if opt.test else 0.95, fp16=opt.fp16, eval_interval=opt.eval_interval)
    trainer.workspace = opt.workspace
    if opt.ckpt == "latest":
        path = io.latest_checkpoint(trainer.checkpoint_dir())
        if path is None and opt.test:
            raise SystemExit(f"--test: no checkpoint under {trainer.checkpoint_dir()}")
    else:
        path = None if opt.ckpt == "scratch" else opt.ckpt
    if path is not None:
        trainer.resume(path, allow_pickle=opt.trust_ckpt)
    return model, trainer


def run(opt):
    """main_train.py:50-101.  Returns what happened: the trainer, the epoch / global_step it started from, the per-step losses, the last validation
    and the test result ({'loss', 'psnr', 'ssim'} or None) and the files written."""
    if not opt.path:
        raise SystemExit("--path: the data set directory (transforms*.json)")
    say = (lambda *a: None) if opt.quiet else print
    model, trainer = build(opt)
    res = dict(trainer=trainer, start_epoch=trainer.epoch, start_step=trainer.global_step, losses=[], valid=None, test=None, point_cloud=None, mesh=None)
    if opt.test:
        test_loader = NeRFDataset(opt, device=opt.device, type="test").dataloader()
        if test_loader.has_gt:
            res["test"] = trainer.evaluate_loader(test_loader)
            say(f"test: {res['test']}")
        res["mesh"] = os.path.join(opt.workspace, "meshes", f"{trainer.name}_{trainer.epoch}.ply")
        trainer.save_mesh(res["mesh"], resolution=opt.resolution, threshold=10, components=opt.components)
        return res
    train_loader = NeRFDataset(opt, device=opt.device, type="train").dataloader()
    valid_loader = NeRFDataset(opt, device=opt.device, type="val", downscale=1).dataloader()
    max_epoch = int(np.ceil(opt.iters / len(train_loader)))
    say(f"{len(train_loader)} training views, epochs {trainer.epoch + 1}..{max_epoch}, workspace {opt.workspace}")
    res["losses"] = trainer.fit(train_loader, valid_loader, max_epoch, opt.workspace)
    if res["losses"]:
        say(f"loss {np.mean(res['losses'][:5]):.5f} -> {np.mean(res['losses'][-20:]):.5f} over {len(res['losses'])} steps")
    if trainer.stats["valid_loss"]:
        res["valid"] = {"loss": trainer.stats["valid_loss"][-1], "psnr": trainer.stats["results"][-1],
                        "ssim": trainer.valid_result["ssim"] if trainer.valid_result else None}   # None: no validation in this run (resumed stats)
        say(f"validation: {res['valid']}")
    test_loader = NeRFDataset(opt, device=opt.device, type="test").dataloader()
    if test_loader.has_gt:   # blender sets have test images, COLMAP's interpolated test poses do not
        res["test"] = trainer.evaluate_loader(test_loader)
        say(f"test: {res['test']}")
    res["point_cloud"] = os.path.join(opt.workspace, "points", f"{trainer.name}_{trainer.epoch}.ply")
    trainer.save_point_cloud(res["point_cloud"], resolution=opt.resolution, threshold=10, components=opt.components)
    return res


if __name__ == "__main__":
    run(parse())
