"""The reference's deformed render loop op by op (nerf/renderer.py:755-907), verbatim in structure, on the drop-in ops (near_far_from_aabb /
get_pnts_in_grids / march_rays_quadratic_bending / network / composite_rays / compaction): what rund_cuda takes with perturb, what the parity tests
compare the one-call frame driver with, and the documentation of its semantics."""
import torch

from .. import raymarching
from .utils import get_pnts_in_grids


class DeformedOpsMixin:
    def rund_cuda_ops(self, rays_o, rays_d, dt_gamma=0, bg_color=None, perturb=False, max_steps=1024, T_thresh=1e-2, **kwargs):
        self._refuse_overlays("the op-by-op loop (rund_cuda_ops)")
        dtype = torch.float32
        prefix = rays_o.shape[:-1]
        rays_o = rays_o.contiguous().view(-1, 3)
        rays_d = rays_d.contiguous().view(-1, 3)
        N, device = rays_o.shape[0], rays_o.device
        max_iter_num, hgs, bound = kwargs.get("max_iter_num"), kwargs.get("hash_grid_size"), kwargs.get("bound")
        cut = kwargs.get("cut")
        cut_bounds = torch.tensor(kwargs.get("cut_bounds") or [0.0] * 6, dtype=dtype, device=device)
        p_def, p_ori, F_IP, dF_IP = self._ip_state(device)
        bmin, bmax = p_def.min(axis=0).values, p_def.max(axis=0).values
        if cut:
            bmin = -bound * torch.ones(3, dtype=dtype, device=device)
            bmax = bound * torch.ones(3, dtype=dtype, device=device)
        marg = 1e-3
        bbmin = bmin - marg * torch.ones(3, dtype=dtype, device=device)
        bbmax = bmax + marg * torch.ones(3, dtype=dtype, device=device)
        resolution = torch.ceil((bbmax - bbmin) / hgs).to(torch.int32)
        aabb = torch.cat((bbmin, bbmax), dim=0)
        nears, fars = raymarching.near_far_from_aabb(rays_o, rays_d, aabb, self.min_near)
        if self.bg_radius > 0:  # renderer.py:799-801
            bg_color = self.background(raymarching.sph_from_ray(rays_o, rays_d, self.bg_radius), rays_d)
        elif bg_color is None:
            bg_color = 1
        weights_sum = torch.zeros(N, dtype=dtype, device=device)
        depth = torch.zeros(N, dtype=dtype, device=device)
        image = torch.zeros(N, 3, dtype=dtype, device=device)
        num_seek_IP = kwargs.get("num_seek_IP")
        n_vtx = p_ori.shape[0]
        n_grid = int(resolution[2] * resolution[1] * resolution[0])
        assert p_def.shape == p_ori.shape and n_vtx > 0
        pig_cnt, pig_bgn, pig_idx = get_pnts_in_grids(n_vtx, n_grid, p_def, bbmin, bbmax, hgs, resolution)
        rays_alive = torch.arange(N, dtype=torch.int32, device=device)
        rays_t = nears.clone()
        step, trips, samples = 0, 0, 0
        while step < max_steps:
            n_alive = rays_alive.shape[0]
            if n_alive <= 0:
                break
            n_step = max(min(N // n_alive, 8), 1)
            xyzs, dirs, deltas = raymarching.march_rays_quadratic_bending(
                pig_cnt, pig_bgn, pig_idx, n_vtx, n_grid, p_def, p_ori, F_IP, dF_IP, max_iter_num, bbmin, bbmax, hgs, resolution, num_seek_IP,
                self.IP_dx, cut, cut_bounds, n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, self.bound, self.density_bitfield, self.cascade,
                self.grid_size, nears, fars, 128, perturb if step == 0 else False, dt_gamma, max_steps)
            sigmas, rgbs = self(xyzs, dirs)
            sigmas = self.density_scale * sigmas
            raymarching.composite_rays(n_alive, n_step, rays_alive, rays_t, sigmas, rgbs, deltas, weights_sum, depth, image, T_thresh)
            rays_alive = raymarching.compact_rays(rays_alive)  # == rays_alive[rays_alive >= 0]
            samples += int((deltas[:, 0] != 0).sum())
            step += n_step
            trips += 1
        self.last_stats = dict(trips=trips, samples=samples, err=0, alive_at_exit=int(rays_alive.shape[0]))
        depth_0 = depth
        image = image + (1 - weights_sum).unsqueeze(-1) * bg_color
        depth = torch.clamp(depth - nears, min=0) / (fars - nears)
        return {"depth": depth.view(*prefix), "image": image.view(*prefix, 3), "depth_0": depth_0.view(*prefix), "weights_sum": weights_sum}
