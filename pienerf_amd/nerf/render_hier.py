"""Hierarchical sampling without a density grid (nerf/renderer.py:19-53, 137-265, 552-585 of the reference): sample_pdf, NeRFRenderer.run with its
one-launch form (pn_render_hier) and its op sequence, and render's staging."""
import ctypes as C

import torch

from .. import raymarching
from .._lib import check, lib, ptr, require_gpu, stream_ptr
from ._outputs import flat_rays, frame_outputs


def sample_pdf(bins, weights, n_samples, det=False):
    """nerf/renderer.py:19-53 (the original NeRF's inverse-CDF sampling), torch ops on whatever device the inputs live on.
    bins [B, T] (the old z values), weights [B, T - 1] (bin weights) -> [B, n_samples] new z values; det: the midpoints of n_samples equal
    slices of [0, 1] instead of uniform random numbers."""
    if weights.shape[-1] < 1:
        raise RuntimeError("sample_pdf: no bin weights (the hierarchical sampler needs num_steps >= 3: weights[:, 1:-1] is empty)")
    weights = weights + 1e-5  # prevent nans
    pdf = weights / torch.sum(weights, -1, keepdim=True)
    cdf = torch.cumsum(pdf, -1)
    cdf = torch.cat([torch.zeros_like(cdf[..., :1]), cdf], -1)
    if det:
        u = torch.linspace(0. + 0.5 / n_samples, 1. - 0.5 / n_samples, steps=n_samples).to(weights.device)
        u = u.expand(list(cdf.shape[:-1]) + [n_samples])
    else:
        u = torch.rand(list(cdf.shape[:-1]) + [n_samples]).to(weights.device)
    u = u.contiguous()
    inds = torch.searchsorted(cdf, u, right=True)
    below = torch.clamp(inds - 1, min=0)
    above = torch.clamp(inds, max=cdf.shape[-1] - 1)
    cdf_lo, cdf_hi = torch.gather(cdf, -1, below), torch.gather(cdf, -1, above)
    bins_lo, bins_hi = torch.gather(bins, -1, below), torch.gather(bins, -1, above)
    denom = cdf_hi - cdf_lo
    denom = torch.where(denom < 1e-5, torch.ones_like(denom), denom)
    t = (u - cdf_lo) / denom
    return bins_lo + t * (bins_hi - bins_lo)


class HierRenderMixin:
    def render(self, rays_o, rays_d, staged=False, max_ray_batch=4096, **kwargs):
        """renderer.py:552-585.  cuda_ray never stages.  Without cuda_ray the rays go through ``run``: staged, in batches of max_ray_batch with only
        depth and image returned (:565-580), otherwise in one call with weights_sum as well.  When ``run`` would take its fused form a staged call is
        served in one piece — that form has no [N, T, ...] intermediates to bound, and its per-ray results do not depend on how the rays are batched."""
        if self.cuda_ray:
            return self.run_cuda(rays_o, rays_d, **kwargs)
        if not staged:
            return self.run(rays_o, rays_d, **kwargs)
        if self._hier_fused_ok(rays_o, **kwargs):
            out = self.run(rays_o, rays_d, **kwargs)
            return {"depth": out["depth"], "image": out["image"]}
        B, N = rays_o.shape[:2]
        depth = torch.empty((B, N), device=rays_o.device)
        image = torch.empty((B, N, 3), device=rays_o.device)
        for b in range(B):
            for head in range(0, N, max_ray_batch):
                tail = min(head + max_ray_batch, N)
                part = self.run(rays_o[b:b + 1, head:tail], rays_d[b:b + 1, head:tail], **kwargs)
                depth[b:b + 1, head:tail] = part["depth"]
                image[b:b + 1, head:tail] = part["image"]
        return {"depth": depth, "image": image}

    @staticmethod
    def _check_hier_steps(num_steps, upsample_steps):
        if int(num_steps) < 1 or int(upsample_steps) < 0:
            raise RuntimeError(f"run: num_steps = {num_steps}, upsample_steps = {upsample_steps}")
        if int(upsample_steps) > 0 and int(num_steps) < 3:
            raise RuntimeError(f"run: upsample_steps = {upsample_steps} needs num_steps >= 3 (got {num_steps}): sample_pdf is handed weights[:, 1:-1], "
                               "which is empty, and the reference fails inside it")

    def _hier_fused_ok(self, rays_o, num_steps=128, upsample_steps=128, bg_color=None, perturb=False, **kwargs):
        """Whether ``run`` takes the fused launch for these arguments (see its docstring)."""
        if self.training or perturb or torch.is_grad_enabled() or self._autocast_half():
            return False
        if int(num_steps) + int(upsample_steps) > int(lib().pn_hier_max_samples()):
            return False
        if self.bg_radius > 0 or not torch.is_tensor(bg_color):
            return True
        n = rays_o.numel() // 3   # one colour [3] or one per ray [N, 3]; any other shape is left to torch's broadcasting in the op sequence
        return tuple(bg_color.shape) in ((3,), (n, 3))

    def run(self, rays_o, rays_d, num_steps=128, upsample_steps=128, bg_color=None, perturb=False, **kwargs):
        """NeRFRenderer.run (nerf/renderer.py:137-265) -> {'depth', 'image', 'weights_sum'}: num_steps stratified samples per ray, a density query,
        upsample_steps samples drawn from the resulting weights, a second density query, the merge, a colour query on the samples whose weight exceeds
        1e-4, and the sums.

        eval() under no_grad, without perturb:  ONE launch (pn_render_hier: a wave per ray, the sample set in LDS), then the background model's blend
                  when bg_radius > 0.  Takes a background of None / a scalar / one colour [3] / one colour per ray [N, 3].
        otherwise (train() mode, autograd recording, perturb, fp16 autocast — there is no half form of the launch —, or
                  num_steps + upsample_steps beyond the launch's LDS-resident limit, pn_hier_max_samples() = 512):  ``run_ops``."""
        self._refuse_overlays("the hierarchical render (run)")
        self._check_hier_steps(num_steps, upsample_steps)
        if self._hier_fused_ok(rays_o, num_steps, upsample_steps, bg_color, perturb):
            return self._run_hier_fused(rays_o, rays_d, int(num_steps), int(upsample_steps), bg_color)
        return self.run_ops(rays_o, rays_d, num_steps, upsample_steps, bg_color, perturb, **kwargs)

    def _run_hier_fused(self, rays_o, rays_d, num_steps, upsample_steps, bg_color):
        prefix = rays_o.shape[:-1]
        rays_o, rays_d = flat_rays(rays_o, rays_d)
        require_gpu(rays_o, rays_d)
        N, device = rays_o.shape[0], rays_o.device
        bg_rays, bg_scalar = None, 1.0
        if self.bg_radius > 0:
            bg_scalar = 0.0   # renderer.py:244-247: the model's colour, blended in below
        elif torch.is_tensor(bg_color):
            bg_rays = bg_color.to(device=device, dtype=torch.float32).expand(N, 3).contiguous()
        elif bg_color is not None:
            bg_scalar = float(bg_color)
        image, depth, _, ws = frame_outputs(N, device)   # (this form has no depth_0)
        aabb = (C.c_float * 6)(*self._aabb_infer_host())
        check(lib().pn_render_hier(self._net_handle(), ptr(rays_o), ptr(rays_d), N, aabb, float(self.min_near), num_steps, upsample_steps,
                                   float(self.density_scale), bg_scalar, ptr(bg_rays), ptr(image), ptr(depth), ptr(ws), 0, stream_ptr()), "render_hier")
        if self.bg_radius > 0 and N > 0:
            self.blend_background(rays_o, rays_d, ws, image)
        return {"depth": depth.view(*prefix), "image": image.view(*prefix, 3), "weights_sum": ws}

    def run_ops(self, rays_o, rays_d, num_steps=128, upsample_steps=128, bg_color=None, perturb=False, **kwargs):
        """``run`` as the reference's op sequence on near_far_from_aabb / density / color / sample_pdf and torch ops: differentiable (the training
        branch), with perturb, under autocast, with any background; the parity tests pin it against the reference's own run."""
        self._refuse_overlays("the hierarchical render (run_ops)")
        self._check_hier_steps(num_steps, upsample_steps)
        prefix = rays_o.shape[:-1]
        rays_o = rays_o.contiguous().view(-1, 3)
        rays_d = rays_d.contiguous().view(-1, 3)
        require_gpu(rays_o, rays_d)
        N, device = rays_o.shape[0], rays_o.device
        aabb = self.aabb_train if self.training else self.aabb_infer
        nears, fars = raymarching.near_far_from_aabb(rays_o, rays_d, aabb, self.min_near)
        nears, fars = nears.unsqueeze(-1), fars.unsqueeze(-1)
        z_vals = torch.linspace(0.0, 1.0, num_steps, device=device).unsqueeze(0).expand((N, num_steps))
        z_vals = nears + (fars - nears) * z_vals
        sample_dist = (fars - nears) / num_steps
        if perturb:
            z_vals = z_vals + (torch.rand(z_vals.shape, device=device) - 0.5) * sample_dist   # unclamped, as in the reference
        xyzs = rays_o.unsqueeze(-2) + rays_d.unsqueeze(-2) * z_vals.unsqueeze(-1)
        xyzs = torch.min(torch.max(xyzs, aabb[:3]), aabb[3:])

        def weights_of(z, sigma):
            deltas = z[..., 1:] - z[..., :-1]
            deltas = torch.cat([deltas, sample_dist * torch.ones_like(deltas[..., :1])], dim=-1)   # the last one is sample_dist, also after the merge
            alphas = 1 - torch.exp(-deltas * self.density_scale * sigma)
            shifted = torch.cat([torch.ones_like(alphas[..., :1]), 1 - alphas + 1e-15], dim=-1)
            return deltas, alphas * torch.cumprod(shifted, dim=-1)[..., :-1]

        dens = {k: v.view(N, num_steps, -1) for k, v in self.density(xyzs.reshape(-1, 3)).items()}
        if upsample_steps > 0:
            with torch.no_grad():
                deltas, weights = weights_of(z_vals, dens["sigma"].squeeze(-1))
                z_mid = z_vals[..., :-1] + 0.5 * deltas[..., :-1]
                new_z = sample_pdf(z_mid, weights[:, 1:-1], upsample_steps, det=not self.training).detach()
                new_xyzs = rays_o.unsqueeze(-2) + rays_d.unsqueeze(-2) * new_z.unsqueeze(-1)
                new_xyzs = torch.min(torch.max(new_xyzs, aabb[:3]), aabb[3:])
            new_dens = {k: v.view(N, upsample_steps, -1) for k, v in self.density(new_xyzs.reshape(-1, 3)).items()}   # only the new points
            z_vals, z_index = torch.sort(torch.cat([z_vals, new_z], dim=1), dim=1)
            xyzs = torch.cat([xyzs, new_xyzs], dim=1)
            xyzs = torch.gather(xyzs, dim=1, index=z_index.unsqueeze(-1).expand_as(xyzs))
            for k in dens:
                both = torch.cat([dens[k], new_dens[k]], dim=1)
                dens[k] = torch.gather(both, dim=1, index=z_index.unsqueeze(-1).expand_as(both))
        _, weights = weights_of(z_vals, dens["sigma"].squeeze(-1))
        dirs = rays_d.view(-1, 1, 3).expand_as(xyzs)
        dens = {k: v.reshape(-1, v.shape[-1]) for k, v in dens.items()}
        mask = weights > 1e-4  # hard coded in the reference
        rgbs = self.color(xyzs.reshape(-1, 3), dirs.reshape(-1, 3), mask=mask.reshape(-1), **dens).view(N, -1, 3)
        weights_sum = weights.sum(dim=-1)
        ori_z_vals = ((z_vals - nears) / (fars - nears)).clamp(0, 1)
        depth = torch.sum(weights * ori_z_vals, dim=-1)   # NaN for a ray that misses the box (near == far), like the reference
        image = torch.sum(weights.unsqueeze(-1) * rgbs, dim=-2)
        if self.bg_radius > 0:
            bg_color = self.background(raymarching.sph_from_ray(rays_o, rays_d, self.bg_radius), rays_d.reshape(-1, 3))
        elif bg_color is None:
            bg_color = 1
        image = image + (1 - weights_sum).unsqueeze(-1) * bg_color
        return {"depth": depth.view(*prefix), "image": image.view(*prefix, 3), "weights_sum": weights_sum}
