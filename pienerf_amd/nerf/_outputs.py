"""The rays a frame driver takes and the tensors it writes: what every render form of NeRFRenderer (renderer.py and the mixins beside it) shares."""
import torch


def flat_rays(rays_o, rays_d):
    """The rays as the frame drivers take them: [N, 3], fp32, contiguous."""
    return rays_o.to(torch.float32).contiguous().view(-1, 3), rays_d.to(torch.float32).contiguous().view(-1, 3)


def take_output(name, shape, dtype, device, *dicts):
    """The output tensor `name` of a frame: the first of `dicts` (None entries are skipped) that holds it, else a new one; whoever's it is, it has
    `shape` and `dtype` and is contiguous."""
    t = next((d[name] for d in dicts if d is not None and d.get(name) is not None), None)
    if t is None:
        t = torch.empty(shape, dtype=dtype, device=device)
    assert t.shape == shape and t.dtype == dtype and t.is_contiguous(), name
    return t


def frame_outputs(N, device, out_buffers=None):
    """(image [N, 3], depth, depth_0, weights_sum [N]) of one frame, fp32: the caller's `out_buffers` where it has them, else new."""
    return tuple(take_output(k, (N, 3) if k == "image" else (N,), torch.float32, device, out_buffers) for k in ("image", "depth", "depth_0", "weights_sum"))
