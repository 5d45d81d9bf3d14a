"""Multi-rank start-up with a background model (bg_radius > 0): the one-off checkpoint broadcast (pienerf_amd/frames.py: checkpoint_tensors /
broadcast_checkpoint) carries encoder_bg.embeddings and the two bg_net weights, so that ranks other than the source do not render a randomly initialised
sky.  Two gloo ranks on the CPU, set up like tests/test_frames_gloo.py's worlds."""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _model(seed, bg_radius):
    from pienerf_amd.nerf.network import NeRFNetwork
    torch.manual_seed(seed)
    m = NeRFNetwork(encoding="hashgrid", bound=1.0, cuda_ray=True, bg_radius=bg_radius)
    with torch.no_grad():
        m.density_bitfield.random_(0, 256)
    return m


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from pienerf_amd.frames import broadcast_checkpoint, checkpoint_tensors
    m = _model(100 + rank, 32)             # seeded differently on every rank
    names = ["encoder.embeddings", "density_bitfield", "sigma_net.0.weight", "sigma_net.1.weight", "color_net.0.weight", "color_net.1.weight",
             "color_net.2.weight", "encoder_bg.embeddings", "bg_net.0.weight", "bg_net.1.weight"]
    sd = m.state_dict()
    ts = checkpoint_tensors(m)
    assert [t.data_ptr() for t in ts] == [sd[n].data_ptr() for n in names]     # the model's own storage, in a fixed order
    m._net_sig = m._bg_sig = ("packed", "earlier")
    broadcast_checkpoint(m, src=0)
    assert m._net_sig is None and m._bg_sig is None     # both packed weight images are rebuilt on next use (a receive into .data moves no version counter)
    torch.save({n: sd[n].clone() for n in names}, os.path.join(out_dir, f"r{rank}.pt"))
    plain = _model(200 + rank, -1)         # without a background model the list is what it always was
    assert len(checkpoint_tensors(plain)) == 7
    broadcast_checkpoint(plain, src=0)
    torch.save(plain.encoder.embeddings.data.clone(), os.path.join(out_dir, f"p{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_checkpoint_broadcast_carries_the_background_model(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    r0, r1 = torch.load(tmp_path / "r0.pt"), torch.load(tmp_path / "r1.pt")
    want = _model(100, 32).state_dict()
    other = _model(101, 32).state_dict()
    for n in r0:
        assert torch.equal(r0[n], want[n]) and torch.equal(r1[n], r0[n]), n      # rank 1 now holds rank 0's tensors ...
    for n in ("encoder_bg.embeddings", "bg_net.0.weight", "bg_net.1.weight"):
        assert not torch.equal(other[n], want[n]), n                               # ... which it did not before
    assert torch.equal(torch.load(tmp_path / "p0.pt"), torch.load(tmp_path / "p1.pt"))
