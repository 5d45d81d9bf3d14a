"""GPU parity: the HIP path (through the C ABI of libpienerf_hip.so) against the CPU oracle on identical seeded inputs.

Bars (BASELINE.json north_star): integer / index work bit-exact; fp32 radiance and fp64 DOF displacements within 1e-4 rel.
The march kernel is built with the same no-contraction, same-promotion arithmetic as the oracle, so its float outputs
are compared bit for bit as well.
"""
import numpy as np
import pytest
import torch

import oracle
from conftest import make_oracle_sim, rel_err
from pienerf_amd import scene

pytestmark = pytest.mark.gpu
DEV = "cuda"


def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def test_library_identity():
    from pienerf_amd._lib import lib
    assert b"gfx950" in lib().pn_version()


# ------------------------------------------------------------------------------------------------ rays
def test_get_rays_and_near_far(small_opt):
    from pienerf_amd import raymarching
    from pienerf_amd.nerf.utils import get_rays
    W = H = 64
    pose = scene.orbit_pose(5.0, 30.0, -20.0)
    intr = scene.orbit_intrinsics(W, H, 50.0)
    o_ref, d_ref = oracle.get_rays(pose, intr, H, W)
    r = get_rays(T(pose[None]), intr, H, W)
    assert np.array_equal(r["rays_o"][0].cpu().numpy(), o_ref)
    assert np.array_equal(r["rays_d"][0].cpu().numpy(), d_ref)  # same op order, correctly rounded div/sqrt on both sides
    # independent check against the reference's torch formulation (nerf/utils.py:124-131), tolerance 1e-6
    i, j = np.meshgrid(np.arange(W, dtype=np.float32) + 0.5, np.arange(H, dtype=np.float32) + 0.5)
    dirs = np.stack([(i - intr[2]) / intr[0], (j - intr[3]) / intr[1], np.ones_like(i)], -1).reshape(-1, 3)
    dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
    assert np.abs(dirs @ pose[:3, :3].T - d_ref).max() < 1e-6
    aabb = np.array([-0.6, -0.8, -0.5, 0.7, 0.9, 0.55], np.float32)
    n_ref, f_ref = oracle.near_far_from_aabb(o_ref, d_ref, aabb, 0.2)
    n, f = raymarching.near_far_from_aabb(r["rays_o"][0], r["rays_d"][0], T(aabb), 0.2)
    assert np.array_equal(n.cpu().numpy(), n_ref) and np.array_equal(f.cpu().numpy(), f_ref)
    assert (n_ref == np.finfo(np.float32).max).any() and (n_ref < 10).any()  # both hit and miss rays are covered


# ------------------------------------------------------------------------------------------------ spatial hash
def test_pnts_in_grids_bit_exact(deformed_ip_state, small_opt):
    from pienerf_amd.nerf.utils import get_pnts_in_grids
    p = deformed_ip_state["p_def"]
    hgs = np.float32(small_opt["hash_grid_size"])
    bbmin, bbmax, res = oracle.render_bbox(p, hgs)
    n_grid = int(res.prod())
    ref = oracle.get_pnts_in_grids(len(p), n_grid, p, bbmin, bbmax, hgs, res)
    got = get_pnts_in_grids(len(p), n_grid, T(p), T(bbmin), T(bbmax), float(hgs), T(res))
    for a, b in zip(got, ref):
        assert np.array_equal(a.cpu().numpy(), b)
    assert ref[0].max() >= 2  # cells with several IPs exist, so the in-cell order is exercised


# ------------------------------------------------------------------------------------------------ march
def _march_inputs(ip, opt, ck, W=72, az=25.0, el=-15.0):
    pose = scene.orbit_pose(5.0, az, el)
    intr = scene.orbit_intrinsics(W, W, 50.0)
    o, d = oracle.get_rays(pose, intr, W, W)
    hgs = np.float32(opt["hash_grid_size"])
    bbmin, bbmax, res = oracle.render_bbox(ip["p_def"], hgs)
    n_grid = int(res.prod())
    pig = oracle.get_pnts_in_grids(len(ip["p_def"]), n_grid, ip["p_def"], bbmin, bbmax, hgs, res)
    nears, fars = oracle.near_far_from_aabb(o, d, np.concatenate([bbmin, bbmax]), 0.2)
    return dict(o=o, d=d, hgs=hgs, bbmin=bbmin, bbmax=bbmax, res=res, n_grid=n_grid, pig=pig, nears=nears, fars=fars)


@pytest.mark.parametrize("num_seek_IP,max_iter_num,n_step", [(1, 1, 1), (3, 1, 4), (2, 3, 8), (3, 5, 8)])
def test_march_bit_exact(deformed_ip_state, small_opt, ckpt, num_seek_IP, max_iter_num, n_step):
    from pienerf_amd import raymarching
    ip, ck = deformed_ip_state, ckpt
    m = _march_inputs(ip, small_opt, ck)
    N = m["o"].shape[0]
    alive = np.nonzero(m["nears"] < 1e30)[0].astype(np.int32)[::1]
    alive = np.concatenate([alive, np.arange(0, N, 97, dtype=np.int32)])  # include rays that miss the box
    n_alive = len(alive)
    rng = np.random.default_rng(1)
    noises = rng.random(n_alive).astype(np.float32) if n_step == 4 else None
    cb = np.zeros(6, np.float32)
    args = (len(ip["p_def"]), m["n_grid"])
    ref = oracle.march_rays_quadratic_bending(*m["pig"], *args, ip["p_def"], ip["p_ori"], ip["F"], ip["dF"], max_iter_num, m["bbmin"], m["bbmax"],
                                              m["hgs"], m["res"], num_seek_IP, np.float32(ip["IP_dx"]), False, cb, n_alive, n_step, alive, m["nears"],
                                              m["o"], m["d"], 1.0, ck["density_bitfield"], ck["cascade"], ck["grid_size"], m["nears"], m["fars"], 128,
                                              False, 0.0, 1024, noises=noises)
    assert not oracle.march_rays_quadratic_bending.last_oob
    pig_t = [T(a) for a in m["pig"]]
    if noises is None:
        got = raymarching.march_rays_quadratic_bending(*pig_t, *args, T(ip["p_def"]), T(ip["p_ori"]), T(ip["F"]), T(ip["dF"]), max_iter_num,
                                                       T(m["bbmin"]), T(m["bbmax"]), float(m["hgs"]), T(m["res"]), num_seek_IP, float(ip["IP_dx"]),
                                                       False, T(cb), n_alive, n_step, T(alive), T(m["nears"]), T(m["o"]), T(m["d"]), 1.0,
                                                       T(ck["density_bitfield"]), ck["cascade"], ck["grid_size"], T(m["nears"]), T(m["fars"]), 128,
                                                       False, 0.0, 1024)
    else:  # explicit noises go through the C ABI directly (the wrapper draws its own with torch.rand)
        from pienerf_amd._lib import check, lib, ptr, stream_ptr
        M = n_alive * n_step
        M += 128 - (M % 128)
        got = [torch.zeros(M, 3, device=DEV), torch.zeros(M, 3, device=DEV), torch.zeros(M, 2, device=DEV)]
        ts = dict(pd=T(ip["p_def"]), po=T(ip["p_ori"]), F=T(ip["F"]), dF=T(ip["dF"]), bmin=T(m["bbmin"]), bmax=T(m["bbmax"]), res=T(m["res"]), cb=T(cb),
                  al=T(alive), t=T(m["nears"]), o=T(m["o"]), d=T(m["d"]), g=T(ck["density_bitfield"]), fa=T(m["fars"]), no=T(noises))
        check(lib().pn_march_rays_quadratic_bending(ptr(pig_t[0]), ptr(pig_t[1]), ptr(pig_t[2]), *args, ptr(ts["pd"]), ptr(ts["po"]), ptr(ts["F"]),
                                                    ptr(ts["dF"]), max_iter_num, ptr(ts["bmin"]), ptr(ts["bmax"]), float(m["hgs"]), ptr(ts["res"]),
                                                    num_seek_IP, float(ip["IP_dx"]), 0, ptr(ts["cb"]), n_alive, n_step, ptr(ts["al"]), ptr(ts["t"]),
                                                    ptr(ts["o"]), ptr(ts["d"]), 1.0, 0.0, 1024, ck["cascade"], ck["grid_size"], ptr(ts["g"]),
                                                    ptr(ts["t"]), ptr(ts["fa"]), ptr(got[0]), ptr(got[1]), ptr(got[2]), ptr(ts["no"]), None,
                                                    stream_ptr()), "march")
    emitted = int((ref[2][:, 0] != 0).sum())
    assert emitted > 200, "test scene must produce samples"
    for name, a, b in zip(("xyzs", "dirs", "deltas"), got, ref):
        a = a.cpu().numpy()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{name}: {np.sum(a != b)} of {a.size} values differ"


@pytest.mark.parametrize("background,num_seek_IP,n_step", [(False, 1, 6), (True, 1, 6), (True, 3, 2), (True, 2, 16)])
def test_march_cut_mode(deformed_ip_state, small_opt, ckpt, background, num_seek_IP, n_step):
    """--cut: bbox = +-bound, samples outside cut_bounds are un-warped background (raymarching.cu:1195-1210,1380-1383).  `background`
    adds occupied density voxels outside the object (blobs of a random pattern), so that static samples are really emitted and the
    lane-per-ray pre-pass (pn_march_skip.h: skip_empty_cells) has to hand over at the right sequence element."""
    from pienerf_amd import raymarching
    ip, ck = deformed_ip_state, dict(ckpt)
    if background:
        rng = np.random.default_rng(5)
        blobs = np.repeat(rng.random(len(ck["density_bitfield"]) // 64) < 0.04, 64)   # runs of 512 morton-consecutive voxels = 8^3 blocks
        ck["density_bitfield"] = ck["density_bitfield"] | np.where(blobs, 0xFF, 0).astype(np.uint8)
    pose = scene.orbit_pose(4.0, 10.0, -5.0)
    W = 32
    o, d = oracle.get_rays(pose, scene.orbit_intrinsics(W, W, 50.0), W, W)
    hgs = np.float32(small_opt["hash_grid_size"])
    bbmin, bbmax, res = oracle.render_bbox(ip["p_def"], hgs, cut=True, bound=1.0)
    n_grid = int(res.prod())
    pig = oracle.get_pnts_in_grids(len(ip["p_def"]), n_grid, ip["p_def"], bbmin, bbmax, hgs, res)
    nears, fars = oracle.near_far_from_aabb(o, d, np.concatenate([bbmin, bbmax]), 0.2)
    alive = np.arange(W * W, dtype=np.int32)
    cb = np.array([-0.3, 0.9, -0.9, 0.5, -0.9, 0.9], np.float32)
    common = (len(ip["p_def"]), n_grid)
    ref = oracle.march_rays_quadratic_bending(*pig, *common, ip["p_def"], ip["p_ori"], ip["F"], ip["dF"], 1, bbmin, bbmax, hgs, res, num_seek_IP,
                                              np.float32(ip["IP_dx"]), True, cb, len(alive), n_step, alive, nears, o, d, 1.0, ck["density_bitfield"],
                                              ck["cascade"], ck["grid_size"], nears, fars, 128, False, 1.0 / 128, 300)
    got = raymarching.march_rays_quadratic_bending(*[T(a) for a in pig], *common, T(ip["p_def"]), T(ip["p_ori"]), T(ip["F"]), T(ip["dF"]), 1, T(bbmin),
                                                   T(bbmax), float(hgs), T(res), num_seek_IP, float(ip["IP_dx"]), True, T(cb), len(alive), n_step, T(alive),
                                                   T(nears), T(o), T(d), 1.0, T(ck["density_bitfield"]), ck["cascade"], ck["grid_size"], T(nears), T(fars),
                                                   128, False, 1.0 / 128, 300)
    emitted = ref[2][:len(alive) * n_step, 0].reshape(len(alive), n_step) != 0
    assert emitted.sum() > 100
    if background:  # many rays emit static samples; some only after a stretch of empty voxels, some not at all
        assert emitted[:, 0].mean() > 0.1 and (~emitted[:, 0]).sum() > 20
    for a, b in zip(got, ref):
        assert np.array_equal(a.cpu().numpy().view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------------ encoders / network
def test_grid_encode_matches_oracle(ckpt):
    from pienerf_amd.gridencoder import grid_encode
    rng = np.random.default_rng(2)
    x = rng.random((5000, 3)).astype(np.float32)
    x[:7] = [[0, 0, 0], [1, 1, 1], [0.5, 0.5, 0.5], [1.0, 0.0, 0.5], [-0.1, 0.5, 0.5], [0.5, 1.2, 0.5], [0.999999, 0.999999, 0.999999]]
    ref = oracle.grid_encode_forward(x, ckpt["embeddings"], ckpt["offsets"], ckpt["per_level_scale"], ckpt["base_resolution"])
    got = grid_encode(T(x), T(ckpt["embeddings"]), T(ckpt["offsets"]), ckpt["per_level_scale"], ckpt["base_resolution"]).cpu().numpy()
    assert got.shape == ref.shape == (5000, 32)
    assert np.abs(got - ref).max() <= 2e-6 * max(1.0, np.abs(ref).max())  # fp32, FMA-contracted on the GPU
    assert np.all(got[4] == 0) and np.all(got[5] == 0)  # out-of-range inputs encode to zero (gridencoder.cu:113-133)


def test_grid_encode_tiled_and_smoothstep(ckpt):
    from pienerf_amd.gridencoder import grid_encode
    rng = np.random.default_rng(3)
    x = rng.random((2000, 3)).astype(np.float32)
    for gridtype, align, interp in ((1, False, 0), (0, True, 0), (0, False, 1), (1, True, 1)):
        ref = oracle.grid_encode_forward(x, ckpt["embeddings"], ckpt["offsets"], ckpt["per_level_scale"], ckpt["base_resolution"], gridtype, align, interp)
        got = grid_encode(T(x), T(ckpt["embeddings"]), T(ckpt["offsets"]), ckpt["per_level_scale"], ckpt["base_resolution"], False, gridtype, align,
                          interp).cpu().numpy()
        assert np.abs(got - ref).max() <= 2e-6, (gridtype, align, interp)


def test_sh_encode_matches_oracle():
    from pienerf_amd.shencoder import sh_encode
    rng = np.random.default_rng(4)
    d = rng.standard_normal((4096, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    for deg in (1, 2, 3, 4):
        ref = oracle.sh_encode_forward(d, deg)
        got = sh_encode(T(d), deg).cpu().numpy()
        assert np.abs(got - ref).max() <= 1e-6


def test_nerf_forward_fused_vs_oracle_and_ops(ckpt):
    """Fused kernel (bf16 three-way split MFMA, fp32-accurate) vs the CPU oracle (sequential fp32) and vs the op-by-op GPU sequence
    (torch Linear).  Tolerance 1e-4 (north-star bar); the measured errors are printed (pytest -s)."""
    from pienerf_amd.nerf.network import NeRFNetwork
    rng = np.random.default_rng(5)
    M = 4099  # not a multiple of the 32-sample tile
    x = (rng.random((M, 3)).astype(np.float32) * 2 - 1) * 0.9
    x[:3] = [[0, 0, 0], [0.99, -0.99, 0.5], [1.5, 0, 0]]  # incl. one out-of-bound sample -> zero features
    d = rng.standard_normal((M, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    s_ref, c_ref = oracle.nerf_forward(x, d, ckpt, 1.0)
    net = NeRFNetwork(encoding="hashgrid", bound=1.0, cuda_ray=True).to(DEV).load_checkpoint_dict(ckpt)
    with torch.no_grad():
        s, c = net(T(x), T(d))
        s2, c2 = net.forward_ops(T(x), T(d))
    s, c, s2, c2 = s.cpu().numpy(), c.cpu().numpy(), s2.cpu().numpy(), c2.cpu().numpy()
    assert np.all(np.isfinite(s)) and np.all(np.isfinite(c))
    print(f"fused vs oracle: sigma rel {np.abs(s / s_ref - 1).max():.2e}, rgb abs {np.abs(c - c_ref).max():.2e}; "
          f"torch ops vs oracle: sigma rel {np.abs(s2 / s_ref - 1).max():.2e}, rgb abs {np.abs(c2 - c_ref).max():.2e}")
    assert np.abs(s / s_ref - 1).max() < 1e-4, np.abs(s / s_ref - 1).max()
    assert np.abs(c - c_ref).max() < 1e-4
    assert np.abs(s2 / s_ref - 1).max() < 1e-4 and np.abs(c2 - c_ref).max() < 1e-4
    assert 20 < np.median(s_ref) < 200  # the synthetic checkpoint's density calibration


def test_nerf_forward_is_bit_reproducible(ckpt):
    """The same launch repeated gives the same bits (round 1 saw 16-sample blocks of ~20 % of 1M-sample launches come out ~1e-2 off in an
    earlier version of the kernel; the cause it named then — packed-fp32 VALU beside bf16 MFMAs — did not reproduce in isolation,
    tools/repro_pk_mfma.hip, so this test is what guards the property itself)."""
    from pienerf_amd.nerf.network import NeRFNetwork
    rng = np.random.default_rng(11)
    M = 600_001
    x = T((rng.random((M, 3)).astype(np.float32) * 2 - 1) * 0.9)
    d = rng.standard_normal((M, 3)).astype(np.float32)
    d = T(d / np.linalg.norm(d, axis=-1, keepdims=True))
    net = NeRFNetwork(encoding="hashgrid", bound=1.0, cuda_ray=True).to(DEV).load_checkpoint_dict(ckpt)
    with torch.no_grad():
        s0, c0 = net(x, d)
        for _ in range(40):
            s, c = net(x, d)
            assert torch.equal(s, s0) and torch.equal(c, c0)


# ------------------------------------------------------------------------------------------------ composite / compaction
def test_composite_and_compaction(ckpt):
    from pienerf_amd import raymarching
    rng = np.random.default_rng(6)
    N, n_alive, n_step = 3000, 1700, 8
    alive = np.sort(rng.choice(N, n_alive, replace=False)).astype(np.int32)
    M = n_alive * n_step
    sig = (rng.random(M).astype(np.float32) * 120)
    rgb = rng.random((M, 3)).astype(np.float32)
    deltas = np.stack([np.full(M, 0.0034, np.float32), (rng.random(M) * 0.01 + 0.0034).astype(np.float32)], 1)
    for n in range(0, n_alive, 3):  # a third of the rays end early (delta == 0 sentinel)
        deltas[n * n_step + rng.integers(0, n_step):(n + 1) * n_step] = 0
    st = dict(t=(rng.random(N).astype(np.float32) + 3), ws=(rng.random(N).astype(np.float32) * 0.9), dep=rng.random(N).astype(np.float32),
              img=rng.random((N, 3)).astype(np.float32))
    ref = {k: v.copy() for k, v in st.items()}
    al_ref = alive.copy()
    oracle.composite_rays(n_alive, n_step, al_ref, ref["t"], sig, rgb, deltas, ref["ws"], ref["dep"], ref["img"], 1e-2)
    g = {k: T(v.copy()) for k, v in st.items()}
    al = T(alive.copy())
    raymarching.composite_rays(n_alive, n_step, al, g["t"], T(sig), T(rgb), T(deltas), g["ws"], g["dep"], g["img"], 1e-2)
    # alive / dead decisions are integer work: bit-exact, as is the survivor list
    assert np.array_equal(al.cpu().numpy(), al_ref)
    assert np.array_equal(raymarching.compact_rays(al).cpu().numpy(), oracle.compact_rays(al_ref))
    assert np.array_equal(oracle.compact_rays(al_ref), al_ref[al_ref >= 0])
    for k in ("t", "ws", "dep", "img"):
        assert rel_err(g[k].cpu().numpy(), ref[k]) < 1e-5, k  # __expf vs expf


@pytest.mark.parametrize("n", [1, 63, 256, 257, 100_003])
def test_compaction_sizes(n):
    from pienerf_amd import raymarching
    rng = np.random.default_rng(n)
    a = np.arange(n, dtype=np.int32)
    a[rng.random(n) < 0.6] = -1
    assert np.array_equal(raymarching.compact_rays(T(a)).cpu().numpy(), a[a >= 0])
    assert raymarching.compact_rays(T(np.full(n, -1, np.int32))).numel() == 0


# ------------------------------------------------------------------------------------------------ whole frame
@pytest.mark.parametrize("num_seek_IP,W", [(3, 96), (1, 64)])
def test_render_deformed_frame(deformed_ip_state, small_opt, ckpt, num_seek_IP, W):
    from pienerf_amd.nerf.network import NeRFNetwork
    ip = deformed_ip_state
    opt = dict(small_opt, num_seek_IP=num_seek_IP)
    pose = scene.orbit_pose(5.0, 20.0, -15.0)
    o, d = oracle.get_rays(pose, scene.orbit_intrinsics(W, W, 50.0), W, W)
    ref = oracle.render_deformed(o, d, ip, ckpt, opt)
    net = NeRFNetwork(encoding="hashgrid", bound=1.0, cuda_ray=True).to(DEV).load_checkpoint_dict(ckpt)
    net.p_def, net.p_ori, net.IP_F, net.IP_dF, net.IP_dx = T(ip["p_def"]), T(ip["p_ori"]), T(ip["F"]), T(ip["dF"]), ip["IP_dx"]
    with torch.no_grad():
        fused = net.render_deformed(T(o)[None], T(d)[None], collect_stats=True, **opt)
        st_f = dict(net.last_stats)
        ops = net.rund_cuda_ops(T(o)[None], T(d)[None], **opt)
        st_o = dict(net.last_stats)
    assert ref["samples"] > 2000
    # trip structure and sample counts are integer outcomes of the loop
    assert st_f["trips"] == st_o["trips"] == ref["trips"]
    assert st_f["samples"] == st_o["samples"] == ref["samples"]
    assert st_f["err"] == 0 and st_f["alive_at_exit"] == 0
    for name, out in (("fused", fused), ("ops", ops)):
        img = out["image"][0].cpu().numpy()
        ws = out["weights_sum"].cpu().numpy()
        d0 = out["depth_0"][0].cpu().numpy()
        assert np.abs(img - ref["image"]).max() < 1e-4, name
        assert np.abs(ws - ref["weights_sum"]).max() < 1e-4, name
        assert rel_err(d0, ref["depth_0"]) < 1e-4, name
        dep = out["depth"][0].cpu().numpy()
        hit = np.isfinite(ref["depth"])
        assert np.array_equal(np.isfinite(dep), hit)  # NaN exactly where nears == fars == FLT_MAX (renderer.py:898)
        assert np.abs(dep[hit] - ref["depth"][hit]).max() < 1e-4, name
    # fused path and op-by-op path run the same kernels in the same order: identical bits
    assert torch.equal(fused["image"], ops["image"]) and torch.equal(fused["depth_0"], ops["depth_0"])


# ------------------------------------------------------------------------------------------------ simulator
def test_sim_kernels_and_step(small_cloud, small_opt):
    from pienerf_amd.simulator.solver import Simulator
    o = small_opt
    ref = make_oracle_sim(small_cloud, o)
    sim = Simulator(dt=o["sim_dt"], iters=o["sim_iters"], bbox=torch.tensor([2.0 * o["bound"]] * 3), dx=o["sim_dx"], stiff=o["sim_stiff"],
                    base=torch.tensor([-o["bound"]] * 3), device=DEV)
    c = small_cloud
    sim.InitializeFromArrays(c["pos"], c["mass"], c["mu"], c["lam"], c["pin"])
    assert sim.n_IP == ref.n_IP and sim.n_k == ref.n_k
    assert np.array_equal(sim.IP_kernel.cpu().numpy(), ref.IP_kernel.numpy())
    assert rel_err(sim.IP_dNx.cpu().numpy(), ref.IP_dNx) < 1e-12
    assert rel_err(sim.Ainv.cpu().numpy(), ref.Ainv) < 1e-8
    assert rel_err(sim.rhs_rest.cpu().numpy().reshape(-1, 3), ref.rhs_rest) < 1e-10
    # rest state: pos = IP position, F = I, dF = 0
    pos, F, dF = sim.get_IP_info()
    assert np.abs(pos.cpu().numpy() - ref.IP_pos.numpy()).max() < 1e-6
    assert np.abs(F.cpu().numpy().reshape(-1, 3, 3) - np.eye(3)).max() < 1e-6 and np.abs(dF.cpu().numpy()).max() < 1e-5
    f = np.array([300.0, 100.0, -200.0])
    vid = sim.n_IP // 2
    sim.update_force(vid, torch.tensor(f))
    ref.update_force(vid, f)
    assert rel_err(sim.dof_f.cpu().numpy().reshape(-1, 3), ref.dof_f) < 1e-14
    for step in range(6):
        sim.stepforward()
        ref.stepforward()
        disp = sim.dof.cpu().numpy().reshape(-1, 3) - ref.dof_rest
        disp_ref = ref.dof - ref.dof_rest
        assert rel_err(disp, disp_ref) < 1e-4, (step, rel_err(disp, disp_ref))
        if step == 2:
            sim.clear_force()
            ref.clear_force()
    p1, F1, dF1 = (t.cpu().numpy() for t in sim.get_IP_info())
    p2, F2, dF2 = ref.get_IP_info()
    print(f"get_IP_info after 6 substeps: pos {np.abs(p1 - p2).max():.2e} abs, F {np.abs(F1 - F2).max():.2e} abs, dF {rel_err(dF1, dF2):.2e} rel")
    assert np.abs(p1 - p2).max() < 1e-5 and np.abs(F1 - F2).max() < 1e-4 and rel_err(dF1, dF2) < 1e-4   # north_star's bar for everything in fp32
    assert np.abs(p2 - ref.IP_pos.numpy()).max() > 1e-3  # the configuration really moved
    # op-level: calc_elastic / collect_rhs on the deformed state
    RF, VF, _ = oracle.calc_elastic(ref.IP_kernel.numpy(), ref.IP_dNx, ref.dof)
    rhs_ref = oracle.collect_rhs_IP(ref.dx, ref.IP_kernel.numpy(), ref.IP_mu, ref.IP_lam, ref.IP_dNx, RF, VF, ref.n_k * 10)
    sim.dof.copy_(T(ref.dof.reshape(-1)))
    assert rel_err(sim.build_rhs().cpu().numpy().reshape(-1, 3), rhs_ref) < 1e-10


def test_harness_step_matches_oracle_sequence(small_cloud, small_opt, ckpt):
    """One GUI-frame equivalent: get_IP_info -> stepforward -> render_deformed (render sees the pre-step state)."""
    from pienerf_amd.harness import SimRenderHarness
    opt = dict(small_opt, W=64, H=64)
    h = SimRenderHarness(opt, cloud=small_cloud, ckpt=ckpt, device=DEV)
    ref = make_oracle_sim(small_cloud, opt)
    p_ori, _, _ = ref.get_IP_info()
    o, d = oracle.get_rays(h.pose, h.intrinsics, 64, 64)
    for frame in range(3):
        p_def, F, dF = ref.get_IP_info()
        ref.stepforward()
        r = oracle.render_deformed(o, d, dict(p_def=p_def, p_ori=p_ori, F=F, dF=dF, IP_dx=ref.dx * 1.05), ckpt, opt)
        out = h.to_host(h.step())
        assert np.abs(out["image"].reshape(-1, 3) - r["image"]).max() < 1e-4, frame   # the north-star bar (measured ~4e-6)
    assert h.frame == 3


def test_graph_replay_equals_eager_steps(small_cloud, small_opt, ckpt):
    """The whole step captured as one HIP graph (sim on a forked stream, async render with a fixed trip count) replays to the
    same images and the same DOF trajectory as the eager path (two harness instances differ only by the summation order of
    the init-time matrix assembly, i.e. at round-off)."""
    from pienerf_amd.harness import SimRenderHarness
    opt = dict(small_opt, W=64, H=64)
    eager = SimRenderHarness(opt, cloud=small_cloud, ckpt=ckpt, device=DEV)
    graph = SimRenderHarness(opt, cloud=small_cloud, ckpt=ckpt, device=DEV).capture(n_trips=8)
    assert torch.equal(graph.sim.dof, eager.sim.dof)  # capture left the simulator state untouched
    for frame in range(4):
        a = eager.step()
        eager.synchronize()
        b = graph.step_graph()
        graph.synchronize()
        assert (a["image"] - b["image"]).abs().max() < 1e-5 and (a["depth_0"] - b["depth_0"]).abs().max() < 1e-4, frame
        assert rel_err((graph.sim.dof - graph.sim.dof_rest).cpu().numpy(), (eager.sim.dof - eager.sim.dof_rest).cpu().numpy()) < 1e-7, frame
    st = graph.model.render_status()
    assert st["alive_at_exit"] == 0 and st["err"] == 0 and st["trips"] >= 3
    # too few captured trips: the frame is finished with further trips (renderer.py:836-891 has no trip limit), bit-identical to the eager frame
    # (fused_from = -1: trip-by-trip launches only — with the later trips as one launch, pn_render_opts.fused_from, one captured trip is enough)
    short = SimRenderHarness(dict(opt, fused_from=-1), cloud=small_cloud, ckpt=ckpt, device=DEV).capture(n_trips=1)
    fresh = SimRenderHarness(opt, cloud=small_cloud, ckpt=ckpt, device=DEV)
    for frame in range(3):
        a = fresh.step()
        fresh.synchronize()
        short.step_graph()
        b = short.finish_graph_frame()
        assert torch.equal(a["image"], b["image"]) and torch.equal(a["depth_0"], b["depth_0"]), frame
        assert short.model.last_stats["alive_at_exit"] == 0 and short.model.last_stats["trips"] >= 3
    assert short.graph_continued == 3


@pytest.mark.parametrize("lanes,depth,ahead,trips", [(2, 2, None, 8), (3, 1, 1, 8), (1, 2, 0, 8), (2, 2, None, 2), (1, 1, 0, None), (2, 1, None, 3)])
def test_pipelined_frames_equal_eager_steps(small_cloud, small_opt, ckpt, lanes, depth, ahead, trips):
    """Frames in flight (frames.FramePipeline on the HIP backend: simulator running ahead on its own stream, one render graph per
    workspace, ordered by snapshot events, results copied to pinned host memory) give the eager sequence of images bit for bit — also
    when the captured trip count (2) is too small and every frame is finished by a continuation, and with a different camera per frame."""
    from pienerf_amd.harness import SimRenderHarness
    opt = dict(small_opt, W=64, H=64)
    eager = SimRenderHarness(opt, cloud=small_cloud, ckpt=ckpt, device=DEV)
    dev_copies = {}

    def keep_device_copy(frame, res):   # runs when the frame is complete, before its workspace is reused
        dev_copies[frame] = res["device"]["image"].clone()
    # a trip count that is too small only matters to the trip-by-trip launches: those cases run with fused_from = -1, the others with the later trips
    # as one launch (pn_render_opts.fused_from, picked by the harness)
    pipe = SimRenderHarness(opt, cloud=small_cloud, ckpt=ckpt, device=DEV).capture_pipelined(lanes=lanes, depth=depth, n_trips=trips, sim_ahead=ahead,
                                                                                             on_retire=keep_device_copy,
                                                                                             render_kw=(dict(fused_from=-1) if trips in (2, 3) else None))
    n_frames = 9
    poses = [scene.orbit_pose(opt["radius"], 7.0 * f, -3.0 * f) for f in range(n_frames)]
    want = []
    for f in range(n_frames):
        want.append(eager.to_host(eager.step(pose=poses[f])))
    eager.synchronize()
    got = []
    for f in range(n_frames):
        for idx, res in pipe.step_pipelined(pose=poses[f]):
            got.append((idx, {k: res[k].copy() for k in ("image", "depth", "depth_0")}))
    for idx, res in pipe.drain_pipeline():
        got.append((idx, {k: res[k].copy() for k in ("image", "depth", "depth_0")}))
    assert [g[0] for g in got] == list(range(n_frames))
    for f in range(n_frames):
        assert np.array_equal(got[f][1]["image"], want[f]["image"]) and np.array_equal(got[f][1]["depth_0"], want[f]["depth_0"]), f
        assert np.array_equal(got[f][1]["depth"], want[f]["depth"], equal_nan=True), f
        assert np.array_equal(dev_copies[f][0].cpu().numpy(), want[f]["image"])       # the device copy is the same frame
    if trips in (2, 3):   # (3: two of the captured trips are margin trips — small grids, two-launch compaction — with most of the frame's rays in them)
        assert pipe._pipe_backend.continued == n_frames                                 # every frame needed the continuation
    else:
        assert pipe._pipe_backend.continued == 0
    # the simulator ran ahead of the last rendered frame by a known number of substeps
    assert pipe.substeps_enqueued == n_frames + (lanes if ahead is None else ahead)
    for _ in range(pipe.substeps_enqueued - n_frames):
        eager.sim.stepforward()
    assert rel_err((pipe.sim.dof - pipe.sim.dof_rest).cpu().numpy(), (eager.sim.dof - eager.sim.dof_rest).cpu().numpy()) < 1e-7
    assert np.abs(want[0]["image"] - want[4]["image"]).max() > 1e-3  # the object (and the camera) really moved between frames


def test_force_change_between_overlapped_steps_matches_oracle(small_cloud, small_opt, ckpt):
    """update_force / clear_force while the substeps run on their own stream (harness.step with overlap_sim, and the pipelined form with
    the simulator running ahead): the change is enqueued on the simulator's stream (Simulator.force_stream), so it lands between two
    substeps — the trajectory equals the oracle's with the force switched at the same substep index (solver.py:578-593, the GUI's drag
    and release).  Repeated to give a race a chance."""
    from pienerf_amd.harness import SimRenderHarness
    opt = dict(small_opt, W=32, H=32)
    f1, f2 = np.array([300.0, 100.0, -200.0]), np.array([-150.0, 220.0, 90.0])
    for rep in range(3):
        h = SimRenderHarness(opt, cloud=small_cloud, ckpt=ckpt, device=DEV)  # overlap_sim=True: substep on a side stream
        assert h.sim.force_stream is h._sim_stream
        ref = make_oracle_sim(small_cloud, opt)
        vid = h.sim.n_IP // 2
        plan = {1: ("set", vid, f1), 3: ("set", vid // 2, f2), 5: ("clear",), 6: ("set", vid, f2)}
        for step in range(8):
            if step in plan:
                if plan[step][0] == "set":
                    h.sim.update_force(plan[step][1], plan[step][2])
                    ref.update_force(plan[step][1], plan[step][2])
                else:
                    h.sim.clear_force()
                    ref.clear_force()
            h.step()       # no synchronisation in between: the force launch must order itself against the running substep
            ref.stepforward()
        h.synchronize()
        disp, want = h.sim.dof.cpu().numpy().reshape(-1, 3) - ref.dof_rest, ref.dof - ref.dof_rest
        assert rel_err(disp, want) < 1e-6, (rep, rel_err(disp, want))
        assert rel_err(h.sim.dof_f.cpu().numpy().reshape(-1, 3), ref.dof_f) < 1e-14
    # pipelined: the simulator is `ahead` substeps in front; a force set now acts from substep `substeps_enqueued`
    p = SimRenderHarness(opt, cloud=small_cloud, ckpt=ckpt, device=DEV).capture_pipelined(lanes=2, n_trips=8)
    ref = make_oracle_sim(small_cloud, opt)
    done = 0
    for frame in range(9):
        if frame in (2, 5):
            while done < p.substeps_enqueued:
                ref.stepforward()
                done += 1
            if frame == 2:
                p.sim.update_force(p.sim.n_IP // 2, f1)
                ref.update_force(p.sim.n_IP // 2, f1)
            else:
                p.sim.clear_force()
                ref.clear_force()
        p.step_pipelined()
    p.drain_pipeline()
    while done < p.substeps_enqueued:
        ref.stepforward()
        done += 1
    assert rel_err(p.sim.dof.cpu().numpy().reshape(-1, 3) - ref.dof_rest, ref.dof - ref.dof_rest) < 1e-6


def _batches_one_after_the_other(h, out, B, **extra):
    """The reference semantics of max_ray_batch (renderer.py:562-576): one render call per batch of B rays.  Returns image, depth_0, the summed
    sample count and the largest trip count."""
    m = h.model
    o, d = out["rays_o"][0], out["rays_d"][0]
    N = o.shape[0]
    img, dep = torch.empty(N, 3, device=DEV), torch.empty(N, device=DEV)
    total, trips = 0, 0
    kw = dict(h.render_kwargs(), **extra)
    kw.pop("ray_batch", None)
    with h._amp():
        for head in range(0, N, B):
            r = m.render_deformed(o[None, head:head + B], d[None, head:head + B], collect_stats=True, frame_slot=7, **kw)
            img[head:head + B], dep[head:head + B] = r["image"][0], r["depth_0"][0]
            total += m.last_stats["samples"]
            trips = max(trips, m.last_stats["trips"])
    return img, dep, total, trips


@pytest.mark.parametrize("fp16", [False, True])
def test_ray_batches_keep_their_own_trip_schedules(small_cloud, small_opt, ckpt, fp16):
    """pn_render_opts.ray_batch (BASELINE configs[4], max_ray_batch): all batches advance inside the same launches, each with its own schedule
    n_step = max(min(N_b // n_alive_b, 8), 1) and its own max_steps count.  Against the batches rendered one after the other (one render call
    per batch): the same image bit for bit, the same number of marched samples (it depends on every batch's n_step sequence), the same number
    of trips as the slowest batch.  (A batch's own `step >= max_steps` exit is kept in the group records as well, but dt_min = 2 sqrt(3) / max_steps
    makes it unreachable inside the box, as in the reference.)"""
    from pienerf_amd.harness import SimRenderHarness
    opt = dict(small_opt, W=60, H=60, fp16=fp16, max_iter_num=5)        # 3600 rays = 3 batches of 1024 + one of 528
    whole = SimRenderHarness(opt, cloud=small_cloud, ckpt=ckpt, device=DEV, overlap_sim=False)
    grouped = SimRenderHarness(dict(opt, ray_batch=1024), cloud=small_cloud, ckpt=ckpt, device=DEV, overlap_sim=False)
    for h in (whole, grouped):
        h.sim.update_force(h.sim.n_IP // 2, np.array([300.0, 100.0, -200.0]))
    for f in range(3):
        pose = scene.orbit_pose(opt["radius"], 9.0 * f, 2.0 * f)
        a = whole.step(pose=pose, collect_stats=True)
        st_w = dict(whole.model.last_stats)
        b = grouped.step(pose=pose, collect_stats=True)
        st_g = dict(grouped.model.last_stats)
        img, dep, total, trips = _batches_one_after_the_other(whole, a, 1024)
        assert st_g["err"] == 0 and st_g["alive_at_exit"] == 0
        assert st_g["samples"] == total and st_g["trips"] == trips, (st_g, total, trips, st_w)
        assert torch.equal(b["image"].reshape(-1, 3), img) and torch.equal(b["depth_0"].reshape(-1), dep)
        # compositing does not depend on the schedule at all, the number of marched samples does
        assert torch.equal(b["image"], a["image"]) and torch.equal(b["depth_0"], a["depth_0"])
        assert st_g["samples"] != st_w["samples"]
    # one batch covering everything is the frame in one piece; a batch size that does not divide the ray count; the smallest batch
    one = SimRenderHarness(dict(opt, ray_batch=4096), cloud=small_cloud, ckpt=ckpt, device=DEV, overlap_sim=False)
    odd = SimRenderHarness(dict(opt, ray_batch=1000), cloud=small_cloud, ckpt=ckpt, device=DEV, overlap_sim=False)
    tiny = SimRenderHarness(dict(opt, ray_batch=64), cloud=small_cloud, ckpt=ckpt, device=DEV, overlap_sim=False)
    ref = SimRenderHarness(opt, cloud=small_cloud, ckpt=ckpt, device=DEV, overlap_sim=False)
    a = ref.step(collect_stats=True)
    st_a = dict(ref.model.last_stats)
    b = one.step(collect_stats=True)
    assert torch.equal(a["image"], b["image"]) and one.model.last_stats["samples"] == st_a["samples"] and one.model.last_stats["trips"] == st_a["trips"]
    for h, B in ((odd, 1000), (tiny, 64)):
        c = h.step(collect_stats=True)
        img, dep, total, trips = _batches_one_after_the_other(ref, a, B)
        assert h.model.last_stats["samples"] == total and h.model.last_stats["trips"] == trips
        assert torch.equal(c["image"].reshape(-1, 3), img)
    with pytest.raises(RuntimeError):
        SimRenderHarness(dict(opt, ray_batch=32), cloud=small_cloud, ckpt=ckpt, device=DEV, overlap_sim=False).step()


@pytest.mark.parametrize("fp16,n_trips", [(False, None), (True, None), (False, 2)])
def test_staged_ray_batches_equal_one_shot_frames(small_cloud, small_opt, ckpt, fp16, n_trips):
    """harness.capture_staged (BASELINE configs[4]: the frame in ray batches — a ray-group dimension of the pipelined frame's launches): rays are
    independent, so the frames equal the one-shot eager frames bit for bit — also the last, partial batch — and a trip count that is too small
    for the slowest batch is made up for by continuing the frame when it is retired."""
    from pienerf_amd.harness import SimRenderHarness
    opt = dict(small_opt, W=60, H=60, fp16=fp16, max_iter_num=5)        # 3600 rays = 3 batches of 1024 + one of 528
    eager = SimRenderHarness(opt, cloud=small_cloud, ckpt=ckpt, device=DEV)
    poses = [scene.orbit_pose(opt["radius"], 9.0 * f, 2.0 * f) for f in range(5)]
    want = [eager.to_host(eager.step(pose=p)) for p in poses]
    eager.synchronize()
    st = SimRenderHarness(opt, cloud=small_cloud, ckpt=ckpt, device=DEV).capture_staged(batch=1024, lanes=2, n_trips=n_trips)
    assert st._pipe_backend.kw["ray_batch"] == 1024 and "ray_batch" not in st.opt   # round-3 advisor: capture_staged no longer edits the harness's options
    got = []
    for p in poses:
        got += [(i, {k: r[k].copy() for k in ("image", "depth", "depth_0")}) for i, r in st.step_pipelined(pose=p)]
    got += [(i, {k: r[k].copy() for k in ("image", "depth", "depth_0")}) for i, r in st.drain_pipeline()]
    assert [i for i, _ in got] == list(range(5))
    for f in range(5):
        assert np.array_equal(got[f][1]["image"], want[f]["image"]) and np.array_equal(got[f][1]["depth_0"], want[f]["depth_0"]), f
        assert np.array_equal(got[f][1]["depth"], want[f]["depth"], equal_nan=True), f
    assert (st._pipe_backend.continued > 0) == (n_trips == 2)   # (the simulator runs ahead of the frames: its dof is not the eager harness's)


def test_force_change_is_ordered_against_substeps_on_the_callers_stream(small_cloud, small_opt, ckpt):
    """The force kernel runs on Simulator.force_stream (the harness's simulator stream); a substep that the CALLER then launches on its own
    stream — sim.stepforward() directly, or the whole-step graph of capture() / step_graph() — must wait for it (round-2 advisor finding:
    the side stream waited for the caller, the caller never waited back).  Trajectories against the oracle, repeated to give a race a chance."""
    from pienerf_amd.harness import SimRenderHarness
    opt = dict(small_opt, W=32, H=32)
    f1, f2 = np.array([300.0, 100.0, -200.0]), np.array([-150.0, 220.0, 90.0])
    for rep in range(3):
        h = SimRenderHarness(opt, cloud=small_cloud, ckpt=ckpt, device=DEV)
        assert h.sim.force_stream is not None
        ref = make_oracle_sim(small_cloud, opt)
        vid = h.sim.n_IP // 2
        for step in range(8):
            f = (f1, f2)[step % 2] * (1 + 0.1 * step)
            h.sim.update_force(vid, f)          # on the side stream ...
            ref.update_force(vid, f)
            h.sim.stepforward()                 # ... the substep on the current stream, no synchronisation in between
            ref.stepforward()
        h.synchronize()
        assert rel_err(h.sim.dof.cpu().numpy().reshape(-1, 3) - ref.dof_rest, ref.dof - ref.dof_rest) < 1e-6, rep
    g = SimRenderHarness(opt, cloud=small_cloud, ckpt=ckpt, device=DEV).capture(n_trips=8)
    ref = make_oracle_sim(small_cloud, opt)
    vid = g.sim.n_IP // 2
    for step in range(8):
        if step in (1, 4):
            g.sim.update_force(vid, f1 if step == 1 else f2)
            ref.update_force(vid, f1 if step == 1 else f2)
        if step == 6:
            g.sim.clear_force()
            ref.clear_force()
        g.step_graph()
        ref.stepforward()
    g.finish_graph_frame()
    g.synchronize()
    assert rel_err(g.sim.dof.cpu().numpy().reshape(-1, 3) - ref.dof_rest, ref.dof - ref.dof_rest) < 1e-6


def test_pipelined_frames_without_a_pose_use_the_harness_pose(small_cloud, small_opt, ckpt):
    """step_pipelined(pose=P) followed by step_pipelined() calls: every workspace keeps its own device copy of the camera, so a frame without
    a pose must re-upload the harness's current pose where the workspace last rendered another one (round-2 advisor finding: frames
    alternated between stale poses), and a change of h.pose after capture is picked up."""
    from pienerf_amd.harness import SimRenderHarness
    opt = dict(small_opt, W=40, H=40)
    eager = SimRenderHarness(opt, cloud=small_cloud, ckpt=ckpt, device=DEV)
    pipe = SimRenderHarness(opt, cloud=small_cloud, ckpt=ckpt, device=DEV).capture_pipelined(lanes=2, depth=2, n_trips=8)
    P = scene.orbit_pose(opt["radius"], 40.0, -20.0)
    Q = scene.orbit_pose(opt["radius"], -30.0, 10.0)
    plan = [P, None, None, None, None, None, "Q", None, None]       # frame 0 with P, then the default pose, then h.pose = Q from frame 6 on
    want, got = [], []
    for p in plan:
        if isinstance(p, str):
            eager.pose = pipe.pose = Q
            p = None
        want.append(eager.to_host(eager.step(pose=p))["image"])
        got += [(i, r["image"].copy()) for i, r in pipe.step_pipelined(pose=p)]
    got += [(i, r["image"].copy()) for i, r in pipe.drain_pipeline()]
    eager.synchronize()
    assert [i for i, _ in got] == list(range(len(plan)))
    for f in range(len(plan)):
        assert np.array_equal(got[f][1], want[f]), f
    assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[5], want[6])
