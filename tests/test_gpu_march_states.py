"""The ray march on crowded, sparse, singular, squashed, twisted and coincident IP states (tests/march_states.py: what each state is and
which path of pn_march_window.h / pn_march_tables.h it is there for).  The op and the split between its two launches bit for bit against the
CPU oracle, the frame tables' in-cell order, whole frames against the oracle's frames at the standing 1e-4, and the frame's launch forms
against each other bit for bit.  tests/test_march_states_host.py shows on the CPU that the reference arithmetic stays finite on every state."""
import numpy as np
import pytest
import torch

import march_states as ms
import oracle
from pienerf_amd import scene
from test_gpu_parity import DEV, T

pytestmark = pytest.mark.gpu

OP_FORMS = [(1, 1, 1), (2, 3, 8), (3, 1, 8), (3, 5, 8), (3, 5, 64)]   # (num_seek_IP, max_iter_num, n_step)
FRAME_FORMS = [(1, 1), (3, 5)]                                        # (num_seek_IP, max_iter_num)
CUT_BOUNDS = [-0.95, 0.95, -0.95, 0.95, -0.95, 0.95]                  # the body (|p_def| < 0.9) stays inside
FRAME_W = 64
_oracle_frames = {}


@pytest.fixture(scope="module")
def states(deformed_ip_state, small_opt):
    out = {}
    for name in ms.NAMES:
        state, facts = ms.build(name, deformed_ip_state, small_opt)
        ms.check_facts(name, facts)
        print(name, facts)
        out[name] = state
    return out


@pytest.fixture(scope="module")
def coincident(deformed_ip_state, small_opt, ckpt):
    state, rays, facts = ms.coincident(deformed_ip_state, small_opt, ckpt)
    ms.check_facts("coincident", facts)
    return state, rays


@pytest.fixture
def tail_rounds():
    from pienerf_amd._lib import check, lib

    def set_rounds(r):
        check(lib().pn_march_set_tail_rounds(int(r)), "set_tail_rounds")
    yield set_rounds
    set_rounds(0)


@pytest.fixture
def skip_dda():
    from pienerf_amd._lib import check, lib

    def set_dda(on):
        check(lib().pn_march_set_skip_dda(int(on)), "set_skip_dda")
    yield set_dda
    set_dda(-1)


def _net(ckpt, ip):
    from pienerf_amd.nerf.network import NeRFNetwork
    net = NeRFNetwork(encoding="hashgrid", bound=1.0, cuda_ray=True).to(DEV).load_checkpoint_dict(ckpt)
    net.p_def, net.p_ori, net.IP_F, net.IP_dF, net.IP_dx = T(ip["p_def"]), T(ip["p_ori"]), T(ip["F"]), T(ip["dF"]), ip["IP_dx"]
    return net


def _device_march(state, m, ck, alive, num_seek_IP, max_iter_num, n_step, rays_t=None):
    from pienerf_amd import raymarching
    rays_t = m["nears"] if rays_t is None else rays_t
    return raymarching.march_rays_quadratic_bending(*[T(a) for a in m["pig"]], len(state["p_def"]), m["n_grid"], T(state["p_def"]), T(state["p_ori"]),
                                                   T(state["F"]), T(state["dF"]), max_iter_num, T(m["bbmin"]), T(m["bbmax"]), float(m["hgs"]), T(m["res"]),
                                                   num_seek_IP, float(state["IP_dx"]), False, T(np.zeros(6, np.float32)), len(alive), n_step, T(alive),
                                                   T(rays_t), T(m["o"]), T(m["d"]), 1.0, T(ck["density_bitfield"]), ck["cascade"], ck["grid_size"],
                                                   T(m["nears"]), T(m["fars"]), 128, False, 0.0, 1024)


def _assert_same_bits(got, ref, what):
    for name, a, b in zip(("xyzs", "dirs", "deltas"), got, ref):
        a = a.cpu().numpy()
        assert a.shape == b.shape
        ne = a.view(np.uint32) != b.view(np.uint32)
        assert not ne.any(), f"{what} {name}: {int(ne.any(-1).sum())} of {len(a)} rows differ, first at row {int(np.nonzero(ne.any(-1))[0][0])}"


# ------------------------------------------------------------------------------------------------ (a) the op, bit for bit
def _alive_rays(m):
    alive = np.nonzero(m["nears"] < 1e30)[0].astype(np.int32)
    return np.concatenate([alive, np.arange(0, m["o"].shape[0], 97, dtype=np.int32)])   # include rays that miss the box


@pytest.mark.parametrize("num_seek_IP,max_iter_num,n_step", OP_FORMS)
@pytest.mark.parametrize("name", ms.NAMES)
def test_march_bit_exact_on_state(states, ckpt, name, num_seek_IP, max_iter_num, n_step):
    state = states[name]
    m = ms.march_inputs(state)
    alive = _alive_rays(m)
    ref = ms.oracle_march(state, m, ckpt, alive, num_seek_IP, max_iter_num, n_step)
    assert not oracle.march_rays_quadratic_bending.last_oob
    emitted = int((ref[2][:, 0] != 0).sum())
    print(f"{name} seek {num_seek_IP} iters {max_iter_num} n_step {n_step}: {emitted} samples emitted")
    # n_step = 1 emits at most one sample per ray, and the squashed body covers the fewest rays (128 of them at this size)
    assert emitted > (100 if n_step == 1 else 200), "the state must produce samples"
    _assert_same_bits(_device_march(state, m, ckpt, alive, num_seek_IP, max_iter_num, n_step), ref, name)


@pytest.mark.parametrize("num_seek_IP", [1, 2, 3])
def test_march_bit_exact_on_coincident_samples(coincident, ckpt, num_seek_IP):
    """Samples ON an IP: d == 0 alone, twice (the tie goes to the earlier candidate), and beside a candidate at d^2 = 2^-140 that comes earlier in
    the list — right only if neither the distance nor the 64-bit key of eval_scan<2,3> loses its denormals."""
    state, rays = coincident
    m = ms.coincident_inputs(state, rays)
    ref = ms.oracle_march(state, m, ckpt, rays["alive"], num_seek_IP, 1, 1, rays_t=rays["t"])
    assert not oracle.march_rays_quadratic_bending.last_oob
    emitted = int((ref[2][:32, 0] != 0).sum())
    print(f"coincident seek {num_seek_IP}: {emitted} of 32 samples emitted")
    assert emitted >= 24
    _assert_same_bits(_device_march(state, m, ckpt, rays["alive"], num_seek_IP, 1, 1, rays_t=rays["t"]), ref, "coincident")


# ------------------------------------------------------------------------------------------------ (b) the split between the two launches
@pytest.mark.parametrize("num_seek_IP,max_iter_num,n_step", [(3, 1, 64), (1, 1, 64)])
@pytest.mark.parametrize("rounds", [1, 1000])
@pytest.mark.parametrize("name", ["crowded", "sparse"])
def test_march_split_between_the_two_launches_on_state(states, ckpt, tail_rounds, name, rounds, num_seek_IP, max_iter_num, n_step):
    """rounds = 1: every ray that needs more than one window of 8 points finishes in the wave-per-ray launch, where the 64 points of one ray
    stage four or five candidate lists — on `crowded` some over the wave's LDS share and some under; rounds = 1000: no ray reaches it."""
    state = states[name]
    m = ms.march_inputs(state)
    alive = np.nonzero(m["nears"] < 1e30)[0].astype(np.int32)
    ref = ms.oracle_march(state, m, ckpt, alive, num_seek_IP, max_iter_num, n_step)
    assert not oracle.march_rays_quadratic_bending.last_oob and (ref[2][:, 0] != 0).sum() > 500
    tail_rounds(rounds)
    _assert_same_bits(_device_march(state, m, ckpt, alive, num_seek_IP, max_iter_num, n_step), ref, f"{name} rounds {rounds}")


# ------------------------------------------------------------------------------------------------ (c) the in-cell order of full cells
@pytest.mark.parametrize("name", ["crowded", "squashed"])
def test_pnts_in_grids_bit_exact_on_state(states, name):
    from pienerf_amd.nerf.utils import get_pnts_in_grids
    p = states[name]["p_def"]
    t = ms.cell_table(p, states[name]["hash_grid_size"])
    got = get_pnts_in_grids(len(p), t["n_grid"], T(p), T(t["bbmin"]), T(t["bbmax"]), float(t["hgs"]), T(t["res"]))
    for a, b in zip(got, t["pig"]):
        assert np.array_equal(a.cpu().numpy(), b)
    assert t["pig"][0].max() >= (100 if name == "crowded" else 18)


# ------------------------------------------------------------------------------------------------ (d) whole frames against the oracle's
def _frame_rays():
    return oracle.get_rays(scene.orbit_pose(5.0, 20.0, -15.0), scene.orbit_intrinsics(FRAME_W, FRAME_W, 50.0), FRAME_W, FRAME_W)


def _oracle_frame(name, state, ckpt, opt):
    key = (name, opt["num_seek_IP"], opt["max_iter_num"], bool(opt.get("cut", False)))
    if key not in _oracle_frames:      # computed once, shared, never written to
        o, d = _frame_rays()
        _oracle_frames[key] = oracle.render_deformed(o, d, state, ckpt, opt)
    return _oracle_frames[key]


def _frame_against_the_oracle(name, state, ckpt, opt):
    o, d = _frame_rays()
    ref = _oracle_frame(name, state, ckpt, opt)
    net = _net(ckpt, state)
    with torch.no_grad():
        out = net.render_deformed(T(o)[None], T(d)[None], collect_stats=True, **opt)
    st = dict(net.last_stats)
    e_img = float(np.abs(out["image"][0].cpu().numpy() - ref["image"]).max())
    e_ws = float(np.abs(out["weights_sum"].cpu().numpy() - ref["weights_sum"]).max())
    print(f"{name} seek {opt['num_seek_IP']} iters {opt['max_iter_num']} cut {bool(opt.get('cut', False))}: {ref['samples']} samples, {ref['trips']} trips, "
          f"image max abs err {e_img:.2e}, weights_sum {e_ws:.2e}")
    assert ref["samples"] > 1000
    assert st["trips"] == ref["trips"] and st["samples"] == ref["samples"], (st, ref["trips"], ref["samples"])
    assert st["err"] == 0 and st["alive_at_exit"] == 0, st
    assert e_img < 1e-4 and e_ws < 1e-4, (e_img, e_ws)


@pytest.mark.parametrize("num_seek_IP,max_iter_num", FRAME_FORMS)
@pytest.mark.parametrize("name", ms.NAMES)
def test_frame_on_state(states, small_opt, ckpt, name, num_seek_IP, max_iter_num):
    _frame_against_the_oracle(name, states[name], ckpt, ms.frame_opt(small_opt, states[name], num_seek_IP=num_seek_IP, max_iter_num=max_iter_num))


@pytest.mark.parametrize("num_seek_IP,max_iter_num", FRAME_FORMS)
@pytest.mark.parametrize("name", ["crowded", "squashed"])
def test_cut_frame_on_state(states, small_opt, ckpt, name, num_seek_IP, max_iter_num):
    """--cut: the spatial hash spans +-bound, so the lists of `crowded` grow further; cut_bounds keep the whole body inside."""
    assert np.abs(states[name]["p_def"]).max() < 0.9
    opt = ms.frame_opt(small_opt, states[name], num_seek_IP=num_seek_IP, max_iter_num=max_iter_num, cut=True, cut_bounds=CUT_BOUNDS, max_steps=256)
    _frame_against_the_oracle(name, states[name], ckpt, opt)


# ------------------------------------------------------------------------------------------------ (e) the frame's forms agree, bit for bit
@pytest.mark.parametrize("name", ["crowded", "sparse"])
def test_frame_forms_agree_on_state(states, small_opt, ckpt, tail_rounds, skip_dda, name):
    state = states[name]
    o, d = _frame_rays()
    opt = ms.frame_opt(small_opt, state)
    net = _net(ckpt, state)

    def frame(rounds=None, dda=None, **kw):
        if rounds is not None:
            tail_rounds(rounds)
        if dda is not None:
            skip_dda(dda)
        with torch.no_grad():
            out = net.render_deformed(T(o)[None], T(d)[None], collect_stats=True, **dict(opt, **kw))
        res = (dict(net.last_stats), out["image"].clone(), out["depth_0"].clone())
        tail_rounds(0)
        skip_dda(-1)
        return res
    s0, i0, d0 = frame()
    assert s0["samples"] > 1000 and s0["err"] == 0 and s0["alive_at_exit"] == 0
    forms = [(f"march_throughput {thr}, trips {trips}", dict(march_throughput=thr, march_throughput_trips=trips)) for thr in (1, 64) for trips in (0, 3)]
    forms += [("ray_tile_w", dict(ray_tile_w=FRAME_W)), ("tail rounds 1", dict(rounds=1)), ("tail rounds 1000", dict(rounds=1000)),
              ("skip_dda 0", dict(dda=0)), ("skip_dda 1", dict(dda=1))]
    for what, kw in forms:
        s1, i1, d1 = frame(**kw)
        assert s1["samples"] == s0["samples"] and s1["err"] == 0 and s1["alive_at_exit"] == 0, (what, s0, s1)
        assert torch.equal(i1, i0) and torch.equal(d1, d0), what
