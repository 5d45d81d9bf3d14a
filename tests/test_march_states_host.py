"""The IP states of tests/march_states.py on the CPU oracle alone: each state has the properties it is built for (`facts`), and the reference
arithmetic — the oracle's march and its whole frame — digests it: finite outputs, samples enough to mean something.  This is also the guard
that tests/test_gpu_march_states.py feeds the kernels nothing the reference itself could not take."""
import numpy as np
import pytest

import march_states as ms
import oracle
from pienerf_amd import scene

MARCH_FORMS = [(1, 1, 8), (3, 5, 8)]   # (num_seek_IP, max_iter_num, n_step)


@pytest.fixture(scope="module")
def states(deformed_ip_state, small_opt):
    return {name: ms.build(name, deformed_ip_state, small_opt) for name in ms.NAMES}


@pytest.fixture(scope="module")
def coincident(deformed_ip_state, small_opt, ckpt):
    return ms.coincident(deformed_ip_state, small_opt, ckpt)


@pytest.mark.parametrize("name", ms.NAMES)
def test_state_has_the_properties_it_is_built_for(states, deformed_ip_state, name):
    state, facts = states[name]
    print(name, facts)
    ms.check_facts(name, facts)
    assert set(deformed_ip_state) <= set(state) and "hash_grid_size" in state
    n = len(state["p_def"])
    assert state["p_ori"].shape == (n, 3) and state["F"].shape == (n, 9) and state["dF"].shape == (n, 27)


def test_the_base_state_is_none_of_this(deformed_ip_state, small_opt):
    """What the issue measured on the fixture every render test used to share — the reason these states exist."""
    t = ms.cell_table(deformed_ip_state["p_def"], small_opt["hash_grid_size"])
    assert t["own"].max() < 10 and t["lists"].max() < 64
    assert (ms.det_f32(deformed_ip_state["F"]) > 0.1).all()
    assert len(np.unique(deformed_ip_state["p_def"], axis=0)) == len(deformed_ip_state["p_def"])


@pytest.mark.parametrize("num_seek_IP,max_iter_num,n_step", MARCH_FORMS)
@pytest.mark.parametrize("name", ms.NAMES)
def test_oracle_march_digests_the_state(states, ckpt, name, num_seek_IP, max_iter_num, n_step):
    state, _ = states[name]
    m = ms.march_inputs(state)
    alive = np.nonzero(m["nears"] < 1e30)[0].astype(np.int32)
    xyzs, dirs, deltas = ms.oracle_march(state, m, ckpt, alive, num_seek_IP, max_iter_num, n_step)
    assert not oracle.march_rays_quadratic_bending.last_oob
    emitted = int((deltas[:, 0] != 0).sum())
    print(f"{name} seek {num_seek_IP} iters {max_iter_num}: {emitted} samples emitted")
    assert np.isfinite(xyzs).all() and np.isfinite(dirs).all() and np.isfinite(deltas).all()
    assert emitted > 200


@pytest.mark.parametrize("num_seek_IP,max_iter_num", [(1, 1), (3, 5)])
@pytest.mark.parametrize("name", ms.NAMES)
def test_oracle_frame_digests_the_state(states, small_opt, ckpt, name, num_seek_IP, max_iter_num):
    state, _ = states[name]
    W = 64
    o, d = oracle.get_rays(scene.orbit_pose(5.0, 20.0, -15.0), scene.orbit_intrinsics(W, W, 50.0), W, W)
    ref = oracle.render_deformed(o, d, state, ckpt, ms.frame_opt(small_opt, state, num_seek_IP=num_seek_IP, max_iter_num=max_iter_num))
    print(f"{name} seek {num_seek_IP} iters {max_iter_num}: {ref['samples']} samples in {ref['trips']} trips")
    for k in ("image", "weights_sum", "depth_0"):
        assert np.isfinite(ref[k]).all(), k
    assert ref["samples"] > 1000


def test_coincident_samples_lie_on_their_points(coincident):
    state, rays, facts = coincident
    print("coincident", facts)
    ms.check_facts("coincident", facts)
    for k in ("p_def", "p_ori", "F", "dF"):
        assert state[k].dtype == np.float32 and np.isfinite(state[k]).all()
    sample = rays["o"] + rays["t"][:, None] * rays["d"]
    assert np.array_equal(sample.view(np.uint32), state["p_def"][rays["ips"]].view(np.uint32))
    # ... also when the compiler contracts o + t * d into one fma (one rounding of the exact sum: the same here, t * d being exact)
    fma = (rays["o"].astype(np.float64) + rays["t"][:, None].astype(np.float64) * rays["d"].astype(np.float64)).astype(np.float32)
    assert np.array_equal(fma.view(np.uint32), sample.view(np.uint32))


@pytest.mark.parametrize("num_seek_IP,max_iter_num", [(1, 1), (2, 1), (3, 1), (3, 5)])
def test_oracle_march_digests_coincident(coincident, ckpt, num_seek_IP, max_iter_num):
    """32 rays, n_step = 1: the first sample of (nearly) every ray is emitted.  With one IP sought the sample at d == 0 warps to that IP's rest
    position exactly: through the ray's own IP — the lower id of a pair at d == 0, the IP at d == 0 beside a lower id at d^2 = 2^-140."""
    state, rays, _ = coincident
    m = ms.coincident_inputs(state, rays)
    xyzs, dirs, deltas = ms.oracle_march(state, m, ckpt, rays["alive"], num_seek_IP, max_iter_num, 1, rays_t=rays["t"])
    assert not oracle.march_rays_quadratic_bending.last_oob
    emitted = deltas[:32, 0] != 0
    print(f"coincident seek {num_seek_IP} iters {max_iter_num}: {int(emitted.sum())} of 32 samples emitted")
    assert np.isfinite(xyzs).all() and np.isfinite(deltas).all()
    assert emitted.sum() >= 24
    if num_seek_IP == 1:
        first = deltas[:32, 1] < 1.5 * deltas[:32, 0]                 # emitted at rays_t itself, not further along the ray
        assert emitted.all() and first.all()
        assert np.array_equal(xyzs[:32].view(np.uint32), state["p_ori"][rays["ips"]].view(np.uint32))
