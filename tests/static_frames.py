"""Named static frames (NeRFRenderer.run_cuda in eval(): pn_render_static, k_march_static_trip, the k_composite / k_compact pair, k_frame_finish's
depth normalisation, pn_render_continue on a static frame) and the CPU oracle's account of each: image, depth, weights_sum AND the trip schedule
[(n_alive, n_step, samples)] with the rays the loop left alive, which oracle.render_static does not return.  numpy + the CPU oracle only; a helper
module, not a conftest.

`reference(name)` restates oracle.render_static's loop from the oracle.* ops (the same calls in the same order) so that it can keep the per-trip
record, the count of rays alive when the loop ended and the sample positions; `agrees_with_render_static` holds the restatement against
oracle.render_static itself.  `check_facts(name, ref)` asserts, on the oracle alone, the edge a case exists for: an edit to a case, to
pienerf_amd/scene.py or to the oracle that quietly loses the edge fails tests/test_static_frames_host.py.

Every number in the facts was measured on the CPU oracle; the cases are frozen.

A case that was planned and is not here: `two_cascades` with the fact "at least 100 samples with max(abs(xyz)) > 1".  No camera can meet it:
scene.make_checkpoint marks a cell of either cascade occupied only where its centre lies within one cell of the chair, which ends at |x| = 0.84, so
no sample of any frame lies beyond 0.9.  `cascade_levels` is that frame (bound 2, dt_gamma 1 / 128, max_steps 300, the n_step set {1, 2, 3, 4, 6, 8})
with the fact that CAN hold about two cascades here: the march looks a sample up on level max(mip_from_pos, mip_from_dt) (raymarching.cu:43-55), dt =
t / 128 passes the first cascade's cell size at t = 2, and the chair spans t = 1.7 .. 3.3 — at least 1000 samples on each level.
"""
import time

import numpy as np

import oracle
from pienerf_amd import scene

FAR_CHAIR_CK = dict(bound=1.0, shaped=True, sigma_target=60.0, seed=0)      # tests/test_gpu_static.py's checkpoint: a solid chair
THIN_CK = dict(bound=1.0, shaped=False, sigma_target=2.0, seed=0)           # a thin medium inside the chair's bitfield: rays live for many trips
INSIDE_CK = dict(bound=1.0, shaped=False, sigma_target=1.0, seed=0)
TWO_CASCADES_CK = dict(bound=2.0, shaped=False, sigma_target=2.0, seed=0)


def _case(ck, radius, az, el, fovy, W, H, fact, dt_gamma=0.0, max_steps=1024, T_thresh=1e-2, bg_color=1.0, density_scale=1.0, fp16=False, turned=None,
          axis=None):
    return dict(ck=ck, radius=radius, az=az, el=el, fovy=fovy, W=W, H=H, dt_gamma=dt_gamma, max_steps=max_steps, T_thresh=T_thresh, bg_color=bg_color,
                density_scale=density_scale, fp16=fp16, turned=turned, axis=axis, fact=fact)


FAR_CHAIR = _case(FAR_CHAIR_CK, 4.0, 40.0, -20.0, 50.0, 80, 60, "far_chair")
THIN_CLOSE = _case(THIN_CK, 1.3, 30.0, -25.0, 40.0, 64, 48, "thin_close", T_thresh=1e-4)
RAGGED_SIZES = ((1, 1), (33, 7), (257, 3), (63, 1), (65, 1))      # N = 1 | 231 | 771 | 63 | 65: below a wave, ragged against 64 and 256, three chunks
OPTS_GRID = tuple((bg, ds, T) for bg in (0.0, 0.3, 1.0) for ds in (1.0, 0.5) for T in (1e-4, 0.3))

CASES = {
    "far_chair": FAR_CHAIR,
    "thin_close": THIN_CLOSE,
    "inside": _case(INSIDE_CK, 0.5, 30.0, -25.0, 60.0, 48, 48, "inside", T_thresh=1e-4),
    "cascade_levels": _case(TWO_CASCADES_CK, 2.5, 30.0, -25.0, 40.0, 64, 48, "cascade_levels", dt_gamma=1.0 / 128, max_steps=300, T_thresh=1e-4),
    "out_of_steps": dict(THIN_CLOSE, max_steps=20, fact="out_of_steps"),
    # far_chair's camera turned a quarter round about its own up axis: no ray's line meets the box, forwards or backwards, so nears == fars everywhere ...
    "all_miss": dict(FAR_CHAIR, turned="side", fact="all_miss"),
    # ... and turned right round (pose[:3, :3] = -pose[:3, :3], as tests/test_gpu_edges.py does): the box lies BEHIND a third of the rays, fars < nears there
    "behind": dict(FAR_CHAIR, turned="round", fact="behind"),
    "half_thin_close": dict(THIN_CLOSE, fp16=True),
    "half_far_chair": dict(FAR_CHAIR, fp16=True),
    # the ray through the centre pixel runs along +z exactly: two direction components are 0, 1 / d is infinite, the empty-voxel hop forms 0 * inf
    "axis_ray": _case(FAR_CHAIR_CK, 3.0, 0.0, 0.0, 30.0, 33, 25, "axis_ray", axis=(0.1, -0.05)),
}
for _w, _h in RAGGED_SIZES:
    CASES[f"ragged_{_w}x{_h}"] = dict(THIN_CLOSE, W=_w, H=_h, fact="ragged")
for _bg, _ds, _T in OPTS_GRID:
    CASES[f"opts_bg{_bg:g}_ds{_ds:g}_T{_T:g}"] = dict(FAR_CHAIR, bg_color=_bg, density_scale=_ds, T_thresh=_T, fact="opts")
OPTS_NAMES = tuple(n for n in CASES if n.startswith("opts_"))
RAGGED_NAMES = tuple(n for n in CASES if n.startswith("ragged_"))

# frames whose whole oracle render no test needs (they are compared with the op loop, and a subset of their rays with the oracle)
MARGIN = dict(THIN_CLOSE, W=160, H=120, fact=None)     # 19 200 rays: trips 1 and 2 keep more than 64 x 256 of them alive (checked on the CPU march)
LARGE = dict(FAR_CHAIR, W=528, H=500, fact=None)       # 264 000 rays > 1024 x 256: the chunk loops of a static frame's full-size grids wrap


# ------------------------------------------------------------------------------------------------ inputs
_CKPTS = {}


def checkpoint(ck_args):
    """scene.make_checkpoint(**ck_args), built once per distinct argument set and shared (read only)."""
    key = tuple(sorted(ck_args.items()))
    if key not in _CKPTS:
        _CKPTS[key] = scene.make_checkpoint(**ck_args)
    return _CKPTS[key]


def rays(case):
    """(rays_o, rays_d) [H * W, 3] of the case's camera."""
    W, H = case["W"], case["H"]
    if case["axis"] is not None:
        # identity rotation, the principal point in the middle of the centre pixel of an odd-sized image: (i + 0.5 - cx) / fx == 0 there, exactly
        assert W % 2 == 1 and H % 2 == 1
        pose = np.eye(4, dtype=np.float32)
        pose[:3, 3] = [case["axis"][0], case["axis"][1], -case["radius"]]
        intr = scene.orbit_intrinsics(W, H, case["fovy"])
        intr[2], intr[3] = W / 2.0, H / 2.0
    else:
        pose = scene.orbit_pose(case["radius"], case["az"], case["el"])
        if case["turned"] == "round":
            pose[:3, :3] = -pose[:3, :3]
        elif case["turned"] == "side":
            pose[:3, :3] = pose[:3, :3] @ np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], np.float32)
        intr = scene.orbit_intrinsics(W, H, case["fovy"])
    return oracle.get_rays(pose, intr, H, W)


def render_opts(case):
    """The keyword arguments run_cuda / run_cuda_ops / render_continue take for the case."""
    return dict(dt_gamma=case["dt_gamma"], max_steps=case["max_steps"], T_thresh=case["T_thresh"], bg_color=case["bg_color"])


# ------------------------------------------------------------------------------------------------ the oracle's frame and its schedule
def render(case, o, d, max_trips=None):
    """oracle.render_static's loop (NeRFRenderer.run_cuda, inference branch, renderer.py:267-387) restated from the oracle's ops, keeping what it drops:
    record [(n_alive, n_step, samples)] per trip, alive_at_exit (the rays alive when `step` reached max_steps, 0 otherwise), nears / fars, and the
    number of samples the march looked up on each cascade level (`levels`).  max_trips: stop behind that many trips, as a fixed-trip render does
    (alive_at_exit: the rays alive there)."""
    ck = dict(checkpoint(case["ck"]), density_scale=case["density_scale"])
    o, d = np.ascontiguousarray(o, np.float32).reshape(-1, 3), np.ascontiguousarray(d, np.float32).reshape(-1, 3)
    N, bound, max_steps = o.shape[0], float(ck["bound"]), int(case["max_steps"])
    with oracle.half_precision(case["fp16"]):
        aabb = np.array([-bound] * 3 + [bound] * 3, np.float32)
        nears, fars = oracle.near_far_from_aabb(o, d, aabb, ck["min_near"])
        ws, depth, image = np.zeros(N, np.float32), np.zeros(N, np.float32), np.zeros((N, 3), np.float32)
        alive, rays_t = np.arange(N, dtype=np.int32), nears.copy()
        step, record, levels = 0, [], np.zeros(int(ck["cascade"]), np.int64)
        while step < max_steps and alive.shape[0] > 0 and (max_trips is None or len(record) < max_trips):
            n_alive = alive.shape[0]
            n_step = max(min(N // n_alive, 8), 1)
            xyzs, dirs, deltas = oracle.march_rays(n_alive, n_step, alive, rays_t, o, d, bound, ck["density_bitfield"], ck["cascade"], ck["grid_size"], nears,
                                                   fars, 128, None, float(case["dt_gamma"]), max_steps)
            live = deltas[:, 0] != 0
            sig, rgb = np.zeros(len(xyzs), np.float32), np.zeros((len(xyzs), 3), np.float32)
            if live.any():
                sig[live], rgb[live] = oracle.nerf_forward(xyzs[live], dirs[live], ck, bound)
                levels += np.bincount(_levels(xyzs[live], deltas[live, 0], ck["grid_size"], ck["cascade"]), minlength=len(levels))
            sig = np.float32(ck["density_scale"]) * sig
            oracle.composite_rays(n_alive, n_step, alive, rays_t, sig, rgb, deltas, ws, depth, image, float(case["T_thresh"]))
            alive = oracle.compact_rays(alive)
            record.append((n_alive, n_step, int(live.sum())))
            step += n_step
    image = image + (1 - ws)[:, None] * np.float32(case["bg_color"])
    with np.errstate(invalid="ignore", divide="ignore"):
        depth = np.maximum(depth - nears, 0) / (fars - nears)
    return dict(image=image.astype(np.float32), depth=depth.astype(np.float32), weights_sum=ws, trips=len(record), samples=sum(r[2] for r in record),
                record=record, alive_at_exit=int(alive.shape[0]), nears=nears, fars=fars, levels=[int(v) for v in levels])


def _levels(xyz, dt, H, C):
    """The cascade level of each sample: max(mip_from_pos(x, y, z), mip_from_dt(dt)), both the exponent of frexpf clamped to [0, C - 1]
    (raymarching.cu:43-55)."""
    e_pos = np.frexp(np.abs(xyz).max(axis=1).astype(np.float32))[1]
    e_dt = np.frexp((dt.astype(np.float32) * np.float32(H)).astype(np.float64) * 0.5)[1]
    return np.clip(np.maximum(e_pos, e_dt), 0, C - 1).astype(np.int64)


_REFS = {}


def reference(name):
    """render(CASES[name]) on the case's own rays, computed once and shared (read only); `seconds`: what the oracle took."""
    if name not in _REFS:
        case = CASES[name]
        o, d = rays(case)
        t0 = time.perf_counter()
        ref = render(case, o, d)
        ref["seconds"] = time.perf_counter() - t0
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REFS[name] = ref
    return _REFS[name]


def agrees_with_render_static(name):
    """The restated loop against oracle.render_static itself: image, depth, weights_sum bit for bit, trips and samples equal."""
    case, ref = CASES[name], reference(name)
    o, d = rays(case)
    ck = dict(checkpoint(case["ck"]), density_scale=case["density_scale"])
    with oracle.half_precision(case["fp16"]):
        own = oracle.render_static(o, d, ck, dict(dt_gamma=case["dt_gamma"], max_steps=case["max_steps"], T_thresh=case["T_thresh"]), case["bg_color"])
    assert own["trips"] == ref["trips"] and own["samples"] == ref["samples"], (name, own["trips"], ref["trips"], own["samples"], ref["samples"])
    for k in ("image", "depth", "weights_sum"):
        assert np.array_equal(own[k], ref[k], equal_nan=True), (name, k)


def n_steps(ref):
    return sorted({r[1] for r in ref["record"]})


def describe(name, ref):
    return (f"{name}: N {len(ref['weights_sum'])}, trips {ref['trips']}, n_step set {n_steps(ref)}, samples {ref['samples']}, alive_at_exit "
            f"{ref['alive_at_exit']}, samples per cascade level {ref['levels']}, first trips {ref['record'][:4]}, oracle {ref['seconds']:.2f} s")


def check_facts(name, ref):
    """What the case is there for, asserted on the oracle alone (the table of the module's cases)."""
    case = CASES[name]
    N, steps, rec = case["W"] * case["H"], n_steps(ref), ref["record"]
    assert len(ref["weights_sum"]) == N and rec[0][:2] == (N, 1) and ref["trips"] == len(rec) and ref["samples"] == sum(r[2] for r in rec)
    assert all(r[1] == max(min(N // r[0], 8), 1) for r in rec)
    fact = case["fact"]
    if fact == "far_chair":                      # today's shape: one sample per ray, then eight (also under fp16)
        assert steps == [1, 8] and ref["alive_at_exit"] == 0 and ref["samples"] > 3000
    elif fact == "thin_close":                   # every schedule the slot arithmetic n * n_step + s can see (also under fp16)
        assert steps == [1, 2, 3, 4, 5, 6, 7, 8] and ref["alive_at_exit"] == 0, steps
        if not case["fp16"]:
            assert ref["trips"] == 122, ref["trips"]
    elif fact == "inside":                       # the camera inside the box: near = min_near
        assert steps == [1, 2, 3, 4, 5, 6, 7, 8] and ref["alive_at_exit"] == 0, steps
        assert (ref["nears"] == np.float32(checkpoint(case["ck"])["min_near"])).mean() >= 0.9
    elif fact == "cascade_levels":
        assert {2, 3, 4, 6} <= set(steps) and len(ref["levels"]) == 2 and min(ref["levels"]) >= 1000, (steps, ref["levels"])
        assert checkpoint(case["ck"])["cascade"] == 2 and case["dt_gamma"] > 0 and ref["alive_at_exit"] == 0
    elif fact == "out_of_steps":                 # the loop ends on `step`, with rays alive, behind a trip that started below max_steps
        total = sum(r[1] for r in rec)
        assert ref["alive_at_exit"] > 0 and total >= case["max_steps"] and total - rec[-1][1] < case["max_steps"], (ref["alive_at_exit"], rec)
        assert case["max_steps"] % 8 != 0
    elif fact == "all_miss":                     # nears == fars: 0 / 0
        assert ref["samples"] == 0 and ref["trips"] == 1 and np.isnan(ref["depth"]).all()
        assert np.array_equal(ref["image"], np.full((N, 3), np.float32(case["bg_color"])))
    elif fact == "behind":                       # no sample either; 0 / 0 where the line misses the box, 0 / (fars - nears) < 0 = -0 where the box is behind
        nan = np.isnan(ref["depth"])
        assert ref["samples"] == 0 and ref["trips"] == 1 and 0.2 * N < nan.sum() < 0.8 * N
        assert (ref["fars"][~nan] < ref["nears"][~nan]).all() and (ref["depth"][~nan] == 0).all() and np.signbit(ref["depth"][~nan]).all()
    elif fact == "ragged":
        assert (N % 64 != 0 or N < 64) and N % 256 != 0
        assert ref["samples"] > 0 or N == 1, (name, ref["samples"])
    elif fact == "opts":
        assert steps == [1, 8] and ref["alive_at_exit"] == 0
    elif fact == "axis_ray":
        o, d = rays(case)
        c = (case["H"] // 2) * case["W"] + case["W"] // 2
        assert d[c, 0] == 0 and d[c, 1] == 0 and d[c, 2] == 1, d[c]
        assert ref["seconds"] < 1.0 and ref["weights_sum"][c] > 0.5, (ref["seconds"], ref["weights_sum"][c])
    else:
        raise AssertionError(f"{name}: no fact named")


def check_opts_differ():
    """`opts`: every one of bg_color, density_scale, T_thresh moves the image by more than 1e-3 somewhere, at every setting of the other two."""
    img = {k: reference(f"opts_bg{k[0]:g}_ds{k[1]:g}_T{k[2]:g}")["image"] for k in OPTS_GRID}
    worst = np.inf
    for a in OPTS_GRID:
        for b in OPTS_GRID:
            if a < b and sum(x != y for x, y in zip(a, b)) == 1:
                diff = float(np.abs(img[a] - img[b]).max())
                worst = min(worst, diff)
                assert diff > 1e-3, (a, b, diff)
    return worst


_MARGIN = {}


def margin_record(k):
    """The first k trips of the MARGIN frame on the oracle -> its record + [(the rays alive behind trip k, 0, 0)]."""
    if k not in _MARGIN:
        o, d = rays(MARGIN)
        r = render(MARGIN, o, d, max_trips=k)
        _MARGIN[k] = r["record"] + [(r["alive_at_exit"], 0, 0)]
    return _MARGIN[k]


def subset_frame(case, o, d, stride):
    """The oracle's frame of every stride-th ray alone."""
    return render(case, o[::stride], d[::stride])
