"""The static frame driver (NeRFRenderer.run_cuda in eval(): pn_render_static -> k_march_static_trip -> march_static_one<false, true>, the two-launch
k_composite / k_compact on trip_grid, k_frame_finish's depth normalisation, pn_render_continue with is_static) on the frames of tests/static_frames.py:
against the CPU oracle's image AND trip schedule, against the op-by-op loop run_cuda_ops, and against itself across fixed-trip renders, continuations,
workspaces and ray sets.

Bars (the project's own for these comparisons, tests/test_gpu_static.py and tests/test_gpu_trainloop.py): trips, samples, alive_at_exit and every
trip's (n_alive, n_step, samples) exact; image and weights_sum within 1e-4 of the oracle; depth with the oracle's NaN pattern and within 1e-4 where
finite; the frame driver equal to run_cuda_ops bit for bit.  fp16: the bars of tests/test_gpu_half.py::test_render_deformed_half_frame for the same
quantities against oracle.half_precision() — samples within 0.5 % + 8, image 1e-2 worst and 5e-4 on average, weights_sum 1e-2, depth 1e-2 relative.

`opts` and `all_miss` against the oracle "bit for bit": a pixel no sample reached is pure background — acc 0 + (1 - 0) * bg — and has the oracle's bits;
a composited pixel cannot have them (the device composites with v_exp_f32, the oracle with expf, the network sums in another order: that is what the
1e-4 bar is for), so for those the test holds the device to itself: the frame over bg equals the frame over 0 followed by the one blend, bit for bit.

What no GPU test ran before this module, numbered; each test names in its docstring the gaps it closes:
 1 continuation of a static frame, 2 the chunk loops of k_march_static_trip / k_composite / k_compact, 3 trip schedules with n_step 2..7, 4 margin trips
 that carry rays, 5 a frame that ends at max_steps with rays alive, 6 two cascades with dt_gamma > 0, 7 the fp16 frame, 8 ragged and tiny ray counts,
 9 a frame whose rays all miss, 10 a camera inside the box, 11 a workspace reused at another N.

What a plausible wrong kernel does to them: k_march_static_trip, k_composite or k_compact without the chunk loop lose the rays behind chunk 1024
(test_large_ray_set (a): the frame's rays are rolled so that those chunks hold the middle of the chair) or behind chunk 64 of a margin trip
(test_margin_trips_carry_most_of_the_frame); a sample slot n * 8 + s, a list base taken before the wave scan, or a scan that drops lane 0 change
the sample list of every trip with n_step in 2..7 (thin_close, inside, cascade_levels: records and images of test 1); dt_min from a fixed 1024 moves
every sample of out_of_steps; a mip level from the position alone misses cascade_levels' samples behind t = 2; a near clamped to the box face instead
of min_near moves every pixel of `inside`; (depth - near) / (far - near) guarded against 0 / 0 loses the NaNs of all_miss and the -0 of `behind`; a
workspace that keeps the longer frame's trip records, list or accumulators fails test_workspace_reuse's second and third frame.

Measured on the MI355X (printed by the tests): worst |image - oracle| per case 1.2e-7 .. 7.8e-7, weights_sum <= 8.9e-7, depth <= 1.3e-6 (bar 1e-4);
all_miss and behind 0; fp16 against the half oracle: thin_close samples equal (bar 1416), image 7.7e-6 worst / 2.2e-7 mean, weights_sum 3.1e-6, depth
5.0e-6 relative; far_chair samples equal (bar 106), image 6.0e-5 / 5.6e-8, weights_sum 6.0e-6, depth 1.8e-5 (bars 1e-2, 5e-4, 1e-2, 1e-2).

Two defects these tests found, fixed with them.  (1) render_continue(static=True) composited on into a NEW tensor for the un-normalised depth (run_cuda
returns the reference's three tensors, not that fourth): every continuation test failed, the books right and the finished frame not the blocking
frame's.  The renderer now keeps the accumulator with the frame workspace.  (2) A frame that ended at max_steps reported alive_at_exit 0 from the driver and 214 from run_cuda_ops and the oracle
("assert (15, 34538, 0) == (15, 34538, 214)"); the compaction now records the rays the step budget ended on (PnTrip::n_left) and the static
frame's status counts them.
"""
import contextlib

import numpy as np
import pytest
import torch

import static_frames as sf
from conftest import rel_err
from pienerf_amd import scene
from test_gpu_parity import DEV, T

pytestmark = pytest.mark.gpu
BAR = 1e-4


@pytest.fixture(scope="module")
def nets():
    """One network per distinct checkpoint, shared by the module's tests."""
    from pienerf_amd.nerf.network import NeRFNetwork
    made = {}

    def get(ck_args, fresh=False, bg_radius=-1):
        key = tuple(sorted(ck_args.items())) + (bg_radius,)
        if fresh or key not in made:
            ck = sf.checkpoint(ck_args) if bg_radius <= 0 else scene.make_checkpoint(bg_radius=bg_radius, **ck_args)
            net = NeRFNetwork(encoding="hashgrid", bound=ck_args["bound"], cuda_ray=True, bg_radius=bg_radius).to(DEV).load_checkpoint_dict(ck).eval()
            if fresh:
                return net
            made[key] = net
        return made[key]

    return get


def _ctx(case):
    return torch.autocast("cuda", dtype=torch.float16) if case["fp16"] else contextlib.nullcontext()


def _rays(case):
    o, d = sf.rays(case)
    return T(o)[None], T(d)[None]


def _render(net, case, o, d, ops=False, **kw):
    """run_cuda (the frame driver) or run_cuda_ops on the case -> (outputs, last_stats or None after a fixed-trip render)."""
    net.density_scale = case["density_scale"]
    with torch.no_grad(), _ctx(case):
        out = (net.run_cuda_ops if ops else net.run_cuda)(o, d, **sf.render_opts(case), **kw)
    return out, (None if kw.get("async_trips") else dict(net.last_stats))


def _continue(net, case, slot, o, d, out, n_trips):
    # whatever the render freed is taken and spoilt first: the continuation must go on from the frame's own accumulators (the un-normalised depth is not
    # among the three tensors run_cuda returns), not from memory that happens to hold them still
    spoil = [torch.full_like(out["depth"].reshape(-1), float("nan")) for _ in range(4)]
    with torch.no_grad(), _ctx(case):
        net.render_continue(slot, o, d, out, n_trips=n_trips, static=True, **sf.render_opts(case))
    del spoil
    return net.render_status(slot=slot) if n_trips else dict(net.last_stats)


def _same(a, b):
    """Bit for bit, NaN where the other has NaN."""
    a, b = a.reshape(-1), b.reshape(-1)
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(a[~na], b[~nb])


def _same_frame(a, b):
    return all(_same(a[k], b[k]) for k in ("image", "depth", "weights_sum"))


def _books(st):
    return (st["trips"], st["samples"], st["alive_at_exit"], st["err"])


def _clone(out):
    return {k: v.clone() for k, v in out.items()}


def _schedule(net, slot=0):
    """[(n_alive, n_step, samples)] of the last render on `slot`, from the device's trip records."""
    return [(r[0], r[1], r[3]) for r in net.trip_records(slot=slot, max_trips=160)]


def _alive_behind(ref, k):
    """Rays alive behind the first k trips of the oracle's frame."""
    return ref["record"][k][0] if k < len(ref["record"]) else ref["alive_at_exit"]


def _samples_of(ref, k):
    return sum(r[2] for r in ref["record"][:k])


def _against_oracle(name, out, ref, bar=BAR):
    img, ws, dep = out["image"].reshape(-1, 3).cpu().numpy(), out["weights_sum"].cpu().numpy(), out["depth"].reshape(-1).cpu().numpy()
    fin = np.isfinite(ref["depth"])
    e_img, e_ws = float(np.abs(img - ref["image"]).max()), float(np.abs(ws - ref["weights_sum"]).max())
    e_dep = float(np.abs(dep[fin] - ref["depth"][fin]).max()) if fin.any() else 0.0
    print(f"{name}: trips {ref['trips']}, samples {ref['samples']}, alive_at_exit {ref['alive_at_exit']}; worst |image| {e_img:.2e} |weights_sum| {e_ws:.2e} "
          f"|depth| {e_dep:.2e} (bar {bar:g}), NaN depths {int((~fin).sum())}")
    assert np.array_equal(np.isfinite(dep), fin), name
    assert e_img < bar and e_ws < bar and e_dep < bar, (name, e_img, e_ws, e_dep)
    return img, ws


# ------------------------------------------------------------------------------------------------ 1: every case against the oracle
FP32_CASES = [n for n in sf.CASES if not sf.CASES[n]["fp16"] and n not in sf.OPTS_NAMES]


@pytest.mark.parametrize("name", FP32_CASES)
def test_frame_and_schedule_match_oracle(name, nets):
    """Gaps 3 (thin_close, inside, cascade_levels: n_step takes 2..7 — the wave scan, the list append and the slot n * n_step + s), 5 (out_of_steps:
    alive_at_exit > 0, dt_min of max_steps = 20), 6 (cascade_levels: both cascades, dt_gamma > 0, through the driver), 8 (ragged_*: N = 1, 63, 65, 231,
    771), 9 (all_miss: every depth 0 / 0; behind: fars < nears), 10 (inside: near = min_near) and the axis-parallel ray (1 / d infinite).  The device's record of every trip —
    rays entering, samples per ray, samples listed — is the oracle's."""
    case, ref = sf.CASES[name], sf.reference(name)
    net = nets(case["ck"])
    out, st = _render(net, case, *_rays(case))
    got = _schedule(net)
    assert got == ref["record"], (name, got[:6], ref["record"][:6])
    assert (st["trips"], st["samples"], st["alive_at_exit"], st["err"]) == (ref["trips"], ref["samples"], ref["alive_at_exit"], 0), (name, st)
    img, _ = _against_oracle(name, out, ref)
    if name in ("all_miss", "behind"):
        assert np.array_equal(img, ref["image"])      # pure background, bit for bit


@pytest.mark.parametrize("ds,Tt", [(ds, Tt) for ds in (1.0, 0.5) for Tt in (1e-4, 0.3)])
def test_options_reach_the_frame(ds, Tt, nets):
    """bg_color x density_scale x T_thresh through pn_render_opts (the oracle's images differ between the settings: static_frames.check_opts_differ):
    schedule and stats exact, the frame within the bars, the uncovered pixels the oracle's bit for bit, and the frame over bg the frame over 0 followed
    by the one blend, bit for bit."""
    frames = {}
    for bg in (0.0, 0.3, 1.0):
        name = f"opts_bg{bg:g}_ds{ds:g}_T{Tt:g}"
        case, ref = sf.CASES[name], sf.reference(name)
        net = nets(case["ck"])
        out, st = _render(net, case, *_rays(case))
        assert _schedule(net) == ref["record"] and (st["trips"], st["samples"], st["alive_at_exit"]) == (ref["trips"], ref["samples"], 0), (name, st)
        img, ws = _against_oracle(name, out, ref)
        bare = ref["weights_sum"] == 0
        assert bare.sum() > 1000 and np.array_equal(ws[bare], ref["weights_sum"][bare]) and np.array_equal(img[bare], ref["image"][bare]), name
        frames[bg] = _clone(out)
    for bg in (0.3, 1.0):
        assert torch.equal(frames[bg]["weights_sum"], frames[0.0]["weights_sum"]) and _same(frames[bg]["depth"], frames[0.0]["depth"])
        blend = frames[0.0]["image"] + (1 - frames[0.0]["weights_sum"]).view(1, -1, 1) * bg
        assert torch.equal(frames[bg]["image"], blend), bg
        assert float((frames[bg]["image"] - frames[0.0]["image"]).abs().max()) > 0.29


@pytest.mark.parametrize("name", ["half_thin_close", "half_far_chair"])
def test_half_frame_matches_half_oracle(name, nets):
    """Gap 7: the fp16 static frame (what Trainer(fp16=True) evaluates through) against the oracle under oracle.half_precision(), with the bars and the
    sample-count treatment of tests/test_gpu_half.py::test_render_deformed_half_frame: the march is unchanged, a half ulp of a sigma logit can move a ray's
    T_thresh exit by a sample."""
    case, ref = sf.CASES[name], sf.reference(name)
    ref32 = sf.reference(name[len("half_"):])
    net = nets(case["ck"])
    out, st = _render(net, case, *_rays(case))
    got = _schedule(net)
    img, ws, dep = out["image"][0].cpu().numpy(), out["weights_sum"].cpu().numpy(), out["depth"][0].cpu().numpy()
    fin = np.isfinite(ref["depth"])
    e_max, e_mean, e_ws = float(np.abs(img - ref["image"]).max()), float(np.abs(img - ref["image"]).mean()), float(np.abs(ws - ref["weights_sum"]).max())
    e_dep = rel_err(dep[fin], ref["depth"][fin])
    print(f"{name}: trips {st['trips']} (oracle {ref['trips']}), samples {st['samples']} (oracle {ref['samples']}: off by {abs(st['samples'] - ref['samples'])}, "
          f"bar {0.005 * ref['samples'] + 8:.0f}); image worst {e_max:.2e} (bar 1e-2) mean {e_mean:.2e} (bar 5e-4), weights_sum worst {e_ws:.2e} (bar 1e-2), "
          f"depth rel {e_dep:.2e} (bar 1e-2), n_step set {sf.n_steps(dict(record=got))}; against the fp32 oracle: worst {np.abs(img - ref32['image']).max():.2e}")
    assert got[0] == ref["record"][0] and st["err"] == 0                   # the first trip's march does not see the network
    assert abs(st["samples"] - ref["samples"]) <= 0.005 * ref["samples"] + 8 and st["alive_at_exit"] == 0
    assert np.array_equal(np.isfinite(dep), fin)
    assert e_max < 1e-2 and e_mean < 5e-4 and e_ws < 1e-2 and e_dep < 1e-2
    plain, _ = _render(net, sf.CASES[name[len("half_"):]], *_rays(case))
    assert not torch.equal(out["image"], plain["image"])                   # fp16 really is in effect: not the fp32 frame's bits


# ------------------------------------------------------------------------------------------------ 2: the driver against the op loop
@pytest.mark.parametrize("name", ["thin_close", "inside", "cascade_levels", "out_of_steps"] + list(sf.RAGGED_NAMES))
def test_driver_equals_op_loop(name, nets):
    """Gaps 3, 5, 6, 8, 10 once more, against the same kernels driven from the host: bit for bit, alive_at_exit included (out_of_steps: the rays
    max_steps ended the loop on — the driver used to report 0 there)."""
    case = sf.CASES[name]
    net = nets(case["ck"])
    o, d = _rays(case)
    a, sa = _render(net, case, o, d)
    b, sb = _render(net, case, o, d, ops=True)
    print(f"{name}: driver {sa}, op loop {sb}")
    assert (sa["trips"], sa["samples"], sa["alive_at_exit"]) == (sb["trips"], sb["samples"], sb["alive_at_exit"]), (name, sa, sb)
    assert sa["alive_at_exit"] == sf.reference(name)["alive_at_exit"]
    assert _same_frame(a, b), name


# ------------------------------------------------------------------------------------------------ 3: continuation
def _continuation(net, case, ref, ks, o, d, slot=0):
    whole, st_whole = _render(net, case, o, d, frame_slot=slot)
    whole = _clone(whole)
    for k in ks:
        out, _ = _render(net, case, o, d, async_trips=k, frame_slot=slot)
        st = net.render_status(slot=slot)
        if ref is not None:
            assert (st["alive_at_exit"], st["samples"], st["trips"]) == (_alive_behind(ref, k), _samples_of(ref, k), min(k, ref["trips"])), (k, st)
        st = _continue(net, case, slot, o, d, out, 2)
        if ref is not None:
            assert (st["alive_at_exit"], st["samples"]) == (_alive_behind(ref, k + 2), _samples_of(ref, k + 2)), (k, st)
        st = _continue(net, case, slot, o, d, out, 0)
        assert (st["trips"], st["samples"], st["alive_at_exit"]) == (st_whole["trips"], st_whole["samples"], st_whole["alive_at_exit"]), (k, st, st_whole)
        assert _same_frame(out, whole), k
    return whole, st_whole


@pytest.mark.parametrize("name", ["thin_close", "cascade_levels"])
def test_static_frame_continues(name, nets):
    """Gap 1 (render_impl mode 2, render_continue(static=True)) with gap 4's margin trips in every fixed-trip render of three trips or more: after k
    trips the status is the oracle's record — rays alive behind trip k, samples of the first k — then two more trips, then a blocking continuation;
    the finished frame is the blocking frame bit for bit.  A frame that had already finished is left as it is."""
    case, ref = sf.CASES[name], sf.reference(name)
    net = nets(case["ck"])
    o, d = _rays(case)
    needed = ref["trips"]
    whole, st_whole = _continuation(net, case, ref, (1, 3, needed - 1), o, d)
    assert (st_whole["trips"], st_whole["samples"]) == (needed, ref["samples"])
    out, _ = _render(net, case, o, d, async_trips=needed + 2)
    st = net.render_status()
    assert (st["alive_at_exit"], st["samples"], st["trips"]) == (0, ref["samples"], needed) and _same_frame(out, whole)
    st = _continue(net, case, 0, o, d, out, 1)
    assert (st["alive_at_exit"], st["samples"], st["trips"]) == (0, ref["samples"], needed) and _same_frame(out, whole)


def test_half_static_frame_continues(nets):
    """Gaps 1 and 7: the continuation reads the autocast state as the render does."""
    case = sf.CASES["half_far_chair"]
    net = nets(case["ck"])
    o, d = _rays(case)
    whole, st = _continuation(net, case, None, (1, 2), o, d)
    plain, _ = _render(net, sf.CASES["far_chair"], o, d)
    assert st["alive_at_exit"] == 0 and not torch.equal(whole["image"], plain["image"])


def test_static_frame_with_background_model_continues(nets):
    """Gap 1 with bg_radius > 0: the continuation's epilogue composites over 0 again and the model's colour is blended in again, once."""
    case = sf.CASES["thin_close"]
    net = nets(case["ck"], bg_radius=32.0)
    o, d = _rays(case)
    whole, st = _continuation(net, case, None, (3,), o, d)
    bare, _ = _render(nets(case["ck"]), dict(case, bg_color=0.0), o, d)
    assert torch.equal(whole["weights_sum"], bare["weights_sum"])
    assert float((whole["image"] - bare["image"]).abs().max()) > 0.05          # the model's colour is there ...
    assert bool((whole["image"] >= bare["image"]).all())                       # ... added, never taken away


# ------------------------------------------------------------------------------------------------ 4: margin trips with rays in them
def test_margin_trips_carry_most_of_the_frame(nets):
    """Gap 4 (and 2 on the 64-workgroup grids): 160 x 120 rays of thin_close's scene rendered with async_trips = 3 — trips 1 and 2 are margin trips
    (64 workgroups for the march, the network and the composite / compaction pair) with more than 64 x 256 rays alive, so every chunk loop wraps.
    Status against the oracle's first three trips; the blocking continuation gives the blocking frame bit for bit."""
    case, rec = sf.MARGIN, sf.margin_record(3)
    assert rec[1][0] > 64 * 256 and rec[2][0] > 64 * 256
    net = nets(case["ck"])
    o, d = _rays(case)
    whole, st_whole = _render(net, case, o, d)
    whole = _clone(whole)
    out, _ = _render(net, case, o, d, async_trips=3)
    st = net.render_status()
    print(f"margin frame: oracle {rec}, status {st}")
    assert _schedule(net)[:3] == rec[:3]
    assert (st["alive_at_exit"], st["samples"], st["trips"]) == (rec[3][0], sum(r[2] for r in rec[:3]), 3), (st, rec)
    st = _continue(net, case, 0, o, d, out, 0)
    assert (st["trips"], st["samples"], st["alive_at_exit"]) == (st_whole["trips"], st_whole["samples"], 0) and _same_frame(out, whole)


# ------------------------------------------------------------------------------------------------ 5: out of steps through the fixed-trip form
@pytest.mark.parametrize("extra", [0, 2])
def test_out_of_steps_with_a_fixed_trip_count(extra, nets):
    """Gap 5 through pn_render_static's fixed-trip form and pn_render_continue: the step budget is spent, not the trips — the rays left are reported,
    the frame is the blocking frame bit for bit, and a blocking continuation changes nothing."""
    case, ref = sf.CASES["out_of_steps"], sf.reference("out_of_steps")
    net = nets(case["ck"])
    o, d = _rays(case)
    whole, st_whole = _render(net, case, o, d)
    whole = _clone(whole)
    assert st_whole["alive_at_exit"] == ref["alive_at_exit"] > 0
    out, _ = _render(net, case, o, d, async_trips=ref["trips"] + extra)
    st = net.render_status()
    assert (st["alive_at_exit"], st["samples"], st["trips"]) == (ref["alive_at_exit"], ref["samples"], ref["trips"]), st
    assert _same_frame(out, whole)
    st = _continue(net, case, 0, o, d, out, 0)
    assert (st["alive_at_exit"], st["samples"], st["trips"]) == (ref["alive_at_exit"], ref["samples"], ref["trips"]), st
    assert _same_frame(out, whole) and _schedule(net) == ref["record"]


# ------------------------------------------------------------------------------------------------ 6: more than 262 144 rays
def test_large_ray_set(nets):
    """Gap 2: 528 x 500 = 264 000 rays, more than trip_grid's 1024 chunks of 256, so the chunk loops of k_march_static_trip and of the k_composite /
    k_compact pair wrap on the first trip.  (a) the driver equals run_cuda_ops bit for bit; (b) every 89th ray rendered as a frame of its own on another
    workspace has the big frame's pixels bit for bit — tests/test_static_frames_host.py shows on the oracle that a ray's pixel does not depend on its
    frame; (c) that subset is within 1e-4 of the oracle's frame of it (the oracle never renders the big frame); (d) the books of the big frame."""
    case = sf.LARGE
    net = nets(case["ck"])
    o, d = _rays(case)
    N = o.shape[1]
    # the first trip takes the rays in the order given, and the last rows of the image see only background: the frame's rays rolled by half the image,
    # so that the chunks behind the 1024th, the wrapped ones, hold the rows through the middle of the chair
    o, d = torch.roll(o, N // 2, dims=1).contiguous(), torch.roll(d, N // 2, dims=1).contiguous()
    a, sa = _render(net, case, o, d)
    rec = net.trip_records(max_trips=160)
    a = _clone(a)
    b, sb = _render(net, case, o, d, ops=True)
    assert N == 264000 and (sa["trips"], sa["samples"], sa["alive_at_exit"]) == (sb["trips"], sb["samples"], 0) and sb["alive_at_exit"] == 0, (sa, sb)
    assert _same_frame(a, b)
    assert int((a["weights_sum"][1024 * 256:] > 0.5).sum()) > 100          # the wrapped chunks carry part of the chair
    assert rec[0][:2] == (N, 1) and sum(r[3] for r in rec) == sa["samples"] and len(rec) == sa["trips"], (rec, sa)
    so, sd = o[:, ::89].contiguous(), d[:, ::89].contiguous()
    part, sp = _render(net, case, so, sd, frame_slot=1)
    assert sp["alive_at_exit"] == 0 and sp["samples"] > 3000
    for k in ("image", "depth"):
        assert _same(part[k], a[k][:, ::89]), k
    assert torch.equal(part["weights_sum"], a["weights_sum"][::89])
    ref = sf.render(case, so[0].cpu().numpy(), sd[0].cpu().numpy())
    assert (sp["trips"], sp["samples"]) == (ref["trips"], ref["samples"]) and _schedule(net, slot=1) == ref["record"]
    _against_oracle("large frame, every 89th ray", part, ref)
    print(f"large frame: {sa}, first trips {rec[:3]}")


# ------------------------------------------------------------------------------------------------ 7: workspace reuse
@pytest.mark.parametrize("slot", [0, 3])
def test_workspace_reuse(slot, nets):
    """Gap 11: one workspace takes thin_close (122 trips), out_of_steps (the same N, 4 trips: the long frame's records lie behind them), ragged 33 x 7
    (another N) and thin_close again.  The first, a repeat of it and the last are the same bits with the same trip records; the frames between equal
    a fresh model's; nothing of a frame's records, lists or accumulators survives into the next."""
    big, cut, small = sf.CASES["thin_close"], sf.CASES["out_of_steps"], sf.CASES["ragged_33x7"]
    net, fresh = nets(big["ck"]), nets(big["ck"], fresh=True)
    ob, db = _rays(big)
    osm, dsm = _rays(small)
    first, st1 = _render(net, big, ob, db, frame_slot=slot)
    first, rec1 = _clone(first), _schedule(net, slot)
    again, st1b = _render(net, big, ob, db, frame_slot=slot)
    assert _same_frame(again, first) and _books(st1b) == _books(st1) and _schedule(net, slot) == rec1
    for case, o, d in ((cut, ob, db), (small, osm, dsm)):
        mid, stm = _render(net, case, o, d, frame_slot=slot)
        recm = _schedule(net, slot)
        want, stw = _render(fresh, case, o, d)
        assert _same_frame(mid, want) and _books(stm) == _books(stw) and recm == _schedule(fresh) == sf.reference("out_of_steps" if case is cut else "ragged_33x7")["record"]
    last, st3 = _render(net, big, ob, db, frame_slot=slot)
    assert _same_frame(last, first) and _books(st3) == _books(st1) and _schedule(net, slot) == rec1 == sf.reference("thin_close")["record"]
