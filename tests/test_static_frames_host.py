"""The static frames of tests/static_frames.py on the CPU oracle alone: every case still has the edge it exists for, and the property the large-frame
GPU test rests on — a ray's pixel does not depend on the frame it is rendered in — holds on the oracle bit for bit.  No GPU.

Measured on the oracle (printed by the tests): far_chair n_step {1, 8}; thin_close 122 trips with n_step 1..8; inside 110 trips with n_step 1..8 and
every near at min_near; cascade_levels n_step {1, 2, 3, 4, 6, 8} with samples in both cascades; out_of_steps 214 rays alive when `step` reaches 20;
axis_ray (two direction components exactly 0, 1 / d infinite) returns in a fraction of a second with samples on the axis ray.
"""
import numpy as np
import pytest

import static_frames as sf


@pytest.mark.parametrize("name", list(sf.CASES))
def test_case_keeps_its_edge(name):
    ref = sf.reference(name)
    print(sf.describe(name, ref))
    sf.check_facts(name, ref)


def test_opts_move_the_image():
    worst = sf.check_opts_differ()
    print(f"opts: smallest image difference between two settings that differ in one option {worst:.3e}")


@pytest.mark.parametrize("name", ["far_chair", "cascade_levels", "out_of_steps", "behind", "half_far_chair", "opts_bg0.3_ds0.5_T0.3"])
def test_restated_loop_agrees_with_render_static(name):
    """static_frames.render keeps what oracle.render_static drops; everything both return is the same, bit for bit."""
    sf.agrees_with_render_static(name)


def _far_chair_96():
    return dict(sf.FAR_CHAIR, W=96, H=96)


@pytest.mark.parametrize("name", ["far_chair_96", "thin_close"])
def test_a_rays_pixel_does_not_depend_on_its_frame(name):
    """While no ray is cut off by max_steps (alive_at_exit == 0): the march continues from rays_t, the composite stops at the same sample whatever the
    chunking into trips, the sums are sequential per ray.  So the oracle's frame of every 7th ray equals those rows of the whole frame — image,
    weights_sum, depth — BIT FOR BIT, though the two frames run different trip schedules.  tests/test_gpu_static_frames.py holds a 264 000-ray frame
    to the oracle through this property."""
    case = _far_chair_96() if name == "far_chair_96" else sf.CASES[name]
    o, d = sf.rays(case)
    whole, part = sf.render(case, o, d), sf.subset_frame(case, o, d, 7)
    assert whole["alive_at_exit"] == 0 and part["alive_at_exit"] == 0 and part["samples"] > 300
    assert [r[1] for r in whole["record"]] != [r[1] for r in part["record"]]          # different schedules
    print(f"{name}: whole {whole['trips']} trips {sf.n_steps(whole)}, every 7th ray {part['trips']} trips {sf.n_steps(part)}")
    for k in ("image", "weights_sum", "depth"):
        assert np.array_equal(whole[k][::7], part[k], equal_nan=True), k


def test_out_of_steps_pixels_do_depend_on_the_schedule():
    """The guard of the test above: where max_steps cuts rays off, the same rays in another frame get other pixels.  Every 7th ray alone would not
    show it — nearly all of them hit, as in the whole frame, and both frames march one sample per trip until step 20 — so they share their frame with
    the rays of the all_miss camera: from the second trip on the schedule is eight samples per trip, and the loop ends at step 25 instead of 20."""
    case = sf.CASES["out_of_steps"]
    o, d = sf.rays(case)
    mo, md = sf.rays(sf.CASES["all_miss"])
    n = len(o[::7])
    whole, part = sf.reference("out_of_steps"), sf.render(case, np.concatenate([o[::7], mo]), np.concatenate([d[::7], md]))
    assert whole["alive_at_exit"] > 0 and [r[1] for r in part["record"]] == [1, 8, 8, 8]
    assert not np.array_equal(whole["image"][::7], part["image"][:n]) and not np.array_equal(whole["weights_sum"][::7], part["weights_sum"][:n])
    # the same mixed frame with max_steps out of the way: the pixels of the whole frame again, bit for bit
    free = sf.CASES["thin_close"]
    whole, part = sf.reference("thin_close"), sf.render(free, np.concatenate([o[::7], mo]), np.concatenate([d[::7], md]))
    for k in ("image", "weights_sum", "depth"):
        assert np.array_equal(whole[k][::7], part[k][:n], equal_nan=True), k


def test_margin_and_large_frames_are_what_their_gpu_tests_need():
    """MARGIN: trips 1 and 2 of the 160 x 120 frame have more than 64 x 256 rays alive, so the 64-workgroup grids of a fixed-trip render's margin trips
    wrap their chunk loops.  Counted with the march alone, which is all that decides it while T_thresh is far away: a ray is alive behind a trip when
    it filled every slot.  LARGE: more rays than 1024 chunks of 256."""
    case = sf.MARGIN
    rec = sf.margin_record(3)
    print(f"margin frame: first trips {rec}")
    assert rec[0][0] == case["W"] * case["H"] == 19200 and rec[1][0] > 64 * 256 and rec[2][0] > 64 * 256, rec
    assert sf.LARGE["W"] * sf.LARGE["H"] == 264000 > 1024 * 256
