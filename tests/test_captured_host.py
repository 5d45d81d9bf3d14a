"""pienerf_amd/_captured.py on hand-made values: which error a replay raises when the current state has left what the capture baked in, and which
one comes first.  No harness, no GPU."""
import pytest

from pienerf_amd._captured import STAGE_NOT_CAPTURED, Captured, refuse_form

OVERLAY = (4096, b"style", None)                          # state address, style bytes, t_max
SHADOWED = OVERLAY + (b"light", 8192, 12288)              # ... with cast_shadows(): the light's bytes and the map buffers' addresses
POINTS = (None, (40.0, 40.0, 16.0, 16.0), 32, 32, b"style", None, None)


def rec(stages=("drag",), overlay=None, points=None, form_epoch=0):
    return Captured(frozenset(stages), overlay, points, form_epoch)


def check(captured, now, kind="graph"):
    captured.check_substep(now, kind)
    captured.check_render(now, kind)


@pytest.mark.parametrize("kind", ["graph", "pipe"])
def test_equal_records_pass(kind):
    check(rec(), rec(), kind)
    check(rec(("drag", "contact"), SHADOWED, POINTS, 3), rec(("contact", "drag"), SHADOWED, POINTS, 3), kind)


@pytest.mark.parametrize("stage,enable", [("pins", "enable_pin_motion"), ("contact", "enable_contact"), ("bodies", "enable_bodies"), ("fields", "enable_fields"),
                                          ("self", "enable_self_contact")])
def test_a_stage_enabled_after_the_capture_raises_its_own_message(stage, enable):
    with pytest.raises(RuntimeError) as e:
        rec().check_substep(rec(("drag", stage)), "graph")
    assert str(e.value) == STAGE_NOT_CAPTURED[stage].format(what="the step graph", again="capture()")
    assert f"captured before {enable}()" in str(e.value) and str(e.value).endswith(": capture() again")
    with pytest.raises(RuntimeError, match=rf"the pipeline was captured before {enable}\(\).*: capture_pipelined\(\) again"):
        rec().check_substep(rec(("drag", stage)), "pipe")
    assert len({m.split(",")[1] for m in STAGE_NOT_CAPTURED.values()}) == len(STAGE_NOT_CAPTURED)   # each stage says what its substep ignores


def test_a_captured_stage_that_is_now_off_does_not_raise():
    check(rec(("drag", "pins", "contact", "bodies", "fields", "self")), rec(()))


def test_overlay():
    with pytest.raises(RuntimeError, match=r"colliders: the step graph was captured before draw_colliders\(\)"):
        check(rec(), rec(overlay=OVERLAY))
    with pytest.raises(RuntimeError, match=r"colliders: the pipeline was captured before cast_shadows\(\), its frames cast no shadows: capture_pipelined\(\) again"):
        check(rec(overlay=OVERLAY), rec(overlay=SHADOWED), "pipe")
    with pytest.raises(RuntimeError, match="colliders: the overlay .* changed since the step graph was captured"):
        check(rec(overlay=OVERLAY), rec(overlay=(4096, b"other", None)))
    with pytest.raises(RuntimeError, match="changed since"):   # set, then removed: now != captured
        check(rec(overlay=OVERLAY), rec())
    with pytest.raises(RuntimeError, match="changed since"):   # shadows hidden again: shorter, so not "before cast_shadows"
        check(rec(overlay=SHADOWED), rec(overlay=OVERLAY))


def test_points():
    with pytest.raises(RuntimeError, match=r"points: the step graph was captured before draw_points\(\)"):
        check(rec(), rec(points=POINTS))
    with pytest.raises(RuntimeError, match="points: the point overlay .* changed since the pipeline was captured"):
        check(rec(points=POINTS), rec(points=POINTS[:2] + (64, 64) + POINTS[4:]), "pipe")
    with pytest.raises(RuntimeError, match="points: .* changed since"):
        check(rec(points=POINTS), rec())


def test_form_epoch():
    with pytest.raises(RuntimeError, match=r"another arithmetic form \(pn_net_form\) since the step was captured: .* capture again"):
        check(rec(), rec(form_epoch=1))
    with pytest.raises(RuntimeError, match="since the pipeline was captured: .* capture again"):
        check(rec(form_epoch=2), rec(form_epoch=1), "pipe")


def test_precedence():
    now = rec(("drag", "contact"), OVERLAY, POINTS, 1)
    with pytest.raises(RuntimeError, match="capture again"):                            # net form, then stages, then colliders, then points
        check(rec(), now)
    with pytest.raises(RuntimeError, match="captured before enable_contact"):          # a new stage and a new overlay: the stage's message
        check(rec(form_epoch=1), now)
    with pytest.raises(RuntimeError, match="captured before draw_colliders"):
        check(rec(("drag", "contact"), form_epoch=1), now)
    with pytest.raises(RuntimeError, match="captured before draw_points"):
        check(rec(("drag", "contact"), OVERLAY, form_epoch=1), now)


def test_refusals_of_a_form():
    both = rec(overlay=OVERLAY, points=POINTS)
    for form, what in (("frame_parallel", "the frame-parallel pipeline"), ("staged", "the staged form"),
                       ("parallel_or_staged", "the frame-parallel / staged pipeline"), ("tile_parallel", "the tile-parallel form")):
        with pytest.raises(RuntimeError, match=f"colliders: {what} does not draw the colliders"):
            refuse_form(form, both, True, True)
        with pytest.raises(RuntimeError, match=f"points: {what} does not draw the points"):
            refuse_form(form, rec(points=POINTS), True, True)
    refuse_form("tile_parallel", rec(), True, True)       # no pipeline: shadows and balls are not its business
    refuse_form("pipelined", both, False, False)
    refuse_form("pipelined", rec(), False, True)
    with pytest.raises(RuntimeError, match="shadows: the pipelined form casts no shadows"):   # shadows before the balls
        refuse_form("pipelined", both, True, True)
    with pytest.raises(RuntimeError, match="bodies: the pipelined form draws the live collider state"):
        refuse_form("staged", rec(overlay=None), False, True) or refuse_form("pipelined", both, False, True)
