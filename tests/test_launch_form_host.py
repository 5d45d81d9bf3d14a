"""The launch form of a pipeline's frames from plain values (pienerf_amd/pipeline_hip.py): trip records written by hand as
(n_alive, n_step, step_base, n_samples, n_emitted, n_tail).  No harness, no GPU."""
import itertools

import pytest

from pienerf_amd.pipeline_hip import THROUGHPUT_FORM_MIN_RAYS, fused_from_of, fused_grid_of, throughput_trips_of, try_fused_fold, try_fused_whole


def trip(n_alive, n_step):
    return (n_alive, n_step, 0, n_alive * n_step, n_alive * n_step // 2, 0)


@pytest.mark.parametrize("steps,want", [((8, 4, 8, 8), 2),      # record 0 never counts
                                        ((1, 8, 8), 1),
                                        ((1, 2, 4, 4), -1),
                                        ((8,), -1),
                                        ((), -1)])
def test_fused_from(steps, want):
    recs = [trip(4096 >> i, s) for i, s in enumerate(steps)]
    assert fused_from_of(recs, None) == want and fused_from_of(recs, 0) == want
    assert fused_from_of(recs, 4096) == -1      # a frame in ray batches: never


@pytest.mark.parametrize("first", [1, 131071, 640000])
def test_throughput_trips(first):
    assert THROUGHPUT_FORM_MIN_RAYS == 131072
    assert throughput_trips_of([trip(first, 1), trip(131072, 1), trip(131072, 2), trip(131071, 4), trip(131072, 8)]) == 3
    assert throughput_trips_of([trip(first, 1), trip(131071, 2), trip(131072, 4)]) == 1
    assert throughput_trips_of([trip(first, 1)]) == 1


def test_fused_grid():
    assert fused_grid_of(2, 256) == 160
    assert fused_grid_of(3, 256) == 128 and fused_grid_of(4, 256) == 128
    assert fused_grid_of(2, 1) == 1 and fused_grid_of(3, 1) == 1


def test_what_is_tried():
    for lanes, fused_from in itertools.product((1, 2, 3, 4), (-1, 0, 1, 2)):
        assert try_fused_whole(lanes, fused_from) == (lanes == 2 and fused_from == 1)
        for whole, order in itertools.product((False, True), (None, False, True, 0, 1)):
            want = lanes >= 3 and not whole and fused_from == 1 and order is not None and not order
            assert bool(try_fused_fold(lanes, whole, fused_from, order)) == want, (lanes, whole, fused_from, order)
    assert try_fused_fold(3, False, 1, False) and try_fused_fold(3, None, 1, 0)       # folded only in list order, asked for explicitly
    assert not try_fused_fold(3, False, 1, None) and not try_fused_fold(3, True, 1, False) and not try_fused_fold(2, False, 1, False)
