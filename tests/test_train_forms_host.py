"""The inputs and the yardstick of tests/test_gpu_train_forms.py, proved on the CPU: the designed composite batch of train_forms_cases.py reaches every
window, carry and window edge of the wave-per-ray composite with many rays; the padding keeps offsets and counts; and the project's fp32 oracle stays
within ORACLE_VS_F64 of the float64 autograd reference, in per-ray / per-sample units, from which the GPU bars are derived."""
import numpy as np
import pytest

import train_forms_cases as tfc
from oracle import training as otr


@pytest.fixture(scope="module", params=tfc.T_THRESHES)
def case(request):
    T_thresh = request.param
    b = tfc.composite_cases(T_thresh, np.random.default_rng(tfc.SEED))
    ref = tfc.composite_ref64(b["sigmas"], b["rgbs"], b["deltas"], b["rays"], T_thresh, b["grad_weights_sum"], b["grad_image"])
    return T_thresh, b, ref


def test_designed_batch_covers_every_window_and_edge(case):
    T_thresh, b, ref = case
    lens, ex = b["rays"][:, 2], ref["exit"]
    assert np.array_equal(ex, b["walls"])                     # T crosses the threshold at the wall and nowhere else
    assert sorted(b["rays"][:, 0]) == list(range(len(lens)))
    assert (ex == 63).sum() >= 8 and (ex == 64).sum() >= 8    # last lane of a window / first lane of the next
    assert (ex == 127).sum() >= 8 and (ex == 128).sum() >= 8
    assert (ex >= 256).sum() >= 8                             # an exit in the fifth window or later
    assert ((lens >= 257) & (ex < 0)).sum() >= 8              # five windows and more carried to the end
    assert (ex == 0).sum() >= 8 and ((lens == 1) & (ex < 0)).sum() >= 8
    assert ref["margin"].min() >= 1.0                         # no ray's exit depends on the precision it is computed in
    # the figures of the design: 16 / 16 / 48 / 16, log-margin 2.2
    assert ((ex == 63).sum(), (ex == 64).sum(), (ex >= 128).sum(), ((lens >= 257) & (ex < 0)).sum()) == (16, 16, 48, 16)
    assert ref["margin"].min() >= 2.2
    # every sample up to the exit is written, none after it
    owner = tfc.sample_rows(b["rays"], len(b["sigmas"]))
    step = np.arange(len(owner)) - b["rays"][owner, 1]
    assert np.array_equal(ref["written"], (ex[owner] < 0) | (step <= ex[owner]))


def test_oracle_within_recorded_distance_of_float64(case):
    T_thresh, b, ref = case
    ws, depth, image = otr.composite_rays_train_forward(b["sigmas"], b["rgbs"], b["deltas"], b["rays"], T_thresh)
    gs, gc = otr.composite_rays_train_backward(b["grad_weights_sum"], b["grad_image"], b["sigmas"], b["rgbs"], b["deltas"], b["rays"], ws, image, T_thresh)
    got = dict(weights_sum=ws, depth=depth, image=image, grad_sigmas=gs, grad_rgbs=gc)
    err = tfc.composite_errors(got, ref, b["rays"], b["deltas"], b["grad_weights_sum"], b["grad_image"], ref["written"])
    worst = {k: float(v.max()) for k, v in err.items()}
    print(f"oracle vs float64, T_thresh {T_thresh:g}: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= tfc.ORACLE_VS_F64[T_thresh][k], (k, v)
        assert v >= 0.25 * tfc.ORACLE_VS_F64[T_thresh][k], (k, v)   # the recorded figure is the measured one, not a loose cap
    # the oracle leaves what the op does not write alone (its caller zero-fills), exactly
    assert not gs[~ref["written"]].any() and not gc[~ref["written"]].any()


def test_reference_gradients_are_the_derivatives(case):
    """composite_ref64's gradients against central differences of its own forward, on a few samples of the longest walled ray."""
    T_thresh, b, ref = case
    rays = b["rays"]
    n = int(np.nonzero((rays[:, 2] == 513) & (b["walls"] == 300))[0][0])
    row = rays[n:n + 1].copy()
    off, L = int(row[0, 1]), int(row[0, 2])
    idx = int(row[0, 0])
    row[0, :2] = 0
    sig, rgb, dl = (b[k][off:off + L].astype(np.float64) for k in ("sigmas", "rgbs", "deltas"))
    gws, gim = b["grad_weights_sum"][idx:idx + 1].astype(np.float64), b["grad_image"][idx:idx + 1].astype(np.float64)

    def loss(s):
        r = tfc.composite_ref64(s, rgb, dl, row, T_thresh, gws, gim)
        return r["weights_sum"][0] * gws[0] + (r["image"][0] * gim[0]).sum()

    for i in (0, 64, 299, 300):
        h = 1e-4 * max(sig[i], 1.0)
        sp, sm = sig.copy(), sig.copy()
        sp[i] += h
        sm[i] -= h
        fd = (loss(sp) - loss(sm)) / (2 * h)
        want = ref["grad_sigmas"][off + i]
        unit = dl[i, 0] * (np.abs(gim[0]).sum() + abs(gws[0]))
        assert abs(fd - want) <= 1e-6 * unit, (i, fd, want)
    assert not ref["grad_sigmas"][off + 301:off + L].any()


@pytest.mark.parametrize("N_total", [tfc.WAVE_FORM_MAX_N, tfc.WAVE_FORM_MAX_N + 77])
def test_padding_keeps_the_designed_rows(case, N_total):
    T_thresh, b, ref = case
    rays = b["rays"]
    padded, pos = tfc.pad_rows(rays, N_total, np.random.default_rng(1))
    assert padded.shape == (N_total, 3) and np.array_equal(padded[pos, 1:], rays[:, 1:])
    assert sorted(padded[:, 0]) == list(range(N_total))
    dead = np.ones(N_total, bool)
    dead[pos] = False
    assert not padded[dead, 2].any() and np.array_equal(padded[:, 1], np.cumsum(padded[:, 2]) - padded[:, 2])
    # front, across a multiple of 128 in the middle, and the batch's very last rows; above the threshold the last block is a partial one
    assert pos[0] == 0 and pos[-1] == N_total - 1 and np.all(np.diff(pos) > 0)
    mid = pos[(pos > 1000) & (pos < N_total - 1000)]
    assert len(mid) > 16 and (mid % 128 == 0).any() and mid.min() % 128 != 0
    if N_total > tfc.WAVE_FORM_MAX_N:
        assert N_total % 128 != 0 and (pos >= N_total // 128 * 128).sum() >= 16
    # the oracle on the padded rows gives the designed rays' values at their new indices and zeros elsewhere
    ws0, _, im0 = otr.composite_rays_train_forward(b["sigmas"], b["rgbs"], b["deltas"], rays, T_thresh)
    ws1, _, im1 = otr.composite_rays_train_forward(b["sigmas"], b["rgbs"], b["deltas"], padded, T_thresh)
    assert np.array_equal(ws1[padded[pos, 0]], ws0[rays[:, 0]]) and np.array_equal(im1[padded[pos, 0]], im0[rays[:, 0]])
    assert not ws1[padded[dead, 0]].any() and not im1[padded[dead, 0]].any()
