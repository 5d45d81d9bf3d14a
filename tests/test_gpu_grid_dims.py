"""The stand-alone hash-grid op (csrc/pn_grid_op.hip) is one template family over the input dimension D = 2, 3, 4, 5: every D through the same
forward / rows-forward / dy_dx / backward / total-variation kernels, against the D-generic CPU oracle (oracle/grid_nd_oracle.cpp), on a hand-built
level table that holds every index form (fully dense, partly strided, hashed into 2^k, hashed into a size that is no power of two), and the
backward's wave-level fold of equal rows on inputs built to make runs (whole waves in one cell, alternating cells, out-of-range lanes inside a run)."""
import functools

import numpy as np
import pytest
import torch

import oracle
from pienerf_amd._lib import check, lib, ptr, stream_ptr
from test_gpu_parity import DEV, T

pytestmark = pytest.mark.gpu

PLS, BASE, L = 2.0, 4, 4          # scales 3, 7, 15, 31; resolutions 4, 8, 16, 32
S = float(np.float32(np.log2(PLS)))


def level_table(D, align):
    """Offsets of four levels: all D dims strided; D - 1 dims strided (tiled grids; a hash grid hashes it, modulo a size that is no power of two);
    128 = 2^7 entries (the mask path); 1000 entries (the modulo path; gridencoder.grid.level_table_offsets never makes such a size)."""
    side = [r + (0 if align else 1) for r in (4, 8, 16, 32)]
    sizes = [side[0] ** D, side[1] ** (D - 2) + 3, 128, 1000]
    assert side[1] ** (D - 2) <= sizes[1] < side[1] ** (D - 1) and sizes[2] < side[2] ** D and sizes[3] < side[3] ** D
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def forward(x, emb, off, D, C, gridtype, align, interp, rows, with_dy_dx):
    B = x.shape[0]
    out = torch.full((B, L * C) if rows else (L, B, C), np.nan, device=DEV)
    dy = torch.full((B, L * D * C), np.nan, device=DEV) if with_dy_dx else None
    check(lib().pn_grid_encode_forward(ptr(x), ptr(emb), off.ctypes.data, ptr(out), B, D, C, L, S, BASE, ptr(dy), gridtype, int(align), interp, int(rows),
                                       stream_ptr()), "grid_encode_forward")
    return out, dy


def backward(grad_lbc, x, emb, off, D, C, gridtype, align, interp, dy):
    B = x.shape[0]
    ge = torch.zeros_like(emb)
    gi = torch.full((B, D), np.nan, device=DEV) if dy is not None else None
    check(lib().pn_grid_encode_backward(ptr(grad_lbc), ptr(x), ptr(emb), off.ctypes.data, ptr(ge), B, D, C, L, S, BASE, ptr(dy), ptr(gi), gridtype, int(align),
                                        interp, stream_ptr()), "grid_encode_backward")
    return ge, gi


@pytest.mark.parametrize("C,gridtype,align,interp", [(1, 0, False, 0), (2, 1, True, 1), (8, 0, False, 1)])
@pytest.mark.parametrize("D", [2, 3, 4, 5])
def test_every_input_dim_through_one_path(D, C, gridtype, align, interp):
    """B = 300 (two workgroups, the second ragged).  Both output layouts and the forward with and without dy_dx are the same bits; the forward is
    within 2e-6 * max(1, |ref|) of the oracle (test_grid_encode_matches_oracle's bar) and dy_dx within 1e-5 relative (test_gpu_ref's); samples out
    of range are exactly zero in the outputs, in dy_dx and in grad_inputs."""
    off = level_table(D, align)
    rng = np.random.default_rng(100 + D)
    emb_np = rng.uniform(-1, 1, (int(off[-1]), C)).astype(np.float32)
    B = 300
    x_np = rng.uniform(0, 1, (B, D)).astype(np.float32)
    x_np[0], x_np[1], x_np[2], x_np[3] = 0.0, 1.0, 0.5, 0.999999
    x_np[4, 0], x_np[5, D - 1] = -0.1, 1.2
    grad_np = rng.standard_normal((L, B, C)).astype(np.float32)
    x, emb = T(x_np), T(emb_np)
    y_lbc, dy = forward(x, emb, off, D, C, gridtype, align, interp, False, True)
    y_rows, dy_rows = forward(x, emb, off, D, C, gridtype, align, interp, True, True)
    y_lbc_plain, _ = forward(x, emb, off, D, C, gridtype, align, interp, False, False)
    y_rows_plain, _ = forward(x, emb, off, D, C, gridtype, align, interp, True, False)
    _, gi = backward(T(grad_np), x, emb, off, D, C, gridtype, align, interp, dy)
    torch.cuda.synchronize()
    assert torch.equal(y_lbc.permute(1, 0, 2).reshape(B, L * C), y_rows)
    assert torch.equal(y_lbc, y_lbc_plain) and torch.equal(y_rows, y_rows_plain) and torch.equal(dy, dy_rows)
    want_y, want_dy = oracle.grid_nd_forward(x_np, emb_np, off, PLS, BASE, gridtype, align, interp, dy_dx=True)
    err_y, err_dy = np.abs(y_rows.cpu().numpy() - want_y).max(), np.abs(dy.cpu().numpy() - want_dy).max()
    print(f"D={D} C={C}: forward {err_y:.3g} (|ref| {np.abs(want_y).max():.3g}), dy_dx {err_dy:.3g} (|ref| {np.abs(want_dy).max():.3g})")
    assert np.abs(want_y).max() > 0.1 and np.abs(want_dy).max() > 0.1
    assert err_y <= 2e-6 * max(1.0, np.abs(want_y).max())
    assert err_dy <= 1e-5 * np.abs(want_dy).max()
    assert not y_rows[4:6].any() and not y_lbc[:, 4:6].any() and not dy[4:6].any() and not gi[4:6].any()
    assert torch.isfinite(gi).all() and gi[6:].abs().max() > 0


@functools.lru_cache(maxsize=None)
def run_fold_case(D, C):
    """130 samples = two full waves and a two-lane tail.  Lanes 0-63: one cell of the coarsest level (0.4 in every coordinate, jittered by 1e-4, so they
    share their cell at every level: 0.4 * scale + 0.5 has a fraction of 0.3 .. 0.9 at all four).  Lanes 64-127: that cell and the one at 0.8 in turn.
    Lanes 5 and 70 are out of range: they break a run and add nothing.  Returns the inputs and the oracle's gradients, computed once, shared and read-only."""
    off = level_table(D, False)
    rng = np.random.default_rng(200 + D)
    emb = rng.uniform(-1, 1, (int(off[-1]), C)).astype(np.float32)
    B = 130
    x = rng.uniform(0, 1, (B, D)).astype(np.float32)
    x[:128] = 0.4
    x[65:128:2] = 0.8
    x[:128] += rng.uniform(-1e-4, 1e-4, (128, D)).astype(np.float32)
    x[5, 0], x[70, D - 1] = -0.1, 1.2
    grad = rng.standard_normal((B, L * C)).astype(np.float32)
    _, dy = oracle.grid_nd_forward(x, emb, off, PLS, BASE, 0, False, 0, dy_dx=True)
    gi, ge = oracle.grid_nd_backward(grad, x, emb.shape, off, PLS, BASE, dy, 0, False, 0)
    tv = oracle.grid_nd_grad_tv(x, emb, off, 0.3, PLS, BASE, 0, False)
    # the rows the runs share carry the gradient: per level at most 2 cells x 2^D corners for lanes 0-127, plus the tail's two cells
    for lvl in range(L):
        rows = np.abs(ge[off[lvl]:off[lvl + 1]]).max(axis=1) > 0
        assert 0 < rows.sum() <= 4 * 2 ** D, (lvl, int(rows.sum()))
        assert np.abs(tv[off[lvl]:off[lvl + 1]]).max() > 0
    for a in (off, emb, x, grad, dy, gi, ge, tv):
        a.setflags(write=False)
    return off, emb, x, grad, dy, gi, ge, tv


@pytest.mark.parametrize("D,C", [(2, 1), (3, 2), (4, 4), (5, 8)])
def test_backward_folds_runs_of_equal_rows_for_every_input_dim(D, C):
    """grad_embeddings, grad_inputs and the total-variation gradient on the run-making inputs, within 1e-4 * |ref|.max() of the oracle (the bar of
    test_grid_encode_other_input_dims_equal_the_reference_kernel: the sums meet in another order than the oracle's)."""
    off, emb_np, x_np, grad_np, dy_np, gi_o, ge_o, tv_o = run_fold_case(D, C)
    B = x_np.shape[0]
    x, emb = T(x_np.copy()), T(emb_np.copy())   # copies: torch.from_numpy wants writable memory
    grad = T(grad_np.reshape(B, L, C).transpose(1, 0, 2))
    ge, gi = backward(grad, x, emb, off, D, C, 0, False, 0, T(dy_np.copy()))
    tv = torch.zeros_like(emb)
    check(lib().pn_grad_total_variation(ptr(x), ptr(emb), ptr(tv), off.ctypes.data, 0.3, B, D, C, L, S, BASE, 0, 0, stream_ptr()), "grad_total_variation")
    torch.cuda.synchronize()
    errs = [float(np.abs(a.cpu().numpy() - b).max() / np.abs(b).max()) for a, b in ((ge, ge_o), (gi, gi_o), (tv, tv_o))]
    print(f"D={D} C={C}: grad_embeddings {errs[0]:.3g}, grad_inputs {errs[1]:.3g}, grad_tv {errs[2]:.3g} (relative to |ref|.max())")
    assert max(errs) <= 1e-4
    assert not gi[5].any() and not gi[70].any()
    assert not ge.cpu().numpy()[np.abs(ge_o).max(axis=1) == 0].any()


def test_half_backward_folds_runs_of_equal_rows():
    """kernel_grid_backward<at::Half> at D = 3, C = 2 on the same 130 samples: against the fp32 oracle on the half-rounded gradients with the bars of
    test_grid_encode_backward_under_autocast — every entry within 2^-6 x the sum of its contributions' magnitudes, 1e-2 of the largest entry overall,
    untouched rows exactly zero."""
    D, C = 3, 2
    off, emb_np, x_np, grad_np, _, _, _, _ = run_fold_case(D, C)
    B = x_np.shape[0]
    grad_h = (grad_np * 1e-2).astype(np.float16)
    _, ge_r = oracle.grid_nd_backward(grad_h.astype(np.float32), x_np, emb_np.shape, off, PLS, BASE, None, 0, False, 0)
    _, ge_abs = oracle.grid_nd_backward(np.abs(grad_h.astype(np.float32)), x_np, emb_np.shape, off, PLS, BASE, None, 0, False, 0)
    x = T(x_np.copy())
    grad = T(grad_h.reshape(B, L, C).transpose(1, 0, 2))
    ge = torch.zeros(emb_np.shape, device=DEV, dtype=torch.float16)
    check(lib().pn_grid_encode_backward_half(ptr(grad), ptr(x), off.ctypes.data, ptr(ge), B, D, C, L, S, BASE, 0, 0, 0, stream_ptr()),
          "grid_encode_backward_half")
    torch.cuda.synchronize()
    got = ge.float().cpu().numpy()
    assert np.isfinite(got).all() and np.abs(ge_r).max() > 1e-2
    print(f"half backward: worst excess over 2^-6 sum|terms| {float((np.abs(got - ge_r) - 2.0 ** -6 * ge_abs).max()):.3g}, "
          f"relative {float(np.abs(got - ge_r).max() / np.abs(ge_r).max()):.3g}")
    assert (np.abs(got - ge_r) <= 2.0 ** -6 * ge_abs + 1e-6).all()
    assert np.abs(got - ge_r).max() / np.abs(ge_r).max() < 1e-2
    assert not got[ge_abs == 0].any()
