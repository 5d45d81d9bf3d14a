"""Connected components on CPU (no kernel is launched): the C ABI entry is declared, exported and bound; its argument checks (they return before
anything is enqueued); select_components on CPU tensors against a numpy restatement; the --con options of the three front ends."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

PN_ERR_ARG = 1


def test_entry_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "pienerf_hip.h")).read()
    assert "int pn_ccl_label(const uint8_t* occ, int nx, int ny, int nz, int connectivity, int* labels, void* stream);" in header
    from pienerf_amd import _lib
    assert "pn_ccl_label" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["pn_ccl_label"]
    assert res is ctypes.c_int and len(args) == 7
    assert hasattr(_lib.lib(), "pn_ccl_label")
    from pienerf_amd import build
    assert "pn_components.hip" in build.UNITS


def test_ccl_label_refuses_bad_arguments_before_enqueueing():
    from pienerf_amd import _lib
    h, d = _lib.lib(), ctypes.c_void_p(256)
    assert h.pn_ccl_label(None, 4, 4, 4, 26, d, None) == PN_ERR_ARG           # no occupancy
    assert h.pn_ccl_label(d, 4, 4, 4, 26, None, None) == PN_ERR_ARG           # no labels
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (4, -3, 4), (4, 4, -2)):   # a side < 1
        assert h.pn_ccl_label(d, *dims, 26, d, None) == PN_ERR_ARG, dims
    for dims in ((1 << 11, 1 << 10, 1 << 10), (1, 2, 1 << 30), (65536, 65536, 1), (0x7fffffff, 0x7fffffff, 0x7fffffff), (46341, 46341, 1),
                 (1291, 1291, 1291)):                                          # nx ny nz >= 2^31 (1291^3 = 2151685171), also where a 64-bit product wraps
        assert dims[0] * dims[1] * dims[2] >= 2 ** 31
        assert h.pn_ccl_label(d, *dims, 26, d, None) == PN_ERR_ARG, dims
        assert h.pn_ccl_label(d, *dims, 6, d, None) == PN_ERR_ARG, dims
    assert h.pn_ccl_label(d, 1, 1, 0x7fffffff, 26, None, None) == PN_ERR_ARG  # 2^31 - 1 voxels is inside the limit: only the null pointer is refused
    for conn in (0, 4, 8, 18, 27, -26, 7):
        assert h.pn_ccl_label(d, 4, 4, 4, conn, d, None) == PN_ERR_ARG, conn
    assert b"argument check failed" in h.pn_last_error()


def test_label_components_refuses_cpu_tensors_and_wrong_types():
    from pienerf_amd.components import label_components
    with pytest.raises(RuntimeError):
        label_components(torch.zeros(4, 4, 4, dtype=torch.bool))


# ------------------------------------------------------------------ select_components
def _restate(labels, keep):
    """numpy restatement: rank by size descending, ties to the smaller root."""
    lab = np.asarray(labels)
    roots, counts = np.unique(lab[lab >= 0], return_counts=True)
    ranked = sorted(zip(roots.tolist(), counts.tolist()), key=lambda rc: (-rc[1], rc[0]))[:keep]
    return np.isin(lab, [r for r, _ in ranked]), ranked


def _labels_of(blobs, shape):
    """A label lattice written by hand: each blob is a list of voxel coordinates, labelled with its smallest flat index."""
    lab = np.full(shape, -1, np.int32)
    for vox in blobs:
        flat = [np.ravel_multi_index(v, shape) for v in vox]
        for v in vox:
            lab[v] = min(flat)
    return lab


def _line(i, j, k0, n):
    return [(i, j, k0 + s) for s in range(n)]


SHAPE = (6, 7, 9)
BLOBS = [_line(0, 0, 0, 3), _line(1, 2, 1, 7), _line(2, 5, 0, 3), _line(3, 3, 2, 5), _line(5, 6, 8, 1), _line(4, 1, 3, 5)]   # sizes 3 7 3 5 1 5


@pytest.mark.parametrize("keep", [1, 2, 3, 4, 5, 6, 7, 100])
def test_select_components_ranks_by_size_then_root(keep):
    from pienerf_amd.components import select_components
    lab = _labels_of(BLOBS, SHAPE)
    mask, kept = select_components(torch.from_numpy(lab), keep)
    want_mask, want = _restate(lab, keep)
    assert mask.dtype == torch.bool and tuple(mask.shape) == SHAPE
    assert kept == want and np.array_equal(mask.numpy(), want_mask)
    assert all(isinstance(r, int) and isinstance(s, int) for r, s in kept)
    if keep >= len(BLOBS):
        assert np.array_equal(mask.numpy(), lab >= 0) and len(kept) == len(BLOBS)


def test_select_components_tie_goes_to_the_smaller_root():
    from pienerf_amd.components import select_components
    a, b = _line(1, 1, 1, 4), _line(4, 4, 2, 4)                     # two identical blobs
    for blobs in ([a, b], [b, a]):
        lab = _labels_of(blobs, SHAPE)
        mask, kept = select_components(torch.from_numpy(lab), 1)
        root = int(np.ravel_multi_index(a[0], SHAPE))
        assert kept == [(root, 4)]
        assert np.array_equal(mask.numpy(), lab == root) and int(mask.sum()) == 4
    lab = _labels_of([_line(5, 5, 0, 5), a, b], SHAPE)              # ranks 2 and 3 tie behind a larger blob with the largest root
    _, kept = select_components(torch.from_numpy(lab), 2)
    assert kept == [(int(np.ravel_multi_index((5, 5, 0), SHAPE)), 5), (int(np.ravel_multi_index(a[0], SHAPE)), 4)]


def test_select_components_refuses_keep_below_one():
    from pienerf_amd.components import select_components
    lab = torch.from_numpy(_labels_of(BLOBS, SHAPE))
    for keep in (0, -1):
        with pytest.raises(ValueError):
            select_components(lab, keep)


def test_select_components_on_an_empty_lattice_selects_nothing():
    from pienerf_amd.components import count_components, select_components
    lab = torch.full((3, 4, 5), -1, dtype=torch.int32)
    mask, kept = select_components(lab, 2)
    assert kept == [] and tuple(mask.shape) == (3, 4, 5) and not bool(mask.any())
    assert count_components(lab) == 0
    assert count_components(torch.from_numpy(_labels_of(BLOBS, SHAPE))) == len(BLOBS)


# ------------------------------------------------------------------ front ends
def test_front_ends_accept_con_and_default_to_off():
    from pienerf_amd import main_train, mesh, sampling
    # sampling stores it as `con` (the option key AdaptiveUniformSampling reads); mesh and main_train as `components` (extract_geometry's argument:
    # main_train's namespace is compared name by name with the reference's, whose unused `con` defaults to 1)
    for mod, name in ((sampling, "con"), (mesh, "components"), (main_train, "components")):
        p = mod.parser()
        assert getattr(p.parse_args([]), name) == 0, mod.__name__
        assert getattr(p.parse_args(["--con", "2"]), name) == 2, mod.__name__
    a = sampling.parser().parse_args([])
    assert a.vres == 96 and sampling.parser().parse_args(["--vres", "64"]).vres == 64


def test_sampler_reads_the_component_options():
    from pienerf_amd.sampling import AdaptiveUniformSampling
    base = dict(bound=1.0, hash_grid_size=0.12)
    s = AdaptiveUniformSampling(base, torch.nn.Identity(), device="cpu")
    assert (s.con, s.vres, s.con_connectivity) == (0, 96, 26)
    s = AdaptiveUniformSampling(dict(base, con=2, vres=40, con_connectivity=6), torch.nn.Identity(), device="cpu")
    assert (s.con, s.vres, s.con_connectivity) == (2, 40, 6)
