"""The order in which a workgroup of the fused launch draws the packets of its share (csrc/pn_fused_order.h), on the CPU: pn_fused_order_host runs the
header functions the kernel runs (pn_order_key, pn_order_rank).  For random and adversarial key sets the order is a permutation, descending in the
packet key and stable (ties keep list order); the first PN_ORDER_CAP = 512 packets are ordered among themselves, the packets behind them stay where
they are."""
import ctypes as C

import numpy as np
import pytest

CAP, PACKET = 512, 8


def _order(t, far):
    from pienerf_amd._lib import check, lib
    t, far = np.ascontiguousarray(t, np.float32), np.ascontiguousarray(far, np.float32)
    n = len(t)
    n_packets = (n + PACKET - 1) // PACKET
    perm = np.full(n_packets + 1, -7, np.int32)   # one guard entry behind the packets
    check(lib().pn_fused_order_host(t.ctypes.data_as(C.c_void_p), far.ctypes.data_as(C.c_void_p), n, perm.ctypes.data_as(C.c_void_p)), "fused_order_host")
    assert perm[n_packets] == -7
    return perm[:n_packets]


def _packet_keys(t, far):
    """The rule restated: far - t where t < far, else 0 (NaN compares false); a packet is as long as its longest ray, missing entries count 0."""
    t, far = np.asarray(t, np.float32), np.asarray(far, np.float32)
    with np.errstate(invalid="ignore"):
        k = np.where(t < far, far - t, np.float32(0)).astype(np.float32)
    k = np.concatenate([k, np.zeros((-len(k)) % PACKET, np.float32)])
    return k.reshape(-1, PACKET).max(axis=1) if len(k) else np.zeros(0, np.float32)


def _check(t, far):
    perm = _order(t, far)
    keys = _packet_keys(t, far)
    n = len(keys)
    m = min(n, CAP)
    assert sorted(perm.tolist()) == list(range(n))                       # a permutation of the share's packets
    assert sorted(perm[:m].tolist()) == list(range(m))                   # ... of the ordered prefix within itself
    assert perm[m:].tolist() == list(range(m, n))                        # behind it: list order
    ko = keys[perm[:m]]
    assert np.all(ko[:-1] >= ko[1:])                                     # descending
    same = ko[:-1] == ko[1:]
    assert np.all(perm[:m][:-1][same] < perm[:m][1:][same])              # stable
    assert perm[:m].tolist() == np.argsort(-keys[:m], kind="stable").tolist()
    return perm


def _rays_of_packet_keys(keys, rng=None):
    """Per-ray (t, far) whose packet keys are `keys` exactly: one ray of the packet carries the key (t = 0, far = key), the others are shorter."""
    keys = np.asarray(keys, np.float32)
    t = np.zeros(len(keys) * PACKET, np.float32)
    far = np.zeros(len(keys) * PACKET, np.float32)
    for p, k in enumerate(keys):
        slot = int(rng.integers(PACKET)) if rng is not None else 0
        far[p * PACKET + slot] = k
    return t, far


LENGTHS = [0, 1, 63, 64, 65, 200, 511, 512, 513, 1000]


@pytest.mark.parametrize("n", LENGTHS)
def test_order_of_random_keys(n):
    rng = np.random.default_rng(100 + n)
    keys = rng.integers(0, 12, n).astype(np.float32) * np.float32(0.25)   # few distinct values: many ties
    _check(*_rays_of_packet_keys(keys, rng))
    t = rng.random(n * PACKET, dtype=np.float32) * 4
    far = t + rng.standard_normal(n * PACKET).astype(np.float32)          # about half the rays with far <= t
    _check(t, far)


@pytest.mark.parametrize("n", LENGTHS)
def test_order_of_adversarial_keys(n):
    perm = _check(*_rays_of_packet_keys(np.full(n, 1.5, np.float32)))     # all equal: list order
    assert perm.tolist() == list(range(n))
    perm = _check(*_rays_of_packet_keys(np.arange(1, n + 1, dtype=np.float32)))   # strictly ascending: the ordered prefix reversed
    m = min(n, CAP)
    assert perm[:m].tolist() == list(range(m))[::-1]
    if n:
        for bad_t, bad_far in ((0.0, np.nan), (np.nan, 1.0), (2.0, 1.0), (0.0, -3.0)):   # a NaN end, a NaN start, a negative span, a negative end
            t, far = _rays_of_packet_keys(np.arange(1, n + 1, dtype=np.float32))
            q = (n // 2) * PACKET
            t[q], far[q] = bad_t, bad_far          # the packet's key ray: the packet counts 0 and goes last in the ordered prefix
            perm = _check(t, far)
            if n // 2 < CAP:
                assert perm[m - 1] == n // 2


@pytest.mark.parametrize("n_rays", [1, 5, 8, 9, 23])
def test_order_of_a_list_that_is_no_multiple_of_a_packet(n_rays):
    t = np.zeros(n_rays, np.float32)
    far = np.arange(1, n_rays + 1, dtype=np.float32)
    perm = _check(t, far)
    assert perm[0] == (n_rays - 1) // PACKET   # the last, partly filled packet holds the longest ray
