"""pn_render_opts.fused_order (csrc/pn_fused_order.h): a workgroup of the fused launch draws the packets of its share longest first.  Every ray's march,
network tiles and composite are a function of the ray alone, so the order a workgroup draws its rays in cannot show in a frame: order on against order
off (list order), in the same process, bit for bit — pixels, trip records, statistics, the trip the launch took over at, no error flag — in the plain
form (rays from the alive list: the form the order acts on), and in the FOLD and WHOLE forms (rays from lists that fill while the launch runs), for the
alive lists and shares at which the hand-out takes another path.  The trip record of the first fused trip is the sum of the workgroups' counts of rays
drawn: it equals the trip-by-trip frame's alive count iff every ray was handed out exactly once.  The order itself (a permutation, descending, stable,
the cap) is checked on the CPU in test_fused_order.py."""
import numpy as np
import pytest
import torch

import oracle
from pienerf_amd import scene
from test_gpu_edges import _net
from test_gpu_parity import DEV, T

pytestmark = pytest.mark.gpu

FORMS = {"plain": dict(fused_from=0), "fold": dict(fused_from=0, fused_fold=True), "whole": dict(fused_from=0, fused_whole=True)}
KEYS = ("image", "depth", "depth_0", "weights_sum")


def _frame(net, o, d, opt, amp=False, **kw):
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=amp):
        out = net.render_deformed(T(o)[None], T(d)[None], collect_stats=True, **dict(opt, **kw))
    fc = net.fused_clocks()
    return dict(stats=dict(net.last_stats), recs=net.trip_records(max_trips=140), out={k: out[k].clone() for k in KEYS}, first=fc["first_trip"], mode=fc.get("mode"))


def _same_frame(a, b, first_rec_tail=True):
    assert a["stats"] == b["stats"] and a["stats"]["err"] == 0 and a["stats"]["alive_at_exit"] == 0, (a["stats"], b["stats"])
    if first_rec_tail:
        assert a["recs"] == b["recs"], (a["recs"], b["recs"])
    else:   # (the sixth entry of the FIRST trip's record is a diagnostic of the form that trip ran in: test_gpu_fused.py)
        assert a["recs"][0][:5] == b["recs"][0][:5] and a["recs"][1:] == b["recs"][1:], (a["recs"], b["recs"])
    for k in KEYS:
        assert torch.equal(torch.nan_to_num(a["out"][k], nan=-1.0), torch.nan_to_num(b["out"][k], nan=-1.0)), k


def _on_off_in_every_form(net, o, d, opt, forms=("plain", "fold", "whole"), amp=False, **kw):
    """Order on == order off in each form, and each == the trip-by-trip frame.  Returns the trip-by-trip frame."""
    ref = _frame(net, o, d, opt, amp=amp, fused_from=-1, **kw)
    assert ref["first"] == -1
    for form in forms:
        on = _frame(net, o, d, opt, amp=amp, fused_order=True, **dict(FORMS[form], **kw))
        off = _frame(net, o, d, opt, amp=amp, fused_order=False, **dict(FORMS[form], **kw))
        assert on["first"] == off["first"] and on["mode"] == off["mode"], (form, on["first"], off["first"])
        assert on["first"] >= 0, form                  # the fused launch did run
        if form == "plain":
            assert on["first"] == 1 and on["mode"] == 0, (on["first"], on["mode"])
        _same_frame(on, off)
        _same_frame(ref, on, first_rec_tail=False)     # ... trip 1's n_alive included: every ray of the alive list drawn exactly once
    return ref


def _rays(W, pose, H=None):
    H = H or W
    return oracle.get_rays(scene.orbit_pose(*pose), scene.orbit_intrinsics(W, H, 50.0), W, H)


def _cus():
    from pienerf_amd._lib import lib
    return int(lib().pn_device_cu_count())


def test_alive_list_shorter_than_one_packet(deformed_ip_state, small_opt, ckpt):
    """Seen from far away the object covers a handful of pixels: fewer than 8 rays go on behind the first trip."""
    W = 48
    o, d = _rays(W, (30.0, 35.0, -25.0))
    ref = _on_off_in_every_form(_net(ckpt, deformed_ip_state), o, d, dict(small_opt, W=W, H=W))
    assert ref["recs"][1][1] == 8 and 0 < ref["recs"][1][0] < 8, ref["recs"]


def test_alive_list_is_no_multiple_of_a_packet_and_most_shares_are_empty(deformed_ip_state, small_opt, ckpt):
    """fused_grid = 0: a workgroup per CU, more of them than the list has packets — the shares behind the last packet are empty."""
    W = 96
    o, d = _rays(W, (5.0, 35.0, -25.0))
    ref = _on_off_in_every_form(_net(ckpt, deformed_ip_state), o, d, dict(small_opt, W=W, H=W), fused_grid=0)
    A = ref["recs"][1][0]
    assert ref["recs"][1][1] == 8 and A % 8 != 0 and (A + 7) // 8 < _cus(), (A, _cus())


@pytest.mark.parametrize("grid", [1, 2])
def test_share_of_more_than_64_packets(deformed_ip_state, small_opt, ckpt, grid):
    """Two workgroups (one) for the whole list: a share is longer than a wave has lanes, with one workgroup longer than the 512 packets that are ordered."""
    W = 192
    o, d = _rays(W, (4.0, 35.0, -25.0))
    ref = _on_off_in_every_form(_net(ckpt, deformed_ip_state), o, d, dict(small_opt, W=W, H=W), fused_grid=grid)
    packets = (ref["recs"][1][0] + 7) // 8
    assert ref["recs"][1][1] == 8 and packets > (128 if grid == 2 else 512), ref["recs"]


def test_thin_slab_seen_face_on(deformed_ip_state, small_opt, ckpt):
    """A one-layer cut of the object seen along its normal: the rays cross it in about a step, so behind the first trip most of them have nothing left to march
    (far <= t: key 0) — packets of equal keys, which keep list order, and rays in the list that end without a sample."""
    ip = deformed_ip_state
    z = np.asarray(ip["p_ori"])[:, 2]
    sel = np.abs(z - np.median(z)) < ip["IP_dx"]
    assert 50 < sel.sum() < len(z)
    F = np.zeros_like(np.asarray(ip["F"])[sel])
    F.reshape(int(sel.sum()), 9)[:, [0, 4, 8]] = 1.0
    slab = dict(p_def=np.asarray(ip["p_ori"])[sel], p_ori=np.asarray(ip["p_ori"])[sel], F=F, dF=np.zeros_like(np.asarray(ip["dF"])[sel]), IP_dx=ip["IP_dx"])
    W = 96
    o, d = _rays(W, (5.0, 0.0, 0.0))
    ref = _on_off_in_every_form(_net(ckpt, slab), o, d, dict(small_opt, W=W, H=W), fused_grid=3)
    assert ref["stats"]["samples"] > 0 and len(ref["recs"]) >= 2, ref["recs"]


@pytest.mark.parametrize("num_seek_IP,max_iter_num,fp16", [(1, 1, False), (3, 3, False), (2, 1, True)])
def test_other_builds_of_the_launch(deformed_ip_state, small_opt, ckpt, num_seek_IP, max_iter_num, fp16):
    """num_seek_IP = 1, several Newton iterations, the fp16 network: other template instances of the kernel."""
    W = 96
    o, d = _rays(W, (5.0, 35.0, -25.0))
    opt = dict(small_opt, W=W, H=W, num_seek_IP=num_seek_IP, max_iter_num=max_iter_num)
    ref = _on_off_in_every_form(_net(ckpt, deformed_ip_state), o, d, opt, amp=fp16, fused_grid=5)
    assert ref["recs"][1][1] == 8 and ref["stats"]["trips"] >= 3, ref["recs"]


def test_captured_frame_replays_the_eager_frame(deformed_ip_state, small_opt, ckpt):
    """The order is built inside the launch from the frame's own rays: a captured frame, replayed, is the eager frame."""
    W = 96
    o, d = _rays(W, (5.0, 35.0, -25.0))
    opt = dict(small_opt, W=W, H=W, fused_from=0, fused_order=True, fused_grid=4)
    net = _net(ckpt, deformed_ip_state)
    eager = _frame(net, o, d, opt)
    assert eager["first"] == 1 and eager["stats"]["alive_at_exit"] == 0
    ro, rd = T(o)[None], T(d)[None]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.no_grad(), torch.cuda.stream(s):
        net.render_deformed(ro, rd, async_trips=1, **opt)   # warm-up of the non-blocking form outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
        out = net.render_deformed(ro, rd, async_trips=1, **opt)
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    st = net.render_status()
    assert st["alive_at_exit"] == 0 and st["err"] == 0 and st["samples"] == eager["stats"]["samples"], st
    for k in KEYS:
        assert torch.equal(torch.nan_to_num(out[k], nan=-1.0), torch.nan_to_num(eager["out"][k], nan=-1.0)), k
