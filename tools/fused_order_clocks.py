#!/usr/bin/env python
"""Phase clocks and launch durations of the fused launch on the 800 x 800 chair, one frame at a time on half the CUs, in the plain and the folded form with
pn_render_opts.fused_order on and off in ONE process: the launch alone (events around it, median and minimum of 9 frames), wave-rounds, the mean and the
longest wave lifetime (march_counters(4), 5 frames).  One JSON line per (form, order), the set twice.

    python tools/fused_order_clocks.py [label]
"""
import json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pienerf_amd import scene
from pienerf_amd.harness import SimRenderHarness
tag = sys.argv[1] if len(sys.argv) > 1 else "tree"   # a label for the output lines
opt = scene.default_opt(W=800, H=800)
h = SimRenderHarness(opt, device="cuda:0")
h.opt.update(march_throughput=64, fused_grid=max(torch.cuda.get_device_properties(0).multi_processor_count // 2, 1))
for _ in range(20):
    h.step()
h.synchronize()
m = h.model
FORMS = {"plain": dict(fused_from=0, fused_fold=False), "fold": dict(fused_from=0, fused_fold=True)}
res = []
for rep in range(2):
  for form, fkw in FORMS.items():
    for order in (True, False):
        kw = dict(fkw, fused_order=order)
        for _ in range(3):
            h.step(simulate=False, render_kw=kw)
        m.march_counters(2)
        reps = []
        for _ in range(9):
            h.step(simulate=False, render_kw=kw)
            reps.append(m.trip_times())
        m.march_counters(0)
        ff = m.fused_clocks()["first_trip"]
        mm = np.array([r[0][:ff + 1] for r in reps])
        launch_ms = float(np.median(mm[:, ff])); launch_min = float(mm[:, ff].min())
        m.march_counters(4); m.fused_clocks(reset=True)
        for _ in range(5):
            h.step(simulate=False, render_kw=kw)
        c = m.fused_clocks(); m.march_counters(0)
        h.step(simulate=False, collect_stats=True, render_kw=kw)
        r = dict(tag=tag, rep=rep, form=form, order=order, first_trip=ff, mode=c.get("mode"), fused_launch_ms_median=round(launch_ms, 4), fused_launch_ms_min=round(launch_min, 4),
                 waves=c["waves"] // 5, wave_rounds=c["wave_rounds"] // 5, max_rounds=c["max_rounds"], mean_life_us=round(c["lifetime_ticks"] / max(c["waves"], 1) / 100.0, 1),
                 longest_life_us=round(c["max_lifetime_ticks"] / 100.0, 1), samples=m.last_stats["samples"], trips=m.last_stats["trips"], n_alive_trip1=m.trip_records(max_trips=140)[1][0])
        print(json.dumps(r), flush=True)
