"""Measurement hooks on a frame workspace of NeRFRenderer (pn_frame_*): work counters, the fused launch's phase clocks, trip records and trip times."""
import ctypes as C

from .._lib import check, lib, stream_ptr


class FrameHooksMixin:
    def march_counters(self, enable, read=False, slot=0):
        """Measurement hook on workspace `slot`: 1 = device-side work counters of the march kernel (iterations, candidates, warps, samples);
        2 = HIP events around each trip's march and network launches (see trip_times)."""
        out = (C.c_uint64 * 4)() if read else None
        check(lib().pn_frame_march_counters(self._frames[slot][0], int(enable), out, stream_ptr()), "march_counters")
        return None if out is None else dict(iterations=int(out[0]), candidates=int(out[1]), warps=int(out[2]), samples=int(out[3]))

    def fused_clocks(self, slot=0, reset=False):
        """Phase clocks of the fused later-trips launches on `slot` (march_counters(4)): dict of cycles summed over waves + the trip the last render
        switched to the fused launch at (-1: it did not)."""
        out, first = (C.c_uint64 * 16)(), C.c_int(-1)
        check(lib().pn_frame_fused_clocks(self._frames[slot][0], out, C.byref(first), int(bool(reset)), stream_ptr()), "fused_clocks")
        return dict(refill=int(out[0]), march=int(out[1]), windows=int(out[2]), network=int(out[3]), composite=int(out[4]), wave_rounds=int(out[5]),
                    waves=int(out[6]), lifetime_ticks=int(out[7]), max_rounds=int(out[8]), max_lifetime_ticks=int(out[9]), first_trip=int(first.value),
                    # whole-frame form (fused_from = 0): the first trip's one-lane march, its 64-lane windows, its network, its composite + hand-over,
                    # the wait at the workgroup barrier behind it
                    a_march=int(out[10]), a_windows=int(out[11]), a_network=int(out[12]), a_composite=int(out[13]), a_barrier=int(out[14]),
                    mode=int(out[15]))   # 0: later trips only, 1: whole frame, 2: first trip's network / composite / compaction folded in

    def trip_records(self, slot=0, max_trips=16):
        """Diagnostics: [(n_alive, n_step, step_base, n_samples, n_emitted, n_tail)] per trip of the last render on `slot`."""
        rec, tail = (C.c_int * (5 * max_trips))(), (C.c_int * max_trips)()
        check(lib().pn_frame_trip_records(self._frames[slot][0], rec, tail, max_trips, stream_ptr()), "trip_records")
        return [tuple(rec[5 * i:5 * i + 5]) + (tail[i],) for i in range(max_trips) if rec[5 * i] > 0]

    def trip_times(self, slot=0):
        """Per-trip (march_ms, network_ms) of the last render on `slot` made while event timing was enabled (HIP events on the launch stream;
        for a captured render: the records of the last replay)."""
        a, b, n = (C.c_float * 64)(), (C.c_float * 64)(), C.c_int(0)
        check(lib().pn_frame_trip_times(self._frames[slot][0], a, b, 64, C.byref(n), stream_ptr()), "trip_times")
        return [float(a[i]) for i in range(n.value)], [float(b[i]) for i in range(n.value)]
