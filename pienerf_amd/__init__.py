"""MI355X-native simulate-and-render path of PIE-NeRF."""
# The pipelined harness keeps 3 render streams + 1 simulator stream busy at once.  ROCm maps streams onto GPU_MAX_HW_QUEUES
# hardware queues, shared with the null stream and torch's side streams; streams that land on one queue serialise (a ~30-launch
# substep behind a whole render).  The package leaves that setting to the environment it runs in: it changes how much the
# streams overlap, never what a frame computes.
