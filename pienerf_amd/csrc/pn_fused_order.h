// The order in which a workgroup of the fused launch (pn_trips_fused.h, plain form) draws the packets of its share: longest first.
//
// The launch is as long as its longest wave, and what decides a workgroup's end is the rounds its last rays still need one after the other (round 4's
// hand-back experiment).  With jobs of unequal length the list-scheduling answer is to hand the longest out first; a ray's length is known before it is
// drawn: the span far - t it still has to march (the prologue has shortened `fars` to where the ray's candidates end), with a fixed step an upper bound
// on the rounds it can take.  A packet (8 consecutive entries of the alive list: neighbouring pixels that share candidate lists, dealt together) is as long
// as its longest ray.
//
// The rule, shared by the kernel and the host entry point pn_fused_order_host (tests/test_fused_order.py checks it on the CPU):
//   key(ray)      = far - t if t < far, else 0 (a finished ray, a NaN on either side: the comparison is false) — never NaN, never negative
//   key(packet)   = the largest key of its rays; entries beyond the list count 0
//   packet a is drawn before packet b  iff  key(a) > key(b), or the keys are equal and a < b (ties keep list order: a pure function of the frame)
// The permutation is built by RANK (the number of packets drawn before this one), every packet on a thread of its own: no exchange network, no chunk
// merge, and a permutation by construction because `before` is a strict total order on (key, position).
//
// A share is not bounded (a small fused_grid, a large image), the LDS beside the weight image is: the first PN_ORDER_CAP packets of a share are ordered
// among themselves, the packets behind them follow in list order.  A share holds at most N / (64 fused_grid) packets (the launch applies from n_alive <=
// N / 8 on), so 512 covers every image up to 2048 x 2048 on half the chip's CUs, the chair's 800 x 800 (78 packets) six times over; beyond that the tail
// of a very long share is as it was.  1 KB of LDS (16-bit positions); the keys are staged in the waves' march staging area, which is free until the first round.
#pragma once

#define PN_ORDER_CAP 512     // packets of a share that are ordered (16-bit positions in LDS)
#define PN_ORDER_PACKET 8    // alive-list entries per packet

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PN_ORDER_HD __host__ __device__ __forceinline__
#else
#define PN_ORDER_HD inline
#endif

PN_ORDER_HD float pn_order_key(float t, float far) { return t < far ? far - t : 0.0f; }

PN_ORDER_HD bool pn_order_before(float ka, int a, float kb, int b) { return ka > kb || (ka == kb && a < b); }

// position of packet i in the drawing order of packets 0 .. n-1
PN_ORDER_HD int pn_order_rank(const float* keys, int n, int i) {
    const float ki = keys[i];
    int r = 0;
    for (int j = 0; j < n; j++) r += pn_order_before(keys[j], j, ki, i) ? 1 : 0;
    return r;
}
