// The substep in its CSR launch form, with the op-level calc_elastic / collect_rhs entries that share its kernels (included by pn_sim.hip only,
// behind k_matvec3).
#pragma once
#include "pn_sim_svd.h"
#include "pn_sim_stamps.h"

// ------------------------------------------------------------------------------------------------ calc_elastic
// 8 lanes per IP.  Writes RF/VF/FF (op-level, any may be NULL) and/or P = dx^3 (mu R + lam V) (step driver).
template <bool MC = false>
__global__ void __launch_bounds__(256) k_elastic(int n_IP, const int* __restrict__ topo, const double* __restrict__ dNx, const double* __restrict__ dof,
                                                 double* __restrict__ RF, double* __restrict__ VF, double* __restrict__ FF, double* __restrict__ P,
                                                 const double* __restrict__ mu, const double* __restrict__ lam, double dx3,
                                                 const int* __restrict__ csr_pos = nullptr, double* __restrict__ P_csr = nullptr,
                                                 double* __restrict__ Vstore = nullptr, int mc_sweeps = 0) {
    PN_SIM_STAMP(1);
    PN_SIM_PRIO();
    const int tid = threadIdx.x + blockIdx.x * blockDim.x;
    const int v = tid >> 3, i = tid & 7;
    const bool live = v < n_IP;
    M3 Fm = {};
    if (live) ip_F_partial(dof + (size_t)topo[v * 8 + i] * 30, dNx + ((size_t)v * 8 + i) * 30, Fm);
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            double s = Fm.m[r][c];
            s += shfl_xor_d(s, 1);
            s += shfl_xor_d(s, 2);
            s += shfl_xor_d(s, 4);
            Fm.m[r][c] = s;
        }
    if (!live) return;  // the 8 lanes of an IP share v: whole groups leave together
    double Pm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (i == 0) {
        M3 U, V;
        double sig[3], sp[3];
        if (MC) {
            svd3_mcadams(Fm, U, sig, V, mc_sweeps);   // the published algorithm: fixed sweeps, no warm start
        } else if (Vstore) {
            // step driver: start from this IP's V of the previous local/global iteration (identity before the first substep), leave the new one.
            // 1e-24: off-diagonals below 1e-12 of the diagonal, ten digits beyond the 1e-4 relative bar of the DOF displacements
            M3 Q0;
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int c = 0; c < 3; c++) Q0.m[r][c] = Vstore[(size_t)v * 9 + r * 3 + c];
            svd3(Fm, U, sig, V, &Q0, 1e-24);
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int c = 0; c < 3; c++) Vstore[(size_t)v * 9 + r * 3 + c] = V.m[r][c];
        } else
        svd3(Fm, U, sig, V);
        volume_invariant_project(sig, sp);
        const double m_ = mu ? mu[v] : 0.0, l_ = lam ? lam[v] : 0.0;
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const double R = U.m[r][0] * V.m[c][0] + U.m[r][1] * V.m[c][1] + U.m[r][2] * V.m[c][2];
                const double Vv = U.m[r][0] * sp[0] * V.m[c][0] + U.m[r][1] * sp[1] * V.m[c][1] + U.m[r][2] * sp[2] * V.m[c][2];
                if (RF) RF[(size_t)v * 9 + r * 3 + c] = R;
                if (VF) VF[(size_t)v * 9 + r * 3 + c] = Vv;
                if (FF) FF[(size_t)v * 9 + r * 3 + c] = U.m[r][0] * sig[0] * V.m[c][0] + U.m[r][1] * sig[1] * V.m[c][1] + U.m[r][2] * sig[2] * V.m[c][2];
                Pm[r * 3 + c] = dx3 * (m_ * R + l_ * Vv);
                if (P) P[(size_t)v * 9 + r * 3 + c] = Pm[r * 3 + c];
            }
    }
    if (P_csr) {
        // step driver: P also goes, once per neighbour slot, to that slot's position in its kernel's CSR list, so that the
        // gather (k_rhs_gather_csr) reads P and dNx as two contiguous streams with no index to chase
        const int src = (threadIdx.x & 63) & ~7;
        double* __restrict__ dst = P_csr + (size_t)csr_pos[v * 8 + i] * 9;
#pragma unroll
        for (int q = 0; q < 9; q++) {
            int2 t = *reinterpret_cast<int2*>(&Pm[q]);
            t.x = __shfl(t.x, src);
            t.y = __shfl(t.y, src);
            dst[q] = *reinterpret_cast<double*>(&t);
        }
    }
}

extern "C" int pn_sim_calc_elastic(int n_IP, const int* topo, const double* dNx, const double* dof, double* RF, double* VF, double* FF,
                                   int mcadams_sweeps, void* stream) {
    PN_REQUIRE(n_IP > 0 && topo && dNx && dof && RF && VF && pn_svd_sweeps_ok(mcadams_sweeps));
    if (mcadams_sweeps)
        k_elastic<true><<<pn_div_up((uint64_t)n_IP * 8, 256), 256, 0, (hipStream_t)stream>>>(n_IP, topo, dNx, dof, RF, VF, FF, nullptr, nullptr, nullptr, 0.0,
                                                                                             nullptr, nullptr, nullptr, mcadams_sweeps);
    else
        k_elastic<false><<<pn_div_up((uint64_t)n_IP * 8, 256), 256, 0, (hipStream_t)stream>>>(n_IP, topo, dNx, dof, RF, VF, FF, nullptr, nullptr, nullptr, 0.0);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

// ------------------------------------------------------------------------------------------------ collect_rhs (gather form)
// One wave per kernel k.  Entry e of the CSR list = vid*8 + dir.  Lane-strided accumulation of the 10x3 block, fixed
// xor-tree reduction.  mode 0: rhs = sum (P from mu/lam/RF/VF); mode 1 (step driver): out = momentum + sum - rhs_rest.
__global__ void __launch_bounds__(256) k_rhs_gather(int n_k, double dx3, const int* __restrict__ csr_bg, const int* __restrict__ csr_cnt,
                                                    const int* __restrict__ csr_buf, const double* __restrict__ mu, const double* __restrict__ lam,
                                                    const double* __restrict__ dNx, const double* __restrict__ RF, const double* __restrict__ VF,
                                                    const double* __restrict__ P, const double* __restrict__ momentum,
                                                    const double* __restrict__ rhs_rest, double* __restrict__ out) {
    PN_SIM_PRIO();
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= n_k) return;
    const int lane = threadIdx.x & 63;
    double acc[30];
#pragma unroll
    for (int q = 0; q < 30; q++) acc[q] = 0.0;
    const int bg = csr_bg[k], cnt = csr_cnt[k];
    for (int e = lane; e < cnt; e += 64) {
        const int code = csr_buf[bg + e];
        const int v = code >> 3;
        double Pm[9];
        if (P) {
#pragma unroll
            for (int q = 0; q < 9; q++) Pm[q] = P[(size_t)v * 9 + q];
        } else {
            const double m_ = mu[v], l_ = lam[v];
#pragma unroll
            for (int q = 0; q < 9; q++) Pm[q] = dx3 * (m_ * RF[(size_t)v * 9 + q] + l_ * VF[(size_t)v * 9 + q]);
        }
        const double* __restrict__ dn = dNx + (size_t)code * 30;  // [c][x]
#pragma unroll
        for (int x = 0; x < 10; x++) {
            const double g0 = dn[x], g1 = dn[10 + x], g2 = dn[20 + x];
#pragma unroll
            for (int r = 0; r < 3; r++) acc[x * 3 + r] += Pm[r * 3] * g0 + Pm[r * 3 + 1] * g1 + Pm[r * 3 + 2] * g2;
        }
    }
#pragma unroll
    for (int q = 0; q < 30; q++) {
        double s = acc[q];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += shfl_xor_d(s, o);
        acc[q] = s;
    }
    if (lane < 30) {
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < 30; q++) if (q == lane) s = acc[q];
        const size_t o = (size_t)k * 30 + lane;
        out[o] = momentum ? (momentum[o] + s - rhs_rest[o]) : s;
    }
}

// Step-driver form of the gather: one 1024-thread workgroup per kernel over CSR-ORDERED copies of dNx (dNx_csr[entry][c][x],
// built once at initialisation) and, when calc_elastic wrote it, of P (P_csr[entry][r][c]): the 240 B + 72 B of every entry are
// read as contiguous streams with no index to follow.  Thread (slot, q = c*10 + x) walks entries slot, slot+32, ... and
// accumulates the three rows r of P[r][c] * dNx[c][x]; the 32 slots x 3 columns c are then reduced through LDS in a fixed
// order (bit-reproducible run to run).  out = momentum + sum - rhs_rest.
#define PN_GATHER_SLOTS 32
__global__ void __launch_bounds__(1024) k_rhs_gather_csr(int n_k, const int* __restrict__ csr_bg, const int* __restrict__ csr_cnt,
                                                         const int* __restrict__ csr_buf, const double* __restrict__ dNx_csr,
                                                         const double* __restrict__ P, const double* __restrict__ P_csr,
                                                         const double* __restrict__ momentum,
                                                         const double* __restrict__ rhs_rest, double* __restrict__ out) {
    PN_SIM_PRIO();
    constexpr int NS = PN_GATHER_SLOTS;
    __shared__ double red[NS][30][3];
    const int k = blockIdx.x;
    const int t = threadIdx.x;
    const int slot = t / 30, q = t - slot * 30, c = q / 10;
    const int bg = csr_bg[k], cnt = csr_cnt[k];
    if (t < NS * 30) {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        const double* __restrict__ g = dNx_csr + (size_t)bg * 30 + q;
        int e = slot;
        if (P_csr) {  // every load is independent of every other
            const double* __restrict__ pc = P_csr + (size_t)bg * 9 + c;
            for (; e + 3 * NS < cnt; e += 4 * NS) {  // four entries in flight
                double gv[4], p0[4], p1[4], p2[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const size_t ee = (size_t)(e + NS * u);
                    gv[u] = g[ee * 30];
                    p0[u] = pc[ee * 9]; p1[u] = pc[ee * 9 + 3]; p2[u] = pc[ee * 9 + 6];
                }
#pragma unroll
                for (int u = 0; u < 4; u++) { a0 += p0[u] * gv[u]; a1 += p1[u] * gv[u]; a2 += p2[u] * gv[u]; }
            }
            for (; e < cnt; e += NS) {
                const double gv = g[(size_t)e * 30];
                a0 += pc[(size_t)e * 9] * gv;
                a1 += pc[(size_t)e * 9 + 3] * gv;
                a2 += pc[(size_t)e * 9 + 6] * gv;
            }
        } else {
            for (; e < cnt; e += NS) {
                const int v = csr_buf[bg + e] >> 3;
                const double gv = g[(size_t)e * 30];
                const double* __restrict__ Pv = P + (size_t)v * 9 + c;
                a0 += Pv[0] * gv;
                a1 += Pv[3] * gv;
                a2 += Pv[6] * gv;
            }
        }
        red[slot][q][0] = a0; red[slot][q][1] = a1; red[slot][q][2] = a2;
    }
    __syncthreads();
    if (t < 30) {
        const int x = t / 3, r = t - x * 3;  // output row x*3 + r of kernel k
        double s = 0.0;
        for (int sl = 0; sl < NS; sl++)
#pragma unroll
            for (int cc = 0; cc < 3; cc++) s += red[sl][cc * 10 + x][r];
        const size_t o = (size_t)k * 30 + t;
        out[o] = momentum[o] + s - rhs_rest[o];
    }
}

// Balanced form of the gather used by the step driver.  One workgroup per kernel leaves the launch as long as its longest list (chair:
// 770 entries against a mean of 206, and only 139 of 256 CUs busy), so the lists are cut into chunks of PN_GCH entries, one
// workgroup per chunk, each writing its 30 partial sums; the chunk sums of a kernel are added in ascending chunk order by the
// workgroup that completes its kernel's set (k_rhs_gather_chunk), so the result is still reproducible bit for bit.
// k_gather_plan (once per simulator, one workgroup) lays the chunks out: kc_bg[k] = first chunk of kernel k, chunk[b] = (first entry, count, kernel,
// chunks of that kernel); every kernel gets at least one chunk (an empty one if it has no entries), unused grid slots have kernel -1.
#ifndef PN_GCH
#define PN_GCH 64   // entries per chunk; the chunk kernel runs PN_GCH / 4 slots x 30 threads.  64 (512-thread workgroups) since round 4: 6.9 instead of 7.7 us alone, and beside the render
                    // lanes a launch of smaller workgroups finds room sooner (start-to-next-start 10.8 instead of 14.4 us; 32: 11.6; profiles/r04_sim_stamps.txt)
#endif
__global__ void __launch_bounds__(512) k_gather_plan(int n_k, int chunks_max, const int* __restrict__ csr_bg, const int* __restrict__ csr_cnt,
                                                     int* __restrict__ kc_bg, int4* __restrict__ chunk, int* __restrict__ kcount) {
    // exclusive scan of the kernels' chunk counts by the whole workgroup (one lane walking the n_k kernels took 40 us of every substep)
    __shared__ int wsum[8];
    __shared__ int carry_s;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (int base = 0; base < n_k; base += 512) {
        const int k = base + (int)threadIdx.x;
        const int cnt = k < n_k ? csr_cnt[k] : 0;
        const int nc = k < n_k ? max((cnt + PN_GCH - 1) / PN_GCH, 1) : 0;
        int inc = nc;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(inc, o);
            if (lane >= o) inc += u;
        }
        if (lane == 63) wsum[wid] = inc;
        __syncthreads();
        int woff = 0, total = 0;
        for (int w = 0; w < 8; w++) { woff += (w < wid) ? wsum[w] : 0; total += wsum[w]; }
        const int first_chunk = carry_s + woff + inc - nc;
        if (k < n_k) {
            kc_bg[k] = first_chunk;
            const int bg = csr_bg[k];
            for (int j = 0; j < nc; j++)  // one load tells a workgroup its work
                chunk[first_chunk + j] = make_int4(bg + j * PN_GCH, max(min(PN_GCH, cnt - j * PN_GCH), 0), k, nc);
            kcount[k] = 0;
        }
        __syncthreads();
        if (threadIdx.x == 0) carry_s += total;
        __syncthreads();
    }
    const int n_chunks = carry_s;
    if (threadIdx.x == 0) kc_bg[n_k] = n_chunks;
    for (int b = n_chunks + threadIdx.x; b < chunks_max; b += blockDim.x) chunk[b] = make_int4(0, 0, -1, 0);  // unused tail of the grid
}

// The workgroup that completes its kernel's set of chunks ("last arriver") also adds them up, in ascending chunk order, and writes
// momentum + sum - rhs_rest: the sums need no launch of their own.  The XCDs' L2s are not coherent with each
// other, so the chunk sums go out as agent-scope stores (written through to the memory side), a workgroup waits for their acknowledgement before it bumps
// its kernel's arrival counter (agent-scope atomic at the memory side), and the last arriver — the one that counts `chunks` arrivals — reads all sums
// with agent-scope loads and stores 0 back into the counter: nobody else arrives at it before the next launch, so the counter is cyclic and a simulator
// that runs for days never wraps it (rounds 1-3 let it grow and tested (n % chunks) == 0, which loses its phase at 2^31 for chunk counts that do not divide 2^32).
__global__ void __launch_bounds__(PN_GCH * 8) k_rhs_gather_chunk(const int4* __restrict__ chunk, const double* __restrict__ dNx_csr,
                                                                  const double* __restrict__ P_csr, double* part, int* kcount,
                                                                  const int* __restrict__ kc_bg, const double* __restrict__ momentum,
                                                                  const double* __restrict__ rhs_rest, double* __restrict__ tot) {
    PN_SIM_STAMP(2);
    PN_SIM_PRIO();
    constexpr int NS = PN_GCH / 4;
    __shared__ double red[NS][30][3];
    __shared__ int last_s;
    const int b = blockIdx.x;
    const int4 ch = chunk[b];
    const int bg = ch.x, cnt = ch.y, kern = ch.z, nck = ch.w;
    if (kern < 0) return;  // the grid is the host-side upper bound 8 n_IP / PN_GCH + n_k
    const int t = threadIdx.x;
    const int slot = t / 30, q = t - slot * 30, c = q / 10;
    if (t < NS * 30) {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        const double* __restrict__ g = dNx_csr + (size_t)bg * 30 + q;
        const double* __restrict__ pc = P_csr + (size_t)bg * 9 + c;
        double gv[4], p0[4], p1[4], p2[4];  // PN_GCH / NS = 4 entries per slot, all loads independent
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int e = slot + NS * u;
            const bool on = e < cnt;
            const size_t ee = on ? (size_t)e : 0;
            gv[u] = on ? g[ee * 30] : 0.0;
            p0[u] = on ? pc[ee * 9] : 0.0; p1[u] = on ? pc[ee * 9 + 3] : 0.0; p2[u] = on ? pc[ee * 9 + 6] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) { a0 += p0[u] * gv[u]; a1 += p1[u] * gv[u]; a2 += p2[u] * gv[u]; }
        red[slot][q][0] = a0; red[slot][q][1] = a1; red[slot][q][2] = a2;
    }
    __syncthreads();
    // 30 outputs x NS slots: NS consecutive lanes add slot sl of output o (its three columns), then a fixed xor tree over those lanes
    // (30 threads adding 96 values each one after the other were 2.5 us of this kernel's 6.3)
    static_assert(NS == 32 || NS == 16 || NS == 8, "a power-of-two group of lanes per output");
    if (t < 30 * NS) {
        const int o = t / NS, sl = t % NS;
        const int x = o / 3, r = o - x * 3;
        double s = (red[sl][x][r] + red[sl][10 + x][r]) + red[sl][20 + x][r];
#pragma unroll
        for (int m = NS / 2; m > 0; m >>= 1) s += shfl_xor_d(s, m);
        if (sl == 0) __hip_atomic_store(part + (size_t)b * 30 + o, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __builtin_amdgcn_s_waitcnt(0);  // the sums are at the memory side
    __syncthreads();
    if (t == 0) {
        const int old = __hip_atomic_fetch_add(kcount + kern, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last_s = (old + 1) == nck;
        if (last_s) __hip_atomic_store(kcount + kern, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-armed for the next launch
    }
    __syncthreads();
    if (!last_s || t >= 30) return;
    const int b0 = kc_bg[kern];
    double sum = 0.0;
    for (int j0 = 0; j0 < nck; j0 += 8) {  // ascending chunk order, eight loads in flight (unconditional, clamped)
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = __hip_atomic_load(part + (size_t)(b0 + min(j0 + u, nck - 1)) * 30 + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int u = 0; u < 8; u++) if (j0 + u < nck) sum += v[u];
    }
    const size_t o = (size_t)kern * 30 + t;
    tot[o] = momentum[o] + sum - rhs_rest[o];
}

extern "C" int pn_sim_collect_rhs(int n_k, double dx, const int* csr_bg, const int* csr_cnt, const int* csr_buf, const double* mu, const double* lam,
                                  const double* dNx, const double* RF, const double* VF, double* rhs, void* stream) {
    PN_REQUIRE(n_k > 0 && csr_bg && csr_cnt && csr_buf && mu && lam && dNx && RF && VF && rhs);
    k_rhs_gather<<<pn_div_up(n_k, 4), 256, 0, (hipStream_t)stream>>>(n_k, pow(dx, 3.0), csr_bg, csr_cnt, csr_buf, mu, lam, dNx, RF, VF, nullptr, nullptr,
                                                                   nullptr, rhs);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

// ------------------------------------------------------------------------------------------------ stepforward
__global__ void __launch_bounds__(256) k_step_begin(int n3, double dt, const double* __restrict__ dof, const double* __restrict__ vel,
                                                    double* __restrict__ tilde, double* __restrict__ last, int* __restrict__ coop_ctl = nullptr) {
    PN_SIM_PRIO();
    const int i = threadIdx.x + blockIdx.x * blockDim.x;
    // persistent form: the barrier counters of k_substep_coop start every substep at zero (the previous substep's launch has ended: stream order)
    if (coop_ctl && blockIdx.x == 0 && threadIdx.x < 10) coop_ctl[threadIdx.x * 32] = 0;  // PnCoopCtl: xcd_ctr[8], glob, gen
    if (i >= n3) return;
    const double d = dof[i];
    tilde[i] = d + dt * vel[i];  // solver.py:575
    last[i] = d;                 // dof_last = dof.clone() (:597)
}
__global__ void __launch_bounds__(256) k_step_end(int n3, double dt, const double* __restrict__ dof, const double* __restrict__ last,
                                                  double* __restrict__ vel) {
    PN_SIM_PRIO();
    const int i = threadIdx.x + blockIdx.x * blockDim.x;
    if (i >= n3) return;
    vel[i] = (dof[i] - last[i]) / dt * 0.998;  // solver.py:602
}

static inline uint64_t pn_gather_chunks_max(int n_k, int n_IP) { return (uint64_t)n_IP * 8 / PN_GCH + (uint64_t)n_k; }
// tilde, last, momentum, tot [n_k*30 each] | P [n_IP*9] | P_csr [n_IP*8*9] | chunk sums [chunks_max*30] | plan: kc_bg [n_k+1] ints, kcount [n_k] ints,
// chunk [chunks_max] int4 | Vstore [n_IP*9]
extern "C" uint64_t pn_sim_work_doubles(int n_k, int n_IP) {
    const uint64_t ch = pn_gather_chunks_max(n_k, n_IP);
    return (uint64_t)n_k * 30 * 4 + (uint64_t)n_IP * 9 + (uint64_t)n_IP * 8 * 9 + ch * 30 + 2 * (((uint64_t)n_k + 2) / 2 + 1) + 2 * ch + 2 + (uint64_t)n_IP * 9;
}
// the plan's three arrays behind the chunk sums
struct PnGatherPlan { int* kc_bg; int* kcount; int4* chunk; };
static inline PnGatherPlan pn_gather_plan_ptrs(double* part, uint64_t chunks_max, int n_k) {
    PnGatherPlan p;
    const size_t slot = ((size_t)n_k + 2) & ~(size_t)1;  // ints, even: every array starts on 8 bytes; the chunk table on 16
    p.kc_bg = reinterpret_cast<int*>(part + chunks_max * 30);
    p.kcount = p.kc_bg + slot;
    p.chunk = reinterpret_cast<int4*>((reinterpret_cast<uintptr_t>(p.kcount + slot) + 15) & ~(uintptr_t)15);
    return p;
}
// where the per-IP rotations of the warm-started SVD live in `work` (behind everything else)
static inline double* pn_sim_vstore(double* work, int n_k, int n_IP) { return work + (pn_sim_work_doubles(n_k, n_IP) - (uint64_t)n_IP * 9); }

__global__ void __launch_bounds__(256) k_vstore_identity(int n_IP, double* __restrict__ Vstore) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n_IP * 9) Vstore[t] = (t % 9) % 4 == 0 ? 1.0 : 0.0;
}

// Once per simulator (and again whenever `work` is re-allocated): what a substep needs in `work` but does not depend on the state — the chunk
// layout of the balanced gather (rounds 1-2 rebuilt it in every substep: one launch of the ~42) and identity rotations for the warm-started SVD.
extern "C" int pn_sim_prepare(int n_k, int n_IP, const int* csr_bg, const int* csr_cnt, double* work, void* stream) {
    PN_REQUIRE(n_k > 0 && n_IP > 0 && csr_bg && csr_cnt && work);
    hipStream_t st = (hipStream_t)stream;
    const int n3 = n_k * 30;
    const uint64_t chunks_max = pn_gather_chunks_max(n_k, n_IP);
    double* part = work + 4 * (size_t)n3 + (size_t)n_IP * 9 + (size_t)n_IP * 8 * 9;
    const PnGatherPlan gp = pn_gather_plan_ptrs(part, chunks_max, n_k);
    k_gather_plan<<<1, 512, 0, st>>>(n_k, (int)chunks_max, csr_bg, csr_cnt, gp.kc_bg, gp.chunk, gp.kcount);
    k_vstore_identity<<<pn_div_up((uint64_t)n_IP * 9, 256), 256, 0, st>>>(n_IP, pn_sim_vstore(work, n_k, n_IP));
    PN_LAUNCH_CHECK();
    return PN_OK;
}

extern "C" int pn_sim_stepforward(int n_k, int n_IP, int iters, double dt, double dx, const int* topo, const int* csr_bg, const int* csr_cnt,
                                  const int* csr_buf, const double* mu, const double* lam, const double* dNx, const double* dNx_csr,
                                  const int* csr_pos, const double* Ainv, const double* Mmat, const double* dof_rest, const double* rhs_rest,
                                  const double* rhs_gravity, const double* dof_f, double* dof, double* dof_vel, double* work, int prepared, int mcadams_sweeps,
                                  void* stream) {
    PN_REQUIRE(n_k > 0 && n_IP > 0 && iters >= 0 && topo && csr_bg && csr_cnt && csr_buf && mu && lam && dNx && Ainv && Mmat);
    PN_REQUIRE(dof_rest && rhs_rest && rhs_gravity && dof_f && dof && dof_vel && work && pn_svd_sweeps_ok(mcadams_sweeps));
    hipStream_t st = (hipStream_t)stream;
    const int n = n_k * 10, n3 = n * 3;
    double* tilde = work;
    double* last = work + n3;
    double* momentum = work + 2 * (size_t)n3;
    double* tot = work + 3 * (size_t)n3;
    double* P = work + 4 * (size_t)n3;
    double* P_csr = P + (size_t)n_IP * 9;
    const uint64_t chunks_max = pn_gather_chunks_max(n_k, n_IP);
    double* part = P_csr + (size_t)n_IP * 8 * 9;
    const PnGatherPlan gp = pn_gather_plan_ptrs(part, chunks_max, n_k);
    int* kc_bg = gp.kc_bg;
    int4* chunk = gp.chunk;
    const double dx3 = pow(dx, 3.0);
    const bool pcsr = dNx_csr && csr_pos;
    // balanced gather: the lists cut into chunks of PN_GCH entries, the chunk kernel's last arriver sums them.  Without the CSR-ordered copies, or for a
    // right-hand side above ~159 KB, one gather workgroup per kernel instead (k_rhs_gather_csr / k_rhs_gather)
    const bool chunked = pcsr && (size_t)n3 * sizeof(double) <= 160 * 1024 - 1024;
    if (chunked && !prepared) k_gather_plan<<<1, 512, 0, st>>>(n_k, (int)chunks_max, csr_bg, csr_cnt, kc_bg, chunk, gp.kcount);
    double* Vstore = prepared ? pn_sim_vstore(work, n_k, n_IP) : nullptr;   // warm-started SVD (prepared == 0: every SVD starts from the identity)
    // k_elastic in one-wave workgroups: a lane's 60 loads (its kernel's 30 DOFs, its 30 shape-function gradients) are 240-B blocks of its own, so every
    // load instruction touches 64 cache lines and keeps the CU's address path busy for ~140 cycles; with 256-thread workgroups the 447 waves of the
    // chair sat four to a CU on 112 of the 256 CUs and queued on that path (31.9 -> 28.3 us per local/global iteration; 16-byte loads on top: nothing)
    const uint32_t el_blocks = pn_div_up((uint64_t)n_IP * 8, 64);
    // ... and the matrix products in one-wave workgroups (two rows each) as well: beside the render lanes' persistent workgroups a launch starts when its
    // workgroups find room, and a single wave finds it sooner than four (start-to-start gap behind k_matvec3 in the pipeline: profiles/r04_sim_stamps.txt)
    const uint32_t mv_blocks = pn_div_up(n, 2);
    // the substep's two elementwise launches ride on the matrix products next to them; k_step_begin / k_step_end as launches when the gather is not
    // chunked or there is no iteration to carry the epilogue
    const bool ends = chunked && iters >= 1;
    if (ends) {
        k_matvec3<<<mv_blocks, 64, 0, st>>>(n, Mmat, dof, momentum, 1, dof_f, rhs_gravity, dof_vel, dt, last);  // dof_tilde on the fly, dof_last = dof
    } else {
        k_step_begin<<<pn_div_up(n3, 256), 256, 0, st>>>(n3, dt, dof, dof_vel, tilde, last);
        k_matvec3<<<mv_blocks, 64, 0, st>>>(n, Mmat, tilde, momentum, 1, dof_f, rhs_gravity);  // compute_momentum (:574-576)
    }
    for (int it = 0; it < iters; it++) {
        if (mcadams_sweeps)
            k_elastic<true><<<el_blocks, 64, 0, st>>>(n_IP, topo, dNx, dof, nullptr, nullptr, nullptr, pcsr ? nullptr : P, mu, lam, dx3, pcsr ? csr_pos : nullptr,
                                                      pcsr ? P_csr : nullptr, Vstore, mcadams_sweeps);
        else
            k_elastic<false><<<el_blocks, 64, 0, st>>>(n_IP, topo, dNx, dof, nullptr, nullptr, nullptr, pcsr ? nullptr : P, mu, lam, dx3, pcsr ? csr_pos : nullptr,
                                                       pcsr ? P_csr : nullptr, Vstore);
        if (chunked)
            k_rhs_gather_chunk<<<(uint32_t)chunks_max, PN_GCH * 8, 0, st>>>(chunk, dNx_csr, P_csr, part, gp.kcount, kc_bg, momentum, rhs_rest, tot);
        else if (dNx_csr)  // CSR-ordered copy of dNx available: the coalesced one-workgroup-per-kernel gather
            k_rhs_gather_csr<<<n_k, 1024, 0, st>>>(n_k, csr_bg, csr_cnt, csr_buf, dNx_csr, P, pcsr ? P_csr : nullptr, momentum, rhs_rest, tot);
        else
            k_rhs_gather<<<pn_div_up(n_k, 4), 256, 0, st>>>(n_k, dx3, csr_bg, csr_cnt, csr_buf, mu, lam, dNx, nullptr, nullptr, P, momentum, rhs_rest, tot);
        if (ends && it == iters - 1) k_matvec3<<<mv_blocks, 64, 0, st>>>(n, Ainv, tot, dof, 3, dof_rest, last, nullptr, dt, nullptr, dof_vel);  // + vel (:602)
        else k_matvec3<<<mv_blocks, 64, 0, st>>>(n, Ainv, tot, dof, 2, dof_rest, nullptr);  // x = G @ rhs ; dof = dof_rest + x (:600-601)
    }
    if (!ends) k_step_end<<<pn_div_up(n3, 256), 256, 0, st>>>(n3, dt, dof, last, dof_vel);
    PN_LAUNCH_CHECK();
    return PN_OK;
}
