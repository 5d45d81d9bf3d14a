// The substep's global solve as a block-sparse preconditioned conjugate gradient (included by pn_sim.hip only, behind pn_sim_cells.h).
#pragma once
#include "pn_sim_cells.h"

// ------------------------------------------------------------------------------------------------ the global step without a dense matrix
// The system block of solver.py:505-511 is sparse by construction: an integration point couples the 8 kernels of its kernel-grid cell, so a kernel's block
// row holds at most 27 blocks of 10 x 10 (28 with a pinned point that names kernel 0).  Instead of the pre-inverted dense matrix (pn_sim_stepforward_cells:
// [10 n_k]^2 doubles, 9 GB at kres 15) this form keeps the matrix in block-sparse rows (BSR: rowptr [n_k + 1], col [nnzb] ascending inside a row, blocks
// [nnzb][10][10] row-major) and solves A X = B for the three coordinate columns at once by conjugate gradients preconditioned with the inverted diagonal
// blocks.  The columns share every product but have their own alpha, beta and stopping state.
//
// Mapping.  One wave owns one kernel = one block row = 10 matrix rows x 3 columns = 30 outputs, four waves to a workgroup:
//   * a block is 800 contiguous bytes: lanes 0..49 read one double2 each (entries 2l, 2l + 1 of the 100: matrix row l / 5, columns 2 (l % 5) and the next),
//     and the six X values they multiply are 48 contiguous, 16-byte aligned bytes of the column kernel's 240-byte row; the five lanes of a matrix row are
//     added through LDS in lane order, so lane q < 30 ends up with output q of the kernel (o = 30 k + q, the layout of dof);
//   * the kernel's 10 rows are in one wave, so z = Dinv r (a 10 x 10 block times the kernel's own 10 x 3) needs no second pass;
//   * every dot product is a sum of per-workgroup partials (waves in ascending order, a wave's 10 rows in ascending order), stored in `work` and re-added in
//     ascending workgroup order by every workgroup of the NEXT launch that needs it: no floating-point atomics, no device-wide barrier, no waiting — only
//     the order of plain launches on one stream.  Two runs with the same history give the same bits.
// Launches per solve: start (r = b - A x0, z, the first partials), then per CG iteration
//   k_pcg_direction   p = z + beta p_old formed on the fly from the gathered rows into the other p buffer, Ap = A p, the p.Ap partials;
//   k_pcg_update      x += alpha p, r -= alpha Ap, z = Dinv r, the r.z and r.r partials;
// and k_pcg_finish (the last stopping test, the statistics and, in a substep, dof = dof_rest + x with the velocity on the last local/global iteration).
// The scalar state of the three columns (flag, iteration count, r.z, |b|^2, all-frozen flag) is a small record written by workgroup 0 of a launch for the
// next launch; two records alternate, so no launch reads the record it writes.  The host enqueues max_iters iterations; once every column is frozen the
// record's `done` makes the remaining launches return at once (workgroup 0 hands the record on).
#define PN_PCG_WAVES 4            // kernels (block rows) per workgroup
#define PN_PCG_STATE_DOUBLES 16   // room for one PcgState
#define PN_PCG_CONVERGED 1
#define PN_PCG_BROKEN 2

struct PcgState {
    double rz[3];     // r.z of the iterate the columns stand at
    double bb[3];     // |b|^2 over the active kernels' rows
    int flag[3];      // 0 running, PN_PCG_CONVERGED, PN_PCG_BROKEN (p.Ap <= 0 or not finite): the last two are frozen
    int iters[3];     // updates applied to the column
    int done;         // every column frozen
    int pad;
};
static_assert(sizeof(PcgState) <= PN_PCG_STATE_DOUBLES * sizeof(double), "PcgState outgrew its slot in the work area");

// sum over the workgroups of the launch that wrote them, ascending, sixteen loads in flight
__device__ inline double pcg_sum_partials(const double* __restrict__ part, int n_part, int c) {
    double sum = 0.0;
    for (int j0 = 0; j0 < n_part; j0 += 16) {
        double v[16];
#pragma unroll
        for (int u = 0; u < 16; u++) v[u] = part[(size_t)min(j0 + u, n_part - 1) * 3 + c];
#pragma unroll
        for (int u = 0; u < 16; u++) if (j0 + u < n_part) sum += v[u];
    }
    return sum;
}

// six consecutive doubles of a [n_k][30] vector starting at an even entry: 48 bytes, 16-byte aligned when the vector's base is — three double2 loads
__device__ inline void pcg_load6(const double* __restrict__ p, double (&x)[6]) {
    const double2* __restrict__ q = reinterpret_cast<const double2*>(p);
    const double2 a = q[0], b = q[1], c = q[2];
    x[0] = a.x; x[1] = a.y; x[2] = b.x; x[3] = b.y; x[4] = c.x; x[5] = c.y;
}
__host__ inline bool pcg_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Lane's share of block row k times X: acc[q] over the lane's two matrix entries per block.  xf(j, e, x) fills x[0..5] = the column kernel j's entries e .. e + 5
// of a [n_k][30] vector (e = 3 * column: two matrix columns x three coordinates).  Lanes >= 50 idle.
template <class XF>
__device__ inline void pcg_row_partial(const int* __restrict__ rowptr, const int* __restrict__ col, const double* __restrict__ blocks, int k, int lane, XF xf,
                                       double (&acc)[3]) {
    acc[0] = acc[1] = acc[2] = 0.0;
    if (lane >= 50) return;
    const int e = (lane % 5) * 6;
    const int b1 = rowptr[k + 1];
    int b = rowptr[k];
    for (; b + 4 <= b1; b += 4) {   // four blocks in flight
        double2 a[4];
        double x[4][6];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            a[u] = reinterpret_cast<const double2*>(blocks + (size_t)(b + u) * 100)[lane];
            xf(col[b + u], e, x[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; u++)
#pragma unroll
            for (int q = 0; q < 3; q++) acc[q] += a[u].x * x[u][q] + a[u].y * x[u][3 + q];
    }
    for (; b < b1; b++) {
        const double2 a = reinterpret_cast<const double2*>(blocks + (size_t)b * 100)[lane];
        double x[6];
        xf(col[b], e, x);
#pragma unroll
        for (int q = 0; q < 3; q++) acc[q] += a.x * x[q] + a.y * x[3 + q];
    }
}

// the five lanes of a matrix row, added in lane order: lane q < 30 of every wave returns output q of its kernel.  All threads of the workgroup call it.
__device__ inline double pcg_row_reduce(double (*s_acc)[50][3], int w, int lane, const double (&acc)[3]) {
    __syncthreads();   // (the buffer may still be read from a previous call)
    if (lane < 50) { s_acc[w][lane][0] = acc[0]; s_acc[w][lane][1] = acc[1]; s_acc[w][lane][2] = acc[2]; }
    __syncthreads();
    double y = 0.0;
    if (lane < 30) {
        const int r = lane / 3, q = lane - r * 3;
#pragma unroll
        for (int u = 0; u < 5; u++) y += s_acc[w][r * 5 + u][q];
    }
    return y;
}

// z = Dinv_k r for the wave's kernel: lane q < 30 holds r[q]; returns z[q].  All threads of the workgroup call it.
__device__ inline double pcg_apply_dinv(double (*s_vec)[30], const double* __restrict__ Dinv, int k, bool on, int w, int lane, double r) {
    __syncthreads();
    if (lane < 30) s_vec[w][lane] = r;
    __syncthreads();
    double z = 0.0;
    if (on && lane < 30) {
        const int row = lane / 3, q = lane - row * 3;
        const double* __restrict__ d = Dinv + (size_t)k * 100 + row * 10;
#pragma unroll
        for (int j = 0; j < 10; j++) z += d[j] * s_vec[w][j * 3 + q];
    }
    return z;
}

// a workgroup's partial of up to three dot products: v[i] is this lane's term (lane < 30: column lane % 3) of product i; waves and rows in ascending order
template <int N>
__device__ inline void pcg_store_partials(double (*s_dot)[PN_PCG_WAVES][30], int w, int lane, int t, const double (&v)[N], double* const (&part)[N]) {
    __syncthreads();
    if (lane < 30) {
#pragma unroll
        for (int i = 0; i < N; i++) s_dot[i][w][lane] = v[i];
    }
    __syncthreads();
    if (t < 3 * N) {
        const int i = t / 3, c = t - i * 3;
        double s = 0.0;
#pragma unroll
        for (int ww = 0; ww < PN_PCG_WAVES; ww++)
#pragma unroll
            for (int r = 0; r < 10; r++) s += s_dot[i][ww][r * 3 + c];
        part[i][(size_t)blockIdx.x * 3 + c] = s;
    }
}

// ------------------------------------------------------------------------------------------------ Y = A X with k_matvec3's epilogues
// modes 0..3, Xv / dt / copy_out / vel_out as k_matvec3 has them (the momentum product and a substep's last update cost no launch of their own)
__global__ void __launch_bounds__(PN_PCG_WAVES * 64) k_bsr_matvec3(int n_k, const int* __restrict__ rowptr, const int* __restrict__ col,
                                                                    const double* __restrict__ blocks, const double* __restrict__ X, double* __restrict__ Y,
                                                                    int mode, const double* __restrict__ add1, const double* __restrict__ add2,
                                                                    const double* __restrict__ Xv, double dt, double* __restrict__ copy_out,
                                                                    double* __restrict__ vel_out) {
    PN_SIM_PRIO();
    __shared__ double s_acc[PN_PCG_WAVES][50][3];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int k = blockIdx.x * PN_PCG_WAVES + w;
    const bool valid = k < n_k;
    double acc[3];
    if (valid)
        pcg_row_partial(rowptr, col, blocks, k, lane, [&](int j, int e, double (&x)[6]) {
            pcg_load6(X + (size_t)j * 30 + e, x);
            if (Xv) {
                double v[6];
                pcg_load6(Xv + (size_t)j * 30 + e, v);
#pragma unroll
                for (int i = 0; i < 6; i++) x[i] = x[i] + dt * v[i];
            }
        }, acc);
    else acc[0] = acc[1] = acc[2] = 0.0;
    double v = pcg_row_reduce(s_acc, w, lane, acc);
    if (valid && lane < 30) {
        const size_t o = (size_t)k * 30 + lane;
        if (copy_out) copy_out[o] = X[o];
        if (mode == 1) v = v + add1[o] + add2[o];
        else if (mode >= 2) v = add1[o] + v;
        Y[o] = v;
        if (mode == 3) vel_out[o] = (v - add2[o]) / dt * 0.998;
    }
}

extern "C" int pn_sim_bsr_matvec3(int n_k, const int* rowptr, const int* col, const double* blocks, const double* X, double* Y, void* stream) {
    PN_REQUIRE(n_k > 0 && rowptr && col && blocks && X && Y && X != Y && pcg_aligned16(blocks) && pcg_aligned16(X));
    k_bsr_matvec3<<<pn_div_up(n_k, PN_PCG_WAVES), PN_PCG_WAVES * 64, 0, (hipStream_t)stream>>>(n_k, rowptr, col, blocks, X, Y, 0, nullptr, nullptr, nullptr,
                                                                                               0.0, nullptr, nullptr);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

// ------------------------------------------------------------------------------------------------ the solve
struct PcgWork {   // views into the work area
    double *r, *z, *p[2], *Ap, *x;
    double *part_rr, *part_rz, *part_bb, *part_pAp;
    PcgState* state[2];
    int n_part;
};
extern "C" uint64_t pn_sim_pcg_work_doubles(int n_k) {
    return (uint64_t)n_k * 30 * 6 + (uint64_t)pn_div_up(n_k, PN_PCG_WAVES) * 3 * 4 + 2 * PN_PCG_STATE_DOUBLES;
}
static PcgWork pcg_work_views(int n_k, double* work) {
    PcgWork v;
    const size_t n3 = (size_t)n_k * 30;
    v.n_part = (int)pn_div_up(n_k, PN_PCG_WAVES);
    v.r = work; v.z = work + n3; v.p[0] = work + 2 * n3; v.p[1] = work + 3 * n3; v.Ap = work + 4 * n3; v.x = work + 5 * n3;
    double* q = work + 6 * n3;
    const size_t np3 = (size_t)v.n_part * 3;
    v.part_rr = q; v.part_rz = q + np3; v.part_bb = q + 2 * np3; v.part_pAp = q + 3 * np3;
    q += 4 * np3;
    v.state[0] = reinterpret_cast<PcgState*>(q);
    v.state[1] = reinterpret_cast<PcgState*>(q + PN_PCG_STATE_DOUBLES);
    return v;
}

// r = b - A x0, z = Dinv r and the partials of |b|^2, r.r, r.z over the active kernels' rows.  x0 = X0, or X0 - rest where `rest` is given (a substep's warm
// start dof - dof_rest), then also written to xout; rows and columns of inactive kernels are left out (their x counts as 0, their r, z stay 0).
__global__ void __launch_bounds__(PN_PCG_WAVES * 64) k_pcg_start(int n_k, const int* __restrict__ rowptr, const int* __restrict__ col,
                                                                  const double* __restrict__ A, const double* __restrict__ Dinv,
                                                                  const int* __restrict__ active, const double* __restrict__ B,
                                                                  const double* __restrict__ X0, const double* __restrict__ rest, double* __restrict__ xout,
                                                                  double* __restrict__ r_, double* __restrict__ z_, double* __restrict__ part_rr,
                                                                  double* __restrict__ part_rz, double* __restrict__ part_bb, PcgState* __restrict__ sout) {
    PN_SIM_PRIO();
    __shared__ double s_acc[PN_PCG_WAVES][50][3];
    __shared__ double s_vec[PN_PCG_WAVES][30];
    __shared__ double s_dot[3][PN_PCG_WAVES][30];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int k = blockIdx.x * PN_PCG_WAVES + w;
    const bool valid = k < n_k;
    const bool on = valid && active[k] != 0;
    if (blockIdx.x == 0 && t == 0) {
        PcgState s = {};
        *sout = s;
    }
    double acc[3] = {0.0, 0.0, 0.0};
    if (on)
        pcg_row_partial(rowptr, col, A, k, lane, [&](int j, int e, double (&x)[6]) {
            const size_t o = (size_t)j * 30 + e;
            const bool aj = active[j] != 0;
            pcg_load6(X0 + o, x);
            if (rest) {
                double v[6];
                pcg_load6(rest + o, v);
#pragma unroll
                for (int i = 0; i < 6; i++) x[i] = x[i] - v[i];
            }
#pragma unroll
            for (int i = 0; i < 6; i++) x[i] = aj ? x[i] : 0.0;
        }, acc);
    const double y = pcg_row_reduce(s_acc, w, lane, acc);
    const size_t o = (size_t)k * 30 + lane;
    double r = 0.0, b = 0.0;
    if (on && lane < 30) { b = B[o]; r = b - y; }
    const double z = pcg_apply_dinv(s_vec, Dinv, k, on, w, lane, r);
    if (valid && lane < 30) {
        r_[o] = r;
        z_[o] = z;
        if (rest) xout[o] = on ? X0[o] - rest[o] : 0.0;
    }
    const double v[3] = {r * r, r * z, b * b};
    double* const parts[3] = {part_rr, part_rz, part_bb};
    pcg_store_partials<3>(s_dot, w, lane, t, v, parts);
}

// launch one of an iteration: the stopping test on the partials the launch before left, then p = z + beta p_old (p = z in the first), Ap and the p.Ap partials
__global__ void __launch_bounds__(PN_PCG_WAVES * 64) k_pcg_direction(int n_k, int n_part, int first, double tol, const int* __restrict__ rowptr,
                                                                      const int* __restrict__ col, const double* __restrict__ A,
                                                                      const int* __restrict__ active, const double* __restrict__ z_,
                                                                      const double* __restrict__ p_old, double* __restrict__ p_new, double* __restrict__ Ap_,
                                                                      double* __restrict__ x_, const double* __restrict__ part_rr,
                                                                      const double* __restrict__ part_rz, const double* __restrict__ part_bb,
                                                                      double* __restrict__ part_pAp, const PcgState* __restrict__ sin,
                                                                      PcgState* __restrict__ sout) {
    PN_SIM_PRIO();
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (sin->done) {
        if (blockIdx.x == 0 && t == 0) *sout = *sin;
        return;
    }
    __shared__ double s_acc[PN_PCG_WAVES][50][3];
    __shared__ double s_dot[1][PN_PCG_WAVES][30];
    __shared__ double s_sum[3][3];
    if (t < (first ? 9 : 6)) {
        const int i = t / 3;
        s_sum[i][t - i * 3] = pcg_sum_partials(i == 0 ? part_rr : i == 1 ? part_rz : part_bb, n_part, t - i * 3);
    }
    __syncthreads();
    // every thread takes the three columns' decisions from the same numbers
    int flag[3];
    double beta[3], rz[3], bb[3];
    bool zero_col[3];
    bool any = false;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        flag[c] = sin->flag[c];
        bb[c] = first ? s_sum[2][c] : sin->bb[c];
        rz[c] = flag[c] == 0 ? s_sum[1][c] : sin->rz[c];
        zero_col[c] = false;
        if (flag[c] == 0) {
            if (first && bb[c] == 0.0) { flag[c] = PN_PCG_CONVERGED; zero_col[c] = true; }   // |b| = 0: x = 0, converged, no iteration
            else if (sqrt(s_sum[0][c]) <= tol * sqrt(bb[c])) flag[c] = PN_PCG_CONVERGED;
        }
        beta[c] = first ? 0.0 : rz[c] / sin->rz[c];
        any = any || flag[c] == 0;
    }
    if (blockIdx.x == 0 && t == 0) {
        PcgState s = *sin;
#pragma unroll
        for (int c = 0; c < 3; c++) { s.flag[c] = flag[c]; s.rz[c] = rz[c]; s.bb[c] = bb[c]; }
        s.done = any ? 0 : 1;
        *sout = s;
    }
    const int k = blockIdx.x * PN_PCG_WAVES + w;
    const bool valid = k < n_k;
    const bool on = valid && active[k] != 0;
    const int c = lane % 3;
    const size_t o = (size_t)k * 30 + lane;
    if (valid && lane < 30 && zero_col[c]) x_[o] = 0.0;
    if (!any) return;
    double acc[3] = {0.0, 0.0, 0.0};
    if (on)
        pcg_row_partial(rowptr, col, A, k, lane, [&](int j, int e, double (&x)[6]) {
            // an inactive kernel's p is never written and a frozen column's not since it froze (never, if |b| = 0): the first is not loaded, the second is
            // selected away, both count as 0 — nothing of `work` that no launch of this solve has written enters the arithmetic
            const size_t oj = (size_t)j * 30 + e;
            const bool aj = active[j] != 0;
            double zz[6], pp[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            pcg_load6(z_ + oj, zz);
            if (!first && aj) pcg_load6(p_old + oj, pp);
#pragma unroll
            for (int i = 0; i < 6; i++) x[i] = (aj && flag[i % 3] == 0) ? (first ? zz[i] : zz[i] + beta[i % 3] * pp[i]) : 0.0;
        }, acc);
    const double y = pcg_row_reduce(s_acc, w, lane, acc);
    double pAp = 0.0;
    if (on && lane < 30 && flag[c] == 0) {   // a frozen column's p and Ap are never written again
        const double zz = z_[o];
        const double p = first ? zz : zz + beta[c] * p_old[o];
        p_new[o] = p;
        Ap_[o] = y;
        pAp = p * y;
    }
    const double v[1] = {pAp};
    double* const parts[1] = {part_pAp};
    pcg_store_partials<1>(s_dot, w, lane, t, v, parts);
}

// launch two: alpha from the p.Ap partials (p.Ap <= 0 or not finite freezes the column, unconverged), x, r, z = Dinv r, the r.r and r.z partials
__global__ void __launch_bounds__(PN_PCG_WAVES * 64) k_pcg_update(int n_k, int n_part, const double* __restrict__ Dinv, const int* __restrict__ active,
                                                                   const double* __restrict__ p_, const double* __restrict__ Ap_, double* __restrict__ x_,
                                                                   double* __restrict__ r_, double* __restrict__ z_, const double* __restrict__ part_pAp,
                                                                   double* __restrict__ part_rr, double* __restrict__ part_rz,
                                                                   const PcgState* __restrict__ sin, PcgState* __restrict__ sout) {
    PN_SIM_PRIO();
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (sin->done) {
        if (blockIdx.x == 0 && t == 0) *sout = *sin;
        return;
    }
    __shared__ double s_vec[PN_PCG_WAVES][30];
    __shared__ double s_dot[2][PN_PCG_WAVES][30];
    __shared__ double s_sum[3];
    if (t < 3) s_sum[t] = sin->flag[t] == 0 ? pcg_sum_partials(part_pAp, n_part, t) : 0.0;
    __syncthreads();
    int flag[3];
    double alpha[3];
    bool any = false;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        flag[c] = sin->flag[c];
        alpha[c] = 0.0;
        if (flag[c] == 0) {
            const double pAp = s_sum[c];
            if (!(pAp > 0.0) || !isfinite(pAp)) flag[c] = PN_PCG_BROKEN;
            else alpha[c] = sin->rz[c] / pAp;
        }
        any = any || flag[c] == 0;
    }
    if (blockIdx.x == 0 && t == 0) {
        PcgState s = *sin;
#pragma unroll
        for (int c = 0; c < 3; c++) { s.flag[c] = flag[c]; if (flag[c] == 0) s.iters[c] += 1; }
        s.done = any ? 0 : 1;
        *sout = s;
    }
    if (!any) return;
    const int k = blockIdx.x * PN_PCG_WAVES + w;
    const bool valid = k < n_k;
    const bool on = valid && active[k] != 0;
    const int c = lane % 3;
    const size_t o = (size_t)k * 30 + lane;
    const bool mine = on && lane < 30 && flag[c] == 0;
    double r = 0.0;
    if (mine) {
        x_[o] = x_[o] + alpha[c] * p_[o];
        r = r_[o] - alpha[c] * Ap_[o];
        r_[o] = r;
    }
    const double z = pcg_apply_dinv(s_vec, Dinv, k, on, w, lane, r);   // (a frozen column's entries of s_vec are 0 here; its z is not written)
    if (mine) z_[o] = z;
    const double v[2] = {mine ? r * r : 0.0, mine ? r * z : 0.0};
    double* const parts[2] = {part_rr, part_rz};
    pcg_store_partials<2>(s_dot, w, lane, t, v, parts);
}

// behind the last iteration: the stopping test once more, the statistics (stats[0] solves, stats[1] unconverged columns, stats[2 + 6 slot + c] iterations and
// stats[5 + 6 slot + c] flag of column c), inactive kernels' rows of x = 0 and, with dof_rest, dof = dof_rest + x (and the substep's velocity with `last`)
__global__ void __launch_bounds__(256) k_pcg_finish(int n_k, int n_part, double tol, const int* __restrict__ active, double* __restrict__ x_,
                                                    const double* __restrict__ part_rr, const PcgState* __restrict__ sin, int* __restrict__ stats, int slot,
                                                    const double* __restrict__ dof_rest, double* __restrict__ dof, const double* __restrict__ last, double dt,
                                                    double* __restrict__ dof_vel) {
    PN_SIM_PRIO();
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g == 0) {
        int bad = 0;
        for (int c = 0; c < 3; c++) {
            int flag = sin->flag[c];
            if (flag == 0 && sqrt(pcg_sum_partials(part_rr, n_part, c)) <= tol * sqrt(sin->bb[c])) flag = PN_PCG_CONVERGED;
            stats[2 + 6 * slot + c] = sin->iters[c];
            stats[5 + 6 * slot + c] = flag;
            bad += flag != PN_PCG_CONVERGED;
        }
        stats[0] += 1;
        stats[1] += bad;
    }
    if (g >= n_k * 30) return;
    const bool on = active[g / 30] != 0;
    if (!dof_rest) {
        if (!on) x_[g] = 0.0;
        return;
    }
    const double v = dof_rest[g] + (on ? x_[g] : 0.0);
    dof[g] = v;
    if (last) dof_vel[g] = (v - last[g]) / dt * 0.998;
}

// the launches of one solve; x0 / rest: see k_pcg_start; x: where the solution is kept (X itself at op level)
static void pcg_enqueue(int n_k, const int* rowptr, const int* col, const double* A, const double* Dinv, const int* active, const double* B, const double* x0,
                        const double* rest, double* x, double tol, int max_iters, const PcgWork& v, int* stats, int slot, const double* dof_rest, double* dof,
                        const double* last, double dt, double* dof_vel, hipStream_t st) {
    const uint32_t nb = pn_div_up(n_k, PN_PCG_WAVES), nt = PN_PCG_WAVES * 64;
    k_pcg_start<<<nb, nt, 0, st>>>(n_k, rowptr, col, A, Dinv, active, B, x0, rest, x, v.r, v.z, v.part_rr, v.part_rz, v.part_bb, v.state[0]);
    for (int it = 0; it < max_iters; it++) {
        k_pcg_direction<<<nb, nt, 0, st>>>(n_k, v.n_part, it == 0, tol, rowptr, col, A, active, v.z, v.p[(it + 1) & 1], v.p[it & 1], v.Ap, x, v.part_rr,
                                           v.part_rz, v.part_bb, v.part_pAp, v.state[0], v.state[1]);
        k_pcg_update<<<nb, nt, 0, st>>>(n_k, v.n_part, Dinv, active, v.p[it & 1], v.Ap, x, v.r, v.z, v.part_pAp, v.part_rr, v.part_rz, v.state[1], v.state[0]);
    }
    k_pcg_finish<<<pn_div_up((uint64_t)n_k * 30, 256), 256, 0, st>>>(n_k, v.n_part, tol, active, x, v.part_rr, v.state[0], stats, slot, dof_rest, dof, last, dt,
                                                                      dof_vel);
}

extern "C" int pn_sim_pcg_solve(int n_k, const int* rowptr, const int* col, const double* A, const double* Dinv, const int* active, const double* B, double* X,
                                double tol, int max_iters, double* work, int* stats, void* stream) {
    PN_REQUIRE(n_k > 0 && rowptr && col && A && Dinv && active && B && X && work && stats && tol >= 0.0 && max_iters >= 1);
    PN_REQUIRE(pcg_aligned16(A) && pcg_aligned16(X) && pcg_aligned16(work));
    const PcgWork v = pcg_work_views(n_k, work);
    pcg_enqueue(n_k, rowptr, col, A, Dinv, active, B, X, nullptr, X, tol, max_iters, v, stats, 0, nullptr, nullptr, nullptr, 0.0, nullptr, (hipStream_t)stream);
    PN_LAUNCH_CHECK();
    return PN_OK;
}

// pn_sim_stepforward_cells with the global step solved instead of multiplied: momentum through the BSR mass product, then per local/global iteration
// k_cells_elastic_gather (unchanged), a solve warm-started from dof - dof_rest, dof = dof_rest + x; the last iteration writes dof_vel as mode 3 does
extern "C" int pn_sim_stepforward_cells_pcg(int n_k, int n_chunks, int iters, double dt, double dx, const int* chunk_tab, const double* dNx_cell,
                                            const double* mu_cell, const double* lam_cell, const int* kp_bg, const int* kp_pos, const int* rowptr,
                                            const int* col, const double* A, const double* M, const double* Dinv, const int* active, double tol, int max_iters,
                                            const double* dof_rest, const double* rhs_rest, const double* rhs_gravity, const double* dof_f, double* dof,
                                            double* dof_vel, double* work, double* pcg_work, int* stats, int mcadams_sweeps, void* stream) {
    PN_REQUIRE(n_k > 0 && n_chunks > 0 && iters >= 1 && chunk_tab && dNx_cell && mu_cell && lam_cell && kp_bg && kp_pos && rowptr && col && A && M);
    PN_REQUIRE(Dinv && active && tol >= 0.0 && max_iters >= 1 && pcg_work && stats);
    PN_REQUIRE(pcg_aligned16(A) && pcg_aligned16(M) && pcg_aligned16(dof) && pcg_aligned16(dof_vel) && pcg_aligned16(dof_rest) && pcg_aligned16(pcg_work));
    PN_REQUIRE(dof_rest && rhs_rest && rhs_gravity && dof_f && dof && dof_vel && work && pn_svd_sweeps_ok(mcadams_sweeps));
    hipStream_t st = (hipStream_t)stream;
    const size_t n3 = (size_t)n_k * 30;
    double* last = work;
    double* momentum = work + n3;
    double* tot = work + 2 * n3;
    double* part = work + 3 * n3;
    double* Vstore = part + (size_t)n_chunks * 240;
    int* kcount = reinterpret_cast<int*>(Vstore + (size_t)n_chunks * PN_CELL_IPS * 9);
    const double dx3 = pow(dx, 3.0);
    const PcgWork v = pcg_work_views(n_k, pcg_work);
    // compute_momentum with dof_tilde = dof + dt * vel on the fly and dof_last = dof (solver.py:574-576,597)
    k_bsr_matvec3<<<pn_div_up(n_k, PN_PCG_WAVES), PN_PCG_WAVES * 64, 0, st>>>(n_k, rowptr, col, M, dof, momentum, 1, dof_f, rhs_gravity, dof_vel, dt, last, nullptr);
    for (int it = 0; it < iters; it++) {
        if (mcadams_sweeps)
            k_cells_elastic_gather<true><<<n_chunks, PN_CELL_WAVES * 64, 0, st>>>(chunk_tab, reinterpret_cast<const double2*>(dNx_cell), mu_cell, lam_cell, dof,
                                                                                   dx3, Vstore, part, kcount, kp_bg, kp_pos, momentum, rhs_rest, tot,
                                                                                   mcadams_sweeps);
        else
            k_cells_elastic_gather<false><<<n_chunks, PN_CELL_WAVES * 64, 0, st>>>(chunk_tab, reinterpret_cast<const double2*>(dNx_cell), mu_cell, lam_cell, dof,
                                                                                    dx3, Vstore, part, kcount, kp_bg, kp_pos, momentum, rhs_rest, tot, 0);
        pcg_enqueue(n_k, rowptr, col, A, Dinv, active, tot, dof, dof_rest, v.x, tol, max_iters, v, stats, it, dof_rest, dof, it == iters - 1 ? last : nullptr, dt,
                    dof_vel, st);   // :600-602
    }
    PN_LAUNCH_CHECK();
    return PN_OK;
}
