// What pn_contact.hip needs of pn_sdf.hip: the launch that adds the signed-distance grids' contact terms to the analytic colliders' (include/pienerf_hip.h:
// pn_sim_contact_sdf_rhs has the law).  The arguments have been checked by the caller.
#pragma once
#include "pn_common.h"

int pn_sdf_points_launch(int n_k, int n_IP, const pn_contact_state* st, const pn_sdf_state* sdf, double dt, const double* dof, const double* dof_vel,
                         const int* topo, const double* Nx, double* accel, hipStream_t stream);
