// tb_mech_gather.hpp — launchers of tb_mech_gather.hip: the second pass of the element strategy on three-component hexahedral fields
#pragma once
#include "tb_internal.h"

namespace tb {
// Once per pattern (and in front of any graph capture): the node list, the check of the node rows, the node records of the staged gather.
// Afterwards p->gnodes_state > 0: the staged gather serves any range of nodes; < 0: the direct gather takes the mesh (all nodes in one launch).
int prepare_tangent_gather(tb_pattern *p);
// node rows [n0, n1) of the tangent from the stored element matrices d_ke, on `stream`
int launch_tangent_gather(tb_pattern *p, hipStream_t stream, int64_t n0, int64_t n1, const double *d_ke, double *d_nz);
// r[d] = Σ (in cell order) of the stored element residuals d_re
int launch_residual_gather(tb_mesh *m, const double *d_re, double *d_r);
} // namespace tb
