// tb_mech_tet4.hip — instances of the tetrahedral mechanics kernels for the first-order field (tb_mech_tet.hpp; a translation unit per field keeps the build parallel)
#include "tb_mech_tet.hpp"

namespace tb {
int launch_hyperelastic_tet4(tb_form *f, tb_pattern *p, int strategy, const double *d_u, double *d_nz, double *d_r) { return dispatch_tet<4>(f, p, strategy, d_u, d_nz, d_r); }
} // namespace tb
