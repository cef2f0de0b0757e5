// tb_interface_planners.hpp — the planning half of the interface unit (tb_interface.hip): a pure host function from the dof lists of the
// zero-thickness interface elements and a CSR pattern to the contribution list the gather kernel reads.  Standard library only, no device, no
// environment, no global state; tests/interface_planner_driver.cpp calls it without a GPU.
#pragma once
#include <cstdint>
#include <vector>

#include "tb_planners.hpp"

namespace tb {
namespace ifplan {

// An interface element has 2·nf dofs: the nf facet dofs of side a (Ferrite's facet-node order of a's local facet), then their copies on side b in
// the same order.  Its element matrix is  Kₑ[I, J] = s(I, J) · F[I mod nf][J mod nf]  with F = G ∫ N_i N_j dΓ (nf × nf, stored row-major per element
// by k_interface_facet) and s = −1 where I and J lie on the same side, +1 across (the jump–jump product of src/modeling/core/diffusion.jl:105-127).
//
// Plan: one record per touched non-zero, ascending; its contributions in the fixed order "ascending interface element, then local entry
// I·2nf + J".  A contribution is  (e·nf² + i·nf + j) << 1 | (1 where s = −1): the position of F's entry in the facet-matrix buffer and its sign.
struct InterfaceHost {
    std::vector<int64_t> nz;   // touched non-zeros, ascending
    std::vector<int64_t> ptr;  // nz.size() + 1 → src
    std::vector<uint32_t> src; // n · (2nf)² contributions
};

// edofs: n × 2nf dofs, 0-based.  TB_OK (0), plan::ERR_PATTERN when a coupling of an interface element is missing from the pattern,
// plan::ERR_BAD_ARG for a dof outside the pattern or more elements than the 31-bit positions hold.
int contributions(int64_t n, int nf, const int32_t *edofs, const plan::PatternView &p, InterfaceHost &out);

} // namespace ifplan
} // namespace tb
