"""thunderbolt.jl_amd — MI355X (gfx950) backend for Thunderbolt.jl's per-cell FE integration and
pointwise reaction hot path.  The compute lives in libtbhip.so (hand-written HIP, C ABI in
include/tbhip.h); this package is the host-side mirror of the reference's operator API.
Import as ``import thunderbolt_jl_amd`` (shim at the repository root)."""
from . import _lib
from ._lib import TBError, build_library, lib  # noqa: F401
from .api import *  # noqa: F401,F403
from . import distributed  # noqa: F401
from . import meshio  # noqa: F401
from . import coordinates  # noqa: F401
from .coordinates import (compute_lv_coordinate_system, compute_midmyocardial_section_coordinate_system, create_microstructure_model,  # noqa: F401
                          create_lumped_microstructure_model, ODB25LTMicrostructureParameters, evaluate_coordinate_axes, evaluate_coordinate,
                          wrap_rotational, apicobasal_from_laplace)
from .meshgen import generate_ring_mesh, generate_open_ring_mesh, generate_ideal_lv_mesh_hex, ideal_lv_microstructure, uniform_refinement  # noqa: F401
from .meshgen import uniform_refinement_with_maps, GridHierarchy  # noqa: F401
from . import amg  # noqa: F401
from .amg import AMGPrecon, AlgebraicHierarchy  # noqa: F401
from . import multigrid  # noqa: F401
from .multigrid import GMGPrecon, PMGPrecon, ChainedMGPrecon, KrylovGMRES, KrylovMGSolver, MultigridHierarchy  # noqa: F401
from . import chamber  # noqa: F401
from .chamber import (RSAFDQ2022SurrogateVolume, Hirschvogel2017SurrogateVolume, ConstantChamberVolume, ChamberVolumeCoupling,  # noqa: F401
                      LumpedFluidSolidCoupler, ChamberForm, ChamberTying, compute_chamber_volume, SchurComplementLinearSolver, BlockedChamberSystem,
                      RSAFDQ2022LumpedCicuitModel, DummyLumpedCircuitModel, Φ_RSAFDQ2022, Phi_RSAFDQ2022, elastance_RSAFDQ2022, integrate_circuit,
                      prepace_circuit, RSAFDQ2022Model, RSAFDQ2022Split, RSAFDQ2022Function, semidiscretize_rsafdq, RSAFDQ2022Integrator)
# `transfer` below is the function (transfer! of the reference); its module stays importable as thunderbolt_jl_amd.transfer through sys.modules
from .transfer import PointEvalHandler, evaluate_at_points, NodalIntergridInterpolation, intergrid_dofs, transfer  # noqa: F401
from . import ecg  # noqa: F401
from .ecg import (Plonsey1964ECGGaussCache, PoissonECGReconstructionCache, Geselowitz1989ECGLeadCache, update_ecg, evaluate_ecg,  # noqa: F401
                  get_closest_vertex, cellset_coefficient, lead_right_hand_sides, vertex_dofs, scrub_scale)
from . import dynamics  # noqa: F401
from .dynamics import ElastodynamicsModel, NewmarkSolver, NewmarkStageOperator, NewmarkIntegrator, Dirichlet, LinearMaxwellMaterial  # noqa: F401
from . import multidomain  # noqa: F401
from .multidomain import (insert_interfaces, InterfaceRecords, interface_dofs, extract_subgrid, NoStimulationProtocol, MonodomainModel,  # noqa: F401
                          InterfaceDiffusionModel, ReactionDiffusionSplit, InterfaceDiffusionForm, PointwiseMultiODEFunction, MultiSolverCache,
                          MultiDomainFunction, plan_ep, semidiscretize_ep, MultiDomainHeatStage, MultiDomainLieTrotterGodunov, heat_dofrange_of, QUAD_FACETS)
from . import bidomain  # noqa: F401
from .bidomain import (ParabolicEllipticBidomainModel, BidomainBackwardEulerStage, BidomainSystem, BidomainMultigrid, BidomainAMGPrecon,  # noqa: F401
                       BidomainAlgebraicMultigrid)
from . import eikonal  # noqa: F401
from .eikonal import EikonalModel, EikonalActivationCache, solve_activation, ActionPotentialTemplate, activation_potential  # noqa: F401
