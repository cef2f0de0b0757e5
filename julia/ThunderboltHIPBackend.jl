# ThunderboltHIPBackend.jl — the reference-side binding a Thunderbolt.jl maintainer would add (as a package extension next to
# ext/CuThunderboltExt.jl) to use libtbhip.so as an `AbstractGPUDevice` backend for the assembly + reaction hot path.
#
# NOT executed in the build container (no Julia toolchain there; stated in DESIGN.md and INTEGRATION.md).  Every `ccall` targets a symbol
# declared in include/tbhip.h with the argument order of that header; tests/abi_driver.c exercises the same entry points in the same order
# from C, and thunderbolt.jl_amd/api.py is the executable mirror.
module ThunderboltHIPBackend

using Thunderbolt, Ferrite, Tensors, SparseArrays, SparseMatricesCSR, LinearAlgebra
import LinearAlgebra: mul!
import Thunderbolt: AbstractGPUDevice, AbstractAssemblyStrategy, AbstractSolver, AbstractSemidiscreteFunction, setup_operator,
    update_operator!, update_linearization!, residual!, add!, needs_update, _pointwise_step_outer_kernel!, create_system_vector,
    create_system_matrix, __add_to_vector!, adapt_vector_type, value_type, index_type, solution_size, AbstractPointwiseSolverCache,
    AbstractPointwiseFunction, num_states, BilinearMassIntegrator, BilinearDiffusionIntegrator, LinearIntegrator, ConstantCoefficient,
    FieldCoefficient, ConductivityToDiffusivityCoefficient, SpectralTensorCoefficient, OrthotropicMicrostructure,
    TransverselyIsotropicMicrostructure, OrthotropicMicrostructureModel, PerColorAssemblyStrategy, ElementAssemblyStrategy,
    QuasiStaticModel, PK1Model, HolzapfelOgden2009Model

const libtbhip = get(ENV, "TBHIP_LIBRARY", "libtbhip.so")

# revision of include/tbhip.h these ccalls were written against (TB_ABI_REVISION); a library of another revision reads / writes other buffer sizes
const TB_ABI_REVISION = 10
const TB_ERR_UNSUPPORTED = Cint(-5) # include/tbhip.h
function __init__()
    have = ccall((:tb_abi_revision, libtbhip), Cint, ())
    have == TB_ABI_REVISION || error("libtbhip ABI revision $have, this binding was written against $TB_ABI_REVISION")
end

check(rc::Cint) = rc == 0 ? nothing :
    error("libtbhip error $rc: " * unsafe_string(ccall((:tb_last_error_string, libtbhip), Cstring, ())))

# ---------------------------------------------------------------- device (replaces FerriteOperators.CudaDevice, ext/CuThunderboltExt.jl:48-49)
mutable struct MI355XDevice{Tv, Ti} <: AbstractGPUDevice
    handle::Ptr{Cvoid}
    function MI355XDevice{Tv, Ti}(id::Integer = 0) where {Tv, Ti}
        h = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:tb_device_create, libtbhip), Cint, (Cint, Ref{Ptr{Cvoid}}), id, h))
        dev = new{Tv, Ti}(h[])
        finalizer(d -> ccall((:tb_device_destroy, libtbhip), Cint, (Ptr{Cvoid},), d.handle), dev)
        return dev
    end
end
# the kernel instance the latest assembly call launched (benchmark lines)
last_kernel_name() = unsafe_string(ccall((:tb_last_kernel_name, libtbhip), Cstring, ()))
MI355XDevice(id = 0) = MI355XDevice{Float64, Int32}(id)
value_type(::MI355XDevice{Tv}) where {Tv} = Tv
index_type(::MI355XDevice{Tv, Ti}) where {Tv, Ti} = Ti
# deferred status: inside a time loop on a fixed mesh the assembly calls then only enqueue their kernels; `poll_status` synchronises and throws the first
# assembly error (detJ ≤ 0, coupling missing from the pattern) raised since the last poll
defer_status!(dev::MI355XDevice, on::Bool = true) = check(ccall((:tb_device_defer_status, libtbhip), Cint, (Ptr{Cvoid}, Cint), dev.handle, on ? 1 : 0))
poll_status(dev::MI355XDevice) = check(ccall((:tb_device_poll_status, libtbhip), Cint, (Ptr{Cvoid},), dev.handle))

# ---------------------------------------------------------------- vectors: an opaque, GC-managed device buffer (finaliser → tb_free).
# Deliberately NOT an AbstractVector: there is no scalar indexing on the device, and the solvers that consume it are the library's own
# (tb_cg_solve …), reached through the methods below — not LinearSolve's generic fallbacks.
mutable struct HIPVector{T}
    dev::MI355XDevice
    ptr::Ptr{T}
    n::Int
    function HIPVector{T}(dev::MI355XDevice, n::Integer) where {T}
        p = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:tb_malloc, libtbhip), Cint, (Ptr{Cvoid}, Csize_t, Ref{Ptr{Cvoid}}), dev.handle, n * sizeof(T), p))
        v = new{T}(dev, Ptr{T}(p[]), n)
        finalizer(x -> ccall((:tb_free, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), x.dev.handle, x.ptr), v)
        return fill!(v, zero(T))
    end
end
Base.length(v::HIPVector) = v.n
Base.eltype(::HIPVector{T}) where {T} = T
Base.similar(v::HIPVector{T}) where {T} = HIPVector{T}(v.dev, v.n)
function Base.fill!(v::HIPVector{T}, x) where {T}
    iszero(x) || error("HIPVector: only zero-fill is provided")
    check(ccall((:tb_memset, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Csize_t), v.dev.handle, v.ptr, 0, v.n * sizeof(T)))
    return v
end
function Base.copyto!(v::HIPVector{T}, a::Vector{T}) where {T}
    length(a) == v.n || throw(DimensionMismatch())
    check(ccall((:tb_memcpy_h2d, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t), v.dev.handle, v.ptr, a, sizeof(a)))
    return v
end
function Base.copyto!(v::HIPVector{T}, w::HIPVector{T}) where {T}
    check(ccall((:tb_memcpy_d2d, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t), v.dev.handle, v.ptr, w.ptr, v.n * sizeof(T)))
    return v
end
function Base.Vector(v::HIPVector{T}) where {T}
    a = Vector{T}(undef, v.n)
    check(ccall((:tb_memcpy_d2h, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t), v.dev.handle, a, v.ptr, sizeof(a)))
    return a
end
HIPVector(dev::MI355XDevice, a::Vector{T}) where {T} = copyto!(HIPVector{T}(dev, length(a)), a)

# the device a vector type lives on: one process drives one GPU (one rank per GPU under torch.distributed / MPI)
const CURRENT_DEVICE = Ref{Union{Nothing, MI355XDevice}}(nothing)
current_device() = something(CURRENT_DEVICE[], (CURRENT_DEVICE[] = MI355XDevice(); CURRENT_DEVICE[]))

# ext/CuThunderboltExt.jl:126-127
create_system_vector(::Type{<:HIPVector{T}}, f::AbstractSemidiscreteFunction) where {T} = HIPVector{T}(current_device(), solution_size(f))
create_system_vector(::Type{<:HIPVector{T}}, dh::DofHandler) where {T} = HIPVector{T}(current_device(), ndofs(dh))
# ext/CuThunderboltExt.jl:141-146
__add_to_vector!(b::Vector, a::HIPVector) = b .+= Vector(a)
function __add_to_vector!(b::HIPVector{T}, a::Vector{T}) where {T}
    tmp = HIPVector(b.dev, a)
    check(ccall((:tb_axpy, libtbhip), Cint, (Ptr{Cvoid}, Int64, Cdouble, Ptr{T}, Ptr{T}), b.dev.handle, b.n, 1.0, tmp.ptr, b.ptr))
    return b
end
adapt_vector_type(::Type{<:HIPVector}, v::Vector) = HIPVector(current_device(), v)

# ---------------------------------------------------------------- strategies (src/Thunderbolt.jl:22-32): the reference's own strategy types carry the
# device; the patch strategy is this backend's addition
struct PatchAssemblyStrategy{D <: MI355XDevice} <: AbstractAssemblyStrategy
    device::D
end
const HIPStrategy = Union{PatchAssemblyStrategy, PerColorAssemblyStrategy{<:MI355XDevice}, ElementAssemblyStrategy{<:MI355XDevice}}
strategy_code(::PerColorAssemblyStrategy) = Cint(1)      # TB_STRATEGY_PER_COLOR
strategy_code(::ElementAssemblyStrategy) = Cint(2)       # TB_STRATEGY_ELEMENT
strategy_code(::PatchAssemblyStrategy) = Cint(3)         # TB_STRATEGY_PATCH

# ---------------------------------------------------------------- mesh, dof table, pattern: Ferrite's own arrays go over as they are, once per DofHandler
# (all operators of one DofHandler share one sparsity pattern, src/solver/time/euler.jl:110-116, newmark.jl:105-110)
mutable struct DeviceDofHandler
    dev::MI355XDevice
    mesh::Ptr{Cvoid}
    pattern::Ptr{Cvoid}
    nnz::Int
    size::Tuple{Int, Int}
    cpu_pattern::SparseMatrixCSR{1, Float64, Int64}   # kept for hosts that want rowptr / colval on the CPU side
end
const DOFHANDLERS = IdDict{Any, DeviceDofHandler}()

function DeviceDofHandler(dev::MI355XDevice, dh::DofHandler)
    haskey(DOFHANDLERS, dh) && return DOFHANDLERS[dh]
    grid = Ferrite.get_grid(dh)
    sdh = only(dh.subdofhandlers)                       # one subdomain, one field (SURVEY §8b)
    sdim = Ferrite.getspatialdim(grid)
    xyz = Float64[i <= sdim ? n.x[i] : 0.0 for n in grid.nodes for i in 1:3]           # AoS, 3 per node; 2-D meshes travel with z = 0 (TB_QUAD4)
    conn = Int32[v for c in grid.cells for v in c.nodes]                                # 1-based
    celldofs = Int32.(dh.cell_dofs)                                                     # dh.cell_dofs / cell_dofs_offset, src/utils.jl:52-56
    kind = grid.cells[1] isa Quadrilateral ? Cint(2) : grid.cells[1] isa Hexahedron ? Cint(3) : Cint(4)   # TB_QUAD4 / TB_HEX8 / TB_TET4
    ip = Ferrite.getfieldinterpolation(sdh, first(sdh.field_names))
    fkind = (kind == 3 && Ferrite.getorder(ip) == 2) ? Cint(5) : (kind == 4 && Ferrite.getorder(ip) == 2) ? Cint(6) : kind   # TB_HEX27 / TB_TET10
    ncomp = Ferrite.n_components(ip)
    mesh = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:tb_mesh_create, libtbhip), Cint,
        (Ptr{Cvoid}, Cint, Int64, Ptr{Float64}, Int64, Ptr{Int32}, Cint, Cint, Ptr{Int32}, Int64, Cint, Ref{Ptr{Cvoid}}),
        dev.handle, kind, length(grid.nodes), xyz, length(grid.cells), conn, fkind, ncomp, celldofs, ndofs(dh), 1, mesh))
    A = SparseMatrixCSR(transpose(allocate_matrix(dh)))                                 # src/solver/interface.jl:162-168
    pat = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:tb_pattern_create, libtbhip), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int32}, Cint, Ref{Ptr{Cvoid}}),
        mesh[], size(A, 1), Int64.(A.rowptr), Int32.(A.colval), 1, pat))
    ddh = DeviceDofHandler(dev, mesh[], pat[], nnz(A), size(A), A)
    finalizer(ddh) do d
        ccall((:tb_pattern_destroy, libtbhip), Cint, (Ptr{Cvoid},), d.pattern)
        ccall((:tb_mesh_destroy, libtbhip), Cint, (Ptr{Cvoid},), d.mesh)
    end
    return DOFHANDLERS[dh] = ddh
end

# Locality numbering for a DofHandler on an arbitrarily numbered grid (a mesh read from a file): call BEFORE the first setup_operator /
# create_system_matrix of this DofHandler.  The reference's cell loop does not care how a mesh is numbered (src/modeling/core/coordinate_systems.jl:145-171);
# the device plans do (shared scatter signatures, SpMV gathers that stay in the caches).  tb_host_locality_permutation sweeps the per-axis cell layers the
# patch planner cuts and numbers the dofs by first visit in that order — what close!(dh) would number on a grid stored in that order.
function locality_renumber!(dh::DofHandler)
    grid = Ferrite.get_grid(dh)
    sdim = Ferrite.getspatialdim(grid)
    xyz = Float64[i <= sdim ? n.x[i] : 0.0 for n in grid.nodes for i in 1:3]
    conn = Int32[v for c in grid.cells for v in c.nodes]
    celldofs = Int32.(dh.cell_dofs)
    kind = grid.cells[1] isa Quadrilateral ? Cint(2) : grid.cells[1] isa Hexahedron ? Cint(3) : Cint(4)
    perm = Vector{Int32}(undef, ndofs(dh))
    check(ccall((:tb_host_locality_permutation, libtbhip), Cint,
        (Cint, Int64, Ptr{Float64}, Int64, Ptr{Int32}, Cint, Ptr{Int32}, Int64, Cint, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}),
        kind, length(grid.nodes), xyz, length(grid.cells), conn, Ferrite.ndofs_per_cell(dh), celldofs, ndofs(dh), 1, C_NULL, C_NULL, perm))
    Ferrite.renumber!(dh, Int.(perm))                    # perm[d] = new number of dof d (Ferrite's convention)
    return dh
end

# device CSR matrix: the shared pattern + one nzval vector (rowptr / colval stay inside the library: tb_pattern_{rowptr,colidx}_device)
struct HIPSparseMatrixCSR{Tv}
    ddh::DeviceDofHandler
    nzval::HIPVector{Tv}
end
Base.size(A::HIPSparseMatrixCSR) = A.ddh.size
SparseArrays.nnz(A::HIPSparseMatrixCSR) = A.ddh.nnz
SparseArrays.nonzeros(A::HIPSparseMatrixCSR) = A.nzval
# ext/CuThunderboltExt.jl:129-139
function create_system_matrix(::Type{<:HIPSparseMatrixCSR{Tv}}, dh::DofHandler) where {Tv}
    ddh = DeviceDofHandler(current_device(), dh)
    return HIPSparseMatrixCSR{Tv}(ddh, HIPVector{Tv}(ddh.dev, ddh.nnz))
end
# y = α·A·x + β·y (src/utils.jl:185-231)
function mul!(y::HIPVector{Tv}, A::HIPSparseMatrixCSR{Tv}, x::HIPVector{Tv}, α::Number = true, β::Number = false) where {Tv}
    check(ccall((:tb_spmv_csr, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Tv}, Ptr{Tv}, Cdouble, Cdouble, Ptr{Tv}),
        A.ddh.pattern, A.nzval.ptr, x.ptr, α, β, y.ptr))
    return y
end

# ---------------------------------------------------------------- coefficients → tb_coef (closures cannot cross the ABI, SURVEY F10)
struct TbCoef
    kind::Int32; wrap::Int32; Cm::Float64; chi::Float64
    p::NTuple{16, Float64}; field::Ptr{Float64}; field_len::Int64
end
pad16(v) = ntuple(i -> i <= length(v) ? Float64(v[i]) : 0.0, 16)
v3(x::Vec{3}) = (x[1], x[2], x[3])
v3(x::Vec{2}) = (x[1], x[2], 0.0)
# returns (TbCoef, keepalive): the field array must outlive tb_form_create, which copies it
lower(c::ConstantCoefficient{<:Real}) = (TbCoef(0, 0, 1.0, 1.0, pad16((c.val,)), C_NULL, 0), nothing)                     # TB_COEF_CONST_SCALAR
function lower(c::ConstantCoefficient{<:Tensors.SecondOrderTensor})                                                         # TB_COEF_CONST_TENSOR, row-major 3×3
    D = zeros(3, 3); d = size(c.val, 1); D[1:d, 1:d] .= Matrix(c.val)
    return (TbCoef(1, 0, 1.0, 1.0, pad16(vec(permutedims(D))), C_NULL, 0), nothing)
end
function lower(c::FieldCoefficient)                                                                                         # TB_COEF_FIELD_SCALAR, field[basis + nb·cell]
    data = Float64.(vec(c.elementwise_data.data))
    return (TbCoef(2, 0, 1.0, 1.0, pad16(()), pointer(data), length(data)), data)
end
function lower(c::SpectralTensorCoefficient)
    λ = c.eigenvalues isa ConstantCoefficient ? Tuple(c.eigenvalues.val) : error("spectral coefficient: constant eigenvalues only")
    ev = c.eigenvectors
    if ev isa ConstantCoefficient{<:OrthotropicMicrostructure}                                                              # TB_COEF_SPECTRAL_CONST: f, s, n, λ
        m = ev.val
        return (TbCoef(3, 0, 1.0, 1.0, pad16((v3(m.f)..., v3(m.s)..., v3(m.n)..., λ...)), C_NULL, 0), nothing)
    elseif ev isa ConstantCoefficient{<:TransverselyIsotropicMicrostructure}                                                # TB_COEF_TRANSVERSE_CONST: f, λ₁, λ₂
        return (TbCoef(5, 0, 1.0, 1.0, pad16((v3(ev.val.f)..., λ[1], λ[2])), C_NULL, 0), nothing)
    elseif ev isa OrthotropicMicrostructureModel                                                                            # TB_COEF_SPECTRAL_FIELD: per cell, per basis f, s, n
        f, s, n = ev.fiber_coefficient.elementwise_data.data, ev.sheetlet_coefficient.elementwise_data.data, ev.normal_coefficient.elementwise_data.data
        data = Float64[x for k in eachindex(f) for vec3 in (f[k], s[k], n[k]) for x in v3(vec3)]                            # cell-major (ElementwiseData, collections.jl:195-233)
        return (TbCoef(4, 0, 1.0, 1.0, pad16(λ), pointer(data), length(data)), data)
    end
    error("spectral coefficient over $(typeof(ev)) is not lowered")
end
function lower(c::ConductivityToDiffusivityCoefficient)                                                                     # κ/(Cₘχ), coefficients.jl:152-162
    k, keep = lower(c.conductivity_tensor_coefficient)
    return (TbCoef(k.kind, 1, c.capacitance_coefficient.val, c.χ_coefficient.val, k.p, k.field, k.field_len), keep)
end

# ---------------------------------------------------------------- operators (src/solver/interface.jl:17-94, euler.jl:143-176)
mutable struct HIPBilinearOperator{Tv}
    form::Ptr{Cvoid}
    strategy::Cint
    A::HIPSparseMatrixCSR{Tv}            # op.A (euler.jl:112-114)
    is_mass::Bool
end
function setup_operator(strategy::HIPStrategy, integrator::Union{BilinearMassIntegrator, BilinearDiffusionIntegrator}, dh::DofHandler)
    ddh = DeviceDofHandler(strategy.device, dh)
    coef, keep = lower(integrator isa BilinearMassIntegrator ? integrator.ρ : integrator.D)
    form = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve keep check(ccall((:tb_form_create, libtbhip), Cint, (Ptr{Cvoid}, Cint, Cint, Ref{TbCoef}, Ref{Ptr{Cvoid}}),
        ddh.mesh, integrator isa BilinearMassIntegrator ? 0 : 1, 0, Ref(coef), form))
    Tv = value_type(strategy.device)
    op = HIPBilinearOperator{Tv}(form[], strategy_code(strategy), HIPSparseMatrixCSR{Tv}(ddh, HIPVector{Tv}(ddh.dev, ddh.nnz)), integrator isa BilinearMassIntegrator)
    finalizer(o -> ccall((:tb_form_destroy, libtbhip), Cint, (Ptr{Cvoid},), o.form), op)
    return op
end
# the 4-argument form the solvers call (interface.jl:66-94): the solver's system_matrix_type is this backend's CSR type already
setup_operator(strategy::HIPStrategy, integrator::Union{BilinearMassIntegrator, BilinearDiffusionIntegrator}, ::AbstractSolver, dh::DofHandler) =
    setup_operator(strategy, integrator, dh)

update_operator!(op::HIPBilinearOperator, t) =
    check(ccall((:tb_assemble_matrix, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Float64, Ptr{Float64}),
        op.form, op.A.ddh.pattern, op.strategy, t, op.A.nzval.ptr))
# update_operator!(mass, t); update_operator!(diffusion, t) of the heat stage's set-up (euler.jl:172-176) in one pass over the mesh
function update_operators!(M::HIPBilinearOperator, K::HIPBilinearOperator, t)
    (M.is_mass && !K.is_mass && M.A.ddh === K.A.ddh) || (update_operator!(M, t); update_operator!(K, t); return nothing)
    check(ccall((:tb_assemble_matrix_pair, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Float64, Ptr{Float64}, Ptr{Float64}),
        M.form, K.form, M.A.ddh.pattern, M.strategy, t, M.A.nzval.ptr, K.A.nzval.ptr))
end
mul!(y::HIPVector, op::HIPBilinearOperator, x::HIPVector, α::Number = true, β::Number = false) = mul!(y, op.A, x, α, β)   # mul!(b, M, uₙ₋₁), euler.jl:85

# linear operators: the source closure f(x, t) is evaluated on the host at every quadrature point and uploaded (TB_SRC_TABULATED)
mutable struct HIPLinearOperator{Tv, F, IV}
    form::Ptr{Cvoid}
    strategy::Cint
    b::HIPVector{Tv}                     # op.b (test/gpu/test_operators.jl:30)
    f::F                                 # (x, t) -> value
    nonzero_intervals::IV
    xq::Vector{Vec{3, Float64}}          # quadrature-point coordinates, [q + nq·(cell − 1)]
end
function setup_operator(strategy::HIPStrategy, integrator::LinearIntegrator, dh::DofHandler)
    ddh = DeviceDofHandler(strategy.device, dh)
    protocol = integrator.integrand                      # AnalyticalTransmembraneStimulationProtocol(f, nonzero_intervals), electrophysiology.jl:260-283
    sdh = only(dh.subdofhandlers)
    ip = Ferrite.getfieldinterpolation(sdh, first(sdh.field_names))
    qr = QuadratureRule{Ferrite.getrefshape(ip)}(max(2 * Ferrite.getorder(ip) - 1, 2))                 # fem.jl:52-55
    gip = Ferrite.geometric_interpolation(typeof(Ferrite.get_grid(dh).cells[1]))
    xq = Vec{3, Float64}[]
    for cell in CellIterator(sdh)
        X = getcoordinates(cell)
        for ξ in Ferrite.getpoints(qr)
            x = sum(Ferrite.reference_shape_value(gip, ξ, a) * X[a] for a in 1:length(X))
            push!(xq, Vec{3, Float64}(i -> i <= length(x) ? x[i] : 0.0))
        end
    end
    coef = TbCoef(3, 0, 1.0, 1.0, pad16(()), C_NULL, 0)                                                # TB_SRC_TABULATED
    form = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:tb_form_create, libtbhip), Cint, (Ptr{Cvoid}, Cint, Cint, Ref{TbCoef}, Ref{Ptr{Cvoid}}), ddh.mesh, 2, 0, Ref(coef), form))
    Tv = value_type(strategy.device)
    op = HIPLinearOperator(form[], strategy_code(strategy), HIPVector{Tv}(ddh.dev, ndofs(dh)), protocol.f.f, protocol.nonzero_intervals, xq)
    finalizer(o -> ccall((:tb_form_destroy, libtbhip), Cint, (Ptr{Cvoid},), o.form), op)
    return op
end
setup_operator(strategy::HIPStrategy, integrator::LinearIntegrator, ::AbstractSolver, dh::DofHandler) = setup_operator(strategy, integrator, dh)
needs_update(op::HIPLinearOperator, t) = any(iv -> iv[1] <= t <= iv[2], op.nonzero_intervals)          # src/discretization/operator.jl:17-26
function update_operator!(op::HIPLinearOperator, t)
    table = Float64[op.f(x, t) for x in op.xq]
    check(ccall((:tb_form_set_table, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64), op.form, table, length(table)))
    check(ccall((:tb_assemble_vector, libtbhip), Cint, (Ptr{Cvoid}, Cint, Float64, Ptr{Float64}), op.form, op.strategy, t, op.b.ptr))
end
function add!(b::HIPVector{Tv}, op::HIPLinearOperator{Tv}) where {Tv}                                   # add!(b, source), euler.jl:90
    check(ccall((:tb_axpy, libtbhip), Cint, (Ptr{Cvoid}, Int64, Cdouble, Ptr{Tv}, Ptr{Tv}), b.dev.handle, b.n, 1.0, op.b.ptr, b.ptr))
    return b
end

# ---------------------------------------------------------------- heat stage algebra and solve (euler.jl:71-116)
# _implicit_euler_heat_solver_update_system_matrix!: Anz = Mnz − Δt·Knz
function Thunderbolt._implicit_euler_heat_solver_update_system_matrix!(A::HIPSparseMatrixCSR, M::HIPBilinearOperator, K::HIPBilinearOperator, Δt)
    check(ccall((:tb_heat_matrix, libtbhip), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Float64}),
        A.ddh.dev.handle, A.ddh.nnz, M.A.nzval.ptr, K.A.nzval.ptr, Δt, A.nzval.ptr))
end
# the linear solve of the stage for device matrices: Jacobi-CG inside the library (KrylovJL_CG(atol, rtol) in the tutorials); converged iff the
# residual met the solver's own stopping threshold
function solve_heat_system!(u::HIPVector, A::HIPSparseMatrixCSR, b::HIPVector; rtol = 1e-5, atol = 1e-6, maxiter = 1000, reuse_diagonal = false)
    iters = Ref{Cint}(0); res = Ref{Cdouble}(0.0); tol = Ref{Cdouble}(0.0)
    check(ccall((:tb_cg_solve, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble, Cint, Cint, Ref{Cint}, Ref{Cdouble}),
        A.ddh.pattern, A.nzval.ptr, b.ptr, u.ptr, rtol, atol, maxiter, reuse_diagonal ? 2 : 1, iters, res))
    check(ccall((:tb_solver_last_tolerance, libtbhip), Cint, (Ptr{Cvoid}, Ref{Cdouble}), A.ddh.pattern, tol))
    return res[] <= tol[], Int(iters[])
end

# ---------------------------------------------------------------- pointwise reaction step, dispatched on the vector type
# (src/solver/time/partitioned_solver.jl:38-44, ext/CuThunderboltExt.jl:111-117)
model_id(::Thunderbolt.ParametrizedFHNModel) = Cint(0)
model_id(::Thunderbolt.ParametrizedAlievPanfilovModel) = Cint(1)
model_id(::Thunderbolt.ParametrizedPCG2019Model) = Cint(2)
params(m) = Float64[getfield(m, f) for f in fieldnames(typeof(m))]      # struct field order == ABI parameter order

function _pointwise_step_outer_kernel!(f::AbstractPointwiseFunction, t::Real, Δt::Real, cache::AbstractPointwiseSolverCache, u::HIPVector)
    p = params(f.ode)
    substeps = hasproperty(cache, :substeps) ? cache.substeps : 1
    threshold = hasproperty(cache, :reaction_threshold) ? cache.reaction_threshold : 0.0
    du = cache.du === nothing ? Ptr{Float64}(C_NULL) : cache.du.ptr
    xs = cache.xs                                                        # Vector{Vec{sdim, Float32}} uploaded as an HIPVector{Float32}, or nothing
    if xs === nothing
        rc = ccall((:tb_reaction_step, libtbhip), Cint,
            (Ptr{Cvoid}, Cint, Ptr{Float64}, Cint, Ptr{Float64}, Ptr{Float64}, Int64, Cint, Cint, Float64, Float64, Cint, Float64),
            u.dev.handle, model_id(f.ode), p, length(p), cache.uₙ.ptr, du, f.npoints, num_states(f.ode),
            0 #= StateBlockedLayout, fem.jl:385-408 =#, t, Δt, substeps, threshold)
    else
        rc = ccall((:tb_reaction_step_x, libtbhip), Cint,
            (Ptr{Cvoid}, Cint, Ptr{Float64}, Cint, Ptr{Float64}, Ptr{Float64}, Int64, Cint, Cint, Ptr{Float32}, Cint, Float64, Float64, Cint, Float64),
            u.dev.handle, model_id(f.ode), p, length(p), cache.uₙ.ptr, du, f.npoints, num_states(f.ode), 0, xs.ptr, xs.n ÷ f.npoints, t, Δt, substeps, threshold)
    end
    return rc == 0
end

# reaction tangent of the RTC controller: `maximum(@view cache.dumat[:, φₘidx])` (src/solver/time/rtc.jl:64-73) on the device, NaN included:
# any NaN in the slice makes the result NaN, as `maximum` does
function reaction_tangent(dev::MI355XDevice, dumat_phi::Ptr{Float64}, npoints::Integer, stride::Integer = 1)
    R = Ref{Float64}()
    check(ccall((:tb_max, libtbhip), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Ref{Float64}), dev.handle, npoints, dumat_phi, stride, R))
    return R[]
end

# ---------------------------------------------------------------- quasi-static mechanics (src/solver/nonlinear/newton_raphson.jl:234-238)
struct TbMaterial
    kind::Int32; penalty::Int32; p::NTuple{16, Float64}
    f::NTuple{3, Float64}; s::NTuple{3, Float64}; n::NTuple{3, Float64}
    fsn_field::Ptr{Float64}; fsn_field_len::Int64
end
energy_id(::HolzapfelOgden2009Model) = Int32(0); energy_id(::Thunderbolt.NullEnergyModel) = Int32(1)
energy_id(::Thunderbolt.BioNeoHookean) = Int32(2); energy_id(::Thunderbolt.TransverseIsotopicNeoHookeanModel) = Int32(3)
energy_id(::Thunderbolt.LinYinPassiveModel) = Int32(4); energy_id(::Thunderbolt.LinYinActiveModel) = Int32(5)
energy_id(::Thunderbolt.HumphreyStrumpfYinModel) = Int32(6); energy_id(::Thunderbolt.LinearSpringModel) = Int32(7)
energy_id(::Thunderbolt.Guccione1991PassiveModel) = Int32(8)
penalty_id(::Thunderbolt.SimpleCompressionPenalty) = Int32(0); penalty_id(::Thunderbolt.NullCompressionPenalty) = Int32(1)
penalty_id(::Thunderbolt.HartmannNeffCompressionPenalty1) = Int32(2); penalty_id(::Thunderbolt.HartmannNeffCompressionPenalty2) = Int32(3)
penalty_id(::Thunderbolt.HartmannNeffCompressionPenalty3) = Int32(4)
# energy parameters = the Float fields of the energy struct in field order (p[1:9]); penalty parameters (β, a, b) in p[11:13]
function lower(m::PK1Model)
    ψ = m.material
    ep = Float64[getfield(ψ, f) for f in fieldnames(typeof(ψ)) if getfield(ψ, f) isa Real]
    pen = hasproperty(ψ, :mpU) ? ψ.mpU : Thunderbolt.NullCompressionPenalty()
    pp = Float64[getfield(pen, f) for f in fieldnames(typeof(pen)) if getfield(pen, f) isa Real]
    p = zeros(16); p[1:length(ep)] .= ep; p[11:10 + length(pp)] .= pp
    energy_id(ψ) == 0 && penalty_id(pen) == 0 && (p[9] = isempty(pp) ? 1.0 : pp[1])       # HO2009 + SimpleCompressionPenalty: β also in p[9] (fast path)
    ms = m.coefficient isa ConstantCoefficient ? m.coefficient.val : error("mechanics: constant microstructure frames only in this binding")
    return TbMaterial(energy_id(ψ), penalty_id(pen), Tuple(p), v3(ms.f), v3(ms.s), v3(ms.n), C_NULL, 0)
end

mutable struct HIPNonlinearOperator{Tv}
    form::Ptr{Cvoid}
    strategy::Cint
    J::HIPSparseMatrixCSR{Tv}            # op.J (src/solver/interface.jl:9)
end
function setup_operator(strategy::HIPStrategy, model::QuasiStaticModel, ::AbstractSolver, dh::DofHandler)
    ddh = DeviceDofHandler(strategy.device, dh)
    form = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:tb_hyperelastic_create, libtbhip), Cint, (Ptr{Cvoid}, Cint, Ref{TbMaterial}, Ref{Ptr{Cvoid}}), ddh.mesh, 0, Ref(lower(model.material_model)), form))
    Tv = value_type(strategy.device)
    op = HIPNonlinearOperator{Tv}(form[], strategy_code(strategy), HIPSparseMatrixCSR{Tv}(ddh, HIPVector{Tv}(ddh.dev, ddh.nnz)))
    finalizer(o -> ccall((:tb_form_destroy, libtbhip), Cint, (Ptr{Cvoid},), o.form), op)
    return op
end
gettime(p::Real) = p
gettime(p) = p.t                                                         # GenericFirstOrderTimeParameters(p, t, Δt, uprev), euler.jl:490-493
function update_linearization!(op::HIPNonlinearOperator, residual::HIPVector, u::HIPVector, p)
    check(ccall((:tb_linearize, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Float64}, Float64, Ptr{Float64}, Ptr{Float64}),
        op.form, op.J.ddh.pattern, op.strategy, u.ptr, gettime(p), op.J.nzval.ptr, residual.ptr))
end
function update_linearization!(op::HIPNonlinearOperator, u::HIPVector, p)
    check(ccall((:tb_linearize, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Float64}, Float64, Ptr{Float64}, Ptr{Float64}),
        op.form, op.J.ddh.pattern, op.strategy, u.ptr, gettime(p), op.J.nzval.ptr, C_NULL))
end
function residual!(op::HIPNonlinearOperator, residual::HIPVector, u::HIPVector, p)
    check(ccall((:tb_residual, libtbhip), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Float64, Ptr{Float64}), op.form, op.strategy, u.ptr, gettime(p), residual.ptr))
end
# apply_zero!(J, r, ch) on the device CSR matrix (src/solver/nonlinear/nlsolve_common.jl:12-26, src/utils.jl:263-278): flags = one byte per dof
function Ferrite.apply_zero!(J::HIPSparseMatrixCSR, r::HIPVector, prescribed_flags::HIPVector{UInt8}, diag::Real)
    check(ccall((:tb_apply_zero_csr, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}, Cdouble), J.ddh.pattern, J.nzval.ptr, r.ptr, prescribed_flags.ptr, diag))
end
function LinearAlgebra.dot(a::HIPVector{Float64}, b::HIPVector{Float64})
    r = Ref{Cdouble}(0.0)
    check(ccall((:tb_dot, libtbhip), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ref{Cdouble}), a.dev.handle, a.n, a.ptr, b.ptr, r))
    return r[]
end
LinearAlgebra.norm(a::HIPVector{Float64}) = sqrt(dot(a, a))

# ---- Float32 value type: MI355XDevice{Float32,Int32} (ext/CuThunderboltExt.jl:126-127 types everything by value_type(device); the reference's GPU
# tests run Float32).  Storage is Float32, the kernels compute in Float64 and round once (include/tbhip.h, "Float32 value type").
function update_operator!(op::HIPBilinearOperator{Float32}, t)
    check(ccall((:tb_assemble_matrix_f32, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Float64, Ptr{Float32}),
        op.form, op.A.ddh.pattern, op.strategy, Float64(t), op.A.nzval.ptr))
end
function update_operators!(mass::HIPBilinearOperator{Float32}, diffusion::HIPBilinearOperator{Float32}, t)
    check(ccall((:tb_assemble_matrix_pair_f32, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Float64, Ptr{Float32}, Ptr{Float32}),
        mass.form, diffusion.form, mass.A.ddh.pattern, mass.strategy, Float64(t), mass.A.nzval.ptr, diffusion.A.nzval.ptr))
end
function update_operator!(op::HIPLinearOperator{Float32}, t)
    check(ccall((:tb_assemble_vector_f32, libtbhip), Cint, (Ptr{Cvoid}, Cint, Float64, Ptr{Float32}), op.form, op.strategy, Float64(t), op.b.ptr))
end
function LinearAlgebra.mul!(y::HIPVector{Float32}, A::HIPSparseMatrixCSR{Float32}, x::HIPVector{Float32}, α::Number, β::Number)
    check(ccall((:tb_spmv_csr_f32, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Cdouble, Cdouble, Ptr{Float32}),
        A.ddh.pattern, A.nzval.ptr, x.ptr, Float64(α), Float64(β), y.ptr))
    return y
end
function heat_system_matrix!(A::HIPSparseMatrixCSR{Float32}, M::HIPSparseMatrixCSR{Float32}, K::HIPSparseMatrixCSR{Float32}, Δt)
    check(ccall((:tb_heat_matrix_f32, libtbhip), Cint, (Ptr{Cvoid}, Int64, Ptr{Float32}, Ptr{Float32}, Cdouble, Ptr{Float32}),
        A.nzval.dev.handle, A.nzval.n, M.nzval.ptr, K.nzval.ptr, Float64(Δt), A.nzval.ptr))
end
function add!(b::HIPVector{Float32}, x::HIPVector{Float32})
    check(ccall((:tb_axpy_f32, libtbhip), Cint, (Ptr{Cvoid}, Int64, Cdouble, Ptr{Float32}, Ptr{Float32}), b.dev.handle, b.n, 1.0, x.ptr, b.ptr))
end
function cg!(x::HIPVector{Float32}, A::HIPSparseMatrixCSR{Float32}, b::HIPVector{Float32}; rtol = 1e-5, atol = 1e-6, maxiter = 1000)
    its = Ref{Cint}(0); res = Ref{Cdouble}(0.0)
    check(ccall((:tb_cg_solve_f32, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Cdouble, Cdouble, Cint, Cint, Ref{Cint}, Ref{Cdouble}),
        A.ddh.pattern, A.nzval.ptr, b.ptr, x.ptr, rtol, atol, maxiter, 1, its, res))
    return its[], res[]
end
# _pointwise_step_outer_kernel! for Float32 solution vectors (partitioned_solver.jl:38-44 dispatches on the vector type)
function pointwise_step_f32!(dev, model_id, p::Vector{Float64}, u::HIPVector{Float32}, du, npoints, nstates, xs, sdim, t, Δt, substeps, threshold)
    check(ccall((:tb_reaction_step_f32, libtbhip), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Float64}, Cint, Ptr{Float32}, Ptr{Float32}, Int64, Cint, Cint, Ptr{Float32}, Cint, Float64, Float64, Cint, Float64),
        dev.handle, model_id, p, length(p), u.ptr, du === nothing ? C_NULL : du.ptr, npoints, nstates, 0, xs === nothing ? C_NULL : xs.ptr, sdim,
        Float64(t), Float64(Δt), substeps, Float64(threshold)))
    return true
end
Base.convert(::Type{HIPVector{Float32}}, v::HIPVector{Float64}) = (w = HIPVector{Float32}(v.dev, v.n);
    check(ccall((:tb_convert_f64_to_f32, libtbhip), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float32}), v.dev.handle, v.n, v.ptr, w.ptr)); w)
Base.convert(::Type{HIPVector{Float64}}, v::HIPVector{Float32}) = (w = HIPVector{Float64}(v.dev, v.n);
    check(ccall((:tb_convert_f32_to_f64, libtbhip), Cint, (Ptr{Cvoid}, Int64, Ptr{Float32}, Ptr{Float64}), v.dev.handle, v.n, v.ptr, w.ptr)); w)

# ---- multi-device path (new work: the reference is shared-memory only, README.md:7).  One Julia process per GPU (MPI.jl); a sub-domain vector holds
# the dofs shared with a neighbouring rank at the positions `idx` (0-based Int32 on the device, both sides in the same order).  The exchange is
# pack → MPI.Isend / MPI.Irecv! on the device buffers (GPU-aware MPI) → unpack; mirrored and tested in thunderbolt.jl_amd/distributed.py (HaloExchange).
struct HaloNeighbour
    peer::Int
    idx::HIPVector{Int32}
    send::HIPVector{Float64}
    recv::HIPVector{Float64}
end
function halo_pack!(nb::HaloNeighbour, v::HIPVector{Float64})
    check(ccall((:tb_gather_indexed, libtbhip), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}), v.dev.handle, nb.idx.n, v.ptr, nb.idx.ptr, nb.send.ptr))
end
function halo_unpack_add!(v::HIPVector{Float64}, nb::HaloNeighbour)
    check(ccall((:tb_scatter_add_indexed, libtbhip), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}), v.dev.handle, nb.idx.n, nb.recv.ptr, nb.idx.ptr, v.ptr))
end
# v[idx] = the rows this rank sent (same kernel as the peer's rows): called before halo_unpack_add! in the overlapped product, so that both sides of an
# interface add the same two numbers
function halo_unpack_own!(v::HIPVector{Float64}, nb::HaloNeighbour)
    check(ccall((:tb_scatter_indexed, libtbhip), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}), v.dev.handle, nb.idx.n, nb.send.ptr, nb.idx.ptr, v.ptr))
end
# interface rows of A·x straight into the send buffer (posted before the whole product is formed, so the transfer overlaps it)
function halo_pack_product_rows!(nb::HaloNeighbour, A::HIPSparseMatrixCSR{Float64}, x::HIPVector{Float64})
    check(ccall((:tb_spmv_csr_rows, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Int32}, Ptr{Float64}),
        A.ddh.pattern, A.nzval.ptr, x.ptr, nb.idx.n, nb.idx.ptr, nb.send.ptr))
end
# work statistics of the patch plan: (patches, cell instances, cells, max instances per patch, max rows per patch, LDS bytes per accumulator block)
function patch_stats(A::HIPSparseMatrixCSR)
    out = zeros(Int64, 6)
    check(ccall((:tb_pattern_patch_stats, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Int64}), A.ddh.pattern, out))
    return out
end
# Sliced mirror of A's values for repeated products (a Krylov solve on a fixed matrix): mul!, mul_dot! and cg! on A then stream the mirrored copy.
# Call again after A's values changed (update_operator!, a new M − Δt·K); unmirror! goes back to the CSR array.  false where the pattern has no mirror.
function mirror!(A::HIPSparseMatrixCSR{Float64})
    rc = ccall((:tb_spmv_mirror, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}), A.ddh.pattern, A.nzval.ptr)
    rc == TB_ERR_UNSUPPORTED && return false
    check(rc)
    return true
end
unmirror!(A::HIPSparseMatrixCSR{Float64}) = check(ccall((:tb_spmv_mirror, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}), A.ddh.pattern, C_NULL))
function diagonal!(d::HIPVector{Float64}, A::HIPSparseMatrixCSR{Float64})
    check(ccall((:tb_extract_diagonal, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), A.ddh.pattern, A.nzval.ptr, d.ptr))
end
# y = A·x and xy[] += xᵀ·y (device scalar): the local quadratic form of the distributed CG
function mul_dot!(y::HIPVector{Float64}, A::HIPSparseMatrixCSR{Float64}, x::HIPVector{Float64}, xy::HIPVector{Float64})
    check(ccall((:tb_spmv_csr_dot, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), A.ddh.pattern, A.nzval.ptr, x.ptr, y.ptr, xy.ptr))
end
# the vector work of one CG iteration with device-resident scalars S = (rz, pAp, rz_new, rr, flag, rr of the last finished iteration) — six doubles; the
# caller all-reduces S[2] and S[3:4] in between and ends the iteration with cgd_rotate! (rz ← rz_new, rr → S[6], accumulators zeroed)
function cgd_dot!(S::HIPVector{Float64}, slot::Int, w::HIPVector{Float64}, a::HIPVector{Float64}, b::HIPVector{Float64})
    check(ccall((:tb_cgd_dot, libtbhip), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), a.dev.handle, a.n, w.ptr, a.ptr, b.ptr, S.ptr + 8 * slot))
end
function cgd_update!(S::HIPVector{Float64}, w::HIPVector{Float64}, dinv::HIPVector{Float64}, p::HIPVector{Float64}, Ap::HIPVector{Float64}, x::HIPVector{Float64}, r::HIPVector{Float64})
    check(ccall((:tb_cgd_update, libtbhip), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        x.dev.handle, x.n, w.ptr, dinv.ptr, p.ptr, Ap.ptr, x.ptr, r.ptr, S.ptr, S.ptr + 8, S.ptr + 16))
end
function cgd_direction!(S::HIPVector{Float64}, dinv::HIPVector{Float64}, r::HIPVector{Float64}, p::HIPVector{Float64})
    check(ccall((:tb_cgd_direction, libtbhip), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), r.dev.handle, r.n, dinv.ptr, r.ptr, p.ptr, S.ptr, S.ptr + 16))
end
# ---------------------------------------------------------------- RCCL behind the ABI: the exchange of the multi-GPU path without GPU-aware MPI on the Julia side.
# Rank 0: id = comm_unique_id(); carry the 128 bytes to the other ranks (MPI.Bcast!, Distributed, a file); every rank: HIPComm(dev, id, rank, nranks).
mutable struct HIPComm
    handle::Ptr{Cvoid}
    dev::MI355XDevice
    function HIPComm(dev::MI355XDevice, id::Vector{UInt8}, rank::Integer, nranks::Integer)
        length(id) == 128 || error("communicator id must be 128 bytes")
        h = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:tb_comm_create, libtbhip), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Cint, Cint, Ref{Ptr{Cvoid}}), dev.handle, id, rank, nranks, h))
        c = new(h[], dev)
        finalizer(x -> ccall((:tb_comm_destroy, libtbhip), Cint, (Ptr{Cvoid},), x.handle), c)
        return c
    end
end
function comm_unique_id()
    id = zeros(UInt8, 128)
    check(ccall((:tb_comm_unique_id, libtbhip), Cint, (Ptr{UInt8},), id))
    return id
end
# sum of interface partials: pack (halo_pack! / halo_pack_product_rows!) → this → halo_unpack_add!
function halo_exchange!(c::HIPComm, nbs::Vector{HaloNeighbour})
    peers = Int32[nb.peer for nb in nbs]; counts = Int64[nb.idx.n for nb in nbs]
    send = Ptr{Float64}[nb.send.ptr for nb in nbs]; recv = Ptr{Float64}[nb.recv.ptr for nb in nbs]
    check(ccall((:tb_comm_exchange, libtbhip), Cint, (Ptr{Cvoid}, Cint, Ptr{Int32}, Ptr{Int64}, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}), c.handle, length(nbs), peers, counts, send, recv))
end
# the same exchange on the communicator's own queue: what is launched between begin and end (the whole-domain product) runs beside the transfer
function halo_exchange_begin!(c::HIPComm, nbs::Vector{HaloNeighbour})
    peers = Int32[nb.peer for nb in nbs]; counts = Int64[nb.idx.n for nb in nbs]
    send = Ptr{Float64}[nb.send.ptr for nb in nbs]; recv = Ptr{Float64}[nb.recv.ptr for nb in nbs]
    check(ccall((:tb_comm_exchange_begin, libtbhip), Cint, (Ptr{Cvoid}, Cint, Ptr{Int32}, Ptr{Int64}, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}), c.handle, length(nbs), peers, counts, send, recv))
end
halo_exchange_end!(c::HIPComm) = check(ccall((:tb_comm_exchange_end, libtbhip), Cint, (Ptr{Cvoid},), c.handle))
allreduce_sum!(c::HIPComm, S::HIPVector{Float64}, first::Int, n::Int) =
    check(ccall((:tb_comm_allreduce, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Cint), c.handle, S.ptr + 8 * first, n, 0))

# ---------------------------------------------------------------- HIP graphs: a fixed sequence of enqueue-only calls captured once, replayed with one launch
# g = capture_graph(dev) do … the calls of one time step / one CG iteration … end;  launch!(g, t)
mutable struct HIPGraph
    handle::Ptr{Cvoid}
    dev::MI355XDevice
end
function capture_graph(f::Function, dev::MI355XDevice)
    check(ccall((:tb_graph_begin, libtbhip), Cint, (Ptr{Cvoid},), dev.handle))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    try
        f()
    finally
        rc = ccall((:tb_graph_end, libtbhip), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}), dev.handle, h)
        check(rc)
    end
    g = HIPGraph(h[], dev)
    finalizer(x -> ccall((:tb_graph_destroy, libtbhip), Cint, (Ptr{Cvoid},), x.handle), g)
    return g
end
launch!(g::HIPGraph, t::Real = 0.0) = check(ccall((:tb_graph_launch, libtbhip), Cint, (Ptr{Cvoid}, Cdouble), g.handle, t))
function node_count(g::HIPGraph)
    n = Ref{Cint}(0)
    check(ccall((:tb_graph_node_count, libtbhip), Cint, (Ptr{Cvoid}, Ref{Cint}), g.handle, n))
    return Int(n[])
end

# one whole iteration of the local CG (a rank without shared dofs): product + pᵀAp, update, direction, rotate in one call
function cgd_iteration!(A::HIPSparseMatrixCSR, dinv::HIPVector{Float64}, x::HIPVector{Float64}, r::HIPVector{Float64}, p::HIPVector{Float64}, Ap::HIPVector{Float64}, S::HIPVector{Float64})
    check(ccall((:tb_cgd_iteration, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        A.ddh.pattern, A.nzval.ptr, dinv.ptr, x.ptr, r.ptr, p.ptr, Ap.ptr, S.ptr))
end
function cgd_rotate!(S::HIPVector{Float64})
    check(ccall((:tb_cgd_rotate, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}), S.dev.handle, S.ptr))
end

# single-reduction (Chronopoulos–Gear) form: S = (γ, δ, ρ, flag, γ_prev, α_prev, δ accumulator) — seven doubles, include/tbhip.h.  Per iteration:
# cg1_update! → w = A·u assembled, with mul_dot!(w, A, u, S) at offset 6 (the δ accumulator) → cg1_fold! → ONE allreduce_sum!(c, S, 0, 3); the host
# reads S[3:4] (ρ = ‖r‖², flag) once per look.  cg1_iteration!: the same three launches from one call for a rank without shared dofs.
function cg1_update!(S::HIPVector{Float64}, wt::HIPVector{Float64}, dinv::HIPVector{Float64}, w::HIPVector{Float64}, p::HIPVector{Float64}, s::HIPVector{Float64},
                     x::HIPVector{Float64}, r::HIPVector{Float64}, u::HIPVector{Float64})
    check(ccall((:tb_cg1_update, libtbhip), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        x.dev.handle, x.n, wt.ptr, dinv.ptr, w.ptr, p.ptr, s.ptr, x.ptr, r.ptr, u.ptr, S.ptr))
end
cg1_fold!(S::HIPVector{Float64}) = check(ccall((:tb_cg1_fold, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}), S.dev.handle, S.ptr))
function cg1_iteration!(A::HIPSparseMatrixCSR, dinv::HIPVector{Float64}, x::HIPVector{Float64}, r::HIPVector{Float64}, u::HIPVector{Float64}, p::HIPVector{Float64},
                        s::HIPVector{Float64}, w::HIPVector{Float64}, S::HIPVector{Float64})
    check(ccall((:tb_cg1_iteration, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        A.ddh.pattern, A.nzval.ptr, dinv.ptr, x.ptr, r.ptr, u.ptr, p.ptr, s.ptr, w.ptr, S.ptr))
end

# ---------------------------------------------------------------- round 6: the rest of the boundary the hot path's rows of SURVEY §8 use, bound the same way
# (device queue and events; pattern accessors; Rush–Larsen and RTC reaction steps; the other Krylov entries; cell sets and accumulation of a form; facet
# forms; sarcomere steps and the condensed-mechanics setters).  The host generators (tb_host_generate_grid_*, tb_host_close_dofs, tb_host_build_pattern,
# tb_host_perturb_nodes) and the host-side evaluators (tb_host_material_eval*, tb_host_sarcomere_*; tb_host_maxwell_eval and tb_host_eikonal_local_solve are bound) stay unbound: Ferrite and the reference's own Julia
# routines are the host side of those.
libtbhip_version() = unsafe_string(ccall((:tb_version, libtbhip), Cstring, ()))
# the library's kernels on a queue the host framework owns (its own stream, or the legacy default stream) — ordering with the host's device work then needs no events
set_stream!(dev::MI355XDevice, hip_stream::Ptr{Cvoid}) = check(ccall((:tb_device_set_stream, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), dev.handle, hip_stream))
use_null_stream!(dev::MI355XDevice) = check(ccall((:tb_device_use_null_stream, libtbhip), Cint, (Ptr{Cvoid},), dev.handle))
synchronize(dev::MI355XDevice) = check(ccall((:tb_device_synchronize, libtbhip), Cint, (Ptr{Cvoid},), dev.handle))
function device_info(dev::MI355XDevice)
    name = Vector{UInt8}(undef, 64); ncu = Ref{Cint}(0); mem = Ref{Csize_t}(0)
    check(ccall((:tb_device_info, libtbhip), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Csize_t, Ref{Cint}, Ref{Csize_t}), dev.handle, name, length(name), ncu, mem))
    return (name = unsafe_string(pointer(name)), n_cu = Int(ncu[]), hbm_bytes = Int(mem[]))
end
mutable struct HIPEvent
    handle::Ptr{Cvoid}
    function HIPEvent(dev::MI355XDevice)
        h = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:tb_event_create, libtbhip), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}), dev.handle, h))
        e = new(h[])
        finalizer(x -> ccall((:tb_event_destroy, libtbhip), Cint, (Ptr{Cvoid},), x.handle), e)
        return e
    end
end
record!(dev::MI355XDevice, e::HIPEvent) = check(ccall((:tb_event_record, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), dev.handle, e.handle))
function elapsed_ms(a::HIPEvent, b::HIPEvent)
    ms = Ref{Cfloat}(0)
    check(ccall((:tb_event_elapsed_ms, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{Cfloat}), a.handle, b.handle, ms))
    return Float64(ms[])
end
mesh_ncells(ddh::DeviceDofHandler) = Int(ccall((:tb_mesh_ncells, libtbhip), Int64, (Ptr{Cvoid},), ddh.mesh))
mesh_ndofs(ddh::DeviceDofHandler) = Int(ccall((:tb_mesh_ndofs, libtbhip), Int64, (Ptr{Cvoid},), ddh.mesh))
pattern_nnz(ddh::DeviceDofHandler) = Int(ccall((:tb_pattern_nnz, libtbhip), Int64, (Ptr{Cvoid},), ddh.pattern))
rowptr_device(ddh::DeviceDofHandler) = ccall((:tb_pattern_rowptr_device, libtbhip), Ptr{Int64}, (Ptr{Cvoid},), ddh.pattern)      # 0-based, on the device
colidx_device(ddh::DeviceDofHandler) = ccall((:tb_pattern_colidx_device, libtbhip), Ptr{Int32}, (Ptr{Cvoid},), ddh.pattern)
function spmv_plan(A::HIPSparseMatrixCSR)   # (row signatures, signature entries): > 0 when the index-compressed product applies
    o = zeros(Int64, 2)
    check(ccall((:tb_pattern_spmv_plan, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Int64}), A.ddh.pattern, o))
    return (o[1], o[2])
end
# cell models: states / parameters / index of the transmembrane potential, defaults (src/modeling/cells/*.jl)
function cell_model_info(model::Integer)
    ns = Ref{Cint}(0); np = Ref{Cint}(0); phi = Ref{Cint}(0)
    check(ccall((:tb_cell_model_info, libtbhip), Cint, (Cint, Ref{Cint}, Ref{Cint}, Ref{Cint}), model, ns, np, phi))
    return (Int(ns[]), Int(np[]), Int(phi[]) + 1)
end
function cell_model_defaults(model::Integer)
    ns, np, _ = cell_model_info(model)
    p = zeros(Float64, np); u0 = zeros(Float64, ns)
    check(ccall((:tb_cell_model_defaults, libtbhip), Cint, (Cint, Ptr{Float64}, Ptr{Float64}), model, p, u0))
    return p, u0
end
# Rush–Larsen step (gates exponentially, the rest forward Euler) and the reaction-tangent-controlled step (src/solver/time/rtc.jl:55-125); states SoA
function reaction_step_rl!(u::HIPVector{Float64}, model::Integer, p::Vector{Float64}, npoints::Integer, nstates::Integer, t::Real, Δt::Real)
    check(ccall((:tb_reaction_step_rl, libtbhip), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Cint, Ptr{Float64}, Int64, Cint, Cint, Cdouble, Cdouble),
        u.dev.handle, model, p, length(p), u.ptr, npoints, nstates, 0, t, Δt))
end
function reaction_step_rtc!(u::HIPVector{Float64}, du, model::Integer, p::Vector{Float64}, npoints::Integer, nstates::Integer, t::Real, Δt::Real, substeps::Integer, threshold::Real)
    rmax = Ref{Cdouble}(0)
    check(ccall((:tb_reaction_step_rtc, libtbhip), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Cint, Ptr{Float64}, Ptr{Float64}, Int64, Cint, Cint, Cdouble, Cdouble, Cint, Cdouble, Ref{Cdouble}),
        u.dev.handle, model, p, length(p), u.ptr, du === nothing ? Ptr{Float64}(C_NULL) : du.ptr, npoints, nstates, 0, t, Δt, substeps, threshold, rmax))
    return rmax[]
end
# Krylov entries beside tb_cg_solve (euler.jl:94-100; newton_raphson.jl:61,215-320): CG started from a residual the caller holds, Chebyshev / ℓ₁-Gauss–Seidel
# preconditioned CG (precond 1 / 2), restarted GMRES with a Jacobi preconditioner for the non-symmetric tangents
function cg_from_residual!(x::HIPVector{Float64}, A::HIPSparseMatrixCSR{Float64}, r0::HIPVector{Float64}; rtol = 1e-5, atol = 1e-6, maxiter = 1000, jacobi = true)
    it = Ref{Cint}(0); res = Ref{Cdouble}(0)
    check(ccall((:tb_cg_solve_from_residual, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble, Cint, Cint, Ref{Cint}, Ref{Cdouble}),
        A.ddh.pattern, A.nzval.ptr, r0.ptr, x.ptr, rtol, atol, maxiter, jacobi ? 1 : 0, it, res))
    return Int(it[]), res[]
end
function pcg!(x::HIPVector{Float64}, A::HIPSparseMatrixCSR{Float64}, b::HIPVector{Float64}; rtol = 1e-5, atol = 1e-6, maxiter = 1000, precond = 1, partsize = 64)
    it = Ref{Cint}(0); res = Ref{Cdouble}(0)
    check(ccall((:tb_pcg_solve, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble, Cint, Cint, Cint, Ref{Cint}, Ref{Cdouble}),
        A.ddh.pattern, A.nzval.ptr, b.ptr, x.ptr, rtol, atol, maxiter, precond, partsize, it, res))
    return Int(it[]), res[]
end
function gmres!(x::HIPVector{Float64}, A::HIPSparseMatrixCSR{Float64}, b::HIPVector{Float64}; rtol = 1e-8, atol = 1e-10, maxiter = 1000, restart = 30, jacobi = true)
    it = Ref{Cint}(0); res = Ref{Cdouble}(0)
    check(ccall((:tb_gmres_solve, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble, Cint, Cint, Cint, Ref{Cint}, Ref{Cdouble}),
        A.ddh.pattern, A.nzval.ptr, b.ptr, x.ptr, rtol, atol, maxiter, restart, jacobi ? 1 : 0, it, res))
    return Int(it[]), res[]
end
l1gs_apply!(z::HIPVector{Float64}, A::HIPSparseMatrixCSR{Float64}, r::HIPVector{Float64}; partsize = 64, sweep = 0) =
    check(ccall((:tb_l1gs_apply, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Cint, Cint, Ptr{Float64}, Ptr{Float64}), A.ddh.pattern, A.nzval.ptr, partsize, sweep, r.ptr, z.ptr))
# Geometric multigrid (src/solver/linear/multigrid.jl, ext/ThunderboltFerriteMultigridExt.jl: GMGPrecon over a grid hierarchy, KrylovMGSolver with CG).
# `patterns`: the tb_pattern handles of the levels, coarsest first (DeviceDofHandlers of the hierarchy's grids with the fine handler's field); `parents`:
# per refinement (parent_ptr::Vector{Int64}, parent_idx::Vector{Int32}), 0-based, of the fine nodes in the next coarser grid; `prescribed`: the flag
# vector tb_apply_zero_csr takes (device pointer, or C_NULL).  `setup!` is the numeric phase of every new Jacobian.
# `p_level = true` (PMGPrecon / ChainedMGPrecon): the last pattern carries a second-order field, the one before it the first-order field on the same
# grid; `parents` then lists the h-levels below only, and the top transfer follows from the two dof tables (tb_mg_set_p_transfer).
mutable struct HIPGMGPrecon
    handle::Ptr{Cvoid}
    degree::Int
    interval_ratio::Float64
end
function HIPGMGPrecon(dev::MI355XDevice, patterns::Vector{Ptr{Cvoid}}, n_nodes::Vector{Int64}, parents::Vector{Tuple{Vector{Int64},Vector{Int32}}};
                      prescribed::Ptr{UInt8} = Ptr{UInt8}(C_NULL), degree = 2, interval_ratio = 4.0, p_level::Bool = false)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:tb_mg_create, libtbhip), Cint, (Ptr{Cvoid}, Cint, Ref{Ptr{Cvoid}}), dev.handle, length(patterns), h))
    for (l, p) in enumerate(patterns)
        check(ccall((:tb_mg_set_level, libtbhip), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}), h[], l - 1, p))
    end
    for (l, (pptr, pidx)) in enumerate(parents)
        check(ccall((:tb_mg_set_transfer, libtbhip), Cint, (Ptr{Cvoid}, Cint, Int64, Ptr{Int64}, Ptr{Int32}), h[], l, n_nodes[l + 1], pptr, pidx))
    end
    p_level && check(ccall((:tb_mg_set_p_transfer, libtbhip), Cint, (Ptr{Cvoid}, Cint), h[], length(patterns) - 1))
    check(ccall((:tb_mg_set_prescribed, libtbhip), Cint, (Ptr{Cvoid}, Ptr{UInt8}), h[], prescribed))
    mg = HIPGMGPrecon(h[], degree, interval_ratio)
    finalizer(m -> ccall((:tb_mg_destroy, libtbhip), Cint, (Ptr{Cvoid},), m.handle), mg)
    return mg
end
setup!(mg::HIPGMGPrecon, A::HIPSparseMatrixCSR{Float64}) =
    check(ccall((:tb_mg_setup, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Cint, Cdouble), mg.handle, A.nzval.ptr, mg.degree, mg.interval_ratio))
mg_apply!(z::HIPVector{Float64}, mg::HIPGMGPrecon, r::HIPVector{Float64}) =
    check(ccall((:tb_mg_apply, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), mg.handle, r.ptr, z.ptr))
mg_prolong!(xf::HIPVector{Float64}, mg::HIPGMGPrecon, fine_level::Integer, xc::HIPVector{Float64}) =
    check(ccall((:tb_mg_prolong, libtbhip), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}), mg.handle, fine_level, xc.ptr, xf.ptr))
mg_restrict!(rc::HIPVector{Float64}, mg::HIPGMGPrecon, fine_level::Integer, rf::HIPVector{Float64}) =
    check(ccall((:tb_mg_restrict, libtbhip), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}), mg.handle, fine_level, rf.ptr, rc.ptr))
function mg_level_matrix(mg::HIPGMGPrecon, level::Integer)
    p = Ref{Ptr{Float64}}(C_NULL)
    check(ccall((:tb_mg_level_matrix, libtbhip), Cint, (Ptr{Cvoid}, Cint, Ref{Ptr{Float64}}), mg.handle, level, p))
    return p[]
end
function mg_lambda_max(mg::HIPGMGPrecon, level::Integer)
    r = Ref{Cdouble}(0)
    check(ccall((:tb_mg_level_lambda_max, libtbhip), Cint, (Ptr{Cvoid}, Cint, Ref{Cdouble}), mg.handle, level, r))
    return r[]
end
# (blocked, n_terms) of the Galerkin plan below fine_level: blocked = one term per pair of 3 × 3 blocks
function mg_level_plan(mg::HIPGMGPrecon, fine_level::Integer)
    b = Ref{Cint}(0); n = Ref{Int64}(0)
    check(ccall((:tb_mg_level_plan, libtbhip), Cint, (Ptr{Cvoid}, Cint, Ref{Cint}, Ref{Int64}), mg.handle, fine_level, b, n))
    return b[] != 0, n[]
end
# the Galerkin product below fine_level alone (what the set-up does per level), for measurements
mg_galerkin!(mg::HIPGMGPrecon, fine_level::Integer) = check(ccall((:tb_mg_galerkin, libtbhip), Cint, (Ptr{Cvoid}, Cint), mg.handle, fine_level))
# KrylovMGSolver(CG, mg): rebuild the numeric phase from the matrix, then CG with one cycle per iteration
function pcg_mg!(x::HIPVector{Float64}, A::HIPSparseMatrixCSR{Float64}, b::HIPVector{Float64}, mg::HIPGMGPrecon; rtol = 1e-5, atol = 1e-6, maxiter = 1000, setup = true)
    setup && setup!(mg, A)
    it = Ref{Cint}(0); res = Ref{Cdouble}(0)
    check(ccall((:tb_pcg_solve_mg, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble, Cint, Ptr{Cvoid}, Ref{Cint}, Ref{Cdouble}),
        A.ddh.pattern, A.nzval.ptr, b.ptr, x.ptr, rtol, atol, maxiter, mg.handle, it, res))
    return Int(it[]), res[]
end
# general mode: the matrix need not be symmetric (pivoted, unsymmetrised coarsest inverse); a change makes the next setup! redo the numeric phase
set_general!(mg::HIPGMGPrecon, general::Bool = true) = check(ccall((:tb_mg_set_general, libtbhip), Cint, (Ptr{Cvoid}, Cint), mg.handle, general ? 1 : 0))
# KrylovMGSolver(KrylovJL_GMRES(gmres_restart = restart), mg) (multigrid.jl:114-115): general mode, the numeric phase from the matrix, then GMRES(restart)
# with one cycle as the fixed right preconditioner; for mildly non-symmetric matrices with a positive diagonal
function gmres_mg!(x::HIPVector{Float64}, A::HIPSparseMatrixCSR{Float64}, b::HIPVector{Float64}, mg::HIPGMGPrecon; rtol = 1e-8, atol = 1e-14, maxiter = 5000,
                   restart = 50, setup = true, general = true)
    set_general!(mg, general)
    setup && setup!(mg, A)
    it = Ref{Cint}(0); res = Ref{Cdouble}(0)
    check(ccall((:tb_gmres_solve_mg, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble, Cint, Cint, Ptr{Cvoid}, Ref{Cint}, Ref{Cdouble}),
        A.ddh.pattern, A.nzval.ptr, b.ptr, x.ptr, rtol, atol, maxiter, restart, mg.handle, it, res))
    return Int(it[]), res[]
end
# Smoothed-aggregation algebraic multigrid (SmoothedAggregationCoarseSolver, the default pcoarse_solver of PMGPrecon: src/solver/linear/multigrid.jl:27).
# `pattern`: the tb_pattern of the matrix; `components`: one Int8 label per dof (empty: one component).  Level 0 is the matrix, level l + 1 the Galerkin
# operator of level l's aggregates.  The first `setup!` plans, every later one redoes the numeric phase on the same aggregates; `replan!` drops the plan.
mutable struct HIPAMGPrecon
    handle::Ptr{Cvoid}
    degree::Int
    interval_ratio::Float64
end
function HIPAMGPrecon(pattern::Ptr{Cvoid}; components::Vector{Int8} = Int8[], theta = 0.25, degree = 2, interval_ratio = 4.0, max_coarse = 1024, max_levels = 16)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:tb_amg_create, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Int8}, Cdouble, Cint, Cint, Ref{Ptr{Cvoid}}), pattern,
        isempty(components) ? Ptr{Int8}(C_NULL) : pointer(components), theta, max_coarse, max_levels, h))
    amg = HIPAMGPrecon(h[], degree, interval_ratio)
    finalizer(a -> ccall((:tb_amg_destroy, libtbhip), Cint, (Ptr{Cvoid},), a.handle), amg)
    return amg
end
setup!(amg::HIPAMGPrecon, A::HIPSparseMatrixCSR{Float64}) =
    check(ccall((:tb_amg_setup, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Cint, Cdouble), amg.handle, A.nzval.ptr, amg.degree, amg.interval_ratio))
replan!(amg::HIPAMGPrecon) = check(ccall((:tb_amg_replan, libtbhip), Cint, (Ptr{Cvoid},), amg.handle))
amg_apply!(z::HIPVector{Float64}, amg::HIPAMGPrecon, r::HIPVector{Float64}) =
    check(ccall((:tb_amg_apply, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), amg.handle, r.ptr, z.ptr))
function amg_n_levels(amg::HIPAMGPrecon)
    n = Ref{Cint}(0)
    check(ccall((:tb_amg_n_levels, libtbhip), Cint, (Ptr{Cvoid}, Ref{Cint}), amg.handle, n))
    return Int(n[])
end
# (dofs, non-zeros, aggregates) of a level (0-based; the last level has no aggregates)
function amg_level_size(amg::HIPAMGPrecon, level::Integer)
    n = Ref{Int64}(0); nnz = Ref{Int64}(0); na = Ref{Int64}(0)
    check(ccall((:tb_amg_level_size, libtbhip), Cint, (Ptr{Cvoid}, Cint, Ref{Int64}, Ref{Int64}, Ref{Int64}), amg.handle, level, n, nnz, na))
    return n[], nnz[], na[]
end
# A_l as host arrays (rowptr, colidx 0-based, values)
function amg_level_csr(amg::HIPAMGPrecon, level::Integer)
    n, nnz, _ = amg_level_size(amg, level)
    ptr = Vector{Int64}(undef, n + 1); col = Vector{Int32}(undef, nnz); val = Vector{Float64}(undef, nnz)
    check(ccall((:tb_amg_level_csr, libtbhip), Cint, (Ptr{Cvoid}, Cint, Ptr{Int64}, Ptr{Int32}, Ptr{Float64}), amg.handle, level, ptr, col, val))
    return ptr, col, val
end
# P from level + 1 to level as host arrays
function amg_level_prolongator(amg::HIPAMGPrecon, level::Integer)
    n, _, _ = amg_level_size(amg, level)
    nnz = Ref{Int64}(0)
    check(ccall((:tb_amg_level_prolongator, libtbhip), Cint, (Ptr{Cvoid}, Cint, Ref{Int64}, Ptr{Int64}, Ptr{Int32}, Ptr{Float64}), amg.handle, level, nnz,
        Ptr{Int64}(C_NULL), Ptr{Int32}(C_NULL), Ptr{Float64}(C_NULL)))
    ptr = Vector{Int64}(undef, n + 1); col = Vector{Int32}(undef, nnz[]); val = Vector{Float64}(undef, nnz[])
    check(ccall((:tb_amg_level_prolongator, libtbhip), Cint, (Ptr{Cvoid}, Cint, Ref{Int64}, Ptr{Int64}, Ptr{Int32}, Ptr{Float64}), amg.handle, level, nnz, ptr, col, val))
    return ptr, col, val
end
function amg_level_aggregates(amg::HIPAMGPrecon, level::Integer)
    agg = Vector{Int32}(undef, amg_level_size(amg, level)[1])
    check(ccall((:tb_amg_level_aggregates, libtbhip), Cint, (Ptr{Cvoid}, Cint, Ptr{Int32}), amg.handle, level, agg))
    return agg
end
function amg_level_strength(amg::HIPAMGPrecon, level::Integer)
    s = Vector{UInt8}(undef, amg_level_size(amg, level)[2])
    check(ccall((:tb_amg_level_strength, libtbhip), Cint, (Ptr{Cvoid}, Cint, Ptr{UInt8}), amg.handle, level, s))
    return s
end
function amg_lambda_max(amg::HIPAMGPrecon, level::Integer)
    r = Ref{Cdouble}(0)
    check(ccall((:tb_amg_level_lambda_max, libtbhip), Cint, (Ptr{Cvoid}, Cint, Ref{Cdouble}), amg.handle, level, r))
    return r[]
end
# Near-null-space of k ≤ 6 candidates on node blocks (rigid-body modes for elasticity): `node_of_dof` 0-based, 3 dofs per node; `B` is ndofs × k and is
# handed over row-major.  Before the first setup! or after replan!.
function set_near_nullspace!(amg::HIPAMGPrecon, n_nodes::Integer, node_of_dof::Vector{Int32}, B::Matrix{Float64})
    Bt = permutedims(B)
    check(ccall((:tb_amg_set_near_nullspace, libtbhip), Cint, (Ptr{Cvoid}, Int64, Ptr{Int32}, Cint, Ptr{Float64}), amg.handle, n_nodes, node_of_dof, size(B, 2), Bt))
end
function amg_level_nodes(amg::HIPAMGPrecon, level::Integer)
    nn = Ref{Int64}(0)
    node = Vector{Int32}(undef, amg_level_size(amg, level)[1])
    check(ccall((:tb_amg_level_nodes, libtbhip), Cint, (Ptr{Cvoid}, Cint, Ref{Int64}, Ptr{Int32}), amg.handle, level, nn, node))
    return nn[], node
end
# B_l (k × n_l: the columns are the dofs' rows of the row-major n_l × k array), rows of eliminated dofs zeroed
function amg_level_near_nullspace(amg::HIPAMGPrecon, level::Integer)
    k = Ref{Cint}(0)
    check(ccall((:tb_amg_level_near_nullspace, libtbhip), Cint, (Ptr{Cvoid}, Cint, Ref{Cint}, Ptr{Float64}), amg.handle, level, k, Ptr{Float64}(C_NULL)))
    B = Matrix{Float64}(undef, Int(k[]), amg_level_size(amg, level)[1])
    check(ccall((:tb_amg_level_near_nullspace, libtbhip), Cint, (Ptr{Cvoid}, Cint, Ref{Cint}, Ptr{Float64}), amg.handle, level, k, B))
    return B
end
# the tentative prolongator T_l, dense, as k × n_l (row i of the row-major array lies in the column block of its node's aggregate)
function amg_level_tentative(amg::HIPAMGPrecon, level::Integer, k::Integer)
    T = Matrix{Float64}(undef, k, amg_level_size(amg, level)[1])
    check(ccall((:tb_amg_level_tentative, libtbhip), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}), amg.handle, level, T))
    return T
end
function amg_level_dead(amg::HIPAMGPrecon, level::Integer)
    dead = Vector{UInt8}(undef, amg_level_size(amg, level + 1)[1])
    check(ccall((:tb_amg_level_dead, libtbhip), Cint, (Ptr{Cvoid}, Cint, Ptr{UInt8}), amg.handle, level, dead))
    return dead
end
# KrylovMGSolver(CG, amg): rebuild the numeric phase from the matrix, then CG with one cycle per iteration
function pcg_amg!(x::HIPVector{Float64}, A::HIPSparseMatrixCSR{Float64}, b::HIPVector{Float64}, amg::HIPAMGPrecon; rtol = 1e-5, atol = 1e-6, maxiter = 1000, setup = true)
    setup && setup!(amg, A)
    it = Ref{Cint}(0); res = Ref{Cdouble}(0)
    check(ccall((:tb_pcg_solve_amg, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble, Cint, Ptr{Cvoid}, Ref{Cint}, Ref{Cdouble}),
        A.ddh.pattern, A.nzval.ptr, b.ptr, x.ptr, rtol, atol, maxiter, amg.handle, it, res))
    return Int(it[]), res[]
end
# general mode and GMRES(restart) with one AMG cycle as the fixed right preconditioner: as set_general! and gmres_mg! of the geometric hierarchy
set_general!(amg::HIPAMGPrecon, general::Bool = true) = check(ccall((:tb_amg_set_general, libtbhip), Cint, (Ptr{Cvoid}, Cint), amg.handle, general ? 1 : 0))
function gmres_amg!(x::HIPVector{Float64}, A::HIPSparseMatrixCSR{Float64}, b::HIPVector{Float64}, amg::HIPAMGPrecon; rtol = 1e-8, atol = 1e-14, maxiter = 5000,
                    restart = 50, setup = true, general = true)
    set_general!(amg, general)
    setup && setup!(amg, A)
    it = Ref{Cint}(0); res = Ref{Cdouble}(0)
    check(ccall((:tb_gmres_solve_amg, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble, Cint, Cint, Ptr{Cvoid}, Ref{Cint}, Ref{Cdouble}),
        A.ddh.pattern, A.nzval.ptr, b.ptr, x.ptr, rtol, atol, maxiter, restart, amg.handle, it, res))
    return Int(it[]), res[]
end
# the coarsest level of a geometric or p-hierarchy is solved by one AMG cycle instead of the dense inverse (call before the first setup!); afterwards
# coarse_amg returns that hierarchy's handle for the amg_* inspectors (owned by the HIPGMGPrecon)
set_coarse_amg!(mg::HIPGMGPrecon; theta = 0.25, max_coarse = 1024, max_levels = 16) =
    check(ccall((:tb_mg_set_coarse_amg, libtbhip), Cint, (Ptr{Cvoid}, Cdouble, Cint, Cint), mg.handle, theta, max_coarse, max_levels))
function set_coarse_amg_near_nullspace!(mg::HIPGMGPrecon, n_nodes::Integer, node_of_dof::Vector{Int32}, B::Matrix{Float64})
    Bt = permutedims(B)
    check(ccall((:tb_mg_set_coarse_amg_near_nullspace, libtbhip), Cint, (Ptr{Cvoid}, Int64, Ptr{Int32}, Cint, Ptr{Float64}), mg.handle, n_nodes, node_of_dof, size(B, 2), Bt))
end
function coarse_amg(mg::HIPGMGPrecon)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:tb_mg_coarse_amg, libtbhip), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}), mg.handle, h))
    return h[]
end
function absmax(v::HIPVector{Float64}; stride = 1)
    r = Ref{Cdouble}(0)
    check(ccall((:tb_absmax, libtbhip), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Ref{Cdouble}), v.dev.handle, v.n ÷ stride, v.ptr, stride, r))
    return r[]
end
function meandiag(A::HIPSparseMatrixCSR{Float64})
    r = Ref{Cdouble}(0)
    check(ccall((:tb_meandiag, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ref{Cdouble}), A.ddh.pattern, A.nzval.ptr, r))
    return r[]
end
# a form restricted to a cell set (OrderedSet of a SubDofHandler) and a form that adds to its output instead of overwriting it
set_cellset!(form::Ptr{Cvoid}, cells::Vector{Int32}) = check(ccall((:tb_form_set_cellset, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Int32}, Int64, Cint), form, cells, length(cells), 1))
clear_cellset!(form::Ptr{Cvoid}) = check(ccall((:tb_form_clear_cellset, libtbhip), Cint, (Ptr{Cvoid},), form))
set_accumulate!(form::Ptr{Cvoid}, on::Bool) = check(ccall((:tb_form_set_accumulate, libtbhip), Cint, (Ptr{Cvoid}, Cint), form, on ? 1 : 0))
# facet terms (src/modeling/solid/weak_boundary_conditions.jl): RobinBC / NormalSpringBC / BendingSpringBC / PressureFieldBC on a facet set
function facet_form(ddh::DeviceDofHandler, bc_kind::Integer, param::Real, facets::Vector{Int32}; facet_qpoints = 0)
    form = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:tb_facet_form_create, libtbhip), Cint, (Ptr{Cvoid}, Cint, Cdouble, Cint, Ptr{Int32}, Int64, Cint, Ref{Ptr{Cvoid}}),
        ddh.mesh, bc_kind, param, facet_qpoints, facets, length(facets) ÷ 2, 1, form))
    return form[]
end
facet_set_param!(form::Ptr{Cvoid}, param::Real) = check(ccall((:tb_facet_form_set_param, libtbhip), Cint, (Ptr{Cvoid}, Cdouble), form, param))
facet_set_field!(form::Ptr{Cvoid}, field::Vector{Float64}) = check(ccall((:tb_facet_form_set_field, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64), form, field, length(field)))
facet_assemble!(form::Ptr{Cvoid}, A::HIPSparseMatrixCSR{Float64}, u::HIPVector{Float64}, r::HIPVector{Float64}, t::Real) =
    check(ccall((:tb_facet_assemble, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Cdouble, Ptr{Float64}, Ptr{Float64}), form, A.ddh.pattern, u.ptr, t, A.nzval.ptr, r.ptr))
# Diffusion across the interface between two subdomains (InterfaceDiffusionModel / BilinearInterfaceDiffusionIntegrator, src/modeling/core/diffusion.jl:76-157).
# `records` holds (cell_a, local_facet_a, cell_b, local_facet_b) per interface element and `pairing` the local vertex of cell_b that copies the k-th
# facet node of a (both 1-based, column-major 4 × n and nf × n); G is one conductance or one per interface element.  interface_assemble! ADDS the
# jump–jump term to the values of a matrix whose pattern holds the couplings among every interface element's dofs: call it after the bulk diffusion
# assembly (update_operator!), like facet_assemble!.  The sum is ordered: two assemblies give the same bits.
struct HIPInterfaceForm
    form::Ptr{Cvoid}
    n::Int
end
function HIPInterfaceForm(ddh::DeviceDofHandler, records::Matrix{Int32}, pairing::Matrix{Int32}, G::Union{Real, Vector{Float64}}; facet_qpoints = 0)
    form = Ref{Ptr{Cvoid}}(C_NULL)
    n = size(records, 2)
    per = G isa Vector{Float64} ? G : Ptr{Float64}(C_NULL)
    check(ccall((:tb_interface_form_create, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Int64, Cint, Cdouble, Ptr{Float64}, Cint, Ref{Ptr{Cvoid}}),
        ddh.mesh, records, pairing, n, facet_qpoints, G isa Real ? Float64(G) : 0.0, per, 1, form))
    return HIPInterfaceForm(form[], n)
end
interface_assemble!(f::HIPInterfaceForm, A::HIPSparseMatrixCSR{Float64}) =
    check(ccall((:tb_interface_assemble, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}), f.form, A.ddh.pattern, A.nzval.ptr))
# 3D–0D chamber coupling (src/modeling/coupler/fsi.jl:118-185, src/modeling/rsafdq2022.jl:22-85): one form per chamber surface; chamber_assemble! ADDS the
# follower-load tangent / residual at pressure p, the J_dp column, the J_pd row and the chamber volume (one device double).  Every output is optional:
# `nothing` passes C_NULL and the library skips it (chamber_assemble!(form, nothing, u, 0.0; volume = v) is compute_chamber_volume)
const TB_VOLUME_RSAFDQ2022 = Cint(0)
const TB_VOLUME_HIRSCHVOGEL2017 = Cint(1)
function chamber_form(ddh::DeviceDofHandler, volume_method::Integer, facets::Vector{Int32}; params::Union{Nothing, Vector{Float64}} = nothing, facet_qpoints = 0)
    form = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:tb_chamber_form_create, libtbhip), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Cint, Ptr{Int32}, Int64, Cint, Ref{Ptr{Cvoid}}),
        ddh.mesh, volume_method, params === nothing ? C_NULL : params, facet_qpoints, facets, length(facets) ÷ 2, 1, form))
    return form[]
end
const OptionalHIPVector = Union{Nothing, HIPVector{Float64}}
device_pointer_or_null(v::OptionalHIPVector) = v === nothing ? Ptr{Float64}(C_NULL) : v.ptr
function chamber_assemble!(form::Ptr{Cvoid}, A::Union{Nothing, HIPSparseMatrixCSR{Float64}}, u::HIPVector{Float64}, p::Real;
        r::OptionalHIPVector = nothing, col::OptionalHIPVector = nothing, row::OptionalHIPVector = nothing, volume::OptionalHIPVector = nothing)
    check(ccall((:tb_chamber_assemble, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Cdouble, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        form, A === nothing ? C_NULL : A.ddh.pattern, u.ptr, p, A === nothing ? Ptr{Float64}(C_NULL) : A.nzval.ptr,
        device_pointer_or_null(r), device_pointer_or_null(col), device_pointer_or_null(row), device_pointer_or_null(volume)))
end
# Point location and nodal inter-grid interpolation (src/ferrite-addons/transfer_operators.jl:20-161).  A HIPPointEvalHandler plays Ferrite's
# PointEvalHandler for a source DeviceDofHandler: per point the lowest-numbered cell that contains it within `tol` (reference coordinates) and ξ there.
# A Thunderbolt maintainer backs transfer! with it like this: build node_to_dof_map and the node positions exactly as transfer_operators.jl:69-114
# does (host code, unchanged), upload `nodes` (3 × n, Float64) and Int32.(node_to_dof_map .- 1), then
#     ph = HIPPointEvalHandler(ddh_from, nodes_dev, n);  n_missing(ph) == 0 || @warn …      (:116-120)
#     transfer!(u_to, ph, ddh_from_field, u_from, scatter_dev)                               (:153-161; no host trip, no allocation)
# `ddh_from_field` may carry any field over the same grid (Q1, Q2, P1, P2; 1 or 3 components).
mutable struct HIPPointEvalHandler
    handle::Ptr{Cvoid}
    ddh::DeviceDofHandler      # keeps the source mesh alive: the locator reads its coordinates and connectivity
end
function HIPPointEvalHandler(ddh::DeviceDofHandler, points::HIPVector{Float64}, npoints::Integer; tol::Real = 1e-10)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:tb_locator_create, libtbhip), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Cdouble, Ref{Ptr{Cvoid}}), ddh.mesh, npoints, points.ptr, tol, h))
    ph = HIPPointEvalHandler(h[], ddh)
    finalizer(p -> (ccall((:tb_locator_destroy, libtbhip), Cint, (Ptr{Cvoid},), p.handle); p.handle = C_NULL), ph)
    return ph
end
relocate!(ph::HIPPointEvalHandler, points::HIPVector{Float64}, npoints::Integer) =
    check(ccall((:tb_locator_relocate, libtbhip), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}), ph.handle, npoints, points.ptr))
n_points(ph::HIPPointEvalHandler) = Int(ccall((:tb_locator_npoints, libtbhip), Int64, (Ptr{Cvoid},), ph.handle))
n_missing(ph::HIPPointEvalHandler) = Int(ccall((:tb_locator_nmissing, libtbhip), Int64, (Ptr{Cvoid},), ph.handle))
cells_device(ph::HIPPointEvalHandler) = ccall((:tb_locator_cells_device, libtbhip), Ptr{Int32}, (Ptr{Cvoid},), ph.handle)      # 0-based, −1 = not found
local_coords_device(ph::HIPPointEvalHandler) = ccall((:tb_locator_xi_device, libtbhip), Ptr{Float64}, (Ptr{Cvoid},), ph.handle)
# Ferrite.evaluate_at_points(ph, dh, u): out[i·ncomp + c]; NaN where the point was not found
evaluate_at_points!(out::HIPVector{Float64}, ph::HIPPointEvalHandler, field::DeviceDofHandler, u::HIPVector{Float64}) =
    check(ccall((:tb_locator_evaluate, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}), ph.handle, field.mesh, u.ptr, out.ptr, C_NULL))
# Thunderbolt.transfer!(u_to, operator, u_from): u_to[node_to_dof_map] .= evaluate_at_points(…), the indexed store fused into the kernel
transfer!(u_to::HIPVector{Float64}, ph::HIPPointEvalHandler, field::DeviceDofHandler, u_from::HIPVector{Float64}, node_to_dof_map0::HIPVector{Int32}) =
    check(ccall((:tb_locator_evaluate, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}), ph.handle, field.mesh, u_from.ptr, u_to.ptr,
        node_to_dof_map0.ptr))
# ---------------------------------------------------------------- pseudo-ECG (src/modeling/electrophysiology/ecg.jl)
# Plonsey1964ECGGaussCache on the device: x̃ and dΩ per quadrature point are built once, update_ecg! writes κ∇φₘ (3 per point, D from the left),
# evaluate_ecg serves all electrodes in one pass.  The reductions are ordered (no floating-point atomics): two evaluations are == (test_ecg.jl).
mutable struct HIPPlonseyECGCache{Tv}
    handle::Ptr{Cvoid}
    op::HIPBilinearOperator{Tv}   # keeps the diffusion form (D, quadrature) and its mesh alive
end
function Plonsey1964ECGGaussCache(op::HIPBilinearOperator{Tv}, φₘ::HIPVector{Tv}) where {Tv}
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:tb_ecg_create, libtbhip), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}), op.form, h))
    cache = HIPPlonseyECGCache{Tv}(h[], op)
    finalizer(c -> (ccall((:tb_ecg_destroy, libtbhip), Cint, (Ptr{Cvoid},), c.handle); c.handle = C_NULL), cache)
    update_ecg!(cache, φₘ)
    return cache
end
n_quadrature_points(cache::HIPPlonseyECGCache) = Int(ccall((:tb_ecg_npoints, libtbhip), Int64, (Ptr{Cvoid},), cache.handle))
fluxes_device(cache::HIPPlonseyECGCache) = ccall((:tb_ecg_fluxes_device, libtbhip), Ptr{Float64}, (Ptr{Cvoid},), cache.handle)   # cache.κ∇φₘ, 3 per point
update_ecg!(cache::HIPPlonseyECGCache, φₘ::HIPVector{Float64}) = check(ccall((:tb_ecg_update, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}), cache.handle, φₘ.ptr))
# evaluate_ecg(cache, x, κₜ) for `n` electrodes (x: 3 × n on the device) → out[1:n]; the reference's vector method (ecg.jl:100-106) keeps the last scalar only
evaluate_ecg!(out::HIPVector{Float64}, cache::HIPPlonseyECGCache, x::HIPVector{Float64}, n::Integer, κₜ::Real) =
    check(ccall((:tb_ecg_evaluate, libtbhip), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Cdouble, Ptr{Float64}), cache.handle, n, x.ptr, κₜ, out.ptr))
# evaluate_ecg(::Geselowitz1989ECGLeadCache) = -cache.Z * cache.κ∇φₘ_t (ecg.jl:617-619) with Z dense, row-major (one lead per row of length ldz) on the device
evaluate_leads!(out::HIPVector{Float64}, Z::HIPVector{Float64}, nleads::Integer, ldz::Integer, v::HIPVector{Float64}; α::Real = -1.0) =
    check(ccall((:tb_ecg_leads, libtbhip), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Cdouble, Ptr{Float64}), v.dev.handle, nleads, v.n, Z.ptr, ldz, v.ptr, α, out.ptr))
# κ∇φₘ_t[isnan.(κ∇φₘ_t)] .= 0.0; κ∇φₘ_t .*= α (ecg.jl:345-347, 612) in one pass
scrub_scale!(x::HIPVector{Float64}, α::Real) = check(ccall((:tb_scrub_scale, libtbhip), Cint, (Ptr{Cvoid}, Int64, Cdouble, Ptr{Float64}), x.dev.handle, x.n, α, x.ptr))

# ---------------------------------------------------------------- eikonal activation times (the reference's planned ep05_eikonal tutorial; no reference code)
# √(∇Tᵀ G ∇T) = 1 with G the tensor of a diffusion form: fast iterative method on the device (Jacobi sweeps on two buffers, flag-array active set, no
# floating-point atomics on T: two solves give identical bits).  Nodes are the dofs of the scalar first-order field; hexahedra are cut implicitly
# into Kuhn tetrahedra.  The potential φₘ = U(t − T) from a tabulated template goes to update_ecg! as it is.
mutable struct HIPEikonalCache{Tv}
    handle::Ptr{Cvoid}
    op::HIPBilinearOperator{Tv}   # keeps the diffusion form (G) and its mesh alive
    sweeps::Int
    converged::Bool
end
function EikonalActivationCache(op::HIPBilinearOperator{Tv}) where {Tv}
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:tb_eikonal_create, libtbhip), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}), op.form, h))
    cache = HIPEikonalCache{Tv}(h[], op, 0, false)
    finalizer(c -> (ccall((:tb_eikonal_destroy, libtbhip), Cint, (Ptr{Cvoid},), c.handle); c.handle = C_NULL), cache)
    return cache
end
# source_dofs0: 0-based dofs of the source vertices, times ≥ 0; T: one entry per dof (+Inf where no source reaches)
function solve_activation!(T::HIPVector{Float64}, cache::HIPEikonalCache, source_dofs0::Vector{Int32}, times::Vector{Float64}; rtol::Real = 1e-12,
                           max_sweeps::Integer = T.n)
    sweeps = Ref{Cint}(0); conv = Ref{Cint}(0)
    check(ccall((:tb_eikonal_solve, libtbhip), Cint, (Ptr{Cvoid}, Int64, Ptr{Int32}, Ptr{Float64}, Cdouble, Cint, Ptr{Float64}, Ref{Cint}, Ref{Cint}),
        cache.handle, length(source_dofs0), source_dofs0, times, rtol, max_sweeps, T.ptr, sweeps, conv))
    cache.sweeps = Int(sweeps[]); cache.converged = conv[] != 0
    return T
end
eikonal_residual!(res::HIPVector{Float64}, cache::HIPEikonalCache, T::HIPVector{Float64}) =
    check(ccall((:tb_eikonal_residual, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), cache.handle, T.ptr, res.ptr))
# (nodes evaluated, updates accepted, local solves made) of the latest solve
function eikonal_last_counts(cache::HIPEikonalCache)
    c = zeros(Int64, 3)
    check(ccall((:tb_eikonal_last_counts, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Int64}), cache.handle, c))
    return (c[1], c[2], c[3])
end
# φₘ = U(t − T): U sampled at t0 + k·dt on the device, clamped at both ends (the first sample where T = Inf)
activation_potential!(φₘ::HIPVector{Float64}, T::HIPVector{Float64}, t::Real, template::HIPVector{Float64}, t0::Real, dt::Real) =
    check(ccall((:tb_eikonal_potential, libtbhip), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Cdouble, Int64, Cdouble, Cdouble, Ptr{Float64}, Ptr{Float64}),
        T.dev.handle, T.n, T.ptr, t, template.n, t0, dt, template.ptr, φₘ.ptr))
# the local solver on the host (one tetrahedron): value and minimiser λ
function eikonal_local_solve(x4::Vector{Float64}, x123::Vector{Float64}, T123::Vector{Float64}, M6::Vector{Float64})
    value = Ref{Cdouble}(0.0); λ = zeros(3)
    check(ccall((:tb_host_eikonal_local_solve, libtbhip), Cint, (Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Cdouble}, Ptr{Float64}),
        x4, x123, T123, M6, value, λ))
    return value[], λ
end

# ---------------------------------------------------------------- parabolic-elliptic bidomain block system (src/modeling/electrophysiology.jl:305-326)
# The 2 × 2 block operator [M − ΔtKᵢ, −ΔtKᵢ; −ΔtKᵢ, −Δt(Kᵢ + Kₑ)] over the scalar pattern, φₑ grounded at flagged nodes.  Block vectors are
# node-interleaved (2n values: φₘ,ⱼ, φₑ,ⱼ); pack! / unpack! move between them and the host's two vectors.
mutable struct HIPBidomainSystem
    handle::Ptr{Cvoid}
    ddh::DeviceDofHandler   # keeps the pattern alive
end
function HIPBidomainSystem(ddh::DeviceDofHandler)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:tb_bidomain_create, libtbhip), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}), ddh.pattern, h))
    sys = HIPBidomainSystem(h[], ddh)
    finalizer(s -> (ccall((:tb_bidomain_destroy, libtbhip), Cint, (Ptr{Cvoid},), s.handle); s.handle = C_NULL), sys)
    return sys
end
# ground_flags: one byte per node; ground_diag: the diagonal of the eliminated φₑ rows (Δt·(meandiag(Kᵢ) + meandiag(Kₑ)) or 1)
update_system_matrix!(sys::HIPBidomainSystem, M::HIPSparseMatrixCSR{Float64}, Kᵢ::HIPSparseMatrixCSR{Float64}, Kₑ::HIPSparseMatrixCSR{Float64}, Δt::Real,
                      ground_flags::HIPVector{UInt8}, ground_diag::Real) =
    check(ccall((:tb_bidomain_set_matrices, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{UInt8}, Cdouble),
        sys.handle, M.ddh.pattern, M.nzval.ptr, Kᵢ.nzval.ptr, Kₑ.nzval.ptr, Δt, ground_flags.ptr, ground_diag))
bidomain_mul!(y::HIPVector{Float64}, sys::HIPBidomainSystem, x::HIPVector{Float64}) =
    check(ccall((:tb_bidomain_apply, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), sys.handle, x.ptr, y.ptr))
function bidomain_solve!(x::HIPVector{Float64}, sys::HIPBidomainSystem, b::HIPVector{Float64}; rtol::Real = 1e-5, atol::Real = 1e-6, maxiter::Integer = 1000)
    iters, res = Ref{Cint}(0), Ref{Cdouble}(0.0)
    check(ccall((:tb_bidomain_solve, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble, Cint, Ref{Cint}, Ref{Cdouble}),
        sys.handle, b.ptr, x.ptr, rtol, atol, maxiter, iters, res))
    return Int(iters[]), res[]
end
pack!(out::HIPVector{Float64}, sys::HIPBidomainSystem, φₘ::HIPVector{Float64}, φₑ::Union{HIPVector{Float64}, Nothing}; zero_ground::Bool = false) =
    check(ccall((:tb_bidomain_pack, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cint, Ptr{Float64}), sys.handle, φₘ.ptr,
        φₑ === nothing ? Ptr{Float64}(C_NULL) : φₑ.ptr, zero_ground ? 1 : 0, out.ptr))
unpack!(φₘ::HIPVector{Float64}, φₑ::HIPVector{Float64}, sys::HIPBidomainSystem, x::HIPVector{Float64}) =
    check(ccall((:tb_bidomain_unpack, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), sys.handle, x.ptr, φₘ.ptr, φₑ.ptr))

# Geometric multigrid preconditioner of the block system (tb_bidomain_mg_*): one V(degree, degree) cycle on the node pairs over the levels of a
# HIPGMGPrecon built WITHOUT prescribed dofs (the ground comes from update_system_matrix!) whose finest pattern is the system's; setup! follows every
# update_system_matrix!, and need not be preceded by setup!(::HIPGMGPrecon, A).
mutable struct HIPBidomainMultigrid
    handle::Ptr{Cvoid}
    sys::HIPBidomainSystem   # both outlive the handle
    mg::HIPGMGPrecon
end
function HIPBidomainMultigrid(sys::HIPBidomainSystem, mg::HIPGMGPrecon)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:tb_bidomain_mg_create, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{Ptr{Cvoid}}), sys.handle, mg.handle, h))
    bmg = HIPBidomainMultigrid(h[], sys, mg)
    finalizer(m -> (ccall((:tb_bidomain_mg_destroy, libtbhip), Cint, (Ptr{Cvoid},), m.handle); m.handle = C_NULL), bmg)
    return bmg
end
setup!(bmg::HIPBidomainMultigrid) =
    check(ccall((:tb_bidomain_mg_setup, libtbhip), Cint, (Ptr{Cvoid}, Cint, Cdouble), bmg.handle, bmg.mg.degree, bmg.mg.interval_ratio))
mg_apply!(z::HIPVector{Float64}, bmg::HIPBidomainMultigrid, r::HIPVector{Float64}) =
    check(ccall((:tb_bidomain_mg_apply, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), bmg.handle, r.ptr, z.ptr))
function bidomain_solve!(x::HIPVector{Float64}, bmg::HIPBidomainMultigrid, b::HIPVector{Float64}; rtol::Real = 1e-5, atol::Real = 1e-6, maxiter::Integer = 1000)
    iters, res = Ref{Cint}(0), Ref{Cdouble}(0.0)
    check(ccall((:tb_bidomain_mg_solve, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble, Cint, Ref{Cint}, Ref{Cdouble}),
        bmg.handle, b.ptr, x.ptr, rtol, atol, maxiter, iters, res))
    return Int(iters[]), res[]
end
function n_levels(bmg::HIPBidomainMultigrid)
    n = Ref{Cint}(0)
    check(ccall((:tb_bidomain_mg_n_levels, libtbhip), Cint, (Ptr{Cvoid}, Ref{Cint}), bmg.handle, n))
    return Int(n[])
end
# the four planes (a₁₁ | a₁₂ | a₂₁ | a₂₂) of a level, each in the CSR order of that level's scalar pattern: (device pointer, nnz)
function mg_level_planes(bmg::HIPBidomainMultigrid, level::Integer)
    p, nnz = Ref{Ptr{Float64}}(C_NULL), Ref{Int64}(0)
    check(ccall((:tb_bidomain_mg_level_planes, libtbhip), Cint, (Ptr{Cvoid}, Cint, Ref{Ptr{Float64}}, Ref{Int64}), bmg.handle, level, p, nnz))
    return p[], nnz[]
end
function mg_level_lambda_max(bmg::HIPBidomainMultigrid, level::Integer)
    λ = Ref{Cdouble}(0.0)
    check(ccall((:tb_bidomain_mg_level_lambda_max, libtbhip), Cint, (Ptr{Cvoid}, Cint, Ref{Cdouble}), bmg.handle, level, λ))
    return λ[]
end
# measurement hook: the coarse tail of a cycle on whatever the level's buffers hold; only its duration means something
mg_cycle_below!(bmg::HIPBidomainMultigrid, level::Integer) = check(ccall((:tb_bidomain_mg_cycle_below, libtbhip), Cint, (Ptr{Cvoid}, Cint), bmg.handle, level))

# Algebraic multigrid preconditioner of the block system (tb_bidomain_amg_*): one smoothed-aggregation V(degree, degree) cycle on the node pairs, built from
# the matrix alone — for tetrahedra and every other mesh without nested grids.  Levels are numbered as HIPAMGPrecon's: 0 is the finest.  setup! follows every
# update_system_matrix!: the first one plans, every later one redoes the numeric phase on the same aggregates; replan! drops the plan.
mutable struct HIPBidomainAlgebraicMultigrid
    handle::Ptr{Cvoid}
    sys::HIPBidomainSystem   # outlives the handle
    degree::Int
    interval_ratio::Float64
end
function HIPBidomainAlgebraicMultigrid(sys::HIPBidomainSystem; theta::Real = 0.25, degree::Integer = 2, interval_ratio::Real = 4.0, max_coarse::Integer = 128,
                                       max_levels::Integer = 16)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:tb_bidomain_amg_create, libtbhip), Cint, (Ptr{Cvoid}, Cdouble, Cint, Cint, Ref{Ptr{Cvoid}}), sys.handle, theta, max_coarse, max_levels, h))
    bamg = HIPBidomainAlgebraicMultigrid(h[], sys, degree, interval_ratio)
    finalizer(m -> (ccall((:tb_bidomain_amg_destroy, libtbhip), Cint, (Ptr{Cvoid},), m.handle); m.handle = C_NULL), bamg)
    return bamg
end
setup!(bamg::HIPBidomainAlgebraicMultigrid) =
    check(ccall((:tb_bidomain_amg_setup, libtbhip), Cint, (Ptr{Cvoid}, Cint, Cdouble), bamg.handle, bamg.degree, bamg.interval_ratio))
replan!(bamg::HIPBidomainAlgebraicMultigrid) = check(ccall((:tb_bidomain_amg_replan, libtbhip), Cint, (Ptr{Cvoid},), bamg.handle))
mg_apply!(z::HIPVector{Float64}, bamg::HIPBidomainAlgebraicMultigrid, r::HIPVector{Float64}) =
    check(ccall((:tb_bidomain_amg_apply, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), bamg.handle, r.ptr, z.ptr))
function bidomain_solve!(x::HIPVector{Float64}, bamg::HIPBidomainAlgebraicMultigrid, b::HIPVector{Float64}; rtol::Real = 1e-5, atol::Real = 1e-6, maxiter::Integer = 1000)
    iters, res = Ref{Cint}(0), Ref{Cdouble}(0.0)
    check(ccall((:tb_bidomain_amg_solve, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble, Cint, Ref{Cint}, Ref{Cdouble}),
        bamg.handle, b.ptr, x.ptr, rtol, atol, maxiter, iters, res))
    return Int(iters[]), res[]
end
function n_levels(bamg::HIPBidomainAlgebraicMultigrid)
    n = Ref{Cint}(0)
    check(ccall((:tb_bidomain_amg_n_levels, libtbhip), Cint, (Ptr{Cvoid}, Ref{Cint}), bamg.handle, n))
    return Int(n[])
end
# (nodes, non-zeros of the scalar pattern, aggregates) of a level; the last level has no aggregates
function amg_level_size(bamg::HIPBidomainAlgebraicMultigrid, level::Integer)
    n, nnz, na = Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0)
    check(ccall((:tb_bidomain_amg_level_size, libtbhip), Cint, (Ptr{Cvoid}, Cint, Ref{Int64}, Ref{Int64}, Ref{Int64}), bamg.handle, level, n, nnz, na))
    return n[], nnz[], na[]
end
# the level's scalar pattern (0-based row pointers and columns) and its four planes (a₁₁, a₁₂, a₂₁, a₂₂) in that CSR order, on the host
function amg_level_blocks(bamg::HIPBidomainAlgebraicMultigrid, level::Integer)
    n, nnz, _ = amg_level_size(bamg, level)
    rowptr, colidx = Vector{Int64}(undef, n + 1), Vector{Int32}(undef, nnz)
    check(ccall((:tb_bidomain_amg_level_csr, libtbhip), Cint, (Ptr{Cvoid}, Cint, Ptr{Int64}, Ptr{Int32}), bamg.handle, level, rowptr, colidx))
    planes = [Vector{Float64}(undef, nnz) for _ in 1:4]
    check(ccall((:tb_bidomain_amg_level_planes, libtbhip), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), bamg.handle, level,
        planes[1], planes[2], planes[3], planes[4]))
    return rowptr, colidx, planes
end
# the scalar P from level + 1 to level (0-based CSR); the block transfer is P ⊗ I₂
function amg_level_prolongator(bamg::HIPBidomainAlgebraicMultigrid, level::Integer)
    n, _, _ = amg_level_size(bamg, level)
    nnz = Ref{Int64}(0)
    check(ccall((:tb_bidomain_amg_level_prolongator, libtbhip), Cint, (Ptr{Cvoid}, Cint, Ref{Int64}, Ptr{Int64}, Ptr{Int32}, Ptr{Float64}), bamg.handle, level, nnz,
        Ptr{Int64}(C_NULL), Ptr{Int32}(C_NULL), Ptr{Float64}(C_NULL)))
    rowptr, colidx, values = Vector{Int64}(undef, n + 1), Vector{Int32}(undef, nnz[]), Vector{Float64}(undef, nnz[])
    check(ccall((:tb_bidomain_amg_level_prolongator, libtbhip), Cint, (Ptr{Cvoid}, Cint, Ref{Int64}, Ptr{Int64}, Ptr{Int32}, Ptr{Float64}), bamg.handle, level, nnz,
        rowptr, colidx, values))
    return rowptr, colidx, values
end
function amg_level_aggregates(bamg::HIPBidomainAlgebraicMultigrid, level::Integer)
    agg = Vector{Int32}(undef, amg_level_size(bamg, level)[1])
    check(ccall((:tb_bidomain_amg_level_aggregates, libtbhip), Cint, (Ptr{Cvoid}, Cint, Ptr{Int32}), bamg.handle, level, agg))
    return agg
end
# (successful set-ups so far, host aggregation runs so far): a numeric-only set-up adds one to the first and nothing to the second
function amg_counts(bamg::HIPBidomainAlgebraicMultigrid)
    s, a = Ref{Int64}(0), Ref{Int64}(0)
    check(ccall((:tb_bidomain_amg_counts, libtbhip), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}), bamg.handle, s, a))
    return s[], a[]
end
# measurement hook: the Galerkin products between `level` and the level below once more, fused or as three launch pairs of the scalar kernel; same bits
amg_products!(bamg::HIPBidomainAlgebraicMultigrid, level::Integer, fused::Bool = true) =
    check(ccall((:tb_bidomain_amg_products, libtbhip), Cint, (Ptr{Cvoid}, Cint, Cint), bamg.handle, level, fused ? 1 : 0))
function amg_level_lambda_max(bamg::HIPBidomainAlgebraicMultigrid, level::Integer)
    λ = Ref{Cdouble}(0.0)
    check(ccall((:tb_bidomain_amg_level_lambda_max, libtbhip), Cint, (Ptr{Cvoid}, Cint, Ref{Cdouble}), bamg.handle, level, λ))
    return λ[]
end

# ---------------------------------------------------------------- Newmark-β elastodynamics (src/solver/time/newmark.jl)
# The mass operator of the displacement field is an ordinary HIPBilinearOperator: tb_assemble_matrix accepts BilinearMassIntegrator on ncomp = 3.
# ũ = uₙ + Δt vₙ + (½−β)Δt² aₙ, ṽ = vₙ + (1−γ)Δt aₙ (newmark.jl:580-581)
newmark_predict!(ũ::HIPVector{Float64}, ṽ::HIPVector{Float64}, u::HIPVector{Float64}, v::HIPVector{Float64}, a::HIPVector{Float64}, Δt::Real, β::Real, γ::Real) =
    check(ccall((:tb_newmark_predict, libtbhip), Cint, (Ptr{Cvoid}, Int64, Cdouble, Cdouble, Cdouble, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        u.dev.handle, u.n, Δt, β, γ, u.ptr, v.ptr, a.ptr, ũ.ptr, ṽ.ptr))
# _add_inertia_residual! and _add_inertia_linearization! (newmark.jl:97-110) in one pass over M: residual += M(u−ũ)/(βΔt²), J += M/(βΔt²); either output may be `nothing`
function newmark_stage!(J::Union{HIPSparseMatrixCSR{Float64}, Nothing}, residual::Union{HIPVector{Float64}, Nothing}, M::HIPSparseMatrixCSR{Float64}, u::HIPVector{Float64},
                        ũ::HIPVector{Float64}, βΔt²::Real)
    check(ccall((:tb_newmark_stage, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Cdouble, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        M.ddh.pattern, M.nzval.ptr, inv(βΔt²), u.ptr, ũ.ptr, J === nothing ? C_NULL : J.nzval.ptr, residual === nothing ? C_NULL : residual.ptr))
end
# aₙ₊₁ = (u−ũ)/(βΔt²), vₙ₊₁ = ṽ + γΔt aₙ₊₁ (newmark.jl:91-95, 171-180)
newmark_correct!(a::HIPVector{Float64}, v::HIPVector{Float64}, u::HIPVector{Float64}, ũ::HIPVector{Float64}, ṽ::HIPVector{Float64}, Δt::Real, β::Real, γ::Real) =
    check(ccall((:tb_newmark_correct, libtbhip), Cint, (Ptr{Cvoid}, Int64, Cdouble, Cdouble, Cdouble, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        u.dev.handle, u.n, Δt, β, γ, u.ptr, ũ.ptr, ṽ.ptr, a.ptr, v.ptr))
# _newmark_hermite! (newmark.jl:305-382) on the displacement block: D-th derivative of the cubic through (uprev, vprev), (u, v) at θ = (t − tprev)/Δt
hermite_interpolate!(out::HIPVector{Float64}, θ::Real, Δt::Real, D::Integer, uprev::HIPVector{Float64}, vprev::HIPVector{Float64}, u::HIPVector{Float64}, v::HIPVector{Float64}) =
    check(ccall((:tb_hermite_interpolate, libtbhip), Cint, (Ptr{Cvoid}, Int64, Cdouble, Cdouble, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        out.dev.handle, out.n, θ, Δt, D, uprev.ptr, vprev.ptr, u.ptr, v.ptr, out.ptr))

# sarcomere models (RDQ20-MF …): explicit and implicit pointwise steps (src/modeling/solid/materials.jl:1403-1640 condenses them per quadrature point)
function sarcomere_model_info(model::Integer)
    ns = Ref{Cint}(0); np = Ref{Cint}(0)
    check(ccall((:tb_sarcomere_model_info, libtbhip), Cint, (Cint, Ref{Cint}, Ref{Cint}), model, ns, np))
    return Int(ns[]), Int(np[])
end
function sarcomere_step!(Q::HIPVector{Float64}, model::Integer, p::Vector{Float64}, npoints::Integer, stretch::Real, velocity::Real, calcium::Real, t::Real, Δt::Real; substeps = 1)
    check(ccall((:tb_sarcomere_step, libtbhip), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Float64}, Cint, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble, Cdouble, Cdouble, Cdouble, Cint, Cint, Ptr{Float64}, Ptr{Float64}),
        Q.dev.handle, model, p, length(p), Q.ptr, npoints, C_NULL, C_NULL, C_NULL, stretch, velocity, calcium, t, Δt, substeps, 0, C_NULL, C_NULL))
end
function sarcomere_implicit_step!(Q::HIPVector{Float64}, Qknown::HIPVector{Float64}, model::Integer, p::Vector{Float64}, npoints::Integer, stretch::Real, velocity::Real, calcium::Real, Δt::Real;
                                  tol = 1e-10, max_iters = 20)
    nf = Ref{Int64}(0)
    check(ccall((:tb_sarcomere_implicit_step, libtbhip), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Float64}, Cint, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble, Cdouble, Cdouble, Cdouble, Cint, Ptr{Float64}, Ptr{Float64},
         Ptr{Int32}, Ref{Int64}),
        Q.dev.handle, model, p, length(p), Q.ptr, Qknown.ptr, npoints, C_NULL, C_NULL, C_NULL, stretch, velocity, calcium, Δt, tol, max_iters, C_NULL, C_NULL, C_NULL, nf))
    return Int(nf[])
end
# condensed internal variables and the other setters of a hyperelastic form (src/modeling/solid/elements.jl:411-630)
set_active_tension!(form::Ptr{Cvoid}, tension::Real) = check(ccall((:tb_hyperelastic_set_active_tension, libtbhip), Cint, (Ptr{Cvoid}, Cdouble, Ptr{Float64}, Int64), form, tension, C_NULL, 0))
set_prestress!(form::Ptr{Cvoid}, F0inv::Vector{Float64}) = check(ccall((:tb_hyperelastic_set_prestress, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}), form, F0inv))
set_condensation!(form::Ptr{Cvoid}, sarcomere_model::Integer, p::Vector{Float64}, tmax::Real; local_tol = 1e-10, local_max_iters = 20) =
    check(ccall((:tb_hyperelastic_set_condensation, libtbhip), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Cint, Cdouble, Cdouble, Cint), form, sarcomere_model, p, length(p), tmax, local_tol, local_max_iters))
function n_quadrature_points(form::Ptr{Cvoid})
    n = Ref{Int64}(0)
    check(ccall((:tb_hyperelastic_n_quadrature_points, libtbhip), Cint, (Ptr{Cvoid}, Ref{Int64}), form, n))
    return Int(n[])
end
set_internal_state!(form::Ptr{Cvoid}, Q::HIPVector{Float64}, Qknown::HIPVector{Float64}, Δt::Real) =
    check(ccall((:tb_hyperelastic_set_internal_state, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble), form, Q.ptr, Qknown.ptr, Δt))
set_previous_solution!(form::Ptr{Cvoid}, uprev::HIPVector{Float64}) = check(ccall((:tb_hyperelastic_set_previous_solution, libtbhip), Cint, (Ptr{Cvoid}, Ptr{Float64}), form, uprev.ptr))
function local_solve_report(form::Ptr{Cvoid})
    nf = Ref{Int64}(0)
    check(ccall((:tb_hyperelastic_local_solve_report, libtbhip), Cint, (Ptr{Cvoid}, Ref{Int64}, Ptr{Int32}, Int64), form, nf, C_NULL, 0))
    return Int(nf[])
end
# LinearMaxwellMaterial (src/modeling/solid/materials.jl:1816-2008): a form of its own kind over the same entries as the condensed sarcomere path —
# set_internal_state! (six values per quadrature point, SymmetricTensor{2,3}.data order), n_quadrature_points, local_solve_report, linearize / residual
function viscoelastic_form(mesh::Ptr{Cvoid}, E₀::Real, E₁::Real, μ::Real, η₁::Real, ν::Real)
    form = Ref{Ptr{Cvoid}}(C_NULL)
    p = Float64[E₀, E₁, μ, η₁, ν]
    check(ccall((:tb_viscoelastic_create, libtbhip), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Cint, Ref{Ptr{Cvoid}}), mesh, 0, p, length(p), form))
    return form[]
end
# the kernels' point routine on the host: (εᵛ₁, σ, ∂σ/∂F) of one local backward-Euler step from Qknown; F and σ row-major
function host_maxwell_eval(p::Vector{Float64}, F::Vector{Float64}, Qknown::Vector{Float64}, Δt::Real)
    Q = zeros(6); P = zeros(9); A = zeros(81)
    check(ccall((:tb_host_maxwell_eval, libtbhip), Cint, (Ptr{Float64}, Cint, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        p, length(p), F, Qknown, Δt, Q, P, A))
    return Q, P, A
end
function comm_rank_size(c::HIPComm)
    r = Ref{Cint}(0); n = Ref{Cint}(0)
    check(ccall((:tb_comm_rank_size, libtbhip), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Cint}), c.handle, r, n))
    return Int(r[]), Int(n[])
end

end # module