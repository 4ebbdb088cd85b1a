# integration/MomCoreRT.jl -- the hand-written Julia host layer above integration/MomCore.jl (the generated `ccall`
# wrappers): the `MI355X <: AbstractArchitecture` methods a vSmartMOM.jl maintainer adds so that
# parameters_from_yaml() / model_from_parameters() / rt_run() keep their surface and the CoreRT layer loop runs in
# libmomcore.so.  Included from src/CoreRT/CoreRT.jl after `include("MomCore.jl")`.
#
# NOT executed in the build image (Julia is absent there).  What IS machine-checked (tests/test_julia_bindings.py):
# every `mom_*` call below names a wrapper that integration/MomCore.jl generates from include/momcore.h, with exactly
# the number of arguments the header declares; the Python twin of each function (radiativetransfer.jl_amd/corert.py,
# same call sequence through ctypes) is what the GPU parity tests execute.
#
# Seams in the reference: src/Architectures.jl:20-55 (architecture types, array_type, devi),
# src/CoreRT/rt_run.jl:19-21 (rt_run(model)), :41-230 (rt_run(RS_type, model, iBand)), CoreKernel/rt_kernel.jl:173-183,
# CoreKernel/elemental.jl:109-118, CoreKernel/doubling.jl:81-86, CoreKernel/interaction_inelastic.jl:474-477,
# rt_run_multisensor.jl:14-191, tools/atmo_prof.jl:427-449.

using .MomCore
using .MomCore: momcheck, MomError

# >>> architecture
# src/Architectures.jl (add): one more architecture; CPU() / GPU() behaviour is untouched because Julia picks the most
# specific method.  Host arrays stay `Array`: device memory is owned by the mom_t handle.
struct MI355X <: AbstractArchitecture
    device::Cint
end
MI355X() = MI355X(0)
array_type(::MI355X) = Array
devi(::MI355X)       = KernelAbstractions.CPU()   # never used on this path
# src/CoreRT/tools/parameters_from_yaml.jl:97-98 -- add "Architectures.MI355X()" to the whitelist of `architecture:`
# <<< architecture

# >>> handle
"""One handle <-> one GPU <-> one HIP stream (include/momcore.h); destroyed by `close` or the finalizer."""
mutable struct MomHandle
    ptr::Ptr{Cvoid}
    N::Int; nStokes::Int; nSpec::Int; max_m::Int
    function MomHandle(arch::MI355X, N, nStokes, nSpec, max_m; float_type = Float64)
        out = Ref{Ptr{Cvoid}}(C_NULL)
        momcheck(MomCore.mom_create(out, arch.device, N, nStokes, nSpec, max_m, float_type === Float32 ? 1 : 0))
        h = new(out[], N, nStokes, nSpec, max_m)
        finalizer(close, h)
        return h
    end
end
function Base.close(h::MomHandle)
    h.ptr == C_NULL && return
    MomCore.mom_destroy(h.ptr)
    h.ptr = C_NULL
    return
end
# <<< handle

iface_code(::ScatteringInterface_00) = Cint(0)
iface_code(::ScatteringInterface_01) = Cint(1)
iface_code(::ScatteringInterface_10) = Cint(2)
iface_code(::ScatteringInterface_11) = Cint(3)

# >>> scene
"""
Host preparation of rt_run.jl:43-138 (unchanged Julia, runs on `Array`) and the upload of the scene: streams,
layer optics in the library's native input form (K phase-matrix bases + per-point weights instead of the N×N×nSpec
array of expandOpticalProperties, compEffectiveLayerProperties.jl:124-135), doubling numbers, interface codes,
surface.  Returns the handle with everything resident in HBM.
"""
function momcore_scene(RS_type, model::vSmartMOM_Model, iBand, arch::MI355X; strict_reference_indexing::Bool = true, split = nothing,
                       z_moments_on_device::Bool = false, z_resident::Bool = false)
    @unpack qp_μ, qp_μN, wt_μN, iμ₀, μ₀ = model.quad_points
    pol   = model.params.polarization_type
    max_m = model.params.max_m
    N     = length(qp_μN)
    nSpec = sum(size(model.τ_abs[iB], 1) for iB in iBand)
    props = constructCoreOpticalProperties(RS_type, iBand, 0, model)[1]                    # τ, ϖ do not depend on m
    ifaces, τ_sum = extractEffectiveProps(props, model.quad_points)
    nd    = Cint[get_dtau_ndoubl(l, model.quad_points)[2] for l in props]                  # GLOBAL maxima (rt_kernel.jl:241)
    τ     = reduce(hcat, [l.τ for l in props]);  ϖ = reduce(hcat, [l.ϖ for l in props])   # [nSpec, Nz]
    # [N,N,K,M] ×2, [K,nSpec,Nz]; z_resident: Zpp = Zmp = nothing -- the handle forms the bases from the Greek sets (stage_greeks!)
    Zpp, Zmp, zw = z_bases_and_weights(RS_type, iBand, model; z_moments_on_device, z_resident)
    node  = Cint[nearest_point(qp_μ, cosd(v)) for v in model.obs_geom.vza]
    cosm  = [cosd(m * a) for a in model.obs_geom.vaz, m in 0:max_m-1]
    sinm  = [sind(m * a) for a in model.obs_geom.vaz, m in 0:max_m-1]
    brdf  = model.params.brdf[iBand[1]]

    # Dual models (rt_run_dual below): `split = (val, part)` takes the values for the uploads here and returns the partials
    val, part = split === nothing ? (identity, A -> nothing) : split
    h = MomHandle(arch, N, pol.n, nSpec, max_m; float_type = model.params.float_type)
    MomCore.mom_set_streams!(h.ptr, qp_μN, wt_μN, N, iμ₀, μ₀, pol.I₀, pol.D, strict_reference_indexing ? 1 : 0)
    albedo = brdf isa LambertianSurfaceScalar ? brdf.albedo : zero(eltype(τ))
    z_resident && stage_greeks!(h, scene_greeks(model, iBand), max_m)      # then Zpp = Zmp = C_NULL below: "the staged bases"
    MomCore.mom_scene_set!(h.ptr, length(nd), size(zw, 1), max_m, val(τ), val(ϖ), val(zw), z_resident ? C_NULL : val(Zpp),
                           z_resident ? C_NULL : val(Zmp), nd, iface_code.(ifaces), val(τ_sum), Float64(val([albedo])[1]), length(node),
                           node, cosm, sinm)
    dRsurf = dalb = nothing
    if brdf isa LambertianSurfaceLegendre                       # lambertian_surface.jl:90-96: spectral albedo
        alb = legendre_albedo(brdf, model, iBand)
        MomCore.mom_scene_set_surface!(h.ptr, 2, max_m, C_NULL, val(alb));  dalb = part(alb)
    elseif !(brdf isa LambertianSurfaceScalar)                  # rpvSurfaceScalar, RossLiSurfaceScalar: BRDF Fourier moments
        Rsurf = cat([(m == 0 ? 2 : 1) * reflectance(brdf, pol, Array(qp_μ), m) for m in 0:max_m-1]...; dims = 3)
        MomCore.mom_scene_set_surface!(h.ptr, 1, max_m, val(Rsurf), C_NULL);  dRsurf = part(Rsurf)
    end
    split === nothing && return h
    return h, (dτ = part(τ), dϖ = part(ϖ), dzw = part(zw), dZpp = z_resident ? nothing : part(Zpp),
               dZmp = z_resident ? nothing : part(Zmp), dalbedo = part([albedo]),
               dRsurf = dRsurf, dalbedo_spec = dalb)
end
# <<< scene

# >>> rt_run_noRS
"""rt_run(RS_type::noRS, model, iBand) on the MI355X: the layer loop of rt_run.jl:125-215 is ONE call."""
function rt_run(RS_type::noRS, model::vSmartMOM_Model, iBand, arch::MI355X)
    h = momcore_scene(RS_type, model, iBand, arch)
    try
        pol, nV, nSpec = model.params.polarization_type, length(model.obs_geom.vza), h.nSpec
        MomCore.mom_rt_run!(h.ptr)                                    # elemental! -> doubling! -> interaction!, surface, post-processing
        R_SFI = zeros(nV, pol.n, nSpec);  T_SFI = similar(R_SFI)      # rt_run.jl:89-90 layout
        MomCore.mom_get_RT!(h.ptr, R_SFI, T_SFI)
        hdr = similar(R_SFI);  bhr_uw = zeros(pol.n, nSpec);  bhr_dw = similar(bhr_uw)    # rt_run.jl:91-94
        MomCore.mom_get_hdr!(h.ptr, hdr, bhr_uw, bhr_dw)
        return R_SFI, T_SFI, zero(R_SFI), zero(R_SFI), hdr, bhr_uw[1, :], bhr_dw[1, :]    # the 7-tuple of rt_run.jl:226
    finally
        close(h)
    end
end

# >>> rt_run_dual
"""
rt_run on a model whose optical properties are ForwardDiff.Dual (the reference's Jacobian route: rt_run.jl:89-96 allocates
R, T, R_SFI, T_SFI in the Dual type and the whole layer loop runs on Dual arrays, gpu_batched.jl:100-150).  The host
preparation above runs unchanged on the Dual arrays; values and partials are separated at the boundary
(`ForwardDiff.value` / `ForwardDiff.partials`), uploaded with mom_scene_set / mom_scene_set_partials, and the results are
re-assembled into Dual arrays of the caller's tag: every downstream `ForwardDiff.jacobian` sees exactly what the CPU run returns.
"""
function rt_run_dual(RS_type::noRS, model::vSmartMOM_Model, iBand, arch::MI355X, ::Type{D}) where {T, V, P, D <: ForwardDiff.Dual{T, V, P}}
    val(A)     = ForwardDiff.value.(A)
    part(A)    = cat((ForwardDiff.partials.(A, i) for i in 1:P)...; dims = ndims(A) + 1)   # partial index = slowest axis
    h, dual_in = momcore_scene(RS_type, model, iBand, arch; split = (val, part))            # τ, ϖ, zw, Z bases, surface as Duals
    try
        pol, nV, nSpec = model.params.polarization_type, length(model.obs_geom.vza), h.nSpec
        nn(x) = x === nothing ? C_NULL : x                            # an input without partials: NULL
        MomCore.mom_scene_set_partials!(h.ptr, P, dual_in.dτ, dual_in.dϖ, dual_in.dzw, dual_in.dZpp, dual_in.dZmp,
                                        dual_in.dalbedo, nn(dual_in.dRsurf), nn(dual_in.dalbedo_spec))
        MomCore.mom_rt_run_dual!(h.ptr)
        R = zeros(nV, pol.n, nSpec);  Tr = similar(R);  dR = zeros(nV, pol.n, nSpec, P);  dT = similar(dR)
        MomCore.mom_get_RT!(h.ptr, R, Tr)
        MomCore.mom_get_RT_partials!(h.ptr, dR, dT)
        hdr = similar(R);  uw = zeros(pol.n, nSpec);  dw = similar(uw)                     # the RAMI extras of rt_run.jl:91-94
        dhdr = similar(dR);  duw = zeros(pol.n, nSpec, P);  ddw = similar(duw)
        MomCore.mom_get_hdr!(h.ptr, hdr, uw, dw)
        MomCore.mom_get_hdr_partials!(h.ptr, dhdr, duw, ddw)
        mk(X, dX) = [D(X[i], ForwardDiff.Partials(ntuple(p -> dX[i, p], P))) for i in CartesianIndices(X)]
        Rd, Td = mk(R, dR), mk(Tr, dT)
        return Rd, Td, zero(Rd), zero(Rd), mk(hdr, dhdr), mk(uw, duw)[1, :], mk(dw, ddw)[1, :]   # the 7-tuple of rt_run.jl:226
    finally
        close(h)
    end
end

"""
The partials of a scene that came from mom_scene_set_optics, formed on the device from the partials of the INGREDIENTS (what the
Dual numbers carry into constructCoreOpticalProperties / createAero, compEffectiveLayerProperties.jl:1-85, and the `+` of
types.jl:632-678) instead of mom_scene_set_partials: w_abs [Nz, 3, P] = (∂p_z/∂x, ∂T_z/∂x, ∂ln(vcd vmr)_z/∂x) onto the resident
∂τ_abs / τ_abs tables of compute_absorption_profile!(...; dual = true), w_rayl [Nz, P] = the relative change of the layer's
Rayleigh depth (atmo_prof.jl:210-224), dτ_aer [nAer, Nz, P], dω̃, dfᵗ [nAer, P]; `nothing` = no dependence.  `surf`: the partials
of the bases and the surface as rt_run_dual passes them.  mom_rt_run_dual follows; neither ∂τ_abs nor dτ, dϖ, dzw cross the bus.
"""
function scene_set_optics_partials!(h::MomHandle, P; w_abs = nothing, w_rayl = nothing, dτ_aer = nothing, dω̃ = nothing, dfᵗ = nothing,
                                    surf = (dZpp = nothing, dZmp = nothing, dalbedo = nothing, dRsurf = nothing, dalbedo_spec = nothing))
    nn(x) = x === nothing ? C_NULL : collect(Float64, x)
    MomCore.mom_scene_set_optics_partials!(h.ptr, P, nn(w_abs), nn(w_rayl), nn(dτ_aer), nn(dω̃), nn(dfᵗ), nn(surf.dZpp), nn(surf.dZmp),
                                           nn(surf.dalbedo), nn(surf.dRsurf), nn(surf.dalbedo_spec))
end
# <<< rt_run_dual

# The architecture is a FIELD of model.params (vSmartMOM_Parameters), not a type parameter of vSmartMOM_Model
# (src/CoreRT/types.jl:483), so the two entry points of rt_run.jl:19-21,41-42 gain a run-time branch and the reference's
# own body moves, unchanged, into `rt_run_reference`:
function rt_run(model::vSmartMOM_Model; i_band::Integer = 1)
    rt_run(noRS(), model, i_band)
end
function rt_run(RS_type::AbstractRamanType, model::vSmartMOM_Model, iBand)
    arch = model.params.architecture
    return arch isa MI355X ? rt_run(RS_type, model, iBand, arch) : rt_run_reference(RS_type, model, iBand)
end
# <<< rt_run_noRS

# >>> rt_run_RRS
"""
rt_run(RS_type::RRS, model, iBand) on the MI355X (src/Inelastic/types.jl:13-33): the host side is the reference's own
(getRamanSSProp!, computeRamanZλ!, constructCoreOpticalProperties stay Julia), only the layer loop moves.
`rrs_strict_reference = true` executes the reference's RRS text as written (MOM_EUNSUPPORTED where the reference itself
raises); `false` applies the corrections D1..D5 of DESIGN.md section 7.
"""
function rt_run(RS_type::RRS, model::vSmartMOM_Model, iBand, arch::MI355X; rrs_strict_reference::Bool = true)
    pol, max_m = model.params.polarization_type, model.params.max_m
    qp_μ = model.quad_points.qp_μ
    h = momcore_scene_rrs(RS_type, model, iBand, arch, rrs_strict_reference)
    try
        nV, nSpec = length(model.obs_geom.vza), h.nSpec
        MomCore.mom_rt_run_rrs!(h.ptr)
        R, T, ieR, ieT = (zeros(nV, pol.n, nSpec) for _ in 1:4)
        MomCore.mom_get_RT_rrs!(h.ptr, R, T, ieR, ieT, C_NULL)
        hdr = zeros(nV, pol.n, nSpec);  bhr_uw = zeros(pol.n, nSpec);  bhr_dw = similar(bhr_uw)
        MomCore.mom_get_hdr_rrs!(h.ptr, hdr, bhr_uw, bhr_dw)
        return R, T, ieR, ieT, hdr, bhr_uw[1, :], bhr_dw[1, :]
    finally
        close(h)
    end
end

function momcore_scene_rrs(RS_type::RRS, model, iBand, arch::MI355X, strict::Bool; shard = nothing, z_moments_on_device::Bool = false)
    pol, max_m = model.params.polarization_type, model.params.max_m
    qp_μ = model.quad_points.qp_μ
    # the elastic scene exactly as for noRS (the Rayleigh ϖ is RS_type.ϖ_Cabannes, compEffectiveLayerProperties.jl:27);
    # the Raman layers are allocated for the unpadded operator edge
    h = momcore_scene(RS_type, model, iBand, arch; z_moments_on_device)
    MomCore.mom_set_option!(h.ptr, MomCore.MOM_OPT_STRIP_PAD, 0)
    MomCore.mom_rrs_set!(h.ptr, length(RS_type.i_λ₁λ₀), Cint.(RS_type.i_λ₁λ₀), RS_type.ϖ_λ₁λ₀, strict ? 1 : 0)
    if shard !== nothing            # (nSpec_global, wlo, lo, hi), 0-based owned slice [lo, hi) of the window starting at wlo
        nSpec_global, wlo, lo, hi = shard
        MomCore.mom_rrs_set_shard!(h.ptr, nSpec_global, wlo, lo - wlo, hi - wlo)
    end
    # fScattRayleigh [nSpec, Nz] (compEffectiveLayerProperties.jl:58, expandBandScalars :150-158) and the Raman phase
    # matrices of every Fourier moment (computeRamanZλ!, inelastic_helper.jl:457-464)
    fScattRayleigh = constructCoreOpticalProperties(RS_type, iBand, 0, model)[2]
    fsc  = reduce(hcat, [expandBandScalars(RS_type, f) for f in fScattRayleigh])
    if z_moments_on_device          # all moments in one mom_z_moments call: [N, N, 1, M]
        Zr4  = compute_Z_moments_batch(arch, pol, Array(qp_μ), [RS_type.greek_raman], max_m)
        Zrpp = Zr4[1][:, :, 1, :];  Zrmp = Zr4[2][:, :, 1, :]
    else
        Zr   = [Scattering.compute_Z_moments(pol, Array(qp_μ), RS_type.greek_raman, m) for m in 0:max_m-1]
        Zrpp = cat((z[1] for z in Zr)...; dims = 3);  Zrmp = cat((z[2] for z in Zr)...; dims = 3)
    end
    MomCore.mom_scene_set_rrs!(h.ptr, fsc, Zrpp, Zrmp)
    return h
end
# <<< rt_run_RRS

# >>> rt_run_ms
"""rt_run_test_ms(RS_type::noRS, sensor_levels, model, iBand) (rt_run_multisensor.jl:14-191): ONE call after the scene is resident."""
function rt_run_test_ms(RS_type::noRS, sensor_levels::Vector{Int64}, model::vSmartMOM_Model, iBand, arch::MI355X)
    h = momcore_scene(RS_type, model, iBand, arch)
    try
        nV, n, nSpec, ns = length(model.obs_geom.vza), model.params.polarization_type.n, h.nSpec, length(sensor_levels)
        uw = zeros(Float64, nV, n, nSpec, ns);  dw = similar(uw)
        MomCore.mom_rt_run_multisensor!(h.ptr, ns, Cint.(sensor_levels), uw, dw)
        uwJ = [uw[:, :, :, i] for i in 1:ns];  dwJ = [dw[:, :, :, i] for i in 1:ns]
        return uwJ, dwJ, zero.(uwJ), zero.(dwJ)          # (uwJ, dwJ, uwieJ, dwieJ), rt_run_multisensor.jl:190
    finally
        close(h)
    end
end
# <<< rt_run_ms

# >>> operators
# Alternative A: keep rt_run's loops in Julia and overload the operators one by one.  The layer state lives in the
# handle; AddedLayer / CompositeLayer become tags that carry it.
struct MomAddedLayer;     h::MomHandle; surface::Bool; end
struct MomCompositeLayer; h::MomHandle; end

# elemental!(pol_type, SFI, τ_sum, dτ, computed_layer_properties, m, ndoubl, scatter, quad_points, added_layer, architecture)
# -- elemental.jl:109-118
function elemental!(pol_type, SFI, τ_sum, dτ, computed_layer_properties, m, ndoubl, scatter, quad_points,
                    added_layer::MomAddedLayer, architecture::MI355X)
    @unpack ϖ, Z⁺⁺, Z⁻⁺ = computed_layer_properties
    MomCore.mom_elemental!(added_layer.h.ptr, m, ndoubl, τ_sum, dτ, ϖ, Z⁺⁺, Z⁻⁺, size(Z⁺⁺, 3))
end
# doubling!(pol_type, SFI, expk, ndoubl, added_layer, I_static, architecture) -- doubling.jl:81-86 (expk updated in place)
doubling!(pol_type, SFI, expk, ndoubl, added_layer::MomAddedLayer, I_static, architecture::MI355X) =
    MomCore.mom_doubling!(added_layer.h.ptr, ndoubl, expk)
# interaction!(RS_type::noRS, scattering_interface, SFI, composite_layer, added_layer, I_static) -- interaction_inelastic.jl:474-477
interaction!(RS_type::noRS, scattering_interface, SFI, composite_layer::MomCompositeLayer, added_layer::MomAddedLayer, I_static) =
    MomCore.mom_interaction!(composite_layer.h.ptr, iface_code(scattering_interface), added_layer.surface ? 1 : 0)
# rt_kernel.jl:227-230: composite_layer.X[:] = added_layer.x for the first layer
copy_added_to_composite!(composite_layer::MomCompositeLayer) = MomCore.mom_copy_added_to_composite!(composite_layer.h.ptr)
# create_surface_layer!(brdf::LambertianSurfaceScalar, added_layer, SFI, m, pol_type, quad_points, τ_sum, architecture)
# -- lambertian_surface.jl:20-27
create_surface_layer!(brdf::LambertianSurfaceScalar, added_layer::MomAddedLayer, SFI, m, pol_type, quad_points, τ_sum,
                      architecture::MI355X) =
    MomCore.mom_surface_lambertian!(added_layer.h.ptr, m, Float64(brdf.albedo), τ_sum)
# postprocessing_vza!(RS_type, iμ₀, pol_type, composite_layer, vza, qp_μ, m, vaz, μ₀, weight, nSpec, SFI, R, R_SFI, T, T_SFI,
#                     ieR_SFI, ieT_SFI) -- postprocessing_vza.jl:9-11 (accumulates in place)
function postprocessing_vza!(RS_type::noRS, iμ₀, pol_type, composite_layer::MomCompositeLayer, vza, qp_μ, m, vaz, μ₀, weight,
                             nSpec, SFI, R, R_SFI, T, T_SFI, ieR_SFI, ieT_SFI)
    node = Cint[nearest_point(qp_μ, cosd(v)) for v in vza]
    MomCore.mom_postprocess!(composite_layer.h.ptr, m, length(vza), node, Float64.(vaz), weight, R_SFI, T_SFI)
end
# batch_inv!(X, A) / A ⊠ B -- gpu_batched.jl:60,85,90-97
batch_inv!(h::MomHandle, X::Array{Float64,3}, A::Array{Float64,3}) = MomCore.mom_batch_inv!(h.ptr, size(A, 1), size(A, 3), A, X)
batched_mul!(h::MomHandle, C::Array{Float64,3}, A::Array{Float64,3}, B::Array{Float64,3}) =
    MomCore.mom_batched_mul!(h.ptr, size(A, 1), size(A, 3), A, B, C)
# Array(composite_layer.J₀⁻) (postprocessing_vza.jl:17-20) and friends
download!(dst::Array{Float64}, h::MomHandle, which::Integer) = MomCore.mom_download!(h.ptr, which, dst)
upload!(h::MomHandle, which::Integer, src::Array{Float64}) = MomCore.mom_upload!(h.ptr, which, src)
# <<< operators

# >>> multigpu
"""
One process per GPU (Julia Distributed / MPI.jl).  Rank r of G runs the binding on its slice of τ, ϖ, zw, τ_sum while
nd / ifaces stay the GLOBAL ones (get_dtau_ndoubl and extractEffectiveProps take maxima over the whole spectral axis),
then ONE RCCL all-gather of the spectra -- behind the C ABI, on the library's own stream.
"""
function momcore_comm_init!(h::MomHandle, r::Integer, G::Integer, bcast!)
    id = Vector{UInt8}(undef, MomCore.MOM_COMM_ID_BYTES)
    r == 0 && momcheck(MomCore.mom_comm_unique_id(id, length(id)))
    bcast!(id)                                                   # any host-side broadcast will do (MPI.Bcast!(id, 0, comm))
    MomCore.mom_comm_init!(h.ptr, r, G, id)
end
function momcore_allgather_RT(h::MomHandle, nV, nStokes, S_loc, G)
    R_SFI = zeros(nV, nStokes, G * S_loc);  T_SFI = similar(R_SFI)
    MomCore.mom_allgather_RT!(h.ptr, R_SFI, T_SFI)
    return R_SFI, T_SFI
end
# <<< multigpu

# >>> absorption
# HitranModel.broadening / HitranModel.CEF (src/Absorption/types.jl) -> the codes of mom_absorption_set_model.  Doppler and Lorentz
# ignore the CEF, as line_shape! does (compute_absorption_cross_section.jl:167-177); every other error function (CPF12, Erfc*) is
# outside the built scope and raises a MethodError here.
momcore_broadening(::Voigt) = MomCore.MOM_BROADENING_VOIGT
momcore_broadening(::Doppler) = MomCore.MOM_BROADENING_DOPPLER
momcore_broadening(::Lorentz) = MomCore.MOM_BROADENING_LORENTZ
momcore_cef(::HumlicekWeidemann32SDErrorFunction) = MomCore.MOM_CEF_HW32SD
momcore_cef(::HumlicekWeidemann32VoigtErrorFunction) = MomCore.MOM_CEF_HW32VOIGT

"""
compute_absorption_profile! (src/CoreRT/tools/atmo_prof.jl:427-449) for a HitranModel (`broadening`, `CEF`: its fields; default Voigt with
HumlicekWeidemann32SDErrorFunction, as parameters_from_yaml.jl:114-115): one
resident line table per absorber, then all layers of the profile in two launches (the reference: a loop over layers
with one kernel launch per line, compute_absorption_cross_section.jl:118-124).  `dual = true`: the same two launches on
ForwardDiff.Dual numbers -- the partials of τ_abs with respect to each layer's pressure and temperature accumulate in the
resident ∂τ_abs table (absorption_partials).
"""
function compute_absorption_profile!(h::MomHandle, grid, hitran, tips, p_full, T, vmr, vcd_dry, wing_cutoff; dual::Bool = false,
                                     broadening = Voigt(), CEF = HumlicekWeidemann32SDErrorFunction())
    Nz = length(p_full)
    broadening isa Voigt || (CEF = HumlicekWeidemann32SDErrorFunction())      # ignored by Doppler and Lorentz
    MomCore.mom_absorption_set_model!(h.ptr, momcore_broadening(broadening), momcore_cef(CEF))
    MomCore.mom_absorption_begin!(h.ptr, Nz, collect(Float64, grid))
    keep = (minimum(grid) - wing_cutoff) .< hitran.νᵢ .< (maximum(grid) + wing_cutoff)      # compute_absorption_cross_section.jl:54-72
    MomCore.mom_absorption_set_lines!(h.ptr, count(keep), hitran.νᵢ[keep], hitran.Sᵢ[keep], hitran.γ_air[keep], hitran.γ_self[keep],
                                      hitran.E″[keep], hitran.n_air[keep], hitran.δ_air[keep], tips.sqrt_mol_weight[keep],
                                      tips.iso_index[keep], tips.nIso, tips.nTmax, tips.nT, tips.T, tips.Q, tips.z)
    ms = Ref{Cdouble}(0)
    if dual
        MomCore.mom_voigt_tau_abs_profile_dual!(h.ptr, Nz, p_full, T, Float64(vmr), Float64(wing_cutoff), vcd_dry .* vmr, ms)
    else
        MomCore.mom_voigt_tau_abs_profile!(h.ptr, Nz, p_full, T, Float64(vmr), Float64(wing_cutoff), vcd_dry .* vmr, ms)
    end
    return ms[]      # τ_abs stays resident; mom_scene_set_optics assembles the layer optics from it
end

"""∂τ_abs [nSpec, Nz, 2] of the Dual calls since mom_absorption_begin: [:, :, 1] with respect to the layer's pressure, [:, :, 2] to its temperature."""
function absorption_partials(h::MomHandle, nSpec, Nz)
    dτ_abs = zeros(Float64, nSpec, Nz, 2)
    MomCore.mom_absorption_get_partials!(h.ptr, dτ_abs)
    return dτ_abs
end

"""compute_absorption_cross_section(model::HitranModel, grid, p, T) with architecture isa MI355X: ONE call for all lines."""
function voigt_xsec(arch::MI355X, ν, γ_d, y, S, ind_start, ind_stop, grid)
    result = zeros(Float64, length(grid))
    momcheck(MomCore.mom_voigt_xsec(arch.device, length(ν), ν, γ_d, y, S, Cint.(ind_start), Cint.(ind_stop), length(grid),
                                    collect(Float64, grid), result))
    return result
end

"""
absorption_cross_section(model, grid, p, T; autodiff = true) (src/Absorption/autodiff_helper.jl:17-51) with architecture isa
MI355X: (σ, J[nGrid, 2]) from ONE call.  dν, dγ_d, dy, dS: the partials of the prefactors with respect to [p, T], each
[nLines, 2] (what ForwardDiff carries through compute_absorption_cross_section.jl:79-101).
"""
function voigt_xsec_dual(arch::MI355X, ν, γ_d, y, S, dν, dγ_d, dy, dS, ind_start, ind_stop, grid)
    result = zeros(Float64, length(grid));  derivs = zeros(Float64, length(grid), 2)
    momcheck(MomCore.mom_voigt_xsec_dual(arch.device, length(ν), ν, γ_d, y, S, collect(Float64, dν), collect(Float64, dγ_d),
                                         collect(Float64, dy), collect(Float64, dS), Cint.(ind_start), Cint.(ind_stop), length(grid),
                                         collect(Float64, grid), result, derivs))
    return result, derivs
end

"""
line_shape!(A, grid, ν, γ_d, γ_l, y, S, broadening, CEF) (compute_absorption_cross_section.jl:167-183) summed over all lines in ONE
call: voigt_xsec for any built absorption model.  An array the broadening does not read may be `C_NULL`.
"""
function lineshape_xsec(arch::MI355X, broadening, CEF, ν, γ_d, γ_l, y, S, ind_start, ind_stop, grid)
    result = zeros(Float64, length(grid))
    cef = broadening isa Voigt ? momcore_cef(CEF) : MomCore.MOM_CEF_HW32SD
    momcheck(MomCore.mom_lineshape_xsec(arch.device, momcore_broadening(broadening), cef, length(ν), ν, γ_d, γ_l, y, S, Cint.(ind_start),
                                        Cint.(ind_stop), length(grid), collect(Float64, grid), result))
    return result
end

"""Its Dual run: (σ, J[nGrid, 2]); dν, dγ_d, dγ_l, dy, dS as for voigt_xsec_dual."""
function lineshape_xsec_dual(arch::MI355X, broadening, CEF, ν, γ_d, γ_l, y, S, dν, dγ_d, dγ_l, dy, dS, ind_start, ind_stop, grid)
    result = zeros(Float64, length(grid));  derivs = zeros(Float64, length(grid), 2)
    cef = broadening isa Voigt ? momcore_cef(CEF) : MomCore.MOM_CEF_HW32SD
    momcheck(MomCore.mom_lineshape_xsec_dual(arch.device, momcore_broadening(broadening), cef, length(ν), ν, γ_d, γ_l, y, S,
                                             collect(Float64, dν), collect(Float64, dγ_d), collect(Float64, dγ_l), collect(Float64, dy),
                                             collect(Float64, dS), Cint.(ind_start), Cint.(ind_stop), length(grid),
                                             collect(Float64, grid), result, derivs))
    return result, derivs
end
# <<< absorption

# >>> interpolation
"""
The InterpolationModel on a handle (src/Absorption/types.jl; make_model_helpers.jl:55-99): `id` names the table of cubic B-spline
coefficients resident on the device, the three grids are the model's ranges.
"""
struct MomInterpolationModel
    h::MomHandle
    id::Cint
    mol::Int
    iso::Int
    ν_grid::AbstractRange
    p_grid::AbstractRange
    t_grid::AbstractRange
end

function lut_create(h::MomHandle, ν_grid::AbstractRange, p_grid::AbstractRange, t_grid::AbstractRange)
    id = Ref{Cint}(-1)
    MomCore.mom_lut_create!(h.ptr, length(ν_grid), Float64(first(ν_grid)), Float64(step(ν_grid)), length(p_grid), Float64(first(p_grid)),
                            Float64(step(p_grid)), length(t_grid), Float64(first(t_grid)), Float64(step(t_grid)), id)
    return id[]
end

"""
make_interpolation_model(hitran, broadening, ν_grid, p_grid, t_grid; wing_cutoff, vmr, CEF) with architecture isa MI355X: the loop
over the (p, T) nodes (make_model_helpers.jl:82-88) and `interpolate(cs_matrix, BSpline(Cubic(Line(OnGrid()))))` (:91) run on the
device from the resident line table; only the line table crosses the bus.
"""
function make_interpolation_model(h::MomHandle, hitran, tips, broadening, ν_grid::AbstractRange, p_grid::AbstractRange,
                                  t_grid::AbstractRange; wing_cutoff = 40, vmr = 0, CEF = HumlicekWeidemann32SDErrorFunction())
    broadening isa Voigt || (CEF = HumlicekWeidemann32SDErrorFunction())
    MomCore.mom_absorption_set_model!(h.ptr, momcore_broadening(broadening), momcore_cef(CEF))
    keep = (first(ν_grid) - wing_cutoff) .< hitran.νᵢ .< (last(ν_grid) + wing_cutoff)
    MomCore.mom_absorption_set_lines!(h.ptr, count(keep), hitran.νᵢ[keep], hitran.Sᵢ[keep], hitran.γ_air[keep], hitran.γ_self[keep],
                                      hitran.E″[keep], hitran.n_air[keep], hitran.δ_air[keep], tips.sqrt_mol_weight[keep],
                                      tips.iso_index[keep], tips.nIso, tips.nTmax, tips.nT, tips.T, tips.Q, tips.z)
    id = lut_create(h, ν_grid, p_grid, t_grid)
    MomCore.mom_lut_build!(h.ptr, id, Float64(vmr), Float64(wing_cutoff), C_NULL)
    iso = all(x -> x == hitran.iso[1], hitran.iso) ? hitran.iso[1] : -1
    return MomInterpolationModel(h, id, hitran.mol[1], iso, ν_grid, p_grid, t_grid)
end

"""An InterpolationModel of a finished cs_matrix [nν, np, nT] (loaded from disk, or derived from ABSCO on the host)."""
function interpolation_model_from_table(h::MomHandle, cs_matrix::Array{Float64,3}, ν_grid, p_grid, t_grid, mol, iso)
    id = lut_create(h, ν_grid, p_grid, t_grid)
    MomCore.mom_lut_set_table!(h.ptr, id, cs_matrix)
    return MomInterpolationModel(h, id, mol, iso, ν_grid, p_grid, t_grid)
end

"""compute_absorption_cross_section(model::InterpolationModel, grid, p, T) (compute_absorption_cross_section.jl:139-159)."""
function compute_absorption_cross_section(model::MomInterpolationModel, grid, pressure::Real, temperature::Real)
    ν = collect(Float64, grid);  σ = zeros(Float64, length(ν))
    MomCore.mom_lut_xsec!(model.h.ptr, model.id, length(ν), ν, Float64(pressure), Float64(temperature), σ, C_NULL)
    return σ
end

"""absorption_cross_section(model, grid, p, T; autodiff = true) (autodiff_helper.jl:17-51): (σ, J[nGrid, 2])."""
function absorption_cross_section_dual(model::MomInterpolationModel, grid, pressure::Real, temperature::Real)
    ν = collect(Float64, grid);  σ = zeros(Float64, length(ν));  J = zeros(Float64, length(ν), 2)
    MomCore.mom_lut_xsec!(model.h.ptr, model.id, length(ν), ν, Float64(pressure), Float64(temperature), σ, J)
    return σ, J
end

"""
compute_absorption_profile! (atmo_prof.jl:427-449) for an InterpolationModel: τ_abs[:, iz] += σ(grid; p[iz], T[iz]) vcd_dry[iz] vmr for
all layers in one launch, on the grid of mom_absorption_begin (`begin_table = false` adds another absorber to the same table).
"""
function compute_absorption_profile!(h::MomHandle, grid, model::MomInterpolationModel, p_full, T, vmr, vcd_dry; dual::Bool = false,
                                     begin_table::Bool = true)
    Nz = length(p_full)
    begin_table && MomCore.mom_absorption_begin!(h.ptr, Nz, collect(Float64, grid))
    ms = Ref{Cdouble}(0)
    if dual
        MomCore.mom_lut_tau_abs_profile_dual!(h.ptr, model.id, Nz, p_full, T, vcd_dry .* vmr, ms)
    else
        MomCore.mom_lut_tau_abs_profile!(h.ptr, model.id, Nz, p_full, T, vcd_dry .* vmr, ms)
    end
    return ms[]
end

destroy!(model::MomInterpolationModel) = MomCore.mom_lut_destroy!(model.h.ptr, model.id)
# <<< interpolation

# >>> mie
"""
compute_aerosol_optical_properties(model::MieModel{<:NAI2}) (src/Scattering/compute_NAI2.jl:16-182) with architecture isa MI355X:
the loop over the radii (:80-112), the bulk sums (:115-123) and the projections (:146-160) are ONE call.  The host keeps what it
already builds -- the radius quadrature, wₓ, μ, w_μ, the π/τ and P/P²/R²/T² tables (column-major [n_μ, n], the layout the ABI reads) --
and the division by the bulk C_sca.  `w_rows` [nR, nW]: column 1 = wₓ, further columns ∂wₓ/∂θ of size-distribution parameters; the
result carries one AerosolOptics-like named tuple per column, the partial ones through the quotient rule.
"""
function mie_nai2(arch::MI355X, r, w_rows, λ, nᵣ, nᵢ, w_μ, leg_π, leg_τ, P, P², R², T²)
    nR, nW = size(w_rows, 1), size(w_rows, 2);  n_μ, n_max = size(leg_π);  l_max = size(P, 2)
    w = collect(Float64, (4π .* r .^ 2) .* w_rows)                       # [nR, nW] column-major = the ABI's [nW, nR] rows
    bulk_f = zeros(Float64, n_μ, 4, nW);  C = zeros(Float64, 2, nW);  greek = zeros(Float64, l_max, 6, nW);  ms = zeros(Float64, 3)
    momcheck(MomCore.mom_mie_nai2(arch.device, nR, collect(Float64, r), nW, w, Float64(λ), Float64(nᵣ), Float64(nᵢ), n_μ,
                                  collect(Float64, w_μ), n_max, collect(Float64, leg_π), collect(Float64, leg_τ), l_max,
                                  collect(Float64, P), collect(Float64, P²), collect(Float64, R²), collect(Float64, T²), 0, bulk_f, C,
                                  greek, ms))
    C_sca, C_ext = C[1, 1], C[2, 1]
    value = (α = greek[:, 1, 1] ./ C_sca, β = greek[:, 2, 1] ./ C_sca, γ = greek[:, 3, 1] ./ C_sca, δ = greek[:, 4, 1] ./ C_sca,
             ϵ = greek[:, 5, 1] ./ C_sca, ζ = greek[:, 6, 1] ./ C_sca, ω̃ = C_sca / C_ext, k = C_ext, fᵗ = 1.0)
    partials = map(2:nW) do j
        d(q) = greek[:, q, j] ./ C_sca .- greek[:, q, 1] .* (C[1, j] / C_sca^2)
        (α = d(1), β = d(2), γ = d(3), δ = d(4), ϵ = d(5), ζ = d(6), ω̃ = C[1, j] / C_ext - C_sca * C[2, j] / C_ext^2, k = C[2, j], fᵗ = 0.0)
    end
    return value, partials, ms
end

"""
compute_aerosol_optical_properties(model; autodiff = true) (src/Scattering/phase_function_autodiff.jl:41-95) with the columns nᵣ and nᵢ
of x = (r_m, σ_g, nᵣ, nᵢ): the same call with the Dual run of the Mie coefficients.  `w_rows` has at most 3 columns (wₓ, ∂wₓ/∂r_m,
∂wₓ/∂σ_g); the device appends two rows, ∂/∂nᵣ and ∂/∂nᵢ of column 1's sums, so `partials` holds nW - 1 + 2 named tuples in the
reference's order of x.
"""
function mie_nai2_dual(arch::MI355X, r, w_rows, λ, nᵣ, nᵢ, w_μ, leg_π, leg_τ, P, P², R², T²)
    nR, nW = size(w_rows, 1), size(w_rows, 2);  n_μ, n_max = size(leg_π);  l_max = size(P, 2);  nO = nW + Int(MomCore.MOM_MIE_INDEX_ROWS)
    w = collect(Float64, (4π .* r .^ 2) .* w_rows)
    bulk_f = zeros(Float64, n_μ, 4, nO);  C = zeros(Float64, 2, nO);  greek = zeros(Float64, l_max, 6, nO);  ms = zeros(Float64, 3)
    momcheck(MomCore.mom_mie_nai2_dual(arch.device, nR, collect(Float64, r), nW, w, Float64(λ), Float64(nᵣ), Float64(nᵢ), n_μ,
                                       collect(Float64, w_μ), n_max, collect(Float64, leg_π), collect(Float64, leg_τ), l_max,
                                       collect(Float64, P), collect(Float64, P²), collect(Float64, R²), collect(Float64, T²), 0, bulk_f, C,
                                       greek, ms))
    C_sca, C_ext = C[1, 1], C[2, 1]
    value = (α = greek[:, 1, 1] ./ C_sca, β = greek[:, 2, 1] ./ C_sca, γ = greek[:, 3, 1] ./ C_sca, δ = greek[:, 4, 1] ./ C_sca,
             ϵ = greek[:, 5, 1] ./ C_sca, ζ = greek[:, 6, 1] ./ C_sca, ω̃ = C_sca / C_ext, k = C_ext, fᵗ = 1.0)
    partials = map(2:nO) do j
        d(q) = greek[:, q, j] ./ C_sca .- greek[:, q, 1] .* (C[1, j] / C_sca^2)
        (α = d(1), β = d(2), γ = d(3), δ = d(4), ϵ = d(5), ζ = d(6), ω̃ = C[1, j] / C_ext - C_sca * C[2, j] / C_ext^2, k = C[2, j], fᵗ = 0.0)
    end
    return value, partials, ms
end

"""
A batch of wavelengths `λ` [nL], each with its own refractive index `nᵣ`, `nᵢ` [nL], in ONE call: radii and weight rows are shared,
and so is one angle grid `μ`, `w_μ` (sized by the caller for the shortest wavelength, `n_max` = its largest per-radius n_max).  The
π/τ and P/P²/R²/T² tables are built on the device from `μ`; the host brings none.  Returns (bulk_f [n_μ, 4, nW, nL], C [2, nW, nL],
greek [l_max, 6, nW, nL], ms [4]), unnormalised as the device returns them: the division by C_sca is that of `mie_nai2`, per wavelength.
"""
function mie_nai2_spectral(arch::MI355X, r, w_rows, λ, nᵣ, nᵢ, μ, w_μ, n_max, l_max; max_batch = 0)
    nR, nW, nL, n_μ = size(w_rows, 1), size(w_rows, 2), length(λ), length(μ)
    w = collect(Float64, (4π .* r .^ 2) .* w_rows)
    bulk_f = zeros(Float64, n_μ, 4, nW, nL);  C = zeros(Float64, 2, nW, nL);  greek = zeros(Float64, l_max, 6, nW, nL);  ms = zeros(Float64, 4)
    momcheck(MomCore.mom_mie_nai2_spectral(arch.device, nR, collect(Float64, r), nW, w, nL, collect(Float64, λ), collect(Float64, nᵣ),
                                           collect(Float64, nᵢ), n_μ, collect(Float64, μ), collect(Float64, w_μ), n_max, l_max, 0,
                                           max_batch, bulk_f, C, greek, ms))
    return bulk_f, C, greek, ms
end

"""
The Dual run of `mie_nai2_spectral` (at most 3 columns of `w_rows`): nW + 2 rows per wavelength, the last two ∂/∂nᵣ and ∂/∂nᵢ of
column 1's sums, as `mie_nai2_dual` has them.
"""
function mie_nai2_spectral_dual(arch::MI355X, r, w_rows, λ, nᵣ, nᵢ, μ, w_μ, n_max, l_max; max_batch = 0)
    nR, nW, nL, n_μ = size(w_rows, 1), size(w_rows, 2), length(λ), length(μ);  nO = nW + Int(MomCore.MOM_MIE_INDEX_ROWS)
    w = collect(Float64, (4π .* r .^ 2) .* w_rows)
    bulk_f = zeros(Float64, n_μ, 4, nO, nL);  C = zeros(Float64, 2, nO, nL);  greek = zeros(Float64, l_max, 6, nO, nL);  ms = zeros(Float64, 4)
    momcheck(MomCore.mom_mie_nai2_spectral_dual(arch.device, nR, collect(Float64, r), nW, w, nL, collect(Float64, λ), collect(Float64, nᵣ),
                                                collect(Float64, nᵢ), n_μ, collect(Float64, μ), collect(Float64, w_μ), n_max, l_max, 0,
                                                max_batch, bulk_f, C, greek, ms))
    return bulk_f, C, greek, ms
end
"""
compute_aerosol_optical_properties(model::MieModel{<:PCW}) (src/Scattering/compute_PCW.jl:16-104) with architecture isa MI355X: the
Mie coefficients, the pair averages of compute_avg_anbns!, the Wigner 3j symbols and the sums S_l of eq. 22 are ONE call.  The device
produces the symbols in registers, so `model.wigner_A` / `model.wigner_B` are not read and need not be loaded.  The host keeps the
radius quadrature and `wₓ` [nR] (the weights themselves, not times 4π r²), N_max = get_n_max(2π r_max / λ), and the (1 / C_sca).
"""
function mie_pcw(arch::MI355X, r, wₓ, λ, nᵣ, nᵢ, N_max)
    nR = length(r);  L = 2N_max - 1
    greek = zeros(Float64, L, 6);  C = zeros(Float64, 2);  ms = zeros(Float64, 3)
    momcheck(MomCore.mom_mie_pcw(arch.device, nR, collect(Float64, r), collect(Float64, wₓ), Float64(λ), Float64(nᵣ), Float64(nᵢ), N_max, 0,
                                 greek, C, ms))
    C_sca, C_ext = C[1], C[2]
    value = (α = (1 / C_sca) .* greek[:, 1], β = (1 / C_sca) .* greek[:, 2], γ = (1 / C_sca) .* greek[:, 3], δ = (1 / C_sca) .* greek[:, 4],
             ϵ = (1 / C_sca) .* greek[:, 5], ζ = (1 / C_sca) .* greek[:, 6], ω̃ = C_sca / C_ext, k = C_ext, fᵗ = 1.0)
    return value, ms
end

"""
compute_wigner_values(m_max, n_max, l_max) (src/Scattering/compute_wigner_values.jl:190-210) on the device: wigner_A and wigner_B
[m_max, n_max, l_max], column-major as the ABI writes them.  A PCW run on the device needs neither.
"""
function compute_wigner_values(arch::MI355X, m_max, n_max, l_max)
    A = zeros(Float64, m_max, n_max, l_max);  B = zeros(Float64, m_max, n_max, l_max)
    momcheck(MomCore.mom_wigner_tables(arch.device, m_max, n_max, l_max, A, B))
    return A, B
end
# <<< mie

# >>> z_moments
"""
Scattering.compute_Z_moments(pol, μ, greek_coefs, m) (compute_Z_matrices.jl:5-84) for every set of `greeks` and the moments
m_first : m_first + M - 1 in ONE device call: Z⁺⁺ and Z⁻⁺ as [N, N, nG, M], column-major as the ABI writes them, which is what
mom_scene_set! takes as Zpp / Zmp with K = nG.  The sets may differ in length (Rayleigh has 3 coefficients, an aerosol l_max).
`set_inner = K` with nG = K P sets ordered k fastest (the derivative sets of P parameters): [N, N, K, M, P], the dZpp / dZmp of
mom_scene_set_partials!.  Off by default wherever the host layer forms Z: the keyword `z_moments_on_device` of its callers.
"""
function compute_Z_moments_batch(arch::MI355X, pol, μ, greeks, M; m_first = 0, set_inner = 0)
    nG = length(greeks);  n_μ = length(μ);  N = pol.n * n_μ
    l_max = Cint[length(g.β) for g in greeks];  l_pad = Int(maximum(l_max))
    greek = zeros(Float64, l_pad, 6, nG)
    for (k, g) in enumerate(greeks), (q, row) in enumerate((g.α, g.β, g.γ, g.δ, g.ϵ, g.ζ))
        greek[1:l_max[k], q, k] .= row
    end
    K = set_inner == 0 ? nG : set_inner
    dims = set_inner == 0 ? (N, N, nG, M) : (N, N, K, M, nG ÷ K)
    Zpp = zeros(Float64, dims);  Zmp = zeros(Float64, dims);  ms = zeros(Float64, 1)
    momcheck(MomCore.mom_z_moments(arch.device, pol.n, n_μ, collect(Float64, μ), nG, l_pad, l_max, greek, m_first, M, set_inner,
                                   Zpp, Zmp, ms))
    return Zpp, Zmp, ms[1]
end

"""The Z⁺⁺ / Z⁻⁺ bases of a scene, [N, N, K, M] with basis 1 = Rayleigh and then the aerosols of `aerosol_optics`: the host loop over
(m, Greek set) of Scattering.compute_Z_moments, or with `z_moments_on_device` one compute_Z_moments_batch call."""
function z_bases(arch::MI355X, pol, μ, greek_rayleigh, aerosol_optics, max_m; z_moments_on_device::Bool = false)
    greeks = vcat([greek_rayleigh], [a.greek_coefs for a in aerosol_optics])
    if z_moments_on_device
        Zpp, Zmp, _ = compute_Z_moments_batch(arch, pol, μ, greeks, max_m)
        return Zpp, Zmp
    end
    Z = [Scattering.compute_Z_moments(pol, Array(μ), g, m) for g in greeks, m in 0:max_m-1]
    N = pol.n * length(μ)
    Zpp = zeros(Float64, N, N, length(greeks), max_m);  Zmp = zeros(Float64, N, N, length(greeks), max_m)
    for k in 1:length(greeks), m in 1:max_m
        Zpp[:, :, k, m] .= Z[k, m][1];  Zmp[:, :, k, m] .= Z[k, m][2]
    end
    return Zpp, Zmp
end
# <<< z_moments

# >>> truncate
"""
Scattering.truncate_phase(mod::δBGE, aero) (truncate_phase.jl:95-220) for every AerosolOptics of `optics` (one l_max for all) in
ONE device call, with the forward-mode partials of the function along `partials[k]` (AerosolOptics holding ∂aero/∂θ, the same
number per set; `nothing`: values only).  The nodes are gausslegendre(l_max) as in the reference; ω̃ and k pass through on the host,
fᵗ = 1 - c₀ and ∂fᵗ = -∂c₀.  Returns the truncated sets and, per set, its partials.  `mod.l_max` above 128 is not built
(MOM_EUNSUPPORTED): keep the host function there.  A set whose fits are singular is named by the error (MOM_ESINGULAR).
"""
function truncate_phase_batch(arch::MI355X, mod::δBGE, optics, partials = nothing)
    nG = length(optics);  nP = partials === nothing ? 0 : length(partials[1])
    l_full = length(optics[1].greek_coefs.β);  l_tr = mod.l_max
    μ, w_μ = gausslegendre(l_full)
    greek = zeros(Float64, l_full, 6, 1 + nP, nG)
    for k in 1:nG, (r, a) in enumerate(vcat([optics[k]], nP == 0 ? [] : partials[k]))
        g = a.greek_coefs
        for (q, row) in enumerate((g.α, g.β, g.γ, g.δ, g.ϵ, g.ζ))
            greek[:, q, r, k] .= row
        end
    end
    greek_t = zeros(Float64, l_tr, 6, 1 + nP, nG);  c₀ = zeros(Float64, 1 + nP, nG)
    status = zeros(Cint, nG);  ms = zeros(Float64, 1)
    momcheck(MomCore.mom_truncate_phase(arch.device, l_full, collect(Float64, μ), collect(Float64, w_μ), nG, nP, l_full, l_tr, greek,
                                        greek_t, c₀, status, ms))
    coefs(r, k) = GreekCoefs((greek_t[:, q, r, k] for q in 1:6)...)
    out = [AerosolOptics(greek_coefs = coefs(1, k), ω̃ = optics[k].ω̃, k = optics[k].k, fᵗ = 1 - c₀[1, k]) for k in 1:nG]
    d_out = [[AerosolOptics(greek_coefs = coefs(1 + j, k), ω̃ = partials[k][j].ω̃, k = partials[k][j].k, fᵗ = -c₀[1 + j, k])
              for j in 1:nP] for k in 1:nG]
    return out, d_out
end
# <<< truncate

# >>> z_resident
"""
Scenes from Greek coefficients: the staged call sequence.  The Greek sets of the K bases (Rayleigh, then the aerosols) go to the
handle, which copies them; the setter that follows is called with Zpp = Zmp = C_NULL and forms the bases in its own memory with the
kernels of mom_z_moments -- padded to the kernels' edge, cut to the (I,Q) sub-problem where moment 0 decouples, the decoupling test
made on the device.  No N × N matrix is built on the host or crosses the bus.  `which = 1` stages the one Raman set that
mom_scene_set_rrs!(h, fscatt, C_NULL, C_NULL) takes.  The keyword `z_resident` of momcore_scene selects the sequence.
"""
function stage_greeks!(h::MomHandle, greeks, M; which = 0)
    nG = length(greeks)
    l_max = Cint[length(g.β) for g in greeks];  l_pad = Int(maximum(l_max))
    greek = zeros(Float64, l_pad, 6, nG)
    for (k, g) in enumerate(greeks), (q, row) in enumerate((g.α, g.β, g.γ, g.δ, g.ϵ, g.ζ))
        greek[1:l_max[k], q, k] .= row
    end
    MomCore.mom_scene_stage_greeks!(h.ptr, which, nG, l_pad, l_max, greek, M)
end

"""Derivative sets for the Dual run: `pairs` = [((k, p), dgreek), ...], 0-based basis k and parameter p < P; the partial setter that
follows is called with dZpp = dZmp = C_NULL."""
function stage_greek_partials!(h::MomHandle, P, pairs)
    nD = length(pairs)
    l_max = Cint[length(g.β) for (_, g) in pairs];  l_pad = Int(maximum(l_max))
    dgreek = zeros(Float64, l_pad, 6, nD)
    for (d, (_, g)) in enumerate(pairs), (q, row) in enumerate((g.α, g.β, g.γ, g.δ, g.ϵ, g.ζ))
        dgreek[1:l_max[d], q, d] .= row
    end
    MomCore.mom_scene_stage_greek_partials!(h.ptr, P, nD, Cint[kp[1] for (kp, _) in pairs], Cint[kp[2] for (kp, _) in pairs], l_pad,
                                            l_max, dgreek)
end

scene_greeks(model, iBand) = vcat([model.greek_rayleigh], [a.greek_coefs for a in model.aerosol_optics[iBand[1]]])
# <<< z_resident
