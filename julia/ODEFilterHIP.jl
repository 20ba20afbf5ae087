# ODEFilterHIP.jl -- the `ccall` binding a ProbNumDiffEq maintainer would add so that
#
#     solve(EnsembleProblem(prob; ...), EK1(order=3), EnsembleHIP(); trajectories=N, dt=..., adaptive=false)
#
# runs the Kalman predict/update/smooth hot path on an MI355X through libodefilter_hip.so
# (C ABI: include/odefilter.h).  NOT EXECUTED in the build image (no Julia toolchain there);
# it mirrors, call for call, what odefilters.jl_amd/host.py does over ctypes, which IS tested.
module ODEFilterHIP

using ProbNumDiffEq            # EK0, EK1 (src/algorithms.jl:23-51), IEKS (src/ieks.jl)
import DiffEqBase
using LinearAlgebra: Diagonal  # sol.diffusions of the MV models

const LIB = get(ENV, "ODEFILTER_HIP_LIB", "libodefilter_hip.so")

# ---- mirrors of the C structs -------------------------------------------------------------
struct OdefConfig                      # odef_config, 56 bytes
    struct_size::Int32; alg::Int32; order::Int32; diffusion::Int32; smooth::Int32
    rhs_id::Int32; d::Int32; n_params::Int32; params_shared::Int32; save_mode::Int32
    device::Int32; want_loglik::Int32; n_traj::Int64
end

const RHS_IDS = Dict(:fhn => 0, :lorenz63 => 1, :lotka_volterra => 2, :vanderpol => 3, :linear => 4, :pleiades => 5, :lorenz96 => 6,
                     :forced => 7)  # :forced is time-dependent, f(u, p, t)
# src/caches.jl:89-96; the MV models (diagonal diffusion, EK0 only, the lane kernels: d(q+1) <= 20) keep d diffusions per save
const DIFFUSIONS = Dict(:dynamic => 0, :fixed => 1, :fixedMAP => 2, :dynamicMV => 3, :fixedMV => 4)
const MV_DIFFUSIONS = (:dynamicMV, :fixedMV)
const F_MEAN, F_COV_TRIL, F_DIFFUSION, F_T, F_LOGLIK, F_NACCEPT, F_NREJECT, F_NF, F_NJAC, F_NSAVED,
      F_RETCODE, F_SMOOTH_MEAN, F_SMOOTH_COV_TRIL = 0:12
const F_SAMPLES = 16
# IEKS (src/ieks.jl): the algorithm id and the field of linearisation points [n_save][d][N] (include/odefilter.h)
const ODEF_IEKS = 2
const F_LINEARIZE_AT = 17
# ensemble summary per time (odef_summary_field, include/odefilter.h): id = S_BASE + 8 * source + quantity, source 0 filter /
# 1 smoothed / 2 dense records, quantity 0 COUNT / 1 MEAN / 2 COV_WITHIN / 3 COV_BETWEEN.  UNTESTED like the rest of this file.
const S_BASE = 64
const S_FILTER_COUNT = 64
const S_FILTER_MEAN = 65
const S_FILTER_COV_WITHIN = 66
const S_FILTER_COV_BETWEEN = 67
const S_SMOOTH_COUNT = 72
const S_SMOOTH_MEAN = 73
const S_SMOOTH_COV_WITHIN = 74
const S_SMOOTH_COV_BETWEEN = 75
const S_DENSE_COUNT = 80
const S_DENSE_MEAN = 81
const S_DENSE_COV_WITHIN = 82
const S_DENSE_COV_BETWEEN = 83
# solution errors per trajectory (odef_errors_field, include/odefilter.h): id = E_BASE + 8 * source + quantity, source 0 filter /
# 1 smoothed records, quantity 0 FINAL / 1 L2 / 2 LINF / 3 CHI2 / 4 NUSED / 5 U_ANALYTIC; E_REFERENCE is the bindable truth
# [n_save][d][N] (odef_bind_device).  UNTESTED like the rest of this file.
const E_BASE = 128
const E_FINAL = 128
const E_L2 = 129
const E_LINF = 130
const E_CHI2 = 131
const E_NUSED = 132
const E_U_ANALYTIC = 133
const E_SMOOTH_FINAL = 136
const E_SMOOTH_L2 = 137
const E_SMOOTH_LINF = 138
const E_SMOOTH_CHI2 = 139
const E_SMOOTH_NUSED = 140
const E_SMOOTH_U_ANALYTIC = 141
const E_REFERENCE = 144
# data log-likelihood of noisy observations per trajectory (odef_data_field, include/odefilter.h): two outputs [N], four inputs
# that odef_bind_device alone takes.  UNTESTED like the rest of this file.
const L_BASE = 192
const L_DATA_LOGLIK = 192
const L_DATA_MAHALANOBIS = 193
const L_OBS_SAVE = 200
const L_OBS_COMPONENT = 201
const L_OBS_VALUE = 202
const L_OBS_NOISE = 203
const L_OBS_TIME = 204
# event location per trajectory (odef_event_field, include/odefilter.h): id = EV_BASE + 8 * source + quantity, two inputs that
# odef_bind_device alone takes.  UNTESTED like the rest of this file.
const EV_BASE = 256
const EV_COUNT = 256
const EV_TIME = 257
const EV_TIME_VAR = 258
const EV_U = 259
const EV_DIRECTION = 260
const EV_SAVE = 261
const EV_NEVAL = 262
const EV_SMOOTH_COUNT = 264
const EV_SMOOTH_TIME = 265
const EV_SMOOTH_TIME_VAR = 266
const EV_SMOOTH_U = 267
const EV_SMOOTH_DIRECTION = 268
const EV_SMOOTH_SAVE = 269
const EV_SMOOTH_NEVAL = 270
const EV_SPEC = 280
const EV_LEVEL = 281
# ensemble quantiles per time (odef_quantile_field, include/odefilter.h): id = Q_BASE + 8 * source + quantity (0 the quantiles,
# 1 the count), one input that odef_bind_device alone takes.  UNTESTED like the rest of this file.
const Q_BASE = 320
const Q_FILTER = 320
const Q_COUNT_FILTER = 321
const Q_SMOOTH = 328
const Q_COUNT_SMOOTH = 329
const Q_DENSE = 336
const Q_COUNT_DENSE = 337
const Q_PROBS = 344
# weighted ensemble summary per time (odef_wsummary_field, include/odefilter.h): id = W_BASE + 8 * source + quantity (0 COUNT,
# 1 MEAN, 2 COV_WITHIN, 3 COV_BETWEEN, 4 LOG_EVIDENCE, 5 ESS), one input that odef_bind_device alone takes.  UNTESTED like the
# rest of this file.
const W_BASE = 384
const W_FILTER_COUNT = 384
const W_FILTER_MEAN = 385
const W_FILTER_COV_WITHIN = 386
const W_FILTER_COV_BETWEEN = 387
const W_FILTER_LOG_EVIDENCE = 388
const W_FILTER_ESS = 389
const W_SMOOTH_COUNT = 392
const W_SMOOTH_MEAN = 393
const W_SMOOTH_COV_WITHIN = 394
const W_SMOOTH_COV_BETWEEN = 395
const W_SMOOTH_LOG_EVIDENCE = 396
const W_SMOOTH_ESS = 397
const W_DENSE_COUNT = 400
const W_DENSE_MEAN = 401
const W_DENSE_COV_WITHIN = 402
const W_DENSE_COV_BETWEEN = 403
const W_DENSE_LOG_EVIDENCE = 404
const W_DENSE_ESS = 405
const W_LOGWEIGHT = 408
const RETCODES = (:Success, :MaxIters, :DtLessThanMin, :Unstable, :Unstable)

"""Ensemble algorithm: all trajectories of an `EnsembleProblem` on one GPU (`devices` empty / one entry) or sharded
over several GPUs of the node by THIS process (`devices = 0:7`): contiguous blocks of the trajectory index, nothing
exchanged while stepping, one RCCL all-gather of the final posterior means at the end (`odef_group_*`, `odef_allgather`
of include/odefilter.h; SURVEY.md 8e)."""
struct EnsembleHIP <: DiffEqBase.EnsembleAlgorithm
    device::Int
    rhs::Symbol          # which compiled-in vector field `prob.f` corresponds to
    devices::Vector{Int32}
end
EnsembleHIP(rhs::Symbol; device=-1, devices=Int32[]) = EnsembleHIP(device, rhs, collect(Int32, devices))

lasterr(ctx) = unsafe_string(ccall((:odef_last_error, LIB), Cstring, (Ptr{Cvoid},), ctx))
# which kernel the last filter (0) / smoother (1) / ensemble-summary (2) / solution-error (3) / data-likelihood (4) / event-location (5) / ensemble-quantile (6) / weighted-summary (7) pass launched, and its device time in ms
function kernel_name(ctx, which::Integer)
    buf = zeros(UInt8, 256)
    GC.@preserve buf ccall((:odef_kernel_name, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{UInt8}, Csize_t), ctx, which, buf, length(buf))
    return unsafe_string(pointer(buf))
end
function kernel_time_ms(ctx, which::Integer)
    ms = Ref{Cfloat}(0); n = Ref{Cint}(0)
    ccall((:odef_kernel_time_ms, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Cfloat}, Ptr{Cint}), ctx, which, ms, n)
    return ms[], n[]
end
check(rc, ctx) = rc == 0 || error("libodefilter_hip: " * lasterr(ctx))

function fetch(ctx, field, ::Type{T}, dims...) where {T}
    out = Array{T}(undef, dims...)
    GC.@preserve out check(ccall((:odef_get, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Csize_t),
                                 ctx, field, out, sizeof(out)), ctx)
    out
end

"""
    ensemble_summary(ctx, d; source=0) -> (n, mean, within, between)

Per-time summary of the ensemble held by the live context `ctx` (state dimension of the ODE `d`), reduced on the device:
`n[s]` included trajectories (Success retcode, finite mean), `mean[:, s]` the mean of their posterior means, `within[:, s]` /
`between[:, s]` the packed lower triangles (element (k,l), k >= l, 0-based, at k(k+1)/2+l) of the mean posterior covariance and
of the covariance of the means (divisor n).  `within + between` is the covariance of the equal-weight Gaussian mixture.
source 0: filter records, 1: smoothed records, 2: the last `odef_dense_output` result (the only one an adaptive solve admits).
"""
function ensemble_summary(ctx, d::Integer; source::Integer=0)
    id(q) = S_BASE + 8 * source + q
    nb = Ref{Csize_t}(0)
    check(ccall((:odef_field_bytes, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Csize_t}), ctx, id(0), nb), ctx)
    n_t = Int(nb[] ÷ 8); tri = d * (d + 1) ÷ 2
    return (n = fetch(ctx, id(0), Int64, n_t), mean = fetch(ctx, id(1), Float64, d, n_t),
            within = fetch(ctx, id(2), Float64, tri, n_t), between = fetch(ctx, id(3), Float64, tri, n_t))
end

"""
    ensemble_quantiles(ctx, d, probs; source=0) -> (n, q)

Per-time quantiles of the ensemble held by the live context `ctx` (state dimension of the ODE `d`), selected on the device:
`q[a, p, s]` is the type-7 quantile (Julia's `quantile` default) `p` of solution component `a` of the posterior means over the
`n[s]` trajectories included at time `s` (Success retcode, finite mean); NaN where `n[s] == 0`.  `probs` is a DEVICE pointer that
stays the caller's, given as `(ptr, bytes)`: Float64 [P], 1 <= P <= 8, each in [0, 1].  The result is the order statistic
itself (exact radix selection), interpolated with one rounding per operation.  source 0: filter records, 1: smoothed records,
2: the last `odef_dense_output` result (the only one an adaptive solve admits).  UNTESTED.
"""
function ensemble_quantiles(ctx, d::Integer, probs; source::Integer=0)
    ptr, bytes = probs
    check(ccall((:odef_bind_device, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Csize_t), ctx, Q_PROBS, ptr, bytes), ctx)
    id(q) = Q_BASE + 8 * source + q
    nb = Ref{Csize_t}(0)
    check(ccall((:odef_field_bytes, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Csize_t}), ctx, id(1), nb), ctx)
    n_t = Int(nb[] ÷ 8); P = Int(bytes ÷ 8)
    return (n = fetch(ctx, id(1), Int64, n_t), q = fetch(ctx, id(0), Float64, d, P, n_t))
end

"""
    weighted_ensemble_summary(ctx, d, log_weights; source=0) -> (n, mean, within, between, log_evidence, ess)

Per-time summary of the ensemble held by the live context `ctx` (state dimension of the ODE `d`) with a weight per trajectory,
reduced on the device: the moments of the mixture with weights proportional to `exp(l_i)`, the log evidence
`log((1/n) sum exp l_i)` and the effective sample size.  `log_weights` is a DEVICE pointer that stays the caller's, given as
`(ptr, bytes)`: Float64 [N]; a value that is not finite excludes its trajectory.  source 0: filter records, 1: smoothed records,
2: the last `odef_dense_output` result (the only one an adaptive solve admits).  UNTESTED.
"""
function weighted_ensemble_summary(ctx, d::Integer, log_weights; source::Integer=0)
    ptr, bytes = log_weights
    check(ccall((:odef_bind_device, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Csize_t), ctx, W_LOGWEIGHT, ptr, bytes), ctx)
    id(q) = W_BASE + 8 * source + q
    nb = Ref{Csize_t}(0)
    check(ccall((:odef_field_bytes, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Csize_t}), ctx, id(0), nb), ctx)
    n_t = Int(nb[] ÷ 8); tri = d * (d + 1) ÷ 2
    return (n = fetch(ctx, id(0), Int64, n_t), mean = fetch(ctx, id(1), Float64, d, n_t),
            within = fetch(ctx, id(2), Float64, tri, n_t), between = fetch(ctx, id(3), Float64, tri, n_t),
            log_evidence = fetch(ctx, id(4), Float64, n_t), ess = fetch(ctx, id(5), Float64, n_t))
end

"""
    solution_errors(ctx, n_traj; source=0) -> Dict(:l∞, :l2, :final, :chi2), nused

`sol.errors` of every trajectory of the live context `ctx` (src/solution.jl:11, 68-74), reduced on the device against the vector
field's `analytic` or the reference bound as `E_REFERENCE`: DiffEqBase's `:l∞`, `:l2`, `:final` of the solution part of the
means, and `:chi2 = mean_k e' Sigma^+ e / d` (about 1 for a calibrated posterior), each of length `n_traj`.  source 0: filter
records, 1: smoothed records.  UNTESTED.
"""
function solution_errors(ctx, n_traj::Integer; source::Integer=0)
    id(q) = E_BASE + 8 * source + q
    errs = Dict(:final => fetch(ctx, id(0), Float64, n_traj), :l2 => fetch(ctx, id(1), Float64, n_traj),
                Symbol("l∞") => fetch(ctx, id(2), Float64, n_traj), :chi2 => fetch(ctx, id(3), Float64, n_traj))
    return errs, fetch(ctx, id(4), Int64, n_traj)
end

"""
    data_loglik(ctx, n_traj, saves, comps, values, noise) -> (loglik, mahalanobis)

Log-likelihood of noisy observations under the posterior of the last fixed-grid solve of the live context `ctx`, per trajectory,
reduced on the device (later versions of the reference: `fenrir_data_loglik`).  The four arguments are DEVICE pointers that stay
the caller's: `saves` Int64 [M] (0-based save indices, increasing), `comps` Int64 [o] (0-based state components, increasing),
`values` Float64 [M][o] or [M][o][N], `noise` Float64 [o] variances, each given as `(ptr, bytes)`.  UNTESTED.
"""
function data_loglik(ctx, n_traj::Integer, saves, comps, values, noise)
    for (f, (ptr, bytes)) in ((L_OBS_TIME, (C_NULL, 0)), (L_OBS_SAVE, saves), (L_OBS_COMPONENT, comps), (L_OBS_VALUE, values), (L_OBS_NOISE, noise))
        check(ccall((:odef_bind_device, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Csize_t), ctx, f, ptr, bytes), ctx)
    end
    return fetch(ctx, L_DATA_LOGLIK, Float64, n_traj), fetch(ctx, L_DATA_MAHALANOBIS, Float64, n_traj)
end

"""
    data_loglik_times(ctx, n_traj, times, comps, values, noise) -> (loglik, mahalanobis)

The same likelihood with the observations given by TIME, after a fixed-grid or an adaptive solve: `times` is a DEVICE pointer
`(ptr, bytes)` to Float64 [M], strictly increasing from t0 on; the times need not be save times (a node predicted by the filter is
inserted per trajectory).  The other arguments as for `data_loglik`.  A trajectory whose records end before the last time gets
NaN.  UNTESTED.
"""
function data_loglik_times(ctx, n_traj::Integer, times, comps, values, noise)
    for (f, (ptr, bytes)) in ((L_OBS_SAVE, (C_NULL, 0)), (L_OBS_TIME, times), (L_OBS_COMPONENT, comps), (L_OBS_VALUE, values),
                              (L_OBS_NOISE, noise))
        check(ccall((:odef_bind_device, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Csize_t), ctx, f, ptr, bytes), ctx)
    end
    return fetch(ctx, L_DATA_LOGLIK, Float64, n_traj), fetch(ctx, L_DATA_MAHALANOBIS, Float64, n_traj)
end

"""
    events(ctx, n_traj, d, K, spec, level; source=0) -> (count, t, t_std, u, direction, save, neval)

Level crossings of one component of the posterior mean per trajectory of the live context `ctx` -- what a `ContinuousCallback` with
the condition `u[c] - level` answers, asked of the finished posterior --, located on the device by a scan of the records and
bracketed Newton on the dense posterior (the state carries u', so the slope costs nothing).  `spec` and `level` are DEVICE pointers
that stay the caller's, each given as `(ptr, bytes)`: `spec` Int64 [3] `{component (0-based), direction (-1, 0, +1), K}`, `level`
Float64 [1] or [N].  `count[i]` counts all crossings, the first `K` are located: `t[i, s]`, `t_std[i, s]`, `u[:, i, s]`; unused
slots hold NaN, direction 0, save -1.  source 0: filter posterior, 1: smoothed.  UNTESTED.
"""
function events(ctx, n_traj::Integer, d::Integer, K::Integer, spec, level; source::Integer=0)
    for (f, (ptr, bytes)) in ((EV_SPEC, spec), (EV_LEVEL, level))
        check(ccall((:odef_bind_device, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Csize_t), ctx, f, ptr, bytes), ctx)
    end
    id(q) = EV_BASE + 8 * source + q
    count = fetch(ctx, id(0), Int32, n_traj)
    t = fetch(ctx, id(1), Float64, n_traj, K)
    return (count = count, t = t, t_std = sqrt.(fetch(ctx, id(2), Float64, n_traj, K)), u = permutedims(fetch(ctx, id(3), Float64, n_traj, d, K), (2, 1, 3)),
            direction = fetch(ctx, id(4), Int32, n_traj, K), save = fetch(ctx, id(5), Int32, n_traj, K), neval = fetch(ctx, id(6), Int32, n_traj, K))
end

"""
    merge_moments(parts) -> (n, mean, within, between)

Exact pooled combination of per-shard `ensemble_summary` results (shards with n = 0 at a time are skipped there):
n = sum n_r, mean = sum n_r mean_r / n, W = sum n_r W_r / n, B = sum n_r (B_r + (mean_r - mean)(mean_r - mean)') / n.
"""
function merge_moments(parts)
    d, n_t = size(parts[1].mean); tri = size(parts[1].within, 1)
    n = sum(p.n for p in parts)
    mean = fill(NaN, d, n_t); within = fill(NaN, tri, n_t); between = fill(NaN, tri, n_t)
    for s in 1:n_t
        n[s] == 0 && continue
        live = [p for p in parts if p.n[s] > 0]
        mean[:, s] = sum(p.n[s] .* p.mean[:, s] for p in live) ./ n[s]
        within[:, s] = sum(p.n[s] .* p.within[:, s] for p in live) ./ n[s]
        acc = zeros(tri)
        for p in live
            dm = p.mean[:, s] .- mean[:, s]
            for k in 0:d-1, l in 0:k
                acc[k * (k + 1) ÷ 2 + l + 1] += p.n[s] * (p.between[k * (k + 1) ÷ 2 + l + 1, s] + dm[k + 1] * dm[l + 1])
            end
        end
        between[:, s] = acc ./ n[s]
    end
    return (n = n, mean = mean, within = within, between = between)
end

"""
    compile_rhs(name, source, d, n_params; include_dir) -> rhs_id

Hand a user vector field to the library as HIP C++ source (`odef_rhs_compile`, include/odefilter.h): the stand-in for
the closure `prob.f` (+ `f.jac`) that `perform_step!` calls at src/perform_step.jl:106,116-121.  The returned id goes
into `OdefConfig.rhs_id` (register it in `RHS_IDS` under a symbol to use it with `EnsembleHIP(:name)`).
State dimensions d(q+1) <= 20 (d <= 10) run on the lane / row-team kernels; above that `odef_create` builds the
matrix-core workgroup kernels around the field for the requested order and algorithm (even d <= 32, d(q+1) <= 176).
"""
function compile_rhs(name::AbstractString, source::AbstractString, d::Integer, n_params::Integer;
                     include_dir::Union{Nothing,AbstractString}=nothing)
    id = Ref{Int32}(-1)
    rc = ccall((:odef_rhs_compile, LIB), Cint, (Cstring, Cstring, Int32, Int32, Cstring, Ptr{Int32}),
               name, source, d, n_params, include_dir === nothing ? C_NULL : include_dir, id)
    rc == 0 || error("libodefilter_hip: " * lasterr(C_NULL))   # the compiler log
    RHS_IDS[Symbol(name)] = Int(id[])
    return Int(id[])
end

"""
    __solve(ensembleprob, alg::Union{EK0,EK1}, ::EnsembleHIP; trajectories, dt, adaptive, abstol, reltol)

`u0s` is a d x N matrix (column = trajectory) -- exactly the memory layout `odef_set_problem` expects.
Returns the per-trajectory solution fields as arrays with the trajectory index FIRST (Julia column-major
view of the device layout [n_save][D][N]): `mean[i, k, s]`.
"""
function DiffEqBase.__solve(eprob::DiffEqBase.EnsembleProblem, alg::Union{EK0,EK1,IEKS}, ealg::EnsembleHIP;
                            trajectories::Int, u0s::Matrix{Float64}, dt=nothing, adaptive=true,
                            abstol=1e-6, reltol=1e-3, max_steps=4096, ieks_iterations::Int=1,
                            nsamples::Int=0, sample_seed::UInt64=UInt64(0x5A3B1E), dense_sample_times=nothing, kwargs...)
    prob = eprob.prob
    d, N = size(u0s); @assert N == trajectories
    q = alg.order; D = d * (q + 1); TRI = D * (D + 1) ÷ 2
    p = collect(Float64, prob.p)
    !adaptive && dt === nothing && error("Fixed timestep methods require a choice of dt or choosing the tstops")
    mv = alg.diffusionmodel in MV_DIFFUSIONS
    mv && !(alg isa EK0) && error("MV diffusion models require EK0")   # src/diffusions.jl:96, :125
    # IEKS: solve_ieks below; IEKS(linearize_at = sol) needs the linearisation points on the device (odef_bind_device of
    # F_LINEARIZE_AT), which this host-array binding does not keep
    alg isa IEKS && alg.linearize_at !== nothing && error("IEKS(linearize_at = sol): bind F_LINEARIZE_AT with odef_bind_device")
    alg isa IEKS && adaptive && error("IEKS relinearisation runs on fixed grids")
    cfg = Ref(OdefConfig(sizeof(OdefConfig), alg isa IEKS ? ODEF_IEKS : alg isa EK1 ? 1 : 0, q, DIFFUSIONS[alg.diffusionmodel],
                         alg.smooth ? 1 : 0, RHS_IDS[ealg.rhs], d, length(p), 1, 1, ealg.device, 1, N))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:odef_create, LIB), Cint, (Ptr{Ptr{Cvoid}}, Ptr{OdefConfig}), h, cfg)
    rc == 0 || error("libodefilter_hip: " * lasterr(C_NULL))
    ctx = h[]
    try
        t0, t1 = Float64.(prob.tspan)
        tgrid = Float64[]
        GC.@preserve u0s p check(ccall((:odef_set_problem, LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble),
                                       ctx, u0s, p, t0), ctx)
        if adaptive
            check(ccall((:odef_solve_adaptive, LIB), Cint,
                        (Ptr{Cvoid}, Cdouble, Cdouble, Cdouble, Cdouble, Ptr{Cvoid}, Int64),
                        ctx, t1, abstol, reltol, dt === nothing ? 1e-3 * (t1 - t0) : dt, C_NULL, max_steps), ctx)
        else
            tgrid = collect(Float64, t0:dt:t1); tgrid[end] < t1 && push!(tgrid, t1)   # OrdinaryDiffEq's clipped last step
            GC.@preserve tgrid check(ccall((:odef_solve_fixed, LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Int64),
                                           ctx, tgrid, length(tgrid)), ctx)
        end
        alg.smooth && check(ccall((:odef_smooth, LIB), Cint, (Ptr{Cvoid},), ctx), ctx)
        # solve_ieks (src/ieks.jl:52-61): odef_smooth has set F_LINEARIZE_AT to the smoothed u on this grid, so every
        # further fixed-grid solve + smoother is the next iteration, on the device
        if alg isa IEKS
            for _ in 2:ieks_iterations
                GC.@preserve tgrid check(ccall((:odef_solve_fixed, LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Int64),
                                               ctx, tgrid, length(tgrid)), ctx)
                check(ccall((:odef_smooth, LIB), Cint, (Ptr{Cvoid},), ctx), ctx)
            end
        end
        ns = Int(ccall((:odef_n_save, LIB), Int64, (Ptr{Cvoid},), ctx))
        mean = fetch(ctx, alg.smooth ? F_SMOOTH_MEAN : F_MEAN, Float64, N, D, ns)
        cov  = fetch(ctx, alg.smooth ? F_SMOOTH_COV_TRIL : F_COV_TRIL, Float64, N, TRI, ns)
        tsave = adaptive ? fetch(ctx, F_T, Float64, N, ns) : fetch(ctx, F_T, Float64, ns)
        nsaved = fetch(ctx, F_NSAVED, Int32, N)
        # Adaptive solves hold one record per ATTEMPTED step: a rejected attempt repeats the previous record at the
        # unchanged time (include/odefilter.h, odef_solve_adaptive).  `keep[i, s]` marks the records the reference
        # would have saved (accepted steps only, src/integrator_utils.jl:33-48): x[i, :, keep[i, :]].
        keep = trues(N, ns)
        if adaptive
            for i in 1:N, s in 1:ns
                keep[i, s] = s <= nsaved[i] && (s == 1 || tsave[i, s] != tsave[i, s - 1])
            end
        end
        # sample_states(sol, n) / dense_sample_states(sol, n) (src/solution_sampling.jl:15-75), while the context lives
        samples = nothing; dense_samples = nothing
        if nsamples > 0 && alg.smooth
            check(ccall((:odef_sample, LIB), Cint, (Ptr{Cvoid}, Int64, UInt64, Cdouble), ctx, nsamples, sample_seed, 1.0), ctx)
            samples = fetch(ctx, F_SAMPLES, Float64, N, nsamples, D, ns)
            tq = dense_sample_times === nothing ? collect(range(t0, t1, length=1000)) : collect(Float64, dense_sample_times)
            GC.@preserve tq check(ccall((:odef_dense_sample, LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Int64, Int64, UInt64, Cdouble),
                                        ctx, tq, length(tq), nsamples, sample_seed, 1.0), ctx)
            dense_samples = (fetch(ctx, F_SAMPLES, Float64, N, nsamples, D, length(tq)), tq)
        end
        return (t = tsave, keep = keep, samples = samples, dense_samples = dense_samples,
                u = view(mean, :, 1:d, :), x_mean = mean, x_cov_tril = cov,
                x_filt_mean = fetch(ctx, F_MEAN, Float64, N, D, ns),
                # MV models: [n_save][d][N] on the device, one Diagonal(sigma_1..sigma_d) per trajectory and step
                diffusions = mv ? (dv = fetch(ctx, F_DIFFUSION, Float64, N, d, ns); [Diagonal(dv[i, :, s]) for i in 1:N, s in 2:ns])
                                : fetch(ctx, F_DIFFUSION, Float64, N, ns)[:, 2:end],
                log_likelihood = fetch(ctx, F_LOGLIK, Float64, N),
                destats = (nf = fetch(ctx, F_NF, Int32, N), njacs = fetch(ctx, F_NJAC, Int32, N),
                           naccept = fetch(ctx, F_NACCEPT, Int32, N), nreject = fetch(ctx, F_NREJECT, Int32, N)),
                nsaved = nsaved,
                retcode = [RETCODES[r + 1] for r in fetch(ctx, F_RETCODE, Int32, N)])
    finally
        ccall((:odef_destroy, LIB), Cvoid, (Ptr{Cvoid},), ctx)
    end
end


"""
    solve_ieks(eprob, alg::IEKS, ealg::EnsembleHIP; iterations=10, kwargs...)

`solve_ieks` (src/ieks.jl:52-61) on one IEKS context: the first iteration is EK1 (the field of linearisation points starts
empty), each further one a fixed-grid solve linearised at the previous smoothed u plus the smoother, with no data leaving
the device between iterations.  Returns what `__solve` returns for the last iteration.  Fixed grids only.
"""
solve_ieks(eprob::DiffEqBase.EnsembleProblem, alg::IEKS, ealg::EnsembleHIP; iterations::Int=10, kwargs...) =
    DiffEqBase.__solve(eprob, IEKS(prior=alg.prior, order=alg.order, diffusionmodel=alg.diffusionmodel), ealg;
                       adaptive=false, kwargs..., ieks_iterations=iterations)

grouperr(g) = unsafe_string(ccall((:odef_group_last_error, LIB), Cstring, (Ptr{Cvoid},), g))
gcheck(rc, g) = rc == 0 || error("libodefilter_hip: " * grouperr(g))

"""
    solve_sharded(eprob, alg, ealg; trajectories, u0s, dt, adaptive, ...) -> (final_mean, shards, ctxs...)

The multi-GPU path of `EnsembleHIP(rhs; devices = 0:7)`: one `odef_group` over `ealg.devices`, the whole ensemble handed
over once (`odef_group_set_problem` cuts it into the shards of `odef_shard_range`), the shards' kernels running
concurrently, and ONE collective at the end: `odef_allgather` leaves the final posterior means of all N trajectories,
`final_mean[i, k]`, on every device (returned here from device 1).  Per-shard time series stay on their device and are
read with `fetch(odef_group_ctx(g, k), ...)` exactly as in the single-GPU method -- a full gather of an every-step
record (48.9 GB at the BASELINE size) is deliberately not part of the path.
"""
function solve_sharded(eprob::DiffEqBase.EnsembleProblem, alg::Union{EK0,EK1}, ealg::EnsembleHIP;
                       trajectories::Int, u0s::Matrix{Float64}, dt=nothing, adaptive=true, abstol=1e-6, reltol=1e-3,
                       max_steps=4096)
    prob = eprob.prob
    d, N = size(u0s); @assert N == trajectories
    q = alg.order; D = d * (q + 1)
    p = collect(Float64, prob.p)
    cfg = Ref(OdefConfig(sizeof(OdefConfig), alg isa EK1 ? 1 : 0, q, DIFFUSIONS[alg.diffusionmodel],
                         alg.smooth ? 1 : 0, RHS_IDS[ealg.rhs], d, length(p), 1, 1, -1, 1, N))
    G = length(ealg.devices)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    devs = ealg.devices
    rc = GC.@preserve devs ccall((:odef_group_create, LIB), Cint, (Ptr{Ptr{Cvoid}}, Ptr{OdefConfig}, Int32, Ptr{Int32}), h, cfg, G, devs)
    rc == 0 || error("libodefilter_hip: " * grouperr(C_NULL))
    g = h[]
    try
        t0, t1 = Float64.(prob.tspan)
        GC.@preserve u0s p gcheck(ccall((:odef_group_set_problem, LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble), g, u0s, p, t0), g)
        if adaptive
            gcheck(ccall((:odef_group_solve_adaptive, LIB), Cint, (Ptr{Cvoid}, Cdouble, Cdouble, Cdouble, Cdouble, Ptr{Cvoid}, Int64),
                         g, t1, abstol, reltol, dt === nothing ? 1e-3 * (t1 - t0) : dt, C_NULL, max_steps), g)
        else
            tgrid = collect(t0:dt:t1); tgrid[end] < t1 && push!(tgrid, t1)
            GC.@preserve tgrid gcheck(ccall((:odef_group_solve_fixed, LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Int64), g, tgrid, length(tgrid)), g)
        end
        alg.smooth && gcheck(ccall((:odef_group_smooth, LIB), Cint, (Ptr{Cvoid},), g), g)
        gcheck(ccall((:odef_allgather, LIB), Cint, (Ptr{Cvoid}, Cint), g, alg.smooth ? 1 : 0), g)   # the one collective
        final_mean = Array{Float64}(undef, N, D)       # C layout [D][N] == Julia (N, D)
        GC.@preserve final_mean gcheck(ccall((:odef_group_get_gathered, LIB), Cint,
                                             (Ptr{Cvoid}, Int32, Ptr{Cdouble}, Ptr{Ptr{Cvoid}}, Ptr{Csize_t}), g, 0, final_mean, C_NULL, C_NULL), g)
        shards = map(0:G-1) do k
            first = Ref{Int64}(0); count = Ref{Int64}(0)
            ccall((:odef_group_shard, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Int64}, Ptr{Int64}), g, k, first, count)
            (first[] + 1):(first[] + count[])      # 1-based trajectory range of shard k
        end
        # ensemble summary of the WHOLE ensemble on a fixed grid: every shard reduces its records on its own device, the
        # per-shard blocks (kilobytes) are pooled on the host -- no collective, no full time-series gather
        summary = adaptive ? nothing :
            merge_moments([ensemble_summary(ccall((:odef_group_ctx, LIB), Ptr{Cvoid}, (Ptr{Cvoid}, Int32), g, k), d; source = alg.smooth ? 1 : 0)
                           for k in 0:G-1])
        return (final_mean = final_mean, u_final = view(final_mean, :, 1:d), shards = shards, summary = summary)
    finally
        ccall((:odef_group_destroy, LIB), Cvoid, (Ptr{Cvoid},), g)
    end
end

end # module
