# RedClustHIP.jl — Julia-side binding of libredclust_hip.so (include/redclust_hip.h).
#
# Drop-in for the sampler of RedClust.jl: `runsampler_hip` has the signature, the defaults and the result of
# `RedClust.runsampler` (src/mcmc.jl:501-590) and runs the whole iteration loop — sample_r!, sample_p!, the split–merge
# proposals, the Gibbs sweep, loglik / logprior of the recorded samples, sortlabels and the co-clustering matrix — in one
# call into the library (rc_run_chain) on an MI355X.  The structs MCMCData / MCMCOptionsList / PriorHyperparamsList /
# MCMCState / MCMCResult are RedClust's own, unchanged; fitprior and the k-medoids initialisation are RedClust's own
# functions, called here exactly as runsampler calls them.
#
# NOT EXECUTED IN THE BUILD IMAGE (no julia binary there).  What is checked instead: every ccall below is compared —
# symbol, arity, argument and return types, struct layouts — with the prototypes of include/redclust_hip.h by
# tests/test_oracle_cpu.py::test_julia_glue_ccalls_match_the_header, and the same entry points are exercised by the
# Python host (redclust.jl_amd/) and its GPU tests.
module RedClustHIP

using RedClust
using RedClust: MCMCData, MCMCOptionsList, PriorHyperparamsList, MCMCState, MCMCResult, fitprior, iac_ess_acf
using Clustering: kmedoids
using Distributions: Beta, Gamma
using StatsBase: mean, mean_and_var
import Random

const LIB = get(ENV, "REDCLUST_HIP_LIB", "libredclust_hip.so")

struct RcParams                      # struct rc_params
    delta1::Cdouble; delta2::Cdouble; alpha::Cdouble; beta::Cdouble; zeta::Cdouble; gamma::Cdouble
    eta::Cdouble; sigma::Cdouble; u::Cdouble; v::Cdouble
    maxK::Int64
    repulsion::UInt8
    pad_::NTuple{7,UInt8}
end
RcParams(p::PriorHyperparamsList) = RcParams(p.δ1, p.δ2, p.α, p.β, p.ζ, p.γ, p.η, p.σ, p.u, p.v,
                                             p.maxK, UInt8(p.repulsion), ntuple(_ -> 0x00, 7))

struct RcChainOptions                # struct rc_chain_options
    numiters::Int64; burnin::Int64; thin::Int64
    numGibbs::Int64; numMH::Int64
    splitmerge_mode::Int32
    pad_::Int32
    seed::UInt64
    first_iter::UInt64
    r0::Cdouble; p0::Cdouble
    proposalsd_r::Cdouble
    r_trace::Ptr{Cdouble}; p_trace::Ptr{Cdouble}
    max_samples::Int64
end

struct RcChainOutputs                # struct rc_chain_outputs (isbits: a Ref or a Vector of them is the C object)
    clusts::Ptr{Int64}
    K::Ptr{Int64}
    r::Ptr{Cdouble}; p::Ptr{Cdouble}; loglik::Ptr{Cdouble}; logposterior::Ptr{Cdouble}
    r_acceptances::Ptr{UInt8}
    splitmerge_acceptances::Ptr{UInt8}; splitmerge_splits::Ptr{UInt8}
    r_all::Ptr{Cdouble}; p_all::Ptr{Cdouble}
    num_samples::Int64
    runtime_s::Cdouble
    r_final::Cdouble; p_final::Cdouble
end

struct RcChainsInput                 # struct rc_chains_input
    n::Int64
    D::Ptr{Cdouble}
    logD_or_null::Ptr{Cdouble}
    points::Ptr{Cdouble}
    dim::Int64
    storage_bits::Int32
    pad_::Int32
    kcap::Int64
    params::Ptr{RcParams}
    init_clusts::Ptr{Int64}
end

# error classes of include/redclust_hip.h: RC_ERR_ARG (-1) and RC_ERR_DOMAIN (-4) are the caller's input — the reference
# throws ArgumentError for those (src/types.jl:149-154); the rest are run-time failures
function check(ctx::Ptr{Cvoid}, rc::Int32)
    rc == 0 && return
    msg = unsafe_string(ccall((:rc_last_error, LIB), Cstring, (Ptr{Cvoid},), ctx))
    (rc == -1 || rc == -4) ? throw(ArgumentError(msg)) : error(msg)
end

# runsampler's defaults, verbatim (src/mcmc.jl:516-527): fitprior on the data, k-medoids labels, r and p from their priors
function default_params_init(data::MCMCData, params, init; verbose)
    if isnothing(params)
        params = fitprior(data.D, "k-medoids", true; verbose=verbose)
    end
    if isnothing(init)
        init = MCMCState(
            clusts=kmedoids(data.D,
                (params.maxK > 0 ? minimum([params.maxK, params.K_initial]) : params.K_initial);
                maxiter=1000).assignments,
            r=rand(Gamma(params.η, 1 / params.σ)),
            p=rand(Beta(params.u, params.v))
        )
    end
    return params, init
end

# the summary block of runsampler after the loop (src/mcmc.jl:562-587), unchanged
function summarise!(result::MCMCResult, options::MCMCOptionsList, params::PriorHyperparamsList, runtime::Real)
    result.K_iac, result.K_ess, result.K_acf = iac_ess_acf(result.K)
    result.K_mean, result.K_variance = mean_and_var(result.K)
    result.r_iac, result.r_ess, result.r_acf = iac_ess_acf(result.r)
    result.r_mean, result.r_variance = mean_and_var(result.r)
    result.p_iac, result.p_ess, result.p_acf = iac_ess_acf(result.p)
    result.p_mean, result.p_variance = mean_and_var(result.p)
    result.splitmerge_acceptance_rate = options.numMH > 0 ? mean(result.splitmerge_acceptances) : 0
    result.r_acceptance_rate = mean(result.r_acceptances)
    result.options = options
    result.params = params
    result.runtime = runtime
    result.mean_iter_time = runtime / options.numiters
    return result
end

"""
    runsampler_hip(data, options = MCMCOptionsList(), params = nothing, init = nothing;
                   verbose = true, seed = rand(UInt64), device = 0, kcap = 0, exact_logD = false,
                   splitmerge = :as_written) -> MCMCResult

`RedClust.runsampler` (src/mcmc.jl:501-590) with the iteration loop on the GPU.  Same positional arguments and defaults:
the default `MCMCOptionsList()` (numMH = 1, numGibbs = 5) is accepted as is, `params = nothing` calls `fitprior` and
`init = nothing` the k-medoids initialisation, exactly as the reference does.  Every field of the result is filled.

Differences, all in the random streams (DESIGN.md "Uniform stream"): the label draws, the split–merge draws and the r / p
updates come from the library's counter-based streams keyed by `seed` (drawn from Julia's RNG by default, so
`Random.seed!` still fixes a run), not from Julia's task-local RNG — same distributions, different numbers.
`splitmerge = :intended` keeps accepted proposals (the reference as written discards them, SURVEY.md §3.2 Q1).
A distance matrix with zero off-diagonal entries is refused with an ArgumentError (the reference would carry
log(0) = -Inf into every log-weight): remove duplicate observations or jitter them.

`points = X, metric = :cityblock` (together; X is n×dim, a name of `METRICS`): the device computes its matrix from the
coordinates in that metric (rc_create_from_points_metric) instead of taking `data.D`; `data` is then
`MCMCData(pairwise(HIPBackend(), X; metric = :cityblock))`, whose D and logD the split–merge scans and `fitprior` read.
"""
function runsampler_hip(data::MCMCData,
    options::MCMCOptionsList=MCMCOptionsList(),
    params::Union{PriorHyperparamsList,Nothing}=nothing,
    init::Union{MCMCState,Nothing}=nothing;
    verbose=true, seed::Integer=rand(UInt64), device::Integer=0, kcap::Integer=0, exact_logD::Bool=false,
    splitmerge::Symbol=:as_written, points::Union{Matrix{Float64},Nothing}=nothing, metric=nothing)::MCMCResult
    ostream = verbose ? stdout : devnull
    splitmerge in (:as_written, :intended) || throw(ArgumentError("splitmerge must be :as_written or :intended"))
    (points === nothing) == (metric === nothing) || throw(ArgumentError("points and metric go together."))
    params, init = default_params_init(data, params, init; verbose=verbose)
    n = size(data.D, 1)
    ns = options.numsamples
    result = MCMCResult(data, options, params)
    printstyled(ostream, "Run MCMC\n"; bold=true, color=:blue)
    printstyled(ostream, "Setup: "; bold=true)
    println(ostream, "$(options.numiters) iterations, $ns samples, $n observations.")
    h = Ref{Ptr{Cvoid}}(C_NULL)
    # MCMCData keeps D and logD = log.(D - Diagonal(D) + I) (src/types.jl:146-147,155).  By default only D is handed over:
    # the library then evaluates logD from its fixed-point D on the fly (DESIGN.md "Derived logD": half the HBM traffic per
    # sweep; each entry within 2^-33 ≈ 1.2e-10 of the package's value, within 1e-12 for entries near the largest).
    # exact_logD = true hands data.logD over instead: the device copy is then the package's logD rounded to the
    # fixed-point grid.  D is symmetric, so column-major == row-major.
    # points with a metric (n×dim, one observation per row; `data` then holds pairwise(HIPBackend(), points; metric) for the
    # host side): the device computes its matrix from the coordinates in that metric (rc_create_from_points_metric)
    if points !== nothing
        size(points, 1) == n || throw(ArgumentError("points must have one row per observation of data."))
        code = metric_code(metric, size(points, 2))
        X = permutedims(points)                                   # dim×n column-major = n×dim row-major
        rc = ccall((:rc_create_from_points_metric, LIB), Int32,
                   (Int64, Int64, Ptr{Cdouble}, Int32, Int32, Int32, Int64, Ref{Ptr{Cvoid}}),
                   n, size(points, 2), X, code, 64, device, kcap, h)
    else
        GC.@preserve data begin
            rc = ccall((:rc_create, LIB), Int32,
                       (Int64, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Int32, Int64, Ref{Ptr{Cvoid}}),
                       n, data.D, exact_logD ? pointer(data.logD) : Ptr{Cdouble}(C_NULL), 64, device, kcap, h)
        end
    end
    check(Ptr{Cvoid}(C_NULL), rc)
    ctx = h[]
    try
        check(ctx, ccall((:rc_set_params, LIB), Int32, (Ptr{Cvoid}, Ref{RcParams}), ctx, Ref(RcParams(params))))
        check(ctx, ccall((:rc_set_state, LIB), Int32, (Ptr{Cvoid}, Ptr{Int64}), ctx, init.clusts))
        check(ctx, ccall((:rc_cocluster_reset, LIB), Int32, (Ptr{Cvoid},), ctx))
        # RC_MODE_INCREMENTAL (1): the row-sum table is computed once and then corrected exactly under label changes instead of being
        # recomputed from D in every sweep — bit-identical results (integer sums), and never more work: while labels move the
        # sweep is bound by the resolver, and the row reduction beside it only takes issue slots (3.9 k against 3.2 k sweeps/s at
        # 40 label changes per sweep, N = 8192).  The Python host's runsampler does the same.
        check(ctx, ccall((:rc_set_mode, LIB), Int32, (Ptr{Cvoid}, Int32), ctx, 1))
        if options.numMH > 0
            # the restricted scans of the split–merge proposals read the host matrices, as the reference's do
            check(ctx, ccall((:rc_attach_host_matrices, LIB), Int32, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}),
                             ctx, data.D, data.logD))
        end
        clusts = Matrix{Int64}(undef, n, max(ns, 1))             # column j = sample j (row-major ns×n for the library)
        racc = zeros(UInt8, options.numiters)
        smacc = zeros(UInt8, max(options.numiters * options.numMH, 1))
        smspl = zeros(UInt8, max(options.numiters * options.numMH, 1))
        opt = RcChainOptions(options.numiters, options.burnin, options.thin, options.numGibbs, options.numMH,
                             splitmerge == :intended ? 1 : 0, 0, seed % UInt64, 0, init.r, init.p, params.proposalsd_r,
                             C_NULL, C_NULL, ns)
        out = Ref(RcChainOutputs(pointer(clusts), pointer(result.K), pointer(result.r), pointer(result.p),
                                 pointer(result.loglik), pointer(result.logposterior), pointer(racc), pointer(smacc),
                                 pointer(smspl), C_NULL, C_NULL, 0, 0.0, 0.0, 0.0))
        GC.@preserve data clusts racc smacc smspl result begin
            check(ctx, ccall((:rc_run_chain, LIB), Int32, (Ptr{Cvoid}, Ref{RcChainOptions}, Ref{RcChainOutputs}),
                             ctx, opt, out))
        end
        for j in 1:ns
            result.clusts[j] .= view(clusts, :, j)
        end
        result.r_acceptances .= view(racc, 1:options.numiters) .!= 0
        result.splitmerge_acceptances .= view(smacc, 1:options.numiters*options.numMH) .!= 0
        result.splitmerge_splits .= view(smspl, 1:options.numiters*options.numMH) .!= 0
        println(ostream, "Computing summary statistics and diagnostics.")
        # row-major n×n from the library == column-major because the matrix is symmetric (src/mcmc.jl:560)
        check(ctx, ccall((:rc_cocluster, LIB), Int32, (Ptr{Cvoid}, Ptr{Cdouble}, Int64),
                         ctx, result.posterior_coclustering, max(ns, 1)))
        return summarise!(result, options, params, out[].runtime_s)
    finally
        ccall((:rc_destroy, LIB), Int32, (Ptr{Cvoid},), ctx)
    end
end

"""
    runsampler_hip_chains(data, options, params, init; devices = [0], seed = rand(UInt64), kcap = 0)
        -> (results::Vector{MCMCResult}, posterior_coclustering::Matrix{Float64}, total_samples::Int)

`length(devices)` independent chains, one per GPU, from one call into the library (rc_run_chains: a host thread and a
context per device, chain c seeded `seed + c - 1`, then one RCCL all-reduce of the co-clustering counts).  Every chain
starts from `init`; `results[c]` is the `MCMCResult` of chain c, the matrix is Σ counts / Σ numsamples over all chains.
"""
function runsampler_hip_chains(data::MCMCData,
    options::MCMCOptionsList=MCMCOptionsList(),
    params::Union{PriorHyperparamsList,Nothing}=nothing,
    init::Union{MCMCState,Nothing}=nothing;
    devices::Vector{<:Integer}=[0], seed::Integer=rand(UInt64), kcap::Integer=0, verbose=true,
    splitmerge::Symbol=:as_written)
    params, init = default_params_init(data, params, init; verbose=verbose)
    n = size(data.D, 1); ns = options.numsamples; nch = length(devices)
    results = [MCMCResult(data, options, params) for _ in 1:nch]
    clusts = [Matrix{Int64}(undef, n, max(ns, 1)) for _ in 1:nch]
    racc = [zeros(UInt8, options.numiters) for _ in 1:nch]
    smacc = [zeros(UInt8, max(options.numiters * options.numMH, 1)) for _ in 1:nch]
    smspl = [zeros(UInt8, max(options.numiters * options.numMH, 1)) for _ in 1:nch]
    outs = [RcChainOutputs(pointer(clusts[c]), pointer(results[c].K), pointer(results[c].r), pointer(results[c].p),
                           pointer(results[c].loglik), pointer(results[c].logposterior), pointer(racc[c]),
                           pointer(smacc[c]), pointer(smspl[c]), C_NULL, C_NULL, 0, 0.0, 0.0, 0.0) for c in 1:nch]
    rcparams = Ref(RcParams(params))
    devs = Int32.(devices)
    opt = RcChainOptions(options.numiters, options.burnin, options.thin, options.numGibbs, options.numMH,
                         splitmerge == :intended ? 1 : 0, 0, seed % UInt64, 0, init.r, init.p, params.proposalsd_r,
                         C_NULL, C_NULL, ns)
    post = zeros(n, n)
    total = Ref{Int64}(0)
    GC.@preserve data init rcparams clusts racc smacc smspl results outs begin
        inp = RcChainsInput(n, pointer(data.D), pointer(data.logD), Ptr{Cdouble}(C_NULL), 0, 64, 0, kcap,
                            Base.unsafe_convert(Ptr{RcParams}, rcparams), pointer(init.clusts))
        rc = ccall((:rc_run_chains, LIB), Int32,
                   (Int32, Ptr{Int32}, Ref{RcChainsInput}, Ref{RcChainOptions}, Ptr{RcChainOutputs}, Ptr{Cdouble},
                    Ref{Int64}, Ptr{Cdouble}),
                   nch, devs, inp, opt, outs, post, total, Ptr{Cdouble}(C_NULL))
        check(Ptr{Cvoid}(C_NULL), rc)
    end
    for c in 1:nch
        runtime = outs[c].runtime_s
        for j in 1:ns
            results[c].clusts[j] .= view(clusts[c], :, j)
        end
        results[c].r_acceptances .= racc[c] .!= 0
        results[c].splitmerge_acceptances .= view(smacc[c], 1:options.numiters*options.numMH) .!= 0
        results[c].splitmerge_splits .= view(smspl[c], 1:options.numiters*options.numMH) .!= 0
        results[c].posterior_coclustering .= post
        summarise!(results[c], options, params, runtime)
    end
    return results, post, Int(total[])
end

"""
    HIPBackend(device = 0)

The reference's own name for the sampler: `RedClust.runsampler` gets one more method, selected by a backend in front of its usual
arguments — `runsampler(HIPBackend(), data, options, params, init)` is `runsampler_hip(data, options, params, init; device = 0)`.
The one line of a user's script that changes (INTEGRATION.md §1): `result = runsampler(data, options, params)` becomes
`result = runsampler(HIPBackend(), data, options, params)`; everything before it (`MCMCData`, `fitprior`, `MCMCOptionsList`) and
after it (`getpointestimate`, `summarise`, the plots) works on the same structs as before.
"""
struct HIPBackend
    device::Int
end
HIPBackend() = HIPBackend(0)

RedClust.runsampler(b::HIPBackend, data::MCMCData,
    options::MCMCOptionsList=MCMCOptionsList(),
    params::Union{PriorHyperparamsList,Nothing}=nothing,
    init::Union{MCMCState,Nothing}=nothing; kwargs...) = runsampler_hip(data, options, params, init; device=b.device, kwargs...)

export runsampler_hip, runsampler_hip_chains, getpointestimate_hip, HIPBackend

"""
    getpointestimate_hip(result; loss = "VI", device = 0) -> (clust, i)

`getpointestimate(result; method = "MPEL", loss)` (src/pointestimate.jl:49-58) with the numsamples² loss matrix computed
on the GPU (rc_loss_matrix).
"""
function getpointestimate_hip(result; loss::String = "VI", device::Integer = 0)
    code = Dict("binder" => 0, "omARI" => 1, "VI" => 2, "ID" => 3)
    haskey(code, loss) || throw(ArgumentError("Invalid loss function specifier."))
    m = length(result.clusts); n = length(result.clusts[1])
    samples = Matrix{Int64}(undef, n, m)                        # column s = sample s: row-major m×n for the library
    for s in 1:m
        samples[:, s] .= result.clusts[s]
    end
    best = Ref{Int64}(0)
    rc = ccall((:rc_loss_matrix, LIB), Int32,
               (Int32, Ptr{Int64}, Int64, Int64, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Int64}, Ptr{Cdouble}),
               device, samples, m, n, code[loss], C_NULL, C_NULL, best, C_NULL)
    check(Ptr{Cvoid}(C_NULL), rc)
    return (result.clusts[best[] + 1], Int(best[]) + 1)
end

"""
    searchpointestimate(HIPBackend(), result; loss = "VI", nruns = 16, maxK = 0, maxsweeps = 100, seed = 0) -> (clust, info)

A greedy search over all partitions for the clustering of minimum expected loss under `result`'s co-clustering counts
(rc_psm_search_samples: the SALSO-style search the reference's documentation sends its users to R for; the counts are built
from `result.clusts` on the GPU and never reach the host).  `nruns` runs from empty
labels in random point orders plus one run started at `getpointestimate_hip(result; loss)`, so the answer is never worse
under the searched criterion than the best sample.  `loss`: "binder" or "VI" (Wade & Ghahramani's lower bound).
`info`: named tuple of the per-run `loss`, `sweeps`, `converged`, `moves`, `K`, all `labels` (n × runs) and `best`.

`exact = true` (`loss = "VI"` only) minimises the posterior expected VI itself — the mean over `result.clusts` of VI(c, sample),
SALSO's "VI" — instead of its lower bound (rc_vi_search: fixed point, every run an exact integer function of its inputs).
Its runs are the same `nruns` orders from empty labels, one from the MPEL VI sample and one from the result of the
lower-bound search with the same arguments, so the answer is never worse in expected VI than either; `info.loss` is then the
expected VI and `info.loss_num` the integer criterion.

`loss = "ID"` minimises the posterior expected information distance — the mean over `result.clusts` of
`infodist(c, sample; normalised = false)`, the `id` of `evaluateclustering` — with the same kernel and fixed point
(rc_id_search); `exact` may be either value.  Its runs are the `nruns` orders from empty labels, one from the MPEL ID sample
and one from the result of `exact = true, loss = "VI"` with the same arguments; `info.loss` is the expected ID.
"""
struct RcPsmRun
    loss::Cdouble
    loss_num::Int64
    sweeps::Int32; converged::Int32
    moves::Int64
    K::Int32; pad_::Int32
end

# column s = sample s: row-major m×n for the library
function samplematrix(result)
    m = length(result.clusts); n = length(result.clusts[1])
    samples = Matrix{Int64}(undef, n, m)
    for s in 1:m
        samples[:, s] .= result.clusts[s]
    end
    return samples
end

psminfo(runs, labels, best) =
    (loss = [x.loss for x in runs], sweeps = [Int(x.sweeps) for x in runs], converged = [x.converged != 0 for x in runs],
     moves = [Int(x.moves) for x in runs], K = [Int(x.K) for x in runs], labels = labels, best = Int(best[1]) + 1)

function searchpointestimate(b::HIPBackend, result; loss::String = "VI", nruns::Integer = 16, maxK::Integer = 0,
                             maxsweeps::Integer = 100, seed::Integer = 0, exact::Bool = false)
    code = Dict("binder" => 0, "VI" => 1)
    loss == "ID" && return searchexactid(b, result, nruns, maxK, maxsweeps, seed)
    haskey(code, loss) || throw(ArgumentError("Invalid loss function specifier."))
    if exact
        loss == "VI" || throw(ArgumentError("exact = true needs loss = \"VI\""))
        return searchexactvi(b, result, nruns, maxK, maxsweeps, seed)
    end
    samples = samplematrix(result)                                # the counts are built from these on the device and stay there
    n, m = size(samples)
    R = Int(nruns) + 1
    init = zeros(Int64, n, R)                                     # column r = run r: row-major R×n for the library
    order = Matrix{Int32}(undef, n, R)
    rng = Random.MersenneTwister(seed)
    for r in 1:nruns
        order[:, r] .= Random.randperm(rng, n)
    end
    start, _ = getpointestimate_hip(result; loss = loss, device = b.device)
    init[:, R] .= start
    order[:, R] .= 1:n
    labels = Matrix{Int64}(undef, n, R)
    runs = Vector{RcPsmRun}(undef, R)
    best = Int32[0]
    rc = ccall((:rc_psm_search_samples, LIB), Int32,
               (Int32, Ptr{Int64}, Int64, Int64, Int32, Int32, Ptr{Int64}, Ptr{Int32}, Int32, Int32, Ptr{Int64}, Ptr{Cvoid},
                Ptr{Int32}, Ptr{Cdouble}, Ptr{Cdouble}),
               b.device, samples, m, n, code[loss], R, init, order, maxK, maxsweeps, labels, runs, best, C_NULL, C_NULL)
    check(Ptr{Cvoid}(C_NULL), rc)
    return (labels[:, best[1] + 1], psminfo(runs, labels, best))
end

"""
    searchpointestimate(HIPBackend(), counts, numsamples; loss = "VI", nruns = 16, maxK = 0, maxsweeps = 100, seed = 0, init = nothing)

The same search for callers that hold the co-clustering counts and not the samples (rc_psm_search): `counts` is the n × n
`Matrix{UInt32}` with `numsamples` on its diagonal, e.g. from `posteriorcounts` or summed over several results.  Runs: `nruns`
from empty labels in random point orders and one per column of `init` (an n × k matrix of labels, identity order).
"""
function searchpointestimate(b::HIPBackend, counts::Matrix{UInt32}, numsamples::Integer; loss::String = "VI",
                             nruns::Integer = 16, maxK::Integer = 0, maxsweeps::Integer = 100, seed::Integer = 0,
                             init::Union{Matrix{Int64},Nothing} = nothing)
    code = Dict("binder" => 0, "VI" => 1)
    haskey(code, loss) || throw(ArgumentError("Invalid loss function specifier."))
    n = size(counts, 1)
    size(counts, 2) == n || throw(ArgumentError("counts must be a square matrix"))
    extra = init === nothing ? 0 : size(init, 2)
    R = Int(nruns) + extra
    R >= 1 || throw(ArgumentError("no run: nruns = 0 and no init"))
    inits = zeros(Int64, n, R)                                    # column r = run r: row-major R×n for the library
    order = Matrix{Int32}(undef, n, R)
    rng = Random.MersenneTwister(seed)
    for r in 1:nruns
        order[:, r] .= Random.randperm(rng, n)
    end
    for k in 1:extra
        inits[:, nruns + k] .= view(init, :, k)
        order[:, nruns + k] .= 1:n
    end
    labels = Matrix{Int64}(undef, n, R)
    runs = Vector{RcPsmRun}(undef, R)
    best = Int32[0]
    rc = ccall((:rc_psm_search, LIB), Int32,
               (Int32, Ptr{Cvoid}, Int64, Int64, Int32, Int32, Ptr{Int64}, Ptr{Int32}, Int32, Int32, Ptr{Int64}, Ptr{Cvoid},
                Ptr{Int32}, Ptr{Cdouble}),
               b.device, counts, numsamples, n, code[loss], R, inits, order, maxK, maxsweeps, labels, runs, best, C_NULL)
    check(Ptr{Cvoid}(C_NULL), rc)
    return (labels[:, best[1] + 1], psminfo(runs, labels, best))
end

"""
    posteriorcounts(HIPBackend(), result) -> Matrix{UInt32}

The exact co-clustering counts of `result.clusts` — entry (i, j) is the number of samples in which i and j share a cluster,
`result.posterior_coclustering` times the number of samples — built on the GPU (rc_samples_counts).
"""
function posteriorcounts(b::HIPBackend, result)
    samples = samplematrix(result)
    n, m = size(samples)
    counts = Matrix{UInt32}(undef, n, n)                          # symmetric: row- and column-major agree
    rc = ccall((:rc_samples_counts, LIB), Int32,
               (Int32, Ptr{Int64}, Int64, Int64, Ptr{Cvoid}, Ptr{Cdouble}),
               b.device, samples, m, n, counts, C_NULL)
    check(Ptr{Cvoid}(C_NULL), rc)
    return counts
end

function searchexactvi(b::HIPBackend, result, nruns::Integer, maxK::Integer, maxsweeps::Integer, seed::Integer)
    samples = samplematrix(result)
    n, m = size(samples)
    lower, _ = searchpointestimate(b, result; loss = "VI", nruns = nruns, maxK = maxK, maxsweeps = maxsweeps, seed = seed)
    R = Int(nruns) + 2
    init = zeros(Int64, n, R)                                     # column r = run r: row-major R×n for the library
    order = Matrix{Int32}(undef, n, R)
    rng = Random.MersenneTwister(seed)
    for r in 1:nruns
        order[:, r] .= Random.randperm(rng, n)
    end
    start, _ = getpointestimate_hip(result; loss = "VI", device = b.device)
    init[:, R - 1] .= start; order[:, R - 1] .= 1:n
    init[:, R] .= lower; order[:, R] .= 1:n
    cap = Int(maxK)
    if cap == 0                                                   # the library's default cap, widened to the starts' cluster counts
        lmax = maximum(length(unique(c)) for c in result.clusts)
        need = max(length(unique(start)), length(unique(lower)))
        cap = need > lmax ? need : 0
    end
    labels = Matrix{Int64}(undef, n, R)
    runs = Vector{RcPsmRun}(undef, R)
    best = Int32[0]
    rc = ccall((:rc_vi_search, LIB), Int32,
               (Int32, Ptr{Int64}, Int64, Int64, Int32, Ptr{Int64}, Ptr{Int32}, Int32, Int32, Ptr{Int64}, Ptr{Cvoid},
                Ptr{Int32}, Ptr{Cdouble}),
               b.device, samples, m, n, R, init, order, cap, maxsweeps, labels, runs, best, C_NULL)
    check(Ptr{Cvoid}(C_NULL), rc)
    info = (loss = [x.loss for x in runs], loss_num = [x.loss_num for x in runs], sweeps = [Int(x.sweeps) for x in runs],
            converged = [x.converged != 0 for x in runs], moves = [Int(x.moves) for x in runs], K = [Int(x.K) for x in runs],
            labels = labels, best = Int(best[1]) + 1)
    return (labels[:, best[1] + 1], info)
end

function searchexactid(b::HIPBackend, result, nruns::Integer, maxK::Integer, maxsweeps::Integer, seed::Integer)
    samples = samplematrix(result)
    n, m = size(samples)
    vi, _ = searchexactvi(b, result, nruns, maxK, maxsweeps, seed)
    R = Int(nruns) + 2
    init = zeros(Int64, n, R)                                     # column r = run r: row-major R×n for the library
    order = Matrix{Int32}(undef, n, R)
    rng = Random.MersenneTwister(seed)
    for r in 1:nruns
        order[:, r] .= Random.randperm(rng, n)
    end
    start, _ = getpointestimate_hip(result; loss = "ID", device = b.device)
    init[:, R - 1] .= start; order[:, R - 1] .= 1:n
    init[:, R] .= vi; order[:, R] .= 1:n
    cap = Int(maxK)
    if cap == 0                                                   # the library's default cap, widened to the starts' cluster counts
        lmax = maximum(length(unique(c)) for c in result.clusts)
        need = max(length(unique(start)), length(unique(vi)))
        cap = need > lmax ? need : 0
    end
    labels = Matrix{Int64}(undef, n, R)
    runs = Vector{RcPsmRun}(undef, R)
    best = Int32[0]
    rc = ccall((:rc_id_search, LIB), Int32,
               (Int32, Ptr{Int64}, Int64, Int64, Int32, Ptr{Int64}, Ptr{Int32}, Int32, Int32, Ptr{Int64}, Ptr{Cvoid},
                Ptr{Int32}, Ptr{Cdouble}),
               b.device, samples, m, n, R, init, order, cap, maxsweeps, labels, runs, best, C_NULL)
    check(Ptr{Cvoid}(C_NULL), rc)
    info = (loss = [x.loss for x in runs], loss_num = [x.loss_num for x in runs], sweeps = [Int(x.sweeps) for x in runs],
            converged = [x.converged != 0 for x in runs], moves = [Int(x.moves) for x in runs], K = [Int(x.K) for x in runs],
            labels = labels, best = Int(best[1]) + 1)
    return (labels[:, best[1] + 1], info)
end

export searchpointestimate, posteriorcounts

# rc_pear_run_t
struct RcPearRun
    pear::Cdouble
    num::Int64; den::Int64
    sweeps::Int32; converged::Int32
    moves::Int64
    K::Int32; pad_::Int32
end

# (num, den) of PEAR as Int128: num = 2(T·X − A·P), den = T(m·A + P) − 2·A·P, T = n(n−1)/2; (0, 1) where den = 0
function pearfraction(clust::AbstractVector{<:Integer}, counts::Matrix{UInt32}, numsamples::Integer)
    n = length(clust)
    size(counts) == (n, n) || throw(ArgumentError("counts must be an n×n matrix matching clust"))
    X = Int128(0); P = Int128(0)
    for j in 2:n, i in 1:j-1
        P += counts[i, j]
        clust[i] == clust[j] && (X += counts[i, j])
    end
    sizes = Dict{Int,Int}()
    for l in clust
        sizes[l] = get(sizes, l, 0) + 1
    end
    A = Int128(sum(s * (s - 1) ÷ 2 for s in values(sizes)))
    T = Int128(n) * (n - 1) ÷ 2
    den = T * (Int128(numsamples) * A + P) - 2 * A * P
    return den == 0 ? (Int128(0), Int128(1)) : (2 * (T * X - A * P), den)
end

"""
    expectedpear(clust, counts, numsamples) -> Float64

The posterior expected adjusted Rand index of `clust` in Fritsch & Ickstadt's form (mcclust's `pear`) from the n × n
co-clustering counts (`posteriorcounts`), evaluated as one exact ratio of two integers on the host; 0 where the denominator is 0.
What `searchmaxpear` maximises.
"""
function expectedpear(clust::AbstractVector{<:Integer}, counts::Matrix{UInt32}, numsamples::Integer)
    num, den = pearfraction(clust, counts, numsamples)
    return Float64(num) / Float64(den)
end

pearinfo(runs, labels, best) =
    (pear = [x.pear for x in runs], num = [x.num for x in runs], den = [x.den for x in runs], sweeps = [Int(x.sweeps) for x in runs],
     converged = [x.converged != 0 for x in runs], moves = [Int(x.moves) for x in runs], K = [Int(x.K) for x in runs],
     labels = labels, best = Int(best[1]) + 1)

# nruns Mersenne-Twister orders from empty labels, then one run per column of starts in the identity order
function pearruns(n, nruns, seed, starts)
    R = Int(nruns) + length(starts)
    R >= 1 || throw(ArgumentError("no run: nruns = 0 and no init"))
    inits = zeros(Int64, n, R)                                    # column r = run r: row-major R×n for the library
    order = Matrix{Int32}(undef, n, R)
    rng = Random.MersenneTwister(seed)
    for r in 1:nruns
        order[:, r] .= Random.randperm(rng, n)
    end
    for (k, s) in enumerate(starts)
        inits[:, nruns + k] .= s
        order[:, nruns + k] .= 1:n
    end
    return R, inits, order
end

"""
    searchmaxpear(HIPBackend(), result; nruns = 16, maxK = 0, maxsweeps = 100, seed = 0) -> (clust, info)
    searchmaxpear(HIPBackend(), counts, numsamples; nruns = 16, maxK = 0, maxsweeps = 100, seed = 0, init = nothing)

A greedy search over all partitions for the clustering of maximum posterior expected adjusted Rand index (`expectedpear`;
mcclust's `maxpear`, SALSO's `omARI.approx`) under the co-clustering counts (rc_pear_search_samples / rc_pear_search): every
comparison is an exact cross-multiplication of integers, so a run is a pure function of its inputs.  Runs: `nruns` from empty
labels in random point orders; with a `result`, one more from the sample of highest PEAR (mcclust's `method = "draws"`), so the
answer is never below the best sample; with counts, one per column of `init`.  `info`: named tuple of the per-run `pear`,
`num`, `den`, `sweeps`, `converged`, `moves`, `K`, all `labels` (n × runs) and `best` (the first run of maximal num/den).
"""
function searchmaxpear(b::HIPBackend, result; nruns::Integer = 16, maxK::Integer = 0, maxsweeps::Integer = 100, seed::Integer = 0)
    samples = samplematrix(result)                                # the counts are built from these on the device and stay there
    n, m = size(samples)
    counts = posteriorcounts(b, result)
    draw = 1
    bnum, bden = pearfraction(result.clusts[1], counts, m)
    for s in 2:m
        num, den = pearfraction(result.clusts[s], counts, m)
        if num * bden > bnum * den
            draw, bnum, bden = s, num, den
        end
    end
    R, inits, order = pearruns(n, nruns, seed, [result.clusts[draw]])
    cap = maxK == 0 ? 0 : max(Int(maxK), length(unique(result.clusts[draw])))
    labels = Matrix{Int64}(undef, n, R)
    runs = Vector{RcPearRun}(undef, R)
    best = Int32[0]
    rc = ccall((:rc_pear_search_samples, LIB), Int32,
               (Int32, Ptr{Int64}, Int64, Int64, Int32, Ptr{Int64}, Ptr{Int32}, Int32, Int32, Ptr{Int64}, Ptr{Cvoid},
                Ptr{Int32}, Ptr{Cdouble}, Ptr{Cdouble}),
               b.device, samples, m, n, R, inits, order, cap, maxsweeps, labels, runs, best, C_NULL, C_NULL)
    check(Ptr{Cvoid}(C_NULL), rc)
    return (labels[:, best[1] + 1], pearinfo(runs, labels, best))
end

function searchmaxpear(b::HIPBackend, counts::Matrix{UInt32}, numsamples::Integer; nruns::Integer = 16, maxK::Integer = 0,
                       maxsweeps::Integer = 100, seed::Integer = 0, init::Union{Matrix{Int64},Nothing} = nothing)
    n = size(counts, 1)
    size(counts, 2) == n || throw(ArgumentError("counts must be a square matrix"))
    starts = init === nothing ? Vector{Int64}[] : [init[:, k] for k in 1:size(init, 2)]
    R, inits, order = pearruns(n, nruns, seed, starts)
    labels = Matrix{Int64}(undef, n, R)
    runs = Vector{RcPearRun}(undef, R)
    best = Int32[0]
    rc = ccall((:rc_pear_search, LIB), Int32,
               (Int32, Ptr{Cvoid}, Int64, Int64, Int32, Ptr{Int64}, Ptr{Int32}, Int32, Int32, Ptr{Int64}, Ptr{Cvoid},
                Ptr{Int32}, Ptr{Cdouble}),
               b.device, counts, numsamples, n, R, inits, order, maxK, maxsweeps, labels, runs, best, C_NULL)
    check(Ptr{Cvoid}(C_NULL), rc)
    return (labels[:, best[1] + 1], pearinfo(runs, labels, best))
end

export searchmaxpear, expectedpear

# rc_hclust_merge_t
struct RcHclustMerge
    a::Int32; b::Int32
    size::Int32
    m_ab::UInt32
    s_ab::Int64
end

const HCLUST_LINKAGES = Dict("average" => 0, "complete" => 1, "single" => 2)

# the cut of minimum loss among K = 1..maxK (ties: the smaller K), its labels from the library's own rc_hclust_cut
function hclustchoose(merges, binder_num, vilb, n::Integer, m::Integer, loss::String, maxK::Integer, kernel_ms)
    pairs = n * (n - 1) ÷ 2
    losses = loss == "binder" ? [pairs == 0 ? 0.0 : binder_num[n - K + 1] / (m * pairs) for K in 1:maxK] : vilb
    K = loss == "binder" ? argmin([binder_num[n - K + 1] for K in 1:maxK]) : argmin(vilb)
    labels = Vector{Int64}(undef, n)
    rc = ccall((:rc_hclust_cut, LIB), Int32, (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}), merges, n, K, labels)
    check(Ptr{Cvoid}(C_NULL), rc)
    return (labels, (loss = losses, K = K, merges = merges[1:n-1], binder_num = binder_num, kernel_ms = kernel_ms[1]))
end

"""
    hclustpointestimate(HIPBackend(), counts, numsamples; loss = "VI", linkage = "average", maxK = 0) -> (clust, info)
    hclustpointestimate(HIPBackend(), result; loss = "VI", linkage = "average", maxK = 0) -> (clust, info)

The hierarchical point estimate (Medvedovic's method; mcclust's `minbinder` / mcclust.ext's `minVI` with `method = "avg"` /
`"comp"`): agglomerative clustering of the co-clustering counts on the GPU (rc_hclust, rc_hclust_samples), cut at the number
of clusters `K` in `1:maxK` of minimum expected loss, ties going to the smaller `K`.  `linkage`: "average", "complete" or
"single", on similarities; ties between pairs go to the smallest cluster name (its smallest member), then the smallest partner,
and every decision is exact integer arithmetic.  `loss`: "binder" (from the exact curve `info.binder_num`, index t + 1 = after t
merges) or "VI" (the lower bound, evaluated for every cut on the device).  `maxK = 0` means ⌈n/8⌉.  `info.merges` holds one
`RcHclustMerge` per step.
"""
function hclustpointestimate(b::HIPBackend, counts::Matrix{UInt32}, numsamples::Integer; loss::String = "VI",
                             linkage::String = "average", maxK::Integer = 0)
    loss in ("binder", "VI") || throw(ArgumentError("Invalid loss function specifier."))
    haskey(HCLUST_LINKAGES, linkage) || throw(ArgumentError("Invalid linkage specifier."))
    n = size(counts, 1)
    size(counts, 2) == n || throw(ArgumentError("counts must be a square matrix"))
    maxK = maxK == 0 ? cld(n, 8) : Int(maxK)
    1 <= maxK <= n || throw(ArgumentError("maxK must lie in 1:n"))
    merges = Vector{RcHclustMerge}(undef, max(n - 1, 1))
    binder_num = Vector{Int64}(undef, n)
    maxcut = loss == "VI" ? maxK : 0
    vilb = Vector{Cdouble}(undef, max(maxcut, 1))
    ms = Cdouble[0]
    rc = ccall((:rc_hclust, LIB), Int32,
               (Int32, Ptr{Cvoid}, Int64, Int64, Int32, Ptr{Cvoid}, Ptr{Int64}, Int32, Ptr{Cdouble}, Ptr{Cdouble}),
               b.device, counts, numsamples, n, HCLUST_LINKAGES[linkage], merges, binder_num, maxcut, vilb, ms)
    check(Ptr{Cvoid}(C_NULL), rc)
    return hclustchoose(merges, binder_num, vilb[1:maxcut], n, numsamples, loss, maxK, ms)
end

function hclustpointestimate(b::HIPBackend, result; loss::String = "VI", linkage::String = "average", maxK::Integer = 0)
    loss in ("binder", "VI") || throw(ArgumentError("Invalid loss function specifier."))
    haskey(HCLUST_LINKAGES, linkage) || throw(ArgumentError("Invalid linkage specifier."))
    samples = samplematrix(result)                                # the counts are built from these on the device and stay there
    n, m = size(samples)
    maxK = maxK == 0 ? cld(n, 8) : Int(maxK)
    1 <= maxK <= n || throw(ArgumentError("maxK must lie in 1:n"))
    merges = Vector{RcHclustMerge}(undef, max(n - 1, 1))
    binder_num = Vector{Int64}(undef, n)
    maxcut = loss == "VI" ? maxK : 0
    vilb = Vector{Cdouble}(undef, max(maxcut, 1))
    ms = Cdouble[0]
    rc = ccall((:rc_hclust_samples, LIB), Int32,
               (Int32, Ptr{Int64}, Int64, Int64, Int32, Ptr{Cvoid}, Ptr{Int64}, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
               b.device, samples, m, n, HCLUST_LINKAGES[linkage], merges, binder_num, maxcut, vilb, ms, C_NULL)
    check(Ptr{Cvoid}(C_NULL), rc)
    return hclustchoose(merges, binder_num, vilb[1:maxcut], n, m, loss, maxK, ms)
end

export hclustpointestimate

"""
    predict(HIPBackend(), result, Dnew; seed = 0) -> (labels, map_labels)

Allocate observations that were not in the fit to the clusters of every sample of `result` on the GPU (rc_predict): under
one sample, the Gibbs full conditional of an (n+1)-th point whose own cluster is empty, and a draw from it.  `Dnew` is q×n,
the distances of every new observation to every training observation (finite and positive).  `labels[i, s]` is the label new
point `i` drew under sample `s`, in that sample's own label names, `0` for a cluster of its own; `map_labels` holds the most
probable label instead.  New observations are allocated independently of each other given a sample.
"""
function predict(b::HIPBackend, result, Dnew::Matrix{Float64}; seed = 0)
    samples = samplematrix(result)
    n, m = size(samples)
    q = size(Dnew, 1)
    size(Dnew, 2) == n || throw(ArgumentError("Dnew must have one column per training observation."))
    rows = permutedims(Dnew)                                      # n×q column-major = q×n row-major
    r = Vector{Float64}(result.r); p = Vector{Float64}(result.p)
    labels = Matrix{Int64}(undef, q, m)                           # column s = sample s: row-major m×q for the library
    maplabels = Matrix{Int64}(undef, q, m)
    rc = ccall((:rc_predict, LIB), Int32,
               (Int32, Int64, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Ptr{Int64}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{RcParams},
                UInt64, UInt64, UInt64, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Cdouble}, Ptr{Int64}, Ptr{Int32}, Ptr{Int32},
                Ptr{Cdouble}),
               b.device, n, q, rows, C_NULL, m, samples, r, p, Ref(RcParams(result.params)), seed % UInt64, UInt64(0),
               UInt64(0), labels, maplabels, 0, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL)
    check(Ptr{Cvoid}(C_NULL), rc)
    return (labels, maplabels)
end

export predict

# include/redclust_hip.h's RC_METRIC_* by their names (SciPy's and Distances.jl's)
const METRICS = Dict(:euclidean => 0, :sqeuclidean => 1, :cityblock => 2, :chebyshev => 3, :cosine => 4, :correlation => 5)

function metric_code(metric, dim::Integer)
    haskey(METRICS, Symbol(metric)) || throw(ArgumentError("unknown metric $(metric): one of $(join(sort(collect(keys(METRICS))), ", "))"))
    (Symbol(metric) == :correlation && dim < 2) && throw(ArgumentError("the correlation metric needs dim >= 2."))
    return Int32(METRICS[Symbol(metric)])
end

"""
    pairwise(HIPBackend(), points[, new_points]; metric = :euclidean)

The raw distances as the device computes them (rc_pairwise), in the arithmetic the header states for each metric: the
symmetric n×n matrix of the n×dim `points` with a zero diagonal, or, with `new_points` (q×dim), the q×n matrix of new point
against training point.  Nothing about the values is refused.
"""
function pairwise(b::HIPBackend, points::Matrix{Float64}, new_points::Union{Matrix{Float64},Nothing} = nothing; metric = :euclidean)
    n, dim = size(points)
    code = metric_code(metric, dim)
    X = permutedims(points)                                       # dim×n column-major = n×dim row-major
    ms = Cdouble[0]
    if new_points === nothing
        out = Matrix{Float64}(undef, n, n)                        # symmetric: column-major == row-major
        rc = ccall((:rc_pairwise, LIB), Int32,
                   (Int32, Int32, Int64, Int64, Ptr{Cdouble}, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                   b.device, code, n, dim, X, 0, C_NULL, out, ms)
        check(Ptr{Cvoid}(C_NULL), rc)
        return out
    end
    size(new_points, 2) == dim || throw(ArgumentError("new_points must have the dimension of points."))
    q = size(new_points, 1)
    Y = permutedims(new_points)
    out = Matrix{Float64}(undef, n, q)                            # n×q column-major = q×n row-major
    rc = ccall((:rc_pairwise, LIB), Int32,
               (Int32, Int32, Int64, Int64, Ptr{Cdouble}, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
               b.device, code, n, dim, X, q, Y, out, ms)
    check(Ptr{Cvoid}(C_NULL), rc)
    return permutedims(out)
end

export pairwise

"""
    predict_points(HIPBackend(), result, points, new_points; relabelling = nothing, seed = 0, metric = :euclidean)

Allocate any number of new observations given by their coordinates to the clusters of every sample of `result` on the GPU
(rc_predict_points): `points` is n×dim, the training observations one per row, `new_points` q×dim.  The distances (direct
differences, one fused multiply-add per coordinate, a correctly rounded root), their logarithms and the quantisation are taken
on the device, and the samples are uploaded once.  Without `relabelling` it returns `(labels, map_labels)` as `predict`.  With
`relabelling` (what `relabel(HIPBackend(), result, pivot)` returned for the same samples) it returns
`(counts = …, map_counts = …, pivot_labels = …)`: `counts[i, k]`, k = 1..K_p+1, is the number of samples in which new
observation `i`'s draw lands in the pivot's cluster `pivot_labels[k-1]` (column 1: a cluster of its own, or one without a
counterpart); nothing of size m×q leaves the device.  `metric`: the distance (a name of `METRICS`), the one the training
matrix was made in (rc_predict_points_metric; `:euclidean` is rc_predict_points' own arithmetic).
"""
function predict_points(b::HIPBackend, result, points::Matrix{Float64}, new_points::Matrix{Float64}; relabelling = nothing, seed = 0,
                        metric = :euclidean)
    samples = samplematrix(result)
    n, m = size(samples)
    dim = size(points, 2)
    q = size(new_points, 1)
    size(points, 1) == n || throw(ArgumentError("points must have one row per training observation."))
    size(new_points, 2) == dim || throw(ArgumentError("new_points must have the dimension of points."))
    code = metric_code(metric, dim)
    X = permutedims(points)                                       # dim×n column-major = n×dim row-major
    Y = permutedims(new_points)
    r = Vector{Float64}(result.r); p = Vector{Float64}(result.p)
    ms = Cdouble[0]
    if relabelling === nothing
        labels = Matrix{Int64}(undef, q, m)                       # column s = sample s: row-major m×q for the library
        maplabels = Matrix{Int64}(undef, q, m)
        rc = ccall((:rc_predict_points_metric, LIB), Int32,
                   (Int32, Int32, Int64, Int64, Ptr{Cdouble}, Int64, Ptr{Cdouble}, Int64, Ptr{Int64}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{RcParams},
                    UInt64, UInt64, UInt64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Int64}, Int64, Ptr{Cvoid}, Ptr{Cvoid},
                    Int64, Ptr{Cdouble}, Ptr{Int64}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Ptr{Int32}, Ptr{Cdouble}),
                   code, b.device, n, dim, X, q, Y, m, samples, r, p, Ref(RcParams(result.params)), seed % UInt64, UInt64(0), UInt64(0),
                   labels, maplabels, C_NULL, 0, C_NULL, 0, C_NULL, C_NULL, 0, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, ms)
        check(Ptr{Cvoid}(C_NULL), rc)
        return (labels, maplabels)
    end
    names = Vector{Int64}(relabelling.pivot_labels)
    Kp = length(names)
    col = Dict(l => k for (k, l) in enumerate(names))             # the library wants pivot labels in 1..n: pass the columns
    maps = permutedims(map(l -> l > 0 ? Int64(col[l]) : Int64(l), relabelling.maps))      # W×m column-major = m×W row-major
    cols = Vector{Int64}(1:Kp)
    counts = Matrix{UInt32}(undef, Kp + 1, q)                     # row-major q×(K_p+1)
    mapcounts = Matrix{UInt32}(undef, Kp + 1, q)
    rc = ccall((:rc_predict_points_metric, LIB), Int32,
               (Int32, Int32, Int64, Int64, Ptr{Cdouble}, Int64, Ptr{Cdouble}, Int64, Ptr{Int64}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{RcParams},
                UInt64, UInt64, UInt64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Int64}, Int64, Ptr{Cvoid}, Ptr{Cvoid},
                Int64, Ptr{Cdouble}, Ptr{Int64}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Ptr{Int32}, Ptr{Cdouble}),
               code, b.device, n, dim, X, q, Y, m, samples, r, p, Ref(RcParams(result.params)), seed % UInt64, UInt64(0), UInt64(0),
               C_NULL, C_NULL, maps, size(maps, 1), cols, Kp, counts, mapcounts, 0, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, ms)
    check(Ptr{Cvoid}(C_NULL), rc)
    return (counts = permutedims(counts), map_counts = permutedims(mapcounts), pivot_labels = names, kernel_ms = ms[1])
end

export predict_points

"""
    predict_joint(HIPBackend(), result, Dnew, Dnn; sweeps = 2, seed = 0) -> (labels, first_labels, K, moves)

Allocate new observations to the clusters of every sample of `result` jointly, on the GPU (rc_predict_joint): under one sample
the new observations are allocated one after the other in the order given, each seeing the training labels and the new
observations before it, and then visited again in `sweeps` Gibbs passes, so that new observations may form clusters with each
other.  `Dnew` is q×n as for `predict`; `Dnn` is q×q, symmetric, the distances among the new observations (the diagonal is
ignored).  `labels[i, s]` is the final label of new point `i` under sample `s` in that sample's own names — a cluster that new
points opened carries a label of 1..n+q the sample did not use, so `vcat(sample, labels[:, s])` is a labelling of n+q points;
`first_labels` holds the labels after the sequential pass, `K[s]` the clusters of the extended sample, `moves[pass, s]` the
visits of each pass whose draw changed the point's label.  A sample's clusters and `q` must fit 4096 slots together.
"""
function predict_joint(b::HIPBackend, result, Dnew::Matrix{Float64}, Dnn::Matrix{Float64}; sweeps = 2, seed = 0)
    samples = samplematrix(result)
    n, m = size(samples)
    q = size(Dnew, 1)
    size(Dnew, 2) == n || throw(ArgumentError("Dnew must have one column per training observation."))
    size(Dnn) == (q, q) || throw(ArgumentError("Dnn must be q×q."))
    sweeps >= 0 || throw(ArgumentError("sweeps must be non-negative."))
    rows = permutedims(Dnew)                                      # n×q column-major = q×n row-major
    rowsn = permutedims(Dnn)
    r = Vector{Float64}(result.r); p = Vector{Float64}(result.p)
    labels = Matrix{Int64}(undef, q, m)                           # column s = sample s: row-major m×q for the library
    first = Matrix{Int64}(undef, q, m)
    K = Vector{Int64}(undef, m)
    moves = Matrix{Int64}(undef, sweeps + 1, m)
    rc = ccall((:rc_predict_joint, LIB), Int32,
               (Int32, Int64, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Ptr{Int64}, Ptr{Cdouble},
                Ptr{Cdouble}, Ref{RcParams}, Int64, UInt64, UInt64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64},
                Ptr{Int32}, Ptr{Int32}, Ptr{Cdouble}),
               b.device, n, q, rows, rowsn, C_NULL, C_NULL, m, samples, r, p, Ref(RcParams(result.params)), sweeps,
               seed % UInt64, UInt64(0), labels, first, K, moves, C_NULL, C_NULL, C_NULL, C_NULL)
    check(Ptr{Cvoid}(C_NULL), rc)
    return (labels, first, K, moves)
end

export predict_joint

const DISTANCE_LOSSES = ("binder", "VI", "ID")

"""
    partitiondistances(HIPBackend(), labellings, result; loss = "VI") -> (dist, info)

The distance from each of `L` labellings (a vector of label vectors) to each of the `m` samples of `result`, on the GPU in
exact integers (rc_partition_distances).  `loss`: "binder" (normalised, as `binderloss`), "VI" or "ID" (nats, as
`infodist(...; normalised = false)`).  `dist` is L×m; `info.num` holds the integer numerators it was divided from once —
Binder: disagreeing pairs; VI, ID: units of 2^-32/n nats, VI_q = A_q + B_q − 2T and ID_q = max(A_q, B_q) − T with the
library's fixed-point table — and `info.K_labellings`, `info.K_samples` the cluster counts.
"""
function partitiondistances(b::HIPBackend, labellings::Vector{<:AbstractVector{<:Integer}}, result; loss::String = "VI")
    loss in DISTANCE_LOSSES || throw(ArgumentError("Invalid loss function specifier."))
    samples = samplematrix(result)
    n, m = size(samples)
    L = length(labellings)
    labels = Matrix{Int64}(undef, n, L)                           # column l = labelling l: row-major L×n for the library
    for l in 1:L
        length(labellings[l]) == n || throw(ArgumentError("Length of the input vectors must be equal."))
        labels[:, l] .= labellings[l]
    end
    part = Matrix{Int64}(undef, m, L)                             # P for "binder", T otherwise: row-major L×m
    labmarg = Matrix{Int64}(undef, 3, L); smpmarg = Matrix{Int64}(undef, 3, m)
    ms = Cdouble[0]
    rc = ccall((:rc_partition_distances, LIB), Int32,
               (Int32, Ptr{Int64}, Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Cdouble}),
               b.device, samples, m, n, L, labels, loss == "binder" ? part : C_NULL, loss == "binder" ? C_NULL : part,
               labmarg, smpmarg, ms)
    check(Ptr{Cvoid}(C_NULL), rc)
    row = loss == "binder" ? 1 : 2
    num = Matrix{Int64}(undef, L, m)
    for l in 1:L, s in 1:m
        a, c, t = labmarg[row, l], smpmarg[row, s], part[s, l]
        num[l, s] = loss == "binder" ? (a + c - 2t) ÷ 2 : loss == "VI" ? a + c - 2t : max(a, c) - t
    end
    den = loss == "binder" ? n * (n - 1) ÷ 2 : 2.0^32 * n
    dist = den == 0 ? zeros(L, m) : num ./ den
    return (dist, (num = num, K_labellings = labmarg[3, :], K_samples = smpmarg[3, :], kernel_ms = ms[1]))
end

"""
    credibleball(HIPBackend(), clust, result; loss = "VI", alpha = 0.05)

The (1 − alpha) credible ball around the point estimate `clust` (Wade & Ghahramani 2018; mcclust.ext's `credibleball`), from
the exact integer distances of `partitiondistances`: with k = m − ⌊alpha·m + 1e-9⌋, `epsilon` is the k-th smallest distance
and the ball is every sample within it (ties at the radius are in).  `horizontal`: the ball's samples at distance epsilon;
`upper` / `lower`: among the ball's samples with the fewest / most clusters, those of greatest distance.  Returns a named
tuple: epsilon, epsilon_num, level, ball, distances, distances_num, K, and per bound `<name>_index` (ascending sample indices)
and `<name>` (the distinct partitions among them, sortlabels'd, in order of first occurrence).
"""
function credibleball(b::HIPBackend, clust::AbstractVector{<:Integer}, result; loss::String = "VI", alpha::Real = 0.05)
    0 <= alpha < 1 || throw(ArgumentError("alpha must lie in [0, 1)"))
    dist, info = partitiondistances(b, [clust], result; loss = loss)
    num = info.num[1, :]; K = info.K_samples
    m = length(num)
    k = m - floor(Int, alpha * m + 1e-9)
    eps_num = sort(num)[k]
    ball = num .<= eps_num
    farthest(mask) = (far = maximum(num[mask]); findall(mask .& (num .== far)))
    index = (horizontal = findall(ball .& (num .== eps_num)), upper = farthest(ball .& (K .== minimum(K[ball]))),
             lower = farthest(ball .& (K .== maximum(K[ball]))))
    parts(idx) = unique([RedClust.sortlabels(result.clusts[s]) for s in idx])
    n = length(clust)
    den = loss == "binder" ? n * (n - 1) ÷ 2 : 2.0^32 * n
    return (epsilon = den == 0 ? 0.0 : eps_num / den, epsilon_num = eps_num, level = count(ball) / m, ball = ball,
            distances = dist[1, :], distances_num = num, K = K,
            horizontal_index = index.horizontal, upper_index = index.upper, lower_index = index.lower,
            horizontal = parts(index.horizontal), upper = parts(index.upper), lower = parts(index.lower))
end

export partitiondistances, credibleball

"""
    relabel(HIPBackend(), result, pivot) -> (labels, maps, overlap, counts, pivot_labels, kernel_ms)

Rename every sample of `result` onto the labelling `pivot` (a point estimate, say) on the GPU in exact integers (rc_relabel):
each sample's clusters are matched to the pivot's so that the number of points on which the two agree is largest, by shortest
augmenting paths with the library's fixed tie rule (the smallest column id among equal reduced costs), so the matching is a
function of the inputs.  `labels` is m×n in the pivot's names (0: the sample's cluster has no counterpart), `maps[s, t]` the
pivot label that the t-th smallest label of sample s is sent to (0 unmatched, −1 past its clusters), `overlap[s]` the number of
points on which the renamed sample agrees with the pivot, and `counts[j, k]`, k = 1..K_p+1, the number of samples in which
point j lands in the pivot's cluster `pivot_labels[k-1]` (column 1: unmatched); `counts ./ m` are allocation probabilities.
"""
function relabel(b::HIPBackend, result, pivot::AbstractVector{<:Integer})
    samples = samplematrix(result)
    n, m = size(samples)
    length(pivot) == n || throw(ArgumentError("Length of the input vectors must be equal."))
    piv = Vector{Int64}(pivot)
    names = sort(unique(piv))
    Kp = length(names)
    W = maximum(length(unique(view(samples, :, s))) for s in 1:m)
    labels = Matrix{Int64}(undef, n, m)                           # column s = sample s: row-major m×n for the library
    maps = Matrix{Int64}(undef, W, m)
    overlap = Vector{Int64}(undef, m)
    counts = Matrix{UInt32}(undef, Kp + 1, n)                     # row-major n×(K_p+1)
    ms = Cdouble[0]
    rc = ccall((:rc_relabel, LIB), Int32,
               (Int32, Ptr{Int64}, Int64, Int64, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Cvoid}, Ptr{Cdouble}),
               b.device, samples, m, n, piv, Kp, labels, maps, W, overlap, counts, ms)
    check(Ptr{Cvoid}(C_NULL), rc)
    return (labels = permutedims(labels), maps = permutedims(maps), overlap = overlap, counts = permutedims(counts),
            pivot_labels = names, kernel_ms = ms[1])
end

export relabel

"""
    scorelabellings(HIPBackend(), data, labellings, params; r = nothing, p = nothing) -> (loglik, logprior, logposterior, K, kernel_ms)

The log-likelihood of each of `L` labellings (a vector of label vectors, or the `clusts` of a result) under the model with
hyperparameters `params`, on the GPU (rc_score_labellings): one pass over the matrices for the whole batch, the K×K block
sums of D and log D of every labelling in exact integers, the scalar part in extended precision.  With `r` and `p` (scalars
or one per labelling) the log-prior and the log-posterior as well; they are `nothing` otherwise.
"""
function scorelabellings(b::HIPBackend, data::MCMCData, labellings::Vector{<:AbstractVector{<:Integer}},
                         params::PriorHyperparamsList; r = nothing, p = nothing)
    n = size(data.D, 1)
    L = length(labellings)
    labels = Matrix{Int64}(undef, n, L)                           # column l = labelling l: row-major L×n for the library
    for l in 1:L
        length(labellings[l]) == n || throw(ArgumentError("Length of the input vectors must be equal."))
        labels[:, l] .= labellings[l]
    end
    (r === nothing) == (p === nothing) || throw(ArgumentError("Give both r and p, or neither."))
    withprior = r !== nothing
    rv = withprior ? (r isa Real ? fill(Float64(r), L) : Vector{Float64}(r)) : Float64[]
    pv = withprior ? (p isa Real ? fill(Float64(p), L) : Vector{Float64}(p)) : Float64[]
    !withprior || (length(rv) == L && length(pv) == L) || throw(ArgumentError("r and p must hold one value per labelling."))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:rc_create, LIB), Int32,
               (Int64, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Int32, Int64, Ref{Ptr{Cvoid}}),
               n, data.D, Ptr{Cdouble}(C_NULL), 64, b.device, 0, h)
    check(Ptr{Cvoid}(C_NULL), rc)
    ctx = h[]
    loglik = Vector{Float64}(undef, L); logprior = Vector{Float64}(undef, L); K = Vector{Int64}(undef, L)
    ms = Cdouble[0]
    try
        rc = GC.@preserve rv pv logprior ccall((:rc_score_labellings, LIB), Int32,
                   (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{RcParams}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int64},
                    Ptr{Int64}, Int64, Ptr{Int32}, Ptr{Int32}, Ptr{Cdouble}),
                   ctx, L, labels, withprior ? pointer(rv) : Ptr{Cdouble}(C_NULL), withprior ? pointer(pv) : Ptr{Cdouble}(C_NULL),
                   Ref(RcParams(params)), loglik, withprior ? pointer(logprior) : Ptr{Cdouble}(C_NULL), K, C_NULL, 0, C_NULL, C_NULL, ms)
        check(ctx, rc)
    finally
        ccall((:rc_destroy, LIB), Int32, (Ptr{Cvoid},), ctx)
    end
    return (loglik = loglik, logprior = withprior ? logprior : nothing, logposterior = withprior ? loglik .+ logprior : nothing,
            K = K, kernel_ms = ms[1])
end

scorelabellings(b::HIPBackend, data::MCMCData, result::MCMCResult, params::PriorHyperparamsList = result.params) =
    scorelabellings(b, data, [Vector{Int64}(c) for c in result.clusts], params; r = result.r, p = result.p)

"""
    mapestimate(HIPBackend(), data, candidates, params; r, p) -> (clust, info)

The candidate labelling of highest log-posterior under the model (the first of equals), with the scores of all of them:
`info.index`, `info.loglik`, `info.logprior`, `info.logposterior`, `info.K`.  `r` and `p` are scalars or one per candidate.
"""
function mapestimate(b::HIPBackend, data::MCMCData, candidates::Vector{<:AbstractVector{<:Integer}},
                     params::PriorHyperparamsList; r, p)
    sc = scorelabellings(b, data, candidates, params; r = r, p = p)
    best = argmax(sc.logposterior)                                # the first maximum
    return (Vector{Int64}(candidates[best]), (index = best, loglik = sc.loglik, logprior = sc.logprior,
                                              logposterior = sc.logposterior, K = sc.K, kernel_ms = sc.kernel_ms))
end

export scorelabellings, mapestimate

struct RcMapRun                      # struct rc_map_run_t
    loglik::Cdouble; logprior::Cdouble; logposterior::Cdouble
    start_logposterior::Cdouble
    sweeps::Int32; converged::Int32; K::Int32; capped::Int32
    moves::Int64
end

"""
    searchmapestimate(HIPBackend(), data, candidates, params; r, p, nruns = 16, maxK = 0, maxsweeps = 100, seed = 0, init = nothing) -> (clust, info)

Search ALL partitions for the labelling of maximum log-posterior (rc_map_search): a one-point-at-a-time climb of
loglik + logprior from the `nruns` distinct candidates of highest log-posterior, each under its own `r` and `p` (scalars or one
per candidate), from every column of `init` (an n × k matrix of labels, 0 = unallocated) and from empty labels, these under the
best candidate's pair.  The moves are decided in Float64 on exact integer block sums; everything reported is
rc_score_labellings' value of the labelling it belongs to.  Never worse than `mapestimate` on the same candidates: when no run
beats the best candidate, that candidate is returned and `info.best` is 0.  `info`: `index` (the best candidate),
`candidate_logposterior`, and per run `start_logposterior` (NaN for a start with unallocated points), `logposterior`, `loglik`,
`logprior`, `sweeps`, `converged`, `moves`, `K`, `capped`, all `labels` (n × runs), `runs` (the starts), `best`, `kernel_ms`.
"""
function searchmapestimate(b::HIPBackend, data::MCMCData, candidates::Vector{<:AbstractVector{<:Integer}},
                           params::PriorHyperparamsList; r, p, nruns::Integer = 16, maxK::Integer = 0, maxsweeps::Integer = 100,
                           seed::Integer = 0, init::Union{Matrix{Int64},Nothing} = nothing)
    n = size(data.D, 1)
    L = length(candidates)
    L >= 1 || throw(ArgumentError("No candidates."))
    sc = scorelabellings(b, data, candidates, params; r = r, p = p)
    rv = r isa Real ? fill(Float64(r), L) : Vector{Float64}(r)
    pv = p isa Real ? fill(Float64(p), L) : Vector{Float64}(p)
    top = argmax(sc.logposterior)                                 # the first maximum
    starts = Vector{Vector{Int64}}(); rs = Float64[]; ps = Float64[]
    seen = Set{Vector{Int64}}()
    for c in sortperm(sc.logposterior; rev = true, alg = MergeSort)   # the highest first, the smaller index on ties
        length(starts) == nruns && break
        key = Vector{Int64}(RedClust.sortlabels(Vector{Int64}(candidates[c])))
        key in seen && continue
        push!(seen, key)
        push!(starts, Vector{Int64}(candidates[c])); push!(rs, rv[c]); push!(ps, pv[c])
    end
    if init !== nothing
        size(init, 1) == n || throw(ArgumentError("Every labelling in init must have n entries."))
        for k in 1:size(init, 2)
            push!(starts, init[:, k]); push!(rs, rv[top]); push!(ps, pv[top])
        end
    end
    push!(starts, zeros(Int64, n)); push!(rs, rv[top]); push!(ps, pv[top])
    R = length(starts)
    initm = Matrix{Int64}(undef, n, R)                            # column q = run q: row-major R×n for the library
    order = Matrix{Int32}(undef, n, R)
    rng = Random.MersenneTwister(seed)
    for q in 1:R
        initm[:, q] .= starts[q]
        order[:, q] .= Random.randperm(rng, n)                    # every run in a permutation of its own, drawn in run order
    end
    labels = Matrix{Int64}(undef, n, R)
    runs = Vector{RcMapRun}(undef, R)
    best = Int32[0]
    ms = Cdouble[0]
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:rc_create, LIB), Int32,
               (Int64, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Int32, Int64, Ref{Ptr{Cvoid}}),
               n, data.D, Ptr{Cdouble}(C_NULL), 64, b.device, 0, h)
    check(Ptr{Cvoid}(C_NULL), rc)
    ctx = h[]
    try
        rc = ccall((:rc_map_search, LIB), Int32,
                   (Ptr{Cvoid}, Int32, Ptr{Int64}, Ptr{Int32}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{RcParams}, Int32, Int32, Ptr{Int64},
                    Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Int32}, Ptr{Cdouble}),
                   ctx, R, initm, order, rs, ps, Ref(RcParams(params)), maxK, maxsweeps, labels, runs, C_NULL, C_NULL, best, ms)
        check(ctx, rc)
    finally
        ccall((:rc_destroy, LIB), Int32, (Ptr{Cvoid},), ctx)
    end
    w = Int(best[1]) + 1
    beaten = runs[w].logposterior > sc.logposterior[top]
    info = (index = top, candidate_logposterior = sc.logposterior, start_logposterior = [x.start_logposterior for x in runs],
            logposterior = [x.logposterior for x in runs], loglik = [x.loglik for x in runs], logprior = [x.logprior for x in runs],
            sweeps = [Int(x.sweeps) for x in runs], converged = [x.converged != 0 for x in runs], moves = [Int(x.moves) for x in runs],
            K = [Int(x.K) for x in runs], capped = [Int(x.capped) for x in runs], labels = labels, runs = initm,
            best = beaten ? w : 0, kernel_ms = ms[1])
    return (beaten ? labels[:, w] : Vector{Int64}(candidates[top]), info)
end

export searchmapestimate

"""
    clusterprofiles(HIPBackend(), data, labellings; points = true) -> (K, medoids, medoid_within, within, nearest, neighbour, silhouette, eD, kernel_ms)

The medoids, silhouette widths and neighbour clusters of each of `L` labellings (a vector of label vectors) against the
dissimilarities of `data`, on the GPU (rc_cluster_profiles), in exact integers of `Dq = D·2^eD`; the diagonal never counts.
With the clusters of a labelling in ascending label order: `medoids[l][k]` is the member of cluster `k` with the least
`within` (the sum of its distances to the other members), the smallest index on ties, and `medoid_within[l][k]` that sum.
Per point (`L×n`, or `nothing` with `points = false`): `within`; `neighbour`, the label of the other cluster of least mean
distance — means compared exactly, the smaller label on ties, 0 with one cluster — and `nearest`, the sum of the distances to
its members; `silhouette = (b̄ − ā)/max(ā, b̄)` with `ā = within/(n_A − 1)` and `b̄ = nearest/n_neighbour`, 0 for a singleton,
for one cluster and when `max(ā, b̄) = 0`.
"""
function clusterprofiles(b::HIPBackend, data::MCMCData, labellings::Vector{<:AbstractVector{<:Integer}}; points::Bool = true)
    n = size(data.D, 1)
    L = length(labellings)
    labels = Matrix{Int64}(undef, n, L)                           # column l = labelling l: row-major L×n for the library
    for l in 1:L
        length(labellings[l]) == n || throw(ArgumentError("Length of the input vectors must be equal."))
        labels[:, l] .= labellings[l]
    end
    Ks = [length(unique(labellings[l])) for l in 1:L]
    ktot = sum(Ks)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:rc_create, LIB), Int32,
               (Int64, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Int32, Int64, Ref{Ptr{Cvoid}}),
               n, data.D, Ptr{Cdouble}(C_NULL), 64, b.device, 0, h)
    check(Ptr{Cvoid}(C_NULL), rc)
    ctx = h[]
    K = Vector{Int64}(undef, L); med = Vector{Int64}(undef, ktot); medw = Vector{Int64}(undef, ktot)
    within = Matrix{Int64}(undef, n, points ? L : 0); nearest = similar(within); neighbour = similar(within)
    eD = Int32[0]; ms = Cdouble[0]
    try
        rc = GC.@preserve within nearest neighbour ccall((:rc_cluster_profiles, LIB), Int32,
                   (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64},
                    Ptr{Int32}, Ptr{Cdouble}),
                   ctx, L, labels, K, med, medw, ktot, points ? pointer(within) : Ptr{Int64}(C_NULL),
                   points ? pointer(nearest) : Ptr{Int64}(C_NULL), points ? pointer(neighbour) : Ptr{Int64}(C_NULL), eD, ms)
        check(ctx, rc)
    finally
        ccall((:rc_destroy, LIB), Int32, (Ptr{Cvoid},), ctx)
    end
    off = cumsum([0; Ks])
    medoids = [med[off[l]+1:off[l+1]] for l in 1:L]
    medoid_within = [medw[off[l]+1:off[l+1]] for l in 1:L]
    points || return (K = K, medoids = medoids, medoid_within = medoid_within, within = nothing, nearest = nothing,
                      neighbour = nothing, silhouette = nothing, eD = eD[1], kernel_ms = ms[1])
    sil = zeros(Float64, L, n)
    for l in 1:L
        z = labellings[l]
        sizes = Dict{Int64,Int}()
        for x in z
            sizes[x] = get(sizes, x, 0) + 1
        end
        for i in 1:n
            na = sizes[z[i]]
            (na > 1 && neighbour[i, l] > 0) || continue
            a = within[i, l] / (na - 1); bb = nearest[i, l] / sizes[neighbour[i, l]]
            hi = max(a, bb)
            sil[l, i] = hi > 0 ? (bb - a) / hi : 0.0
        end
    end
    return (K = K, medoids = medoids, medoid_within = medoid_within, within = permutedims(within), nearest = permutedims(nearest),
            neighbour = permutedims(neighbour), silhouette = sil, eD = eD[1], kernel_ms = ms[1])
end

clusterprofiles(b::HIPBackend, data::MCMCData, result::MCMCResult; points::Bool = true) =
    clusterprofiles(b, data, [Vector{Int64}(c) for c in result.clusts]; points = points)

export clusterprofiles

"""
    visearchgroups(HIPBackend(), result, group, inits, orders, rungroup; maxK = 0, maxsweeps = 100) -> info

Many exact expected-VI searches in one launch (rc_vi_search_groups): run r searches all partitions for the minimum expected VI
over the samples s of `result` with `group[s] == rungroup[r]` (groups 0-based as in the library, -1 = in no group), from the
labels `inits[r]` (0 = unallocated) in the order `orders[r]` (a permutation of 1:n) — bit for bit rc_vi_search on that
sub-array.  `info.best[g + 1]` is the 1-based run of least `loss_num` of group g, 0 where no run searches it.
"""
function visearchgroups(b::HIPBackend, result, group::AbstractVector{<:Integer}, inits::Vector{<:AbstractVector{<:Integer}},
                        orders::Vector{<:AbstractVector{<:Integer}}, rungroup::AbstractVector{<:Integer};
                        maxK::Integer = 0, maxsweeps::Integer = 100)
    samples = samplematrix(result)
    n, m = size(samples)
    R = length(inits)
    (length(orders) == R && length(rungroup) == R) || throw(ArgumentError("inits, orders and rungroup must have one entry per run"))
    length(group) == m || throw(ArgumentError("group must hold one group id per sample"))
    init = Matrix{Int64}(undef, n, R); order = Matrix{Int32}(undef, n, R)   # column r = run r: row-major R×n for the library
    for r in 1:R
        init[:, r] .= inits[r]; order[:, r] .= orders[r]
    end
    grp = Vector{Int32}(group); rg = Vector{Int32}(rungroup)
    ngroups = max(Int(maximum(grp)) + 1, 1)
    labels = Matrix{Int64}(undef, n, R)
    runs = Vector{RcPsmRun}(undef, R)
    best = fill(Int32(-1), ngroups)
    ms = Cdouble[0]
    rc = ccall((:rc_vi_search_groups, LIB), Int32,
               (Int32, Ptr{Int64}, Int64, Int64, Ptr{Int32}, Int32, Int32, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}, Int32, Int32,
                Ptr{Int64}, Ptr{Cvoid}, Ptr{Int32}, Ptr{Cdouble}),
               b.device, samples, m, n, grp, ngroups, R, rg, init, order, maxK, maxsweeps, labels, runs, best, ms)
    check(Ptr{Cvoid}(C_NULL), rc)
    return (loss = [x.loss for x in runs], loss_num = [x.loss_num for x in runs], sweeps = [Int(x.sweeps) for x in runs],
            converged = [x.converged != 0 for x in runs], moves = [Int(x.moves) for x in runs], K = [Int(x.K) for x in runs],
            labels = labels, best = Int.(best) .+ 1, kernel_ms = ms[1])
end

# every sample to its nearest particle (ties: the lowest index): (assignment, the samples' distances, W)
function wasabiassign(num::Matrix{Int64})
    L, m = size(num)
    a = [argmin(view(num, :, s)) for s in 1:m]
    d = [num[a[s], s] for s in 1:m]
    return (a, d, sum(Int128.(d)))
end

# the unused sample of greatest positive distance, ties to the lowest index; 0 when there is none
function wasabifarthest(d::Vector{Int64}, used::Set{Int})
    best = 0
    for s in eachindex(d)
        (s in used || d[s] <= 0) && continue
        (best == 0 || d[s] > d[best]) && (best = s)
    end
    return best
end

"""
    wasabi(HIPBackend(), result, L; nstarts = 4, maxiter = 50, nruns = 1, maxK = 0, maxsweeps = 100, seed = 0)

Summarise the samples of `result` by `L` weighted partitions that minimise the Wasserstein distance to the sample distribution
with VI as ground metric (Balocchi & Wade's WASABI): the loop of the Python package's `wasabi` (DESIGN.md §8 "Several-partition
summary") on `partitiondistances` and `visearchgroups` — assignment to the nearest particle, repair of empty groups by the
farthest samples, one grouped exact-VI search per iteration, the start of least final W.  The random draws are Julia's
(`MersenneTwister(seed)`: the `nruns` orders first, then per start the L seeding draws), not NumPy's Philox, so the two
languages agree in law, not draw by draw.  Returns a named tuple: particles (by descending weight), weights, assignment,
group_num, objective_num, wasserstein, trace, iterations, converged, start, starts.
"""
function wasabi(b::HIPBackend, result, L::Integer; nstarts::Integer = 4, maxiter::Integer = 50, nruns::Integer = 1,
                maxK::Integer = 0, maxsweeps::Integer = 100, seed::Integer = 0)
    (L >= 1 && nstarts >= 1 && maxiter >= 1) || throw(ArgumentError("L, nstarts and maxiter must be at least 1"))
    S = [Vector{Int64}(c) for c in result.clusts]
    m = length(S); n = length(S[1])
    cap = maxK > 0 ? Int(maxK) : maximum(length(unique(c)) for c in S)
    rng = Random.MersenneTwister(seed)
    orders = [Vector{Int32}(Random.randperm(rng, n)) for _ in 1:nruns]
    dist(P) = partitiondistances(b, P, result; loss = "VI")[2].num
    runs = []
    for t in 1:nstarts
        # k-medoids++ on partition space
        chosen = [rand(rng, 1:m)]
        dmin = dist([S[chosen[1]]])[1, :]
        for j in 2:L
            W = sum(Int128.(dmin))
            W == 0 && break
            thr = (Int128(rand(rng, UInt64) >> 11) * W) >> 53
            acc = Int128(0); idx = m
            for s in 1:m
                acc += dmin[s]
                if acc > thr
                    idx = s
                    break
                end
            end
            push!(chosen, idx)
            dmin = min.(dmin, dist([S[idx]])[1, :])
        end
        P = [Vector{Int64}(RedClust.sortlabels(S[i])) for i in chosen]
        # the iteration
        trace = Int128[]; prev = nothing; converged = false; it = 0
        a, d, W = wasabiassign(dist(P)); push!(trace, W)
        while it < maxiter
            it += 1
            repaired = false
            empty = [l for l in eachindex(P) if !(l in a)]
            if !isempty(empty)
                W == 0 && break
                used = Set{Int}()
                for l in empty
                    s = wasabifarthest(d, used)
                    s == 0 && break
                    push!(used, s)
                    P[l] = Vector{Int64}(RedClust.sortlabels(S[s])); repaired = true
                end
                if repaired
                    a, d, W = wasabiassign(dist(P)); push!(trace, W)
                end
            end
            groups = sort(unique(a))
            inits = Vector{Int64}[]; ords = Vector{Int32}[]; rungroup = Int32[]
            for l in groups
                push!(inits, P[l]); push!(ords, Vector{Int32}(1:n)); push!(rungroup, l - 1)
                for o in orders
                    push!(inits, zeros(Int64, n)); push!(ords, o); push!(rungroup, l - 1)
                end
            end
            info = visearchgroups(b, result, a .- 1, inits, ords, rungroup; maxK = cap, maxsweeps = maxsweeps)
            changed = false
            for l in groups
                new = info.labels[:, info.best[l]]
                if new != P[l]
                    P[l] = new; changed = true
                end
            end
            if !changed && !repaired && prev == a
                converged = true
                break
            end
            prev = a
            a, d, W = wasabiassign(dist(P)); push!(trace, W)
        end
        push!(runs, (P = P, a = a, d = d, W = W, trace = trace, iterations = it, converged = converged || W == 0))
    end
    starts = [r.W for r in runs]
    win = argmin(starts)
    r = runs[win]
    sizes = [count(==(l), r.a) for l in eachindex(r.P)]
    keep = sort([l for l in eachindex(r.P) if sizes[l] > 0]; by = l -> (-sizes[l], l))
    assignment = [findfirst(==(l), keep) for l in r.a]
    return (particles = [r.P[l] for l in keep], weights = [sizes[l] / m for l in keep], assignment = assignment,
            group_num = [sum(Int128.(r.d[assignment .== l])) for l in eachindex(keep)], objective_num = r.W,
            wasserstein = Float64(r.W) / (2.0^32 * n * m), trace = r.trace, iterations = r.iterations, converged = r.converged,
            start = win, starts = starts)
end

export visearchgroups, wasabi

end # module
