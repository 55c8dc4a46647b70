# MPFmtHIP.jl -- libmpfmt.so (MI355X) under MotionPlanning.jl's own dispatch.  `include` after `using MotionPlanning`.
# Julia 0.5/0.6 dialect like the reference (type / immutable / Ptr{Void}).  Julia is not installed where this repository is
# built: every ccall below is executed, with exactly these argument widths, by tests/abi_c/abi_caller.c and abi_caller2.c (gcc,
# -m gpu; a width that differs from include/mpfmt.h fails their build), and what they return is compared with the oracle.
import MotionPlanning: helper_data_structures, inball, is_free_state, is_free_motion, closest, closeR, sample_free!,
                       DistanceDataStructure, SweptCollisionChecker, EmptyControlCache, BruteDistanceDS, BoxBounds, ImmutableNNC,
                       MetricNN, statevec2mat, LinearQuadratic, ChoppedMetric, ChoppedQuasiMetric, ReedsSheppExact, DubinsExact,
                       SE2State, PointRobot2D, Circle, Polygon, Compound2D, Shape2D
const libmpfmt = "libmpfmt"                      # motionplanning.jl_amd/libmpfmt.so on LD_LIBRARY_PATH
lasterr(ctx) = unsafe_string(ccall((:mpfmt_last_error, libmpfmt), Cstring, (Ptr{Void},), ctx))
chk(ctx::Ptr{Void}, rc::Int32) = rc == 0 || error(lasterr(ctx))

# ---- plugin point 1: index build, helper_data_structures(V, ::Euclidean) (geometric.jl:14) -------------------------
immutable HIPDistanceDS{T} <: DistanceDataStructure{T}
    ctx::Ptr{Void}
end
function HIPDistanceDS{S}(V::Vector{S}, device::Integer = 0)
    h = Ref{Ptr{Void}}(C_NULL)
    rc = ccall((:mpfmt_ctx_create, libmpfmt), Int32, (Int32, Ptr{Ptr{Void}}), device, h)
    rc == 0 || error(lasterr(C_NULL))
    X = statevec2mat(V)                          # zero-copy d x N view (primitivetypes.jl:21-24)
    chk(h[], ccall((:mpfmt_upload_samples, libmpfmt), Int32, (Ptr{Void}, Ptr{Float64}, Int64, Int32),
                   h[], X, size(X, 2), size(X, 1)))
    HIPDistanceDS{eltype(S)}(h[])
end
helper_data_structures{S}(V::Vector{S}, M::Euclidean) = (HIPDistanceDS(V), EmptyControlCache())

# ---- plugin point 2: r-disc query, inball (nearneighbors.jl:179-183) and the whole cache (nearneighbors.jl:23-27) --
function inball{S}(V::Vector{S}, dist::Euclidean, DS::HIPDistanceDS, v::Int, r, forwards::Bool = true)
    N = length(V); inds = Vector{Int}(N); ds = Vector{Float64}(N); k = Ref{Int64}(0)
    chk(DS.ctx, ccall((:mpfmt_rdisc_query, libmpfmt), Int32,
                      (Ptr{Void}, Int64, Float64, Ptr{Int64}, Ptr{Float64}, Int64, Ptr{Int64}),
                      DS.ctx, v, r, inds, ds, N, k))
    SparseVector(N, resize!(inds, k[]), resize!(ds, k[]))      # ascending, self excluded, 1-based
end
function hip_neighbor_graph(DS::HIPDistanceDS, N::Int, r::Float64)
    colptr = Vector{Int}(N + 1); nnz = Ref{Int64}(0)
    chk(DS.ctx, ccall((:mpfmt_rdisc_count, libmpfmt), Int32, (Ptr{Void}, Float64, Ptr{Int64}, Ptr{Int64}),
                      DS.ctx, r, colptr, nnz))
    rowval = Vector{Int}(nnz[]); nzval = Vector{Float64}(nnz[])
    chk(DS.ctx, ccall((:mpfmt_rdisc_fill, libmpfmt), Int32, (Ptr{Void}, Ptr{Int64}, Ptr{Float64}), DS.ctx, rowval, nzval))
    SparseMatrixCSC(N, N, colptr, rowval, nzval)
end

# ---- plugin point 3: collision checker (boxesND.jl:15-28) ------------------------------------------------------------
# After `precompute!` every is_free_motion(V[y], V[x], CC) of the UNMODIFIED fmtstar! (fmt.jl:75) is a lookup: the sample
# index of each end point from a Dict, a binary search for y in column x of the CSC, one bit of the edge BitVector.  States
# that are not samples (adaptive_shortcut, sample_free!) fall through to the reference's own scalar code on CC.boxes --
# identical arithmetic -- so no call ever launches a one-edge kernel.
type HIPBoxes{N,T} <: SweptCollisionChecker
    boxes::Vector{BoxBounds{N,T}}
    count::Int                                   # fmt.jl:12,106 need a mutable count
    ctx::Ptr{Void}
    index::Dict{Any,Int}                         # sample -> 1-based index
    D::SparseMatrixCSC{Float64,Int}              # the r-disc graph the edge bits refer to
    free::BitVector                              # bit e <-> is_free_motion(V[rowval[e]], V[column of e])
    pinned::Vector{Ptr{Void}}                    # page-locked arrays behind D and free (hip_precompute_step!)
end
function HIPBoxes{N,T}(boxes::Vector{BoxBounds{N,T}}, DS::HIPDistanceDS, SS)
    lohi = reinterpret(T, boxes, (2N, length(boxes)))          # [lo(N); hi(N)] per box, zero copy
    chk(DS.ctx, ccall((:mpfmt_upload_boxes, libmpfmt), Int32,
                      (Ptr{Void}, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Int32),
                      DS.ctx, lohi, length(boxes), N, collect(SS.lo), collect(SS.hi), length(SS.lo)))
    HIPBoxes(boxes, 0, DS.ctx, Dict{Any,Int}(), spzeros(0, 0), falses(0), Ptr{Void}[])
end
# graph + every edge bit in one go, and the reference's own neighbour cache installed: inball! becomes viewcol (nearneighbors.jl:128)
function precompute!(P::MPProblem, r::Float64)
    CC = P.CC; N = length(P.V)
    CC.D = hip_neighbor_graph(P.V.DS, N, r)
    CC.free = falses(nnz(CC.D))
    chk(CC.ctx, ccall((:mpfmt_graph_edges_free, libmpfmt), Int32, (Ptr{Void}, Ptr{UInt64}), CC.ctx, CC.free.chunks))
    CC.index = Dict{Any,Int}(zip(P.V.V, 1:N))
    P.V = MetricNN(P.V.V, P.V.dist, P.V.init, ImmutableNNC(CC.D, fill(r, N)), P.V.DS, P.V.US)
    P
end
# The same precompute! without a second build, a second sweep or a pageable copy: ONE mpfmt_graph_step_device (index, half build of the
# graph, edge tests fused into it, mask written by the ordering pass -- the path bench.py times), then ONE mpfmt_graph_export_pinned into
# the ctx's page-locked export arena (2.6 GB at the north star, at link speed).  The arena lives as long as the ctx: page-locking it
# (~0.2 s per GB) is paid by the first graph of a ctx only, every later precompute of the same problem costs the copy alone.  The
# arrays back the SparseMatrixCSC and the BitVector directly (pointer_to_array, own = false) and are overwritten by the next export of
# the ctx; hip_release!(CC) drops the references (the library frees the arena with the ctx).
function hip_precompute_step!(P::MPProblem, r::Float64)
    CC = P.CC; N = length(P.V); ctx = CC.ctx
    nnz = Ref{Int64}(0)
    chk(ctx, ccall((:mpfmt_graph_step_device, libmpfmt), Int32, (Ptr{Void}, Float64, Ptr{Int64}), ctx, r, nnz))
    # the arrays of the previous export live in the ctx's arena, which an export of a LARGER graph frees: drop them before the call
    # (include/mpfmt.h, mpfmt_graph_export_pinned)
    CC.D = spzeros(0, 0); CC.free = falses(0)
    pc = Ref{Ptr{Int64}}(C_NULL); pr = Ref{Ptr{Int64}}(C_NULL); pv = Ref{Ptr{Float64}}(C_NULL); pm = Ref{Ptr{UInt64}}(C_NULL)
    rate = Ref{Float64}(0.0)
    chk(ctx, ccall((:mpfmt_graph_export_pinned, libmpfmt), Int32,
                   (Ptr{Void}, Ptr{Ptr{Int64}}, Ptr{Ptr{Int64}}, Ptr{Ptr{Float64}}, Ptr{Ptr{UInt64}}, Ptr{Int64}, Ptr{Float64}),
                   ctx, pc, pr, pv, pm, nnz, rate))
    words = (nnz[] + 63) >> 6
    colptr = pointer_to_array(pc[], N + 1, false)
    rowval = pointer_to_array(pr[], nnz[], false)
    nzval = pointer_to_array(pv[], nnz[], false)
    CC.D = SparseMatrixCSC(N, N, colptr, rowval, nzval)
    CC.free = falses(0)
    CC.free.chunks = pointer_to_array(pm[], words, false); CC.free.len = nnz[]; CC.free.dims = (nnz[],)
    CC.index = Dict{Any,Int}(zip(P.V.V, 1:N))
    P.V = MetricNN(P.V.V, P.V.dist, P.V.init, ImmutableNNC(CC.D, fill(r, N)), P.V.DS, P.V.US)
    rate[]                                       # GB/s of the export
end
# The same export into page-locked arrays that outlive the ctx (mpfmt_pinned_alloc per array -- page-locking paid per call -- returned
# by hip_release!): for a graph that is kept while the ctx goes on to other sample sets.
function hip_export_owned!(CC::HIPBoxes, N::Int, nnz::Int)
    words = (nnz + 63) >> 6
    ptrs = Ptr{Void}[]
    for bytes in (8(N + 1), 8max(nnz, 1), 8max(nnz, 1), 8max(words, 1))
        p = Ref{Ptr{Void}}(C_NULL)
        ccall((:mpfmt_pinned_alloc, libmpfmt), Int32, (Int64, Ptr{Ptr{Void}}), bytes, p) == 0 || error("mpfmt_pinned_alloc")
        push!(ptrs, p[])
    end
    rate = Ref{Float64}(0.0)
    chk(CC.ctx, ccall((:mpfmt_graph_export, libmpfmt), Int32, (Ptr{Void}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{UInt64}, Ptr{Float64}),
                      CC.ctx, ptrs[1], ptrs[2], ptrs[3], ptrs[4], rate))
    CC.D = SparseMatrixCSC(N, N, pointer_to_array(convert(Ptr{Int64}, ptrs[1]), N + 1, false),
                           pointer_to_array(convert(Ptr{Int64}, ptrs[2]), nnz, false), pointer_to_array(convert(Ptr{Float64}, ptrs[3]), nnz, false))
    CC.free = falses(0)
    CC.free.chunks = pointer_to_array(convert(Ptr{UInt64}, ptrs[4]), words, false); CC.free.len = nnz; CC.free.dims = (nnz,)
    CC.pinned = ptrs
    rate[]
end
function hip_release!(CC::HIPBoxes)
    CC.D = spzeros(0, 0); CC.free = falses(0)
    for p in CC.pinned
        ccall((:mpfmt_pinned_free, libmpfmt), Int32, (Ptr{Void},), p)
    end
    CC.pinned = Ptr{Void}[]
end
function is_free_motion(v::AbstractVector, w::AbstractVector, CC::HIPBoxes)
    CC.count += 1                                # boxesND.jl:26
    y = get(CC.index, v, 0); x = get(CC.index, w, 0)
    if x > 0 && y > 0
        rng = CC.D.colptr[x]:(CC.D.colptr[x+1]-1)
        e = searchsortedfirst(CC.D.rowval, y, first(rng), last(rng), Base.Order.Forward)
        e <= last(rng) && CC.D.rowval[e] == y && return CC.free[e]
    end
    is_free_motion(v, w, CC.boxes)               # not a graph edge: the reference's scalar predicate (boxesND.jl:52-56)
end
is_free_state(v::AbstractVector, CC::HIPBoxes) = is_free_state(v, CC.boxes)     # boxesND.jl:42-43 (points: sampler, init)

# ---- whole solve on the device: fmtstar! (fmt.jl:3-119), recursion included (include/mpfmt.h, mpfmt_fmtstar_wavefront) ----
immutable FmtResult
    status::Int32; cost::Float64; z::Int64; collision_checks::Int64; path_len::Int64; nnz::Int64
    ms_graph::Float64; ms_sweep::Float64; ms_host_loop::Float64
end
immutable WfInfo
    done::Int32; nz::Int32; nx::Int32; nconn::Int32; ntrip::Int32; iters::Int64; checks::Int64; cmin::Float64
    tot_z::Int64; tot_x::Int64; tot_conn::Int64
end
# band = cost width of a wavefront; single = true reproduces the reference's pop order exactly (one node per step)
function fmtstar_hip!(P::MPProblem, r::Float64; init_idx = 1, checkpts = true, band = 0.25r, single = false)
    DS = P.V.DS; N = length(P.V)
    A = Vector{Int}(N); C = Vector{Float64}(N); path = Vector{Int}(N); res = Ref{FmtResult}(); info = Ref{WfInfo}()
    g = [P.goal.center; P.goal.radius]           # BallGoal (goals.jl:17-21) = MPFMT_GOAL_BALL
    rc = ccall((:mpfmt_fmtstar_wavefront, libmpfmt), Int32,
               (Ptr{Void}, Float64, Int64, Int32, Int32, Ptr{Float64}, Float64, Int32,
                Ptr{Int64}, Ptr{Float64}, Ptr{Int64}, Ptr{FmtResult}, Ptr{WfInfo}),
               DS.ctx, r, init_idx, checkpts, 1, g, band, single ? 1 : 0, A, C, path, res, info)
    rc == -6 && (warn("Initial state is infeasible!"); P.status = :failed; return Inf)      # fmt.jl:24-29
    chk(DS.ctx, rc)
    P.CC.count = res[].collision_checks
    P.status = res[].status == 1 ? :solved : :failed
    P.solution = MPSolution(P.status, res[].cost, (res[].ms_graph + res[].ms_sweep + res[].ms_host_loop) / 1e3,
                            Dict("collision_checks" => res[].collision_checks, "tree" => A, "cost" => res[].cost,
                                 "path" => path[1:res[].path_len], "planner" => "FMTstar", "r" => r, "num_samples" => N,
                                 "wavefronts" => info[].iters))
    P.status, P.solution.cost, P.solution.elapsed
end

# ---- PRM*: the graph planner the reference leaves open (src/problems.jl:57, "# TODO: graph (PRM)"): exact cost-to-come of every
#      sample over the free-edge graph, on the device (include/mpfmt.h "roadmap queries").  The symbols are named here once; the C
#      caller that executes these calls with the same widths is tests/abi_c/abi_caller3.c. ----
const sym_prmstar = :mpfmt_prmstar
const sym_knn_prmstar = :mpfmt_knn_prmstar
const sym_graph_sssp = :mpfmt_graph_sssp
immutable SsspInfo
    reached::Int64; rounds::Int64; relaxations::Int64; ms_device::Float64
end
# connections = :R (radius r) or :K (k nearest); metadata["cost_to_come"] = the field (Inf = unreachable)
function hip_prmstar!(P::MPProblem, r::Float64; init_idx = 1, checkpts = true, connections = :R, k = 0)
    DS = P.V.DS; N = length(P.V)
    A = Vector{Int}(N); C = Vector{Float64}(N); path = Vector{Int}(N); res = Ref{FmtResult}()
    g = [P.goal.center; P.goal.radius]           # BallGoal (goals.jl:17-21) = MPFMT_GOAL_BALL
    rc = connections == :K ?
        ccall((sym_knn_prmstar, libmpfmt), Int32,
              (Ptr{Void}, Int64, Int64, Int32, Int32, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}, Ptr{FmtResult}),
              DS.ctx, k, init_idx, checkpts, 1, g, A, C, path, res) :
        ccall((sym_prmstar, libmpfmt), Int32,
              (Ptr{Void}, Float64, Int64, Int32, Int32, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}, Ptr{FmtResult}),
              DS.ctx, r, init_idx, checkpts, 1, g, A, C, path, res)
    rc == -6 && (warn("Initial state is infeasible!"); P.status = :failed; return Inf)
    chk(DS.ctx, rc)
    P.status = res[].status == 1 ? :solved : :failed
    P.solution = MPSolution(P.status, res[].cost, (res[].ms_graph + res[].ms_sweep + res[].ms_host_loop) / 1e3,
                            Dict("collision_checks" => res[].collision_checks, "tree" => A, "cost" => res[].cost,
                                 "path" => path[1:res[].path_len], "planner" => "prmstar", "r" => r, "num_samples" => N,
                                 "cost_to_come" => C))
    P.status, P.solution.cost, P.solution.elapsed
end
# multi-query use: the fields of several sources over the graph and mask a step (or hip_prmstar!) left resident; C is N x nsrc
function hip_graph_sssp(DS::HIPDistanceDS, N::Int, sources::Vector{Int}; checkpts = true)
    n = length(sources)
    C = Matrix{Float64}(N, n); A = Matrix{Int}(N, n); info = Vector{SsspInfo}(n)
    chk(DS.ctx, ccall((sym_graph_sssp, libmpfmt), Int32, (Ptr{Void}, Ptr{Int64}, Int64, Int32, Ptr{Float64}, Ptr{Int64}, Ptr{SsspInfo}),
                      DS.ctx, sources, n, checkpts, C, A, info))
    C, A, info
end

# ---- PRM* over the steering graphs and the cost-to-go field (include/mpfmt.h "cost-to-go").  The symbols are named here once; the C
#      caller that executes these calls with the same widths is tests/abi_c/abi_caller10.c. ----
# (the three planners are executed by abi_caller10.c, not by abi_caller3.c, which holds the Euclidean planners' symbols)
const sym_host_graph_sssp_to = :mpfmt_host_graph_sssp_to
const sym_graph_sssp_to = :mpfmt_graph_sssp_to
const sym_di_prmstar = Symbol("mpfmt_di_prmstar")
const sym_dubins_prmstar = Symbol("mpfmt_dubins_prmstar")
const sym_reedsshepp_prmstar = Symbol("mpfmt_reedsshepp_prmstar")
# the feedback policy over the resident swept graph (r-disc, k-nearest or steering): from every sample the optimal cost to the target
# set and the next sample on the way; G[i] = Inf: no target reachable, S[i] = 0: target or unreached
function hip_graph_sssp_to(DS::HIPDistanceDS, N::Int, targets::Vector{Int}; checkpts = true)
    G = Vector{Float64}(N); S = Vector{Int}(N); info = Ref{SsspInfo}()
    chk(DS.ctx, ccall((sym_graph_sssp_to, libmpfmt), Int32, (Ptr{Void}, Ptr{Int64}, Int64, Int32, Ptr{Float64}, Ptr{Int64}, Ptr{SsspInfo}),
                      DS.ctx, targets, length(targets), checkpts, G, S, info))
    G, S, info[]
end
# the same field on the host over exported arrays (colptr 0-based, rowval 0-based Int32, packed masks; F may be C_NULL)
function host_graph_sssp_to(colptr::Vector{Int}, rowval::Vector{Int32}, nzval::Vector{Float64}, efree::Vector{UInt64}, F, targets::Vector{Int})
    N = length(colptr) - 1
    G = Vector{Float64}(N); S = Vector{Int}(N)
    rc = ccall((sym_host_graph_sssp_to, libmpfmt), Int32,
               (Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Float64}, Ptr{UInt64}, Ptr{UInt64}, Ptr{Int64}, Int64, Ptr{Float64}, Ptr{Int64}),
               N, colptr, rowval, nzval, efree, F, targets, length(targets), G, S)
    rc == 0 || error("mpfmt_host_graph_sssp_to rejected its arguments")
    G, S
end
# PRM* in the double-integrator space (rho, cost radius r) and in the car spaces (kind = :dubins or :reedsshepp; turning radius, speed, r)
function hip_steer_prmstar!(P::MPProblem, kind::Symbol, a::Float64, b::Float64, r::Float64; init_idx = 1, checkpts = true)
    DS = P.V.DS; N = length(P.V)
    A = Vector{Int}(N); C = Vector{Float64}(N); path = Vector{Int}(N); res = Ref{FmtResult}()
    g = [P.goal.center; P.goal.radius]
    rc = kind == :di ?
        ccall((sym_di_prmstar, libmpfmt), Int32,
              (Ptr{Void}, Float64, Float64, Int64, Int32, Int32, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}, Ptr{FmtResult}),
              DS.ctx, a, r, init_idx, checkpts, 1, g, A, C, path, res) :
        kind == :dubins ?
        ccall((sym_dubins_prmstar, libmpfmt), Int32,
              (Ptr{Void}, Float64, Float64, Float64, Int64, Int32, Int32, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}, Ptr{FmtResult}),
              DS.ctx, a, b, r, init_idx, checkpts, 1, g, A, C, path, res) :
        ccall((sym_reedsshepp_prmstar, libmpfmt), Int32,
              (Ptr{Void}, Float64, Float64, Float64, Int64, Int32, Int32, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}, Ptr{FmtResult}),
              DS.ctx, a, b, r, init_idx, checkpts, 1, g, A, C, path, res)
    rc == -6 && (warn("Initial state is infeasible!"); P.status = :failed; return Inf)
    chk(DS.ctx, rc)
    P.status = res[].status == 1 ? :solved : :failed
    P.solution = MPSolution(P.status, res[].cost, (res[].ms_graph + res[].ms_sweep + res[].ms_host_loop) / 1e3,
                            Dict("collision_checks" => res[].collision_checks, "tree" => A, "cost" => res[].cost,
                                 "path" => path[1:res[].path_len], "planner" => "prmstar", "r" => r, "num_samples" => N,
                                 "cost_to_come" => C))
    P.status, P.solution.cost, P.solution.elapsed
end

# states that are NOT samples (the robot's present pose, candidate goals) against the resident roadmap: nothing is rebuilt.
# S, G: d x n matrices (one state per column).  hip_roadmap_query -> (cost[n], path_ptr[n + 1] 0-based, path (1-based samples), info[n]);
# hip_roadmap_attach -> the goal half for many goals over ONE field C (a column of hip_graph_sssp): (cost[n], parent[n], 0 = none)
const sym_roadmap_query = :mpfmt_roadmap_query
const sym_roadmap_attach = :mpfmt_roadmap_attach
immutable RoadmapInfo
    status::Int32; pad::Int32; near_s::Int64; usable_s::Int64; near_g::Int64; usable_g::Int64; rounds::Int64; path_len::Int64
    ms_device::Float64
end
function hip_roadmap_query(DS::HIPDistanceDS, S::Matrix{Float64}, G::Matrix{Float64}; checkpts = true, path_cap = 64 * size(S, 2))
    n = size(S, 2)
    cost = Vector{Float64}(n); pptr = Vector{Int}(n + 1); path = Vector{Int}(max(path_cap, 1)); info = Vector{RoadmapInfo}(n)
    rc = ccall((sym_roadmap_query, libmpfmt), Int32,
               (Ptr{Void}, Ptr{Float64}, Ptr{Float64}, Int64, Int32, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{RoadmapInfo}),
               DS.ctx, S, G, n, checkpts, cost, pptr, path, path_cap, info)
    rc == -5 && return hip_roadmap_query(DS, S, G; checkpts = checkpts, path_cap = pptr[n + 1])
    chk(DS.ctx, rc)
    cost, pptr, path[1:pptr[n + 1]], info
end
function hip_roadmap_attach(DS::HIPDistanceDS, Q::Matrix{Float64}, C::Vector{Float64})
    n = size(Q, 2)
    cost = Vector{Float64}(n); parent = Vector{Int}(n)
    chk(DS.ctx, ccall((sym_roadmap_attach, libmpfmt), Int32, (Ptr{Void}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}),
                      DS.ctx, Q, n, C, parent, cost))
    cost, parent
end

# the same on a resident steering graph (double integrator, Dubins, Reeds-Shepp; include/mpfmt.h, "roadmap queries for external
# states, steering spaces"): the states attach by the space's own steer, with the resident graph's parameters.  hip_steer_roadmap_near
# -> (ptr[n + 1] 0-based, idx 1-based ascending, cost, free) of the tail (direction 0) or head (1) lists.  The C caller that executes
# these calls with the same widths is tests/abi_c/abi_caller12.c.
const sym_steer_roadmap_query = :mpfmt_steer_roadmap_query
const sym_steer_roadmap_near = :mpfmt_steer_roadmap_near
const sym_steer_roadmap_attach = :mpfmt_steer_roadmap_attach
function hip_steer_roadmap_query(DS::HIPDistanceDS, S::Matrix{Float64}, G::Matrix{Float64}; checkpts = true, path_cap = 64 * size(S, 2))
    n = size(S, 2)
    cost = Vector{Float64}(n); pptr = Vector{Int}(n + 1); path = Vector{Int}(max(path_cap, 1)); info = Vector{RoadmapInfo}(n)
    rc = ccall((sym_steer_roadmap_query, libmpfmt), Int32,
               (Ptr{Void}, Ptr{Float64}, Ptr{Float64}, Int64, Int32, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{RoadmapInfo}),
               DS.ctx, S, G, n, checkpts, cost, pptr, path, path_cap, info)
    rc == -5 && return hip_steer_roadmap_query(DS, S, G; checkpts = checkpts, path_cap = pptr[n + 1])
    chk(DS.ctx, rc)
    cost, pptr, path[1:pptr[n + 1]], info
end
function hip_steer_roadmap_near(DS::HIPDistanceDS, Q::Matrix{Float64}, direction::Int; cap = 0)
    n = size(Q, 2)
    ptr = Vector{Int}(n + 1); total = Ref{Int64}(0)
    idx = Vector{Int}(max(cap, 1)); dist = Vector{Float64}(max(cap, 1)); free = falses(max(cap, 1))
    rc = ccall((sym_steer_roadmap_near, libmpfmt), Int32,
               (Ptr{Void}, Ptr{Float64}, Int64, Int32, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{UInt64}, Ptr{Int64}),
               DS.ctx, Q, n, direction, ptr, cap, idx, dist, free.chunks, total)
    rc == -5 && return hip_steer_roadmap_near(DS, Q, direction; cap = total[])
    chk(DS.ctx, rc)
    ptr, idx[1:total[]], dist[1:total[]], free[1:total[]]
end
function hip_steer_roadmap_attach(DS::HIPDistanceDS, Q::Matrix{Float64}, C::Vector{Float64})
    n = size(Q, 2)
    cost = Vector{Float64}(n); parent = Vector{Int}(n)
    chk(DS.ctx, ccall((sym_steer_roadmap_attach, libmpfmt), Int32, (Ptr{Void}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}),
                      DS.ctx, Q, n, C, parent, cost))
    cost, parent
end

# ---- a cost-to-come field kept valid across box edits (include/mpfmt.h): hip_prmstar!(P, r) computes a field and throws it away;
#      hip_field_begin! keeps the field of init_idx in the ctx, and after mpfmt_boxes_add / _remove (INTEGRATION.md, "obstacles that
#      change") hip_replan! repairs it -- work that follows the edit -- and extracts goal and path again.  The C caller that executes
#      these calls with the same widths is tests/abi_c/abi_caller7.c. ----
const sym_field_begin = :mpfmt_field_begin
const sym_field_update = :mpfmt_field_update
const sym_field_read = :mpfmt_field_read
const sym_field_goal = :mpfmt_field_goal
const sym_field_drop = :mpfmt_field_drop
immutable FieldInfo
    reached::Int64; invalidated::Int64; dirty_columns::Int64; columns_read::Int64; column_visits::Int64; entries_read::Int64
    rounds::Int64; relaxations::Int64; ms_device::Float64; path::Int32; pad::Int32
end
function hip_field_begin!(DS::HIPDistanceDS; init_idx = 1, checkpts = true)
    info = Ref{FieldInfo}()
    chk(DS.ctx, ccall((sym_field_begin, libmpfmt), Int32, (Ptr{Void}, Int64, Int32, Ptr{FieldInfo}), DS.ctx, init_idx, checkpts, info))
    info[]
end
hip_field_drop!(DS::HIPDistanceDS) = chk(DS.ctx, ccall((sym_field_drop, libmpfmt), Int32, (Ptr{Void},), DS.ctx))
# after the box edits: repair (info.path == 1) or, where an edit could not be applied in place, recompute (0); then goal and path
function hip_replan!(P::MPProblem)
    DS = P.V.DS; N = length(P.V)
    info = Ref{FieldInfo}()
    chk(DS.ctx, ccall((sym_field_update, libmpfmt), Int32, (Ptr{Void}, Ptr{FieldInfo}), DS.ctx, info))
    A = Vector{Int}(N); C = Vector{Float64}(N); path = Vector{Int}(N); res = Ref{FmtResult}()
    g = [P.goal.center; P.goal.radius]           # BallGoal (goals.jl:17-21) = MPFMT_GOAL_BALL
    chk(DS.ctx, ccall((sym_field_goal, libmpfmt), Int32, (Ptr{Void}, Int32, Ptr{Float64}, Ptr{Int64}, Ptr{FmtResult}), DS.ctx, 1, g, path, res))
    chk(DS.ctx, ccall((sym_field_read, libmpfmt), Int32, (Ptr{Void}, Ptr{Float64}, Ptr{Int64}), DS.ctx, C, A))
    P.status = res[].status == 1 ? :solved : :failed
    P.solution = MPSolution(P.status, res[].cost, (info[].ms_device + res[].ms_host_loop) / 1e3,
                            Dict("collision_checks" => 0, "tree" => A, "cost" => res[].cost, "path" => path[1:res[].path_len],
                                 "planner" => "prmstar", "num_samples" => N, "cost_to_come" => C, "field_info" => info[]))
    P.status, P.solution.cost, P.solution.elapsed
end

# ---- a cost-to-go policy kept valid across box edits, on any resident swept graph (include/mpfmt.h; r-disc, k-nearest, double
#      integrator, Dubins, Reeds-Shepp): hip_graph_sssp_to computes the policy and throws it away; hip_togo_begin! keeps it in the ctx,
#      and after mpfmt_boxes_add / _remove hip_togo_update! repairs it -- the robot has left init: what it needs again after every edit
#      is the policy towards the fixed goal from wherever it stands.  The C caller that executes these calls with the same widths is
#      tests/abi_c/abi_caller11.c. ----
const sym_togo_begin = :mpfmt_togo_begin
const sym_togo_update = :mpfmt_togo_update
const sym_togo_read = :mpfmt_togo_read
const sym_togo_drop = :mpfmt_togo_drop
immutable TogoInfo
    reached::Int64; invalidated::Int64; dirty_columns::Int64; columns_read::Int64; column_visits::Int64; entries_read::Int64
    rounds::Int64; relaxations::Int64; atomics::Int64; ms_device::Float64; path::Int32; pad::Int32
end
function hip_togo_begin!(DS::HIPDistanceDS, targets::Vector{Int}; checkpts = true)
    info = Ref{TogoInfo}()
    chk(DS.ctx, ccall((sym_togo_begin, libmpfmt), Int32, (Ptr{Void}, Ptr{Int64}, Int64, Int32, Ptr{TogoInfo}),
                      DS.ctx, targets, length(targets), checkpts, info))
    info[]
end
# after the box edits: repair (info.path == 1) or, where an edit could not be applied in place and the mask was swept whole, recompute (0)
function hip_togo_update!(DS::HIPDistanceDS)
    info = Ref{TogoInfo}()
    chk(DS.ctx, ccall((sym_togo_update, libmpfmt), Int32, (Ptr{Void}, Ptr{TogoInfo}), DS.ctx, info))
    info[]
end
# G[i] = Inf: no target reachable from sample i; S[i] = the next sample on the way, 0: target or unreached
function hip_togo_read(DS::HIPDistanceDS, N::Int)
    G = Vector{Float64}(N); S = Vector{Int}(N)
    chk(DS.ctx, ccall((sym_togo_read, libmpfmt), Int32, (Ptr{Void}, Ptr{Float64}, Ptr{Int64}), DS.ctx, G, S))
    G, S
end
hip_togo_drop!(DS::HIPDistanceDS) = chk(DS.ctx, ccall((sym_togo_drop, libmpfmt), Int32, (Ptr{Void},), DS.ctx))

# ---- post-processing: adaptive_shortcut!(P, iterations) (src/postprocessors.jl:41-50) on the device; the checker of P.V.DS.ctx is the
#      one the last upload bound (hip_bind! / the planner calls).  max_states bounds the working path (include/mpfmt.h).
const sym_adaptive_shortcut = :mpfmt_adaptive_shortcut
immutable ShortcutInfo
    status::Int32; iterations_done::Int32; n_out::Int64; max_working_len::Int64; max_halvings::Int64; collision_checks::Int64
    tests_evaluated::Int64
end
function hip_adaptive_shortcut!(P::MPProblem, iterations::Int = 10; max_states::Int = 256)
    P.status == :solved || error("Cannot post-process unsolved problem! (adaptive-shortcut)")
    isa(P.SS.dist, Euclidean) || error("Adaptive-shortcut requires Euclidean SS")
    DS = P.V.DS; S = P.solution
    path = P.V.V[S.metadata["path"]]                       # Vector{SVector{d,Float64}} = d x n column-major in memory
    d = length(path[1])
    out = Matrix{Float64}(d, max_states); cum = Vector{Float64}(max_states); info = Ref{ShortcutInfo}()
    chk(DS.ctx, ccall((sym_adaptive_shortcut, libmpfmt), Int32,
                      (Ptr{Void}, Ptr{Float64}, Int64, Int32, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{ShortcutInfo}),
                      DS.ctx, path, length(path), iterations, max_states, out, max_states, cum, info))
    n = info[].n_out
    P.CC.count += info[].collision_checks
    S.metadata["smoothed_path"] = [typeof(path[1])(out[:, i]) for i in 1:n]
    S.metadata["smoothed_cumcost"] = cum[1:n]
    S.metadata["smoothed_cost"] = cum[n]
    cum[n]
end

# ---- post-processing in the steering spaces (include/mpfmt.h, "steering shortcut"): the pair primitive and the batched shortcut.
#      space: 1 double integrator (params (rho, tmax)), 2 Dubins, 3 Reeds-Shepp (params (turn radius, speed)); the checker of ctx is the
#      one the last upload bound.  P, Q: d x n column-major.
const sym_steer_motions_free = :mpfmt_steer_motions_free
const sym_steer_shortcut_batch = :mpfmt_steer_shortcut_batch
immutable SteerShortcutInfo
    status::Int32; iterations_done::Int32; n_out::Int64; max_working_len::Int64; inserted::Int64; legs_blocked::Int64
    collision_checks::Int64; tests_evaluated::Int64; cost_in::Float64; cost_out::Float64
end
function hip_steer_motions_free(ctx::Ptr{Void}, space::Integer, params::Vector{Float64}, P::Matrix{Float64}, Q::Matrix{Float64})
    d, n = size(P)
    mask = zeros(UInt64, max(div(n + 63, 64), 1)); cost = Vector{Float64}(n); dur = Vector{Float64}(n); nseg = Vector{Int32}(n)
    chk(ctx, ccall((sym_steer_motions_free, libmpfmt), Int32,
                   (Ptr{Void}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{UInt64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                   ctx, space, d, params, P, Q, n, mask, cost, dur, nseg))
    [(mask[div(e - 1, 64) + 1] >> ((e - 1) % 64)) & 1 == 1 for e in 1:n], cost, dur, nseg
end
# paths: a vector of d x n_b matrices -> a vector of (path, cumcost, origin, info)
function hip_steer_shortcut(ctx::Ptr{Void}, space::Integer, params::Vector{Float64}, paths::Vector{Matrix{Float64}}, iterations::Int = 4;
                            max_states::Int = 256)
    B = length(paths); d = size(paths[1], 1)
    offsets = cumsum(vcat(Int64[0], Int64[size(p, 2) for p in paths])); P = hcat(paths...)
    cap = B * max_states
    out = Matrix{Float64}(d, cap); cum = Vector{Float64}(cap); org = Vector{Int32}(cap); out_off = Vector{Int64}(B + 1)
    info = Vector{SteerShortcutInfo}(B)
    chk(ctx, ccall((sym_steer_shortcut_batch, libmpfmt), Int32,
                   (Ptr{Void}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Int64, Int32, Int64, Ptr{Float64}, Ptr{Int64}, Int64, Ptr{Float64},
                    Ptr{Int32}, Ptr{SteerShortcutInfo}),
                   ctx, space, d, params, P, offsets, B, iterations, max_states, out, out_off, cap, cum, org, info))
    [(out[:, out_off[b]+1:out_off[b+1]], cum[out_off[b]+1:out_off[b+1]], org[out_off[b]+1:out_off[b+1]], info[b]) for b in 1:B]
end

# ---- multi-GPU: ONE Julia thread, G ctxs (SURVEY 8e); the RCCL exchange lives behind the ABI ------------------------
function hip_comm_create!(ctxs::Vector{Ptr{Void}})
    id = Vector{UInt8}(128)
    ccall((:mpfmt_comm_unique_id, libmpfmt), Int32, (Ptr{UInt8},), id) == 0 || error(lasterr(C_NULL))
    ccall((:mpfmt_group_begin, libmpfmt), Int32, ())
    for (g, c) in enumerate(ctxs)
        chk(c, ccall((:mpfmt_comm_create, libmpfmt), Int32, (Ptr{Void}, Int32, Int32, Ptr{UInt8}), c, g - 1, length(ctxs), id))
    end
    ccall((:mpfmt_group_end, libmpfmt), Int32, ())
end


# One thread, G ctxs, one step of the eager hot path on every GPU and the free-edge masks of all shards on each of them
# (what `bench.py --gpus G` does with one process per GPU).  Launch everything, then finish everything: no call blocks on a
# peer this thread has yet to launch.  `first` = true on the first step (the thread has seen every shard's nnz: it agrees the
# capacity itself instead of the blocking lengths exchange).  Returns per-ctx (device pointer, stride in words, words, nnz).
function hip_graph_step!(ctxs::Vector{Ptr{Void}}, r::Float64; first::Bool = false)
    G = length(ctxs); nnz = Vector{Int64}(G)
    for c in ctxs
        chk(c, ccall((:mpfmt_graph_step_launch, libmpfmt), Int32, (Ptr{Void}, Float64), c, r))
    end
    for (g, c) in enumerate(ctxs)
        n = Ref{Int64}(0)
        chk(c, ccall((:mpfmt_graph_step_finish, libmpfmt), Int32, (Ptr{Void}, Ptr{Int64}), c, n)); nnz[g] = n[]
    end
    hint = first ? div(maximum(nnz) + 63, 64) + 64 : 0
    ccall((:mpfmt_group_begin, libmpfmt), Int32, ())
    for c in ctxs
        chk(c, ccall((:mpfmt_allgather_free_mask_launch, libmpfmt), Int32, (Ptr{Void}, Int64), c, hint))
    end
    ccall((:mpfmt_group_end, libmpfmt), Int32, ())
    hip_gather_finish!(ctxs)
end
function hip_gather_finish!(ctxs::Vector{Ptr{Void}})
    G = length(ctxs)
    out = Vector{Any}(G)
    while true
        again = false
        for (g, c) in enumerate(ctxs)
            ptr = Ref{Ptr{Void}}(C_NULL); stride = Ref{Int64}(0); words = Vector{Int64}(G); nnzs = Vector{Int64}(G)
            rc = ccall((:mpfmt_allgather_free_mask_finish, libmpfmt), Int32,
                       (Ptr{Void}, Ptr{Ptr{Void}}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}), c, ptr, stride, words, nnzs)
            rc == 1 ? (again = true) : chk(c, rc)             # MPFMT_RETRY: a shard outgrew the capacity (every ctx reports it)
            out[g] = (ptr[], stride[], words, nnzs)
        end
        again || return out
        ccall((:mpfmt_group_begin, libmpfmt), Int32, ())
        for c in ctxs
            chk(c, ccall((:mpfmt_allgather_free_mask_relaunch, libmpfmt), Int32, (Ptr{Void},), c))
        end
        ccall((:mpfmt_group_end, libmpfmt), Int32, ())
    end
end

# ---- LinearQuadratic (double integrator): helper_data_structures(V, M::LinearQuadratic) (linearquadratic.jl:68-77) ----------
# States are uploaded with mpfmt_upload_samples(ctx, X, N, 2m), obstacles with mpfmt_upload_boxes(ctx, lohi, M, m, lo, hi, 2m)
# (workspace = first m coordinates, OutputMatrix([I 0]), linearquadratic.jl:51-52).
function helper_data_structures{S}(V::Vector{S}, M::LinearQuadratic, DS::HIPDistanceDS)
    N = length(V); colptr = Vector{Int}(N + 1); nnz = Ref{Int64}(0)
    chk(DS.ctx, ccall((:mpfmt_di_graph_count, libmpfmt), Int32, (Ptr{Void}, Float64, Float64, Ptr{Int64}, Ptr{Int64}),
                      DS.ctx, M.bvp.R[1,1], M.cmax, colptr, nnz))
    rowval = Vector{Int}(nnz[]); nzval = Vector{Float64}(nnz[]); tval = Vector{Float64}(nnz[])
    chk(DS.ctx, ccall((:mpfmt_di_graph_fill, libmpfmt), Int32, (Ptr{Void}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}),
                      DS.ctx, rowval, nzval, tval))
    Dmat = SparseMatrixCSC(N, N, colptr, rowval, nzval)
    BruteDistanceDS(Dmat'), EmptyControlCache(), BruteDistanceDS(Dmat), EmptyControlCache()   # DSF, USF, DSB, USB
end
# every is_free_motion(V[y], V[x], CC, SS) of the steering graph (5 collision waypoints, linearquadratic.jl:85-88) and the
# number of workspace segment tests the reference would have made for it (its CC.count increments)
function hip_di_edges_free(DS::HIPDistanceDS, nnz::Int)
    free = falses(nnz); nseg = Vector{UInt8}(nnz)
    chk(DS.ctx, ccall((:mpfmt_di_graph_edges_free, libmpfmt), Int32, (Ptr{Void}, Ptr{UInt64}, Ptr{UInt8}), DS.ctx, free.chunks, nseg))
    free, nseg
end

# ---- simple cars (simplecars.jl:42-49): chopped Reeds-Shepp metric / Dubins quasi-metric ---------------------------------------
function helper_data_structures{S<:SE2State,R<:ReedsSheppExact}(V::Vector{S}, M::ChoppedMetric{R}, DS::HIPDistanceDS)
    N = length(V); colptr = Vector{Int}(N + 1); nnz = Ref{Int64}(0)
    chk(DS.ctx, ccall((:mpfmt_reedsshepp_graph_count, libmpfmt), Int32, (Ptr{Void}, Float64, Float64, Float64, Ptr{Int64}, Ptr{Int64}),
                      DS.ctx, M.m.r, M.m.s, M.chopval, colptr, nnz))
    rowval = Vector{Int}(nnz[]); nzval = Vector{Float64}(nnz[])
    chk(DS.ctx, ccall((:mpfmt_reedsshepp_graph_fill, libmpfmt), Int32, (Ptr{Void}, Ptr{Int64}, Ptr{Float64}), DS.ctx, rowval, nzval))
    BruteDistanceDS(SparseMatrixCSC(N, N, colptr, rowval, nzval)), EmptyControlCache()      # column v = inball(v), ds = d(v, w)
end
function helper_data_structures{S<:SE2State,R<:DubinsExact}(V::Vector{S}, M::ChoppedQuasiMetric{R}, DS::HIPDistanceDS)
    N = length(V); colptr = Vector{Int}(N + 1); nnz = Ref{Int64}(0)
    chk(DS.ctx, ccall((:mpfmt_dubins_graph_count, libmpfmt), Int32, (Ptr{Void}, Float64, Float64, Float64, Ptr{Int64}, Ptr{Int64}),
                      DS.ctx, M.m.r, M.m.s, M.chopval, colptr, nnz))
    rowval = Vector{Int}(nnz[]); nzval = Vector{Float64}(nnz[])
    chk(DS.ctx, ccall((:mpfmt_dubins_graph_fill, libmpfmt), Int32, (Ptr{Void}, Ptr{Int64}, Ptr{Float64}), DS.ctx, rowval, nzval))
    Dmat = SparseMatrixCSC(N, N, colptr, rowval, nzval)                                      # column x = backward set of x
    BruteDistanceDS(Dmat'), EmptyControlCache(), BruteDistanceDS(Dmat), EmptyControlCache()
end

# ---- closest / closeR (boxesND.jl:33-34,61-86; robots2D.jl:25-26), one call for a batch of query points (columns of P) ----------
function closest(P::Matrix{Float64}, CC::HIPBoxes, W::Matrix{Float64})
    n = size(P, 2); d2 = Vector{Float64}(n); v = similar(P); k = Vector{Int}(n); fails = Ref{Int64}(0)
    chk(CC.ctx, ccall((:mpfmt_closest, libmpfmt), Int32,
                      (Ptr{Void}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}),
                      CC.ctx, P, n, W, d2, v, k, fails))
    fails[] == 0 || error("bvls returned nothing for $(fails[]) (point, box) pair(s)")     # what bvls.jl:67 leads to in the reference
    d2, v
end
function closeR(P::Matrix{Float64}, CC::HIPBoxes, W::Matrix{Float64}, r2::Float64)
    n = size(P, 2); dw = size(P, 1); ptr = Vector{Int}(n + 1); total = Ref{Int64}(0); fails = Ref{Int64}(0)
    cap = n * length(CC.boxes)                   # every (point, obstacle) pair at most
    obstacle = Vector{Int}(cap); d2 = Vector{Float64}(cap); v = Matrix{Float64}(dw, cap)
    chk(CC.ctx, ccall((:mpfmt_closeR, libmpfmt), Int32,
                      (Ptr{Void}, Ptr{Float64}, Int64, Ptr{Float64}, Float64, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64},
                       Ptr{Int64}, Ptr{Int64}),
                      CC.ctx, P, n, W, r2, ptr, cap, obstacle, d2, v, total, fails))
    ptr, obstacle[1:total[]], d2[1:total[]], v[:, 1:total[]]
end

# ---- 2-D SAT world: PointRobot2D(Compound2D(parts)) (robots2D.jl:5-14) -----------------------------------------------------------
# kinds 0 = Circle (cx, cy, r), 1 = Polygon (x1, y1, x2, y2, ...); afterwards every validity entry point of the ctx answers with
# the SAT predicates (SAT2D.jl:119-178) until mpfmt_upload_boxes switches back
function hip_upload_shapes!(ctx::Ptr{Void}, parts::Vector, lo::Vector{Float64}, hi::Vector{Float64})
    kinds = Int32[]; nverts = Int32[]; data = Float64[]
    for s in parts
        if isa(s, Circle)
            push!(kinds, 0); push!(nverts, 0); append!(data, [s.c[1], s.c[2], s.r])
        else
            push!(kinds, 1); push!(nverts, length(s.points)); for p in s.points; append!(data, [p[1], p[2]]); end
        end
    end
    chk(ctx, ccall((:mpfmt_upload_shapes2d, libmpfmt), Int32,
                   (Ptr{Void}, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                   ctx, length(kinds), kinds, nverts, data, lo, hi))
end

# ---- the shape list edited in place (include/mpfmt.h, DESIGN.md 7o): what addobstacle(CC, o) / addblocker(CC, p, r) = Circle(p, r) of
#      robots2D.jl:23-24 become on a resident roadmap -- the free-edge mask of a swept Euclidean graph follows in place and the tracked
#      fields stay (hip_replan! / hip_togo_update! then repair).  ids are 1-based into the flat parts list.  The C caller that executes
#      these calls with the same widths is tests/abi_c/abi_caller13.c.
#      Under a swept steering graph (double integrator in R^4, Dubins, Reeds-Shepp over the shape world) the same two calls keep its
#      mask and segment counts up to date in place once the ctx's option "steer_shapes_delta" is 1 (DESIGN.md 7p; default 0: the graph
#      is swept again): mpfmt_set_option(ctx, "steer_shapes_delta", 1), widths (Ptr{Void}, Cstring, Int64) -> Int32, executed by
#      tests/abi_c/abi_caller14.c.  This glue does not set it. ----
const sym_shapes2d_add = :mpfmt_shapes2d_add
const sym_shapes2d_remove = :mpfmt_shapes2d_remove
function hip_shapes_add!(ctx::Ptr{Void}, parts::Vector)
    kinds = Int32[]; nverts = Int32[]; data = Float64[]
    for s in parts
        if isa(s, Circle)
            push!(kinds, 0); push!(nverts, 0); append!(data, [s.c[1], s.c[2], s.r])
        else
            push!(kinds, 1); push!(nverts, length(s.points)); for p in s.points; append!(data, [p[1], p[2]]); end
        end
    end
    chk(ctx, ccall((sym_shapes2d_add, libmpfmt), Int32, (Ptr{Void}, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}),
                   ctx, length(kinds), kinds, nverts, data))
end
hip_addblocker!(ctx::Ptr{Void}, p, r) = hip_shapes_add!(ctx, Any[Circle(p, r)])
function hip_shapes_remove!(ctx::Ptr{Void}, ids::Vector{Int})
    chk(ctx, ccall((sym_shapes2d_remove, libmpfmt), Int32, (Ptr{Void}, Ptr{Int64}, Int32), ctx, ids, length(ids)))
end

# ---- sample_free!(P, N) (sampling.jl:11-45): the rejection loop in device batches (counter-based stream, sequential semantics) ----
function hip_sample_free!(ctx::Ptr{Void}, seed::UInt64, N::Int, init::Vector{Float64}, goal_kind::Int32, goal_params::Vector{Float64},
                          goal_ct::Int32)
    X = Matrix{Float64}(length(init), N); attempts = Ref{Int64}(0)
    chk(ctx, ccall((:mpfmt_sample_free, libmpfmt), Int32,
                   (Ptr{Void}, UInt64, Int64, Ptr{Float64}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Int64}),
                   ctx, seed, N, init, goal_kind, goal_params, goal_ct, X, attempts))
    X, attempts[]
end
