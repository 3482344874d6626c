# Prospective screening on a resident graph: the `ccall` layer of include/simspread_hip_screening.h (query sets bound to
# a graph, support lists of (row, target) hits), one function per exported symbol, on the handles of SimSpreadHIP.
#
#     include("SimSpreadHIP.jl"); include("SimSpreadScreening.jl")
#     g = SimSpreadHIP.graph_fingerprint(nothing, F, sparse(y); alpha=0.5)
#     q = SimSpreadScreening.queries_fingerprint(g, Fb, F; alpha=0.5)
#     yhat = SimSpreadScreening.predict_queries(g, q; clean=true)
module SimSpreadScreening

using SparseArrays
using ..SimSpreadHIP: LIB, Graph, check, _csr, _sim_metric, SS_MEM_HOST, SS_ROWS_QUERY, SS_LAYOUT_COLMAJOR

const SS_ROWS_LOO = Cint(2)

"""
A block of query rows bound to one resident graph (`ss_queries_*`): build and cross-validate a graph once, then screen
new batches on it.  `predict(g, q)` gives bitwise the scores of the graph built with these queries, and nothing the
graph itself returns changes while query sets exist.
"""
mutable struct Queries{T<:Union{Float32,Float64}}
    handle::Ptr{Cvoid}
    nq::Int
    nf::Int
    function Queries{T}(h) where {T}
        sizes = Vector{Int64}(undef, 3)
        check(ccall((:ss_queries_info, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}), h, sizes))
        q = new{T}(h, sizes[1], sizes[2])
        finalizer(destroy!, q)
        return q
    end
end

function destroy!(q::Queries)
    if q.handle != C_NULL
        ccall((:ss_queries_destroy, LIB), Cint, (Ptr{Cvoid},), q.handle)
        q.handle = C_NULL
    end
    return nothing
end

"`queries(g, Xq)`: the `nq x nf` block itself."
function queries(g::Graph{T}, Xq::SparseMatrixCSC) where {T}
    size(Xq, 2) == g.nf || throw(AssertionError("Number of features between test and training sets doesn't match"))
    qp, qi, qv = _csr(Xq, T)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = if T === Float32
        ccall((:ss_queries_create_csr_f32, LIB), Cint,
              (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Float32}, Cint, Cint, Ref{Ptr{Cvoid}}),
              g.handle, size(Xq, 1), qp, qi, qv, 1, SS_MEM_HOST, h)
    else
        ccall((:ss_queries_create_csr_f64, LIB), Cint,
              (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Float64}, Cint, Cint, Ref{Ptr{Cvoid}}),
              g.handle, size(Xq, 1), qp, qi, qv, 1, SS_MEM_HOST, h)
    end
    check(rc)
    return Queries{T}(h[])
end

"`queries_fingerprint(g, Fq, Fs; alpha, weighted)`: the cross block of `graph_fingerprint` (pass its `Fs`, `alpha`, `weighted`)."
function queries_fingerprint(g::Graph{T}, Fq::Matrix{UInt64}, Fs::Matrix{UInt64}; alpha::Real,
                             weighted::Bool=true) where {T}
    nwords, ns = size(Fs)
    size(Fq, 1) == nwords || throw(ArgumentError("Fq and Fs have different fingerprint widths"))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = if T === Float32
        ccall((:ss_queries_create_fingerprint_f32, LIB), Cint,
              (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{UInt64}, Ptr{UInt64}, Float32, Cint, Cint, Ref{Ptr{Cvoid}}),
              g.handle, size(Fq, 2), ns, nwords, Fq, Fs, Float32(alpha), weighted ? 1 : 0, SS_MEM_HOST, h)
    else
        ccall((:ss_queries_create_fingerprint_f64, LIB), Cint,
              (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{UInt64}, Ptr{UInt64}, Float64, Cint, Cint, Ref{Ptr{Cvoid}}),
              g.handle, size(Fq, 2), ns, nwords, Fq, Fs, Float64(alpha), weighted ? 1 : 0, SS_MEM_HOST, h)
    end
    check(rc)
    return Queries{T}(h[])
end

"`queries_features(g, Fq, Fs; alpha, weighted)`: the cross block of `graph_features`."
function queries_features(g::Graph{T}, Fq::Matrix{T}, Fs::Matrix{T}; alpha::Real, weighted::Bool=true) where {T}
    ns, d = size(Fs)
    size(Fq, 2) == d || throw(ArgumentError("Fq and Fs have different numbers of features"))
    nq = size(Fq, 1)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = if T === Float32
        ccall((:ss_queries_create_features_f32, LIB), Cint,
              (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Float32}, Int64, Ptr{Float32}, Int64, Float32, Cint, Cint,
               Ref{Ptr{Cvoid}}),
              g.handle, nq, ns, d, Fq, max(nq, 1), Fs, max(ns, 1), Float32(alpha), weighted ? 1 : 0, SS_MEM_HOST, h)
    else
        ccall((:ss_queries_create_features_f64, LIB), Cint,
              (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Float64, Cint, Cint,
               Ref{Ptr{Cvoid}}),
              g.handle, nq, ns, d, Fq, max(nq, 1), Fs, max(ns, 1), Float64(alpha), weighted ? 1 : 0, SS_MEM_HOST, h)
    end
    check(rc)
    return Queries{T}(h[])
end

"`queries_vectors(g, Fq, Fs; metric, alpha, weighted)`: the cross block of `graph_vectors`."
function queries_vectors(g::Graph{T}, Fq::Matrix{T}, Fs::Matrix{T}; metric::Symbol=:cosine, alpha::Real,
                         weighted::Bool=true) where {T}
    ns, d = size(Fs)
    size(Fq, 2) == d || throw(ArgumentError("Fq and Fs have different numbers of features"))
    nq = size(Fq, 1)
    m = _sim_metric(metric)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = if T === Float32
        ccall((:ss_queries_create_vectors_f32, LIB), Cint,
              (Ptr{Cvoid}, Int64, Int64, Int64, Cint, Ptr{Float32}, Int64, Ptr{Float32}, Int64, Float32, Cint, Cint,
               Ref{Ptr{Cvoid}}),
              g.handle, nq, ns, d, m, Fq, max(nq, 1), Fs, max(ns, 1), Float32(alpha), weighted ? 1 : 0, SS_MEM_HOST, h)
    else
        ccall((:ss_queries_create_vectors_f64, LIB), Cint,
              (Ptr{Cvoid}, Int64, Int64, Int64, Cint, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Float64, Cint, Cint,
               Ref{Ptr{Cvoid}}),
              g.handle, nq, ns, d, m, Fq, max(nq, 1), Fs, max(ns, 1), Float64(alpha), weighted ? 1 : 0, SS_MEM_HOST, h)
    end
    check(rc)
    return Queries{T}(h[])
end

"Stored entries of every query row; 0 = outside the applicability domain."
function queries_degrees(q::Queries)
    kq = Vector{Int64}(undef, q.nq)
    check(ccall((:ss_queries_degrees, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Cint), q.handle, kq, SS_MEM_HOST))
    return kq
end

"`predict_queries(g, q; clean, range)`: the rows of the query set `q` against all targets."
function predict_queries(g::Graph{T}, q::Queries{T}; clean::Bool=false, range=nothing) where {T}
    lo, hi = range === nothing ? (0, q.nq) : (first(range) - 1, last(range))
    out = Matrix{T}(undef, hi - lo, g.nt)
    rc = if T === Float32
        ccall((:ss_predict_queries_f32, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Cint, Ptr{Float32}, Int64, Cint, Cint),
              g.handle, q.handle, lo, hi, clean ? 1 : 0, out, max(hi - lo, 1), SS_LAYOUT_COLMAJOR, SS_MEM_HOST)
    else
        ccall((:ss_predict_queries_f64, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Cint, Ptr{Float64}, Int64, Cint, Cint),
              g.handle, q.handle, lo, hi, clean ? 1 : 0, out, max(hi - lo, 1), SS_LAYOUT_COLMAJOR, SS_MEM_HOST)
    end
    check(rc)
    return Matrix{Float64}(out)
end

"""
    support(g, rows, targets; M=16, queries=nothing, loo=false) -> (src, contrib, nsupp)

Which sources carry the scores of the pairs `zip(rows, targets)` (1-based): column `p` of `src` / `contrib` lists the
sources with the largest contributions `T[r,s] * Ys[s,t]` in descending order (`src` 1-based, 0 = unused slot),
`nsupp[p]` how many sources contribute at all.  Rows of `queries`, of the graph's own query block, or leave-one-out
folds (`loo=true`).
"""
function support(g::Graph{T}, rows::AbstractVector{<:Integer}, targets::AbstractVector{<:Integer}; M::Integer=16,
                 queries::Union{Nothing,Queries{T}}=nothing, loo::Bool=false) where {T}
    length(rows) == length(targets) || throw(ArgumentError("one target per row is needed"))
    n = length(rows)
    r, t = Vector{Int64}(rows .- 1), Vector{Int32}(targets .- 1)
    src, contrib, nsupp = Matrix{Int32}(undef, max(M, 1), n), Matrix{T}(undef, max(M, 1), n), Vector{Int32}(undef, n)
    qh = queries === nothing ? C_NULL : queries.handle
    kind = loo ? SS_ROWS_LOO : SS_ROWS_QUERY
    rc = if T === Float32
        ccall((:ss_support_f32, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Ptr{Int64}, Ptr{Int32}, Cint, Ptr{Int32}, Ptr{Float32}, Ptr{Int32}, Cint),
              g.handle, qh, kind, n, r, t, M, src, contrib, nsupp, SS_MEM_HOST)
    else
        ccall((:ss_support_f64, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Ptr{Int64}, Ptr{Int32}, Cint, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}, Cint),
              g.handle, qh, kind, n, r, t, M, src, contrib, nsupp, SS_MEM_HOST)
    end
    check(rc)
    return src .+ Int32(1), Matrix{Float64}(contrib), Vector{Int}(nsupp)
end

end # module
