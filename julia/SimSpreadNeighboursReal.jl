# The neighbour floor for graphs from real-valued rows: the `ccall` layer of include/simspread_hip_neighbours_real.h
# (weighted Jaccard of descriptors, cosine / Tanimoto / Dice of embeddings, each with a per-row k-th-similarity cut next
# to the cutoff alpha: "at least the k nearest sources, whatever alpha says"), one function per exported symbol, on the
# handles of SimSpreadHIP and SimSpreadScreening.
#
#     include("SimSpreadHIP.jl"); include("SimSpreadScreening.jl"); include("SimSpreadNeighboursReal.jl")
#     g = SimSpreadNeighboursReal.graph_features_floor(nothing, X, sparse(y); alpha=0.9, k=6)
#     q = SimSpreadNeighboursReal.queries_features_floor(g, Xnew, X; alpha=0.9, k=6)
#     yhat = SimSpreadScreening.predict_queries(g, q; clean=true)
#
# Row i keeps entry (i, j) iff v != 0 and (s >= alpha or (s > 0 and s >= tau_i)), tau_i the k-th largest of its positive
# similarities (+0 when it has fewer than k: all of them stay).  Ties at tau_i are all kept; negative similarities never
# count among the k; the result is in general not symmetric; alpha = Inf gives the pure k-nearest graph; k = 0 is the
# plain producer.  In a leave-one-out fold the held-out source's own column is dropped as always: pass k + 1 for k
# neighbours in every fold.  Feature matrices are `n x d`, one sample per row (a plain Julia `Matrix`, column-major).
module SimSpreadNeighboursReal

using SparseArrays
using ..SimSpreadHIP: LIB, Graph, check, _csr, _sim_metric, SS_MEM_HOST
using ..SimSpreadScreening: Queries

_second(Fa::Matrix{T}, Fb) where {T} = begin
    na, d = size(Fa)
    Fb === nothing || size(Fb, 2) == d || throw(ArgumentError("Fa and Fb have different numbers of features"))
    (na, d, Fb === nothing ? na : size(Fb, 1), Fb === nothing ? Ptr{T}(C_NULL) : pointer(Fb))
end

"""
    jaccard_kth(Fa::Matrix{T}, Fb=nothing; k) where T<:Union{Float32,Float64}

`tau[i]`: the `k`-th largest positive weighted-Jaccard similarity of row `i` of `Fa` against the rows of `Fb` (`nothing`:
`Fa` itself, the diagonal included), `0` where there are fewer than `k`.  `1 <= k <= 64`.
"""
function jaccard_kth(Fa::Matrix{T}, Fb::Union{Nothing,Matrix{T}}=nothing; k::Integer) where {T<:Union{Float32,Float64}}
    na, d, nb, pb = _second(Fa, Fb)
    tau = Vector{T}(undef, na)
    rc = GC.@preserve Fa Fb if T === Float32
        ccall((:ss_similarity_jaccard_kth_f32, LIB), Cint,
              (Ptr{Float32}, Int64, Int64, Ptr{Float32}, Int64, Int64, Int64, Cint, Ptr{Float32}, Cint),
              Fa, na, max(na, 1), pb, nb, max(nb, 1), d, k, tau, SS_MEM_HOST)
    else
        ccall((:ss_similarity_jaccard_kth_f64, LIB), Cint,
              (Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Int64, Int64, Cint, Ptr{Float64}, Cint),
              Fa, na, max(na, 1), pb, nb, max(nb, 1), d, k, tau, SS_MEM_HOST)
    end
    check(rc)
    return tau
end

"""
    dot_kth(Fa::Matrix{T}, Fb=nothing; metric=:cosine, k) where T<:Union{Float32,Float64}

`tau[i]` of `dot_floor_csr`: the `k`-th largest positive similarity `metric` of row `i` of `Fa` against the rows of `Fb`
(`nothing`: `Fa` itself, the diagonal, exactly 1, included), `0` where there are fewer than `k`.  `1 <= k <= 64`.
"""
function dot_kth(Fa::Matrix{T}, Fb::Union{Nothing,Matrix{T}}=nothing; metric::Symbol=:cosine,
                 k::Integer) where {T<:Union{Float32,Float64}}
    na, d, nb, pb = _second(Fa, Fb)
    m = _sim_metric(metric)
    tau = Vector{T}(undef, na)
    rc = GC.@preserve Fa Fb if T === Float32
        ccall((:ss_similarity_dot_kth_f32, LIB), Cint,
              (Ptr{Float32}, Int64, Int64, Ptr{Float32}, Int64, Int64, Int64, Cint, Cint, Ptr{Float32}, Cint),
              Fa, na, max(na, 1), pb, nb, max(nb, 1), d, m, k, tau, SS_MEM_HOST)
    else
        ccall((:ss_similarity_dot_kth_f64, LIB), Cint,
              (Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Int64, Int64, Cint, Cint, Ptr{Float64}, Cint),
              Fa, na, max(na, 1), pb, nb, max(nb, 1), d, m, k, tau, SS_MEM_HOST)
    end
    check(rc)
    return tau
end

# the size protocol of the two CSR producers: call(idx, val, capacity) is the `ccall` with everything else bound
function _two_calls(call, ::Type{T}, na, nb, ptr, nnz) where {T}
    check(call(Ptr{Int32}(C_NULL), Ptr{T}(C_NULL), 0))             # size query
    idx, val = Vector{Int32}(undef, nnz[]), Vector{T}(undef, nnz[])
    check(call(idx, val, nnz[]))
    # row-major CSR of (na x nb) == CSC of its (nb x na) transpose, 1-based
    return permutedims(SparseMatrixCSC(nb, na, ptr .+ 1, Vector{Int}(idx) .+ 1, val))
end

"""
    jaccard_floor_csr(Fa::Matrix{T}, Fb=nothing; alpha, k, weighted=true)

`SimSpreadHIP.jaccard_csr` with the neighbour floor `k` (`0 <= k <= 64`).  Returns the `na x nb` matrix as a
`SparseMatrixCSC`.
"""
function jaccard_floor_csr(Fa::Matrix{T}, Fb::Union{Nothing,Matrix{T}}=nothing; alpha::Real, k::Integer,
                           weighted::Bool=true) where {T<:Union{Float32,Float64}}
    na, d, nb, pb = _second(Fa, Fb)
    ptr = Vector{Int64}(undef, na + 1)
    nnz = Ref{Int64}(0)
    call(idx, val, cap) = if T === Float32
        ccall((:ss_similarity_jaccard_floor_csr_f32, LIB), Cint,
              (Ptr{Float32}, Int64, Int64, Ptr{Float32}, Int64, Int64, Int64, Float32, Cint, Cint, Ptr{Int64},
               Ptr{Int32}, Ptr{Float32}, Int64, Ptr{Int64}, Cint),
              Fa, na, max(na, 1), pb, nb, max(nb, 1), d, Float32(alpha), k, weighted ? 1 : 0, ptr, idx, val, cap, nnz,
              SS_MEM_HOST)
    else
        ccall((:ss_similarity_jaccard_floor_csr_f64, LIB), Cint,
              (Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Int64, Int64, Float64, Cint, Cint, Ptr{Int64},
               Ptr{Int32}, Ptr{Float64}, Int64, Ptr{Int64}, Cint),
              Fa, na, max(na, 1), pb, nb, max(nb, 1), d, Float64(alpha), k, weighted ? 1 : 0, ptr, idx, val, cap, nnz,
              SS_MEM_HOST)
    end
    return GC.@preserve Fa Fb _two_calls(call, T, na, nb, ptr, nnz)
end

"""
    dot_floor_csr(Fa::Matrix{T}, Fb=nothing; metric=:cosine, alpha, k, weighted=true)

`SimSpreadHIP.dot_csr` with the neighbour floor `k` (`0 <= k <= 64`).  Negative similarities never count among the `k`;
with `Fb === nothing` the diagonal is exactly 1 and counts, and the result is in general not symmetric.
"""
function dot_floor_csr(Fa::Matrix{T}, Fb::Union{Nothing,Matrix{T}}=nothing; metric::Symbol=:cosine, alpha::Real,
                       k::Integer, weighted::Bool=true) where {T<:Union{Float32,Float64}}
    na, d, nb, pb = _second(Fa, Fb)
    m = _sim_metric(metric)
    ptr = Vector{Int64}(undef, na + 1)
    nnz = Ref{Int64}(0)
    call(idx, val, cap) = if T === Float32
        ccall((:ss_similarity_dot_floor_csr_f32, LIB), Cint,
              (Ptr{Float32}, Int64, Int64, Ptr{Float32}, Int64, Int64, Int64, Cint, Float32, Cint, Cint, Ptr{Int64},
               Ptr{Int32}, Ptr{Float32}, Int64, Ptr{Int64}, Cint),
              Fa, na, max(na, 1), pb, nb, max(nb, 1), d, m, Float32(alpha), k, weighted ? 1 : 0, ptr, idx, val, cap, nnz,
              SS_MEM_HOST)
    else
        ccall((:ss_similarity_dot_floor_csr_f64, LIB), Cint,
              (Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Int64, Int64, Cint, Float64, Cint, Cint, Ptr{Int64},
               Ptr{Int32}, Ptr{Float64}, Int64, Ptr{Int64}, Cint),
              Fa, na, max(na, 1), pb, nb, max(nb, 1), d, m, Float64(alpha), k, weighted ? 1 : 0, ptr, idx, val, cap, nnz,
              SS_MEM_HOST)
    end
    return GC.@preserve Fa Fb _two_calls(call, T, na, nb, ptr, nnz)
end

function _graph_sizes(Fq, Fs::Matrix{T}, Y::SparseMatrixCSC) where {T}
    ns, d = size(Fs)
    nq = Fq === nothing ? 0 : size(Fq, 1)
    Fq === nothing || size(Fq, 2) == d || throw(ArgumentError("Fq and Fs have different numbers of features"))
    size(Y, 1) == ns || throw(AssertionError("Labels and features have different number of source nodes"))
    (nq, ns, d, size(Y, 2), Fq === nothing ? Ptr{T}(C_NULL) : pointer(Fq))
end

"""
    graph_features_floor(Fq, Fs::Matrix{T}, Y::SparseMatrixCSC; alpha, k, weighted=true)

`SimSpreadHIP.graph_features` with the neighbour floor: every source and every query also keeps its `k` nearest sources.
An ordinary CSR graph afterwards.
"""
function graph_features_floor(Fq::Union{Nothing,Matrix{T}}, Fs::Matrix{T}, Y::SparseMatrixCSC; alpha::Real, k::Integer,
                              weighted::Bool=true) where {T<:Union{Float32,Float64}}
    nq, ns, d, nt, pq = _graph_sizes(Fq, Fs, Y)
    yp, yi, yv = _csr(Y, T)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = GC.@preserve Fq if T === Float32
        ccall((:ss_graph_create_features_floor_f32, LIB), Cint,
              (Int64, Int64, Int64, Int64, Ptr{Float32}, Int64, Ptr{Float32}, Int64, Ptr{Int64}, Ptr{Int32},
               Ptr{Float32}, Cint, Float32, Cint, Cint, Cint, Ref{Ptr{Cvoid}}),
              nq, ns, nt, d, pq, max(nq, 1), Fs, max(ns, 1), yp, yi, yv, 1, Float32(alpha), k, weighted ? 1 : 0,
              SS_MEM_HOST, h)
    else
        ccall((:ss_graph_create_features_floor_f64, LIB), Cint,
              (Int64, Int64, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Int32},
               Ptr{Float64}, Cint, Float64, Cint, Cint, Cint, Ref{Ptr{Cvoid}}),
              nq, ns, nt, d, pq, max(nq, 1), Fs, max(ns, 1), yp, yi, yv, 1, Float64(alpha), k, weighted ? 1 : 0,
              SS_MEM_HOST, h)
    end
    check(rc)
    return Graph{T}(h[], nq, ns, ns, nt)
end

"""
    graph_vectors_floor(Fq, Fs::Matrix{T}, Y::SparseMatrixCSC; metric=:cosine, alpha, k, weighted=true)

`SimSpreadHIP.graph_vectors` with the neighbour floor: every source and every query also keeps its `k` nearest sources
(the `k` largest positive similarities).  An ordinary CSR graph afterwards.
"""
function graph_vectors_floor(Fq::Union{Nothing,Matrix{T}}, Fs::Matrix{T}, Y::SparseMatrixCSC; metric::Symbol=:cosine,
                             alpha::Real, k::Integer, weighted::Bool=true) where {T<:Union{Float32,Float64}}
    nq, ns, d, nt, pq = _graph_sizes(Fq, Fs, Y)
    m = _sim_metric(metric)
    yp, yi, yv = _csr(Y, T)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = GC.@preserve Fq if T === Float32
        ccall((:ss_graph_create_vectors_floor_f32, LIB), Cint,
              (Int64, Int64, Int64, Int64, Cint, Ptr{Float32}, Int64, Ptr{Float32}, Int64, Ptr{Int64}, Ptr{Int32},
               Ptr{Float32}, Cint, Float32, Cint, Cint, Cint, Ref{Ptr{Cvoid}}),
              nq, ns, nt, d, m, pq, max(nq, 1), Fs, max(ns, 1), yp, yi, yv, 1, Float32(alpha), k, weighted ? 1 : 0,
              SS_MEM_HOST, h)
    else
        ccall((:ss_graph_create_vectors_floor_f64, LIB), Cint,
              (Int64, Int64, Int64, Int64, Cint, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Int32},
               Ptr{Float64}, Cint, Float64, Cint, Cint, Cint, Ref{Ptr{Cvoid}}),
              nq, ns, nt, d, m, pq, max(nq, 1), Fs, max(ns, 1), yp, yi, yv, 1, Float64(alpha), k, weighted ? 1 : 0,
              SS_MEM_HOST, h)
    end
    check(rc)
    return Graph{T}(h[], nq, ns, ns, nt)
end

"`queries_features_floor(g, Fq, Fs; alpha, k, weighted)`: the cross block of `graph_features_floor`; every query keeps its `k` nearest sources."
function queries_features_floor(g::Graph{T}, Fq::Matrix{T}, Fs::Matrix{T}; alpha::Real, k::Integer,
                                weighted::Bool=true) where {T}
    ns, d = size(Fs)
    size(Fq, 2) == d || throw(ArgumentError("Fq and Fs have different numbers of features"))
    nq = size(Fq, 1)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = if T === Float32
        ccall((:ss_queries_create_features_floor_f32, LIB), Cint,
              (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Float32}, Int64, Ptr{Float32}, Int64, Float32, Cint, Cint, Cint,
               Ref{Ptr{Cvoid}}),
              g.handle, nq, ns, d, Fq, max(nq, 1), Fs, max(ns, 1), Float32(alpha), k, weighted ? 1 : 0, SS_MEM_HOST, h)
    else
        ccall((:ss_queries_create_features_floor_f64, LIB), Cint,
              (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Float64, Cint, Cint, Cint,
               Ref{Ptr{Cvoid}}),
              g.handle, nq, ns, d, Fq, max(nq, 1), Fs, max(ns, 1), Float64(alpha), k, weighted ? 1 : 0, SS_MEM_HOST, h)
    end
    check(rc)
    return Queries{T}(h[])
end

"`queries_vectors_floor(g, Fq, Fs; metric, alpha, k, weighted)`: the cross block of `graph_vectors_floor`; every query keeps its `k` nearest sources."
function queries_vectors_floor(g::Graph{T}, Fq::Matrix{T}, Fs::Matrix{T}; metric::Symbol=:cosine, alpha::Real,
                               k::Integer, weighted::Bool=true) where {T}
    ns, d = size(Fs)
    size(Fq, 2) == d || throw(ArgumentError("Fq and Fs have different numbers of features"))
    nq = size(Fq, 1)
    m = _sim_metric(metric)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = if T === Float32
        ccall((:ss_queries_create_vectors_floor_f32, LIB), Cint,
              (Ptr{Cvoid}, Int64, Int64, Int64, Cint, Ptr{Float32}, Int64, Ptr{Float32}, Int64, Float32, Cint, Cint, Cint,
               Ref{Ptr{Cvoid}}),
              g.handle, nq, ns, d, m, Fq, max(nq, 1), Fs, max(ns, 1), Float32(alpha), k, weighted ? 1 : 0, SS_MEM_HOST, h)
    else
        ccall((:ss_queries_create_vectors_floor_f64, LIB), Cint,
              (Ptr{Cvoid}, Int64, Int64, Int64, Cint, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Float64, Cint, Cint, Cint,
               Ref{Ptr{Cvoid}}),
              g.handle, nq, ns, d, m, Fq, max(nq, 1), Fs, max(ns, 1), Float64(alpha), k, weighted ? 1 : 0, SS_MEM_HOST, h)
    end
    check(rc)
    return Queries{T}(h[])
end

end # module
