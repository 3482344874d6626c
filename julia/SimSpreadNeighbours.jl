# Fingerprint graphs with a neighbour floor: the `ccall` layer of include/simspread_hip_neighbours.h (a per-row
# k-th-similarity cut next to the cutoff alpha: "at least the k nearest sources, whatever alpha says"), one function per
# exported symbol, on the handles of SimSpreadHIP and SimSpreadScreening.
#
#     include("SimSpreadHIP.jl"); include("SimSpreadScreening.jl"); include("SimSpreadNeighbours.jl")
#     g = SimSpreadNeighbours.graph_fingerprint_floor(nothing, F, sparse(y); alpha=0.5, k=8)
#     q = SimSpreadNeighbours.queries_fingerprint_floor(g, Fb, F; alpha=0.5, k=8)
#     yhat = SimSpreadScreening.predict_queries(g, q; clean=true)
#
# Row i keeps entry (i, j) iff v != 0 and (s >= alpha or (s > 0 and s >= tau_i)), tau_i the k-th largest of its positive
# similarities (+0 when it has fewer than k: all of them stay).  Ties at tau_i are all kept, so a row may get more than
# k entries; the result is in general not symmetric; alpha = Inf gives the pure k-nearest graph; k = 0 is the plain
# producer.  In a leave-one-out fold the held-out source's own column is dropped as always: pass k + 1 for k neighbours
# in every fold.  `ss_graph_recut_*` treats a floor graph as any other parent.
module SimSpreadNeighbours

using SparseArrays
using ..SimSpreadHIP: LIB, Graph, check, _csr, SS_MEM_HOST
using ..SimSpreadScreening: Queries

"""
    tanimoto_kth(Fa::Matrix{UInt64}, Fb=nothing; k, T=Float32)

`tau[i]`: the `k`-th largest positive Tanimoto similarity of fingerprint `i` of `Fa` (`nwords x na`) against those of `Fb`
(`nothing`: `Fa` itself, the diagonal included), `0` where there are fewer than `k`.  `1 <= k <= 64`.
"""
function tanimoto_kth(Fa::Matrix{UInt64}, Fb::Union{Nothing,Matrix{UInt64}}=nothing; k::Integer, T::Type=Float32)
    nwords, na = size(Fa)
    nb = Fb === nothing ? na : size(Fb, 2)
    Fb === nothing || size(Fb, 1) == nwords || throw(ArgumentError("Fa and Fb have different fingerprint widths"))
    pb = Fb === nothing ? Ptr{UInt64}(C_NULL) : pointer(Fb)
    tau = Vector{T}(undef, na)
    rc = GC.@preserve Fa Fb if T === Float32
        ccall((:ss_similarity_tanimoto_kth_f32, LIB), Cint,
              (Ptr{UInt64}, Int64, Ptr{UInt64}, Int64, Int64, Cint, Ptr{Float32}, Cint),
              Fa, na, pb, nb, nwords, k, tau, SS_MEM_HOST)
    else
        ccall((:ss_similarity_tanimoto_kth_f64, LIB), Cint,
              (Ptr{UInt64}, Int64, Ptr{UInt64}, Int64, Int64, Cint, Ptr{Float64}, Cint),
              Fa, na, pb, nb, nwords, k, tau, SS_MEM_HOST)
    end
    check(rc)
    return tau
end

"""
    tanimoto_floor_csr(Fa::Matrix{UInt64}, Fb=nothing; alpha, k, weighted=true, T=Float32)

`SimSpreadHIP.tanimoto_csr` with the neighbour floor `k` (`0 <= k <= 64`).  Returns the `na x nb` matrix as a
`SparseMatrixCSC`.
"""
function tanimoto_floor_csr(Fa::Matrix{UInt64}, Fb::Union{Nothing,Matrix{UInt64}}=nothing; alpha::Real, k::Integer,
                            weighted::Bool=true, T::Type=Float32)
    nwords, na = size(Fa)
    nb = Fb === nothing ? na : size(Fb, 2)
    Fb === nothing || size(Fb, 1) == nwords || throw(ArgumentError("Fa and Fb have different fingerprint widths"))
    pb = Fb === nothing ? Ptr{UInt64}(C_NULL) : pointer(Fb)
    ptr = Vector{Int64}(undef, na + 1)
    nnz = Ref{Int64}(0)
    call(idx, val, cap) = if T === Float32
        ccall((:ss_similarity_tanimoto_floor_csr_f32, LIB), Cint,
              (Ptr{UInt64}, Int64, Ptr{UInt64}, Int64, Int64, Float32, Cint, Cint, Ptr{Int64}, Ptr{Int32}, Ptr{Float32},
               Int64, Ptr{Int64}, Cint),
              Fa, na, pb, nb, nwords, Float32(alpha), k, weighted ? 1 : 0, ptr, idx, val, cap, nnz, SS_MEM_HOST)
    else
        ccall((:ss_similarity_tanimoto_floor_csr_f64, LIB), Cint,
              (Ptr{UInt64}, Int64, Ptr{UInt64}, Int64, Int64, Float64, Cint, Cint, Ptr{Int64}, Ptr{Int32}, Ptr{Float64},
               Int64, Ptr{Int64}, Cint),
              Fa, na, pb, nb, nwords, Float64(alpha), k, weighted ? 1 : 0, ptr, idx, val, cap, nnz, SS_MEM_HOST)
    end
    GC.@preserve Fa Fb begin
        check(call(Ptr{Int32}(C_NULL), Ptr{T}(C_NULL), 0))             # size query
        idx, val = Vector{Int32}(undef, nnz[]), Vector{T}(undef, nnz[])
        check(call(idx, val, nnz[]))
    end
    # row-major CSR of (na x nb) == CSC of its (nb x na) transpose, 1-based
    return permutedims(SparseMatrixCSC(nb, na, ptr .+ 1, Vector{Int}(idx) .+ 1, val))
end

"""
    graph_fingerprint_floor(Fq, Fs::Matrix{UInt64}, Y::SparseMatrixCSC; alpha, k, weighted=true, T=Float32)

`SimSpreadHIP.graph_fingerprint` with the neighbour floor: every source and every query also keeps its `k` nearest
sources.  An ordinary CSR graph afterwards.
"""
function graph_fingerprint_floor(Fq::Union{Nothing,Matrix{UInt64}}, Fs::Matrix{UInt64}, Y::SparseMatrixCSC;
                                 alpha::Real, k::Integer, weighted::Bool=true, T::Type=Float32)
    nwords, ns = size(Fs)
    nq = Fq === nothing ? 0 : size(Fq, 2)
    Fq === nothing || size(Fq, 1) == nwords || throw(ArgumentError("Fq and Fs have different fingerprint widths"))
    size(Y, 1) == ns || throw(AssertionError("Labels and features have different number of source nodes"))
    pq = Fq === nothing ? Ptr{UInt64}(C_NULL) : pointer(Fq)
    yp, yi, yv = _csr(Y, T)
    nt = size(Y, 2)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = GC.@preserve Fq if T === Float32
        ccall((:ss_graph_create_fingerprint_floor_f32, LIB), Cint,
              (Int64, Int64, Int64, Int64, Ptr{UInt64}, Ptr{UInt64}, Ptr{Int64}, Ptr{Int32}, Ptr{Float32},
               Cint, Float32, Cint, Cint, Cint, Ref{Ptr{Cvoid}}),
              nq, ns, nt, nwords, pq, Fs, yp, yi, yv, 1, Float32(alpha), k, weighted ? 1 : 0, SS_MEM_HOST, h)
    else
        ccall((:ss_graph_create_fingerprint_floor_f64, LIB), Cint,
              (Int64, Int64, Int64, Int64, Ptr{UInt64}, Ptr{UInt64}, Ptr{Int64}, Ptr{Int32}, Ptr{Float64},
               Cint, Float64, Cint, Cint, Cint, Ref{Ptr{Cvoid}}),
              nq, ns, nt, nwords, pq, Fs, yp, yi, yv, 1, Float64(alpha), k, weighted ? 1 : 0, SS_MEM_HOST, h)
    end
    check(rc)
    return Graph{T}(h[], nq, ns, ns, nt)
end

"`queries_fingerprint_floor(g, Fq, Fs; alpha, k, weighted)`: the cross block with the floor; every query keeps its `k` nearest sources."
function queries_fingerprint_floor(g::Graph{T}, Fq::Matrix{UInt64}, Fs::Matrix{UInt64}; alpha::Real, k::Integer,
                                   weighted::Bool=true) where {T}
    nwords, ns = size(Fs)
    size(Fq, 1) == nwords || throw(ArgumentError("Fq and Fs have different fingerprint widths"))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = if T === Float32
        ccall((:ss_queries_create_fingerprint_floor_f32, LIB), Cint,
              (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{UInt64}, Ptr{UInt64}, Float32, Cint, Cint, Cint, Ref{Ptr{Cvoid}}),
              g.handle, size(Fq, 2), ns, nwords, Fq, Fs, Float32(alpha), k, weighted ? 1 : 0, SS_MEM_HOST, h)
    else
        ccall((:ss_queries_create_fingerprint_floor_f64, LIB), Cint,
              (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{UInt64}, Ptr{UInt64}, Float64, Cint, Cint, Cint, Ref{Ptr{Cvoid}}),
              g.handle, size(Fq, 2), ns, nwords, Fq, Fs, Float64(alpha), k, weighted ? 1 : 0, SS_MEM_HOST, h)
    end
    check(rc)
    return Queries{T}(h[])
end

end # module
