# Graphs from embeddings stored in 16 bits: the `ccall` layer of include/simspread_hip_half.h (the inner-product producer
# -- cosine / Tanimoto / Dice -- on bfloat16 or Float16 rows, computed on the 16-bit matrix instructions with Float32
# accumulation), one function per exported symbol, on the handles of SimSpreadHIP and SimSpreadScreening.
#
#     include("SimSpreadHIP.jl"); include("SimSpreadScreening.jl"); include("SimSpreadHalf.jl")
#     E = Float16.(embeddings)                       # d x n: ONE SAMPLE PER COLUMN
#     g = SimSpreadHalf.graph_vectors_h16(nothing, E, sparse(y); alpha=0.8)
#     q = SimSpreadHalf.queries_vectors_h16(g, Enew, E; alpha=0.8)
#
# LAYOUT: unlike every other feature matrix of these bindings (`n x d`, one sample per row), the 16-bit matrices are
# `d x n`, one sample per column: the library reads 16-bit rows row-major, element (i, k) at F[i * ld + k], which is a
# column-major Julia `d x n` matrix with ld = d.  `Matrix{Float16}` is storage `:f16`; `Matrix{UInt16}` holds raw bit
# patterns of the storage named by `storage` (`:bf16` by default: the upper halves of Float32 values).  Every product of
# two 16-bit values is exact in Float32, so the result is a valid output of the Float32 rule on the widened inputs up to
# the order of the sums.  The graph is a `Graph{Float32}`; a NaN pattern is refused.
module SimSpreadHalf

using SparseArrays
using ..SimSpreadHIP: LIB, Graph, check, _csr, _sim_metric, SS_MEM_HOST
using ..SimSpreadScreening: Queries

const SS_H16_BF16 = Cint(0)
const SS_H16_F16 = Cint(1)

const Half = Union{Matrix{Float16},Matrix{UInt16}}
_storage(::Matrix{Float16}, storage) = SS_H16_F16
_storage(::Matrix{UInt16}, storage::Symbol) =
    storage === :bf16 ? SS_H16_BF16 : storage === :f16 ? SS_H16_F16 : throw(ArgumentError("storage must be :bf16 or :f16"))
# one storage per call: both matrices must be of the same element type (a `Matrix{UInt16}` of bf16 patterns next to a
# `Matrix{Float16}` would otherwise be read as Float16)
function _storage(F::Half, G::Union{Nothing,Half}, storage)
    G === nothing || eltype(F) === eltype(G) ||
        throw(ArgumentError("both feature matrices must be Matrix{Float16} or both Matrix{UInt16}"))
    return _storage(F, storage)
end
_bits(F::Matrix{UInt16}) = F
_bits(F::Matrix{Float16}) = reinterpret(UInt16, F)

"""
    dot_csr_h16(Fa, Fb=nothing; storage=:bf16, metric=:cosine, alpha, weighted=true)

`SimSpreadHIP.dot_csr` on 16-bit columns: `Fa` is `d x na`, `Fb` `d x nb` (`nothing`: `Fa` against itself).  Returns the
`na x nb` matrix as a `SparseMatrixCSC{Float32}`.
"""
function dot_csr_h16(Fa::Half, Fb::Union{Nothing,Half}=nothing; storage::Symbol=:bf16, metric::Symbol=:cosine,
                     alpha::Real, weighted::Bool=true)
    d, na = size(Fa)
    Fb === nothing || size(Fb, 1) == d || throw(ArgumentError("Fa and Fb have different numbers of features"))
    nb = Fb === nothing ? na : size(Fb, 2)
    st, m = _storage(Fa, Fb, storage), _sim_metric(metric)
    A = _bits(Fa)
    B = Fb === nothing ? nothing : _bits(Fb)
    pb = B === nothing ? Ptr{UInt16}(C_NULL) : pointer(B)
    ptr = Vector{Int64}(undef, na + 1)
    nnz = Ref{Int64}(0)
    call(idx, val, cap) =
        ccall((:ss_similarity_dot_csr_h16, LIB), Cint,
              (Ptr{UInt16}, Int64, Int64, Ptr{UInt16}, Int64, Int64, Int64, Cint, Cint, Float32, Cint, Ptr{Int64},
               Ptr{Int32}, Ptr{Float32}, Int64, Ptr{Int64}, Cint),
              A, na, max(d, 1), pb, nb, max(d, 1), d, st, m, Float32(alpha), weighted ? 1 : 0, ptr, idx, val, cap, nnz,
              SS_MEM_HOST)
    GC.@preserve A B begin
        check(call(Ptr{Int32}(C_NULL), Ptr{Float32}(C_NULL), 0))       # size query
        idx, val = Vector{Int32}(undef, nnz[]), Vector{Float32}(undef, nnz[])
        check(call(idx, val, nnz[]))
        # row-major CSR of (na x nb) == CSC of its (nb x na) transpose, 1-based
        return permutedims(SparseMatrixCSC(nb, na, ptr .+ 1, Vector{Int}(idx) .+ 1, val))
    end
end

"""
    graph_vectors_h16(Fq, Fs, Y::SparseMatrixCSC; storage=:bf16, metric=:cosine, alpha, weighted=true)

`SimSpreadHIP.graph_vectors` on 16-bit columns (`Fs`: `d x ns`, `Fq`: `d x nq` or `nothing`).  An ordinary
`Graph{Float32}` afterwards.
"""
function graph_vectors_h16(Fq::Union{Nothing,Half}, Fs::Half, Y::SparseMatrixCSC; storage::Symbol=:bf16,
                           metric::Symbol=:cosine, alpha::Real, weighted::Bool=true)
    d, ns = size(Fs)
    nq = Fq === nothing ? 0 : size(Fq, 2)
    Fq === nothing || size(Fq, 1) == d || throw(ArgumentError("Fq and Fs have different numbers of features"))
    size(Y, 1) == ns || throw(AssertionError("Labels and features have different number of source nodes"))
    st, m = _storage(Fs, Fq, storage), _sim_metric(metric)
    S = _bits(Fs)
    Q = Fq === nothing ? nothing : _bits(Fq)
    pq = Q === nothing ? Ptr{UInt16}(C_NULL) : pointer(Q)
    yp, yi, yv = _csr(Y, Float32)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = GC.@preserve S Q ccall((:ss_graph_create_vectors_h16, LIB), Cint,
              (Int64, Int64, Int64, Int64, Cint, Cint, Ptr{UInt16}, Int64, Ptr{UInt16}, Int64, Ptr{Int64}, Ptr{Int32},
               Ptr{Float32}, Cint, Float32, Cint, Cint, Ref{Ptr{Cvoid}}),
              nq, ns, size(Y, 2), d, st, m, pq, max(d, 1), S, max(d, 1), yp, yi, yv, 1, Float32(alpha), weighted ? 1 : 0,
              SS_MEM_HOST, h)
    check(rc)
    return Graph{Float32}(h[], nq, ns, ns, size(Y, 2))
end

"`queries_vectors_h16(g, Fq, Fs; storage, metric, alpha, weighted)`: the cross block of `graph_vectors_h16` as a query set of any `Graph{Float32}` with features named after the sources."
function queries_vectors_h16(g::Graph{Float32}, Fq::Half, Fs::Half; storage::Symbol=:bf16, metric::Symbol=:cosine,
                             alpha::Real, weighted::Bool=true)
    d, ns = size(Fs)
    size(Fq, 1) == d || throw(ArgumentError("Fq and Fs have different numbers of features"))
    nq = size(Fq, 2)
    st, m = _storage(Fs, Fq, storage), _sim_metric(metric)
    S, Q = _bits(Fs), _bits(Fq)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = GC.@preserve S Q ccall((:ss_queries_create_vectors_h16, LIB), Cint,
              (Ptr{Cvoid}, Int64, Int64, Int64, Cint, Cint, Ptr{UInt16}, Int64, Ptr{UInt16}, Int64, Float32, Cint, Cint,
               Ref{Ptr{Cvoid}}),
              g.handle, nq, ns, d, st, m, Q, max(d, 1), S, max(d, 1), Float32(alpha), weighted ? 1 : 0, SS_MEM_HOST, h)
    check(rc)
    return Queries{Float32}(h[])
end

end # module
