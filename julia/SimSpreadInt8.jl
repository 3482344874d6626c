# Exact graphs from rows stored as signed 8-bit integers: the `ccall` layer of include/simspread_hip_int8.h (the
# inner-product producer -- cosine / Tanimoto / Dice -- and its neighbour floor on Int8 rows, computed on the integer
# matrix instruction with exact Int32 sums), one function per exported symbol, on the handles of SimSpreadHIP and
# SimSpreadScreening.
#
#     include("SimSpreadHIP.jl"); include("SimSpreadScreening.jl"); include("SimSpreadInt8.jl")
#     Q, scale = SimSpreadInt8.quantize_i8(embeddings)     # d x n: ONE SAMPLE PER COLUMN
#     g = SimSpreadInt8.graph_vectors_i8(nothing, Q, sparse(y); alpha=0.8, k=3)
#     q = SimSpreadInt8.queries_vectors_i8(g, Qnew, Q; alpha=0.8, k=3)
#
# LAYOUT: as SimSpreadHalf, the Int8 matrices are `d x n`, one sample per column: the library reads rows row-major,
# element (i, k) at F[i * ld + k], which is a column-major Julia `d x n` matrix with ld = d.  g = a.b, |a|^2 and |b|^2 are
# exact integers (d <= 131071), each converted to Float32 once, so the result is bitwise defined for every input.
# `k` is the neighbour floor (0 <= k <= 64; 0: none).  The graph is a `Graph{Float32}`.
module SimSpreadInt8

using SparseArrays
using ..SimSpreadHIP: LIB, Graph, check, _csr, _sim_metric, SS_MEM_HOST
using ..SimSpreadScreening: Queries

"""
    quantize_i8(X) -> (Q::Array{Int8}, scale)

Symmetric per-tensor quantisation: `Q = round(X * 127 / max|X|)` (ties to even), `X ~ Q * scale`; an all-zero `X` gives
scale 1.  The three metrics are invariant under a common scale: quantise blocks that meet with ONE scale.
"""
function quantize_i8(X::AbstractArray{<:Real})
    all(isfinite, X) || throw(ArgumentError("quantize_i8: X holds a NaN or an infinity"))
    top = isempty(X) ? 0.0 : Float64(maximum(abs, X))
    top == 0 && return (zeros(Int8, size(X)), 1.0)
    return (Int8.(clamp.(round.(Float64.(X) .* (127.0 / top), RoundNearest), -127, 127)), top / 127.0)
end

"""
    dot_csr_i8(Fa, Fb=nothing; metric=:cosine, alpha, k=0, weighted=true)

`SimSpreadHIP.dot_csr` on Int8 columns: `Fa` is `d x na`, `Fb` `d x nb` (`nothing`: `Fa` against itself).  Returns the
`na x nb` matrix as a `SparseMatrixCSC{Float32}`.
"""
function dot_csr_i8(Fa::Matrix{Int8}, Fb::Union{Nothing,Matrix{Int8}}=nothing; metric::Symbol=:cosine, alpha::Real,
                    k::Integer=0, weighted::Bool=true)
    d, na = size(Fa)
    Fb === nothing || size(Fb, 1) == d || throw(ArgumentError("Fa and Fb have different numbers of features"))
    nb = Fb === nothing ? na : size(Fb, 2)
    m = _sim_metric(metric)
    pb = Fb === nothing ? Ptr{Int8}(C_NULL) : pointer(Fb)
    ptr = Vector{Int64}(undef, na + 1)
    nnz = Ref{Int64}(0)
    call(idx, val, cap) =
        ccall((:ss_similarity_dot_csr_i8, LIB), Cint,
              (Ptr{Int8}, Int64, Int64, Ptr{Int8}, Int64, Int64, Int64, Cint, Float32, Cint, Cint, Ptr{Int64},
               Ptr{Int32}, Ptr{Float32}, Int64, Ptr{Int64}, Cint),
              Fa, na, max(d, 1), pb, nb, max(d, 1), d, m, Float32(alpha), k, weighted ? 1 : 0, ptr, idx, val, cap, nnz,
              SS_MEM_HOST)
    GC.@preserve Fa Fb begin
        check(call(Ptr{Int32}(C_NULL), Ptr{Float32}(C_NULL), 0))       # size query
        idx, val = Vector{Int32}(undef, nnz[]), Vector{Float32}(undef, nnz[])
        check(call(idx, val, nnz[]))
        # row-major CSR of (na x nb) == CSC of its (nb x na) transpose, 1-based
        return permutedims(SparseMatrixCSC(nb, na, ptr .+ 1, Vector{Int}(idx) .+ 1, val))
    end
end

"`dot_kth_i8(Fa, Fb=nothing; metric, k)`: the k-th largest positive similarity of every column of `Fa` (1 <= k <= 64), +0 where there are fewer."
function dot_kth_i8(Fa::Matrix{Int8}, Fb::Union{Nothing,Matrix{Int8}}=nothing; metric::Symbol=:cosine, k::Integer)
    d, na = size(Fa)
    Fb === nothing || size(Fb, 1) == d || throw(ArgumentError("Fa and Fb have different numbers of features"))
    nb = Fb === nothing ? na : size(Fb, 2)
    pb = Fb === nothing ? Ptr{Int8}(C_NULL) : pointer(Fb)
    tau = Vector{Float32}(undef, na)
    rc = GC.@preserve Fa Fb ccall((:ss_similarity_dot_kth_i8, LIB), Cint,
              (Ptr{Int8}, Int64, Int64, Ptr{Int8}, Int64, Int64, Int64, Cint, Cint, Ptr{Float32}, Cint),
              Fa, na, max(d, 1), pb, nb, max(d, 1), d, _sim_metric(metric), k, tau, SS_MEM_HOST)
    check(rc)
    return tau
end

"""
    graph_vectors_i8(Fq, Fs, Y::SparseMatrixCSC; metric=:cosine, alpha, k=0, weighted=true)

`SimSpreadHIP.graph_vectors` on Int8 columns (`Fs`: `d x ns`, `Fq`: `d x nq` or `nothing`).  An ordinary
`Graph{Float32}` afterwards.
"""
function graph_vectors_i8(Fq::Union{Nothing,Matrix{Int8}}, Fs::Matrix{Int8}, Y::SparseMatrixCSC; metric::Symbol=:cosine,
                          alpha::Real, k::Integer=0, weighted::Bool=true)
    d, ns = size(Fs)
    nq = Fq === nothing ? 0 : size(Fq, 2)
    Fq === nothing || size(Fq, 1) == d || throw(ArgumentError("Fq and Fs have different numbers of features"))
    size(Y, 1) == ns || throw(AssertionError("Labels and features have different number of source nodes"))
    pq = Fq === nothing ? Ptr{Int8}(C_NULL) : pointer(Fq)
    yp, yi, yv = _csr(Y, Float32)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = GC.@preserve Fs Fq ccall((:ss_graph_create_vectors_i8, LIB), Cint,
              (Int64, Int64, Int64, Int64, Cint, Ptr{Int8}, Int64, Ptr{Int8}, Int64, Ptr{Int64}, Ptr{Int32},
               Ptr{Float32}, Cint, Float32, Cint, Cint, Cint, Ref{Ptr{Cvoid}}),
              nq, ns, size(Y, 2), d, _sim_metric(metric), pq, max(d, 1), Fs, max(d, 1), yp, yi, yv, 1, Float32(alpha), k,
              weighted ? 1 : 0, SS_MEM_HOST, h)
    check(rc)
    return Graph{Float32}(h[], nq, ns, ns, size(Y, 2))
end

"`queries_vectors_i8(g, Fq, Fs; metric, alpha, k, weighted)`: the cross block of `graph_vectors_i8` as a query set of any `Graph{Float32}` with features named after the sources."
function queries_vectors_i8(g::Graph{Float32}, Fq::Matrix{Int8}, Fs::Matrix{Int8}; metric::Symbol=:cosine, alpha::Real,
                            k::Integer=0, weighted::Bool=true)
    d, ns = size(Fs)
    size(Fq, 1) == d || throw(ArgumentError("Fq and Fs have different numbers of features"))
    nq = size(Fq, 2)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = GC.@preserve Fs Fq ccall((:ss_queries_create_vectors_i8, LIB), Cint,
              (Ptr{Cvoid}, Int64, Int64, Int64, Cint, Ptr{Int8}, Int64, Ptr{Int8}, Int64, Float32, Cint, Cint, Cint,
               Ref{Ptr{Cvoid}}),
              g.handle, nq, ns, d, _sim_metric(metric), Fq, max(d, 1), Fs, max(d, 1), Float32(alpha), k, weighted ? 1 : 0,
              SS_MEM_HOST, h)
    check(rc)
    return Queries{Float32}(h[])
end

end # module
