# SimSpreadHIP.jl -- raw `ccall` layer over libsimspread_hip.so (C ABI: include/simspread_hip.h), MI355X / gfx950.
#
# One Julia function per exported `ss_*` symbol, nothing else: argument conversion, the ccall, the error check.  The
# reference-compatible method table (featurize / construct / predict / clean! ... of src/SimSpread.jl:21-56) lives in
# SimSpreadDevice.jl, which is written on top of this module.
#
# NOT executed in this repository: Julia is installed neither in the build container nor on the GPU box.  What keeps the
# file honest is tests/test_julia_binding.py, which parses every ccall below and compares its name, return type and
# argument tuple with the C header and with the ctypes table of the Python mirror (simspread.jl_amd/_lib.py) that the
# parity tests drive.  No CUDA.jl, no dual backend.
module SimSpreadHIP

using SparseArrays

const LIB = get(ENV, "SIMSPREAD_HIP_LIB", joinpath(@__DIR__, "..", "simspread.jl_amd", "libsimspread_hip.so"))

const SS_MEM_HOST = Cint(0)
const SS_MEM_DEVICE = Cint(1)
const SS_ROWS_QUERY = Cint(0)
const SS_ROWS_SOURCE = Cint(1)
const SS_LAYOUT_ROWMAJOR = Cint(0)
const SS_LAYOUT_COLMAJOR = Cint(1)

struct SimSpreadHIPError <: Exception
    code::Cint
    msg::String
end

# ------------------------------------------------------------------------------------------------ runtime
version() = ccall((:ss_version, LIB), Cint, ())
last_error() = unsafe_string(ccall((:ss_last_error, LIB), Cstring, ()))
source_hash() = unsafe_string(ccall((:ss_source_hash, LIB), Cstring, ()))
device_count() = ccall((:ss_device_count, LIB), Cint, ())

function check(rc::Cint)
    rc == 0 && return nothing
    msg = last_error()
    # -1 (SS_EINVAL) is what the reference's @assert would have caught on the Julia side
    rc == -1 ? throw(AssertionError(msg)) : throw(SimSpreadHIPError(rc, msg))
end

"Bind this process to one GPU (replaces the reference's `GPU::Bool` switch, src/core.jl:402,404,446,448)."
init(device::Integer=0) = check(ccall((:ss_init, LIB), Cint, (Cint,), device))
shutdown() = check(ccall((:ss_shutdown, LIB), Cint, ()))
set_stream(stream::Ptr{Cvoid}) = check(ccall((:ss_set_stream, LIB), Cint, (Ptr{Cvoid},), stream))
reset_stream() = check(ccall((:ss_reset_stream, LIB), Cint, ()))
synchronize() = check(ccall((:ss_synchronize, LIB), Cint, ()))
timing_hold(enable::Bool) = check(ccall((:ss_timing_hold, LIB), Cint, (Cint,), enable ? 1 : 0))

"Stage timings (ms) of the last predict / spmm call of this task's thread: total, transfer, spmm, epilogue, h2d, d2h, #spmm, #transfer."
function timing_last()
    ms = zeros(Float64, 8)
    check(ccall((:ss_timing_last, LIB), Cint, (Ptr{Float64}, Cint), ms, 8))
    return (total_ms=ms[1], transfer_ms=ms[2], spmm_ms=ms[3], epilogue_ms=ms[4], h2d_ms=ms[5], d2h_ms=ms[6],
            spmm_launches=Int(ms[7]), transfer_launches=Int(ms[8]))
end

"Kernel tags the last predict / spmm call went through (e.g. \"transfer_dense_bf16_ring\", \"spmm_sell\")."
function path_last()
    buf = zeros(UInt8, 512)
    check(ccall((:ss_path_last, LIB), Cint, (Ptr{UInt8}, Cint), buf, 512))
    return split(unsafe_string(pointer(buf)), ","; keepempty=false)
end

# ------------------------------------------------------------------------------------------------ final score gather (RCCL)
"128 bytes created by rank 0; hand them to the other processes (MPI.bcast, Distributed.jl, ...)."
function comm_unique_id()
    id = zeros(UInt8, 128)
    check(ccall((:ss_comm_unique_id, LIB), Cint, (Ptr{UInt8},), id))
    return id
end
comm_init(id::Vector{UInt8}, rank::Integer, nranks::Integer) =
    check(ccall((:ss_comm_init, LIB), Cint, (Ptr{UInt8}, Cint, Cint), id, rank, nranks))
comm_destroy() = check(ccall((:ss_comm_destroy, LIB), Cint, ()))
function comm_info()
    rank, nranks = Ref{Cint}(0), Ref{Cint}(0)
    check(ccall((:ss_comm_info, LIB), Cint, (Ref{Cint}, Ref{Cint}), rank, nranks))
    return Int(rank[]), Int(nranks[])
end

"""
    gather_rows(local::Ptr, ncols, counts, full::Ptr; root=-1, T=Float32)

Direct exchange of finished score rows between the ranks (device pointers, row-major blocks): rank r contributes
`counts[r+1]` rows; `root = -1`: every rank receives the full matrix.
"""
function gather_rows(local_::Ptr{Cvoid}, ncols::Integer, counts::Vector{Int64}, full::Ptr{Cvoid}; root::Integer=-1, T::Type=Float32)
    rc = if T === Float32
        ccall((:ss_gather_rows_f32, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Cvoid}, Cint), local_, ncols, counts, full, root)
    else
        ccall((:ss_gather_rows_f64, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Cvoid}, Cint), local_, ncols, counts, full, root)
    end
    check(rc)
end

# ------------------------------------------------------------------------------------------------ cutoff / k / spread
"cutoff(X, alpha, weighted) on the device (src/core.jl:37-43,55-60): x >= alpha ? (weighted ? x : 1) : 0."
function cutoff(X::Matrix{Float64}, alpha::Float64, weighted::Bool=false)
    out = similar(X)
    ld = max(size(X, 1), 1)
    check(ccall((:ss_cutoff_f64, LIB), Cint,
                (Ptr{Float64}, Int64, Int64, Int64, Float64, Cint, Ptr{Float64}, Int64, Cint),
                X, size(X, 1), size(X, 2), ld, alpha, weighted ? 1 : 0, out, ld, SS_MEM_HOST))
    return out
end
function cutoff(X::Matrix{Float32}, alpha::Float32, weighted::Bool=false)
    out = similar(X)
    ld = max(size(X, 1), 1)
    check(ccall((:ss_cutoff_f32, LIB), Cint,
                (Ptr{Float32}, Int64, Int64, Int64, Float32, Cint, Ptr{Float32}, Int64, Cint),
                X, size(X, 1), size(X, 2), ld, alpha, weighted ? 1 : 0, out, ld, SS_MEM_HOST))
    return out
end

"k(G): number of non-zeros of every row (src/graphs.jl:9-11) -> Vector{Int64}."
function row_degree(G::Matrix{Float64})
    deg = Vector{Int64}(undef, size(G, 1))
    check(ccall((:ss_row_degree_f64, LIB), Cint, (Ptr{Float64}, Int64, Int64, Int64, Ptr{Int64}, Cint),
                G, size(G, 1), size(G, 2), max(size(G, 1), 1), deg, SS_MEM_HOST))
    return deg
end
function row_degree(G::Matrix{Float32})
    deg = Vector{Int64}(undef, size(G, 1))
    check(ccall((:ss_row_degree_f32, LIB), Cint, (Ptr{Float32}, Int64, Int64, Int64, Ptr{Int64}, Cint),
                G, size(G, 1), size(G, 2), max(size(G, 1), 1), deg, SS_MEM_HOST))
    return deg
end

"spread(G): W[i,j] = G[i,j] / k(i), rows of degree 0 give 0 (src/core.jl:365-371)."
function spread(G::Matrix{Float64})
    W = similar(G)
    ld = max(size(G, 1), 1)
    check(ccall((:ss_spread_f64, LIB), Cint, (Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Int64, Cint),
                G, size(G, 1), size(G, 2), ld, W, ld, SS_MEM_HOST))
    return W
end
function spread(G::Matrix{Float32})
    W = similar(G)
    ld = max(size(G, 1), 1)
    check(ccall((:ss_spread_f32, LIB), Cint, (Ptr{Float32}, Int64, Int64, Int64, Ptr{Float32}, Int64, Cint),
                G, size(G, 1), size(G, 2), ld, W, ld, SS_MEM_HOST))
    return W
end

"`1 .- pairwise(Jaccard(), X, dims=1)` (docs/src/tutorial/fishers-flowers.jl:66) on the device."
function jaccard_similarity(X::Matrix{Float64})
    n, d = size(X)
    S = Matrix{Float64}(undef, n, n)
    check(ccall((:ss_similarity_jaccard_f64, LIB), Cint, (Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Int64, Cint),
                X, n, d, max(n, 1), S, max(n, 1), SS_MEM_HOST))
    return S
end
function jaccard_similarity(X::Matrix{Float32})
    n, d = size(X)
    S = Matrix{Float32}(undef, n, n)
    check(ccall((:ss_similarity_jaccard_f32, LIB), Cint, (Ptr{Float32}, Int64, Int64, Int64, Ptr{Float32}, Int64, Cint),
                X, n, d, max(n, 1), S, max(n, 1), SS_MEM_HOST))
    return S
end

"""
    tanimoto_csr(Fa::Matrix{UInt64}, Fb=nothing; alpha, weighted=true, T=Float32)

`featurize(1 .- pairwise(Jaccard(), F, dims=1), alpha, weighted)` for binary fingerprints, produced as CSR on the device
without the dense similarity.  `Fa` is `nwords x na` with column `i` = `fps[i].chunks` of a `BitVector` (bits past the
fingerprint length zero, as `BitVector` keeps them); `Fb === nothing`: the symmetric block of `Fa` against itself.
Returns the `na x nb` matrix as a `SparseMatrixCSC` (the library's row-major CSR read as the CSC of the transpose).
"""
function tanimoto_csr(Fa::Matrix{UInt64}, Fb::Union{Nothing,Matrix{UInt64}}=nothing; alpha::Real, weighted::Bool=true,
                      T::Type=Float32)
    nwords, na = size(Fa)
    nb = Fb === nothing ? na : size(Fb, 2)
    Fb === nothing || size(Fb, 1) == nwords || throw(ArgumentError("Fa and Fb have different fingerprint widths"))
    pb = Fb === nothing ? Ptr{UInt64}(C_NULL) : pointer(Fb)
    ptr = Vector{Int64}(undef, na + 1)
    nnz = Ref{Int64}(0)
    call(idx, val, cap) = if T === Float32
        ccall((:ss_similarity_tanimoto_csr_f32, LIB), Cint,
              (Ptr{UInt64}, Int64, Ptr{UInt64}, Int64, Int64, Float32, Cint, Ptr{Int64}, Ptr{Int32}, Ptr{Float32},
               Int64, Ptr{Int64}, Cint),
              Fa, na, pb, nb, nwords, Float32(alpha), weighted ? 1 : 0, ptr, idx, val, cap, nnz, SS_MEM_HOST)
    else
        ccall((:ss_similarity_tanimoto_csr_f64, LIB), Cint,
              (Ptr{UInt64}, Int64, Ptr{UInt64}, Int64, Int64, Float64, Cint, Ptr{Int64}, Ptr{Int32}, Ptr{Float64},
               Int64, Ptr{Int64}, Cint),
              Fa, na, pb, nb, nwords, Float64(alpha), weighted ? 1 : 0, ptr, idx, val, cap, nnz, SS_MEM_HOST)
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
    jaccard_csr(Fa::Matrix{T}, Fb=nothing; alpha, weighted=true) where T<:Union{Float32,Float64}

`featurize(1 .- pairwise(Jaccard(), X, dims=1), alpha, weighted)` for real-valued feature rows
(docs/src/tutorial/fishers-flowers.jl:66,95-96), produced as CSR on the device without the dense similarity: the
weighted Jaccard Σmin / Σmax of every pair of rows, bitwise what `jaccard_similarity` followed by the cutoff gives.
`Fa` is `na x d` with one sample per row (a plain Julia `Matrix`, column-major); `Fb === nothing`: the symmetric block of
`Fa` against itself.  Returns the `na x nb` matrix as a `SparseMatrixCSC`.
"""
function jaccard_csr(Fa::Matrix{T}, Fb::Union{Nothing,Matrix{T}}=nothing; alpha::Real,
                     weighted::Bool=true) where {T<:Union{Float32,Float64}}
    na, d = size(Fa)
    nb = Fb === nothing ? na : size(Fb, 1)
    Fb === nothing || size(Fb, 2) == d || throw(ArgumentError("Fa and Fb have different numbers of features"))
    pb = Fb === nothing ? Ptr{T}(C_NULL) : pointer(Fb)
    ptr = Vector{Int64}(undef, na + 1)
    nnz = Ref{Int64}(0)
    call(idx, val, cap) = if T === Float32
        ccall((:ss_similarity_jaccard_csr_f32, LIB), Cint,
              (Ptr{Float32}, Int64, Int64, Ptr{Float32}, Int64, Int64, Int64, Float32, Cint, Ptr{Int64}, Ptr{Int32},
               Ptr{Float32}, Int64, Ptr{Int64}, Cint),
              Fa, na, max(na, 1), pb, nb, max(nb, 1), d, Float32(alpha), weighted ? 1 : 0, ptr, idx, val, cap, nnz,
              SS_MEM_HOST)
    else
        ccall((:ss_similarity_jaccard_csr_f64, LIB), Cint,
              (Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Int64, Int64, Float64, Cint, Ptr{Int64}, Ptr{Int32},
               Ptr{Float64}, Int64, Ptr{Int64}, Cint),
              Fa, na, max(na, 1), pb, nb, max(nb, 1), d, Float64(alpha), weighted ? 1 : 0, ptr, idx, val, cap, nnz,
              SS_MEM_HOST)
    end
    GC.@preserve Fa Fb begin
        check(call(Ptr{Int32}(C_NULL), Ptr{T}(C_NULL), 0))             # size query
        idx, val = Vector{Int32}(undef, nnz[]), Vector{T}(undef, nnz[])
        check(call(idx, val, nnz[]))
    end
    return permutedims(SparseMatrixCSC(nb, na, ptr .+ 1, Vector{Int}(idx) .+ 1, val))
end

const SIM_METRICS = Dict(:cosine => 0, :tanimoto => 1, :dice => 2)   # SS_SIM_* of include/simspread_hip.h
_sim_metric(m::Symbol) = haskey(SIM_METRICS, m) ? Cint(SIM_METRICS[m]) :
    throw(ArgumentError("metric must be :cosine, :tanimoto or :dice, got $(repr(m))"))

"""
    dot_csr(Fa::Matrix{T}, Fb=nothing; metric=:cosine, alpha, weighted=true) where T<:Union{Float32,Float64}

`featurize(S, alpha, weighted)` with `S` an inner-product similarity of real-valued rows (embeddings, continuous
descriptors), produced as CSR on the device without the dense similarity, the Gram blocks on the matrix cores in full `T`
precision.  With `g = a⋅b`: `:cosine` `g / (|a| |b|)`, `:tanimoto` `g / (|a|² + |b|² - g)`, `:dice` `2g / (|a|² + |b|²)`;
two all-zero rows have `s = 1`.  `Fa` is `na x d` with one sample per row; `Fb === nothing`: the symmetric block of `Fa`
against itself (diagonal exactly 1).  Returns the `na x nb` matrix as a `SparseMatrixCSC`.
"""
function dot_csr(Fa::Matrix{T}, Fb::Union{Nothing,Matrix{T}}=nothing; metric::Symbol=:cosine, alpha::Real,
                 weighted::Bool=true) where {T<:Union{Float32,Float64}}
    na, d = size(Fa)
    nb = Fb === nothing ? na : size(Fb, 1)
    Fb === nothing || size(Fb, 2) == d || throw(ArgumentError("Fa and Fb have different numbers of features"))
    pb = Fb === nothing ? Ptr{T}(C_NULL) : pointer(Fb)
    m = _sim_metric(metric)
    ptr = Vector{Int64}(undef, na + 1)
    nnz = Ref{Int64}(0)
    call(idx, val, cap) = if T === Float32
        ccall((:ss_similarity_dot_csr_f32, LIB), Cint,
              (Ptr{Float32}, Int64, Int64, Ptr{Float32}, Int64, Int64, Int64, Cint, Float32, Cint, Ptr{Int64}, Ptr{Int32},
               Ptr{Float32}, Int64, Ptr{Int64}, Cint),
              Fa, na, max(na, 1), pb, nb, max(nb, 1), d, m, Float32(alpha), weighted ? 1 : 0, ptr, idx, val, cap, nnz,
              SS_MEM_HOST)
    else
        ccall((:ss_similarity_dot_csr_f64, LIB), Cint,
              (Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Int64, Int64, Cint, Float64, Cint, Ptr{Int64}, Ptr{Int32},
               Ptr{Float64}, Int64, Ptr{Int64}, Cint),
              Fa, na, max(na, 1), pb, nb, max(nb, 1), d, m, Float64(alpha), weighted ? 1 : 0, ptr, idx, val, cap, nnz,
              SS_MEM_HOST)
    end
    GC.@preserve Fa Fb begin
        check(call(Ptr{Int32}(C_NULL), Ptr{T}(C_NULL), 0))             # size query
        idx, val = Vector{Int32}(undef, nnz[]), Vector{T}(undef, nnz[])
        check(call(idx, val, nnz[]))
    end
    return permutedims(SparseMatrixCSC(nb, na, ptr .+ 1, Vector{Int}(idx) .+ 1, val))
end

"""
    cutoff_csr(X::SparseMatrixCSC{T}, alpha; weighted=false) where T<:Union{Float32,Float64}

`featurize(X, alpha, weighted)` (src/core.jl:106-112) on a sparse matrix, on the device: a stored `v` stays iff
`v >= alpha`, as `v` when `weighted` and `1` otherwise.  `alpha` must be positive (an unstored zero would pass an
unweighted cutoff at `alpha <= 0`).  Returns a `SparseMatrixCSC` of the same size.
"""
function cutoff_csr(X::SparseMatrixCSC{T}, alpha::Real; weighted::Bool=false) where {T<:Union{Float32,Float64}}
    rows, cols = size(X)
    ip, ii, iv = _csr(X, T)
    ptr = Vector{Int64}(undef, rows + 1)
    nnz = Ref{Int64}(0)
    call(idx, val, cap) = if T === Float32
        ccall((:ss_cutoff_csr_f32, LIB), Cint,
              (Int64, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Float32}, Cint, Float32, Cint, Ptr{Int64}, Ptr{Int32},
               Ptr{Float32}, Int64, Ptr{Int64}, Cint),
              rows, cols, ip, ii, iv, 1, Float32(alpha), weighted ? 1 : 0, ptr, idx, val, cap, nnz, SS_MEM_HOST)
    else
        ccall((:ss_cutoff_csr_f64, LIB), Cint,
              (Int64, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Float64}, Cint, Float64, Cint, Ptr{Int64}, Ptr{Int32},
               Ptr{Float64}, Int64, Ptr{Int64}, Cint),
              rows, cols, ip, ii, iv, 1, Float64(alpha), weighted ? 1 : 0, ptr, idx, val, cap, nnz, SS_MEM_HOST)
    end
    check(call(Ptr{Int32}(C_NULL), Ptr{T}(C_NULL), 0))             # size query
    idx, val = Vector{Int32}(undef, nnz[]), Vector{T}(undef, nnz[])
    check(call(idx, val, nnz[]))
    # the result is 0-based row-major CSR of (rows x cols) == CSC of its transpose
    return permutedims(SparseMatrixCSC(cols, rows, ptr .+ 1, Vector{Int}(idx) .+ 1, val))
end

# ------------------------------------------------------------------------------------------------ graph handles
mutable struct Graph{T<:Union{Float32,Float64}}
    handle::Ptr{Cvoid}
    nq::Int
    ns::Int
    nf::Int
    nt::Int
    function Graph{T}(h, nq, ns, nf, nt) where {T}
        g = new{T}(h, nq, ns, nf, nt)
        finalizer(destroy!, g)
        return g
    end
end

function destroy!(g::Graph)
    if g.handle != C_NULL
        ccall((:ss_graph_destroy, LIB), Cint, (Ptr{Cvoid},), g.handle)
        g.handle = C_NULL
    end
    return nothing
end

# A SparseMatrixCSC is the 1-based CSR of its transpose: hand over the transposes with index_base = 1.
_csr(M::SparseMatrixCSC, ::Type{T}) where {T} = (t = sparse(M'); (Vector{Int64}(t.colptr), Vector{Int32}(t.rowval), Vector{T}(t.nzval)))

"""
    graph(Xq, Xs, Y; alpha=nothing, weighted=true, T=Float64)

Device-resident replacement of `construct` (src/core.jl:148-201,217-276,308-337): dense column-major blocks
`Xq = A[queries, features]`, `Xs = A[sources, features]`, `Y = A[sources, targets]`.  With `alpha` the featurize
cutoff (src/core.jl:106-112) is fused into the on-device CSR assembly.  `Xq === nothing`: the 3-layer graph of
`construct(y, X)`.
"""
function graph(Xq::Union{Nothing,AbstractMatrix}, Xs::AbstractMatrix, Y::AbstractMatrix;
               alpha=nothing, weighted::Bool=true, T::Type=Float64)
    size(Y, 1) == size(Xs, 1) || throw(AssertionError("Labels and features have different number of source nodes"))
    Xq === nothing || size(Xq, 2) == size(Xs, 2) ||
        throw(AssertionError("Number of features between test and training sets doesn't match"))
    q = Xq === nothing ? Matrix{T}(undef, 0, size(Xs, 2)) : Matrix{T}(Xq)
    s, y = Matrix{T}(Xs), Matrix{T}(Y)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    nq, ns, nf, nt = size(q, 1), size(s, 1), size(s, 2), size(y, 2)
    cut, a = alpha === nothing ? 0 : 1, alpha === nothing ? zero(T) : T(alpha)
    rc = if T === Float32
        ccall((:ss_graph_create_dense_f32, LIB), Cint,
              (Int64, Int64, Int64, Int64, Ptr{Float32}, Int64, Ptr{Float32}, Int64, Ptr{Float32}, Int64,
               Cint, Float32, Cint, Cint, Ref{Ptr{Cvoid}}),
              nq, ns, nf, nt, q, max(nq, 1), s, max(ns, 1), y, max(ns, 1), cut, a, weighted ? 1 : 0, SS_MEM_HOST, h)
    else
        ccall((:ss_graph_create_dense_f64, LIB), Cint,
              (Int64, Int64, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64,
               Cint, Float64, Cint, Cint, Ref{Ptr{Cvoid}}),
              nq, ns, nf, nt, q, max(nq, 1), s, max(ns, 1), y, max(ns, 1), cut, a, weighted ? 1 : 0, SS_MEM_HOST, h)
    end
    check(rc)
    return Graph{T}(h[], nq, ns, nf, nt)
end

"Sparse blocks (`SparseMatrixCSC`)."
function graph(Xq::SparseMatrixCSC, Xs::SparseMatrixCSC, Y::SparseMatrixCSC; T::Type=Float64)
    (qp, qi, qv), (sp, si, sv), (yp, yi, yv) = _csr(Xq, T), _csr(Xs, T), _csr(Y, T)
    nq, ns, nf, nt = size(Xq, 1), size(Xs, 1), size(Xs, 2), size(Y, 2)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = if T === Float32
        ccall((:ss_graph_create_csr_f32, LIB), Cint,
              (Int64, Int64, Int64, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Float32}, Ptr{Int64}, Ptr{Int32}, Ptr{Float32},
               Ptr{Int64}, Ptr{Int32}, Ptr{Float32}, Cint, Cint, Ref{Ptr{Cvoid}}),
              nq, ns, nf, nt, qp, qi, qv, sp, si, sv, yp, yi, yv, 1, SS_MEM_HOST, h)
    else
        ccall((:ss_graph_create_csr_f64, LIB), Cint,
              (Int64, Int64, Int64, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Float64}, Ptr{Int64}, Ptr{Int32}, Ptr{Float64},
               Ptr{Int64}, Ptr{Int32}, Ptr{Float64}, Cint, Cint, Ref{Ptr{Cvoid}}),
              nq, ns, nf, nt, qp, qi, qv, sp, si, sv, yp, yi, yv, 1, SS_MEM_HOST, h)
    end
    check(rc)
    return Graph{T}(h[], nq, ns, nf, nt)
end

"""
    graph_similarity(Sq, Ss, Y::SparseMatrixCSC; alpha, weighted=true)

Dense-similarity regime (thresholded similarity too full for CSR): raw similarities `Sq` (nq x ns, or `nothing`) and
`Ss` (ns x ns) stay dense on the device, featurize's cutoff is applied inside the matrix-core product
(`T=Float32`: bf16 planes, `T=Float64`: the fp64 matrix instruction).
"""
function graph_similarity(Sq::Union{Nothing,AbstractMatrix}, Ss::AbstractMatrix, Y::SparseMatrixCSC;
                          alpha::Real, weighted::Bool=true, T::Type=Float32)
    ns = size(Ss, 1)
    q = Sq === nothing ? Matrix{T}(undef, 0, ns) : Matrix{T}(Sq)
    s = Matrix{T}(Ss)
    yp, yi, yv = _csr(Y, T)
    nq, nt = size(q, 1), size(Y, 2)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = if T === Float32
        ccall((:ss_graph_create_similarity_f32, LIB), Cint,
              (Int64, Int64, Int64, Ptr{Float32}, Int64, Ptr{Float32}, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Float32},
               Cint, Float32, Cint, Cint, Ref{Ptr{Cvoid}}),
              nq, ns, nt, q, max(nq, 1), s, max(ns, 1), yp, yi, yv, 1, Float32(alpha), weighted ? 1 : 0, SS_MEM_HOST, h)
    else
        ccall((:ss_graph_create_similarity_f64, LIB), Cint,
              (Int64, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Float64},
               Cint, Float64, Cint, Cint, Ref{Ptr{Cvoid}}),
              nq, ns, nt, q, max(nq, 1), s, max(ns, 1), yp, yi, yv, 1, Float64(alpha), weighted ? 1 : 0, SS_MEM_HOST, h)
    end
    check(rc)
    return Graph{T}(h[], nq, ns, ns, nt)
end

"""
    graph_fingerprint(Fq, Fs::Matrix{UInt64}, Y::SparseMatrixCSC; alpha, weighted=true, T=Float32)

`construct(y, X)` with `X = featurize(Tanimoto(F), alpha, weighted)` for binary fingerprints (`nwords x n` matrices,
column `i` = `fps[i].chunks`): the thresholded similarity blocks are produced as CSR on the device.  `Fq === nothing`:
the 3-layer graph of `construct(y, X)` (leave-one-out / k-fold).
"""
function graph_fingerprint(Fq::Union{Nothing,Matrix{UInt64}}, Fs::Matrix{UInt64}, Y::SparseMatrixCSC;
                           alpha::Real, weighted::Bool=true, T::Type=Float32)
    nwords, ns = size(Fs)
    nq = Fq === nothing ? 0 : size(Fq, 2)
    Fq === nothing || size(Fq, 1) == nwords || throw(ArgumentError("Fq and Fs have different fingerprint widths"))
    size(Y, 1) == ns || throw(AssertionError("Labels and features have different number of source nodes"))
    pq = Fq === nothing ? Ptr{UInt64}(C_NULL) : pointer(Fq)
    yp, yi, yv = _csr(Y, T)
    nt = size(Y, 2)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = GC.@preserve Fq if T === Float32
        ccall((:ss_graph_create_fingerprint_f32, LIB), Cint,
              (Int64, Int64, Int64, Int64, Ptr{UInt64}, Ptr{UInt64}, Ptr{Int64}, Ptr{Int32}, Ptr{Float32},
               Cint, Float32, Cint, Cint, Ref{Ptr{Cvoid}}),
              nq, ns, nt, nwords, pq, Fs, yp, yi, yv, 1, Float32(alpha), weighted ? 1 : 0, SS_MEM_HOST, h)
    else
        ccall((:ss_graph_create_fingerprint_f64, LIB), Cint,
              (Int64, Int64, Int64, Int64, Ptr{UInt64}, Ptr{UInt64}, Ptr{Int64}, Ptr{Int32}, Ptr{Float64},
               Cint, Float64, Cint, Cint, Ref{Ptr{Cvoid}}),
              nq, ns, nt, nwords, pq, Fs, yp, yi, yv, 1, Float64(alpha), weighted ? 1 : 0, SS_MEM_HOST, h)
    end
    check(rc)
    return Graph{T}(h[], nq, ns, ns, nt)
end

"""
    graph_features(Fq, Fs::Matrix{T}, Y::SparseMatrixCSC; alpha, weighted=true) where T<:Union{Float32,Float64}

`construct(y, X)` with `X = featurize(1 .- pairwise(Jaccard(), F, dims=1), alpha, weighted)` for real-valued feature
rows (`n x d` matrices, one sample per row; docs/src/tutorial/fishers-flowers.jl:66,95-96): the thresholded weighted
Jaccard blocks are produced as CSR on the device.  `Fq === nothing`: the 3-layer graph of `construct(y, X)`
(leave-one-out / k-fold).
"""
function graph_features(Fq::Union{Nothing,Matrix{T}}, Fs::Matrix{T}, Y::SparseMatrixCSC; alpha::Real,
                        weighted::Bool=true) where {T<:Union{Float32,Float64}}
    ns, d = size(Fs)
    nq = Fq === nothing ? 0 : size(Fq, 1)
    Fq === nothing || size(Fq, 2) == d || throw(ArgumentError("Fq and Fs have different numbers of features"))
    size(Y, 1) == ns || throw(AssertionError("Labels and features have different number of source nodes"))
    pq = Fq === nothing ? Ptr{T}(C_NULL) : pointer(Fq)
    yp, yi, yv = _csr(Y, T)
    nt = size(Y, 2)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = GC.@preserve Fq if T === Float32
        ccall((:ss_graph_create_features_f32, LIB), Cint,
              (Int64, Int64, Int64, Int64, Ptr{Float32}, Int64, Ptr{Float32}, Int64, Ptr{Int64}, Ptr{Int32},
               Ptr{Float32}, Cint, Float32, Cint, Cint, Ref{Ptr{Cvoid}}),
              nq, ns, nt, d, pq, max(nq, 1), Fs, max(ns, 1), yp, yi, yv, 1, Float32(alpha), weighted ? 1 : 0,
              SS_MEM_HOST, h)
    else
        ccall((:ss_graph_create_features_f64, LIB), Cint,
              (Int64, Int64, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Int32},
               Ptr{Float64}, Cint, Float64, Cint, Cint, Ref{Ptr{Cvoid}}),
              nq, ns, nt, d, pq, max(nq, 1), Fs, max(ns, 1), yp, yi, yv, 1, Float64(alpha), weighted ? 1 : 0,
              SS_MEM_HOST, h)
    end
    check(rc)
    return Graph{T}(h[], nq, ns, ns, nt)
end

"""
    graph_vectors(Fq, Fs::Matrix{T}, Y::SparseMatrixCSC; metric=:cosine, alpha, weighted=true)

`construct(y, X)` with `X = featurize(S(F), alpha, weighted)`, `S` the inner-product similarity `metric` of `dot_csr`
between real-valued rows (`n x d` matrices, one sample per row): the thresholded blocks are produced as CSR on the
device.  `Fq === nothing`: the 3-layer graph of `construct(y, X)` (leave-one-out / k-fold).
"""
function graph_vectors(Fq::Union{Nothing,Matrix{T}}, Fs::Matrix{T}, Y::SparseMatrixCSC; metric::Symbol=:cosine,
                       alpha::Real, weighted::Bool=true) where {T<:Union{Float32,Float64}}
    ns, d = size(Fs)
    nq = Fq === nothing ? 0 : size(Fq, 1)
    Fq === nothing || size(Fq, 2) == d || throw(ArgumentError("Fq and Fs have different numbers of features"))
    size(Y, 1) == ns || throw(AssertionError("Labels and features have different number of source nodes"))
    pq = Fq === nothing ? Ptr{T}(C_NULL) : pointer(Fq)
    m = _sim_metric(metric)
    yp, yi, yv = _csr(Y, T)
    nt = size(Y, 2)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = GC.@preserve Fq if T === Float32
        ccall((:ss_graph_create_vectors_f32, LIB), Cint,
              (Int64, Int64, Int64, Int64, Cint, Ptr{Float32}, Int64, Ptr{Float32}, Int64, Ptr{Int64}, Ptr{Int32},
               Ptr{Float32}, Cint, Float32, Cint, Cint, Ref{Ptr{Cvoid}}),
              nq, ns, nt, d, m, pq, max(nq, 1), Fs, max(ns, 1), yp, yi, yv, 1, Float32(alpha), weighted ? 1 : 0,
              SS_MEM_HOST, h)
    else
        ccall((:ss_graph_create_vectors_f64, LIB), Cint,
              (Int64, Int64, Int64, Int64, Cint, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Int32},
               Ptr{Float64}, Cint, Float64, Cint, Cint, Ref{Ptr{Cvoid}}),
              nq, ns, nt, d, m, pq, max(nq, 1), Fs, max(ns, 1), yp, yi, yv, 1, Float64(alpha), weighted ? 1 : 0,
              SS_MEM_HOST, h)
    end
    check(rc)
    return Graph{T}(h[], nq, ns, ns, nt)
end

"""
    graph_general(L, B, Wt; T=Float64)

Any caller-built adjacency pair (src/core.jl:402-425 accepts arbitrary named `A`, `B`): `L = A[rows of y, :]` (nr x n),
`B` (n x n), `Wt = B[:, cols of y]'` (nc x n), all `SparseMatrixCSC`.  `predict(g, :query)` then returns the
nr x nc block of `A * spread(B)^2`.
"""
function graph_general(L::SparseMatrixCSC, B::SparseMatrixCSC, Wt::SparseMatrixCSC; T::Type=Float64)
    n, nr, nc = size(B, 1), size(L, 1), size(Wt, 1)
    (lp, li, lv), (bp, bi, bv), (wp, wi, wv) = _csr(L, T), _csr(B, T), _csr(Wt, T)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = if T === Float32
        ccall((:ss_graph_create_general_f32, LIB), Cint,
              (Int64, Int64, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Float32}, Ptr{Int64}, Ptr{Int32}, Ptr{Float32},
               Ptr{Int64}, Ptr{Int32}, Ptr{Float32}, Cint, Cint, Ref{Ptr{Cvoid}}),
              n, nr, nc, lp, li, lv, bp, bi, bv, wp, wi, wv, 1, SS_MEM_HOST, h)
    else
        ccall((:ss_graph_create_general_f64, LIB), Cint,
              (Int64, Int64, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Float64}, Ptr{Int64}, Ptr{Int32}, Ptr{Float64},
               Ptr{Int64}, Ptr{Int32}, Ptr{Float64}, Cint, Cint, Ref{Ptr{Cvoid}}),
              n, nr, nc, lp, li, lv, bp, bi, bv, wp, wi, wv, 1, SS_MEM_HOST, h)
    end
    check(rc)
    return Graph{T}(h[], nr, n, n, nc)
end

"""
    recut(g::Graph, alpha; weighted=true)

Cutoff sweeps: a new, independent graph equal to `g` with `Xq`, `Xs` replaced by `featurize(X, alpha, weighted)` of the
blocks resident on the device (two streaming passes; no all-pairs producer, no sort).  For a parent built weighted at a
cutoff `a0 > 0` and `alpha >= a0` the child is bitwise the graph the parent's constructor builds at `(alpha, weighted)`.
`g` stays usable and may be destroyed first.  Dense-similarity graphs use `set_cutoff!`.
"""
function recut(g::Graph{T}, alpha::Real; weighted::Bool=true) where {T}
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = if T === Float32
        ccall((:ss_graph_recut_f32, LIB), Cint, (Ptr{Cvoid}, Float32, Cint, Ref{Ptr{Cvoid}}),
              g.handle, Float32(alpha), weighted ? 1 : 0, h)
    else
        ccall((:ss_graph_recut_f64, LIB), Cint, (Ptr{Cvoid}, Float64, Cint, Ref{Ptr{Cvoid}}),
              g.handle, Float64(alpha), weighted ? 1 : 0, h)
    end
    check(rc)
    return Graph{T}(h[], g.nq, g.ns, g.nf, g.nt)
end

"""
    set_cutoff!(g::Graph, alpha; weighted=true)

Dense-similarity graphs (`graph_similarity`): move the cutoff in place.  The raw similarities stay resident; afterwards
`g` behaves bitwise like a fresh `graph_similarity` at `(alpha, weighted)`.  `alpha` may go down as well as up.
"""
function set_cutoff!(g::Graph{T}, alpha::Real; weighted::Bool=true) where {T}
    rc = if T === Float32
        ccall((:ss_graph_set_cutoff_f32, LIB), Cint, (Ptr{Cvoid}, Float32, Cint), g.handle, Float32(alpha), weighted ? 1 : 0)
    else
        ccall((:ss_graph_set_cutoff_f64, LIB), Cint, (Ptr{Cvoid}, Float64, Cint), g.handle, Float64(alpha), weighted ? 1 : 0)
    end
    check(rc)
    return g
end

"sizes after dropping stored zeros: (nq, ns, nf, nt, nnz(Xq), nnz(Xs), nnz(Ys))."
function graph_info(g::Graph)
    sizes = Vector{Int64}(undef, 7)
    check(ccall((:ss_graph_info, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}), g.handle, sizes))
    return sizes
end

"Count degrees of the query-free graph B: (kf, ks, kt)."
function graph_degrees(g::Graph)
    kf, ks, kt = Vector{Int64}(undef, g.nf), Vector{Int64}(undef, g.ns), Vector{Int64}(undef, g.nt)
    check(ccall((:ss_graph_degrees, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}), g.handle, kf, ks, kt))
    return kf, ks, kt
end

# ------------------------------------------------------------------------------------------------ predict
"""
    predict(g, rows=:query; clean=false, range=nothing) -> Matrix{Float64}

The `rows x targets` block of `A * spread(B)^2` (src/core.jl:402-425,446-466), column-major like every Julia matrix;
`clean=true` fuses `clean!` (src/core.jl:478-484).  Float32 results are widened to Float64 as the reference does for
`GPU=true` (src/core.jl:413).
"""
function predict(g::Graph{T}, rows::Symbol=:query; clean::Bool=false, range=nothing) where {T}
    kind = rows === :query ? SS_ROWS_QUERY : SS_ROWS_SOURCE
    n = rows === :query ? g.nq : g.ns
    lo, hi = range === nothing ? (0, n) : (first(range) - 1, last(range))
    out = Matrix{T}(undef, hi - lo, g.nt)
    rc = if T === Float32
        ccall((:ss_predict_f32, LIB), Cint, (Ptr{Cvoid}, Cint, Int64, Int64, Cint, Ptr{Float32}, Int64, Cint, Cint),
              g.handle, kind, lo, hi, clean ? 1 : 0, out, max(hi - lo, 1), SS_LAYOUT_COLMAJOR, SS_MEM_HOST)
    else
        ccall((:ss_predict_f64, LIB), Cint, (Ptr{Cvoid}, Cint, Int64, Int64, Cint, Ptr{Float64}, Int64, Cint, Cint),
              g.handle, kind, lo, hi, clean ? 1 : 0, out, max(hi - lo, 1), SS_LAYOUT_COLMAJOR, SS_MEM_HOST)
    end
    check(rc)
    return Matrix{Float64}(out)
end

"""
    predict_loo(g; clean=true, range=nothing)

All leave-one-out folds of `construct(y, X, [source_i])` + `predict` (+ `clean!`) from one resident graph
(`g = graph(nothing, X, y)` with square `X`), rows `range` (default all sources).
"""
function predict_loo(g::Graph{T}; clean::Bool=true, range=nothing) where {T}
    lo, hi = range === nothing ? (0, g.ns) : (first(range) - 1, last(range))
    out = Matrix{T}(undef, hi - lo, g.nt)
    rc = if T === Float32
        ccall((:ss_predict_loo_f32, LIB), Cint, (Ptr{Cvoid}, Int64, Int64, Cint, Ptr{Float32}, Int64, Cint, Cint),
              g.handle, lo, hi, clean ? 1 : 0, out, max(hi - lo, 1), SS_LAYOUT_COLMAJOR, SS_MEM_HOST)
    else
        ccall((:ss_predict_loo_f64, LIB), Cint, (Ptr{Cvoid}, Int64, Int64, Cint, Ptr{Float64}, Int64, Cint, Cint),
              g.handle, lo, hi, clean ? 1 : 0, out, max(hi - lo, 1), SS_LAYOUT_COLMAJOR, SS_MEM_HOST)
    end
    check(rc)
    return Matrix{Float64}(out)
end

"""
    predict_kfold(g, fold_of_source; clean=true)

k-fold cross-validation in one call (`fold_of_source[i] in 1:k`, e.g. from `split`): row `i` is what the fold loop
`construct(y, X, members)` + `predict` (+ `clean!`) gives for source `i` when its fold is held out.
"""
function predict_kfold(g::Graph{T}, fold_of_source::AbstractVector{<:Integer}; clean::Bool=true) where {T}
    length(fold_of_source) == g.ns || throw(AssertionError("one fold index per source is needed"))
    folds = Vector{Int32}(fold_of_source .- 1)
    nfolds = Int(maximum(folds)) + 1
    out = Matrix{T}(undef, g.ns, g.nt)
    rc = if T === Float32
        ccall((:ss_predict_kfold_f32, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}, Cint, Cint, Ptr{Float32}, Int64, Cint, Cint),
              g.handle, folds, nfolds, clean ? 1 : 0, out, max(g.ns, 1), SS_LAYOUT_COLMAJOR, SS_MEM_HOST)
    else
        ccall((:ss_predict_kfold_f64, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}, Cint, Cint, Ptr{Float64}, Int64, Cint, Cint),
              g.handle, folds, nfolds, clean ? 1 : 0, out, max(g.ns, 1), SS_LAYOUT_COLMAJOR, SS_MEM_HOST)
    end
    check(rc)
    return Matrix{Float64}(out)
end

# ------------------------------------------------------------------------------------------------ ranked evaluation
"""
    topl(scores::Matrix{Float32}, L) -> (idx, val)

The L best targets of every row of a `rows x targets` score matrix in `sortperm(yhat, rev=true)` order
(src/performance.jl:308-385: recallatL / precisionatL need nothing else).  The library wants the block row-major,
i.e. the transpose of the Julia matrix as it lies in memory.  `idx` is 1-based.
"""
function topl(scores::Matrix{Float32}, L::Integer)
    nrows, ncols = size(scores)
    rowmajor = Matrix{Float32}(scores')          # ncols x nrows column-major == nrows x ncols row-major
    idx = Matrix{Int32}(undef, L, nrows)
    val = Matrix{Float32}(undef, L, nrows)
    check(ccall((:ss_topl_f32, LIB), Cint, (Ptr{Float32}, Int64, Int64, Int64, Cint, Ptr{Int32}, Ptr{Float32}, Cint),
                rowmajor, nrows, ncols, ncols, L, idx, val, SS_MEM_HOST))
    return Matrix{Int}(idx') .+ 1, Matrix{Float32}(val')
end

"""
    rank_metrics(y, yhat; alpha=20.0) -> (AuROC, AuPRC, BEDROC, validity_ratio)

The threshold-free metrics of src/performance.jl:22-89,558-560 for one label / score vector, on the device.
"""
function rank_metrics(y::AbstractVector, yhat::AbstractVector; alpha::Float64=20.0)
    length(y) == length(yhat) || throw(AssertionError("The number of scores must be equal to the number of labels"))
    labels = Vector{UInt8}(y .!= 0)
    scores = Vector{Float32}(yhat)
    out = Vector{Float64}(undef, 4)
    check(ccall((:ss_rank_metrics_f32, LIB), Cint, (Ptr{UInt8}, Ptr{Float32}, Int64, Float64, Ptr{Float64}, Cint),
                labels, scores, length(scores), alpha, out, SS_MEM_HOST))
    return (AuROC=out[1], AuPRC=out[2], BEDROC=out[3], validity_ratio=out[4])
end

"""
    rank_metrics_rows(y, yhat; alpha=20.0, L=20) -> Matrix{Float64} (rows x 6)

The ranking metrics of every row of a `rows x targets` score matrix against the 0/1 label matrix `y` of the same
size, on the device: columns AuROC, AuPRC, BEDROC(alpha), validity ratio (src/performance.jl:22-89,558-560),
recall@L and precision@L (src/performance.jl:308-385).  The labels go over as host CSR (the transpose of `y` as a
SparseMatrixCSC is the CSR of `y`), the scores row-contiguous (the transpose of the Julia matrix as it lies in memory).
"""
function rank_metrics_rows(y::AbstractMatrix, yhat::AbstractMatrix{T}; alpha::Float64=20.0, L::Integer=20) where {T<:Union{Float32,Float64}}
    size(y) == size(yhat) || throw(AssertionError("Number of predictions and labels don't match"))
    nrows, ncols = size(yhat)
    ncols > L || throw(AssertionError("Number of labels is less than length (L > y)"))
    yt = SparseMatrixCSC{Float64,Int64}(sparse(transpose(y .!= 0)))   # columns of yt = rows of y
    dropzeros!(yt)
    ptr = Vector{Int64}(yt.colptr)        # 1-based
    idx = Vector{Int32}(yt.rowval)        # 1-based
    rowmajor = Matrix{T}(transpose(yhat))
    out = Matrix{Float64}(undef, 6, nrows)
    rc = if T === Float32
        ccall((:ss_rank_metrics_rows_f32, LIB), Cint,
              (Ptr{Int64}, Ptr{Int32}, Cint, Ptr{Float32}, Int64, Int64, Int64, Float64, Cint, Ptr{Float64}, Cint),
              ptr, idx, 1, rowmajor, nrows, ncols, ncols, alpha, L, out, SS_MEM_HOST)
    else
        ccall((:ss_rank_metrics_rows_f64, LIB), Cint,
              (Ptr{Int64}, Ptr{Int32}, Cint, Ptr{Float64}, Int64, Int64, Int64, Float64, Cint, Ptr{Float64}, Cint),
              ptr, idx, 1, rowmajor, nrows, ncols, ncols, alpha, L, out, SS_MEM_HOST)
    end
    check(rc)
    return Matrix{Float64}(out')
end

"""
    evaluate_loo(g, i_begin, i_end; clean=true, alpha=20.0, L=20, block_rows=0) -> Matrix{Float64} (n x 6)

The leave-one-out folds `i_begin:i_end` (1-based, inclusive) of `predict_loo` ranked against the graph's own labels,
without the scores leaving the device: one row of `rank_metrics_rows` per fold.
"""
function evaluate_loo(g::Graph{T}, i_begin::Integer, i_end::Integer; clean::Bool=true, alpha::Float64=20.0,
                      L::Integer=20, block_rows::Integer=0) where {T}
    lo, hi = i_begin - 1, i_end
    out = Matrix{Float64}(undef, 6, max(hi - lo, 0))
    rc = if T === Float32
        ccall((:ss_evaluate_loo_f32, LIB), Cint, (Ptr{Cvoid}, Int64, Int64, Cint, Float64, Cint, Int64, Ptr{Float64}, Cint),
              g.handle, lo, hi, clean ? 1 : 0, alpha, L, block_rows, out, SS_MEM_HOST)
    else
        ccall((:ss_evaluate_loo_f64, LIB), Cint, (Ptr{Cvoid}, Int64, Int64, Cint, Float64, Cint, Int64, Ptr{Float64}, Cint),
              g.handle, lo, hi, clean ? 1 : 0, alpha, L, block_rows, out, SS_MEM_HOST)
    end
    check(rc)
    return Matrix{Float64}(out')
end

"""
    binary_metrics_rows(y, yhat) -> Matrix{Float64} (rows x 18)

Binary prediction metrics of every row of a `rows x targets` score matrix over all of the row's thresholds, on the
device: for f1score, mcc, accuracy, balancedaccuracy, recall and precision (src/performance.jl:102-296) the max, mean
and std over the row's distinct scores, as maxperformance / meanperformance / meanstdperformance
(src/performance.jl:420-520) give them; column 3m + s (1-based: 3(m-1) + s) with s = max, mean, std.  A vector pair is
one row.
"""
function binary_metrics_rows(y::AbstractMatrix, yhat::AbstractMatrix{T}) where {T<:Union{Float32,Float64}}
    size(y) == size(yhat) || throw(AssertionError("Number of predictions and labels don't match"))
    nrows, ncols = size(yhat)
    yt = SparseMatrixCSC{Float64,Int64}(sparse(transpose(y .!= 0)))   # columns of yt = rows of y
    dropzeros!(yt)
    ptr = Vector{Int64}(yt.colptr)        # 1-based
    idx = Vector{Int32}(yt.rowval)        # 1-based
    rowmajor = Matrix{T}(transpose(yhat))
    out = Matrix{Float64}(undef, 18, nrows)
    rc = if T === Float32
        ccall((:ss_binary_metrics_rows_f32, LIB), Cint,
              (Ptr{Int64}, Ptr{Int32}, Cint, Ptr{Float32}, Int64, Int64, Int64, Ptr{Float64}, Cint),
              ptr, idx, 1, rowmajor, nrows, ncols, ncols, out, SS_MEM_HOST)
    else
        ccall((:ss_binary_metrics_rows_f64, LIB), Cint,
              (Ptr{Int64}, Ptr{Int32}, Cint, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Cint),
              ptr, idx, 1, rowmajor, nrows, ncols, ncols, out, SS_MEM_HOST)
    end
    check(rc)
    return Matrix{Float64}(out')
end
binary_metrics_rows(y::AbstractVector, yhat::AbstractVector) = binary_metrics_rows(reshape(y, 1, :), reshape(yhat, 1, :))

"""
    evaluate_loo_binary(g, i_begin, i_end; clean=true, block_rows=0) -> Matrix{Float64} (n x 18)

The leave-one-out folds `i_begin:i_end` (1-based, inclusive) of `predict_loo` judged by the binary prediction metrics
against the graph's own labels, without the scores leaving the device: one row of `binary_metrics_rows` per fold.
"""
function evaluate_loo_binary(g::Graph{T}, i_begin::Integer, i_end::Integer; clean::Bool=true,
                             block_rows::Integer=0) where {T}
    lo, hi = i_begin - 1, i_end
    out = Matrix{Float64}(undef, 18, max(hi - lo, 0))
    rc = if T === Float32
        ccall((:ss_evaluate_loo_binary_f32, LIB), Cint, (Ptr{Cvoid}, Int64, Int64, Cint, Int64, Ptr{Float64}, Cint),
              g.handle, lo, hi, clean ? 1 : 0, block_rows, out, SS_MEM_HOST)
    else
        ccall((:ss_evaluate_loo_binary_f64, LIB), Cint, (Ptr{Cvoid}, Int64, Int64, Cint, Int64, Ptr{Float64}, Cint),
              g.handle, lo, hi, clean ? 1 : 0, block_rows, out, SS_MEM_HOST)
    end
    check(rc)
    return Matrix{Float64}(out')
end

"""
    predict_kfold_rows(g, fold_of_source, i_begin, i_end; clean=true) -> Matrix{Float64} (n x nt)

Rows `i_begin:i_end` (1-based, inclusive) of `predict_kfold(g, fold_of_source)`, bitwise: a k-fold sweep sharded by
source range like `predict_loo`.  The whole assignment is checked; only the folds with members in the range are
recounted and predicted.
"""
function predict_kfold_rows(g::Graph{T}, fold_of_source::AbstractVector{<:Integer}, i_begin::Integer, i_end::Integer;
                            clean::Bool=true) where {T}
    length(fold_of_source) == g.ns || throw(AssertionError("one fold index per source is needed"))
    folds = Vector{Int32}(fold_of_source .- 1)
    nfolds = Int(maximum(folds)) + 1
    lo, hi = i_begin - 1, i_end
    out = Matrix{T}(undef, max(hi - lo, 0), g.nt)
    rc = if T === Float32
        ccall((:ss_predict_kfold_rows_f32, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Int32}, Cint, Int64, Int64, Cint, Ptr{Float32}, Int64, Cint, Cint),
              g.handle, folds, nfolds, lo, hi, clean ? 1 : 0, out, max(hi - lo, 1), SS_LAYOUT_COLMAJOR, SS_MEM_HOST)
    else
        ccall((:ss_predict_kfold_rows_f64, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Int32}, Cint, Int64, Int64, Cint, Ptr{Float64}, Int64, Cint, Cint),
              g.handle, folds, nfolds, lo, hi, clean ? 1 : 0, out, max(hi - lo, 1), SS_LAYOUT_COLMAJOR, SS_MEM_HOST)
    end
    check(rc)
    return Matrix{Float64}(out)
end

"""
    evaluate_kfold(g, fold_of_source, i_begin, i_end; clean=true, alpha=20.0, L=20, block_rows=0) -> Matrix{Float64} (n x 6)

The k-fold rows `i_begin:i_end` (1-based, inclusive) of `predict_kfold_rows` ranked against the graph's own labels,
without the scores leaving the device: one row of `rank_metrics_rows` per source.
"""
function evaluate_kfold(g::Graph{T}, fold_of_source::AbstractVector{<:Integer}, i_begin::Integer, i_end::Integer;
                        clean::Bool=true, alpha::Float64=20.0, L::Integer=20, block_rows::Integer=0) where {T}
    length(fold_of_source) == g.ns || throw(AssertionError("one fold index per source is needed"))
    folds = Vector{Int32}(fold_of_source .- 1)
    nfolds = Int(maximum(folds)) + 1
    lo, hi = i_begin - 1, i_end
    out = Matrix{Float64}(undef, 6, max(hi - lo, 0))
    rc = if T === Float32
        ccall((:ss_evaluate_kfold_f32, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Int32}, Cint, Int64, Int64, Cint, Float64, Cint, Int64, Ptr{Float64}, Cint),
              g.handle, folds, nfolds, lo, hi, clean ? 1 : 0, alpha, L, block_rows, out, SS_MEM_HOST)
    else
        ccall((:ss_evaluate_kfold_f64, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Int32}, Cint, Int64, Int64, Cint, Float64, Cint, Int64, Ptr{Float64}, Cint),
              g.handle, folds, nfolds, lo, hi, clean ? 1 : 0, alpha, L, block_rows, out, SS_MEM_HOST)
    end
    check(rc)
    return Matrix{Float64}(out')
end

"""
    evaluate_kfold_binary(g, fold_of_source, i_begin, i_end; clean=true, block_rows=0) -> Matrix{Float64} (n x 18)

The k-fold rows `i_begin:i_end` (1-based, inclusive) of `predict_kfold_rows` judged by the binary prediction metrics
against the graph's own labels, without the scores leaving the device: one row of `binary_metrics_rows` per source.
"""
function evaluate_kfold_binary(g::Graph{T}, fold_of_source::AbstractVector{<:Integer}, i_begin::Integer,
                               i_end::Integer; clean::Bool=true, block_rows::Integer=0) where {T}
    length(fold_of_source) == g.ns || throw(AssertionError("one fold index per source is needed"))
    folds = Vector{Int32}(fold_of_source .- 1)
    nfolds = Int(maximum(folds)) + 1
    lo, hi = i_begin - 1, i_end
    out = Matrix{Float64}(undef, 18, max(hi - lo, 0))
    rc = if T === Float32
        ccall((:ss_evaluate_kfold_binary_f32, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Int32}, Cint, Int64, Int64, Cint, Int64, Ptr{Float64}, Cint),
              g.handle, folds, nfolds, lo, hi, clean ? 1 : 0, block_rows, out, SS_MEM_HOST)
    else
        ccall((:ss_evaluate_kfold_binary_f64, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Int32}, Cint, Int64, Int64, Cint, Int64, Ptr{Float64}, Cint),
              g.handle, folds, nfolds, lo, hi, clean ? 1 : 0, block_rows, out, SS_MEM_HOST)
    end
    check(rc)
    return Matrix{Float64}(out')
end

# ------------------------------------------------------------------------------------------------ raw W*R SpMM
mutable struct SpMat{T<:Union{Float32,Float64}}
    handle::Ptr{Cvoid}
    rows::Int
    cols::Int
    function SpMat{T}(h, rows, cols) where {T}
        w = new{T}(h, rows, cols)
        finalizer(destroy!, w)
        return w
    end
end

function destroy!(w::SpMat)
    if w.handle != C_NULL
        ccall((:ss_spmat_destroy, LIB), Cint, (Ptr{Cvoid},), w.handle)
        w.handle = C_NULL
    end
    return nothing
end

"One sparse operand W of F = W*R, device resident (kernel unit tests and the roofline benchmark)."
function spmat(W::SparseMatrixCSC; T::Type=Float64)
    p, i, v = _csr(W, T)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = if T === Float32
        ccall((:ss_spmat_create_csr_f32, LIB), Cint,
              (Int64, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Float32}, Cint, Cint, Ref{Ptr{Cvoid}}),
              size(W, 1), size(W, 2), p, i, v, 1, SS_MEM_HOST, h)
    else
        ccall((:ss_spmat_create_csr_f64, LIB), Cint,
              (Int64, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Float64}, Cint, Cint, Ref{Ptr{Cvoid}}),
              size(W, 1), size(W, 2), p, i, v, 1, SS_MEM_HOST, h)
    end
    check(rc)
    return SpMat{T}(h[], size(W, 1), size(W, 2))
end

"F = W * R for a dense column-major R (cols(W) x B)."
function spmm(w::SpMat{T}, R::Matrix{T}) where {T}
    size(R, 1) == w.cols || throw(DimensionMismatch("R must have cols(W) rows"))
    B = size(R, 2)
    F = Matrix{T}(undef, w.rows, B)
    rc = if T === Float32
        ccall((:ss_spmm_f32, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Int64, Int64, Cint, Ptr{Float32}, Int64, Cint, Cint),
              w.handle, R, B, max(w.cols, 1), SS_LAYOUT_COLMAJOR, F, max(w.rows, 1), SS_LAYOUT_COLMAJOR, SS_MEM_HOST)
    else
        ccall((:ss_spmm_f64, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Cint, Ptr{Float64}, Int64, Cint, Cint),
              w.handle, R, B, max(w.cols, 1), SS_LAYOUT_COLMAJOR, F, max(w.rows, 1), SS_LAYOUT_COLMAJOR, SS_MEM_HOST)
    end
    check(rc)
    return F
end

"Algorithmic bytes and flops of one spmm call with B columns (SURVEY.md 8d)."
function spmat_cost(w::SpMat, B::Integer)
    bytes, flops = Ref{Float64}(0.0), Ref{Float64}(0.0)
    check(ccall((:ss_spmat_cost, LIB), Cint, (Ptr{Cvoid}, Int64, Ref{Float64}, Ref{Float64}), w.handle, B, bytes, flops))
    return bytes[], flops[]
end

# ------------------------------------------------------------------------------------------------ pooled evaluation
"""A pooled (score, label) table on the device: AuROC(vec(y), vec(ŷ)), AuPRC and maxperformance(vec(y), vec(ŷ), f)
of a whole cross-validation, built where the scores are produced (include/simspread_hip.h, pooled evaluation)."""
mutable struct Pool{T<:Union{Float32,Float64}}
    handle::Ptr{Cvoid}
    function Pool{T}(h) where {T}
        p = new{T}(h)
        finalizer(destroy!, p)
        return p
    end
end

function destroy!(p::Pool)
    if p.handle != C_NULL
        ccall((:ss_pool_destroy, LIB), Cint, (Ptr{Cvoid},), p.handle)
        p.handle = C_NULL
    end
    return nothing
end

"An empty pool; max_entries = 0: the library's bound from the free device memory."
function pool(T::Type=Float64; max_entries::Integer=0)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = if T === Float32
        ccall((:ss_pool_create_f32, LIB), Cint, (Int64, Ref{Ptr{Cvoid}}), max_entries, h)
    else
        ccall((:ss_pool_create_f64, LIB), Cint, (Int64, Ref{Ptr{Cvoid}}), max_entries, h)
    end
    check(rc)
    return Pool{T}(h[])
end

pool_reset!(p::Pool) = (check(ccall((:ss_pool_reset, LIB), Cint, (Ptr{Cvoid},), p.handle)); p)

"(pairs, positives, entries stored, max_entries)"
function pool_info(p::Pool)
    info = zeros(Int64, 4)
    check(ccall((:ss_pool_info, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}), p.handle, info))
    return Tuple(info)
end

"""Pool every (ŷ[i, j], y[i, j]) pair of a score matrix.  Pooling ignores order, so the column-major matrix is passed as
the rows of its transpose, and the CSC pattern of y (same shape) is the 1-based CSR of those rows."""
function pool_add!(p::Pool{T}, y::SparseMatrixCSC, yhat::Matrix{T}) where {T}
    size(y) == size(yhat) || throw(DimensionMismatch("labels and scores differ in shape"))
    yb = dropzeros(y)
    ptr, idx = Vector{Int64}(yb.colptr), Vector{Int32}(yb.rowval)
    nr, nc = size(yhat, 2), size(yhat, 1)
    rc = if T === Float32
        ccall((:ss_pool_add_rows_f32, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int32}, Cint, Ptr{Float32}, Int64, Int64, Int64, Cint),
              p.handle, ptr, idx, 1, yhat, nr, nc, max(nc, 1), SS_MEM_HOST)
    else
        ccall((:ss_pool_add_rows_f64, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int32}, Cint, Ptr{Float64}, Int64, Int64, Int64, Cint),
              p.handle, ptr, idx, 1, yhat, nr, nc, max(nc, 1), SS_MEM_HOST)
    end
    check(rc)
    return p
end

"Pool the leave-one-out folds i_begin:i_end (1-based, inclusive) against the graph's own labels."
function pool_add_loo!(p::Pool{T}, g::Graph{T}, i_begin::Integer, i_end::Integer; clean::Bool=true,
                       block_rows::Integer=0) where {T}
    rc = if T === Float32
        ccall((:ss_pool_add_loo_f32, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Cint, Int64),
              p.handle, g.handle, i_begin - 1, i_end, clean ? 1 : 0, block_rows)
    else
        ccall((:ss_pool_add_loo_f64, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Cint, Int64),
              p.handle, g.handle, i_begin - 1, i_end, clean ? 1 : 0, block_rows)
    end
    check(rc)
    return p
end

"Pool the k-fold rows i_begin:i_end (1-based, inclusive; fold ids 1..k per source)."
function pool_add_kfold!(p::Pool{T}, g::Graph{T}, fold_of_source::AbstractVector{<:Integer}, i_begin::Integer,
                         i_end::Integer; clean::Bool=true, block_rows::Integer=0) where {T}
    length(fold_of_source) == g.ns || throw(AssertionError("one fold index per source is needed"))
    folds = Vector{Int32}(fold_of_source .- 1)
    nfolds = Int(maximum(folds)) + 1
    rc = if T === Float32
        ccall((:ss_pool_add_kfold_f32, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int32}, Cint, Int64, Int64, Cint, Int64, Cint),
              p.handle, g.handle, folds, nfolds, i_begin - 1, i_end, clean ? 1 : 0, block_rows, SS_MEM_HOST)
    else
        ccall((:ss_pool_add_kfold_f64, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int32}, Cint, Int64, Int64, Cint, Int64, Cint),
              p.handle, g.handle, folds, nfolds, i_begin - 1, i_end, clean ? 1 : 0, block_rows, SS_MEM_HOST)
    end
    check(rc)
    return p
end

"dst gains every pair of src."
function pool_merge!(dst::Pool{T}, src::Pool{T}) where {T}
    check(ccall((:ss_pool_merge, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), dst.handle, src.handle))
    return dst
end

"The table: (scores descending, positives, negatives)."
function pool_export(p::Pool{T}) where {T}
    n = Ref{Int64}(0)
    if T === Float32
        check(ccall((:ss_pool_export_f32, LIB), Cint,
                    (Ptr{Cvoid}, Ptr{Float32}, Ptr{Int64}, Ptr{Int64}, Int64, Ref{Int64}, Cint),
                    p.handle, C_NULL, C_NULL, C_NULL, 0, n, SS_MEM_HOST))
    else
        check(ccall((:ss_pool_export_f64, LIB), Cint,
                    (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Int64, Ref{Int64}, Cint),
                    p.handle, C_NULL, C_NULL, C_NULL, 0, n, SS_MEM_HOST))
    end
    keys, np, nn = Vector{T}(undef, n[]), Vector{Int64}(undef, n[]), Vector{Int64}(undef, n[])
    rc = if T === Float32
        ccall((:ss_pool_export_f32, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Float32}, Ptr{Int64}, Ptr{Int64}, Int64, Ref{Int64}, Cint),
              p.handle, keys, np, nn, length(keys), n, SS_MEM_HOST)
    else
        ccall((:ss_pool_export_f64, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Int64, Ref{Int64}, Cint),
              p.handle, keys, np, nn, length(keys), n, SS_MEM_HOST)
    end
    check(rc)
    return keys, np, nn
end

"Add a table such as pool_export returns (another rank's, for instance)."
function pool_import!(p::Pool{T}, keys::Vector{T}, npos::Vector{Int64}, nneg::Vector{Int64}) where {T}
    length(keys) == length(npos) == length(nneg) || throw(DimensionMismatch("table columns differ in length"))
    rc = if T === Float32
        ccall((:ss_pool_import_f32, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Int64}, Ptr{Int64}, Int64, Cint),
              p.handle, keys, npos, nneg, length(keys), SS_MEM_HOST)
    else
        ccall((:ss_pool_import_f64, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Int64, Cint),
              p.handle, keys, npos, nneg, length(keys), SS_MEM_HOST)
    end
    check(rc)
    return p
end

const POOL_FIELDS = (:AuROC, :AuPRC, :validity_ratio,
                     (Symbol(m, "_", s) for m in (:f1score, :mcc, :accuracy, :balancedaccuracy, :recall, :precision)
                      for s in (:max, :mean, :std))...)

"The 21 pooled numbers as a NamedTuple (AuROC, AuPRC, validity_ratio, then max / mean / std of the six metrics)."
function pool_metrics(p::Pool)
    out = zeros(Float64, 21)
    check(ccall((:ss_pool_metrics, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}), p.handle, out))
    return NamedTuple{POOL_FIELDS}(Tuple(out))
end

# ------------------------------------------------------------------------------------------------ per-target top-L
"""Per target the L best rows seen so far on the device: recallatL / precisionatL(y, ŷ, grouping, L) with grouping =
the target of every entry of vec(ŷ), and the virtual-screening list of every target (include/simspread_hip.h,
per-target top-L)."""
mutable struct TargetTopL{T<:Union{Float32,Float64}}
    handle::Ptr{Cvoid}
    function TargetTopL{T}(h) where {T}
        p = new{T}(h)
        finalizer(destroy!, p)
        return p
    end
end

function destroy!(p::TargetTopL)
    if p.handle != C_NULL
        ccall((:ss_target_topl_destroy, LIB), Cint, (Ptr{Cvoid},), p.handle)
        p.handle = C_NULL
    end
    return nothing
end

"An empty table for nt targets, lists of L (1 <= L <= 1024)."
function target_topl(T::Type, nt::Integer, L::Integer=20)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = if T === Float32
        ccall((:ss_target_topl_create_f32, LIB), Cint, (Int64, Cint, Ref{Ptr{Cvoid}}), nt, L, h)
    else
        ccall((:ss_target_topl_create_f64, LIB), Cint, (Int64, Cint, Ref{Ptr{Cvoid}}), nt, L, h)
    end
    check(rc)
    return TargetTopL{T}(h[])
end

target_topl_reset!(p::TargetTopL) = (check(ccall((:ss_target_topl_reset, LIB), Cint, (Ptr{Cvoid},), p.handle)); p)

"(nt, L, rows added, positives)"
function target_topl_info(p::TargetTopL)
    info = zeros(Int64, 4)
    check(ccall((:ss_target_topl_info, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}), p.handle, info))
    return Tuple(info)
end

"""Add the rows of a score matrix ŷ (rows x targets) with labels y (same shape); row i gets the id
row_begin + i - 1 (0-based ids, distinct across adds)."""
function target_topl_add!(p::TargetTopL{T}, y::SparseMatrixCSC, yhat::Matrix{T}; row_begin::Integer=0) where {T}
    size(y) == size(yhat) || throw(DimensionMismatch("labels and scores differ in shape"))
    yr = permutedims(yhat)                       # column-major nt x n = the rows of ŷ, row-major
    yt = dropzeros(copy(transpose(y)))           # its CSC = the 1-based CSR of y's rows
    ptr, idx = Vector{Int64}(yt.colptr), Vector{Int32}(yt.rowval)
    nr, nc = size(yhat, 1), size(yhat, 2)
    rc = if T === Float32
        ccall((:ss_target_topl_add_rows_f32, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int32}, Cint, Ptr{Float32}, Int64, Int64, Int64, Int64, Cint),
              p.handle, ptr, idx, 1, yr, nr, nc, max(nc, 1), row_begin, SS_MEM_HOST)
    else
        ccall((:ss_target_topl_add_rows_f64, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int32}, Cint, Ptr{Float64}, Int64, Int64, Int64, Int64, Cint),
              p.handle, ptr, idx, 1, yr, nr, nc, max(nc, 1), row_begin, SS_MEM_HOST)
    end
    check(rc)
    return p
end

"Add the leave-one-out folds i_begin:i_end (1-based, inclusive) against the graph's own labels."
function target_topl_add_loo!(p::TargetTopL{T}, g::Graph{T}, i_begin::Integer, i_end::Integer; clean::Bool=true,
                              block_rows::Integer=0) where {T}
    rc = if T === Float32
        ccall((:ss_target_topl_add_loo_f32, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Cint, Int64),
              p.handle, g.handle, i_begin - 1, i_end, clean ? 1 : 0, block_rows)
    else
        ccall((:ss_target_topl_add_loo_f64, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Cint, Int64),
              p.handle, g.handle, i_begin - 1, i_end, clean ? 1 : 0, block_rows)
    end
    check(rc)
    return p
end

"Add the k-fold rows i_begin:i_end (1-based, inclusive; fold ids 1..k per source)."
function target_topl_add_kfold!(p::TargetTopL{T}, g::Graph{T}, fold_of_source::AbstractVector{<:Integer},
                                i_begin::Integer, i_end::Integer; clean::Bool=true, block_rows::Integer=0) where {T}
    length(fold_of_source) == g.ns || throw(AssertionError("one fold index per source is needed"))
    folds = Vector{Int32}(fold_of_source .- 1)
    nfolds = Int(maximum(folds)) + 1
    rc = if T === Float32
        ccall((:ss_target_topl_add_kfold_f32, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int32}, Cint, Int64, Int64, Cint, Int64, Cint),
              p.handle, g.handle, folds, nfolds, i_begin - 1, i_end, clean ? 1 : 0, block_rows, SS_MEM_HOST)
    else
        ccall((:ss_target_topl_add_kfold_f64, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int32}, Cint, Int64, Int64, Cint, Int64, Cint),
              p.handle, g.handle, folds, nfolds, i_begin - 1, i_end, clean ? 1 : 0, block_rows, SS_MEM_HOST)
    end
    check(rc)
    return p
end

"dst gains every row of src."
function target_topl_merge!(dst::TargetTopL{T}, src::TargetTopL{T}) where {T}
    check(ccall((:ss_target_topl_merge, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), dst.handle, src.handle))
    return dst
end

"The table: (scores, row ids, labels) as fill x nt matrices (column t = target t's list), npos, rows added."
function target_topl_export(p::TargetTopL{T}) where {T}
    nt, L, rows, _ = target_topl_info(p)
    fill = min(L, rows)
    vals, rid, lab = Matrix{T}(undef, fill, nt), Matrix{Int64}(undef, fill, nt), Matrix{UInt8}(undef, fill, nt)
    np, n = Vector{Int64}(undef, nt), Ref{Int64}(0)
    rc = if T === Float32
        ccall((:ss_target_topl_export_f32, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Float32}, Ptr{Int64}, Ptr{UInt8}, Ptr{Int64}, Ref{Int64}, Cint),
              p.handle, vals, rid, lab, np, n, SS_MEM_HOST)
    else
        ccall((:ss_target_topl_export_f64, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int64}, Ptr{UInt8}, Ptr{Int64}, Ref{Int64}, Cint),
              p.handle, vals, rid, lab, np, n, SS_MEM_HOST)
    end
    check(rc)
    return vals, rid, lab, np, n[]
end

"Add a table such as target_topl_export returns (another rank's, for instance)."
function target_topl_import!(p::TargetTopL{T}, vals::Matrix{T}, rid::Matrix{Int64}, lab::Matrix{UInt8},
                             npos::Vector{Int64}, rows_added::Integer) where {T}
    rc = if T === Float32
        ccall((:ss_target_topl_import_f32, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Float32}, Ptr{Int64}, Ptr{UInt8}, Ptr{Int64}, Int64, Cint),
              p.handle, vals, rid, lab, npos, rows_added, SS_MEM_HOST)
    else
        ccall((:ss_target_topl_import_f64, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int64}, Ptr{UInt8}, Ptr{Int64}, Int64, Cint),
              p.handle, vals, rid, lab, npos, rows_added, SS_MEM_HOST)
    end
    check(rc)
    return p
end

"""(recallatL, precisionatL, recall over the targets with positives, targets with positives, hits, npos): the first
two are the reference's grouped numbers with grouping = target."""
function target_topl_metrics(p::TargetTopL)
    nt = target_topl_info(p)[1]
    hits, np, out = Vector{Int64}(undef, nt), Vector{Int64}(undef, nt), zeros(Float64, 4)
    check(ccall((:ss_target_topl_metrics, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Cint),
                p.handle, hits, np, out, SS_MEM_HOST))
    return (recallatL=out[1], precisionatL=out[2], recall_with_positives=out[3], targets_with_positives=Int(out[4]),
            hits=hits, npos=np)
end

end # module
