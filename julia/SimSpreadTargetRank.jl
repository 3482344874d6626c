# Per-target AuROC, AuPRC, BEDROC, validity ratio, recall@L and precision@L of whole sweeps: the `ccall` layer of
# include/simspread_hip_target_rank.h, one function per exported symbol, on the conventions of SimSpreadHIP.
#
#     include("SimSpreadHIP.jl"); include("SimSpreadTargetRank.jl")
#     h = SimSpreadTargetRank.target_rank(Float64, g.nt)
#     SimSpreadTargetRank.add_loo!(h, g, 1, g.ns)         # pass 1: collect the positives' scores
#     SimSpreadTargetRank.seal!(h)
#     SimSpreadTargetRank.add_loo!(h, g, 1, g.ns)         # pass 2: count the negatives against them
#     M = SimSpreadTargetRank.metrics(h; alpha=20.0, L=20)   # 6 x nt: column t = target t
#
# Row t of the result is what the per-row metrics give for (y[:, t], yhat[:, t]), ties by ascending row.  It costs two
# sweeps because the score matrix is never kept: the header explains why, and how the second pass is checked against
# the first.  Row ids are 0-based, as the library counts them.
module SimSpreadTargetRank

using SparseArrays
using ..SimSpreadHIP: LIB, check, Graph, SS_MEM_HOST

mutable struct TargetRank{T<:Union{Float32,Float64}}
    handle::Ptr{Cvoid}
    function TargetRank{T}(h) where {T}
        p = new{T}(h)
        finalizer(destroy!, p)
        return p
    end
end

function destroy!(p::TargetRank)
    if p.handle != C_NULL
        ccall((:ss_target_rank_destroy, LIB), Cint, (Ptr{Cvoid},), p.handle)
        p.handle = C_NULL
    end
    return nothing
end

"An empty handle for nt targets, collecting."
function target_rank(T::Type, nt::Integer)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = if T === Float32
        ccall((:ss_target_rank_create_f32, LIB), Cint, (Int64, Ref{Ptr{Cvoid}}), nt, h)
    else
        ccall((:ss_target_rank_create_f64, LIB), Cint, (Int64, Ref{Ptr{Cvoid}}), nt, h)
    end
    check(rc)
    return TargetRank{T}(h[])
end

reset!(p::TargetRank) = (check(ccall((:ss_target_rank_reset, LIB), Cint, (Ptr{Cvoid},), p.handle)); p)

"(nt, phase (0 collect, 1 count), rows collected, positives collected, rows counted, 0)"
function info(p::TargetRank)
    v = zeros(Int64, 6)
    check(ccall((:ss_target_rank_info, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}), p.handle, v))
    return Tuple(v)
end

"""Add the rows of a score matrix ŷ (rows x targets) with labels y (same shape); row i gets the id row_begin + i - 1.
Collected before `seal!`, counted after it."""
function add!(p::TargetRank{T}, y::SparseMatrixCSC, yhat::Matrix{T}; row_begin::Integer=0) where {T}
    size(y) == size(yhat) || throw(DimensionMismatch("labels and scores differ in shape"))
    yr = permutedims(yhat)                       # column-major nt x n = the rows of ŷ, row-major
    yt = dropzeros(copy(transpose(y)))           # its CSC = the 1-based CSR of y's rows
    ptr, idx = Vector{Int64}(yt.colptr), Vector{Int32}(yt.rowval)
    nr, nc = size(yhat, 1), size(yhat, 2)
    rc = if T === Float32
        ccall((:ss_target_rank_add_rows_f32, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int32}, Cint, Ptr{Float32}, Int64, Int64, Int64, Int64, Cint),
              p.handle, ptr, idx, 1, yr, nr, nc, max(nc, 1), row_begin, SS_MEM_HOST)
    else
        ccall((:ss_target_rank_add_rows_f64, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int32}, Cint, Ptr{Float64}, Int64, Int64, Int64, Int64, Cint),
              p.handle, ptr, idx, 1, yr, nr, nc, max(nc, 1), row_begin, SS_MEM_HOST)
    end
    check(rc)
    return p
end

"Add the leave-one-out folds i_begin:i_end (1-based, inclusive) against the graph's own labels."
function add_loo!(p::TargetRank{T}, g::Graph{T}, i_begin::Integer, i_end::Integer; clean::Bool=true,
                  block_rows::Integer=0) where {T}
    rc = if T === Float32
        ccall((:ss_target_rank_add_loo_f32, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Cint, Int64),
              p.handle, g.handle, i_begin - 1, i_end, clean ? 1 : 0, block_rows)
    else
        ccall((:ss_target_rank_add_loo_f64, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Cint, Int64),
              p.handle, g.handle, i_begin - 1, i_end, clean ? 1 : 0, block_rows)
    end
    check(rc)
    return p
end

"Add the k-fold rows i_begin:i_end (1-based, inclusive; fold ids 1..k per source)."
function add_kfold!(p::TargetRank{T}, g::Graph{T}, fold_of_source::AbstractVector{<:Integer}, i_begin::Integer,
                    i_end::Integer; clean::Bool=true, block_rows::Integer=0) where {T}
    length(fold_of_source) == g.ns || throw(AssertionError("one fold index per source is needed"))
    folds = Vector{Int32}(fold_of_source .- 1)
    nfolds = Int(maximum(folds)) + 1
    rc = if T === Float32
        ccall((:ss_target_rank_add_kfold_f32, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int32}, Cint, Int64, Int64, Cint, Int64, Cint),
              p.handle, g.handle, folds, nfolds, i_begin - 1, i_end, clean ? 1 : 0, block_rows, SS_MEM_HOST)
    else
        ccall((:ss_target_rank_add_kfold_f64, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int32}, Cint, Int64, Int64, Cint, Int64, Cint),
              p.handle, g.handle, folds, nfolds, i_begin - 1, i_end, clean ? 1 : 0, block_rows, SS_MEM_HOST)
    end
    check(rc)
    return p
end

"End the collect phase: the positives are sorted, later adds count."
seal!(p::TargetRank) = (check(ccall((:ss_target_rank_seal, LIB), Cint, (Ptr{Cvoid},), p.handle)); p)

"Collecting: dst gains src's positives and rows.  Counting: dst gains src's counts (the same sealed positives)."
function merge!(dst::TargetRank{T}, src::TargetRank{T}) where {T}
    check(ccall((:ss_target_rank_merge, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), dst.handle, src.handle))
    return dst
end

"(targets (0-based), row ids, scores, rows collected): collection order before `seal!`, sorted after it."
function export_positives(p::TargetRank{T}) where {T}
    np = info(p)[4]
    t, r, v, n = Vector{Int32}(undef, np), Vector{Int64}(undef, np), Vector{T}(undef, np), Ref{Int64}(0)
    rc = if T === Float32
        ccall((:ss_target_rank_export_positives_f32, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int64}, Ptr{Float32}, Ref{Int64}, Cint), p.handle, t, r, v, n, SS_MEM_HOST)
    else
        ccall((:ss_target_rank_export_positives_f64, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int64}, Ptr{Float64}, Ref{Int64}, Cint), p.handle, t, r, v, n, SS_MEM_HOST)
    end
    check(rc)
    return t, r, v, n[]
end

"Collecting: add positives such as export_positives returns (another rank's)."
function import_positives!(p::TargetRank{T}, t::Vector{Int32}, r::Vector{Int64}, v::Vector{T},
                           rows_added::Integer) where {T}
    length(t) == length(r) == length(v) || throw(DimensionMismatch("targets, rows and scores differ in length"))
    rc = if T === Float32
        ccall((:ss_target_rank_import_positives_f32, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int64}, Ptr{Float32}, Int64, Int64, Cint),
              p.handle, t, r, v, length(t), rows_added, SS_MEM_HOST)
    else
        ccall((:ss_target_rank_import_positives_f64, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int64}, Ptr{Float64}, Int64, Int64, Cint),
              p.handle, t, r, v, length(t), rows_added, SS_MEM_HOST)
    end
    check(rc)
    return p
end

"Counting: the Int64 count table (3 positives + 6 nt entries, layout in the header) and the rows counted."
function export_counts(p::TargetRank)
    nt, _, _, np = info(p)
    c, n = Vector{Int64}(undef, 3np + 6nt), Ref{Int64}(0)
    check(ccall((:ss_target_rank_export_counts, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ref{Int64}, Cint),
                p.handle, c, n, SS_MEM_HOST))
    return c, n[]
end

"Counting: add a table such as export_counts returns, taken against the same sealed positives."
function import_counts!(p::TargetRank, c::Vector{Int64}, rows_counted::Integer)
    check(ccall((:ss_target_rank_import_counts, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Int64, Int64, Cint),
                p.handle, c, length(c), rows_counted, SS_MEM_HOST))
    return p
end

"6 x nt: AuROC, AuPRC, BEDROC(alpha), validity ratio, recall@L, precision@L of every target."
function metrics(p::TargetRank; alpha::Real=20.0, L::Integer=20)
    out = Matrix{Float64}(undef, 6, info(p)[1])
    check(ccall((:ss_target_rank_metrics, LIB), Cint, (Ptr{Cvoid}, Float64, Cint, Ptr{Float64}, Cint),
                p.handle, Float64(alpha), L, out, SS_MEM_HOST))
    return out
end

end # module
