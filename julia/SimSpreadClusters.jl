# Butina clusters of the similarity graph and cluster-aware folds: the `ccall` layer of
# include/simspread_hip_clusters.h, one function per exported symbol, on the conventions of SimSpreadHIP.
#
#     include("SimSpreadHIP.jl"); include("SimSpreadClusters.jl")
#     c = SimSpreadClusters.butina_fingerprint(F; cutoff=0.65)            # F: nwords x n packed fingerprints
#     fold = SimSpreadClusters.cluster_folds(c.label, 5)                  # 0-based fold ids, clusters kept whole
#     X = SimSpreadHIP.tanimoto_csr(F; alpha=0.65, weighted=false)
#     leak = SimSpreadClusters.cross_fold_edges(X, fold, 5)               # what the split still leaks, per fold
#
# The rule.  Neighbours N(i) = { j != i : (i,j) or (j,i) stored } (diagonal and duplicate entries ignored, an asymmetric
# pattern symmetrised by union), degree d_i = |N(i)|; i precedes j iff d_i > d_j, or d_i == d_j and i < j.  In that
# order every still-unassigned source becomes a centre and takes its still-unassigned neighbours (Taylor-Butina without
# re-counting).  Ties between equal degrees go to the lower index, which is not RDKit's tie order.  The result is unique
# and bitwise repeatable.  All outputs are 0-based, as the library writes them: `centre[i] + 1` is a Julia index.
module SimSpreadClusters

using SparseArrays
using ..SimSpreadHIP: LIB, check, _sim_metric, SS_MEM_HOST

"`centre[i]`: 0-based index of source i's centre; `label[i]`: its cluster, 0..nclusters-1 in priority order of the centres; `size[l+1]`: sources with label l; `rounds`: rounds of the device loop."
struct Clusters
    centre::Vector{Int32}
    label::Vector{Int32}
    size::Vector{Int32}
    rounds::Int
end

_outputs(n) = (Vector{Int32}(undef, n), Vector{Int32}(undef, n), Vector{Int32}(undef, n), Ref{Int64}(0), Ref{Int64}(0))
_result(centre, label, sizes, nc, rounds) = Clusters(centre, label, sizes[1:nc[]], Int(rounds[]))

# The pattern of a SparseMatrixCSC is handed over as the 1-based CSR of its transpose; the rule symmetrises, so the
# clusters are those of X itself.
function _pattern(X::SparseMatrixCSC)
    n = size(X, 1)
    n == size(X, 2) || throw(ArgumentError("a neighbour pattern is square"))
    return n, Vector{Int64}(X.colptr), Vector{Int32}(X.rowval)
end

"""
    butina_csr(X::SparseMatrixCSC) -> Clusters

Clusters of the n x n neighbour pattern `X` (values are not read).
"""
function butina_csr(X::SparseMatrixCSC)
    n, ptr, idx = _pattern(X)
    centre, label, sizes, nc, rounds = _outputs(n)
    check(ccall((:ss_cluster_butina_csr, LIB), Cint,
                (Int64, Ptr{Int64}, Ptr{Int32}, Cint, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}, Ptr{Int64}, Cint),
                n, ptr, idx, 1, centre, label, sizes, nc, rounds, SS_MEM_HOST))
    return _result(centre, label, sizes, nc, rounds)
end

"""
    butina_fingerprint(F::Matrix{UInt64}; cutoff, T=Float32) -> Clusters

Clusters of the fingerprints `F` (`nwords x n`) under Tanimoto `>= cutoff`: the pattern of `SimSpreadHIP.tanimoto_csr(F;
alpha=cutoff, weighted=false)`, made and consumed on the device.
"""
function butina_fingerprint(F::Matrix{UInt64}; cutoff::Real, T::Type=Float32)
    nwords, n = size(F)
    centre, label, sizes, nc, rounds = _outputs(n)
    rc = GC.@preserve F if T === Float32
        ccall((:ss_cluster_butina_fingerprint_f32, LIB), Cint,
              (Ptr{UInt64}, Int64, Int64, Float32, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}, Ptr{Int64}, Cint),
              F, n, nwords, Float32(cutoff), centre, label, sizes, nc, rounds, SS_MEM_HOST)
    else
        ccall((:ss_cluster_butina_fingerprint_f64, LIB), Cint,
              (Ptr{UInt64}, Int64, Int64, Float64, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}, Ptr{Int64}, Cint),
              F, n, nwords, Float64(cutoff), centre, label, sizes, nc, rounds, SS_MEM_HOST)
    end
    check(rc)
    return _result(centre, label, sizes, nc, rounds)
end

"""
    butina_features(F::Matrix{T}; cutoff) where T<:Union{Float32,Float64} -> Clusters

Clusters of the descriptor rows `F` (`n x d`) under weighted Jaccard `>= cutoff` (the pattern of
`SimSpreadHIP.jaccard_csr`).
"""
function butina_features(F::Matrix{T}; cutoff::Real) where {T<:Union{Float32,Float64}}
    n, d = size(F)
    centre, label, sizes, nc, rounds = _outputs(n)
    rc = GC.@preserve F if T === Float32
        ccall((:ss_cluster_butina_features_f32, LIB), Cint,
              (Ptr{Float32}, Int64, Int64, Int64, Float32, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}, Ptr{Int64},
               Cint),
              F, n, d, max(n, 1), Float32(cutoff), centre, label, sizes, nc, rounds, SS_MEM_HOST)
    else
        ccall((:ss_cluster_butina_features_f64, LIB), Cint,
              (Ptr{Float64}, Int64, Int64, Int64, Float64, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}, Ptr{Int64},
               Cint),
              F, n, d, max(n, 1), Float64(cutoff), centre, label, sizes, nc, rounds, SS_MEM_HOST)
    end
    check(rc)
    return _result(centre, label, sizes, nc, rounds)
end

"""
    butina_vectors(F::Matrix{T}; metric=:cosine, cutoff) where T<:Union{Float32,Float64} -> Clusters

Clusters of the embedding rows `F` (`n x d`) under `metric` (`:cosine`, `:tanimoto`, `:dice`) `>= cutoff` (the pattern of
`SimSpreadHIP.dot_csr`).
"""
function butina_vectors(F::Matrix{T}; metric::Symbol=:cosine, cutoff::Real) where {T<:Union{Float32,Float64}}
    n, d = size(F)
    m = _sim_metric(metric)
    centre, label, sizes, nc, rounds = _outputs(n)
    rc = GC.@preserve F if T === Float32
        ccall((:ss_cluster_butina_vectors_f32, LIB), Cint,
              (Cint, Ptr{Float32}, Int64, Int64, Int64, Float32, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int64},
               Ptr{Int64}, Cint),
              m, F, n, d, max(n, 1), Float32(cutoff), centre, label, sizes, nc, rounds, SS_MEM_HOST)
    else
        ccall((:ss_cluster_butina_vectors_f64, LIB), Cint,
              (Cint, Ptr{Float64}, Int64, Int64, Int64, Float64, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int64},
               Ptr{Int64}, Cint),
              m, F, n, d, max(n, 1), Float64(cutoff), centre, label, sizes, nc, rounds, SS_MEM_HOST)
    end
    check(rc)
    return _result(centre, label, sizes, nc, rounds)
end

"""
    cluster_folds(label::Vector{Int32}, nfolds) -> Vector{Int32}

0-based fold ids that keep every cluster whole: clusters by size descending (ties: label ascending), each to the fold
with the fewest sources so far (ties: the lowest fold id).  Host code in the library.  The vector goes straight into
`SimSpreadHIP.predict_kfold` / `evaluate_kfold`.
"""
function cluster_folds(label::Vector{Int32}, nfolds::Integer)
    n = length(label)
    nc = n == 0 ? 0 : Int(maximum(label)) + 1
    fold = Vector{Int32}(undef, n)
    check(ccall((:ss_cluster_folds, LIB), Cint, (Ptr{Int32}, Int64, Int64, Cint, Ptr{Int32}, Cint),
                label, n, nc, nfolds, fold, SS_MEM_HOST))
    return fold
end

"""
    cross_fold_edges(X::SparseMatrixCSC, fold::Vector{Int32}, nfolds) -> Vector{Int64}

`count[f+1]`: stored off-diagonal entries of `X` with one end in fold `f` and the other in another fold, counted by the
fold of the entry's column (the CSC is read as the CSR of the transpose; for a symmetric pattern that is the same).
"""
function cross_fold_edges(X::SparseMatrixCSC, fold::Vector{Int32}, nfolds::Integer)
    n, ptr, idx = _pattern(X)
    length(fold) == n || throw(ArgumentError("fold needs one entry per source"))
    count = zeros(Int64, nfolds)
    check(ccall((:ss_cluster_cross_edges, LIB), Cint,
                (Int64, Ptr{Int64}, Ptr{Int32}, Cint, Ptr{Int32}, Cint, Ptr{Int64}, Cint),
                n, ptr, idx, 1, fold, nfolds, count, SS_MEM_HOST))
    return count
end

end # module
