# Cutoff profiles: the `ccall` layer of include/simspread_hip_profile.h, one function per exported symbol, next to the
# producers of SimSpreadHIP and SimSpreadHalf.  For up to 32 ascending cuts, one pass over the pairs gives the exact `nnz`
# and the exact row degrees of the CSR the matching producer (`tanimoto_csr`, `jaccard_csr`, `dot_csr`, `dot_csr_h16`)
# would build at each of them -- no graph is built, and there is no 2^31 refusal.
#
#     include("SimSpreadHIP.jl"); include("SimSpreadScreening.jl"); include("SimSpreadHalf.jl")
#     include("SimSpreadProfile.jl")
#     p = SimSpreadProfile.dot_profile(E; metric=:cosine, cuts=0.5:0.05:0.95)
#     p.nnz                                        # Vector{Int64}, one per cut
#     SimSpreadProfile.coverage(p)                 # share of rows with a neighbour, per cut
#     SimSpreadProfile.alpha_for_nnz(p, 2^31 - 1)  # the lowest cut whose graph a producer accepts
#
# LAYOUT: exactly the matching producer's -- fingerprints `nwords x n` (`Matrix{UInt64}`), feature rows `n x d`, 16-bit
# matrices `d x n` (see SimSpreadHalf.jl).
module SimSpreadProfile

using ..SimSpreadHIP: LIB, check, _sim_metric, SS_MEM_HOST
using ..SimSpreadHalf: Half, _storage, _bits

const PROFILE_CUTS_MAX = 32

"""
    CutoffProfile

`cuts` (ascending), `nnz[b]` (`Int64`) and `degrees[i, b]` (`na x ncuts`, `Int32`) of the producer's graph at
`alpha = cuts[b]`, the `shape` `(na, nb)` and whether the profile is `symmetric` (`Fb === nothing`).
"""
struct CutoffProfile{T}
    cuts::Vector{T}
    nnz::Vector{Int64}
    degrees::Matrix{Int32}
    shape::Tuple{Int,Int}
    symmetric::Bool
end

# sorted, no NaN, 1..32: what the library refuses with SS_EINVAL, said here in Julia's words
function _cuts(::Type{T}, cuts) where {T}
    c = collect(T, cuts)
    1 <= length(c) <= PROFILE_CUTS_MAX || throw(ArgumentError("a profile takes 1..$PROFILE_CUTS_MAX cuts"))
    any(isnan, c) && throw(ArgumentError("a cut is NaN"))
    issorted(c) || throw(ArgumentError("cuts must be sorted (nondecreasing)"))
    return c
end

# the library writes rows[i * ncuts + b]: an ncuts x na column-major matrix, returned as na x ncuts
_outputs(na, nc) = (Vector{Int64}(undef, nc), Matrix{Int32}(undef, nc, na))
_profile(c, total, rows, na, nb, sym) = CutoffProfile(c, total, permutedims(rows), (na, nb), sym)

"""
    tanimoto_profile(Fa::Matrix{UInt64}, Fb=nothing; cuts, weighted=true, T=Float32)

The profile of `SimSpreadHIP.tanimoto_csr` at every cut.
"""
function tanimoto_profile(Fa::Matrix{UInt64}, Fb::Union{Nothing,Matrix{UInt64}}=nothing; cuts, weighted::Bool=true,
                          T::Type=Float32)
    nwords, na = size(Fa)
    nb = Fb === nothing ? na : size(Fb, 2)
    Fb === nothing || size(Fb, 1) == nwords || throw(ArgumentError("Fa and Fb have different fingerprint widths"))
    pb = Fb === nothing ? Ptr{UInt64}(C_NULL) : pointer(Fb)
    c = _cuts(T, cuts)
    total, rows = _outputs(na, length(c))
    rc = GC.@preserve Fa Fb if T === Float32
        ccall((:ss_similarity_tanimoto_profile_f32, LIB), Cint,
              (Ptr{UInt64}, Int64, Ptr{UInt64}, Int64, Int64, Ptr{Float32}, Cint, Cint, Ptr{Int64}, Ptr{Int32}, Cint),
              Fa, na, pb, nb, nwords, c, length(c), weighted ? 1 : 0, total, rows, SS_MEM_HOST)
    else
        ccall((:ss_similarity_tanimoto_profile_f64, LIB), Cint,
              (Ptr{UInt64}, Int64, Ptr{UInt64}, Int64, Int64, Ptr{Float64}, Cint, Cint, Ptr{Int64}, Ptr{Int32}, Cint),
              Fa, na, pb, nb, nwords, c, length(c), weighted ? 1 : 0, total, rows, SS_MEM_HOST)
    end
    check(rc)
    return _profile(c, total, rows, na, nb, Fb === nothing)
end

"""
    jaccard_profile(Fa::Matrix{T}, Fb=nothing; cuts, weighted=true) where T<:Union{Float32,Float64}

The profile of `SimSpreadHIP.jaccard_csr` at every cut (`Fa`: `na x d`, one sample per row).
"""
function jaccard_profile(Fa::Matrix{T}, Fb::Union{Nothing,Matrix{T}}=nothing; cuts,
                         weighted::Bool=true) where {T<:Union{Float32,Float64}}
    na, d = size(Fa)
    nb = Fb === nothing ? na : size(Fb, 1)
    Fb === nothing || size(Fb, 2) == d || throw(ArgumentError("Fa and Fb have different numbers of features"))
    pb = Fb === nothing ? Ptr{T}(C_NULL) : pointer(Fb)
    c = _cuts(T, cuts)
    total, rows = _outputs(na, length(c))
    rc = GC.@preserve Fa Fb if T === Float32
        ccall((:ss_similarity_jaccard_profile_f32, LIB), Cint,
              (Ptr{Float32}, Int64, Int64, Ptr{Float32}, Int64, Int64, Int64, Ptr{Float32}, Cint, Cint, Ptr{Int64},
               Ptr{Int32}, Cint),
              Fa, na, max(na, 1), pb, nb, max(nb, 1), d, c, length(c), weighted ? 1 : 0, total, rows, SS_MEM_HOST)
    else
        ccall((:ss_similarity_jaccard_profile_f64, LIB), Cint,
              (Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Cint, Cint, Ptr{Int64},
               Ptr{Int32}, Cint),
              Fa, na, max(na, 1), pb, nb, max(nb, 1), d, c, length(c), weighted ? 1 : 0, total, rows, SS_MEM_HOST)
    end
    check(rc)
    return _profile(c, total, rows, na, nb, Fb === nothing)
end

"""
    dot_profile(Fa::Matrix{T}, Fb=nothing; metric=:cosine, cuts, weighted=true) where T<:Union{Float32,Float64}

The profile of `SimSpreadHIP.dot_csr` at every cut; in symmetric mode the diagonal counts with `s = 1` exactly.
"""
function dot_profile(Fa::Matrix{T}, Fb::Union{Nothing,Matrix{T}}=nothing; metric::Symbol=:cosine, cuts,
                     weighted::Bool=true) where {T<:Union{Float32,Float64}}
    na, d = size(Fa)
    nb = Fb === nothing ? na : size(Fb, 1)
    Fb === nothing || size(Fb, 2) == d || throw(ArgumentError("Fa and Fb have different numbers of features"))
    pb = Fb === nothing ? Ptr{T}(C_NULL) : pointer(Fb)
    m = _sim_metric(metric)
    c = _cuts(T, cuts)
    total, rows = _outputs(na, length(c))
    rc = GC.@preserve Fa Fb if T === Float32
        ccall((:ss_similarity_dot_profile_f32, LIB), Cint,
              (Ptr{Float32}, Int64, Int64, Ptr{Float32}, Int64, Int64, Int64, Cint, Ptr{Float32}, Cint, Cint, Ptr{Int64},
               Ptr{Int32}, Cint),
              Fa, na, max(na, 1), pb, nb, max(nb, 1), d, m, c, length(c), weighted ? 1 : 0, total, rows, SS_MEM_HOST)
    else
        ccall((:ss_similarity_dot_profile_f64, LIB), Cint,
              (Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Int64, Int64, Cint, Ptr{Float64}, Cint, Cint, Ptr{Int64},
               Ptr{Int32}, Cint),
              Fa, na, max(na, 1), pb, nb, max(nb, 1), d, m, c, length(c), weighted ? 1 : 0, total, rows, SS_MEM_HOST)
    end
    check(rc)
    return _profile(c, total, rows, na, nb, Fb === nothing)
end

"""
    dot_profile_h16(Fa, Fb=nothing; storage=:bf16, metric=:cosine, cuts, weighted=true)

The profile of `SimSpreadHalf.dot_csr_h16` at every cut: `Fa` is `d x na`, one sample per column, as there.
"""
function dot_profile_h16(Fa::Half, Fb::Union{Nothing,Half}=nothing; storage::Symbol=:bf16, metric::Symbol=:cosine, cuts,
                         weighted::Bool=true)
    d, na = size(Fa)
    Fb === nothing || size(Fb, 1) == d || throw(ArgumentError("Fa and Fb have different numbers of features"))
    nb = Fb === nothing ? na : size(Fb, 2)
    st, m = _storage(Fa, Fb, storage), _sim_metric(metric)
    A = _bits(Fa)
    B = Fb === nothing ? nothing : _bits(Fb)
    pb = B === nothing ? Ptr{UInt16}(C_NULL) : pointer(B)
    c = _cuts(Float32, cuts)
    total, rows = _outputs(na, length(c))
    rc = GC.@preserve A B ccall((:ss_similarity_dot_profile_h16, LIB), Cint,
              (Ptr{UInt16}, Int64, Int64, Ptr{UInt16}, Int64, Int64, Int64, Cint, Cint, Ptr{Float32}, Cint, Cint,
               Ptr{Int64}, Ptr{Int32}, Cint),
              A, na, max(d, 1), pb, nb, max(d, 1), d, st, m, c, length(c), weighted ? 1 : 0, total, rows, SS_MEM_HOST)
    check(rc)
    return _profile(c, total, rows, na, nb, Fb === nothing)
end

# ---- what a profile is asked, on the host
"`fill(p)`: `nnz / (na * nb)` per cut."
fill(p::CutoffProfile) = prod(p.shape) == 0 ? zeros(length(p.cuts)) : p.nnz ./ prod(p.shape)

"""
    coverage(p; min_degree=1, exclude_self=false)

Per cut, the share of rows with at least `min_degree` entries.  `exclude_self` (symmetric profiles) does not count the
diagonal entry, whose similarity is 1: it is an entry exactly at the cuts `<= 1`.
"""
function coverage(p::CutoffProfile; min_degree::Integer=1, exclude_self::Bool=false)
    exclude_self && !p.symmetric && throw(ArgumentError("exclude_self needs a symmetric profile"))
    na = p.shape[1]
    na == 0 && return zeros(length(p.cuts))
    self = exclude_self ? Int.(p.cuts .<= 1) : zeros(Int, length(p.cuts))
    return [count(i -> max(p.degrees[i, b] - self[b], 0) >= min_degree, 1:na) / na for b in eachindex(p.cuts)]
end

"`alpha_for_nnz(p, budget)`: the smallest cut whose `nnz <= budget`, `nothing` when none."
function alpha_for_nnz(p::CutoffProfile, budget::Real)
    b = findfirst(<=(budget), p.nnz)
    return b === nothing ? nothing : p.cuts[b]
end

"`alpha_for_mean_degree(p, k)`: the smallest cut whose mean row degree `nnz / na <= k`, `nothing` when none."
function alpha_for_mean_degree(p::CutoffProfile, k::Real)
    b = findfirst(<=(k * p.shape[1]), p.nnz)
    return b === nothing ? nothing : p.cuts[b]
end

end # module
