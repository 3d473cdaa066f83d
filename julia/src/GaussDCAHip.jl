# GaussDCAHip.jl -- the reference-side binding of libgdca.so.
#
# Drop-in for the hot path of GaussDCA.jl (src/GaussDCA.jl:28-42): same exported names, same
# keyword arguments and defaults as `gDCA` (src/GaussDCA.jl:8-16); the DCAUtils-named operators
# used by the reference (compute_weights, compute_weighted_frequencies, add_pseudocount,
# compute_FN, compute_DI_gauss) are thin `ccall` wrappers over include/gdca.h.
#
# The host pieces of the reference that are NOT on the hot path are not restated here: argument checks, ranking and
# printing are the reference's own functions (GaussDCA.check_arguments / compute_ranking / printrank,
# src/GaussDCA.jl:49-65, :88-99, :67-74), FASTA reading and duplicate removal are DCAUtils'.
#
# NOT EXECUTED in the build image (no Julia toolchain there); kept minimal and literal.  The struct layouts and
# status codes below are checked mechanically against include/gdca.h by
# tests/test_cabi_cpu.py::test_struct_layouts_agree_across_c_ctypes_and_julia.
module GaussDCAHip

export gDCA, gDCA_stepwise, printrank, compute_weights, compute_weighted_frequencies, add_pseudocount,
       compute_FN, compute_DI_gauss, sequence_energies, gDCA_energies, inv_cholesky_logdet, gDCA_loglik, pair_energies, mutation_scan, gDCA_mutation_scan, double_mutant_scan, double_mutant_energies, gDCA_double_mutant_scan, gDCA_double_mutants,
       species_blocks, pair_energies_blocked_dev, assign_blocks_dev, run_partner_match_dev, gDCA_partner_match

using LinearAlgebra
import DCAUtils                                   # host-side I/O only: read_fasta_alignment, remove_duplicate_sequences
import GaussDCA: check_arguments, compute_ranking, printrank   # unchanged host code of the reference

const libgdca = get(ENV, "LIBGDCA", "libgdca.so")

struct GdcaParams
    pseudocount::Cdouble
    theta::Cdouble      # < 0  =>  :auto
    score::Int32        # 0 = :frob, 1 = :DI
    apc::Int32
end

mutable struct GdcaStats
    theta::Cdouble; Meff::Cdouble; pair_identity_sum::UInt64
    thresh::Int32; info::Int32; N::Int32; M::Int32; q::Int32; n::Int32; n_pad::Int32; update_launches::Int32
    inverse_batch::Int32; refined::Int32
    ms_total::Cdouble; ms_theta::Cdouble; ms_weights::Cdouble; ms_covariance::Cdouble
    ms_inverse::Cdouble; ms_inverse_update::Cdouble; ms_score::Cdouble
    inverse_flops::Cdouble; update_flops::Cdouble
    sweep_ghz::Cdouble; inverse_norm1::Cdouble; matrix_norm1::Cdouble; cond_bound::Cdouble
    ms_fn::Cdouble; ms_pair_tally::Cdouble
    sweep_retries::Int32; reserved0::Int32
    GdcaStats() = new()
end

const CTX = Ref{Ptr{Cvoid}}(C_NULL)

function ctx()
    if CTX[] == C_NULL
        dev = parse(Int32, get(ENV, "GDCA_DEVICE", "0"))
        st = ccall((:gdca_ctx_create, libgdca), Cint, (Int32, Ref{Ptr{Cvoid}}), dev, CTX)
        st == 0 || error("gdca_ctx_create failed (status $st): no usable HIP device; there is no CPU fallback")
        # the library writes ITS sizeof(gdca_stats) into our struct: refuse a build whose layout is not the one mirrored above
        ver = ccall((:gdca_version, libgdca), Int32, ())
        sb = ccall((:gdca_stats_bytes, libgdca), Int32, ())
        pb = ccall((:gdca_params_bytes, libgdca), Int32, ())
        (ver == 6 && sb == sizeof(GdcaStats) && pb == sizeof(GdcaParams)) ||
            error("libgdca is version $ver with gdca_stats of $sb bytes; this binding mirrors version 6 with $(sizeof(GdcaStats)) bytes")
    end
    return CTX[]
end

function check(st::Integer, info::Integer = 0)
    st == 0 && return
    msg = unsafe_string(ccall((:gdca_last_error, libgdca), Cstring, (Ptr{Cvoid},), ctx()))
    st == 1 && throw(ArgumentError(msg))
    st == 2 && throw(PosDefException(info))
    st == 4 && throw(OutOfMemoryError())
    st == 5 && throw(LinearAlgebra.LAPACKException(info))   # what eigvals() raises inside compute_DI_gauss (:37)
    error("libgdca: $msg")
end

theta_arg(θ) = θ === :auto ? -1.0 : Float64(θ)

# tuning switch of the context (include/gdca.h: gdca_ctx_set_option), e.g. set_option("REFINE", "0") or set_option("GROUP", 4);
# the GDCA_* environment variables are read once, when the context is created
function set_option(key::AbstractString, value)
    check(ccall((:gdca_ctx_set_option, libgdca), Cint, (Ptr{Cvoid}, Cstring, Cstring), ctx(), String(key), string(value)))
end

# ---- the fused hot path: src/GaussDCA.jl:28-42 in one call --------------------------------
function hot_path(Z::Matrix{Int8}, q::Integer, pseudocount::Real, θ, score::Symbol)
    N, M = size(Z)
    S = Matrix{Float64}(undef, N, N)
    p = Ref(GdcaParams(Float64(pseudocount), theta_arg(θ), score == :DI ? 1 : 0, 1))
    st = GdcaStats()
    GC.@preserve Z S begin
        rc = ccall((:gdca_run, libgdca), Cint,
                   (Ptr{Cvoid}, Ptr{Int8}, Int32, Int32, Int32, Ref{GdcaParams}, Ptr{Float64}, Ref{GdcaStats}),
                   ctx(), Z, N, M, q, p, S, st)
    end
    check(rc, st.info)
    return S, st
end

# ... and src/GaussDCA.jl:28-44: the same followed by compute_ranking on the device; only the sorted ranking comes back
function hot_path_ranked(Z::Matrix{Int8}, q::Integer, pseudocount::Real, θ, score::Symbol, min_separation::Integer)
    N, M = size(Z)
    len = max(ccall((:gdca_ranking_length, libgdca), Int64, (Int32, Int32), N, min_separation), 0)
    ri = Vector{Int32}(undef, len)
    rj = Vector{Int32}(undef, len)
    rs = Vector{Float64}(undef, len)
    p = Ref(GdcaParams(Float64(pseudocount), theta_arg(θ), score == :DI ? 1 : 0, 1))
    st = GdcaStats()
    GC.@preserve Z ri rj rs begin
        rc = ccall((:gdca_run_ranked, libgdca), Cint,
                   (Ptr{Cvoid}, Ptr{Int8}, Int32, Int32, Int32, Ref{GdcaParams}, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ref{GdcaStats}),
                   ctx(), Z, N, M, q, p, min_separation, ri, rj, rs, st)
    end
    check(rc, st.info)
    return [(Int(ri[t]), Int(rj[t]), rs[t]) for t in 1:len], st
end

function gDCA(filename::AbstractString; pseudocount::Real = 0.8, θ = :auto, max_gap_fraction::Real = 0.9,
              score::Symbol = :frob, min_separation::Integer = 5, remove_dups::Bool = false)
    check_arguments(filename, pseudocount, θ, max_gap_fraction, score, min_separation)
    Z = DCAUtils.read_fasta_alignment(filename, max_gap_fraction)
    if remove_dups
        Z, _ = DCAUtils.remove_duplicate_sequences(Z)
    end
    q = Int(maximum(Z))
    q ≥ 32 && error("parameter q=$q is too big (max 31 is allowed)")
    R, st = hot_path_ranked(Z, q, pseudocount, θ, score, min_separation)
    # (gdca.h, gdca_stats.refined: -1 = the refinement of an ill-conditioned inverse cannot have converged and the Cholesky
    # fallback is switched off -- the Python mirror warns in the same case)
    st.refined < 0 && @warn "covariance too ill-conditioned for the refinement step and option CHOLESKY=0: scores are unreliable" pseudocount kappa_1 = st.matrix_norm1 * st.inverse_norm1
    return R
end

# ---- DCAUtils-named operators (call sites src/GaussDCA.jl:28,30,37,39) ----------------------
function compute_weights(Z::Matrix{Int8}, q::Integer, θ)
    N, M = size(Z)
    W = Vector{Float64}(undef, M); Meff = Ref{Cdouble}(0); th = Ref{Cdouble}(0); thr = Ref{Int32}(0)
    GC.@preserve Z W check(ccall((:gdca_compute_weights, libgdca), Cint,
        (Ptr{Cvoid}, Ptr{Int8}, Int32, Int32, Cdouble, Ptr{Float64}, Ref{Cdouble}, Ref{Cdouble}, Ref{Int32}),
        ctx(), Z, N, M, theta_arg(θ), W, Meff, th, thr))
    return W, Meff[]
end

function compute_weighted_frequencies(Z::Matrix{Int8}, q::Integer, θ)
    W, Meff = compute_weights(Z, q, θ)
    N, M = size(Z); n = N * (q - 1)
    Pi = Vector{Float64}(undef, n); Pij = Matrix{Float64}(undef, n, n)
    GC.@preserve Z W Pi Pij check(ccall((:gdca_frequencies, libgdca), Cint,
        (Ptr{Cvoid}, Ptr{Int8}, Int32, Int32, Int32, Ptr{Float64}, Cdouble, Ptr{Float64}, Ptr{Float64}),
        ctx(), Z, N, M, q, W, Meff, Pi, Pij))
    return Pi, Pij, Meff, W
end

function add_pseudocount(Pi_true::Vector{Float64}, Pij_true::Matrix{Float64}, pc::Float64, q::Integer = 21)
    n = length(Pi_true); N = n ÷ (q - 1)
    Pi = similar(Pi_true); Pij = similar(Pij_true)
    GC.@preserve Pi_true Pij_true Pi Pij check(ccall((:gdca_add_pseudocount, libgdca), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Cdouble, Ptr{Float64}, Ptr{Float64}),
        ctx(), Pi_true, Pij_true, N, q, pc, Pi, Pij))
    return Pi, Pij
end

function inv_cholesky(C::Matrix{Float64})   # mJ = inv(cholesky(C)), src/GaussDCA.jl:34
    A = copy(C); n = size(A, 1); info = Ref{Int32}(0)
    rc = GC.@preserve A ccall((:gdca_spd_inverse, libgdca), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int32, Ref{Int32}),
                              ctx(), A, n, info)
    check(rc, info[])
    return A
end

# (mJ, log det C): inv_cholesky and the sum of the logarithms of the pivots the inverse met (include/gdca.h, "log-likelihoods") --
# the constant between sequence_energies and a log-likelihood; mJ is bit for bit inv_cholesky's
function inv_cholesky_logdet(C::Matrix{Float64})
    A = copy(C); n = size(A, 1); info = Ref{Int32}(0); logdet = Ref{Float64}(NaN)
    rc = GC.@preserve A ccall((:gdca_spd_inverse_logdet, libgdca), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int32, Ref{Int32}, Ref{Float64}),
                              ctx(), A, n, info, logdet)
    check(rc, info[])
    return A, logdet[]
end

function compute_FN(mJ::Matrix{Float64}, q::Integer = 21)
    N = size(mJ, 1) ÷ (q - 1); S = Matrix{Float64}(undef, N, N)
    GC.@preserve mJ S check(ccall((:gdca_fn, libgdca), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int32, Int32, Ptr{Float64}),
                                  ctx(), mJ, N, q, S))
    return S
end

# E[k] = 1/2 (x_k - Pi)' mJ (x_k - Pi) for the K columns of X (N x K like Z): minus the log-likelihood of each sequence under the
# fitted Gaussian model, up to the model's constant (include/gdca.h, "energies").  Lower = fits better.
function sequence_energies(mJ::Matrix{Float64}, Pi::Vector{Float64}, X::Matrix{Int8}, q::Integer = 21)
    N, K = size(X); n = N * (q - 1)
    (size(mJ) == (n, n) && length(Pi) == n) || throw(ArgumentError("incompatible sizes of mJ, Pi, X and q"))
    E = Vector{Float64}(undef, K)
    GC.@preserve mJ Pi X E check(ccall((:gdca_energies, libgdca), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Ptr{Int8}, Int32, Ptr{Float64}), ctx(), mJ, Pi, N, q, X, K, E))
    return E
end

# E[a, b] for every pairing of the columns of XA (split x K_A: protein A's sites) with the columns of XB ((N - split) x K_B) under the
# model of the concatenated alignment (include/gdca.h, "pair energies"): what = :energy, the energy sequence_energies gives a (+) b, or
# :coupling, only the part that depends on the pairing (Pi may then be nothing)
function pair_energies(mJ::Matrix{Float64}, Pi::Union{Vector{Float64}, Nothing}, XA::Matrix{Int8}, XB::Matrix{Int8}, q::Integer = 21;
                       what::Symbol = :energy)
    what in (:energy, :coupling) || throw(ArgumentError("invalid what value: $what (must be either :energy or :coupling)"))
    split, KA = size(XA); NB, KB = size(XB); N = split + NB; n = N * (q - 1)
    (Pi === nothing && what == :energy) && throw(ArgumentError("what = :energy needs Pi"))
    (size(mJ) == (n, n) && (Pi === nothing || length(Pi) == n)) || throw(ArgumentError("incompatible sizes of mJ, Pi, XA, XB and q"))
    E = Matrix{Float64}(undef, KA, KB)
    Pp = Pi === nothing ? Ptr{Float64}(C_NULL) : pointer(Pi)
    GC.@preserve mJ Pi XA XB E check(ccall((:gdca_pair_energies, libgdca), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Int32, Ptr{Int8}, Int32, Ptr{Int8}, Int32, Int32, Ptr{Float64}),
        ctx(), mJ, Pp, N, q, split, XA, KA, XB, KB, what == :energy ? 1 : 0, E))
    return E
end

# ---- partner matching per species (include/gdca.h, "partner matching per species") ----
# Sequences grouped by species: (perm_a, perm_b, offA, offB, labels) -- labels the sorted union of both sides' integer labels, perm_* the
# stable orders that sort each side by species (1-based), offA / offB the 0-based Int32 offsets (S + 1 each) the library takes
function species_blocks(labels_a::AbstractVector{<:Integer}, labels_b::AbstractVector{<:Integer})
    labels = sort(union(labels_a, labels_b))
    isempty(labels) && throw(ArgumentError("species labels hold no sequence"))
    perm_a = sortperm(labels_a; alg = MergeSort); perm_b = sortperm(labels_b; alg = MergeSort)
    offs(l) = Int32[0; [count(<=(s), l) for s in labels]]
    return perm_a, perm_b, offs(labels_a), offs(labels_b), labels
end

# device pointers (Ptr{Cvoid} into HBM) for the model, the species-sorted sequences and the packed result; offA / offB on the host
function pair_energies_blocked_dev(mJ::Ptr{Cvoid}, Pi::Ptr{Cvoid}, N::Integer, q::Integer, split::Integer, XA::Ptr{Cvoid}, KA::Integer,
                                   XB::Ptr{Cvoid}, KB::Integer, offA::Vector{Int32}, offB::Vector{Int32}, what::Symbol, E::Ptr{Cvoid})
    what in (:energy, :coupling) || throw(ArgumentError("invalid what value: $what (must be either :energy or :coupling)"))
    length(offA) == length(offB) || throw(ArgumentError("offA and offB must have S + 1 entries each"))
    GC.@preserve offA offB check(ccall((:gdca_pair_energies_blocked_dev, libgdca), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32, Int32, Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32,
         Ptr{Cvoid}),
        ctx(), mJ, Pi, N, q, split, XA, KA, XB, KB, pointer(offA), pointer(offB), length(offA) - 1, what == :energy ? 1 : 0, E))
    return E
end

# the minimum-cost assignment inside every block of a packed cost matrix in HBM: match (Int32, offA[end] entries) and gap (Float64, or
# C_NULL) are device pointers
function assign_blocks_dev(E::Ptr{Cvoid}, offA::Vector{Int32}, offB::Vector{Int32}, match::Ptr{Cvoid}, gap::Ptr{Cvoid} = C_NULL)
    length(offA) == length(offB) || throw(ArgumentError("offA and offB must have S + 1 entries each"))
    GC.@preserve offA offB check(ccall((:gdca_assign_blocks_dev, libgdca), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Cvoid}, Ptr{Cvoid}),
        ctx(), E, pointer(offA), pointer(offB), length(offA) - 1, match, gap))
    return match, gap
end

# the fused form on device pointers: Z (N x M), the species-sorted XA / XB (C_NULL: that half of Z's own sequences), E (C_NULL: kept
# inside the context), match and gap in HBM.  Returns the stats.
function run_partner_match_dev(Z::Ptr{Cvoid}, N::Integer, M::Integer, q::Integer, pseudocount::Real, θ, split::Integer, XA::Ptr{Cvoid},
                               KA::Integer, XB::Ptr{Cvoid}, KB::Integer, offA::Vector{Int32}, offB::Vector{Int32}, what::Symbol,
                               E::Ptr{Cvoid}, match::Ptr{Cvoid}, gap::Ptr{Cvoid})
    what in (:energy, :coupling) || throw(ArgumentError("invalid what value: $what (must be either :energy or :coupling)"))
    length(offA) == length(offB) || throw(ArgumentError("offA and offB must have S + 1 entries each"))
    p = Ref(GdcaParams(Float64(pseudocount), theta_arg(θ), 0, 0))
    st = GdcaStats()
    GC.@preserve offA offB begin
        rc = ccall((:gdca_run_partner_match_dev, libgdca), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32, Int32, Ref{GdcaParams}, Int32, Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int32, Ptr{Cvoid},
                    Ptr{Cvoid}, Int32, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{GdcaStats}),
                   ctx(), Z, N, M, q, p, split, XA, KA, XB, KB, pointer(offA), pointer(offB), length(offA) - 1, what == :energy ? 1 : 0,
                   E, match, gap, st)
    end
    check(rc, st.info)
    return st
end

# gDCA's fit, then inside every species the one-to-one matching of the sequences of A (split x K_A) with those of B ((N - split) x K_B)
# at minimum total energy.  species_a / species_b: one integer label per sequence, in any order.  Returns (match, gap) in the caller's
# order: match[a] the 1-based column of seqs_b matched to a (0: unmatched), gap[a] the least other energy of a inside its species
# minus the matched one.
function gDCA_partner_match(filename::AbstractString, split::Integer, seqs_a::Matrix{Int8}, seqs_b::Matrix{Int8},
                            species_a::AbstractVector{<:Integer}, species_b::AbstractVector{<:Integer}; what::Symbol = :energy,
                            pseudocount::Real = 0.8, θ = :auto, max_gap_fraction::Real = 0.9, remove_dups::Bool = false)
    check_arguments(filename, pseudocount, θ, max_gap_fraction, :frob, 1)
    what in (:energy, :coupling) || throw(ArgumentError("invalid what value: $what (must be either :energy or :coupling)"))
    Z = DCAUtils.read_fasta_alignment(filename, max_gap_fraction)
    if remove_dups
        Z, _ = DCAUtils.remove_duplicate_sequences(Z)
    end
    q = Int(maximum(Z))
    q ≥ 32 && error("parameter q=$q is too big (max 31 is allowed)")
    N, M = size(Z)
    1 ≤ split ≤ N - 1 || throw(ArgumentError("invalid split value: $split (must be between 1 and N - 1 = $(N - 1))"))
    (size(seqs_a, 1) == split && size(seqs_b, 1) == N - split) || throw(ArgumentError("seqs_a / seqs_b do not have the sites of protein A / B"))
    KA = size(seqs_a, 2); KB = size(seqs_b, 2)
    (length(species_a) == KA && length(species_b) == KB) || throw(ArgumentError("one species label per sequence is needed"))
    perm_a, perm_b, offA, offB, _ = species_blocks(species_a, species_b)
    XA = seqs_a[:, perm_a]; XB = seqs_b[:, perm_b]
    m = Vector{Int32}(undef, KA); g = Vector{Float64}(undef, KA)
    p = Ref(GdcaParams(Float64(pseudocount), theta_arg(θ), 0, 0))
    st = GdcaStats()
    GC.@preserve Z XA XB offA offB m g begin
        rc = ccall((:gdca_run_partner_match, libgdca), Cint,
                   (Ptr{Cvoid}, Ptr{Int8}, Int32, Int32, Int32, Ref{GdcaParams}, Int32, Ptr{Int8}, Int32, Ptr{Int8}, Int32, Ptr{Cvoid},
                    Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ref{GdcaStats}),
                   ctx(), Z, N, M, q, p, split, XA, KA, XB, KB, pointer(offA), pointer(offB), length(offA) - 1, what == :energy ? 1 : 0,
                   Ptr{Float64}(C_NULL), m, g, st)
    end
    check(rc, st.info)
    st.refined < 0 && @warn "covariance too ill-conditioned for the refinement step and option CHOLESKY=0: matches are unreliable" pseudocount
    match = Vector{Int}(undef, KA); gap = Vector{Float64}(undef, KA)
    for i in 1:KA
        match[perm_a[i]] = m[i] < 0 ? 0 : perm_b[m[i] + 1]
        gap[perm_a[i]] = g[i]
    end
    return match, gap
end

# gDCA's fit (same keywords, minus score and min_separation), then the energies of `sequences` under it: nothing = the alignment's
# own sequences, a Matrix{Int8} (N x K), or the name of a second FASTA file (read with max_gap_fraction = 1: every record kept)
function gDCA_energies(filename::AbstractString; sequences = nothing, pseudocount::Real = 0.8, θ = :auto,
                       max_gap_fraction::Real = 0.9, remove_dups::Bool = false)
    check_arguments(filename, pseudocount, θ, max_gap_fraction, :frob, 1)
    Z = DCAUtils.read_fasta_alignment(filename, max_gap_fraction)
    if remove_dups
        Z, _ = DCAUtils.remove_duplicate_sequences(Z)
    end
    q = Int(maximum(Z))
    q ≥ 32 && error("parameter q=$q is too big (max 31 is allowed)")
    X = sequences isa AbstractString ? DCAUtils.read_fasta_alignment(sequences, 1.0) : sequences
    N, M = size(Z)
    (X === nothing || size(X, 1) == N) || throw(ArgumentError("sequences have $(size(X, 1)) sites, the alignment has $N"))
    K = X === nothing ? M : size(X, 2)
    E = Vector{Float64}(undef, K)
    p = Ref(GdcaParams(Float64(pseudocount), theta_arg(θ), 0, 0))
    st = GdcaStats()
    Xp = X === nothing ? Ptr{Int8}(C_NULL) : pointer(X)
    GC.@preserve Z X E begin
        rc = ccall((:gdca_run_energies, libgdca), Cint,
                   (Ptr{Cvoid}, Ptr{Int8}, Int32, Int32, Int32, Ref{GdcaParams}, Ptr{Int8}, Int32, Ptr{Float64}, Ref{GdcaStats}),
                   ctx(), Z, N, M, q, p, Xp, K, E, st)
    end
    check(rc, st.info)
    st.refined < 0 && @warn "covariance too ill-conditioned for the refinement step and option CHOLESKY=0: energies are unreliable" pseudocount
    return E
end

# gDCA's fit (the keywords of gDCA_energies), then (L, logdet): L[k] = log p(x_k) = -E(x_k) - 1/2 (n log 2 pi + log det C) of
# `sequences` under it -- the density of the Gaussian N(Pi, C) at the one-hot point, on one scale for every model -- and log det C
function gDCA_loglik(filename::AbstractString; sequences = nothing, pseudocount::Real = 0.8, θ = :auto,
                     max_gap_fraction::Real = 0.9, remove_dups::Bool = false)
    check_arguments(filename, pseudocount, θ, max_gap_fraction, :frob, 1)
    Z = DCAUtils.read_fasta_alignment(filename, max_gap_fraction)
    if remove_dups
        Z, _ = DCAUtils.remove_duplicate_sequences(Z)
    end
    q = Int(maximum(Z))
    q ≥ 32 && error("parameter q=$q is too big (max 31 is allowed)")
    X = sequences isa AbstractString ? DCAUtils.read_fasta_alignment(sequences, 1.0) : sequences
    N, M = size(Z)
    (X === nothing || size(X, 1) == N) || throw(ArgumentError("sequences have $(size(X, 1)) sites, the alignment has $N"))
    K = X === nothing ? M : size(X, 2)
    L = Vector{Float64}(undef, K)
    logdet = Ref{Float64}(NaN)
    p = Ref(GdcaParams(Float64(pseudocount), theta_arg(θ), 0, 0))
    st = GdcaStats()
    Xp = X === nothing ? Ptr{Int8}(C_NULL) : pointer(X)
    GC.@preserve Z X L begin
        rc = ccall((:gdca_run_loglik, libgdca), Cint,
                   (Ptr{Cvoid}, Ptr{Int8}, Int32, Int32, Int32, Ref{GdcaParams}, Ptr{Int8}, Int32, Ptr{Float64}, Ref{Float64}, Ref{GdcaStats}),
                   ctx(), Z, N, M, q, p, Xp, K, L, logdet, st)
    end
    check(rc, st.info)
    st.refined < 0 && @warn "covariance too ill-conditioned for the refinement step and option CHOLESKY=0: log-likelihoods are unreliable" pseudocount
    return L, logdet[]
end

# D[b, i, k] for every single substitution of the K columns of X (N x K like Z) under the model (include/gdca.h, "mutation scan"):
# what = :delta, the energy change of setting site i of sequence k to symbol b (exactly 0 at the sequence's own symbol; b = q deletes
# the residue), or :potential, the site potentials V the changes are differences of.  A q x N x K array.
function mutation_scan(mJ::Matrix{Float64}, Pi::Vector{Float64}, X::Matrix{Int8}, q::Integer = 21; what::Symbol = :delta)
    what in (:delta, :potential) || throw(ArgumentError("invalid what value: $what (must be either :delta or :potential)"))
    N, K = size(X); n = N * (q - 1)
    (size(mJ) == (n, n) && length(Pi) == n) || throw(ArgumentError("incompatible sizes of mJ, Pi, X and q"))
    D = Array{Float64, 3}(undef, q, N, K)
    GC.@preserve mJ Pi X D check(ccall((:gdca_mutation_scan, libgdca), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Ptr{Int8}, Int32, Int32, Ptr{Float64}),
        ctx(), mJ, Pi, N, q, X, K, what == :potential ? 1 : 0, D))
    return D
end

# gDCA's fit (same keywords as gDCA_energies), then the scan of `sequences` under it: nothing = the alignment's own sequences, a
# Matrix{Int8} (N x K), or the name of a second FASTA file (read with max_gap_fraction = 1: every record kept)
function gDCA_mutation_scan(filename::AbstractString; sequences = nothing, what::Symbol = :delta, pseudocount::Real = 0.8, θ = :auto,
                            max_gap_fraction::Real = 0.9, remove_dups::Bool = false)
    check_arguments(filename, pseudocount, θ, max_gap_fraction, :frob, 1)
    what in (:delta, :potential) || throw(ArgumentError("invalid what value: $what (must be either :delta or :potential)"))
    Z = DCAUtils.read_fasta_alignment(filename, max_gap_fraction)
    if remove_dups
        Z, _ = DCAUtils.remove_duplicate_sequences(Z)
    end
    q = Int(maximum(Z))
    q ≥ 32 && error("parameter q=$q is too big (max 31 is allowed)")
    X = sequences isa AbstractString ? DCAUtils.read_fasta_alignment(sequences, 1.0) : sequences
    (X === nothing || X isa Matrix{Int8}) || throw(ArgumentError("sequences must be a Matrix{Int8} of symbols 1..q, a FASTA file name or nothing"))
    N, M = size(Z)
    (X === nothing || size(X, 1) == N) || throw(ArgumentError("sequences have $(size(X, 1)) sites, the alignment has $N"))
    K = X === nothing ? M : size(X, 2)
    D = Array{Float64, 3}(undef, q, N, K)
    p = Ref(GdcaParams(Float64(pseudocount), theta_arg(θ), 0, 0))
    st = GdcaStats()
    Xp = X === nothing ? Ptr{Int8}(C_NULL) : pointer(X)
    GC.@preserve Z X D begin
        rc = ccall((:gdca_run_mutation_scan, libgdca), Cint,
                   (Ptr{Cvoid}, Ptr{Int8}, Int32, Int32, Int32, Ref{GdcaParams}, Ptr{Int8}, Int32, Int32, Ptr{Float64}, Ref{GdcaStats}),
                   ctx(), Z, N, M, q, p, Xp, K, what == :potential ? 1 : 0, D, st)
    end
    check(rc, st.info)
    st.refined < 0 && @warn "covariance too ill-conditioned for the refinement step and option CHOLESKY=0: energy changes are unreliable" pseudocount
    return D
end

# The double-mutant landscape of the K columns of X under the model (include/gdca.h, "double-mutant scan"), an entry a site pair:
# (ddE_min, sub_i, sub_j, epistasis), each N x N x K and indexed [i, j, k] -- the lowest energy change over the true double
# substitutions of sites i and j (the gap q is a target), the symbols it puts at i and at j (0 on the diagonal), and the pair's
# epistasis strength sqrt(sum eps^2) in that sequence.  No mutant is written down.
function decode_double_code(code::Array{Int32, 3}, q::Integer)
    sub_i = map(c -> c < 0 ? Int8(0) : Int8(c % q + 1), code)
    sub_j = map(c -> c < 0 ? Int8(0) : Int8(c ÷ q + 1), code)
    return sub_i, sub_j
end

function double_mutant_scan(mJ::Matrix{Float64}, Pi::Vector{Float64}, X::Matrix{Int8}, q::Integer = 21)
    N, K = size(X); n = N * (q - 1)
    (N ≥ 2 && size(mJ) == (n, n) && length(Pi) == n) || throw(ArgumentError("incompatible sizes of mJ, Pi, X and q"))
    Emin = Array{Float64, 3}(undef, N, N, K); code = Array{Int32, 3}(undef, N, N, K); epi = Array{Float64, 3}(undef, N, N, K)
    GC.@preserve mJ Pi X Emin code epi check(ccall((:gdca_double_mutant_scan, libgdca), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Ptr{Int8}, Int32, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}),
        ctx(), mJ, Pi, N, q, X, K, Emin, code, epi))
    sub_i, sub_j = decode_double_code(code, q)
    return Emin, sub_i, sub_j, epi
end

# records (k, i, b, j, c) as a 5 x L integer matrix, k and the sites 1-based as everything in Julia -> the library's 0-based int32
function double_mutant_records(muts::AbstractMatrix{<:Integer})
    size(muts, 1) == 5 || throw(ArgumentError("mutations must be a 5 x L matrix of records (k, i, b, j, c)"))
    size(muts, 2) ≥ 1 || throw(ArgumentError("mutations holds no record"))
    m = Matrix{Int32}(muts)
    m[1, :] .-= Int32(1); m[2, :] .-= Int32(1); m[4, :] .-= Int32(1)
    return m
end

# The energy change of the listed double mutants: column l of muts = (k, i, b, j, c) -- sequence k (a column of X), sites i != j,
# the symbols b (put at i) and c (put at j) in 1..q.  L entries; which substitution is named first does not matter.
function double_mutant_energies(mJ::Matrix{Float64}, Pi::Vector{Float64}, X::Matrix{Int8}, muts::AbstractMatrix{<:Integer}, q::Integer = 21)
    N, K = size(X); n = N * (q - 1)
    (N ≥ 2 && size(mJ) == (n, n) && length(Pi) == n) || throw(ArgumentError("incompatible sizes of mJ, Pi, X and q"))
    m = double_mutant_records(muts); L = size(m, 2)
    out = Vector{Float64}(undef, L)
    GC.@preserve mJ Pi X m out check(ccall((:gdca_double_mutants, libgdca), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Ptr{Int8}, Int32, Ptr{Cvoid}, Int32, Ptr{Float64}),
        ctx(), mJ, Pi, N, q, X, K, m, L, out))
    return out
end

# what the two fused double-mutant entries share: gDCA's reading of the alignment and of `sequences` (required: a Matrix{Int8}, N x K,
# or the name of a FASTA file read with max_gap_fraction = 1)
function double_mutant_inputs(filename, sequences, pseudocount, θ, max_gap_fraction, remove_dups)
    check_arguments(filename, pseudocount, θ, max_gap_fraction, :frob, 1)
    Z = DCAUtils.read_fasta_alignment(filename, max_gap_fraction)
    if remove_dups
        Z, _ = DCAUtils.remove_duplicate_sequences(Z)
    end
    q = Int(maximum(Z))
    q ≥ 32 && error("parameter q=$q is too big (max 31 is allowed)")
    X = sequences isa AbstractString ? DCAUtils.read_fasta_alignment(sequences, 1.0) : sequences
    X isa Matrix{Int8} || throw(ArgumentError("sequences must be a Matrix{Int8} of symbols 1..q or a FASTA file name"))
    size(X, 1) == size(Z, 1) || throw(ArgumentError("sequences have $(size(X, 1)) sites, the alignment has $(size(Z, 1))"))
    return Z, X, q
end

function gDCA_double_mutant_scan(filename::AbstractString, sequences; pseudocount::Real = 0.8, θ = :auto, max_gap_fraction::Real = 0.9,
                                 remove_dups::Bool = false)
    Z, X, q = double_mutant_inputs(filename, sequences, pseudocount, θ, max_gap_fraction, remove_dups)
    N, M = size(Z); K = size(X, 2)
    Emin = Array{Float64, 3}(undef, N, N, K); code = Array{Int32, 3}(undef, N, N, K); epi = Array{Float64, 3}(undef, N, N, K)
    p = Ref(GdcaParams(Float64(pseudocount), theta_arg(θ), 0, 0))
    st = GdcaStats()
    GC.@preserve Z X Emin code epi begin
        rc = ccall((:gdca_run_double_mutant_scan, libgdca), Cint,
                   (Ptr{Cvoid}, Ptr{Int8}, Int32, Int32, Int32, Ref{GdcaParams}, Ptr{Int8}, Int32, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ref{GdcaStats}),
                   ctx(), Z, N, M, q, p, X, K, Emin, code, epi, st)
    end
    check(rc, st.info)
    st.refined < 0 && @warn "covariance too ill-conditioned for the refinement step and option CHOLESKY=0: energy changes are unreliable" pseudocount
    sub_i, sub_j = decode_double_code(code, q)
    return Emin, sub_i, sub_j, epi
end

function gDCA_double_mutants(filename::AbstractString, sequences, mutations::AbstractMatrix{<:Integer}; pseudocount::Real = 0.8, θ = :auto,
                             max_gap_fraction::Real = 0.9, remove_dups::Bool = false)
    Z, X, q = double_mutant_inputs(filename, sequences, pseudocount, θ, max_gap_fraction, remove_dups)
    N, M = size(Z); K = size(X, 2)
    m = double_mutant_records(mutations); L = size(m, 2)
    out = Vector{Float64}(undef, L)
    p = Ref(GdcaParams(Float64(pseudocount), theta_arg(θ), 0, 0))
    st = GdcaStats()
    GC.@preserve Z X m out begin
        rc = ccall((:gdca_run_double_mutants, libgdca), Cint,
                   (Ptr{Cvoid}, Ptr{Int8}, Int32, Int32, Int32, Ref{GdcaParams}, Ptr{Int8}, Int32, Ptr{Cvoid}, Int32, Ptr{Float64}, Ref{GdcaStats}),
                   ctx(), Z, N, M, q, p, X, K, m, L, out, st)
    end
    check(rc, st.info)
    st.refined < 0 && @warn "covariance too ill-conditioned for the refinement step and option CHOLESKY=0: energy changes are unreliable" pseudocount
    return out
end

function compute_DI_gauss(mJ::Matrix{Float64}, C::Matrix{Float64}, q::Integer = 21)
    N = size(mJ, 1) ÷ (q - 1); S = Matrix{Float64}(undef, N, N)
    GC.@preserve mJ C S check(ccall((:gdca_di, libgdca), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Ptr{Float64}), ctx(), mJ, C, N, q, S))
    return S
end

# ---- device-resident form of the reference's statement-by-statement pipeline ---------------------------------
# src/GaussDCA.jl:28-42 kept as six statements, every array in HBM (gdca_dbuf handles; `_dev` entry points of
# include/gdca.h): only Z goes in and S comes out over PCIe.
mutable struct DBuf
    h::Ptr{Cvoid}
    function DBuf(bytes::Integer)
        r = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:gdca_dbuf_alloc, libgdca), Cint, (Ptr{Cvoid}, UInt64, Ref{Ptr{Cvoid}}), ctx(), bytes, r))
        b = new(r[])
        finalizer(x -> ccall((:gdca_dbuf_free, libgdca), Cint, (Ptr{Cvoid},), x.h), b)
        return b
    end
end
dptr(b::DBuf) = ccall((:gdca_dbuf_ptr, libgdca), Ptr{Cvoid}, (Ptr{Cvoid},), b.h)
upload!(b::DBuf, a::Array) = GC.@preserve a check(ccall((:gdca_dbuf_upload, libgdca), Cint,
    (Ptr{Cvoid}, Ptr{Cvoid}, UInt64, Ptr{Cvoid}, UInt64), ctx(), b.h, 0, a, sizeof(a)))
download!(a::Array, b::DBuf) = GC.@preserve a check(ccall((:gdca_dbuf_download, libgdca), Cint,
    (Ptr{Cvoid}, Ptr{Cvoid}, UInt64, Ptr{Cvoid}, UInt64), ctx(), b.h, 0, a, sizeof(a)))

function gDCA_stepwise(Z::Matrix{Int8}; pseudocount::Real = 0.8, θ = :auto, score::Symbol = :frob,
                       min_separation::Integer = 5)
    N, M = size(Z); q = Int(maximum(Z)); n = N * (q - 1)
    q ≥ 32 && error("parameter q=$q is too big (max 31 is allowed)")
    dZ = DBuf(N * M); upload!(dZ, Z)
    dW = DBuf(8M); dPi = DBuf(8n); dPij = DBuf(8n * n); dS = DBuf(8N * N)
    Meff = Ref{Cdouble}(0); th = Ref{Cdouble}(0); thr = Ref{Int32}(0); info = Ref{Int32}(0)
    c = ctx()
    # Pi_true, Pij_true, Meff, _ = compute_weighted_frequencies(Z, q, θ)                          (:28)
    check(ccall((:gdca_compute_weights_dev, libgdca), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32, Cdouble, Ptr{Cvoid}, Ref{Cdouble}, Ref{Cdouble}, Ref{Int32}),
        c, dptr(dZ), N, M, theta_arg(θ), dptr(dW), Meff, th, thr))
    check(ccall((:gdca_frequencies_dev, libgdca), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32, Int32, Ptr{Cvoid}, Cdouble, Ptr{Cvoid}, Ptr{Cvoid}),
        c, dptr(dZ), N, M, q, dptr(dW), Meff[], dptr(dPi), dptr(dPij)))
    # Pi, Pij = add_pseudocount(Pi_true, Pij_true, Float64(pseudocount), q)   (in place)          (:30)
    check(ccall((:gdca_add_pseudocount_dev, libgdca), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32, Cdouble, Ptr{Cvoid}, Ptr{Cvoid}),
        c, dptr(dPi), dptr(dPij), N, q, Float64(pseudocount), dptr(dPi), dptr(dPij)))
    # C = compute_C(Pi, Pij)                                                                       (:32)
    dC = DBuf(8n * n)
    check(ccall((:gdca_covariance_dev, libgdca), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Cvoid}),
        c, dptr(dPi), dptr(dPij), n, dptr(dC)))
    # mJ = inv(cholesky(C))        (dPij is reused for mJ; C itself is kept for compute_DI_gauss)  (:34)
    check(ccall((:gdca_covariance_dev, libgdca), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Cvoid}),
        c, dptr(dPi), dptr(dPij), n, dptr(dPij)))
    rc = ccall((:gdca_spd_inverse_dev, libgdca), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ref{Int32}), c, dptr(dPij), n, info)
    check(rc, info[])
    # S = score == :DI ? compute_DI_gauss(mJ, C, q) : compute_FN(mJ, q)                            (:36-40)
    if score == :DI
        check(ccall((:gdca_di_dev, libgdca), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32, Ptr{Cvoid}),
            c, dptr(dPij), dptr(dC), N, q, dptr(dS)))
    else
        check(ccall((:gdca_fn_dev, libgdca), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32, Ptr{Cvoid}),
            c, dptr(dPij), N, q, dptr(dS)))
    end
    # S = correct_APC(S)                                                                           (:42)
    check(ccall((:gdca_apc_dev, libgdca), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32), c, dptr(dS), N))
    S = Matrix{Float64}(undef, N, N); download!(S, dS)
    return compute_ranking(S, min_separation)                                                    # :44
end

end # module
