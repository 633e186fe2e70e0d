# SPXShim.jl -- the reference-side binding a ShiftedProximalOperators.jl maintainer would add
# (e.g. as a package extension `ext/ShiftedProximalOperatorsSPXExt.jl` loaded when AMDGPU.jl is present).
#
# NOT EXECUTED IN THIS REPOSITORY'S PIPELINE: no Julia toolchain exists in the build image or on the GPU
# box.  It is the `ccall` counterpart of shiftedproximaloperators.jl_amd/_lib.py + shifted.py, which bind
# exactly the same C symbols (include/spx.h) and ARE exercised by tests/ on the MI355X.
#
# Idea: the reference's struct fields are type parameters `<: AbstractVector{R}` (src/shiftedNormL1Box.jl:3-21),
# so `shifted(h, xk::ROCVector{Float64}, ...)` already builds a ψ whose xk/sj/sol live in HBM -- the
# constructors need no change.  What cannot run on device arrays is the body of prox! (scalar-indexing loops).
# This file adds prox! methods that dispatch on ψ with ROCArray storage and forward to libspx.

module SPXShim

using ShiftedProximalOperators
using ShiftedProximalOperators:
  ShiftedNormL1, ShiftedNormL0, ShiftedRootNormLhalf, ShiftedNormL1Box, ShiftedNormL0Box,
  ShiftedRootNormLhalfBox, ShiftedIndBallL0, ShiftedIndBallL0BInf, ShiftedGroupNormL2, ShiftedGroupNormL2Binf
import ShiftedProximalOperators: prox!, iprox!
using AMDGPU  # ROCArray, AMDGPU.stream(), AMDGPU.device_id

const libspx = get(ENV, "LIBSPX", "libspx.so")
# Device vectors the C ABI takes as they are: a ROCVector, or a UNIT-STRIDE view of one (`view(x, 2:n)`: the reference builds
# operators on views, test/runtests.jl:196-209).  `pointer(v)` of such a view is the base pointer advanced by the offset
# (round 3: by pointer arithmetic, no copy, no CPU fallback); libspx handles vectors that start at any element (8-byte
# aligned: the kernels peel to the 16-byte boundary or take 8-byte accesses).  Strided views (`1:2:10`) still fall through to
# the reference's own method.
const DVec = Union{ROCVector{Float64}, SubArray{Float64, 1, <:ROCVector{Float64}, <:Tuple{AbstractUnitRange}, true}}

# ---------------------------------------------------------------------------------------------
# context: one per (device, HIP stream); enqueue on AMDGPU.jl's current stream so prox! is ordered with
# the solver's own broadcasts (R2 does `mν∇fk .= -ν .* ∇fk; prox!(s, ψ, mν∇fk, ν)`).
# ---------------------------------------------------------------------------------------------
const CTX = Dict{Tuple{Int, Ptr{Cvoid}}, Ptr{Cvoid}}()

# Status 7 (SPX_ERR_INTERNAL) is the device side reporting a failure of an EARLIER asynchronous call on this context (a kernel
# that synchronises inside one launch gave up waiting: another process or a graph replay held the CUs) -- libspx raises it on
# the next call, whichever it is; the results since then are NaN.  `ccall((:spx_sync, libspx), Cint, (Ptr{Cvoid},), ctx())`
# acknowledges it and resets the context.
function check(status::Cint)
  status == 0 && return
  msg = unsafe_string(ccall((:spx_last_error, libspx), Cstring, ()))
  error("libspx status $status: $msg")
end

function ctx()
  dev = AMDGPU.device_id(AMDGPU.device()) - 1
  st = Ptr{Cvoid}(UInt(AMDGPU.stream().stream))      # hipStream_t of the task-local stream
  get!(CTX, (dev, st)) do
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:spx_ctx_create_on_stream, libspx), Cint, (Cint, Ptr{Cvoid}, Ptr{Ptr{Cvoid}}), dev, st, h))
    h[]
  end
end

dptr(v::DVec) = Ptr{Cdouble}(UInt(pointer(v)))
dptr(::Nothing) = Ptr{Cdouble}(C_NULL)
vec_or_nothing(b) = b isa Real ? nothing : b            # `isa(ψ.l, Real) ? ψ.l : ψ.l[i]`
scal(b) = b isa Real ? Float64(b) : 0.0
mptr(m) = m === nothing ? Ptr{UInt8}(C_NULL) : Ptr{UInt8}(UInt(pointer(m)))   # device byte mask or NULL
function with_value(f)                                   # entry points that return a scalar through a double*
  out = Ref{Cdouble}(0.0)
  check(f(out))
  out[]
end

# ---------------------------------------------------------------------------------------------
# separable, unboxed          src/shiftedNormL1.jl:40-54, shiftedNormL0.jl:38-55, shiftedRootNormLhalf.jl:41-63
# ---------------------------------------------------------------------------------------------
for (T, sym) in ((:ShiftedNormL1, :spx_prox_l1), (:ShiftedNormL0, :spx_prox_l0),
                 (:ShiftedRootNormLhalf, :spx_prox_lhalf))
  @eval function prox!(y::DVec, ψ::$T{Float64, <:DVec, <:DVec, <:DVec}, q::DVec, σ::Float64)
    n = length(ψ.xk)
    (length(y) == n && length(q) == n) || throw(BoundsError())
    check(ccall(($(QuoteNode(sym)), libspx), Cint,
                (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Cdouble, Cdouble),
                ctx(), dptr(y), dptr(q), dptr(ψ.xk), dptr(ψ.sj), n, ψ.λ, σ))
    return y
  end
end

# ---------------------------------------------------------------------------------------------
# separable, boxed            src/shiftedNormL1Box.jl:89-125, shiftedNormL0Box.jl:89-131,
#                             shiftedRootNormLhalfBox.jl:86-120
# `selected` (any AbstractArray{<:Integer}, 1-based) -> device byte mask, built once per ψ and cached;
# the default 1:length(xk) needs no mask.
# ---------------------------------------------------------------------------------------------
const MASKS = IdDict{Any, Any}()   # ψ.selected (shared by a twice-shifted ψ) => ROCVector{UInt8} | nothing

function mask_for(ψ)
  n = length(ψ.xk)
  sel = ψ.selected
  (sel isa AbstractUnitRange && first(sel) <= 1 && last(sel) >= n) && return nothing
  get!(MASKS, sel) do
    idx0 = ROCVector{Int64}(collect(Int64, sel) .- 1)            # 0-based for the C ABI
    m = ROCVector{UInt8}(undef, n)
    check(ccall((:spx_build_mask, libspx), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Int64, Ptr{Int64}, Int64),
                ctx(), Ptr{UInt8}(UInt(pointer(m))), n, Ptr{Int64}(UInt(pointer(idx0))), length(idx0)))
    AMDGPU.synchronize()                                         # idx0 may be freed after this
    m
  end
end

for (T, sym) in ((:ShiftedNormL1Box, :spx_prox_l1_box), (:ShiftedNormL0Box, :spx_prox_l0_box),
                 (:ShiftedRootNormLhalfBox, :spx_prox_lhalf_box))
  @eval function prox!(y::DVec, ψ::$T{Float64, <:DVec, <:DVec, <:DVec}, q::DVec, σ::Float64)
    n = length(ψ.xk)
    (length(y) == n && length(q) == n) || throw(BoundsError())
    (ψ.l isa Real || ψ.l isa DVec) && (ψ.u isa Real || ψ.u isa DVec) ||
      return invoke(prox!, Tuple{AbstractVector{Float64}, $T{Float64}, AbstractVector{Float64}, Float64}, y, ψ, q, σ)
    m = mask_for(ψ)
    check(ccall(($(QuoteNode(sym)), libspx), Cint,
                (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Cdouble, Cdouble,
                 Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Cdouble, Ptr{UInt8}),
                ctx(), dptr(y), dptr(q), dptr(ψ.xk), dptr(ψ.sj), n, ψ.λ, σ,
                dptr(vec_or_nothing(ψ.l)), dptr(vec_or_nothing(ψ.u)), scal(ψ.l), scal(ψ.u),
                mptr(m)))
    return y
  end
end

# ---------------------------------------------------------------------------------------------
# iprox!                      src/shiftedNormL1.jl:60-75, shiftedNormL0.jl:61-80, shiftedNormL1Box.jl:131-225,
#                             shiftedNormL0Box.jl:137-231
# ---------------------------------------------------------------------------------------------
for (T, sym) in ((:ShiftedNormL1, :spx_iprox_l1), (:ShiftedNormL0, :spx_iprox_l0))
  @eval function iprox!(y::DVec, ψ::$T{Float64, <:DVec, <:DVec, <:DVec}, g::DVec, d::DVec)
    n = length(ψ.xk)
    st = ccall(($(QuoteNode(sym)), libspx), Cint,
               (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Cdouble, Cint),
               ctx(), dptr(y), dptr(g), dptr(d), dptr(ψ.xk), dptr(ψ.sj), n, ψ.λ, 1)
    st == 6 && throw(AssertionError("d[i] > 0"))   # SPX_ERR_ASSERT
    check(st)
    return y
  end
end
for (T, sym) in ((:ShiftedNormL1Box, :spx_iprox_l1_box), (:ShiftedNormL0Box, :spx_iprox_l0_box))
  @eval function iprox!(y::DVec, ψ::$T{Float64, <:DVec, <:DVec, <:DVec}, g::DVec, d::DVec)
    n = length(ψ.xk)
    m = mask_for(ψ)
    check(ccall(($(QuoteNode(sym)), libspx), Cint,
                (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Cdouble,
                 Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Cdouble, Ptr{UInt8}),
                ctx(), dptr(y), dptr(g), dptr(d), dptr(ψ.xk), dptr(ψ.sj), n, ψ.λ,
                dptr(vec_or_nothing(ψ.l)), dptr(vec_or_nothing(ψ.u)), scal(ψ.l), scal(ψ.u),
                mptr(m)))
    return y
  end
end

# ---------------------------------------------------------------------------------------------
# top-r                       src/shiftedIndBallL0.jl:54-72, shiftedIndBallL0BInf.jl:73-95
# (ψ.p, the Vector{Int} permutation scratch, is not used: libspx selects, it does not sort)
# ---------------------------------------------------------------------------------------------
function prox!(y::DVec, ψ::ShiftedIndBallL0{<:Integer, Float64, <:DVec, <:DVec, <:DVec}, q::DVec, σ::Float64)
  n = length(ψ.xk)
  check(ccall((:spx_prox_indball_l0, libspx), Cint,
              (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Int64),
              ctx(), dptr(y), dptr(q), dptr(ψ.xk), dptr(ψ.sj), n, ψ.r))
  return y
end

function prox!(y::DVec, ψ::ShiftedIndBallL0BInf{<:Integer, Float64, <:DVec, <:DVec, <:DVec}, q::DVec, σ::Float64)
  n = length(ψ.xk)
  check(ccall((:spx_prox_indball_l0_binf, libspx), Cint,
              (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Int64, Cdouble),
              ctx(), dptr(y), dptr(q), dptr(ψ.xk), dptr(ψ.sj), n, ψ.r, ψ.Δ))
  return y
end

# ---------------------------------------------------------------------------------------------
# the unshifted value types the reference defines itself: prox!(y, h, x, γ) and h(x) on device arrays
#   RootNormLhalf  src/rootNormLhalf.jl:27-51   (returns h(y)),   GroupNormL2  src/groupNormL2.jl:33-58
# They run the shifted kernels with xk = sj = 0 (q + (0 + 0) = q and y - (0 + 0) = y are exact).
# ---------------------------------------------------------------------------------------------
const ZEROS = Dict{Int, ROCVector{Float64}}()
zeros_for(n) = get!(() -> AMDGPU.zeros(Float64, n), ZEROS, n)

function prox!(y::DVec, f::ShiftedProximalOperators.RootNormLhalf{Float64}, x::DVec, γ::Real = 1.0)
  n = length(x); z = zeros_for(n); out = Ref{Cdouble}(0.0)
  check(ccall((:spx_proxval_lhalf, libspx), Cint,
              (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Cdouble, Cdouble, Cdouble, Ptr{Cdouble}),
              ctx(), dptr(y), dptr(x), dptr(z), dptr(z), n, f.lambda, Float64(γ), 1.0, out))
  return out[]                                                   # λ Σ sqrt|y_i|, as :50
end
function (f::ShiftedProximalOperators.RootNormLhalf{Float64})(x::DVec)
  z = zeros_for(length(x))
  with_value() do out
    ccall((:spx_obj_lhalf, libspx), Cint,
          (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Cdouble, Ptr{Cdouble}),
          ctx(), dptr(x), dptr(z), dptr(z), length(x), f.lambda, out)
  end
end
# GroupNormL2: prox!(y, f, x, γ) = group_call on ψ = shifted(f, zeros) with q = x; its return value Σ λ_g ‖x_g‖ is
# spx_obj_group_l2 of the input (layout_for(f, n) supplies offsets / gather indices / weights, as in group_call).

# ---------------------------------------------------------------------------------------------
# prox! fused with h at the result (no counterpart in the reference; what R2 does in two steps:
# `prox!(s, ψ, mν∇fk, ν)` then `hkn = ψ(s)`): one pass over the vectors instead of two.  Headline operator shown;
# spx_proxval_l1 / l0 / lhalf / l0_box / lhalf_box follow the same pattern.
# ---------------------------------------------------------------------------------------------
function prox_value!(y::DVec, ψ::ShiftedNormL1Box{Float64, <:DVec, <:DVec, <:DVec}, q::DVec, σ::Float64;
                     q_scale::Float64 = 1.0)   # prox at q_scale .* q (R2: q = ∇fk, q_scale = -ν)
  n = length(ψ.xk)
  (length(y) == n && length(q) == n) || throw(BoundsError())
  m = mask_for(ψ)
  out = Ref{Cdouble}(0.0)
  check(ccall((:spx_proxval_l1_box, libspx), Cint,
              (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Cdouble, Cdouble,
               Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Cdouble, Ptr{UInt8}, Cdouble, Ptr{Cdouble}),
              ctx(), dptr(y), dptr(q), dptr(ψ.xk), dptr(ψ.sj), n, ψ.λ, σ,
              dptr(vec_or_nothing(ψ.l)), dptr(vec_or_nothing(ψ.u)), scal(ψ.l), scal(ψ.u),
              mptr(m), q_scale, out))
  return y, out[]
end

# ---------------------------------------------------------------------------------------------
# prox! fused with the step statistics of an iteration (spx_proxstep_*; no counterpart in the reference: what R2 / TR do
# around the prox -- `ψ(s)`, `dot(∇fk, s)`, `xk + s`, `norm(s)` -- in the pass that stores s).  Returns (y, h, qy, yy):
#   h  = λ Σ over the selected indices of Term((xk + sj) + y)      (the value prox_value! returns)
#   qy = Σ over all i of q[i] y[i], with the q that was passed, not q_scale .* q       yy = Σ over all i of y[i]^2
# xkn (a device vector that is none of y, q, ψ.xk, ψ.sj, l, u; or nothing) receives (xk + sj) + y.
# `out` = a ROCVector{Float64} of at least 3 elements: the three sums stay on the device, nothing is read back and the
# call does not synchronise; returns (y, out).  y must not be q.  Float64 device vectors; the group operators' methods
# (spx_proxstep_group_l2[_binf]) sit with their layout helpers further down.
# Headline operator and the unboxed ℓ1 norm shown; spx_proxstep_l0 / lhalf / l0_box / lhalf_box follow the same pattern.
# ---------------------------------------------------------------------------------------------
function prox_step!(y::DVec, ψ::ShiftedNormL1Box{Float64, <:DVec, <:DVec, <:DVec}, q::DVec, σ::Float64;
                    q_scale::Float64 = 1.0, xkn::Union{Nothing, DVec} = nothing, out::Union{Nothing, DVec} = nothing)
  n = length(ψ.xk)
  (length(y) == n && length(q) == n && (xkn === nothing || length(xkn) == n)) || throw(BoundsError())
  (out === nothing || length(out) >= 3) || throw(ArgumentError("out needs at least 3 elements"))
  m = mask_for(ψ)
  stats = zeros(Cdouble, 3)
  check(ccall((:spx_proxstep_l1_box, libspx), Cint,
              (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Cdouble, Cdouble,
               Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Cdouble, Ptr{UInt8}, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
              ctx(), dptr(y), dptr(q), dptr(ψ.xk), dptr(ψ.sj), n, ψ.λ, σ,
              dptr(vec_or_nothing(ψ.l)), dptr(vec_or_nothing(ψ.u)), scal(ψ.l), scal(ψ.u),
              mptr(m), q_scale, dptr(xkn), out === nothing ? pointer(stats) : Ptr{Cdouble}(C_NULL), dptr(out)))
  return out === nothing ? (y, stats[1], stats[2], stats[3]) : (y, out)
end
function prox_step!(y::DVec, ψ::ShiftedNormL1{Float64, <:DVec, <:DVec, <:DVec}, q::DVec, σ::Float64;
                    q_scale::Float64 = 1.0, xkn::Union{Nothing, DVec} = nothing, out::Union{Nothing, DVec} = nothing)
  n = length(ψ.xk)
  (length(y) == n && length(q) == n && (xkn === nothing || length(xkn) == n)) || throw(BoundsError())
  (out === nothing || length(out) >= 3) || throw(ArgumentError("out needs at least 3 elements"))
  stats = zeros(Cdouble, 3)
  check(ccall((:spx_proxstep_l1, libspx), Cint,
              (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Cdouble, Cdouble, Cdouble,
               Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
              ctx(), dptr(y), dptr(q), dptr(ψ.xk), dptr(ψ.sj), n, ψ.λ, σ, q_scale,
              dptr(xkn), out === nothing ? pointer(stats) : Ptr{Cdouble}(C_NULL), dptr(out)))
  return out === nothing ? (y, stats[1], stats[2], stats[3]) : (y, out)
end

# ---------------------------------------------------------------------------------------------
# The same for `batch` problems in ONE call, every per-problem scalar read from DEVICE memory (spx_proxstep_{l1,l0}[_box]_batch;
# no counterpart in the reference): a regularisation path, folds, multi-start, one trust region per problem.  Problem b is
# column b of the n × batch device matrices Y, Q, XK, SJ (and xkn): Julia's column-major layout with leading dimension
# ld = stride(Y, 2) >= n is the library's row layout.  λ, σ, q_scale (and l, u: one scalar per problem, l = -Δ, u = Δ for a
# trust region) are ROCVector{Float64} of length batch: the kernel reads them, nothing is read back, and a captured call
# follows the values a solver leaves there (R2's ν update stays on the device).  `selected`: ONE byte mask of length n shared
# by the problems, or nothing.  out: a 3 × batch device matrix; out[:, b] = (h, qy, yy) of problem b as prox_step! returns
# them.  kind = :l1 or :l0; the box form is taken when l and u are given.  Returns (Y, out); never synchronises.
# ---------------------------------------------------------------------------------------------
const DMat = ROCMatrix{Float64}
const libspx_batch = get(ENV, "LIBSPX_BATCH", "libspx_batch.so")   # include/spx_batch.h: a library of its own, linked against libspx
dptr(v::DMat) = Ptr{Cdouble}(UInt(pointer(v)))
for kind in (:l1, :l0)   # (ccall wants its symbol as a literal: one method per operator)
  plain, boxed = QuoteNode(Symbol(:spx_proxstep_, kind, :_batch)), QuoteNode(Symbol(:spx_proxstep_, kind, :_box_batch))
  @eval proxstep_batch_call(::Val{$(QuoteNode(kind))}, Y, Q, XK, SJ, n, batch, ld, λ, σ, q_scale, xkn, out) =
    ccall(($plain, libspx_batch), Cint,
          (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Int64, Int64,
           Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
          ctx(), dptr(Y), dptr(Q), dptr(XK), dptr(SJ), n, batch, ld, dptr(λ), dptr(σ), dptr(q_scale), dptr(xkn), dptr(out))
  @eval proxstep_batch_call(::Val{$(QuoteNode(kind))}, Y, Q, XK, SJ, n, batch, ld, λ, σ, l, u, selected, q_scale, xkn, out) =
    ccall(($boxed, libspx_batch), Cint,
          (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Int64, Int64,
           Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{UInt8}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
          ctx(), dptr(Y), dptr(Q), dptr(XK), dptr(SJ), n, batch, ld, dptr(λ), dptr(σ), dptr(l), dptr(u), mptr(selected),
          dptr(q_scale), dptr(xkn), dptr(out))
end
function prox_step_batch!(Y::DMat, kind::Symbol, Q::DMat, XK::DMat, SJ::DMat, λ::DVec, σ::DVec, q_scale::DVec;
                          l::Union{Nothing, DVec} = nothing, u::Union{Nothing, DVec} = nothing,
                          selected::Union{Nothing, ROCVector{UInt8}} = nothing, xkn::Union{Nothing, DMat} = nothing,
                          out::DMat = ROCMatrix{Float64}(undef, 3, size(Y, 2)))
  kind in (:l1, :l0) || throw(ArgumentError("kind is :l1 or :l0"))
  n, batch = size(Y)
  ld = batch > 1 ? stride(Y, 2) : max(n, 1)
  for M in (Q, XK, SJ, xkn)
    M === nothing && continue
    (size(M) == (n, batch) && (batch <= 1 || stride(M, 2) == ld)) || throw(BoundsError())
  end
  (length(λ) == batch && length(σ) == batch && length(q_scale) == batch && size(out) == (3, batch)) || throw(BoundsError())
  (l === nothing) == (u === nothing) || throw(ArgumentError("l and u are given together"))
  if l === nothing
    selected === nothing || throw(ArgumentError("selected needs the box form"))
    check(proxstep_batch_call(Val(kind), Y, Q, XK, SJ, n, batch, ld, λ, σ, q_scale, xkn, out))
  else
    (length(l) == batch && length(u) == batch && (selected === nothing || length(selected) == n)) || throw(BoundsError())
    check(proxstep_batch_call(Val(kind), Y, Q, XK, SJ, n, batch, ld, λ, σ, l, u, selected, q_scale, xkn, out))
  end
  return Y, out
end

# ---------------------------------------------------------------------------------------------
# iprox! fused with the step statistics of a diagonal quasi-Newton iteration (spx_iproxstep_*; no counterpart in the
# reference: what R2DH does around iprox! -- `ψ(s)`, `dot(∇fk, s)`, `dot(s, d .* s)`, `xk + s`, `norm(s)` -- in the pass that
# stores s).  Returns (y, h, gy, ydy, yy):
#   h   = λ Σ over the selected indices of Term((xk + sj) + y)
#   gy  = Σ over all i of g[i] y[i]      ydy = Σ over all i of (d[i] y[i]) y[i]  (the caller halves)      yy = Σ over all i of y[i]^2
# xkn (a device vector that is none of y, g, d, ψ.xk, ψ.sj, l, u; or nothing) receives (xk + sj) + y.
# `out` = a ROCVector{Float64} of at least 4 elements: the four sums stay on the device, nothing is read back and the call
# does not synchronise; returns (y, out).  check_d = true (unboxed forms) asserts d .> 0 and needs out === nothing.
# y must be neither g nor d.  Headline operator and the unboxed ℓ1 norm shown; spx_iproxstep_l0 / l0_box follow the same pattern.
# ---------------------------------------------------------------------------------------------
function iprox_step!(y::DVec, ψ::ShiftedNormL1Box{Float64, <:DVec, <:DVec, <:DVec}, g::DVec, d::DVec;
                     xkn::Union{Nothing, DVec} = nothing, out::Union{Nothing, DVec} = nothing)
  n = length(ψ.xk)
  (length(y) == n && length(g) == n && length(d) == n && (xkn === nothing || length(xkn) == n)) || throw(BoundsError())
  (out === nothing || length(out) >= 4) || throw(ArgumentError("out needs at least 4 elements"))
  m = mask_for(ψ)
  stats = zeros(Cdouble, 4)
  check(ccall((:spx_iproxstep_l1_box, libspx), Cint,
              (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Cdouble,
               Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Cdouble, Ptr{UInt8}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
              ctx(), dptr(y), dptr(g), dptr(d), dptr(ψ.xk), dptr(ψ.sj), n, ψ.λ,
              dptr(vec_or_nothing(ψ.l)), dptr(vec_or_nothing(ψ.u)), scal(ψ.l), scal(ψ.u),
              mptr(m), dptr(xkn), out === nothing ? pointer(stats) : Ptr{Cdouble}(C_NULL), dptr(out)))
  return out === nothing ? (y, stats[1], stats[2], stats[3], stats[4]) : (y, out)
end
function iprox_step!(y::DVec, ψ::ShiftedNormL1{Float64, <:DVec, <:DVec, <:DVec}, g::DVec, d::DVec;
                     check_d::Bool = false, xkn::Union{Nothing, DVec} = nothing, out::Union{Nothing, DVec} = nothing)
  n = length(ψ.xk)
  (length(y) == n && length(g) == n && length(d) == n && (xkn === nothing || length(xkn) == n)) || throw(BoundsError())
  (out === nothing || length(out) >= 4) || throw(ArgumentError("out needs at least 4 elements"))
  (check_d && out !== nothing) && throw(ArgumentError("check_d = true needs the host form of the statistics (out = nothing)"))
  stats = zeros(Cdouble, 4)
  st = ccall((:spx_iproxstep_l1, libspx), Cint,
             (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Cdouble, Cint,
              Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
             ctx(), dptr(y), dptr(g), dptr(d), dptr(ψ.xk), dptr(ψ.sj), n, ψ.λ, check_d ? 1 : 0,
             dptr(xkn), out === nothing ? pointer(stats) : Ptr{Cdouble}(C_NULL), dptr(out))
  st == 6 && throw(AssertionError("d[i] > 0"))      # SPX_ERR_ASSERT
  check(st)
  return out === nothing ? (y, stats[1], stats[2], stats[3], stats[4]) : (y, out)
end

# ---------------------------------------------------------------------------------------------
# The same for `batch` problems in ONE call, every per-problem scalar read from DEVICE memory (spx_iproxstep_{l1,l0}[_box]_batch;
# no counterpart in the reference): a path of R2DH problems in lock step.  Problem b is column b of the n × batch device
# matrices Y, G, D, XK, SJ (and xkn), as for prox_step_batch!.  λ (and l, u: one scalar per problem) are ROCVector{Float64} of
# length batch.  d_shift: a ROCVector{Float64} of length batch or nothing -- given, every element site sees D[i, b] + d_shift[b],
# ONE rounded add formed on the fly, in place of D[i, b]: R2DH's D + σ_b needs no pass of its own and follows the σ_b a solver
# leaves on the device; nothing: D enters as it is.  out: a 4 × batch device matrix; out[:, b] = (h, gy, ydy, yy) of problem b as
# iprox_step! returns them (ydy with D + d_shift).  d_flag (unboxed kinds): a ROCVector{Int32} of length batch; after the call
# d_flag[b] is 1 when some D[i, b] + d_shift[b] <= 0 or NaN occurred in problem b (the reference's `@assert d[i] > 0`, per problem,
# not read back), else 0.  kind = :l1 or :l0; the box form is taken when l and u are given.  Returns (Y, out); never synchronises.
# ---------------------------------------------------------------------------------------------
const libspx_ibatch = get(ENV, "LIBSPX_IBATCH", "libspx_ibatch.so")   # include/spx_ibatch.h: a third library, linked against libspx
i32ptr(v::ROCVector{Int32}) = Ptr{Int32}(UInt(pointer(v)))
for kind in (:l1, :l0)   # (ccall wants its symbol as a literal: one method per operator)
  plain, boxed = QuoteNode(Symbol(:spx_iproxstep_, kind, :_batch)), QuoteNode(Symbol(:spx_iproxstep_, kind, :_box_batch))
  @eval iproxstep_batch_call(::Val{$(QuoteNode(kind))}, Y, G, D, XK, SJ, n, batch, ld, λ, d_shift, d_flag::ROCVector{Int32}, xkn, out) =
    ccall(($plain, libspx_ibatch), Cint,
          (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Int64, Int64,
           Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Ptr{Cdouble}, Ptr{Cdouble}),
          ctx(), dptr(Y), dptr(G), dptr(D), dptr(XK), dptr(SJ), n, batch, ld, dptr(λ), dptr(d_shift), i32ptr(d_flag), dptr(xkn),
          dptr(out))
  @eval iproxstep_batch_call(::Val{$(QuoteNode(kind))}, Y, G, D, XK, SJ, n, batch, ld, λ, d_shift, l::DVec, u::DVec, selected, xkn, out) =
    ccall(($boxed, libspx_ibatch), Cint,
          (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Int64, Int64,
           Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{UInt8}, Ptr{Cdouble}, Ptr{Cdouble}),
          ctx(), dptr(Y), dptr(G), dptr(D), dptr(XK), dptr(SJ), n, batch, ld, dptr(λ), dptr(d_shift), dptr(l), dptr(u),
          mptr(selected), dptr(xkn), dptr(out))
end
function iprox_step_batch!(Y::DMat, kind::Symbol, G::DMat, D::DMat, XK::DMat, SJ::DMat, λ::DVec;
                           d_shift::Union{Nothing, DVec} = nothing, l::Union{Nothing, DVec} = nothing,
                           u::Union{Nothing, DVec} = nothing, selected::Union{Nothing, ROCVector{UInt8}} = nothing,
                           xkn::Union{Nothing, DMat} = nothing, out::DMat = ROCMatrix{Float64}(undef, 4, size(Y, 2)),
                           d_flag::Union{Nothing, ROCVector{Int32}} = nothing)
  kind in (:l1, :l0) || throw(ArgumentError("kind is :l1 or :l0"))
  n, batch = size(Y)
  ld = batch > 1 ? stride(Y, 2) : max(n, 1)
  for M in (G, D, XK, SJ, xkn)
    M === nothing && continue
    (size(M) == (n, batch) && (batch <= 1 || stride(M, 2) == ld)) || throw(BoundsError())
  end
  (length(λ) == batch && (d_shift === nothing || length(d_shift) == batch) && size(out) == (4, batch)) || throw(BoundsError())
  (l === nothing) == (u === nothing) || throw(ArgumentError("l and u are given together"))
  if l === nothing
    selected === nothing || throw(ArgumentError("selected needs the box form"))
    flag = d_flag === nothing ? ROCVector{Int32}(undef, max(batch, 1)) : d_flag
    (d_flag === nothing || length(d_flag) == batch) || throw(BoundsError())
    check(iproxstep_batch_call(Val(kind), Y, G, D, XK, SJ, n, batch, ld, λ, d_shift, flag, xkn, out))
  else
    d_flag === nothing || throw(ArgumentError("d_flag belongs to the unboxed kinds"))
    (length(l) == batch && length(u) == batch && (selected === nothing || length(selected) == n)) || throw(BoundsError())
    check(iproxstep_batch_call(Val(kind), Y, G, D, XK, SJ, n, batch, ld, λ, d_shift, l, u, selected, xkn, out))
  end
  return Y, out
end

# ---------------------------------------------------------------------------------------------
# group_prox_step! of the plain operator (ShiftedGroupNormL2) for `batch` problems in ONE call, every per-problem parameter read
# from DEVICE memory (spx_proxstep_group_l2_batch; no counterpart in the reference): a path of group-lasso problems in lock step.
# Problem b is column b of the n × batch device matrices Y, Q, XK, SJ (and xkn), n = ngroups * group_size in uniform contiguous
# groups of group_size (1 .. 512) elements.  λ: the group weights, a ROCVector{Float64} of length ngroups (ONE weight vector
# shared by the problems: ldl = 0) or an ngroups × batch device matrix (one column per problem: ldl = its column stride).
# λ_scale: a ROCVector{Float64} of length batch or nothing -- given, the weight of group g of problem b is λ_scale[b] * λ[g(, b)],
# ONE rounded multiply.  σ, q_scale: ROCVector{Float64} of length batch.  out: a 3 × batch device matrix; out[:, b] = (h, qy, yy) of
# problem b as group_prox_step! returns them.  Returns (Y, out); never synchronises.
# (This binding has never been executed: there is no Julia toolchain where the library is built and tested.)
# ---------------------------------------------------------------------------------------------
const libspx_gbatch = get(ENV, "LIBSPX_GBATCH", "libspx_gbatch.so")   # include/spx_gbatch.h: a fourth library, linked against libspx
function prox_step_group_batch!(Y::DMat, Q::DMat, XK::DMat, SJ::DMat, group_size::Integer, λ::Union{DVec, DMat}, σ::DVec,
                                q_scale::DVec; λ_scale::Union{Nothing, DVec} = nothing, xkn::Union{Nothing, DMat} = nothing,
                                out::DMat = ROCMatrix{Float64}(undef, 3, size(Y, 2)))
  n, batch = size(Y)
  (1 <= group_size <= 512 && n % group_size == 0) || throw(ArgumentError("uniform groups of 1 .. 512 elements"))
  ngroups = n ÷ group_size
  ld = batch > 1 ? stride(Y, 2) : max(n, 1)
  for M in (Q, XK, SJ, xkn)
    M === nothing && continue
    (size(M) == (n, batch) && (batch <= 1 || stride(M, 2) == ld)) || throw(BoundsError())
  end
  ldl = 0
  if λ isa DMat
    size(λ) == (ngroups, batch) || throw(BoundsError())
    ldl = batch > 1 ? stride(λ, 2) : max(ngroups, 1)
  else
    length(λ) == ngroups || throw(BoundsError())
  end
  (length(σ) == batch && length(q_scale) == batch && (λ_scale === nothing || length(λ_scale) == batch) &&
   size(out) == (3, batch)) || throw(BoundsError())
  check(ccall((:spx_proxstep_group_l2_batch, libspx_gbatch), Cint,
              (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Int64, Int64, Int64,
               Ptr{Cdouble}, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
              ctx(), dptr(Y), dptr(Q), dptr(XK), dptr(SJ), group_size, ngroups, batch, ld, dptr(λ), ldl, dptr(λ_scale), dptr(σ),
              dptr(q_scale), dptr(xkn), dptr(out)))
  return Y, out
end

# ---------------------------------------------------------------------------------------------
# The same for the trust-region operator (ShiftedGroupNormL2Binf, spx_proxstep_group_l2_binf_batch; no counterpart in the
# reference): `batch` TR problems in ONE call, every problem with its own radius.  Δ: a ROCVector{Float64} of length batch, read
# by the kernel like σ and q_scale -- a loop that shrinks and grows the radii on the device needs no host round trip.  Everything
# else as prox_step_group_batch!.  Column b of Y and xkn has the bits of group_prox_step! on that column alone (under tuning key
# 9 of the context), on vectors of the launch's alignment class (include/spx_gbinf_batch.h).
# (This binding has never been executed: there is no Julia toolchain where the library is built and tested.)
# ---------------------------------------------------------------------------------------------
const libspx_gbinf_batch = get(ENV, "LIBSPX_GBINF_BATCH", "libspx_gbinf_batch.so")   # include/spx_gbinf_batch.h: a fifth library, linked against libspx
function prox_step_group_binf_batch!(Y::DMat, Q::DMat, XK::DMat, SJ::DMat, group_size::Integer, λ::Union{DVec, DMat}, σ::DVec,
                                     Δ::DVec, q_scale::DVec; λ_scale::Union{Nothing, DVec} = nothing,
                                     xkn::Union{Nothing, DMat} = nothing, out::DMat = ROCMatrix{Float64}(undef, 3, size(Y, 2)))
  n, batch = size(Y)
  (1 <= group_size <= 512 && n % group_size == 0) || throw(ArgumentError("uniform groups of 1 .. 512 elements"))
  ngroups = n ÷ group_size
  ld = batch > 1 ? stride(Y, 2) : max(n, 1)
  for M in (Q, XK, SJ, xkn)
    M === nothing && continue
    (size(M) == (n, batch) && (batch <= 1 || stride(M, 2) == ld)) || throw(BoundsError())
  end
  ldl = 0
  if λ isa DMat
    size(λ) == (ngroups, batch) || throw(BoundsError())
    ldl = batch > 1 ? stride(λ, 2) : max(ngroups, 1)
  else
    length(λ) == ngroups || throw(BoundsError())
  end
  (length(σ) == batch && length(Δ) == batch && length(q_scale) == batch && (λ_scale === nothing || length(λ_scale) == batch) &&
   size(out) == (3, batch)) || throw(BoundsError())
  check(ccall((:spx_proxstep_group_l2_binf_batch, libspx_gbinf_batch), Cint,
              (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Int64, Int64, Int64,
               Ptr{Cdouble}, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
              ctx(), dptr(Y), dptr(Q), dptr(XK), dptr(SJ), group_size, ngroups, batch, ld, dptr(λ), ldl, dptr(λ_scale), dptr(σ),
              dptr(Δ), dptr(q_scale), dptr(xkn), dptr(out)))
  return Y, out
end

# ---------------------------------------------------------------------------------------------
# prox! + step statistics of ShiftedNormL1B2 for MANY problems in ONE call (spx_proxstep_l1_b2_batch; no counterpart in the
# reference): column b of the n × batch matrices is one lasso problem inside its own l2 ball.  λ, σ, Δ, q_scale:
# ROCVector{Float64}s of length batch, read by the one workgroup that owns the column -- a loop that shrinks and grows the radii
# on the device needs no host round trip; χλ: one host number (χ.lambda, 1.0 in the reference).  n <= 2^20 (larger problems:
# prox_step! on ShiftedNormL1B2, one problem per call).  Column b of Y meets the accuracy of that call (1e-12 on the scale
# max(‖y‖, ‖xk‖)) and has its bits where the trust region is inactive; out[:, b] = (λ_b ‖xk + sj + y‖₁, Σ q .* y, Σ y .^ 2);
# the bits of a column depend on n, the launch's alignment class and the column's own data only (include/spx_b2_batch.h).
# (This binding has never been executed: there is no Julia toolchain where the library is built and tested.)
# ---------------------------------------------------------------------------------------------
const libspx_b2_batch = get(ENV, "LIBSPX_B2_BATCH", "libspx_b2_batch.so")   # include/spx_b2_batch.h: a sixth library, linked against libspx
function prox_step_b2_batch!(Y::DMat, Q::DMat, XK::DMat, SJ::DMat, λ::DVec, σ::DVec, Δ::DVec, q_scale::DVec; χλ::Float64 = 1.0,
                             xkn::Union{Nothing, DMat} = nothing, out::DMat = ROCMatrix{Float64}(undef, 3, size(Y, 2)))
  n, batch = size(Y)
  ld = batch > 1 ? stride(Y, 2) : max(n, 1)
  for M in (Q, XK, SJ, xkn)
    M === nothing && continue
    (size(M) == (n, batch) && (batch <= 1 || stride(M, 2) == ld)) || throw(BoundsError())
  end
  (length(λ) == batch && length(σ) == batch && length(Δ) == batch && length(q_scale) == batch && size(out) == (3, batch)) ||
    throw(BoundsError())
  check(ccall((:spx_proxstep_l1_b2_batch, libspx_b2_batch), Cint,
              (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Int64, Int64,
               Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}),
              ctx(), dptr(Y), dptr(Q), dptr(XK), dptr(SJ), n, batch, ld, dptr(λ), dptr(σ), dptr(Δ), dptr(q_scale), χλ, dptr(xkn),
              dptr(out)))
  return Y, out
end

# ---------------------------------------------------------------------------------------------
# prox! + step statistics of ShiftedIndBallL0 / ShiftedIndBallL0BInf for MANY problems in ONE call
# (spx_proxstep_indball_l0_batch, spx_proxstep_indball_l0_binf_batch; no counterpart in the reference): column b of the n × batch
# matrices is one top-r problem.  r: a ROCVector{Int64}, q_scale and Δ: ROCVector{Float64}s of length batch, read by the one
# workgroup that owns the column -- a sparsity path, folds or multi-start need no host round trip.  Δ === nothing: the plain form.
# n <= 2^20 (larger problems: prox! on ShiftedIndBallL0[BInf], one problem per call).  Column b of Y has the BITS of that prox! at
# q_scale[b] .* Q[:, b]; out[:, b] = (count(!iszero, xk + sj + y), Σ q .* y, Σ y .^ 2): h of the new point is 0 iff out[1, b] <= r[b]
# (include/spx_topr_batch.h).  Y must be none of Q, XK, SJ.
# (This binding has never been executed: there is no Julia toolchain where the library is built and tested.)
# ---------------------------------------------------------------------------------------------
const libspx_topr_batch = get(ENV, "LIBSPX_TOPR_BATCH", "libspx_topr_batch.so")   # include/spx_topr_batch.h: a seventh library, linked against libspx
function prox_step_topr_batch!(Y::DMat, Q::DMat, XK::DMat, SJ::DMat, r::ROCVector{Int64}, q_scale::DVec;
                               Δ::Union{Nothing, DVec} = nothing, xkn::Union{Nothing, DMat} = nothing,
                               out::DMat = ROCMatrix{Float64}(undef, 3, size(Y, 2)))
  n, batch = size(Y)
  ld = batch > 1 ? stride(Y, 2) : max(n, 1)
  for M in (Q, XK, SJ, xkn)
    M === nothing && continue
    (size(M) == (n, batch) && (batch <= 1 || stride(M, 2) == ld)) || throw(BoundsError())
  end
  (length(r) == batch && length(q_scale) == batch && (Δ === nothing || length(Δ) == batch) && size(out) == (3, batch)) ||
    throw(BoundsError())
  rptr = Ptr{Int64}(UInt(pointer(r)))
  if Δ === nothing
    check(ccall((:spx_proxstep_indball_l0_batch, libspx_topr_batch), Cint,
                (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Int64, Int64,
                 Ptr{Int64}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                ctx(), dptr(Y), dptr(Q), dptr(XK), dptr(SJ), n, batch, ld, rptr, dptr(q_scale), dptr(xkn), dptr(out)))
  else
    check(ccall((:spx_proxstep_indball_l0_binf_batch, libspx_topr_batch), Cint,
                (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Int64, Int64,
                 Ptr{Int64}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                ctx(), dptr(Y), dptr(Q), dptr(XK), dptr(SJ), n, batch, ld, rptr, dptr(Δ), dptr(q_scale), dptr(xkn), dptr(out)))
  end
  return Y, out
end

# ---------------------------------------------------------------------------------------------
# prox! + step statistics of ShiftedRootNormLhalf / ShiftedRootNormLhalfBox for MANY problems in ONE call
# (spx_proxstep_lhalf_batch, spx_proxstep_lhalf_box_batch; no counterpart in the reference): the arguments and the layout of
# prox_step_batch! above -- column b of the n × batch matrices is one problem, λ, σ, q_scale (and l, u) are ROCVector{Float64}s of
# length batch read by the kernel, `selected` is ONE byte mask shared by the problems, out[:, b] = (λ_b Σ √|xk + sj + y|, Σ q .* y,
# Σ y .^ 2).  Box form (l and u given): column b of Y has the BITS of prox_step! on that column.  Unboxed form: the same except
# for an element whose |q_scale q + (xk + sj)| lies between the host's threshold 54^(1/3) (2σλ)^(2/3) / 4 and the device's (4 ulps
# apart at most), which has the other branch of the prox's jump (include/spx_lhalf_batch.h); lhalf_threshold_batch! returns the
# device's thresholds.
# (These bindings have never been executed: there is no Julia toolchain where the library is built and tested.)
# ---------------------------------------------------------------------------------------------
const libspx_lhalf_batch = get(ENV, "LIBSPX_LHALF_BATCH", "libspx_lhalf_batch.so")   # include/spx_lhalf_batch.h: an eighth library, linked against libspx
function prox_step_lhalf_batch!(Y::DMat, Q::DMat, XK::DMat, SJ::DMat, λ::DVec, σ::DVec, q_scale::DVec;
                                l::Union{Nothing, DVec} = nothing, u::Union{Nothing, DVec} = nothing,
                                selected::Union{Nothing, ROCVector{UInt8}} = nothing, xkn::Union{Nothing, DMat} = nothing,
                                out::DMat = ROCMatrix{Float64}(undef, 3, size(Y, 2)))
  n, batch = size(Y)
  ld = batch > 1 ? stride(Y, 2) : max(n, 1)
  for M in (Q, XK, SJ, xkn)
    M === nothing && continue
    (size(M) == (n, batch) && (batch <= 1 || stride(M, 2) == ld)) || throw(BoundsError())
  end
  (length(λ) == batch && length(σ) == batch && length(q_scale) == batch && size(out) == (3, batch)) || throw(BoundsError())
  (l === nothing) == (u === nothing) || throw(ArgumentError("l and u are given together"))
  if l === nothing
    selected === nothing || throw(ArgumentError("selected needs the box form"))
    check(ccall((:spx_proxstep_lhalf_batch, libspx_lhalf_batch), Cint,
                (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Int64, Int64,
                 Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                ctx(), dptr(Y), dptr(Q), dptr(XK), dptr(SJ), n, batch, ld, dptr(λ), dptr(σ), dptr(q_scale), dptr(xkn), dptr(out)))
  else
    (length(l) == batch && length(u) == batch && (selected === nothing || length(selected) == n)) || throw(BoundsError())
    check(ccall((:spx_proxstep_lhalf_box_batch, libspx_lhalf_batch), Cint,
                (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Int64, Int64,
                 Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{UInt8}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                ctx(), dptr(Y), dptr(Q), dptr(XK), dptr(SJ), n, batch, ld, dptr(λ), dptr(σ), dptr(l), dptr(u), mptr(selected),
                dptr(q_scale), dptr(xkn), dptr(out)))
  end
  return Y, out
end
function lhalf_threshold_batch!(p::DVec, λ::DVec, σ::DVec)
  (length(λ) == length(p) && length(σ) == length(p)) || throw(BoundsError())
  check(ccall((:spx_lhalf_threshold_batch, libspx_lhalf_batch), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Ptr{Cdouble}),
              ctx(), dptr(λ), dptr(σ), length(p), dptr(p)))
  return p
end

# ---------------------------------------------------------------------------------------------
# l1 norm + l2-ball trust region    src/shiftedNormL1B2.jl:50-67   (χ = NormL2(χ.lambda))
# ---------------------------------------------------------------------------------------------
function prox!(y::DVec, ψ::ShiftedProximalOperators.ShiftedNormL1B2{Float64, <:DVec, <:DVec, <:DVec}, q::DVec, σ::Float64)
  n = length(ψ.xk)
  (length(y) == n && length(q) == n) || throw(BoundsError())
  check(ccall((:spx_prox_l1_b2, libspx), Cint,
              (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Cdouble, Cdouble, Cdouble, Cdouble),
              ctx(), dptr(y), dptr(q), dptr(ψ.xk), dptr(ψ.sj), n, ψ.λ, σ, ψ.Δ, ψ.χ.lambda))
  return y
end

# ---------------------------------------------------------------------------------------------
# groups                      src/shiftedGroupNormL2.jl:52-79, shiftedGroupNormL2Binf.jl:67-119
# ψ.h.idx as consecutive contiguous ranges (UnitRanges or [:]) takes the CSR / uniform entry points; any other
# index sets (Vector{Int}s, gaps, overlaps, any order) take the gather entry points, which reproduce the reference's
# sequential loop literally.  Offsets / indices / weights are uploaded once per h and cached.
# ---------------------------------------------------------------------------------------------
const LAYOUTS = IdDict{Any, Any}()

function layout_for(h, n)
  get!(LAYOUTS, h) do
    # `[:]` is the whole vector; an explicit index vector that is a contiguous run (`collect(4:6)`, runtests.jl:290) is a range
    asrange(g) = g isa Colon ? (1:n) :
                 (g isa AbstractVector{<:Integer} && !(g isa AbstractUnitRange) && !isempty(g) &&
                  all(i -> g[i + 1] - g[i] == 1, 1:(length(g) - 1))) ? (first(g):last(g)) : g
    rngs = map(asrange, h.idx)
    lam = ROCVector{Float64}(collect(Float64, h.lambda))
    if !(all(g -> g isa AbstractUnitRange, rngs) &&
         all(i -> first(rngs[i + 1]) == last(rngs[i]) + 1, 1:(length(rngs) - 1)))
      ptr = Int64[0; cumsum(Int64[length(g) for g in rngs])]       # gather form: 0-based ptr / index
      index = Int64[i - 1 for g in rngs for i in g]
      all(i -> 0 <= i < n, index) || throw(BoundsError())
      return (gather = true, ptr = ROCVector{Int64}(ptr), index = ROCVector{Int64}(index), nnz = length(index),
              ngroups = length(rngs), lambda = lam)
    end
    off = Int64[first(rngs[1]) - 1; [last(g) for g in rngs]]      # 0-based CSR offsets
    sizes = diff(off)
    uniform = off[1] == 0 && off[end] == n && all(==(sizes[1]), sizes)
    # with offsets, gsize is the size bound that lets libspx use its register-tile / LDS-resident kernels
    (gather = false, offsets = uniform ? nothing : ROCVector{Int64}(off), gsize = uniform ? sizes[1] : maximum(sizes),
     ngroups = length(rngs), lambda = lam)
  end
end

function group_call(y, ψ, q, σ, extra...)   # extra = (Δ,) for the Binf form
  n = length(ψ.xk)
  L = layout_for(ψ.h, n)
  if L.gather
    ip(v) = Ptr{Int64}(UInt(pointer(v)))
    if isempty(extra)
      check(ccall((:spx_prox_group_l2_gather, libspx), Cint,
                  (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Ptr{Int64}, Ptr{Int64}, Int64,
                   Int64, Ptr{Cdouble}, Cdouble),
                  ctx(), dptr(y), dptr(q), dptr(ψ.xk), dptr(ψ.sj), n, ip(L.ptr), ip(L.index), L.ngroups, L.nnz,
                  dptr(L.lambda), σ))
    else
      check(ccall((:spx_prox_group_l2_binf_gather, libspx), Cint,
                  (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Ptr{Int64}, Ptr{Int64}, Int64,
                   Int64, Ptr{Cdouble}, Cdouble, Cdouble),
                  ctx(), dptr(y), dptr(q), dptr(ψ.xk), dptr(ψ.sj), n, ip(L.ptr), ip(L.index), L.ngroups, L.nnz,
                  dptr(L.lambda), σ, extra[1]))
    end
    return y
  end
  offp = L.offsets === nothing ? Ptr{Int64}(C_NULL) : Ptr{Int64}(UInt(pointer(L.offsets)))
  if isempty(extra)
    check(ccall((:spx_prox_group_l2, libspx), Cint,
                (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Ptr{Int64}, Int64, Int64,
                 Ptr{Cdouble}, Cdouble),
                ctx(), dptr(y), dptr(q), dptr(ψ.xk), dptr(ψ.sj), n, offp, L.gsize, L.ngroups, dptr(L.lambda), σ))
  else
    check(ccall((:spx_prox_group_l2_binf, libspx), Cint,
                (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Ptr{Int64}, Int64, Int64,
                 Ptr{Cdouble}, Cdouble, Cdouble),
                ctx(), dptr(y), dptr(q), dptr(ψ.xk), dptr(ψ.sj), n, offp, L.gsize, L.ngroups, dptr(L.lambda), σ,
                extra[1]))
  end
  return y
end

function prox!(y::DVec, ψ::ShiftedGroupNormL2{Float64, RR, I, <:DVec, <:DVec, <:DVec}, q::DVec, σ::Float64) where {RR, I}
  group_call(y, ψ, q, σ)
end

function prox!(y::DVec, ψ::ShiftedGroupNormL2Binf{Float64, RR, I, <:DVec, <:DVec, <:DVec}, q::DVec, σ::Float64) where {RR, I}
  group_call(y, ψ, q, σ, ψ.Δ)
end

# prox! fused with h at the result, group forms (spx_proxval_group_l2[_binf]; contiguous groups only: a gather layout throws).
# One pass over the vectors for groups of at most 512 elements, the prox followed by ψ's reduction inside the call beyond.
function group_value_call(y, ψ, q, σ, q_scale, extra...)   # extra = (Δ,) for the Binf form
  n = length(ψ.xk)
  (length(y) == n && length(q) == n) || throw(BoundsError())
  L = layout_for(ψ.h, n)
  L.gather && throw(ArgumentError("prox_value! needs contiguous groups"))
  offp = L.offsets === nothing ? Ptr{Int64}(C_NULL) : Ptr{Int64}(UInt(pointer(L.offsets)))
  out = Ref{Cdouble}(0.0)
  if isempty(extra)
    check(ccall((:spx_proxval_group_l2, libspx), Cint,
                (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Ptr{Int64}, Int64, Int64,
                 Ptr{Cdouble}, Cdouble, Cdouble, Ptr{Cdouble}),
                ctx(), dptr(y), dptr(q), dptr(ψ.xk), dptr(ψ.sj), n, offp, L.gsize, L.ngroups, dptr(L.lambda), σ, q_scale, out))
  else
    check(ccall((:spx_proxval_group_l2_binf, libspx), Cint,
                (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Ptr{Int64}, Int64, Int64,
                 Ptr{Cdouble}, Cdouble, Cdouble, Cdouble, Ptr{Cdouble}),
                ctx(), dptr(y), dptr(q), dptr(ψ.xk), dptr(ψ.sj), n, offp, L.gsize, L.ngroups, dptr(L.lambda), σ,
                extra[1], q_scale, out))
  end
  return y, out[]
end

function prox_value!(y::DVec, ψ::ShiftedGroupNormL2{Float64, RR, I, <:DVec, <:DVec, <:DVec}, q::DVec, σ::Float64;
                     q_scale::Float64 = 1.0) where {RR, I}
  group_value_call(y, ψ, q, σ, q_scale)
end

function prox_value!(y::DVec, ψ::ShiftedGroupNormL2Binf{Float64, RR, I, <:DVec, <:DVec, <:DVec}, q::DVec, σ::Float64;
                     q_scale::Float64 = 1.0) where {RR, I}
  group_value_call(y, ψ, q, σ, q_scale, ψ.Δ)   # the h part of ψ(y): the prox lies inside the trust region
end

# prox! fused with the step statistics, group forms (spx_proxstep_group_l2[_binf]; prox_step! above for the separable operators):
# (y, h, qy, yy) with h = Σ_g λ_g ‖((xk + sj) + y)[g]‖ as prox_value! returns it, qy and yy over ALL i with the q that was passed;
# xkn receives (xk + sj) + y at every index.  `out`: the three sums stay on the device, returns (y, out).  Contiguous groups only.
# One pass over the vectors for uniform groups of at most 512 elements; prox_value!'s launches plus one streaming launch beyond.
function group_step_call(y, ψ, q, σ, q_scale, xkn, out, extra...)   # extra = (Δ,) for the Binf form
  n = length(ψ.xk)
  (length(y) == n && length(q) == n && (xkn === nothing || length(xkn) == n)) || throw(BoundsError())
  (out === nothing || length(out) >= 3) || throw(ArgumentError("out needs at least 3 elements"))
  L = layout_for(ψ.h, n)
  L.gather && throw(ArgumentError("prox_step! needs contiguous groups"))
  offp = L.offsets === nothing ? Ptr{Int64}(C_NULL) : Ptr{Int64}(UInt(pointer(L.offsets)))
  stats = zeros(Cdouble, 3)
  sp = out === nothing ? pointer(stats) : Ptr{Cdouble}(C_NULL)
  if isempty(extra)
    check(ccall((:spx_proxstep_group_l2, libspx), Cint,
                (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Ptr{Int64}, Int64, Int64,
                 Ptr{Cdouble}, Cdouble, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                ctx(), dptr(y), dptr(q), dptr(ψ.xk), dptr(ψ.sj), n, offp, L.gsize, L.ngroups, dptr(L.lambda), σ, q_scale,
                dptr(xkn), sp, dptr(out)))
  else
    check(ccall((:spx_proxstep_group_l2_binf, libspx), Cint,
                (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Ptr{Int64}, Int64, Int64,
                 Ptr{Cdouble}, Cdouble, Cdouble, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                ctx(), dptr(y), dptr(q), dptr(ψ.xk), dptr(ψ.sj), n, offp, L.gsize, L.ngroups, dptr(L.lambda), σ,
                extra[1], q_scale, dptr(xkn), sp, dptr(out)))
  end
  return out === nothing ? (y, stats[1], stats[2], stats[3]) : (y, out)
end

function prox_step!(y::DVec, ψ::ShiftedGroupNormL2{Float64, RR, I, <:DVec, <:DVec, <:DVec}, q::DVec, σ::Float64;
                    q_scale::Float64 = 1.0, xkn::Union{Nothing, DVec} = nothing, out::Union{Nothing, DVec} = nothing) where {RR, I}
  group_step_call(y, ψ, q, σ, q_scale, xkn, out)
end

function prox_step!(y::DVec, ψ::ShiftedGroupNormL2Binf{Float64, RR, I, <:DVec, <:DVec, <:DVec}, q::DVec, σ::Float64;
                    q_scale::Float64 = 1.0, xkn::Union{Nothing, DVec} = nothing, out::Union{Nothing, DVec} = nothing) where {RR, I}
  group_step_call(y, ψ, q, σ, q_scale, xkn, out, ψ.Δ)
end

# prox! fused with h at the result, ShiftedNormL1B2 (spx_proxval_l1_b2): the one launch of prox! with λ‖xk + sj + y‖₁ formed
# from the stored y on the way -- the h part of ψ(y): the prox lies inside the ℓ2 ball.  (Like the rest of this shim, never
# executed where the library is built and tested: there is no Julia toolchain there.)
function prox_value!(y::DVec, ψ::ShiftedProximalOperators.ShiftedNormL1B2{Float64, <:DVec, <:DVec, <:DVec}, q::DVec, σ::Float64;
                     q_scale::Float64 = 1.0)   # prox at q_scale .* q (TR: q = ∇fk, q_scale = -ν)
  n = length(ψ.xk)
  (length(y) == n && length(q) == n) || throw(BoundsError())
  out = Ref{Cdouble}(0.0)
  check(ccall((:spx_proxval_l1_b2, libspx), Cint,
              (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Cdouble, Cdouble, Cdouble, Cdouble,
               Cdouble, Ptr{Cdouble}),
              ctx(), dptr(y), dptr(q), dptr(ψ.xk), dptr(ψ.sj), n, ψ.λ, σ, ψ.Δ, ψ.χ.lambda, q_scale, out))
  return y, out[]
end

# prox! fused with the step statistics, ShiftedNormL1B2 (spx_proxstep_l1_b2): (y, h, qy, yy) with h as prox_value! returns it, qy
# and yy over ALL i with the q that was passed; xkn receives (xk + sj) + y at every index.  `out`: the three sums stay on the
# device, returns (y, out).  One launch on the register, LDS and 16-byte streaming forms; prox_value!'s launch plus one streaming
# launch on vectors of mixed alignment.
function prox_step!(y::DVec, ψ::ShiftedProximalOperators.ShiftedNormL1B2{Float64, <:DVec, <:DVec, <:DVec}, q::DVec, σ::Float64;
                    q_scale::Float64 = 1.0, xkn::Union{Nothing, DVec} = nothing, out::Union{Nothing, DVec} = nothing)
  n = length(ψ.xk)
  (length(y) == n && length(q) == n && (xkn === nothing || length(xkn) == n)) || throw(BoundsError())
  (out === nothing || length(out) >= 3) || throw(ArgumentError("out needs at least 3 elements"))
  stats = zeros(Cdouble, 3)
  sp = out === nothing ? pointer(stats) : Ptr{Cdouble}(C_NULL)
  check(ccall((:spx_proxstep_l1_b2, libspx), Cint,
              (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Cdouble, Cdouble, Cdouble, Cdouble,
               Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
              ctx(), dptr(y), dptr(q), dptr(ψ.xk), dptr(ψ.sj), n, ψ.λ, σ, ψ.Δ, ψ.χ.lambda, q_scale, dptr(xkn), sp, dptr(out)))
  return out === nothing ? (y, stats[1], stats[2], stats[3]) : (y, out)
end

# ---------------------------------------------------------------------------------------------
# ψ(y)                      src/ShiftedProximalOperators.jl:51-54, shiftedNormL1Box.jl:70-82 (idem L0Box, L½Box),
#                             shiftedIndBallL0BInf.jl:44-49, shiftedGroupNormL2Binf.jl:34-39
# ---------------------------------------------------------------------------------------------
# (ccall needs a literal symbol and a literal argument-type tuple: every entry point is spelled out)
for (T, sym) in ((:ShiftedNormL1, :spx_obj_l1), (:ShiftedNormL0, :spx_obj_l0), (:ShiftedRootNormLhalf, :spx_obj_lhalf))
  @eval (ψ::$T{Float64, <:DVec, <:DVec, <:DVec})(y::DVec) = with_value() do out
    ccall(($(QuoteNode(sym)), libspx), Cint,
          (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Cdouble, Ptr{Cdouble}),
          ctx(), dptr(y), dptr(ψ.xk), dptr(ψ.sj), length(y), ψ.λ, out)
  end
end
for (T, sym) in ((:ShiftedNormL1Box, :spx_obj_l1_box), (:ShiftedNormL0Box, :spx_obj_l0_box),
                 (:ShiftedRootNormLhalfBox, :spx_obj_lhalf_box))
  @eval function (ψ::$T{Float64, <:DVec, <:DVec, <:DVec})(y::DVec)
    m = mask_for(ψ)
    with_value() do out
      ccall(($(QuoteNode(sym)), libspx), Cint,
            (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble,
             Cdouble, Ptr{UInt8}, Ptr{Cdouble}),
            ctx(), dptr(y), dptr(ψ.xk), dptr(ψ.sj), length(y), ψ.λ, dptr(vec_or_nothing(ψ.l)),
            dptr(vec_or_nothing(ψ.u)), scal(ψ.l), scal(ψ.u), mptr(m), out)
    end
  end
end
(ψ::ShiftedIndBallL0{<:Integer, Float64, <:DVec, <:DVec, <:DVec})(y::DVec) = with_value() do out
  ccall((:spx_obj_indball_l0, libspx), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Int64, Ptr{Cdouble}),
        ctx(), dptr(y), dptr(ψ.xk), dptr(ψ.sj), length(y), ψ.r, out)
end
(ψ::ShiftedProximalOperators.ShiftedNormL1B2{Float64, <:DVec, <:DVec, <:DVec})(y::DVec) = with_value() do out  # src/shiftedNormL1B2.jl:32
  ccall((:spx_obj_l1_b2, libspx), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Cdouble, Cdouble, Ptr{Cdouble}),
        ctx(), dptr(y), dptr(ψ.xk), dptr(ψ.sj), length(y), ψ.λ, ψ.Δ, out)
end
(ψ::ShiftedIndBallL0BInf{<:Integer, Float64, <:DVec, <:DVec, <:DVec})(y::DVec) = with_value() do out
  ccall((:spx_obj_indball_l0_binf, libspx), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Int64, Cdouble, Ptr{Cdouble}),
        ctx(), dptr(y), dptr(ψ.xk), dptr(ψ.sj), length(y), ψ.r, ψ.Δ, out)
end
# (group forms: spx_obj_group_l2 / spx_obj_group_l2_binf with the layout_for(ψ.h, n) arguments, as in group_call)


# ---------------------------------------------------------------------------------------------
# Float32 (round 2): the reference is generic in R <: Real; spx_prox_*_f32 reproduce the NormL1 / NormL0 bodies bit for bit
# in fp32, on contiguous views that start at any element (src/shiftedNormL1Box.jl:89-94, test/runtests.jl:196-209).
# RootNormLhalf{Float32} keeps the reference's own method (its body computes in Float64).
# ---------------------------------------------------------------------------------------------
const DVec32 = Union{ROCVector{Float32}, SubArray{Float32, 1, <:ROCVector{Float32}, <:Tuple{AbstractUnitRange}, true}}
dptr32(v) = v === nothing ? Ptr{Cfloat}(C_NULL) : Ptr{Cfloat}(UInt(pointer(v)))
vec32_or_nothing(b) = b isa Real ? nothing : b
scal32(b) = b isa Real ? Float32(b) : 0.0f0

for (T, sym) in ((:ShiftedNormL1, :spx_prox_l1_f32), (:ShiftedNormL0, :spx_prox_l0_f32))
  @eval function prox!(y::DVec32, ψ::$T{Float32, <:DVec32, <:DVec32, <:DVec32}, q::DVec32, σ::Float32)
    n = length(ψ.xk)
    (length(y) == n && length(q) == n) || throw(BoundsError())
    check(ccall(($(QuoteNode(sym)), libspx), Cint,
                (Ptr{Cvoid}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Cfloat, Cfloat),
                ctx(), dptr32(y), dptr32(q), dptr32(ψ.xk), dptr32(ψ.sj), n, ψ.λ, σ))
    return y
  end
end
for (T, sym) in ((:ShiftedNormL1Box, :spx_prox_l1_box_f32), (:ShiftedNormL0Box, :spx_prox_l0_box_f32))
  @eval function prox!(y::DVec32, ψ::$T{Float32, <:DVec32, <:DVec32, <:DVec32}, q::DVec32, σ::Float32)
    n = length(ψ.xk)
    (length(y) == n && length(q) == n) || throw(BoundsError())
    (ψ.l isa Real || ψ.l isa DVec32) && (ψ.u isa Real || ψ.u isa DVec32) ||
      return invoke(prox!, Tuple{AbstractVector{Float32}, $T{Float32}, AbstractVector{Float32}, Float32}, y, ψ, q, σ)
    m = mask_for(ψ)
    check(ccall(($(QuoteNode(sym)), libspx), Cint,
                (Ptr{Cvoid}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Cfloat, Cfloat,
                 Ptr{Cfloat}, Ptr{Cfloat}, Cfloat, Cfloat, Ptr{UInt8}),
                ctx(), dptr32(y), dptr32(q), dptr32(ψ.xk), dptr32(ψ.sj), n, ψ.λ, σ,
                dptr32(vec32_or_nothing(ψ.l)), dptr32(vec32_or_nothing(ψ.u)), scal32(ψ.l), scal32(ψ.u), mptr(m)))
    return y
  end
end

# iprox! on Float32 vectors (round 3: spx_iprox_*_f32; src/shiftedNormL1.jl:60-75, shiftedNormL0.jl:61-80, shiftedNormL1Box.jl:131-225,
# shiftedNormL0Box.jl:137-231).  check_d = 1: the reference's `@assert d[i] > 0` (status 6 -> AssertionError).
for (T, sym) in ((:ShiftedNormL1, :spx_iprox_l1_f32), (:ShiftedNormL0, :spx_iprox_l0_f32))
  @eval function iprox!(y::DVec32, ψ::$T{Float32, <:DVec32, <:DVec32, <:DVec32}, g::DVec32, d::DVec32)
    n = length(ψ.xk)
    (length(y) == n && length(g) == n && length(d) == n) || throw(BoundsError())
    st = ccall(($(QuoteNode(sym)), libspx), Cint,
               (Ptr{Cvoid}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Cfloat, Cint),
               ctx(), dptr32(y), dptr32(g), dptr32(d), dptr32(ψ.xk), dptr32(ψ.sj), n, ψ.λ, 1)
    st == 6 && throw(AssertionError("d[i] > 0"))
    check(st)
    return y
  end
end
for (T, sym) in ((:ShiftedNormL1Box, :spx_iprox_l1_box_f32), (:ShiftedNormL0Box, :spx_iprox_l0_box_f32))
  @eval function iprox!(y::DVec32, ψ::$T{Float32, <:DVec32, <:DVec32, <:DVec32}, g::DVec32, d::DVec32)
    n = length(ψ.xk)
    (length(y) == n && length(g) == n && length(d) == n) || throw(BoundsError())
    (ψ.l isa Real || ψ.l isa DVec32) && (ψ.u isa Real || ψ.u isa DVec32) ||
      return invoke(iprox!, Tuple{AbstractVector{Float32}, $T{Float32}, AbstractVector{Float32}, AbstractVector{Float32}}, y, ψ, g, d)
    m = mask_for(ψ)
    check(ccall(($(QuoteNode(sym)), libspx), Cint,
                (Ptr{Cvoid}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Cfloat,
                 Ptr{Cfloat}, Ptr{Cfloat}, Cfloat, Cfloat, Ptr{UInt8}),
                ctx(), dptr32(y), dptr32(g), dptr32(d), dptr32(ψ.xk), dptr32(ψ.sj), n, ψ.λ,
                dptr32(vec32_or_nothing(ψ.l)), dptr32(vec32_or_nothing(ψ.u)), scal32(ψ.l), scal32(ψ.u), mptr(m)))
    return y
  end
end

# ψ(y) on Float32 vectors (spx_obj_*_f32): element operations in Float32 as in the reference, the sum in Float64, the result
# rounded to the Float32 the reference returns.  test/runtests.jl:196-209, 268-282, 346-360, 397-412, 524-550.
for (T, sym) in ((:ShiftedNormL1, :spx_obj_l1_f32), (:ShiftedNormL0, :spx_obj_l0_f32), (:ShiftedRootNormLhalf, :spx_obj_lhalf_f32))
  @eval (ψ::$T{Float32, <:DVec32, <:DVec32, <:DVec32})(y::DVec32) = Float32(with_value() do out
    ccall(($(QuoteNode(sym)), libspx), Cint, (Ptr{Cvoid}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Cfloat, Ptr{Cdouble}),
          ctx(), dptr32(y), dptr32(ψ.xk), dptr32(ψ.sj), length(y), ψ.λ, out)
  end)
end
for (T, sym) in ((:ShiftedNormL1Box, :spx_obj_l1_box_f32), (:ShiftedNormL0Box, :spx_obj_l0_box_f32),
                 (:ShiftedRootNormLhalfBox, :spx_obj_lhalf_box_f32))
  @eval function (ψ::$T{Float32, <:DVec32, <:DVec32, <:DVec32})(y::DVec32)
    m = mask_for(ψ)
    v = with_value() do out
      ccall(($(QuoteNode(sym)), libspx), Cint,
            (Ptr{Cvoid}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Cfloat, Ptr{Cfloat}, Ptr{Cfloat}, Cfloat, Cfloat, Ptr{UInt8},
             Ptr{Cdouble}),
            ctx(), dptr32(y), dptr32(ψ.xk), dptr32(ψ.sj), length(y), ψ.λ, dptr32(vec32_or_nothing(ψ.l)),
            dptr32(vec32_or_nothing(ψ.u)), scal32(ψ.l), scal32(ψ.u), mptr(m), out)
    end
    return isinf(v) ? Inf : Float32(v)   # (the reference returns the Float64 literal Inf on an infeasible point, :78)
  end
end
(ψ::ShiftedIndBallL0{<:Integer, Float32, <:DVec32, <:DVec32, <:DVec32})(y::DVec32) = with_value() do out
  ccall((:spx_obj_indball_l0_f32, libspx), Cint, (Ptr{Cvoid}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Int64, Ptr{Cdouble}),
        ctx(), dptr32(y), dptr32(ψ.xk), dptr32(ψ.sj), length(y), ψ.r, out)
end
(ψ::ShiftedIndBallL0BInf{<:Integer, Float32, <:DVec32, <:DVec32, <:DVec32})(y::DVec32) = with_value() do out
  ccall((:spx_obj_indball_l0_binf_f32, libspx), Cint,
        (Ptr{Cvoid}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Int64, Cfloat, Ptr{Cdouble}),
        ctx(), dptr32(y), dptr32(ψ.xk), dptr32(ψ.sj), length(y), ψ.r, ψ.Δ, out)
end
# (group forms: spx_obj_group_l2_f32 / spx_obj_group_l2_binf_f32 with the layout_for(ψ.h, n) arguments and a Float32 λ vector)

# top-r on Float32 vectors (round 3: spx_prox_indball_l0[_binf]_f32; src/shiftedIndBallL0.jl:54-72, shiftedIndBallL0BInf.jl:73-95
# with R = Float32): v = (xk + sj) + q, the magnitude order and the final subtraction / clamp are Float32 operations.  One launch
# with the vector on chip up to 2^23 elements.
function prox!(y::DVec32, ψ::ShiftedIndBallL0{<:Integer, Float32, <:DVec32, <:DVec32, <:DVec32}, q::DVec32, σ::Float32)
  n = length(ψ.xk)
  (length(y) == n && length(q) == n) || throw(BoundsError())
  check(ccall((:spx_prox_indball_l0_f32, libspx), Cint,
              (Ptr{Cvoid}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Int64),
              ctx(), dptr32(y), dptr32(q), dptr32(ψ.xk), dptr32(ψ.sj), n, ψ.r))
  return y
end
function prox!(y::DVec32, ψ::ShiftedIndBallL0BInf{<:Integer, Float32, <:DVec32, <:DVec32, <:DVec32}, q::DVec32, σ::Float32)
  n = length(ψ.xk)
  (length(y) == n && length(q) == n) || throw(BoundsError())
  check(ccall((:spx_prox_indball_l0_binf_f32, libspx), Cint,
              (Ptr{Cvoid}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Int64, Cfloat),
              ctx(), dptr32(y), dptr32(q), dptr32(ψ.xk), dptr32(ψ.sj), n, ψ.r, ψ.Δ))
  return y
end

# ShiftedGroupNormL2 on Float32 vectors, contiguous groups (round 3: spx_prox_group_l2_f32; src/shiftedGroupNormL2.jl:52-79 with
# R = Float32; index sets keep the reference's method).  λ travels as a Float32 device vector, cached per h (and per content).
# (ADVICE r3: the cache is keyed on the lambda ARRAY (mutable, so it can be held weakly: entries die with it) and on a hash of
#  its contents -- `h.lambda .= ...` in a continuation loop must not leave a stale device copy behind)
const LAMBDA32 = WeakKeyDict{Any, Any}()
function lambda32_for(h)
  lam = h.lambda
  key = hash(lam)
  ent = get(LAMBDA32, lam, nothing)
  if ent === nothing || ent[1] != key
    ent = (key, ROCVector{Float32}(collect(Float32, lam)))
    LAMBDA32[lam] = ent
  end
  return ent[2]
end
function prox!(y::DVec32, ψ::ShiftedGroupNormL2{Float32, <:Any, <:Any, <:DVec32, <:DVec32, <:DVec32}, q::DVec32, σ::Float32)
  n = length(ψ.xk)
  (length(y) == n && length(q) == n) || throw(BoundsError())
  L = layout_for(ψ.h, n)
  L.gather && return invoke(prox!, Tuple{AbstractVector{Float32}, typeof(ψ), AbstractVector{Float32}, Float32}, y, ψ, q, σ)  # index sets: the reference's own method
  lam32 = lambda32_for(ψ.h)
  offp = L.offsets === nothing ? Ptr{Int64}(C_NULL) : Ptr{Int64}(UInt(pointer(L.offsets)))
  check(ccall((:spx_prox_group_l2_f32, libspx), Cint,
              (Ptr{Cvoid}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Ptr{Int64}, Int64, Int64, Ptr{Cfloat}, Cfloat),
              ctx(), dptr32(y), dptr32(q), dptr32(ψ.xk), dptr32(ψ.sj), n, offp, L.gsize, L.ngroups, dptr32(lam32), σ))
  return y
end

# ---------------------------------------------------------------------------------------------
# Device-resident values (round 2): `device_values(out::ROCVector{Float64}) do ... end` -- inside the block ψ(y) and prox_value!
# store their Float64 result in out[1] and return NaN; nothing is read back (spx_ctx_set_value_target).
# ---------------------------------------------------------------------------------------------
function device_values(f, out::ROCVector{Float64})
  check(ccall((:spx_ctx_set_value_target, libspx), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), ctx(), dptr(out)))
  try
    return f()
  finally
    check(ccall((:spx_ctx_set_value_target, libspx), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), ctx(), Ptr{Cdouble}(C_NULL)))
  end
end

# shift!, set_radius!, set_bounds!, prox (src/ShiftedProximalOperators.jl:72-111,189-190) need no methods:
# they are broadcasts / field updates on the stored (device) arrays and already work on ROCArrays.
# The Box constructors' `any(l .> u)` (src/shiftedNormL1Box.jl:33-35) is a device reduction via broadcasting.

end # module
