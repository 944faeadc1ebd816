"""Per-element checks of kernel outputs against fp64 references.

No GPU dependency: everything works on whatever device its arguments live
on. `U` = 2^-8 is the bf16 unit roundoff (8 significand bits, round to
nearest even).

  assert_exact(out, ref64)            out == ref64 rounded ONCE to out.dtype
  assert_within(out, ref64, tol64)    |out - ref| <= tol for every element
  gemm_tol(ref64, absprod64, K)       any-order f32 accumulation + one bf16
                                      rounding
  int_probe(shape, lo, hi, gen)       integer-valued bf16 tensors

Integer probes make a GEMM check exact: with small integer operands every
product and every partial sum is an integer below 2^24, so the f32
accumulation is exact in any order and the only rounding left is the final
one to bf16, which must then match the fp64 result rounded once.
"""

import torch

U = 2.0 ** -8          # bf16 unit roundoff
EPS32 = 2.0 ** -23     # see gemm_tol


def round_once(ref64, dtype):
    """fp64 -> bf16 / fp32 with a single round-to-nearest-even.

    torch converts fp64 -> bf16 through fp32, which rounds twice and can
    land on the wrong side of a bf16 tie. The first step is therefore made
    round-to-odd (truncate toward zero, set the last bit if inexact): with
    16 spare bits the final RNE step then sees exactly which side of every
    bf16 tie the fp64 value lies on.
    """
    assert ref64.dtype == torch.float64
    if dtype == torch.float32:
        return ref64.float()
    assert dtype == torch.bfloat16, dtype
    f = ref64.float()
    back = f.double()
    fin = torch.isfinite(back)
    inexact = fin & (back != ref64)
    bits = f.view(torch.int32)
    # sign-magnitude: one step toward zero is magnitude bits - 1
    away = inexact & (back.abs() > ref64.abs())
    bits = torch.where(away, bits - 1, bits)
    bits = torch.where(inexact, bits | 1, bits)
    return bits.view(torch.float32).to(torch.bfloat16)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16
                               else torch.int32)


def _unravel(flat, shape):
    idx = []
    for s in reversed(shape):
        idx.append(flat % s)
        flat //= s
    return tuple(reversed(idx))


def assert_exact(out, ref64, what=""):
    """`out` equals `ref64` rounded once (RNE) to out.dtype, bit for bit."""
    assert tuple(out.shape) == tuple(ref64.shape), (out.shape, ref64.shape)
    want = round_once(ref64, out.dtype)
    bad = _bits(out) != _bits(want)
    n = int(bad.sum())
    if n:
        flat = bad.reshape(-1).nonzero().reshape(-1)[:5].tolist()
        o, w = out.reshape(-1), want.reshape(-1)
        first = [(_unravel(i, out.shape), o[i].item(), w[i].item())
                 for i in flat]
        raise AssertionError(
            "%s: %d of %d elements differ from the once-rounded fp64 "
            "reference; first (index, got, want): %s"
            % (what or "assert_exact", n, out.numel(), first))


def assert_within(out, ref64, tol64, what=""):
    """Every element satisfies |out - ref| <= tol (none excluded; a NaN or
    Inf anywhere fails). Returns the worst err / tol ratio."""
    assert tuple(out.shape) == tuple(ref64.shape), (out.shape, ref64.shape)
    assert ref64.dtype == torch.float64
    tol = torch.as_tensor(tol64, dtype=torch.float64,
                          device=ref64.device).expand_as(ref64)
    err = (out.double() - ref64).abs()
    bad = ~(err <= tol)                      # NaN counts as a violation
    ratio = torch.where(tol > 0, err / tol,
                        torch.where(err == 0, torch.zeros_like(err),
                                    torch.full_like(err, float("inf"))))
    ratio = torch.where(torch.isnan(ratio),
                        torch.full_like(ratio, float("inf")), ratio)
    worst, at = ratio.reshape(-1).max(0)
    n = int(bad.sum())
    if n:
        i = int(at)
        raise AssertionError(
            "%s: %d of %d elements out of tolerance; worst err/tol %.4g at "
            "%s (got %r, ref %r, tol %.4g)"
            % (what or "assert_within", n, out.numel(), worst.item(),
               _unravel(i, out.shape), out.reshape(-1)[i].item(),
               ref64.reshape(-1)[i].item(), tol.reshape(-1)[i].item()))
    return worst.item()


def gemm_tol(ref64, absprod64, K):
    """u*|ref| + (1+u)*(K+3)*2^-23*absprod, absprod = |A| @ |B| + |bias|.

    A length-K dot product accumulated in f32 in any order, with alpha and
    bias applied in f32 (K products are exact in f32 for bf16 operands; K-1
    adds, the bias add and the alpha multiply make at most K+1 roundings,
    K+3 leaves slack for a split-K finish), is within (K+3)*eps*absprod of
    the true value to first order; 2^-23 rather than 2^-24 so the bound
    holds whichever way the matrix unit rounds its accumulate. The final
    bf16 rounding adds u times the accumulated value, itself within the
    accumulation bound of |ref|: hence the (1+u) factor.
    """
    return U * ref64.abs() + (1 + U) * (K + 3) * EPS32 * absprod64


def int_probe(shape, lo, hi, gen):
    """bf16 tensor of integers uniform in {lo..hi} on the generator's
    device (|lo|, |hi| <= 256 so every value is exact in bf16)."""
    assert -256 <= lo <= hi <= 256
    return torch.randint(lo, hi + 1, tuple(shape), generator=gen,
                         device=gen.device).to(torch.bfloat16)
