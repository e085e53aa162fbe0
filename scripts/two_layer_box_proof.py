#!/usr/bin/env python3
"""Checks that one EXACT two-layer RK4 sub-step started inside the boxes of rscm_amd/csrc/two_layer_box.hpp keeps every numerator in
spec_div's window, so that the state-guarded year loop of two_layer_body.hpp may skip the per-numerator tags.

Every value of the sub-step is followed as an abstract double: which of {+0, -0, positive, negative} it can be, a power of two
2^lo that bounds its magnitude from below when it is not zero, and a number hi that bounds it from above.  The operations are the
kernel's, in its order (two_layer_body.hpp, rhs_exact / rk4_step_exact), each rounded to nearest:

  product   nonzero x*y: |x*y| >= 2^(lo_x + lo_y), a double, so the rounded product is too; hi = hi_x * hi_y rounded up.
            A zero factor gives a zero whose sign is the product of the signs.
  quotient  by a divisor in [2^dlo, 2^dhi): a nonzero quotient exceeds 2^(lo_n - dhi); hi = hi_n / 2^dlo.
  sum       x + y of nonzero operands.  Same sign: |x + y| >= max(|x|, |y|).  Opposite signs: if |y| < |x|/2 the sum exceeds |x|/2,
            if |y| > 2|x| it exceeds |x|; otherwise both operands are at least |x|/2 >= 2^(lo_x - 1), so both are multiples of
            2^(lo_x - 53) and so is their difference: it is 0 or at least 2^(lo_x - 53).  The same holds with x and y exchanged, so a
            nonzero sum is at least 2^(max(lo_x, lo_y) - 53).  A sum that cancels exactly is +0; it is -0 only if both operands are
            -0.  With one zero operand the sum is the other operand (or a zero by the rules of signs).

Every lower bound stays far above 2^-1022, so denormals (where the ulp argument would change) never enter.  The numerators must
be +0 (spec_div(+0) = +0 = IEEE; -0 would come out as +0) or lie in [2^-511, 2^513), and k2, k3 below 2^1023 so that 2*k2 and 2*k3
are finite (rk4_combine_fused2).  The end of the sub-step needs nothing: it is the next sub-step's start, checked there.

    python scripts/two_layer_box_proof.py            # prints the bounds of every numerator; exit status 1 if the proof fails

prove_chunk() makes the same argument for kChunkSubSteps consecutive sub-steps of rscm_amd/csrc/two_layer_chunk_box.hpp, started from
its state box and NOT re-boxed in between: the states at the start of the second and later sub-steps are the abstract results of the
RK4 combination y + ((fma(k2, 2, k1) + 2*k3) + k4) * (h/6) (the doubling is exact), and may be +0 where a combination cancels.  Its
numerators must lie in the wide window that spec_div keeps for boxed divisors (rk4_device.hpp); check_wide_window() checks that window
against the hardware's conditions for the unscaled division.
"""
import math
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "rscm_amd", "csrc", "two_layer_box.hpp")
CHUNK_HEADER = os.path.join(ROOT, "rscm_amd", "csrc", "two_layer_chunk_box.hpp")
PAIR_HEADER = os.path.join(ROOT, "rscm_amd", "csrc", "pair_div_verdict.hpp")

WINDOW_LO, WINDOW_HI = -511, 513     # numerator window [2^-511, 2^513): biased exponent in [512, 1535]
DIVISOR_LO, DIVISOR_HI = -128, 129   # divisor window [2^-128, 2^129)
MIN_EXP = -1022 + 60                 # lower bounds must stay this far above the denormals


def read_constants(path):
    """{name: value} of the header's `constexpr int kXxx = n` constants."""
    text = open(path).read()
    vals = {}
    for line in re.findall(r"^\s*constexpr\s+int\s+([^;]*);", text, re.M):
        vals.update((m.group(1), int(m.group(2))) for m in re.finditer(r"k(\w+)\s*=\s*(-?\d+)", line))
    return vals


def read_boxes(path=HEADER):
    """{name: (lo, hi)} from the constexpr pairs of the header (kXxxLo = a, kXxxHi = b)."""
    vals = read_constants(path)
    boxes = {}
    for k, v in vals.items():
        if k.endswith("Lo"):
            boxes[k[:-2]] = (v, vals[k[:-2] + "Hi"])
    return boxes


def _up(x):
    return math.nextafter(x, math.inf)


class V:
    """An abstract double: kinds (subset of '+0', '-0', '+', '-'), nonzero magnitude >= 2^lo, magnitude <= hi."""

    def __init__(self, kinds, lo, hi):
        self.kinds, self.lo, self.hi = frozenset(kinds), lo, hi
        if self.nonzero():
            if lo < MIN_EXP:
                raise ProofError(f"lower bound 2^{lo} too close to the denormals")
            if not hi < math.ldexp(1.0, 1023):
                raise ProofError(f"upper bound {hi!r} may overflow")

    def nonzero(self):
        return bool(self.kinds & {"+", "-"})

    def __repr__(self):
        return f"V({sorted(self.kinds)}, >=2^{self.lo}, <={self.hi:.3g})"


class ProofError(Exception):
    pass


def positive_box(lo, hi, zero=False):
    return V({"+", "+0"} if zero else {"+"}, lo, math.ldexp(1.0, hi))


def magnitude_box(lo, hi, zero=False):
    return V({"+", "-", "+0"} if zero else {"+", "-"}, lo, math.ldexp(1.0, hi))


def _sign(k):
    return -1 if k in ("-", "-0") else 1


def mul(x, y):
    kinds = set()
    for a in x.kinds:
        for b in y.kinds:
            s = _sign(a) * _sign(b)
            if a in ("+0", "-0") or b in ("+0", "-0"):
                kinds.add("+0" if s > 0 else "-0")
            else:
                kinds.add("+" if s > 0 else "-")
    return V(kinds, x.lo + y.lo, _up(x.hi * y.hi))


def neg(x):
    flip = {"+0": "-0", "-0": "+0", "+": "-", "-": "+"}
    return V({flip[k] for k in x.kinds}, x.lo, x.hi)


def add(x, y):
    kinds, los = set(), []
    for a in x.kinds:
        for b in y.kinds:
            za, zb = a in ("+0", "-0"), b in ("+0", "-0")
            if za and zb:
                kinds.add("-0" if (a, b) == ("-0", "-0") else "+0")
            elif za:
                kinds.add(b)
                los.append(y.lo)
            elif zb:
                kinds.add(a)
                los.append(x.lo)
            elif a == b:
                kinds.add(a)
                los.append(max(x.lo, y.lo))
            else:
                kinds |= {"+", "-", "+0"}
                los.append(max(x.lo, y.lo) - 53)
    return V(kinds, min(los) if los else 0, _up(x.hi + y.hi))


def sub(x, y):
    return add(x, neg(y))


def div(n, dlo, dhi):
    """n / d for d in [2^dlo, 2^dhi), d > 0."""
    return V(set(n.kinds), n.lo - dhi, _up(n.hi / math.ldexp(1.0, dlo)))


def check_numerator(name, x, window=(WINDOW_LO, WINDOW_HI)):
    lo, hi = window
    if "-0" in x.kinds:
        raise ProofError(f"{name} may be -0")
    if x.nonzero():
        if x.lo < lo:
            raise ProofError(f"{name} may be as small as 2^{x.lo}, below 2^{lo}")
        if not x.hi < math.ldexp(1.0, hi):
            raise ProofError(f"{name} may reach {x.hi!r}, not below 2^{hi}")


def prove(boxes, log=None):
    """Raise ProofError unless every numerator of a sub-step started inside `boxes` is +0 or inside the window; return the
    numerators' abstract values {name: V}."""
    b = boxes
    for name in ("Cs", "Cd"):
        lo, hi = b[name]
        if lo < DIVISOR_LO or hi > DIVISOR_HI:
            raise ProofError(f"{name} box [2^{lo}, 2^{hi}) leaves the divisor window")
    for name, (lo, hi) in b.items():
        if lo >= hi:
            raise ProofError(f"{name} box [2^{lo}, 2^{hi}) is empty")
    lam0 = positive_box(*b["Lambda0"])
    pa = positive_box(*b["A"], zero=True)
    ee = positive_box(*b["EffEta"])
    eta = positive_box(*b["Eta"])
    erf = magnitude_box(*b["Forcing"], zero=True)
    h = positive_box(*b["H"])                         # h and h / 2 alike
    ts = magnitude_box(*b["State"])
    td = magnitude_box(*b["State"])
    cs, cd = b["Cs"], b["Cd"]

    out = {}

    def rhs(stage, x, y):
        diff = sub(x, y)
        lam = sub(lam0, mul(pa, x))
        num_s = sub(sub(erf, mul(lam, x)), mul(ee, diff))
        num_d = mul(eta, diff)
        for nm, v in ((f"num_s[{stage}]", num_s), (f"num_d[{stage}]", num_d)):
            check_numerator(nm, v)
            out[nm] = v
            if log:
                log(f"{nm:10s} {sorted(v.kinds)}  nonzero >= 2^{v.lo}  <= {v.hi:.4g} (2^{math.log2(v.hi):.1f})")
        return div(num_s, *cs), div(num_d, *cd)

    k1s, k1d = rhs(1, ts, td)
    k2s, k2d = rhs(2, add(ts, mul(k1s, h)), add(td, mul(k1d, h)))
    k3s, k3d = rhs(3, add(ts, mul(k2s, h)), add(td, mul(k2d, h)))
    rhs(4, add(ts, mul(k3s, h)), add(td, mul(k3d, h)))
    for nm, k in (("k2s", k2s), ("k2d", k2d), ("k3s", k3s), ("k3d", k3d)):
        if not 2.0 * k.hi < math.inf:
            raise ProofError(f"2*{nm} may overflow")
    return out


def check_wide_window(boxes):
    """The wide numerator window [2^nlo, 2^nhi) for divisors d in [2^dlo, 2^dhi) (both positive powers of two apart from the edges)
    against the conditions under which v_div_scale_f64 leaves n and d unscaled and v_div_fixup_f64 passes the quotient through
    (rk4_device.hpp): d and 1/d normal, exponent(n) - exponent(d) < 768, n/d normal, biased exponent of n above 53.  The last one is
    also what makes the remainder fma(-d, q, n) exact: it is a multiple of ulp(d) * ulp(q) >= 2^(e_n - 1 - 104) >= 2^-1074."""
    dlo, dhi = boxes["WideDiv"]
    nlo, nhi = boxes["WideNum"]
    if dlo < DIVISOR_LO or dhi > DIVISOR_HI:
        raise ProofError(f"wide divisor box [2^{dlo}, 2^{dhi}) leaves the divisor window")
    if nlo - 1 + 1023 <= 53:
        raise ProofError(f"numerators down to 2^{nlo} would be scaled (biased exponent <= 53)")
    if (nhi - 1) - dlo >= 768:
        raise ProofError(f"numerators up to 2^{nhi} against divisors from 2^{dlo}: exponent difference reaches 768")
    if nlo - dhi < -1022 + 8:
        raise ProofError(f"quotients down to 2^{nlo - dhi} come too close to the denormals")
    for name in ("Cs", "Cd"):
        lo, hi = boxes[name]
        if lo < dlo or hi > dhi:
            raise ProofError(f"{name} box [2^{lo}, 2^{hi}) leaves the wide divisor box [2^{dlo}, 2^{dhi})")


def prove_chunk(boxes, n_sub=None, log=None):
    """Raise ProofError unless every numerator of n_sub (default: the header's kChunkSubSteps) consecutive sub-steps started inside
    the chunk boxes is +0 or inside the wide window and every 2*k2, 2*k3 is finite; return the numerators' abstract values."""
    b = boxes
    if n_sub is None:
        n_sub = read_constants(CHUNK_HEADER)["ChunkSubSteps"]
    check_wide_window(b)
    for name, (lo, hi) in b.items():
        if lo >= hi:
            raise ProofError(f"{name} box [2^{lo}, 2^{hi}) is empty")
    window = b["WideNum"]
    lam0 = positive_box(*b["Lambda0"])
    pa = positive_box(*b["A"], zero=True)
    ee = positive_box(*b["EffEta"])
    eta = positive_box(*b["Eta"])
    erf = magnitude_box(*b["Forcing"], zero=True)
    h, half, sixth = positive_box(*b["H"]), positive_box(*b["Half"]), positive_box(*b["Sixth"])
    two = V({"+"}, 1, 2.0)                            # the exact doubling of rk4_combine_fused2
    ts = magnitude_box(*b["State"])
    td = magnitude_box(*b["State"])
    cs, cd = b["Cs"], b["Cd"]
    out = {}

    def rhs(tag, x, y):
        diff = sub(x, y)
        lam = sub(lam0, mul(pa, x))
        num_s = sub(sub(erf, mul(lam, x)), mul(ee, diff))
        num_d = mul(eta, diff)
        for nm, v in ((f"num_s[{tag}]", num_s), (f"num_d[{tag}]", num_d)):
            check_numerator(nm, v, window)
            out[nm] = v
            if log:
                log(f"{nm:12s} {sorted(v.kinds)}  nonzero >= 2^{v.lo}  <= {v.hi:.4g} (2^{math.log2(v.hi):.1f})")
        return div(num_s, *cs), div(num_d, *cd)

    def combine(y, k1, k2, k3, k4):
        return add(y, mul(add(add(add(k1, mul(k2, two)), mul(k3, two)), k4), sixth))

    for s in range(n_sub):
        k1s, k1d = rhs(f"{s}.1", ts, td)
        k2s, k2d = rhs(f"{s}.2", add(ts, mul(k1s, half)), add(td, mul(k1d, half)))
        k3s, k3d = rhs(f"{s}.3", add(ts, mul(k2s, half)), add(td, mul(k2d, half)))
        k4s, k4d = rhs(f"{s}.4", add(ts, mul(k3s, h)), add(td, mul(k3d, h)))
        for nm, k in (("k2s", k2s), ("k2d", k2d), ("k3s", k3s), ("k3d", k3d)):
            if not 2.0 * k.hi < math.inf:
                raise ProofError(f"2*{nm} of sub-step {s} may overflow")
        ts, td = combine(ts, k1s, k2s, k3s, k4s), combine(td, k1d, k2d, k3d, k4d)
    return out


def check_pair_window(boxes=None, pair=None, surface_lo=None):
    """pair_div's numerator windows (pair_div_verdict.hpp) against what they need for divisors of the wide divisor box, and against
    the chunk guard: every numerator prove_chunk() admits must be +0 or inside its window -- the deep equation's in [2^kNumLo, 2^kNumHi),
    which holds for every divisor the verdict calls safe, the surface equation's in [2^kSurfaceNumFloor, 2^kNumHi), which the verdict is
    asked for by name.  The needs (rk4_device.hpp, "the pair window"): a tried non-zero zl is at least 2^(-105 - dhi - 1) in magnitude,
    so n zl is normal from 2^(-1022 + 105 + dhi + 1) on whatever the divisor; zh is at most 2^-dlo, so n zh stays finite below
    2^(1023 + dlo); zh is above 2^-dhi and so is 1/d, so n zh and the quotient are normal above 2^(-1022 + dhi)."""
    boxes = read_boxes(CHUNK_HEADER) if boxes is None else boxes
    lo, hi = read_boxes(PAIR_HEADER)["Num"] if pair is None else pair
    surface_lo = read_constants(PAIR_HEADER)["SurfaceNumFloor"] if surface_lo is None else surface_lo
    dlo, dhi = boxes["WideDiv"]
    if lo < -1022 + 105 + dhi + 1:
        raise ProofError(f"numerators down to 2^{lo}: n*zl may be denormal (zl as small as 2^{-105 - dhi - 1})")
    if hi - dlo >= 1023:
        raise ProofError(f"numerators up to 2^{hi}: n*zh may overflow")
    if min(lo, surface_lo) - dhi <= -1022:
        raise ProofError(f"quotients down to 2^{min(lo, surface_lo) - dhi} may be denormal")
    for nm, v in prove_chunk(boxes).items():
        check_numerator(nm, v, (surface_lo if nm.startswith("num_s") else lo, hi))
    return lo, hi, surface_lo


def main():
    boxes = read_boxes()
    for k, (lo, hi) in sorted(boxes.items()):
        print(f"{k:8s} [2^{lo}, 2^{hi})")
    try:
        prove(boxes, log=print)
    except ProofError as e:
        print(f"FAILED: {e}")
        return 1
    print("every numerator is +0 or inside [2^-511, 2^513); 2*k2 and 2*k3 are finite")
    chunk = read_boxes(CHUNK_HEADER)
    n_sub = read_constants(CHUNK_HEADER)["ChunkSubSteps"]
    print(f"\nchunks of {n_sub} sub-steps:")
    for k, (lo, hi) in sorted(chunk.items()):
        print(f"{k:8s} [2^{lo}, 2^{hi})")
    try:
        prove_chunk(chunk, log=print)
    except ProofError as e:
        print(f"FAILED: {e}")
        return 1
    lo, hi = chunk["WideNum"]
    print(f"every numerator of {n_sub} sub-steps is +0 or inside [2^{lo}, 2^{hi}); 2*k2 and 2*k3 are finite")
    try:
        lo, hi, slo = check_pair_window(chunk)
    except ProofError as e:
        print(f"FAILED: {e}")
        return 1
    print(f"... and inside pair_div's windows: [2^{lo}, 2^{hi}) for the deep equation's, [2^{slo}, 2^{hi}) for the surface equation's")
    return 0


if __name__ == "__main__":
    sys.exit(main())
