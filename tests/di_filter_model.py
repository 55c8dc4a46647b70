"""An independent model of the double-integrator matrix-core prefilter (csrc/kernels_di_mfma.hip), in numpy / longdouble.

Derived from the identity in the kernel's header comment, not from csrc/di_mf_bound.h.  For states (p, v), P = 6 (p - p_c) / r^2 and
V = 2 v / r (p_c: the centre of the samples' box),

    Q(i -> j) = 36 a / r^4 - 24 b / r^3 + 4 c / r^2,   a = |p_j - p_i|^2, b = (p_j - p_i).(v_i + v_j), c = |v_i|^2 + v_i.v_j + |v_j|^2
              = |P_i + V_i|^2 + |P_j - V_j|^2 + P_j.(-2 P_i - 2 V_i) + V_j.(2 P_i + V_i)
              = n0_i + n1_j + sum_k f_k(j) g_k(i),      f = (P, V), g = (-2 (P + V), 2 P + V), n1 = sum (P - V)^2, n0 = sum (P + V)^2,

and dcost(r) = 1 - rho Q.  Every f, g, n is split into fp16 hi + lo (hi = fp16(x), lo = fp16(x - hi)) and the matrix core sums, per
pair, 16 products T_k S_k (T: the target's slots, S: the source's) on top of C = negT = -T:

    slot k = 0 .. 3      f_hi g_hi            (k = q m + i: q = 0 the P features, q = 1 the V features, i the workspace axis)
    slot 4 + k           f_hi g_lo
    slot 8 + k           f_lo g_hi            (the lo x lo product is dropped)
    slots 12, 13         n1_hi, n1_lo of the target against 1.0
    slots 14, 15         1.0 against n0_hi, n0_lo of the source

A pad state has no features; its norm is PAD_NORM in slot 12 (target role) / 14 (source role), above every threshold.

THE PER-VALUE ALLOWANCE  |x - hi - lo| <= d(x) = 2^-22 |x| + 6.2e-5, whatever the core does with subnormal inputs:
  * |x| >= 2^-14 (hi normal): |x - hi| <= 2^-11 |x| (round to nearest, 11 significand bits), and rem = x - hi is exact in fp64.
      - |rem| >= 2^-14: lo is normal, |rem - lo| <= 2^-11 |rem| <= 2^-22 |x|.
      - |rem| <  2^-14: lo is subnormal (spacing 2^-24): kept, the error is <= 2^-25; flushed to zero, it is |rem| < 2^-14.
  * |x| < 2^-14: hi is subnormal: kept, |x - hi| <= 2^-25 and lo = 0 or one more subnormal; flushed (hi and lo both), the error is |x| < 2^-14.
  2^-14 = 6.104e-5 <= 6.2e-5.  No value overflows: the model asserts every maximum below 65504 / (1 + 2^-11).

THE BOX-LEVEL BUDGET  B_box (b_box): the largest per-pair budget any two states of the box can have.  Per workspace axis i the box allows
|P_i| <= Pmax_i = (half extent of axis i) 6 / r^2 and |V_i| <= Vmax_i = max |v_i| 2 / r, so a feature slot has |f| <= fmax, |g| <= gmax with
(fmax, gmax) = (Pmax_i, 2 (Pmax_i + Vmax_i)) for a P slot and (Vmax_i, 2 Pmax_i + Vmax_i) for a V slot, and both norms are <= Nmax =
sum_i (Pmax_i + Vmax_i)^2.
  operand part.  Write f = f~ + ef, g = g~ + eg with f~ = f_hi + f_lo what the core sees, |ef| <= d(fmax), |eg| <= d(gmax).  Then
      f g - (f_hi g_hi + f_hi g_lo + f_lo g_hi) = ef g + f~ eg + f_lo g_lo,
  in magnitude <= d(fmax) gmax + (fmax + d(fmax)) d(gmax) + lf lg, with |f_lo| <= lf = 2^-11 fmax (1 + 2^-11) + 2^-24 (the remainder, rounded).
  The norms add d(Nmax) each.  The fp64 evaluation of the features and norms themselves (a handful of roundings at 2^-53 each on
  quantities bounded by the same maxima) is covered by 64 x 2^-53 (sum_k fmax gmax + 2 Nmax).
  accumulation part.  The products are exact in fp32 (two 11-bit significands).  ROUNDING MODEL: the 16 products and C are summed in at
  most 17 fp32 additions in any order and grouping, each losing at most 2^-23 of its result's magnitude (one unit in the last place:
  truncation; round-to-nearest loses half of that), and no partial sum exceeds A = sum_k |T_k S_k| + |C| in magnitude by more than the
  roundings themselves -- so the sum is off by at most 17 x 2^-23 A (16 additions sum 17 terms: the seventeenth covers the second
  order, (1 + 2^-23)^16 < 17 / 16).  Over the box  sum_k |T_k S_k| <= sum_slots (hh + hl + lh) + 2 (Nmax (1 + 2^-11) + ln) with
  hh = fmax gmax (1 + 2^-11)^2, hl = fmax (1 + 2^-11) lg, lh = lf gmax (1 + 2^-11), ln = 2^-11 Nmax (1 + 2^-11) + 2^-24.

THE PER-PAIR BUDGET  B_pair (b_pair) is the same two parts for one pair, the operand part COMPUTED from the operands actually used:
|sum_k T_k S_k - Q_exact| (longdouble: 64 significand bits, the sum of 16 exact products is off by 2^-60 of A at most), plus
17 x 2^-23 (sum_k |T_k S_k| + |negT|).
"""
import math

import numpy as np

LD = np.longdouble
PAD_NORM = 60000.0
TINY = 6.2e-5
U11 = 2.0 ** -11
ADD_ULP = 2.0 ** -23           # what one fp32 addition may lose of its result's magnitude (the bound's rounding model)
NADDS = 17


def box_centre(lo, hi, m):
    return 0.5 * (np.asarray(lo, np.float64)[:m] + np.asarray(hi, np.float64)[:m])


def features(X, m, r, pc):
    """fp64 features as the identity defines them, evaluated left to right without contraction: f [N, 2m], g [N, 2m], n1 [N], n0 [N]."""
    X = np.asarray(X, np.float64)
    sp, sv = 6.0 / (r * r), 2.0 / r
    P = (X[:, :m] - pc[None, :m]) * sp
    V = X[:, m:] * sv
    f = np.concatenate([P, V], axis=1)
    g = np.concatenate([-2.0 * (P + V), 2.0 * P + V], axis=1)
    n1 = np.zeros(len(X)); n0 = np.zeros(len(X))
    for i in range(m):
        n1 = n1 + (P[:, i] - V[:, i]) * (P[:, i] - V[:, i])
        n0 = n0 + (P[:, i] + V[:, i]) * (P[:, i] + V[:, i])
    return f, g, n1, n0


def split16(x):
    hi = np.asarray(x, np.float64).astype(np.float16)
    lo = (np.asarray(x, np.float64) - hi.astype(np.float64)).astype(np.float16)
    return hi, lo


def operands(X, m, r, pc, npad=None):
    """The sixteen slots of every state in both roles, fp16 [npad, 16] each; rows >= N are pad states."""
    N = len(X)
    npad = ((N + 63) // 64) * 64 if npad is None else npad
    f, g, n1, n0 = features(X, m, r, pc)
    T = np.zeros((npad, 16), np.float16); S = np.zeros((npad, 16), np.float16)
    fh, fl = split16(f); gh, gl = split16(g)
    k = 2 * m
    T[:N, 0:k] = fh; S[:N, 0:k] = gh
    T[:N, 4:4 + k] = fh; S[:N, 4:4 + k] = gl
    T[:N, 8:8 + k] = fl; S[:N, 8:8 + k] = gh
    T[:N, 12], T[:N, 13] = split16(n1)
    S[:N, 14], S[:N, 15] = split16(n0)
    T[:, 14:16] = 1.0; S[:, 12:14] = 1.0
    T[N:, 12] = PAD_NORM; S[N:, 14] = PAD_NORM
    return T, S


def q_exact(X, m, r, I, J):
    """Q(I -> J) in longdouble from the raw states, and the magnitudes (ta, |tb|, tc) of its three terms."""
    X = np.asarray(X, np.float64).astype(LD)
    rr = LD(r)
    p = X[J, :m] - X[I, :m]
    vi, vj = X[I, m:], X[J, m:]
    a = (p * p).sum(axis=1)
    b = (p * (vi + vj)).sum(axis=1)
    c = (vi * vi + vi * vj + vj * vj).sum(axis=1)
    ta, tb, tc = LD(36) * a / rr ** 4, LD(24) * b / rr ** 3, LD(4) * c / rr ** 2
    return ta - tb + tc, ta, np.abs(tb), tc


def slack(rho, ta, tb, tc):
    """The margin of the fp64 test behind the filter: a pair with rho Q < 1 + slack may reach the exact test, so the filter must keep it."""
    return LD(1e-9) * (LD(1) + LD(rho) * (ta + tb + tc))


def pair_terms(T, S, I, J):
    """The 16 products T_k(J) S_k(I) of the pairs (I -> J), exact in float64 (and in fp32)."""
    return T[J].astype(np.float64) * S[I].astype(np.float64)


def b_pair(terms, negT, Q):
    """(operand part, accumulation part) of the per-pair budget."""
    t = terms.astype(LD)
    op = np.abs(t.sum(axis=1) - Q)
    acc = LD(NADDS) * LD(ADD_ULP) * (np.abs(t).sum(axis=1) + LD(abs(float(negT))))
    return op, acc


def b_box(m, rho, r, lo, hi, negT):
    """(operand part, accumulation part) of the box-level budget: the module docstring has the derivation."""
    lo = np.asarray(lo, np.float64).astype(LD); hi = np.asarray(hi, np.float64).astype(LD)
    pc = box_centre(lo.astype(np.float64), hi.astype(np.float64), m).astype(LD)
    rr = LD(r)
    infl = LD(1) + LD(2.0 ** -50)
    Pmax = np.maximum(hi[:m] - pc, pc - lo[:m]) * LD(6) / (rr * rr) * infl
    Vmax = np.maximum(np.abs(lo[m:2 * m]), np.abs(hi[m:2 * m])) * LD(2) / rr * infl
    slots = [(Pmax[i], 2 * (Pmax[i] + Vmax[i])) for i in range(m)] + [(Vmax[i], 2 * Pmax[i] + Vmax[i]) for i in range(m)]
    Nmax = ((Pmax + Vmax) ** 2).sum()
    top = LD(65504.0) / (1 + LD(U11))
    in_range = bool(Nmax < top and all(f < top and g < top for f, g in slots))
    d = lambda x: LD(2.0 ** -22) * x + LD(TINY)                                       # noqa: E731
    low = lambda x: LD(U11) * x * (1 + LD(U11)) + LD(2.0 ** -24)                      # noqa: E731
    op = LD(0); A = LD(0); fg = LD(0)
    for f, g in slots:
        op += d(f) * g + (f + d(f)) * d(g) + low(f) * low(g)
        A += f * g * (1 + LD(U11)) ** 2 + f * (1 + LD(U11)) * low(g) + low(f) * g * (1 + LD(U11))
        fg += f * g
    op += 2 * d(Nmax) + LD(64) * LD(2.0 ** -53) * (fg + 2 * Nmax)
    A += 2 * (Nmax * (1 + LD(U11)) + low(Nmax))
    acc = LD(NADDS) * LD(ADD_ULP) * (A + LD(abs(float(negT))))
    return op, acc, in_range


# ---- three emulations of the accumulation.  terms17: float64 [n, 17], column 0 = C, in the order the emulation adds them ----

def with_c(terms, negT, order="slot"):
    t = np.concatenate([np.full((len(terms), 1), np.float64(negT)), terms], axis=1)
    if order == "descending":                                                        # largest magnitude first
        t = np.take_along_axis(t, np.argsort(-np.abs(t), axis=1, kind="stable"), axis=1)
    return t


def emul_seq_nearest(terms17):
    """fp32 additions one after the other, each rounded to nearest even."""
    t = terms17.astype(np.float32)
    assert np.array_equal(t.astype(np.float64), terms17)
    acc = t[:, 0].copy()
    for k in range(1, t.shape[1]):
        acc = acc + t[:, k]
    return acc


def _chop24(s, e):
    """s + e (s = fl64(a + b), e its exact residual) truncated toward zero to 24 significand bits."""
    bits = s.view(np.int64)
    mask = np.int64(~((1 << 29) - 1))
    t = (bits & mask).view(np.float64)
    back = (t == s) & (e != 0) & (np.sign(e) == -np.sign(s))                          # on the grid, the exact sum just inside it
    t2 = (bits - np.int64(1 << 29)).view(np.float64)
    return np.where(back, t2, t)


def emul_seq_truncate(terms17):
    """fp32 additions one after the other, each truncated toward zero (what an adder does that drops the bits shifted out on alignment)."""
    acc = terms17[:, 0].copy()
    for k in range(1, terms17.shape[1]):
        b = terms17[:, k]
        s = acc + b
        bb = s - acc
        e = (acc - (s - bb)) + (b - bb)
        acc = _chop24(np.ascontiguousarray(s), e)
    out = acc.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), acc)
    return out


def exact_sum(terms17):
    """The exact sum of every row, correctly rounded to float64 (math.fsum)."""
    return np.array([math.fsum(row) for row in terms17.tolist()])


def emul_exact_once(terms17):
    """The exact sum, rounded once to fp32 (nearest even)."""
    s = exact_sum(terms17)
    out = s.astype(np.float32)
    tie = (s.view(np.int64) & np.int64((1 << 29) - 1)) == np.int64(1 << 28)           # fl64(sum) halfway between two fp32 values
    for n in np.nonzero(tie)[0]:
        e = math.fsum(terms17[n].tolist() + [-s[n]])                                  # which side of the tie the exact sum lies on
        if e != 0.0:
            down = np.float64(s[n]).view(np.int64) & np.int64(~((1 << 29) - 1))
            lo_mag = down.view(np.float64)
            hi_mag = (down + np.int64(1 << 29)).view(np.float64)
            out[n] = np.float32(hi_mag if (e > 0) == (s[n] > 0) else lo_mag)
    return out


EMULATIONS = (("sequential, nearest", emul_seq_nearest), ("sequential, truncating", emul_seq_truncate), ("exact sum, one rounding", emul_exact_once))
