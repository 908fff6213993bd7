"""An exact-arithmetic witness of the node split search (section 6 of the C ABI).

Every other check of the split search compares with a transcription of the reference's loops. This module is written
from the definition of the criteria instead and does all of its arithmetic on Python integers: every float32 / float64
input is m * 2^e exactly, so after scaling a node's weights (and responses) by a common power of two all sums, squares
and products below are integers and a quality is an exact ratio of two integers. Floats appear only (1) to screen which
few candidates need an exact comparison, (2) for the rounding bound B, which is rounded up.

The criteria (L / R the two sides, W a sum of weights, S a sum of response * weight, c0 / c1 per-class weights):
  regression (LOGIT, GENTLE)  q = (S_L^2 W_R + S_R^2 W_L) / (W_L W_R)
  class, GINI                 q = ((l0^2 + l1^2) W_R + (r0^2 + r1^2) W_L) / (W_L W_R)
  class, MISCLASS             q = max(l0 + r1, l1 + r0)
  a class criterion other than GINI / MISCLASS means MISCLASS for DISCRETE boost and GINI otherwise.
The totals are the exact sums over the node, never weights[n], weights[n + 1] or node_value; check_totals() holds the
caller's totals to the exact ones separately.

Ordered variables: samples sorted by (value, tie key); boundary i (between sorted positions i and i + 1) is legal iff
float32(v[i]) + float32(2 * FLT_EPSILON) < v[i + 1] with the sum rounded to float32; ord_c = float32 (v[i] + v[i+1]) * 0.5f.

Categorical variables (256 categories). Key of a category: its mean response S_c / W_c (regression; 0 when
W_c <= DBL_EPSILON, so also for absent categories) or its class-1 weight (class). The reference moves categories from
right to left in increasing key order and never moves the last one. How skipped categories count: a category whose
weight is not above FLT_EPSILON (regression: W_c <= FLT_EPSILON, class: W_c < FLT_EPSILON) is skipped -- it is never
added to the left sums and never subtracted from the right sums, whichever side of the cut it lies on, yet it is put
into the reported left subset when an effective category after it is moved. So the quality of a reported subset is
that of the bipartition (effective categories of the subset | everything else), and regression / GINI cuts need
W_L > FLT_EPSILON and W_R > FLT_EPSILON. The order of categories with equal keys is whatever std::sort leaves, so
the witness treats it as open: the legal cuts it enumerates are those at boundaries between groups of equal key, and a
candidate that cuts inside a group is judged by its own exact quality. Every criterion is a convex function of the
left sums, and the members of a group of equal mean (or of class-1 weight 0) add collinear vectors, so a cut inside
such a group lies on a segment between the group's two boundary cuts and cannot beat both: q(lambda) <=
(1 - lambda) q_a + lambda q_b, with lambda at least (smallest member weight / group weight) away from either end.
`decided` uses that bound; groups of equal non-zero class-1 weight are not collinear and leave a variable undecided.

Rounding bound B on |double running-sum evaluation - exact|, u = 2^-53, N = n + 8 (ordered) or n + 520 (categorical:
n accumulations into categories, a division and a multiplication per category, up to 256 additions for each total and
256 moves). A running sum of at most N non-negative terms, each the product of two floats, has relative error
<= N u: d(W_L) = N u W_L, d(S_L) = N u A_L with A the sum of |response * weight|. The right sums start from a total
(itself a rounded sum: error N u W_tot, N u A_tot) and subtract up to N terms, every intermediate bounded by the
total plus what was subtracted: d(W_R) = N u Rbar, Rbar = 2 W_tot + W_L; d(S_R) = N u Abar, Abar = 2 A_tot + A_L.
Propagated through q = S_L^2 / W_L + S_R^2 / W_R:
  regression  B = 2 [ (2|S_L| dS_L + dS_L^2) / W_L + (|S_L| + dS_L)^2 dW_L / W_L^2
                    + (2|S_R| dS_R + dS_R^2) / W_R + (|S_R| + dS_R)^2 dW_R / W_R^2 ] + 16 u q
  GINI        the same shape with S^2 replaced by a = l0^2 + l1^2 (da = 2 N u a, positive terms) and b = r0^2 + r1^2
              (db = 6 N u (c0_tot^2 + c1_tot^2): each r_k carries N u (2 c_k,tot + l_k) and enters as 2 r_k dr_k)
  MISCLASS    B = 2 N u (W_L + Rbar) + 4 u q
The leading 2 covers the second-order terms of the quotient, valid while dW_R / W_R < 2^-12; beyond that B is infinite
(the double evaluation itself has lost the cut, reported as `toothless`). 16 u q covers the <= 8 operations of the
final expression, all on non-negative terms. The constants come from this count, not from any observed result.

Verdict on a candidate (split point or subset, float quality) of one variable, see Node.verdict_*:
 (a) the split point is a legal boundary / the subset is a down-set of the key order over all 256 categories, is not
     everything, and its effective part is a legal cut; keys closer than their own double rounding count as equal;
 (b) float32 round-down(exact quality of that split - B) <= quality <= float32 round-up(exact + B);
 (c) that exact quality >= exact maximum over legal splits - (B + B_max);
 (d) if the variable is decided (the maximum exceeds every other legal split by more than the sum of their B, and every
     cut inside a tie group by the convexity bound) the split is the exact argmax, and ord_c is bit-equal;
 (e) "no split" is right iff no legal split exists (a lone effective category under MISCLASS that ties with the absent
     ones may or may not be moved: either answer passes).
"""
from fractions import Fraction

import numpy as np

FLT_EPSILON = np.float32(1.1920929e-07)
U = 2.0 ** -53
DISCRETE, REAL, LOGIT, GENTLE = 0, 1, 2, 3
GINI, MISCLASS = 1, 3
NCAT = 256
INF = float("inf")


def _exact_ints(a):
    """floats -> (object array of ints, D) with a[i] == ints[i] / D exactly, D a power of two."""
    ratios = [float(x).as_integer_ratio() for x in a]
    D = max([d for _, d in ratios] + [1])
    return np.array([p * (D // d) for p, d in ratios] + [None], dtype=object)[:-1], D


def _f32_down(x: Fraction) -> np.float32:
    with np.errstate(over="ignore"):
        f = np.float32(float(x))
    while Fraction(float(f)) > x:
        f = np.nextafter(f, np.float32(-np.inf))
    return f


def _f32_up(x: Fraction) -> np.float32:
    with np.errstate(over="ignore"):
        f = np.float32(float(x))
    while Fraction(float(f)) < x:
        f = np.nextafter(f, np.float32(np.inf))
    return f


def effective_criterion(boost_type, split_criteria):
    if boost_type in (LOGIT, GENTLE):
        return "reg"
    if split_criteria not in (GINI, MISCLASS):
        split_criteria = MISCLASS if boost_type == DISCRETE else GINI
    return "gini" if split_criteria == GINI else "misclass"


def subset_to_set(subset) -> frozenset:
    bits = np.asarray(subset, np.int32).view(np.uint32)
    return frozenset(c for c in range(NCAT) if (int(bits[c >> 5]) >> (c & 31)) & 1)


class Node:
    def __init__(self, vals, weights, *, tie_key=None, responses=None, class_labels=None, boost_type=GENTLE,
                 split_criteria=0, categorical=False):
        self.vals = np.ascontiguousarray(vals, np.float32)
        self.F, self.n = self.vals.shape
        n = self.n
        self.tie = np.arange(n) if tie_key is None else np.asarray(tie_key)
        self.categorical = categorical
        self.crit = effective_criterion(boost_type, split_criteria)
        wts = np.asarray(weights, np.float64)[:n]
        assert (wts > 0).all(), "the witness expects positive sample weights"
        self.w, self.Dw = _exact_ints(wts)
        if self.crit == "reg":
            r, self.Dr = _exact_ints(np.asarray(responses, np.float32))
            t = r * self.w
            self.comps = (self.w, t, np.array([abs(x) for x in t] + [None], dtype=object)[:-1])
            self.K = self.Dw * self.Dr * self.Dr  # q = num / den / K
            self.scales = (self.Dw, self.Dw * self.Dr, self.Dw * self.Dr)
        else:
            lab = np.asarray(class_labels)
            assert ((lab == 0) | (lab == 1)).all()
            zero = np.array([0] * n + [None], dtype=object)[:-1]
            self.comps = (np.where(lab == 0, self.w, zero), np.where(lab == 1, self.w, zero))
            self.K = self.Dw
            self.scales = (self.Dw, self.Dw)
        self.tot = tuple(sum(c.tolist()) for c in self.comps)
        self.N = n + (520 if categorical else 8)
        self._cache = {}

    # ---------------------------------------------------------------- totals
    def check_totals(self, weights, node_value=0.0):
        """The caller's totals (weights[n], weights[n+1], node_value * weights[n]) against the exact ones, each to the
        error of a rounded sum of n terms (and three more roundings for node_value * R)."""
        n, Nu = self.n, self.N * U
        if self.crit == "reg":
            Wt, St, At = (Fraction(x, s) for x, s in zip(self.tot, self.scales))
            assert abs(Fraction(float(weights[n])) - Wt) <= Fraction(Nu) * Wt, "weights[n] is not the node's weight"
            got = Fraction(float(node_value)) * Fraction(float(weights[n]))
            assert abs(got - St) <= Fraction(2 * Nu) * At, "node_value * weights[n] is not the node's response sum"
        else:
            for k in (0, 1):
                ck = Fraction(self.tot[k], self.Dw)
                assert abs(Fraction(float(weights[n + k])) - ck) <= Fraction(Nu) * ck, f"weights[n+{k}] is not class {k}'s weight"

    # ---------------------------------------------------------------- the criteria
    def _evaluate(self, left):
        """left: object arrays of exact left sums, one entry per cut. -> num, den (q = num / den / K exactly; den == 0
        where a side is empty), qf (float approximation), B (float, rounded up)."""
        Nu = self.N * U
        m = len(left[0])
        f = lambda arr, s: np.array([x / s for x in arr], np.float64).reshape(m)
        if self.crit == "misclass":
            l0, l1 = left
            r0, r1 = self.tot[0] - l0, self.tot[1] - l1
            a, b = l0 + r1, l1 + r0
            num = np.where(a > b, a, b) if m else a
            den = np.array([1] * m + [None], dtype=object)[:-1]
            qf = f(num, self.K)
            Wt = (self.tot[0] + self.tot[1]) / self.Dw
            Lf = f(l0 + l1, self.Dw)
            B = 2 * Nu * (Lf + 2 * Wt + Lf) + 4 * U * qf
            return num, den, qf, B * (1 + 1e-9)
        if self.crit == "reg":
            L, SL, AL = left
            R, SR = self.tot[0] - L, self.tot[1] - SL
            num = SL * SL * R + SR * SR * L
            den = L * R
            Lf, Rf = f(L, self.Dw), f(R, self.Dw)
            sl, sr, al = np.abs(f(SL, self.scales[1])), np.abs(f(SR, self.scales[1])), f(AL, self.scales[1])
            Wt, At = self.tot[0] / self.Dw, self.tot[2] / self.scales[1]
            dsl, dsr = Nu * al, Nu * (2 * At + al)
            dL, dR = Nu * Lf, Nu * (2 * Wt + Lf)
            with np.errstate(divide="ignore", invalid="ignore"):
                qf = np.array([(x / (y * self.K)) if y else np.nan for x, y in zip(num, den)], np.float64).reshape(m)
                B = 2 * ((2 * sl * dsl + dsl * dsl) / Lf + (sl + dsl) ** 2 * dL / Lf ** 2
                         + (2 * sr * dsr + dsr * dsr) / Rf + (sr + dsr) ** 2 * dR / Rf ** 2) + 16 * U * qf
                B = np.where(dR / Rf < 2.0 ** -12, B, INF)
            return num, den, qf, B * (1 + 1e-9)
        l0, l1 = left
        r0, r1 = self.tot[0] - l0, self.tot[1] - l1
        L, R = l0 + l1, r0 + r1
        a, b = l0 * l0 + l1 * l1, r0 * r0 + r1 * r1
        num = a * R + b * L
        den = L * R
        Lf, Rf = f(L, self.Dw), f(R, self.Dw)
        af, bf = f(a, self.Dw ** 2), f(b, self.Dw ** 2)
        Wt = (self.tot[0] + self.tot[1]) / self.Dw
        T2 = (self.tot[0] ** 2 + self.tot[1] ** 2) / self.Dw ** 2
        da, db = 2 * Nu * af, 6 * Nu * T2
        dL, dR = Nu * Lf, Nu * (2 * Wt + Lf)
        with np.errstate(divide="ignore", invalid="ignore"):
            qf = np.array([(x / (y * self.K)) if y else np.nan for x, y in zip(num, den)], np.float64).reshape(m)
            B = 2 * (da / Lf + (af + da) * dL / Lf ** 2 + db / Rf + (bf + db) * dR / Rf ** 2) + 16 * U * qf
            B = np.where(dR / Rf < 2.0 ** -12, B, INF)
        return num, den, qf, B * (1 + 1e-9)

    def _q(self, ev, i) -> Fraction:
        return Fraction(int(ev[0][i]), int(ev[1][i]) * self.K)

    def _limit_value(self) -> float:
        """The criterion with everything on one side (what a cut tends to as a side empties)."""
        if self.crit == "reg":
            return float(Fraction(self.tot[1] ** 2, self.tot[0] * self.K))
        if self.crit == "gini":
            return float(Fraction(self.tot[0] ** 2 + self.tot[1] ** 2, (self.tot[0] + self.tot[1]) * self.K))
        return max(self.tot) / self.K

    def _argmax_and_decided(self, ev, legal_idx, extra_upper=()):
        """Exact first argmax over the cuts legal_idx of ev, and whether it beats every other by more than the sum of
        the two bounds (and every value of extra_upper, float upper bounds of cuts not enumerated, by 2 B)."""
        num, den, qf, B = ev
        qs = qf[legal_idx]
        top = qs.max()
        near = [i for i in legal_idx if qf[i] >= top - 1e-9 * abs(top)]
        best = near[0]
        qbest = self._q(ev, best)
        for i in near[1:]:
            qi = self._q(ev, i)
            if qi > qbest:
                best, qbest = i, qi
        decided = np.isfinite(B[best])
        if decided:
            for i in legal_idx:
                if i == best:
                    continue
                slack = B[best] + B[i]
                if not qf[best] - qf[i] > 2 * slack + 1e-9 * abs(top):  # not clear in floats: compare exactly
                    if not (np.isfinite(slack) and qbest - self._q(ev, i) > Fraction(float(slack))):
                        decided = False
                        break
        if decided:
            for ub in extra_upper:
                if not qf[best] - ub > 2 * B[best] + 1e-9 * abs(top):
                    decided = False
        return best, qbest, bool(decided)

    # ---------------------------------------------------------------- ordered variables
    def ordered(self, f):
        if f in self._cache:
            return self._cache[f]
        v = self.vals[f]
        order = np.lexsort((self.tie, v))
        sv = v[order]
        with np.errstate(over="ignore", invalid="ignore"):
            legal = (sv[:-1] + np.float32(2) * FLT_EPSILON) < sv[1:]
            assert (sv[:-1] + np.float32(2) * FLT_EPSILON).dtype == np.float32
            mid = (sv[:-1] + sv[1:]) * np.float32(0.5)
        idx = np.nonzero(legal)[0]
        a = {"order": order, "sv": sv, "legal": legal, "idx": idx, "ord_c": mid, "pos": {int(p): k for k, p in enumerate(idx)}}
        if len(idx):
            left = tuple(np.cumsum(c[order])[idx] for c in self.comps)
            ev = self._evaluate(left)
            k, qbest, decided = self._argmax_and_decided(ev, list(range(len(idx))))
            a.update(ev=ev, best=int(idx[k]), qbest=qbest, Bbest=float(ev[3][k]), decided=decided)
        self._cache[f] = a
        return a

    def verdict_ordered(self, f, point, quality, ord_c=None, quality64=None):
        """-> (list of failures, info). quality: the float32 the search reports (-1 with point < 0 for "no split");
        quality64: its unrounded double, if it hands one out, held to exact +- B as it is. info["toothless"] marks a
        cut whose B is infinite and which therefore passes (b) and (c) unchecked: callers count them."""
        a = self.ordered(f)
        fails, info = [], {"decided": a.get("decided", False), "has_split": len(a["idx"]) > 0, "toothless": False}
        if point < 0:
            if len(a["idx"]):
                fails.append(f"(e) var {f}: no split reported, {len(a['idx'])} legal boundaries, exact best {float(a['qbest'])!r} at {a['best']}")
            return fails, info
        if not len(a["idx"]):
            return [f"(e) var {f}: split {point} reported but no boundary is legal"], info
        if point not in a["pos"]:
            return [f"(a) var {f}: split point {point} is not a legal boundary"], info
        k = a["pos"][point]
        q, B = self._q(a["ev"], k), float(a["ev"][3][k])
        info.update(B=B, q=float(q), Bbest=a["Bbest"], err=abs(Fraction(float(quality)) - q), toothless=not np.isfinite(B))
        fails += self._check_64(f"var {f} split {point}", q, B, quality64, info)
        fails += self._check_bcd(f"var {f} split {point}", q, B, quality, a["qbest"], a["Bbest"], a["decided"], point == a["best"],
                                 f"exact argmax {a['best']}")
        if ord_c is not None and np.float32(ord_c).view(np.uint32) != a["ord_c"][point].view(np.uint32):
            fails.append(f"(d) var {f}: ord_c {ord_c!r} != float32 midpoint {a['ord_c'][point]!r} of split {point}")
        return fails, info

    def _check_bcd(self, what, q, B, quality, qbest, Bbest, decided, is_best, best_txt):
        fails = []
        if not np.isfinite(B):
            return fails  # toothless cut: the double evaluation itself is meaningless here; counted by the caller
        lo, hi = _f32_down(q - Fraction(B)), _f32_up(q + Fraction(B))
        if not lo <= np.float32(quality) <= hi:
            fails.append(f"(b) {what}: reported quality {float(quality)!r} outside [{float(lo)!r}, {float(hi)!r}], exact {float(q)!r}, B {B:.3g}")
        if np.isfinite(Bbest) and q < qbest - Fraction(B + Bbest):
            fails.append(f"(c) {what}: exact quality {float(q)!r} is below the exact maximum {float(qbest)!r} ({best_txt}) by more than {B + Bbest:.3g}")
        if decided and not is_best:
            fails.append(f"(d) {what}: the variable is decided and the split is not the {best_txt}")
        return fails

    # ---------------------------------------------------------------- categorical variables
    def categories(self, f):
        if ("c", f) in self._cache:
            return self._cache[("c", f)]
        codes = self.vals[f].astype(np.int64)
        assert ((codes >= 0) & (codes < NCAT)).all()
        nc = len(self.comps)
        sums = [[0] * nc for _ in range(NCAT)]
        cols = [c.tolist() for c in self.comps]
        for i, c in enumerate(codes.tolist()):
            s = sums[c]
            for k in range(nc):
                s[k] += cols[k][i]
        reg = self.crit == "reg"
        Wc = [s[0] if reg else s[0] + s[1] for s in sums]
        eps23 = 1 << 23  # FLT_EPSILON = 2^-23
        eff = [(w * eps23 > self.Dw) if reg else (w * eps23 >= self.Dw) for w in Wc]
        if reg:
            key = [Fraction(s[1], s[0]) if s[0] * (1 << 52) > self.Dw else Fraction(0) for s in sums]
            tol = [4 * self.N * U * (s[2] / s[0] / self.Dr) if s[0] else 0.0 for s in sums]
            key_f = [float(k) / self.Dr for k in key]
        else:
            key = [s[1] for s in sums]
            tol = [2 * self.N * U * s[1] / self.Dw for s in sums]
            key_f = [k / self.Dw for k in key]
        order = sorted(range(NCAT), key=lambda c: (key[c], c))
        groups = []
        for c in order:
            if groups and key[groups[-1][0]] == key[c]:
                groups[-1].append(c)
            else:
                groups.append([c])
        # cuts at group boundaries, one per group (but the last) that adds an effective category
        cuts, run, moved = [], [0] * nc, []
        for g, members in enumerate(groups[:-1]):
            new = [c for c in members if eff[c]]
            if not new:
                continue
            for c in new:
                for k in range(nc):
                    run[k] += sums[c][k]
            moved = moved + new
            cuts.append({"group": g, "left": tuple(run), "E": frozenset(moved)})
        a = {"sums": sums, "Wc": Wc, "eff": eff, "key": key, "key_f": key_f, "tol": tol, "groups": groups, "cuts": cuts,
             "present": [c for c in range(NCAT) if Wc[c] > 0], "n_eff": sum(eff)}
        if cuts:
            ev = self._evaluate(tuple(np.array([c["left"][k] for c in cuts] + [None], dtype=object)[:-1] for k in range(nc)))
            legal = [i for i, c in enumerate(cuts) if self._legal_cut(c["left"])]
            a.update(ev=ev, legal=legal)
            if legal:
                k, qbest, decided = self._argmax_and_decided(ev, legal, self._ingroup_upper(a))
                if self._open_groups(a):
                    decided = False
                a.update(best=k, qbest=qbest, Bbest=float(ev[3][k]), decided=decided)
        # does the reference find any split? yes with a legal boundary cut; cuts inside a group can add some
        if a.get("legal"):
            a["has_split"] = True
        else:
            a["has_split"] = self._ingroup_only(a)
        self._cache[("c", f)] = a
        return a

    def _legal_cut(self, left):
        if self.crit == "misclass":
            return True
        L = left[0] if self.crit == "reg" else left[0] + left[1]
        Wt = self.tot[0] if self.crit == "reg" else self.tot[0] + self.tot[1]
        return L * (1 << 23) > self.Dw and (Wt - L) * (1 << 23) > self.Dw

    def _open_groups(self, a):
        """Tie groups with two or more effective members whose vectors are not collinear (equal non-zero class-1 weight)."""
        if self.crit == "reg":
            return False
        return any(a["key"][g[0]] != 0 and sum(a["eff"][c] for c in g) >= 2 for g in a["groups"])

    def _ingroup_upper(self, a):
        """Float upper bounds of the cuts inside collinear tie groups, from convexity (module docstring)."""
        ups = []
        qf = a["ev"][2]
        by_group = {c["group"]: i for i, c in enumerate(a["cuts"])}
        lim = self._limit_value()
        prev = lim  # value of the cut before the first group: nothing on the left
        for g, members in enumerate(a["groups"]):
            effm = [c for c in members if a["eff"][c]]
            if g in by_group and np.isfinite(qf[by_group[g]]):
                after = qf[by_group[g]]
            elif effm:
                after = lim  # the last group: everything on the left
            else:
                after = prev
            if len(effm) >= 2:
                ws = [a["Wc"][c] for c in effm]
                lam = min(ws) / sum(ws)
                ups.append(max((1 - lam) * prev + lam * after, lam * prev + (1 - lam) * after))
            prev = after
        return ups

    def _ingroup_only(self, a):
        """No legal boundary cut: True / False / None (open) for whether the reference still finds a split."""
        n_eff = a["n_eff"]
        if n_eff == 0:
            return False
        if self.crit != "misclass":
            # a cut needs effective weight on both sides beyond FLT_EPSILON; with one tie group holding all effective
            # categories the cuts inside it are legal whenever it has two members
            return n_eff >= 2
        if n_eff >= 2:
            return True
        c = [c for c in range(NCAT) if a["eff"][c]][0]
        g = [g for g in a["groups"] if c in g][0]
        if g is a["groups"][-1]:
            return None if len(g) > 1 else False  # moved only if std::sort does not leave it last
        return True

    def _left_sums(self, a, E):
        nc = len(self.comps)
        return tuple(sum(a["sums"][c][k] for c in E) for k in range(nc))

    def _eval_left(self, left):
        return self._evaluate(tuple(np.array([x, None], dtype=object)[:1] for x in left))

    def verdict_categorical(self, f, quality, subset=None, count=None, quality64=None):
        """The candidate is a subset (bit mask of 8 int32) or, where a search reports no more, the number of categories
        sent left (`count`). quality64: the search's unrounded double, if it hands one out, held to exact +- B as it is.
        -> (failures, info); info["weak"] marks a count whose left sums could not be identified, info["toothless"] a
        cut whose B is infinite: both pass (b) unchecked, so callers count them."""
        a = self.categories(f)
        fails, info = [], {"decided": a.get("decided", False), "has_split": a["has_split"], "weak": False, "toothless": False}
        none = (subset is None and (count is None or count <= 0))
        if none:
            if a["has_split"]:
                fails.append(f"(e) var {f}: no split reported but {len(a.get('legal', []))} legal cuts exist")
            return fails, info
        if a["has_split"] is False:
            return [f"(e) var {f}: a split is reported but no legal cut exists"], info
        if subset is not None:
            S = subset_to_set(subset)
            if len(S) == NCAT or not S:
                return [f"(a) var {f}: the subset holds {len(S)} categories"], info
            kin = max(S, key=lambda c: a["key"][c])
            kout = min((c for c in range(NCAT) if c not in S), key=lambda c: a["key"][c])
            if a["key"][kin] > a["key"][kout] and a["key_f"][kin] - a["key_f"][kout] > a["tol"][kin] + a["tol"][kout]:
                return [f"(a) var {f}: category {kin} (key {a['key_f'][kin]!r}) is left, {kout} (key {a['key_f'][kout]!r}) is not"], info
            lefts, complete = [self._left_sums(a, [c for c in S if a["eff"][c]])], True
        else:
            lefts, complete = self._sums_of_count(a, count)
            if not lefts and complete:
                return [f"(a) var {f}: no down-set of {count} categories ends on an effective category"], info
        matched = None
        for left in lefts:
            if not any(left):
                continue
            ev = self._eval_left(left)
            if not self._legal_cut(left) or not ev[1][0]:
                continue
            q, B = self._q(ev, 0), float(ev[3][0])
            if not np.isfinite(B):
                matched = (left, q, B)
                break
            if _f32_down(q - Fraction(B)) <= np.float32(quality) <= _f32_up(q + Fraction(B)):
                matched = (left, q, B)
                break
            if matched is None:
                matched = (left, q, B, "miss")
        if not complete and (matched is None or len(matched) == 4):  # too many sums to list: only the maximum can be checked
            info["weak"] = True
            if "qbest" in a and np.isfinite(a["Bbest"]):
                if np.float32(quality) < _f32_down(a["qbest"] - Fraction(2 * a["Bbest"])):
                    fails.append(f"(c) var {f}: quality {float(quality)!r} of a {count}-category cut is below the exact maximum {float(a['qbest'])!r}")
                if a["decided"]:
                    fails.append(f"(d) var {f}: decided, and {count} categories are not the exact argmax")
            return fails, info
        if matched is None:
            return [f"(a) var {f}: the effective part of the left set is not a legal cut"], info
        left, q, B = matched[:3]
        info.update(B=B, q=float(q), err=abs(Fraction(float(quality)) - q), toothless=not np.isfinite(B))
        fails += self._check_64(f"var {f}", q, B, quality64, info)
        what = f"var {f} left sums {[x / sc for x, sc in zip(left, self.scales)]}"
        if "qbest" not in a:
            if np.isfinite(B) and len(matched) == 4:
                fails.append(f"(b) {what}: reported quality {float(quality)!r}, exact {float(q)!r}, B {B:.3g}")
            return fails, info
        info["Bbest"] = a["Bbest"]
        best = a["cuts"][a["best"]]
        fails += self._check_bcd(what, q, B, quality, a["qbest"], a["Bbest"], a["decided"], tuple(left) == tuple(best["left"]),
                                 f"exact argmax {sorted(best['E'])}")
        return fails, info

    def _check_64(self, what, q, B, quality64, info):
        if quality64 is None or not np.isfinite(B):
            return []
        err = abs(Fraction(float(quality64)) - q)
        info["err64"] = float(err)
        if err > Fraction(B):
            return [f"(b) {what}: the double quality {float(quality64)!r} is {float(err):.3g} from the exact {float(q)!r}, B {B:.3g}"]
        return []

    MAX_SUMS = 100000

    def _sums_of_count(self, a, k):
        """Effective left sums a reported count of k left categories can stand for (the order inside a group of equal
        keys is open), the boundary cut first, and whether the list is complete (False: more than MAX_SUMS distinct
        sums). Distinct sums, not sets: with one weight per class thousands of sets share a few hundred sums."""
        nc = len(self.comps)
        cum = 0
        before = (0,) * nc
        add = lambda x, c: tuple(x[i] + a["sums"][c][i] for i in range(nc))
        for g, members in enumerate(a["groups"]):
            effm = [c for c in members if a["eff"][c]]
            if k <= cum + len(members):
                t = k - cum
                p, z = len(effm), len(members) - len(effm)
                if g == len(a["groups"]) - 1 and t == len(members):
                    return [], True  # the last category is never moved
                lo, hi = max(1, t - z), min(p, t)
                if lo > hi:
                    return [], True
                out = []
                if hi == p:  # the whole group first: a boundary cut
                    whole = before
                    for c in effm:
                        whole = add(whole, c)
                    out.append(whole)
                    if lo == p:
                        return out, True
                layers = [{before}] + [set() for _ in range(hi)]  # layers[j]: sums of j members
                states = 1
                for c in effm:
                    for j in range(hi - 1, -1, -1):
                        new = {add(x, c) for x in layers[j]} - layers[j + 1]
                        layers[j + 1] |= new
                        states += len(new)
                    if states > self.MAX_SUMS:
                        return out, False
                for j in range(hi, lo - 1, -1):
                    out += [x for x in layers[j] if x not in out[:1]]
                return out, True
            cum += len(members)
            for c in effm:
                before = add(before, c)
        return [], True

    def best_bipartition(self, f, max_present=12):
        """Regression: exact maximum over ALL bipartitions of the effective categories (None beyond max_present)."""
        a = self.categories(f)
        effc = [c for c in range(NCAT) if a["eff"][c]]
        if self.crit != "reg" or len(effc) > max_present or len(effc) < 2:
            return None
        best = None
        first, rest = effc[0], effc[1:]
        for mask in range(1 << len(rest)):  # `first` stays right: each bipartition once
            E = [c for b, c in enumerate(rest) if mask >> b & 1]
            if not E:
                continue
            left = self._left_sums(a, E)
            ev = self._eval_left(left)
            if self._legal_cut(left) and ev[1][0]:
                q = self._q(ev, 0)
                if best is None or q > best:
                    best = q
        return best


def check_winner(result, q32, points, categorical):
    """The winner over variables from the candidate's own per-variable float qualities: the first variable holding the
    largest one; found iff it is > 0. result: dict / record with found, var_idx, quality, split_point, subset."""
    fails = []
    best, var = np.float32(-1), -1
    for f in range(len(q32)):
        if points[f] >= 0 and np.float32(q32[f]) > best:
            best, var = np.float32(q32[f]), f
    found = var >= 0 and best > 0
    if bool(result["found"]) != bool(found):
        return [f"winner: found {bool(result['found'])}, but the largest per-variable quality is {float(best)!r}"]
    if not found:
        return fails
    if int(result["var_idx"]) != var:
        fails.append(f"winner: variable {int(result['var_idx'])} reported, first largest quality {float(best)!r} is at {var}")
    elif np.float32(result["quality"]) != best:
        fails.append(f"winner: quality {float(result['quality'])!r} != its per-variable entry {float(best)!r}")
    elif categorical:
        if len(subset_to_set(result["subset"])) - 1 != int(points[var]):
            fails.append(f"winner: subset of {len(subset_to_set(result['subset']))} categories, per-variable entry {int(points[var])}")
    elif int(result["split_point"]) != int(points[var]):
        fails.append(f"winner: split point {int(result['split_point'])} != its per-variable entry {int(points[var])}")
    return fails
