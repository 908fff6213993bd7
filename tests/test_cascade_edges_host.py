"""The cascades of tests/cascade_edges.py are what they claim to be (CPU only), so that a pass of
tests/test_gpu_cascade_edges.py means something: on which side of its bound each one lies (the load-time predicates
restated with exact integers), that the witness vote sequences separate the sequential sum from every other order,
that the weight features really round differently when fused or evaluated in integers, and that the oracle alone finds
enough ties, enough windows on both sides of every critical stage and tiles on both sides of the wave-phase limit."""
from fractions import Fraction

import numpy as np
import pytest

from oracle import oracle as orc
from tests import cascade_edges as ce

F32 = np.float32


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("cascade_edges")


@pytest.fixture(scope="module")
def refs(tmp):
    """name -> (oracle cascade, [oracle result per frame]); computed once per cascade."""
    cache = {}

    def get(name):
        if name not in cache:
            o = ce.oracle_cascade(tmp, name)
            cache[name] = (o, [orc.detect_raw(o, img, sf, nthreads=8, full=True) for img, sf in ce.frames(name)])
        return cache[name]
    return get


# ------------------------------------------------------------------ restated predicates: which side of the bound
def test_order_independence_bound_sides(tmp):
    """Critical-stage sum max(|l|,|r|) / q: just below 2^53 / 4, between 2^53 / 4 and 2^53, between 2^53 and 2^55 (where a
    headroom wrong by up to 16 would still let the delta form in), far above."""
    want = {"a_below_quarter": (Fraction(99, 100) * 2 ** 51, 2 ** 51), "a_between": (2 ** 51, 2 ** 53), "a_at_bound": (2 ** 53, 2 ** 55),
            "a_far_above": (2 ** 70, 2 ** 90)}
    for name, (lo, hi) in want.items():
        o = ce.oracle_cascade(tmp, name)
        crit = ce.built(name).critical
        ratio = ce.stage_ratio(o, crit)
        assert lo <= ratio < hi, (name, float(ratio))
        assert all(ce.stage_ratio(o, s) < 2 ** 45 for s in range(o.nstages) if s != crit), name  # only the critical stage decides
        assert ce.order_independent(o, 4) == (name == "a_below_quarter")
        assert ce.order_independent(o, 1) == (name in ("a_below_quarter", "a_between"))
    # the critical stage is last in one cascade of each kind and in the middle in the other
    assert [ce.built(n).critical == ce.built(n).nstages - 1 for n in ce.A_NAMES] == [True, False, True, False]


def test_int32_vote_bound_sides(tmp):
    want = {"b_below": 2 ** 31 - 2, "b_at": 2 ** 31 - 1, "b_above": 2 ** 31 + 2 ** 24 - 1}
    for name, ratio in want.items():
        o = ce.oracle_cascade(tmp, name)
        assert ce.order_independent(o, 4), name  # the delta form is on: only stage_quantum decides
        for s in (2, 3):
            mag, q = ce.stage_magnitude(o, s)
            assert q == Fraction(1, 2 ** 24) and mag / q == ratio, (name, s)
            assert ce.quantum_ok(o, s) == (name == "b_below")
        sl = ce.stage_slices(o)
        # stage 2: one sign throughout, so the sum reaches +-(sum max) on some vote pattern; stage 3 alternates
        l, r = o.stump_left[sl[2]], o.stump_right[sl[2]]
        forced = o.stump_threshold[sl[2]] > 1e38
        sign = -1 if name == "b_at" else 1
        assert (np.sign(l[forced]) == sign).all() and (np.sign(l[~forced]) == sign).all() and (np.sign(r[~forced]) == sign).all()
        assert sum(ce.exact(v) for v in np.where(forced, l, np.where(np.abs(l) > np.abs(r), l, r))) == sign * ratio * q
        v3 = np.where(o.stump_threshold[sl[3]] > 1e38, o.stump_left[sl[3]], o.stump_right[sl[3]])[:-4]
        assert (v3[0::2] == 1).all() and (v3[1::2] == -1).all()
        # stage 4: left and right of one sign and different magnitudes (max(|l|,|r|), the constant of the delta form)
        l4, r4 = o.stump_left[sl[4]], o.stump_right[sl[4]]
        assert ((np.sign(l4) * np.sign(r4) >= 0) & (np.abs(l4) != np.abs(r4))).all() and ce.quantum_ok(o, 4)


def test_weight_features_bound_sides():
    small, big = ce.c_features(75, 32), ce.c_features(128, 40)
    assert ce.int_form_ok(small["w64"]) and not ce.int_form_ok(small["w65"]) and ce.int_bound(small["w65"]) < 2 ** 24
    assert not ce.int_form_ok(small["frac"]) and [float(w) for w in small["frac"]["wt"]] == [2.5, -0.75, 0.0]
    assert ce.int_bound(big["below"]) == 2 ** 24 - 1 and ce.int_form_ok(big["below"])
    assert ce.int_bound(big["above"]) == 2 ** 24 + 254 and not ce.int_form_ok(big["above"])
    assert big["tilt_below"]["tilted"] and 2 ** 24 - 5000 < ce.int_bound(big["tilt_below"]) < 2 ** 24 and ce.int_form_ok(big["tilt_below"])
    assert big["tilt_above"]["tilted"] and 2 ** 24 <= ce.int_bound(big["tilt_above"]) < 2 ** 24 + 200000 and not ce.int_form_ok(big["tilt_above"])
    assert 2 ** 24 <= ce.int_bound(big["wide63"]) < 3.0e7  # inside a bound widened to 3e7
    for f in (small["tri"], big["tri_big"]):
        assert [float(w) for w in f["wt"]] == [63.0, -61.0, 59.0] and (f["r"][:, 2] * f["r"][:, 3] >= 1040).all() and not ce.int_form_ok(f)
    for f in (small["sat_odd"], big["sat_odd"], big["sat_odd2"]):  # one product on a saturated rectangle: odd and above 2^24
        p = int(abs(f["wt"][0])) * 255 * int(f["r"][0][2] * f["r"][0][3])
        assert p % 2 == 1 and 2 ** 24 < p < 2 ** 25 and f["wt"][0] == -f["wt"][1] and (f["r"][0][2:] == f["r"][1][2:]).all()


def test_tile16_features_bound_sides():
    f24, f44 = ce.d_features(24, 24), ce.d_features(44, 12)
    for f in f24["net128"] + f44["net128"]:
        assert ce.value_range(f, 44, 24) == (-32640, 32640)  # fits int16
    for f in f24["net129"] + f44["net129"]:
        assert ce.value_range(f, 44, 24)[1] == 32895          # does not: int16 holds up to 32767
    for f in f24["neg129"]:
        assert ce.value_range(f, 24, 24)[0] == -32895
    area = lambda f: int(f["r"][0][2] * f["r"][0][3])
    assert [area(f) for f in f24["area256"]] == [256, 256] and [area(f) for f in f24["area260"]] == [260, 260]
    assert area(f24["area264"][0]) == 264 and [area(f) for f in f44["area258"]] == [258, 258]
    assert 255 * 257 <= 65535 < 255 * 258  # the strip cutter's limit; 257 is prime, so no window the 16-bit tile accepts holds such a rectangle
    assert tuple(f24["row"][0]["r"][0]) == (0, 11, 24, 1) and tuple(f44["row"][0]["r"][0]) == (0, 5, 44, 1)


# ------------------------------------------------------------------ witnesses
@pytest.mark.parametrize("which", ["at_bound", "far_above"])
def test_witness_sequences_separate_the_sequential_sum(which):
    """For every vote pattern of the two calibrated stumps the sequential double sum differs from the reversed order, the
    pairwise tree, the strided split into 2 and 4 slices, the 64-lane tree per 64-stump chunk (detector and miner) and the
    delta form in 1 and 8 parts; where the two stumps cancel, the stage threshold lies between the sequential sum and all
    of the others, so the decision flips and not only the reported sum."""
    seq = ce.WITNESS_AT if which == "at_bound" else ce.WITNESS_FAR
    eff, seq_passes = ce.witness_threshold(seq)
    t = ce.WITNESS_TAIL
    for tail in ([t, t], [t, -t], [-t, t], [-t, -t]):
        votes = list(seq) + tail
        s = ce.sum_sequential(votes)
        others = ce.other_orders(votes, ce.witness_rights(seq))
        assert all(x != s for x in others.values()), (tail, s, others)
        if tail[0] != tail[1]:
            assert (s >= float(eff)) == seq_passes
            assert all((x >= float(eff)) != seq_passes for x in others.values()), (tail, s, float(eff), others)
    assert float(ce.effective_threshold(ce.stage_threshold_for(eff))) == float(eff)
    exact_sum = sum(Fraction(v) for v in seq)
    assert exact_sum != Fraction(ce.sum_sequential(seq))  # the CPU's own sum is a rounded one: only its order reproduces it


@pytest.mark.parametrize("name", ["c_75x32", "c_128x40"])
def test_weight_features_round_differently_when_fused_or_in_integers(name):
    """On the windows of the cascade's first frame (stride 5 x 3): the fused form changes the value of every feature whose
    products can exceed 2^24 on at least one window in a hundred, and so does the integer form on the integer-weight
    features outside int_ok. Shares found (fused, integer): 75x32 sat_odd 0.271, 0.079; tri 0.300, 0.336; 128x40 sat_odd
    0.267, 0.073; sat_odd2 0.270, 0.187; wide63 0.173, 0.173; tri_big 0.272, 0.315. Inside int_ok, and for w65 and frac whose
    products stay below 2^24 here, all three forms agree on every window."""
    b = ce.built(name)
    img = ce.frames(name)[0][0]
    ii = np.zeros((img.shape[0] + 1, img.shape[1] + 1), np.int64)
    ii[1:, 1:] = img.astype(np.int64).cumsum(0).cumsum(1)
    ys, xs = np.meshgrid(np.arange(0, img.shape[0] - b.H + 1, 3), np.arange(0, img.shape[1] - b.W + 1, 5), indexing="ij")
    ys, xs = ys.ravel(), xs.ravel()
    shares = {}
    for key, f in ce.c_features(b.W, b.H).items():
        if f["tilted"]:
            continue
        cols = []
        for j in range(3):
            if f["wt"][j] != 0:
                x, y, w, h = (int(v) for v in f["r"][j])
                cols.append(ii[ys + y + h, xs + x + w] - ii[ys + y, xs + x + w] - ii[ys + y + h, xs + x] + ii[ys + y, xs + x])
        sep, fused, whole = ce.haar_forms(f, np.stack(cols, 1))
        shares[key] = (float((sep != fused).mean()), None if whole is None else float((sep != whole).mean()))
    print(name, {k: tuple(None if x is None else round(x, 3) for x in v) for k, v in shares.items()})
    for key, (fu, wh) in shares.items():
        if key.startswith(("sat", "tri", "wide")):
            assert fu >= 0.01 and wh >= 0.01, (key, fu, wh)
        if ce.int_form_ok(ce.c_features(b.W, b.H)[key]):
            assert wh == 0.0, key  # inside int_ok the integer form is the float expression


def _first_scale(ref, o, img, sf):
    sc = orc.scales(o.win_w, o.win_h, img.shape[1], img.shape[0], sf)[0]
    n = int(sc["nx"]) * int(sc["ny"])
    return ref.codes[:n], ref.sums[:n]


@pytest.mark.parametrize("name", ["c_75x32", "c_int_edge"])
def test_fused_and_integer_forms_flip_decisions(refs, name):
    """Not only values: results. The oracle's walk is restated in numpy (emulate_first_scale) and equals the oracle on every
    window of the first scale; with the feature values fused, or in the integer form, codes or reported sums differ on at
    least 18 windows. Found: c_75x32 fused 710 windows (integer form 0: its only stump outside int_ok with integer weights
    above 2^24 is tri, on calibrated thresholds); c_int_edge integer form 18, every pasted reference window, fused 18."""
    o, results = refs(name)
    img, sf = ce.frames(name)[0]
    codes, sums = _first_scale(results[0], o, img, sf)
    c0, s0 = ce.emulate_first_scale(o, img, sf, 0)
    assert (c0 == codes).all() and (s0 == sums).all()
    differ = {}
    for form in (1, 2):
        c, s = ce.emulate_first_scale(o, img, sf, form)
        differ[form] = int(((c != c0) | (s != s0)).sum())
    print(name, differ)
    if name == "c_75x32":
        assert differ[1] >= 20
    else:
        assert differ[2] >= len(ce.INT_EDGE_SLOTS)
        nx = int(orc.scales(128, 40, img.shape[1], img.shape[0], sf)[0]["nx"])
        c2, s2 = ce.emulate_first_scale(o, img, sf, 2)
        at_slots = [(y // 2) * nx + x // 2 for (x, y) in ce.INT_EDGE_SLOTS]
        assert all(c2[i] != c0[i] or s2[i] != s0[i] for i in at_slots)  # every pasted reference window flips
        for f in ce.INT_EDGE:
            assert 2 ** 24 <= ce.int_bound(f) < 3.0e7 and not ce.int_form_ok(f) and all(float(w) == int(w) and abs(w) <= 64 for w in f["wt"])


def test_saturated_features_flip_decisions_when_fused(refs):
    """c_128x40 (tilted features beside them, so no full emulation): on the windows of the first scale that reach their stage,
    the sat_odd / sat_odd2 stumps with thresholds +-1e-30 decide differently when the products are fused. Found: 1 386 and
    346 (window, stump) pairs."""
    o, results = refs("c_128x40")
    img, sf = ce.frames("c_128x40")[0]
    codes, _ = _first_scale(results[0], o, img, sf)
    sc = orc.scales(128, 40, img.shape[1], img.shape[0], sf)[0]
    ys, xs = (v.ravel() for v in np.meshgrid(np.arange(int(sc["ny"])) * 2, np.arange(int(sc["nx"])) * 2, indexing="ij"))
    sl = ce.stage_slices(o)
    feats = ce.c_features(128, 40)
    for key in ("sat_odd", "sat_odd2"):
        flips = 0
        for s in range(o.nstages):
            for k in range(sl[s].start, sl[s].stop):
                f = o.haar[o.stump_feature[k]]
                if f != feats[key] or abs(o.stump_threshold[k]) > 1e-20:
                    continue
                (vf, vu, _), ok = ce.window_values(f, img, xs, ys, 128, 40)
                thr = o.stump_threshold[k]
                flips += int((ok & ce.reached(codes, s) & ((vf < thr) != (vu < thr))).sum())
        print(key, flips)
        assert flips >= 200, (key, flips)


# ------------------------------------------------------------------ what the oracle alone finds on the inputs
@pytest.mark.parametrize("name", ce.A_NAMES + ce.B_NAMES + ce.E_HAAR_NAMES + ce.E_LBP_NAMES + [ce.REFUSED])
def test_both_sides_of_the_critical_stage(refs, name):
    """At least 5 % of the windows that enter the critical stage pass it and at least 5 % fail it, on every frame (b: also
    the two stages behind it; stage-size cascades: every stage from 2 on). Shares of failing windows found: 0.084 (b_above, stage 3) to 0.906 (a_far_above)."""
    o, results = refs(name)
    crit = ce.built(name).critical
    stages = [crit] if name in ce.A_NAMES or "stages" in name else [crit, crit + 1, crit + 2] if name in ce.B_NAMES else range(2, o.nstages)
    for ref in results:
        for s in stages:
            entered = ce.reached(ref.codes, s)
            failed = ref.codes == -s
            n = int(entered.sum())
            assert n >= 500, (name, s, n)
            print(name, s, n, round(float(failed.sum() / n), 3))
            assert 0.05 <= failed.sum() / n <= 0.95, (name, s, n, int(failed.sum()))


@pytest.mark.parametrize("name", ce.A_NAMES + ["e_sizes_small", "e_sizes_large"])
def test_tiles_on_both_sides_of_the_wave_phase_limit(refs, name):
    """Per tile of 64 x 8 window origins, the windows that enter the critical stage: at least one tile holds 1 to 23 (the
    wave phase takes it) and one more than 24 (thread phase; its leftover row groups are split by stumps)."""
    o, results = refs(name)
    crit = ce.built(name).critical
    for (img, sf), ref in zip(ce.frames(name), results):
        for s in ([crit] if name in ce.A_NAMES else range(2, o.nstages)):
            t = ce.tile_counts(o, img, sf, ref.codes, s)
            assert ((t >= 1) & (t <= 23)).any() and (t > 24).any(), (name, s, sorted(t.tolist()))


# (accepted, rejected at stage 0, candidates) the oracle finds on the one-stage inputs. The LBP rows are the figures of the
# issue that asked for these cases; its Haar rows (7967 / 3472 / 7009 and 5793 / 5646 / 4571) came from calibration windows it
# does not specify and that no regular grid over the frame reproduces: the Haar cascades here are calibrated on
# ce.windows_of(frame, 24, 24), and these are their counts.
ONE_STAGE_COUNTS = {"g_one_stage_lbp_stump": (6225, 5214, 4362), "g_one_stage_lbp_tree": (4668, 6771, 3149),
                    "g_one_stage_haar_tree": (7735, 3704, 6753), "g_one_stage_tilted_stump": (6317, 5122, 5061)}


@pytest.mark.parametrize("name", ce.G_NAMES)
def test_one_stage_inputs(refs, name):
    """One stage, 11 439 grid windows: the oracle alone finds accepted windows, windows rejected at stage 0, and fewer
    candidates than accepted windows, so the stage-0 skip rule bites."""
    o, (ref,) = refs(name)
    assert o.nstages == 1 and ref.n_grid_windows == 11439 and len(ce.frames(name)) == 1
    got = (int((ref.codes == 1).sum()), int((ref.codes == 0).sum()), len(ref.candidates))
    assert got == ONE_STAGE_COUNTS[name], (name, got)
    accepted, rejected, candidates = got
    assert accepted > 0 and rejected > 0 and 0 < candidates < accepted
    assert accepted + rejected + int((ref.codes == -1).sum()) == 11439  # -1: no variance (Haar)


def _stage_ties(o, img, sf):
    """Windows whose stage sum equals the effective stage threshold exactly, per stage: the cascade cut after stage k accepts
    them with that sum."""
    out = []
    for k in range(o.nstages):
        ref = orc.detect_raw(ce.truncated(o, k), img, sf, nthreads=8, full=True)
        eff = np.float64(ce.effective_threshold(o.stage_threshold[k]))
        out.append(int(((ref.codes == 1) & (ref.sums == eff)).sum()))
    return out


@pytest.mark.parametrize("name", ce.F_NAMES)
def test_tie_inputs_tie(refs, name):
    """Every tie input (cascade, frame): at least 200 windows whose stage sum equals the stage threshold exactly, 50 of them
    before the last stage; the Haar ones at least 1000 (window, node) pairs with v == thr exactly. Found (first / second
    frame): f_node_ties 756 933 / 223 311 pairs, stage ties [38173, 5480, 8759, 4418] / [12051, 1191, 3390, 2177];
    f_node_ties_plain 815 997 / 264 630, [39783, 7028, 5129, 4358] / [12397, 2008, 2452, 2069]; f_stage_ties 738 463 / 179 675,
    [35540, 4941, 0, 0, 1530, 0] / [11147, 1207, 0, 0, 515, 0]; f_lbp_ties [13395, 7047, 0, 0, 471, 219] / [3329, 1705, 0, 0, 94, 55].
    The stages with 0 are those whose threshold sits one float32 ulp, or 1e-5, beside a reachable sum."""
    o, results = refs(name)
    for (img, sf), ref in zip(ce.frames(name), results):
        ties = _stage_ties(o, img, sf)
        pairs = ce.zero_value_pairs(o, img, sf, ref.codes) if o.feature_type == 0 else None
        print(name, sf, pairs, ties)
        assert sum(ties) >= 200 and sum(ties[:-1]) >= 50, (name, ties)
        if pairs is not None:
            assert pairs >= 1000, (name, pairs)
    sl = ce.stage_slices(o)
    if name.startswith("f_node_ties"):
        thr = o.stump_threshold[np.abs(o.stump_threshold) < 1e38]
        assert (thr == 0).all() and np.signbit(thr).sum() >= 8 and (~np.signbit(thr)).sum() >= 8  # -0.0 and 0.0
        # the delta form of the generated stages (v_cmpx_gt_f32) for one, the plain form (v < thr ? left : right) for the other
        assert ce.order_independent(o, 1) and ce.order_independent(o, 4) == (name == "f_node_ties")
        return
    effs = [ce.effective_threshold(t) for t in o.stage_threshold]  # one ulp above and one below a reachable sum, and 0.0
    grid = [float(e) * 8 == int(float(e) * 8) for e in effs]
    assert grid.count(False) >= 2 and grid.count(True) >= 2, effs
    if name == "f_stage_ties":
        assert float(effs[1]) == 0.0
        assert o.stage_threshold[5] == 0 and np.signbit(o.stage_threshold[5])  # a stageThreshold written as -0.0
    assert ce.order_independent(o, 4)
    for s in range(o.nstages):  # leaves in multiples of 2^-3
        assert (o.stump_left[sl[s]] * 8 == np.rint(o.stump_left[sl[s]] * 8)).all() and (o.stump_right[sl[s]] * 8 == np.rint(o.stump_right[sl[s]] * 8)).all()


def test_shape_limit_cascades(tmp):
    assert ce.oracle_cascade(tmp, "e_63_stages").nstages == 63 and ce.oracle_cascade(tmp, ce.REFUSED).nstages == 64
    for name, sizes in ce.E_SIZES.items():
        assert tuple(ce.oracle_cascade(tmp, name).stage_ntrees) == sizes
    assert sorted(set(ce.E_SIZES["e_sizes_small"] + ce.E_SIZES["e_sizes_large"])) == [1, 2, 3, 8, 63, 64, 65, 128, 129]
    for name, ((W, H), sizes) in ce.LBP_SIZES.items():
        o = ce.oracle_cascade(tmp, name)
        assert (o.win_w, o.win_h) == (W, H) and tuple(o.stage_ntrees) == sizes and o.feature_type == 1
    s64, s65 = ce.LBP_SIZES["e_lbp_64"][1], ce.LBP_SIZES["e_lbp_65"][1]
    assert 64 in s64 and s64[3] + s64[4] == 64 and s64[5:] == (14, 7, 7)                  # chunk of exactly 64; groups 14 | 7 + 7
    assert s65[2] + s65[3] == 65 and s65[4] == 15 and s65[5] + s65[6] == 15                # chunk boundary; 15 and 7 + 8 exceed the budget
    assert max(ce.LBP_SIZES["e_lbp_long"][1]) == 65 and max(s64) == 64 and max(s65) <= 64  # wave phase off / on
