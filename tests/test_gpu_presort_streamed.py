"""GPU tests of the split presort (cc_eval_presort_split; cc_presort.hip, cc_split.hip, cc_boost.hip): a resident head of the presorted
range and a tail that is evaluated, sorted and searched chunk by chunk at every node. The contract is one line: every
record, every tree and the whole per-sample state of every round are bit-identical to a run with all tables resident. Each
case runs two evaluators with the same contents, one presorted as ever and one split, and compares them with tolerance
0.0 after every round; one case per mode also goes through tests/boost_witness.py / tests/tree_witness.py (exp taken from the
device, as tests/test_gpu_boost.py does), which shows that both runs are right and not merely equal."""
import numpy as np
import pytest

import cascadeclassifier_amd as cc
from cascadeclassifier_amd import _lib as L
from cascadeclassifier_amd import evaluator as ev
from tests import boost_witness as bw
from tests import tree_cases as tc
from tests import tree_witness as tw
from tests.test_gpu_split import _node_value, _samples, _weights
from tests.test_gpu_training_sizes import HAAR_RANGE

pytestmark = pytest.mark.gpu

WIN = (8, 8)  # Haar BASIC: 2 056 variables
F0 = 900
N = 300
SEED = 9  # chosen on the resident run (CPU witness): winners 2, 141, 41, 154, 148, 196 of the 200 variables from F0


def _evaluator(ftype, mode, win, imgs, labels):
    e = cc.CvFeatureEvaluator.create(ftype)
    e.init(cc.CvFeatureParams(ftype, mode), len(imgs), win)
    e.setImages(imgs, labels)
    return e


def _pair(imgs, labels, var_range, resident, chunk=64, ftype=ev.HAAR, mode=ev.BASIC, win=WIN):
    """Two evaluators over the same samples: all tables resident, and a head of `resident` variables with the rest streamed."""
    a, b = (_evaluator(ftype, mode, win, imgs, labels) for _ in range(2))
    a.presort(len(imgs), *var_range)
    assert b.presort(len(imgs), *var_range, resident_vars=resident, chunk_vars=chunk) == (resident, chunk)
    return a, b


def _rounds_equal(ea, eb, n, rounds, where, witness=None, **params):
    """`rounds` rounds of a booster over each evaluator: records, trees and states equal after each (and equal to the witness's)."""
    a, b = cc.CascadeBoost(ea, n, **params), cc.CascadeBoost(eb, n, **params)
    depth = params.get("max_depth", 1)
    recs = []
    for r in range(rounds):
        ra, rb = a.round(), b.round()
        sa, sb = a.state(), b.state()
        assert set(ra) == set(rb)
        bw.assert_round_equal(rb, ra, sb, sa, (where, "streamed against resident", r))
        if depth > 1 and ra["trained"]:
            tw.assert_tree_equal(rb, ra, (where, "streamed against resident", r))
            (na, la), (nb, lb) = a.last_tree(), b.last_tree()
            tw.assert_tree_equal({"nodes": nb, "leaves": lb}, {"nodes": na, "leaves": la}, (where, "last_tree", r))
        if witness is not None:
            want = witness.round()
            bw.assert_round_equal(rb, want, sb, witness.state(), (where, "streamed against the witness", r))
            if depth > 1 and want["trained"]:
                tw.assert_tree_equal(rb, want, (where, "streamed against the witness", r))
        recs.append(rb)
    return recs


@pytest.fixture(scope="module")
def case200():
    imgs, labels = _samples(N, WIN, SEED, dup=12)
    return imgs, labels, tc.values(ev.HAAR, ev.BASIC, WIN, imgs, (F0, F0 + 200))


# ---- 1. three chunks, the last a partial group ----------------------------------------------------------------------
@pytest.mark.parametrize("resident", [0, 64, 128, 200])
def test_gentle_200_variables_in_chunks_of_64(case200, resident):
    """F = 200, chunks of 64 (the last holds 8 variables), n = 300, Gentle, six rounds, trimming 0.95. resident_vars = 200 is
    today's call: the same tables, nothing held for streaming."""
    imgs, labels, vals = case200
    ea, eb = _pair(imgs, labels, (F0, F0 + 200), resident)
    if resident == 200:
        assert eb.table_bytes() == ea.table_bytes()
    wit = bw.BoostWitness(vals, labels, exp=cc.device_exp, weight_trim_rate=0.95, var0=F0) if resident == 64 else None
    recs = _rounds_equal(ea, eb, N, 6, ("gentle", resident), wit, weight_trim_rate=0.95)
    assert all(r["trained"] for r in recs)
    winners = [r["var_idx"] - F0 for r in recs]
    if resident in (64, 128):  # winners in the head and in the tail, a tail winner followed by a head winner and the reverse
        assert any(w < resident for w in winners) and any(w >= resident for w in winners), winners
    assert any(w >= 192 for w in winners), winners  # the partial last group wins a round


# ---- 2. one chunk; a chunk of one variable ------------------------------------------------------------------------------
@pytest.mark.parametrize("resident", [0, 64])
@pytest.mark.parametrize("nvars", [64, 65])
def test_gentle_one_chunk_and_a_chunk_of_one_variable(case200, nvars, resident):
    """F = 64: everything in one chunk, or (resident_vars = 64 = F) today's call. F = 65: two chunks, or a head of 64 and a
    chunk that holds a single variable."""
    imgs, labels, vals = case200
    ea, eb = _pair(imgs, labels, (F0, F0 + nvars), resident)
    wit = bw.BoostWitness(vals[:nvars], labels, exp=cc.device_exp, weight_trim_rate=0.95, var0=F0) if (nvars, resident) == (65, 64) else None
    recs = _rounds_equal(ea, eb, N, 6, ("one chunk", nvars, resident), wit, weight_trim_rate=0.95)
    assert all(r["trained"] for r in recs)


# ---- 3. the other two ordered kernels ------------------------------------------------------------------------------------
@pytest.mark.parametrize("boost_type", [ev.BOOST_REAL, ev.BOOST_DISCRETE], ids=["real_gini", "discrete_misclass"])
def test_real_and_discrete(case200, boost_type):
    imgs, labels, vals = case200
    ea, eb = _pair(imgs, labels, (F0, F0 + 200), 64)
    exp = cc.device_exp if boost_type == ev.BOOST_REAL else bw.libm_exp
    wit = bw.BoostWitness(vals, labels, boost_type=boost_type, exp=exp, weight_trim_rate=0.95, var0=F0)
    recs = _rounds_equal(ea, eb, N, 4, ("classifier", boost_type), wit, boost_type=boost_type, weight_trim_rate=0.95)
    assert all(r["trained"] for r in recs)


# ---- 4. inner nodes --------------------------------------------------------------------------------------------------------
def test_trees_of_depth_three():
    """max_depth = 3, Gentle: node tables written by k_boost_table, several searches per round, each with its own winner row."""
    imgs, labels = tc.noisy_samples(N, WIN, SEED, dup=12)
    vals = tc.values(ev.HAAR, ev.BASIC, WIN, imgs, (F0, F0 + 200))
    ea, eb = _pair(imgs, labels, (F0, F0 + 200), 64)
    wit = tw.TreeWitness(vals, labels, max_depth=3, exp=cc.device_exp, weight_trim_rate=0.95, var0=F0)
    recs = _rounds_equal(ea, eb, N, 4, "depth 3", wit, max_depth=3, weight_trim_rate=0.95)
    assert recs[0]["trained"] and max(len(r["nodes"]) for r in recs if r["trained"]) >= 4
    used = {nd["var_idx"] - F0 for r in recs if r["trained"] for nd in r["nodes"]}
    assert any(v < 64 for v in used) and any(v >= 64 for v in used), used


# ---- 5. exact quality ties across the boundary -------------------------------------------------------------------------------
def _mirror_samples(n, seed):
    """Samples that are their own left-right mirror image: a vertical-edge or line feature and its mirror image have equal
    values on every sample. Positives are brighter in the upper half."""
    rng = np.random.default_rng(seed)
    labels = (rng.random(n) < 0.5).astype(np.uint8)
    left = rng.integers(0, 256, (n, 8, 4)).astype(np.int64)
    imgs = np.concatenate([left, left[:, :, ::-1]], axis=2)
    upper = (np.arange(8) < 4)[None, :, None]
    imgs = np.where(labels[:, None, None] == 1, imgs + upper * 30, imgs)
    return np.clip(imgs, 0, 255).astype(np.uint8), labels


def test_quality_ties_across_the_boundary_go_to_the_lower_variable():
    """The whole 8x8 catalog (2 056 variables), a head of 512 and chunks of 256. Seed 2 was chosen on the resident run: its
    four winners are 105, 38, 1378 and 1004, whose mirror twins are 573, 921, 1632 and 1613 -- the first two pairs straddle
    the head's end, the last two lie in two different chunks each. The lower number must win every time."""
    n, resident, chunk = N, 512, 256
    imgs, labels = _mirror_samples(n, 2)
    assert (imgs == imgs[:, :, ::-1]).all()
    vals = tc.values(ev.HAAR, ev.BASIC, WIN, imgs)
    rows = {}
    for f in range(len(vals)):
        rows.setdefault(vals[f].tobytes(), []).append(f)
    twin = {g[0]: g[1] for g in rows.values() if len(g) == 2}
    ea, eb = _pair(imgs, labels, (0, len(vals)), resident, chunk)
    # the tie exists: on the host, from the resident presort's per-variable qualities at the root of round one
    w = np.concatenate([np.full(n, 1. / n), [0.0, 0.0]])
    for i in range(n):
        w[n] += w[i]
    resp = (labels.astype(np.int32) * 2 - 1).astype(np.float32)
    root, q, pt = ea.find_best_split(w, responses=resp, node_value=_node_value(w, resp), per_var=True)
    first = root["var_idx"]
    assert first in twin and q[first] == q[twin[first]] and pt[first] == pt[twin[first]] and first < resident <= twin[first]
    assert np.float32(q[first]) == root["quality"] == np.float32(q.max())
    wit = bw.BoostWitness(vals, labels, exp=cc.device_exp, weight_trim_rate=0.95)
    recs = _rounds_equal(ea, eb, n, 4, "ties", wit, weight_trim_rate=0.95)
    part = lambda f: -1 if f < resident else (f - resident) // chunk  # noqa: E731
    straddle = apart = 0
    for r in recs:
        f = r["var_idx"]
        assert r["trained"] and f in twin and f < twin[f], (f, twin.get(f))
        straddle += part(f) < 0 <= part(twin[f])
        apart += 0 <= part(f) < part(twin[f])
    assert recs[0]["var_idx"] == first and straddle >= 1 and apart >= 1, [(r["var_idx"], twin[r["var_idx"]]) for r in recs]


# ---- 6. the sizes at which the tables change form -------------------------------------------------------------------------------
@pytest.mark.parametrize("n,rounds", [(20480, 1), (20481, 1), (65537, 2)])
def test_sizes_where_the_tables_change_form(n, rounds):
    """20 480: the last size with the node table in LDS; 20 481: the first with it in global memory; 65 537: the first with
    32-bit sample numbers (and rows sorted by the device-wide segmented sort). The 192 variables of
    tests/test_gpu_training_sizes.py, a head of 64 and two chunks."""
    imgs, labels = _samples(n, WIN, 17)
    ea, eb = _pair(imgs, labels, HAAR_RANGE, 64)
    recs = _rounds_equal(ea, eb, n, rounds, ("form", n))
    assert all(r["trained"] and HAAR_RANGE[0] <= r["var_idx"] < HAAR_RANGE[1] for r in recs)


# ---- 7. HOG ------------------------------------------------------------------------------------------------------------------
def test_hog_all_streamed():
    """HOG, 16x16 window: one block, 36 variables, all of them streamed in one chunk of a partial group."""
    n, win = N, (16, 16)
    imgs, labels = _samples(n, win, 11)
    ea, eb = _pair(imgs, labels, (0, 36), 0, ftype=ev.HOG, mode=0, win=win)
    vals = ea.calc_batch(0, 36, n_samples=n)
    recs = _rounds_equal(ea, eb, n, 3, "hog", bw.BoostWitness(vals, labels, exp=cc.device_exp))
    assert all(r["trained"] for r in recs)


# ---- 8. cc_eval_find_best_split covers the tail ------------------------------------------------------------------------------
@pytest.mark.parametrize("boost_type", [ev.BOOST_GENTLE, ev.BOOST_REAL, ev.BOOST_DISCRETE])
@pytest.mark.parametrize("resident", [0, 64, 128])
def test_find_best_split_over_a_split_presort(case200, resident, boost_type):
    """The winner and, for all F variables, per_var quality and split point: a root node and a sub-sample node."""
    imgs, labels, _ = case200
    ea, eb = _pair(imgs, labels, (F0, F0 + 200), resident)
    classifier = boost_type != ev.BOOST_GENTLE
    sub = np.sort(np.random.default_rng(5).permutation(N)[:170]).astype(np.int32)
    for idx in (None, sub):
        lab = (labels if idx is None else labels[idx]).astype(np.int32)
        w = _weights(len(lab), lab, 3, classifier)
        kw = {"class_labels": lab} if classifier else {"responses": (lab * 2 - 1).astype(np.float32)}
        if not classifier:
            kw["node_value"] = _node_value(w, kw["responses"])
        (ra, qa, pa), (rb, qb, pb) = (e.find_best_split(w, sample_idx=idx, boost_type=boost_type, per_var=True, **kw) for e in (ea, eb))
        assert ra["found"] and len(qb) == 200
        assert (qa.view(np.uint64) == qb.view(np.uint64)).all() and (pa == pb).all()
        assert all(np.array_equal(np.asarray(ra[k]), np.asarray(rb[k])) for k in ra), (ra, rb)
        assert (pa >= 0).sum() > 150  # the comparison is not one of empty results


# ---- 9. budgets ---------------------------------------------------------------------------------------------------------------
def test_table_bytes_stay_within_the_budget(case200):
    """Half of what the resident tables of the whole 8x8 catalog need: the plan streams, and what the evaluator then holds
    for tables and streaming scratch is within the budget -- also after an earlier, larger presort."""
    imgs, labels, _ = case200
    e = _evaluator(ev.HAAR, ev.BASIC, WIN, imgs, labels)
    f = e.getNumVariables()
    assert f == 2056 and e.table_bytes() == 0
    e.presort()
    full = e.table_bytes()
    assert full >= (f + 63) // 64 * 64 * N * 6
    budget = (f + 63) // 64 * 64 * N * 6 // 2
    resident, chunk, need = e.presort_plan(N, budget_bytes=budget)
    assert chunk >= 64 and resident < f and need <= budget
    assert e.presort(budget_bytes=budget) == (resident, chunk)
    assert 0 < e.table_bytes() <= budget
    rec = cc.CascadeBoost(e, N).round()
    e2 = _evaluator(ev.HAAR, ev.BASIC, WIN, imgs, labels)
    e2.presort()
    want = cc.CascadeBoost(e2, N).round()
    assert all(np.array_equal(np.asarray(rec[k]), np.asarray(want[k])) for k in want)
    assert e.table_bytes() <= budget  # a round allocates nothing for tables
    # budget 0: the free memory and what is held; everything fits a 288 GB device, and the scratch goes back
    assert e.presort_plan(N)[:2] == (f, 0)
    assert e.presort(budget_bytes=0) == (f, 0) and e.table_bytes() == full


def test_train_cascade_within_a_table_budget():
    """train_cascade with half the memory of a stage's resident tables (24x24 Haar BASIC, the set-up of
    tests/test_gpu_train_cascade.py): the same stages and the same end reason as without a budget."""
    from tests.test_gpu_train_cascade import NUM_NEG, NUM_POS, NUM_STAGES, PARAMS, _assert_records_equal, _backgrounds, _positives
    positives, backgrounds = _positives(80, 17), _backgrounds()
    kw = dict(feature_type=ev.HAAR, win=(24, 24), haar_mode=ev.BASIC, **PARAMS)
    cascade, records, end = cc.train_cascade(positives, backgrounds, NUM_POS, NUM_NEG, NUM_STAGES, **kw)
    budget = (162336 + 63) // 64 * 64 * (NUM_POS + NUM_NEG) * 6 // 2
    assert ev.presort_plan(ev.HAAR, 162336, NUM_POS + NUM_NEG, budget)[1] >= 64  # the budget makes every stage stream
    cascade_b, records_b, end_b = cc.train_cascade(positives, backgrounds, NUM_POS, NUM_NEG, NUM_STAGES, table_budget_bytes=budget, **kw)
    assert end_b == end and sum(r["weak"] is not None for r in records) >= 2
    _assert_records_equal(records_b, records)
    ma, mb = cascade.model(), cascade_b.model()
    for k in ("stage_first", "stage_ntrees", "stage_threshold", "stump_feature", "stump_threshold", "stump_left", "stump_right"):
        assert (getattr(ma, k) == getattr(mb, k)).all(), k


# ---- 10. what a split presort holds does not depend on what was held before ------------------------------------------------
def test_split_presort_after_a_larger_resident_presort_holds_the_same(case200):
    """A split presort (head 64, chunks of 64, 200 variables) on a fresh evaluator, and on one that first presorted the
    whole 8x8 catalog: the larger tables go back, both hold the same bytes, and one Gentle round is equal."""
    imgs, labels, _ = case200
    a, b = (_evaluator(ev.HAAR, ev.BASIC, WIN, imgs, labels) for _ in range(2))
    b.presort()
    full = b.table_bytes()
    for e in (a, b):
        assert e.presort(N, F0, F0 + 200, resident_vars=64, chunk_vars=64) == (64, 64)
    assert 0 < a.table_bytes() == b.table_bytes() < full
    assert _rounds_equal(a, b, N, 1, "after a resident presort")[0]["trained"]


def test_split_presort_after_one_of_the_other_index_width_holds_the_same():
    """16-bit sample numbers (300 samples) and then 32-bit ones (65 537), and the reverse: the index buffer of the other
    width goes back, and the evaluator holds what a fresh one holds after the second call alone. The 192 variables of
    tests/test_gpu_training_sizes.py, a head of 64 and two chunks; one Gentle round is equal."""
    big = 65537
    imgs, labels = _samples(big, WIN, 17)
    for first, then in ((N, big), (big, N)):
        a, b = (_evaluator(ev.HAAR, ev.BASIC, WIN, imgs, labels) for _ in range(2))
        assert b.presort(first, *HAAR_RANGE, resident_vars=64, chunk_vars=64) == (64, 64)
        for e in (a, b):
            assert e.presort(then, *HAAR_RANGE, resident_vars=64, chunk_vars=64) == (64, 64)
        assert 0 < a.table_bytes() == b.table_bytes(), (first, then)
        assert _rounds_equal(a, b, then, 1, ("width", first, then))[0]["trained"]


# ---- 11. refusals and invalidation ------------------------------------------------------------------------------------------
def test_refusals(case200):
    imgs, labels, _ = case200
    lbp = _evaluator(ev.LBP, 0, WIN, imgs, labels)
    f = lbp.getNumVariables()
    with pytest.raises(cc.CascadeError) as ei:
        lbp.presort(N, resident_vars=0, chunk_vars=64)
    assert ei.value.status == L.CC_ERR_UNSUPPORTED and "categorical variables are not streamed" in str(ei.value)
    assert lbp.presort(N, resident_vars=f, chunk_vars=64) == (f, 64)  # resident_vars = F: today's presort
    assert cc.CascadeBoost(lbp, N).round()["trained"]
    e = _evaluator(ev.HAAR, ev.BASIC, WIN, imgs, labels)
    for kw in (dict(resident_vars=64, chunk_vars=65), dict(resident_vars=64, chunk_vars=0), dict(resident_vars=63, chunk_vars=64),
               dict(resident_vars=256, chunk_vars=64), dict(resident_vars=-64, chunk_vars=64)):
        with pytest.raises(cc.CascadeError) as ei:
            e.presort(N, F0, F0 + 200, **kw)
        assert ei.value.status == L.CC_ERR_INVALID_ARG, kw
    with pytest.raises(cc.CascadeError) as ei:
        e.find_best_split(np.ones(N + 2), responses=np.ones(N, np.float32))
    assert "cc_eval_presort first" in str(ei.value)  # none of the refused calls presorted anything
    with pytest.raises(ValueError):
        e.presort(N, resident_vars=64, budget_bytes=1 << 30)


def test_a_later_presort_or_set_images_invalidates_the_booster(case200):
    imgs, labels, _ = case200
    e = _evaluator(ev.HAAR, ev.BASIC, WIN, imgs, labels)
    e.presort(N, F0, F0 + 200, resident_vars=64, chunk_vars=64)
    b = cc.CascadeBoost(e, N)
    assert b.round()["trained"]
    e.presort(N, F0, F0 + 200, resident_vars=64, chunk_vars=64)
    with pytest.raises(cc.CascadeError) as ei:
        b.round()
    assert ei.value.status == L.CC_ERR_INVALID_ARG and "create a new booster" in str(ei.value)
    b = cc.CascadeBoost(e, N)
    assert b.round()["trained"]
    e.setImages(imgs[:1], first_idx=3)
    with pytest.raises(cc.CascadeError) as ei:
        b.round()
    assert ei.value.status == L.CC_ERR_INVALID_ARG and "create a new booster" in str(ei.value)
