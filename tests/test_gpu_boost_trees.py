"""GPU tests of the device booster growing trees (cc_boost_create_depth, cc_boost_last_tree; cc_boost.hip) against
tests/tree_witness.py. Every record, every node, every leaf and the full per-sample state are compared with tolerance 0.0
after every round; for Gentle and Real AdaBoost the witness takes its vector exp from the device (cc_debug_exp64). The
seeds and sets are those tests/test_tree_witness_host.py examines on the CPU."""
import ctypes as C

import numpy as np
import pytest

import cascadeclassifier_amd as cc
from cascadeclassifier_amd import _lib as L
from cascadeclassifier_amd import evaluator as ev
from tests import boost_witness as bw
from tests import tree_cases as tc
from tests import tree_witness as tw
from tests.test_gpu_training_sizes import HAAR_RANGE

pytestmark = pytest.mark.gpu

BOOST_CHUNK = 512  # cc_boost.hip: samples staged per step of a serial sum (block_serial_sums)
APPLY_CHUNK = 1024  # cc_boost.hip: ranks per step of k_boost_apply_ord


def _evaluator(ftype, mode, win, imgs, labels, var_range=None):
    e = cc.CvFeatureEvaluator.create(ftype)
    e.init(cc.CvFeatureParams(ftype, mode), len(imgs), win)
    e.setImages(imgs, labels)
    if var_range:
        e.presort(len(imgs), *var_range)
    else:
        e.presort()
    return e


def _run(e, vals, labels, rounds, *, max_depth, categorical, exp=bw.libm_exp, var0=0, where="", **params):
    """`rounds` rounds on the device and in the witness: every record, the tree and the whole state equal after each."""
    b = cc.CascadeBoost(e, len(labels), max_depth=max_depth, **params)
    wit = tw.TreeWitness(vals, labels, max_depth=max_depth, categorical=categorical, exp=exp, var0=var0, **params)
    recs, active = [], []
    for r in range(rounds):
        got, want = b.round(), wit.round()
        bw.assert_round_equal(got, want, b.state(), wit.state(), (where, r))
        assert set(got) == set(want), (where, r)
        if want["trained"] and max_depth > 1:
            tw.assert_tree_equal(got, want, (where, r))
        recs.append(got)
        active.append(int(sum(wit.mask)))
    return recs, active, wit


# ---- depth sweep -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["haar", "lbp"])
def sweep(request):
    ftype, mode, win, imgs, labels, vals = tc.sweep_case(request.param)
    return ftype, _evaluator(ftype, mode, win, imgs, labels), labels, vals


@pytest.mark.parametrize("boost_type", [ev.BOOST_DISCRETE, ev.BOOST_GENTLE, ev.BOOST_REAL], ids=["discrete", "gentle", "real"])
@pytest.mark.parametrize("depth", [2, 3])
def test_depth_sweep_equals_the_witness(sweep, depth, boost_type):
    """12x12 Haar CORE (13 168 variables) and LBP 24x24, n = 360, trimming 0.95: Discrete six rounds, Gentle and Real ten."""
    ftype, e, labels, vals = sweep
    exp = bw.libm_exp if boost_type == ev.BOOST_DISCRETE else cc.device_exp
    recs, _, wit = _run(e, vals, labels, tc.SWEEP_ROUNDS[boost_type], max_depth=depth, categorical=ftype == ev.LBP, exp=exp, boost_type=boost_type,
                        weight_trim_rate=tc.TRIM, where=("sweep", depth, boost_type))
    assert sum(r["trained"] for r in recs) >= 2
    assert max(len(r["nodes"]) for r in recs if r["trained"]) >= 2


# ---- kernel edges ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [63, 64, 65, BOOST_CHUNK - 1, BOOST_CHUNK, BOOST_CHUNK + 1, APPLY_CHUNK - 1, APPLY_CHUNK + 1])
def test_sizes_at_kernel_edges(n):
    """One wavefront more or less, and one sample below / above the chunk of the serial sums (BOOST_CHUNK) and of the
    split-apply pass (APPLY_CHUNK). 8x8 Haar BASIC, max_depth 2, Gentle, three rounds."""
    win = (8, 8)
    imgs, labels = tc.noisy_samples(n, win, 7 + n, dup=4)
    e = _evaluator(ev.HAAR, ev.BASIC, win, imgs, labels)
    recs, _, _ = _run(e, tc.values(ev.HAAR, ev.BASIC, win, imgs), labels, 3, max_depth=2, categorical=False, exp=cc.device_exp, where=("edge", n))
    assert recs[0]["trained"]


@pytest.mark.parametrize("n", [20480, 20481, 65537])
def test_sizes_where_the_tables_change_form(n):
    """20 480 is the last size whose node table fits LDS (8-byte entries), 20 481 the first with the table in global memory;
    65 537 the first with 32-bit sample numbers in the presorted tables. 8x8 window, the 192 variables of
    tests/test_gpu_training_sizes.py, max_depth 2, one Gentle round: three searches."""
    win = (8, 8)
    imgs, labels = tc.noisy_samples(n, win, 17)
    e = _evaluator(ev.HAAR, ev.BASIC, win, imgs, labels, HAAR_RANGE)
    vals = tc.values(ev.HAAR, ev.BASIC, win, imgs, HAAR_RANGE)
    recs, _, _ = _run(e, vals, labels, 1, max_depth=2, categorical=False, exp=cc.device_exp, var0=HAAR_RANGE[0], where=("form", n))
    assert recs[0]["trained"] and len(recs[0]["nodes"]) == 3
    assert all(HAAR_RANGE[0] <= nd["var_idx"] < HAAR_RANGE[1] for nd in recs[0]["nodes"])


# ---- exits -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_left", [10, 11])
def test_exit_ten_samples_stay_a_leaf_eleven_are_searched(n_left):
    """tests/tree_cases.exit_case: the root's split leaves an impure child of exactly n_left samples beside a pure one. With
    10 it stays a leaf (min_sample_count, o_cvdtree.cpp:130), with 11 it is searched and splits; the pure child stays a leaf."""
    imgs, labels = tc.exit_case(n_left)
    e = _evaluator(ev.HAAR, ev.BASIC, (8, 8), imgs, labels)
    recs, _, wit = _run(e, tc.values(ev.HAAR, ev.BASIC, (8, 8), imgs), labels, 1, max_depth=2, categorical=False, boost_type=ev.BOOST_DISCRETE,
                        where=("exit", n_left))
    nodes = recs[0]["nodes"]
    assert len(nodes) == (1 if n_left == 10 else 2) and nodes[0]["n_samples"] == len(labels)
    assert sorted(len(c["idx"]) for c in (wit.roots[0]["left"], wit.roots[0]["right"])) == [n_left, len(labels) - n_left]
    if n_left == 11:
        assert nodes[1]["n_samples"] == 11 and nodes[1]["depth"] == 1
        assert sorted((nodes[0]["left"], nodes[0]["right"])) == [0, 1]  # the pure child is leaf 0, the other node 1


def _valid_tree(nodes, leaves):
    assert len(leaves) == len(nodes) + 1
    seen_nodes, seen_leaves = {0}, set()
    for k, nd in enumerate(nodes):
        for c in (nd["left"], nd["right"]):
            if c > 0:
                assert k < c < len(nodes) and c not in seen_nodes
                seen_nodes.add(c)
            else:
                assert -c < len(leaves) and -c not in seen_leaves
                seen_leaves.add(-c)
    assert len(seen_nodes) == len(nodes) and len(seen_leaves) == len(leaves)


def test_exit_depth_25_on_forty_samples_terminates():
    imgs, labels = tc.noisy_samples(40, (8, 8), 3)
    e = _evaluator(ev.HAAR, ev.BASIC, (8, 8), imgs, labels)
    vals = tc.values(ev.HAAR, ev.BASIC, (8, 8), imgs)
    for depth in (25, 1000):  # values above 25 are clamped to 25 (o_cvdtreetraindata.cpp:105)
        recs, _, _ = _run(e, vals, labels, 2, max_depth=depth, categorical=False, exp=cc.device_exp, where=("depth", depth))
        assert recs[0]["trained"]
        for r in recs:
            if r["trained"]:
                _valid_tree(r["nodes"], r["leaves"])
                assert max(nd["depth"] for nd in r["nodes"]) < 25
    with pytest.raises(cc.CascadeError) as ei:
        cc.CascadeBoost(e, 40, max_depth=0)
    assert ei.value.status == L.CC_ERR_INVALID_ARG


def test_last_tree_buffers_and_order_of_calls():
    imgs, labels = tc.noisy_samples(200, (8, 8), 5)
    e = _evaluator(ev.HAAR, ev.BASIC, (8, 8), imgs, labels)
    b = cc.CascadeBoost(e, 200, max_depth=3)
    lib, k = L.lib(), C.c_int(-7)
    nodes, leaves = (L.TreeNode * 8)(), np.zeros(9, np.float64)
    vp = leaves.ctypes.data_as(C.c_void_p)
    assert lib.cc_boost_last_tree(b._b, nodes, 8, vp, 9, C.byref(k)) == L.CC_ERR_INVALID_ARG  # no trained round yet
    rec = b.round()
    assert rec["trained"] and len(rec["nodes"]) >= 2
    before = b.state()
    assert lib.cc_boost_last_tree(b._b, nodes, len(rec["nodes"]) - 1, vp, 9, C.byref(k)) == L.CC_ERR_BUFFER_TOO_SMALL
    assert k.value == len(rec["nodes"])
    k = C.c_int(-7)
    assert lib.cc_boost_last_tree(b._b, nodes, 8, vp, len(rec["nodes"]), C.byref(k)) == L.CC_ERR_BUFFER_TOO_SMALL  # one leaf short
    assert k.value == len(rec["nodes"]) and (leaves == 0).all()
    after = b.state()
    assert all((before[name] == after[name]).all() for name in before)
    again, again_leaves = b.last_tree()  # fetching changes nothing
    assert [nd["var_idx"] for nd in again] == [nd["var_idx"] for nd in rec["nodes"]] and (again_leaves == rec["leaves"]).all()


# ---- depth 1 -----------------------------------------------------------------------------------------------------
def _booster_from_cc_boost_create(e, n, **params):
    """A CascadeBoost around cc_boost_create, the entry point without a depth."""
    b = cc.CascadeBoost.__new__(cc.CascadeBoost)
    b._b, b._evaluator, b.n_samples, b.max_weak_count, b.max_depth = C.c_void_p(), e, n, 100, 1
    p = L.BoostParams(params.get("boost_type", ev.BOOST_GENTLE), 0, 0.95, 0.995, 0.5, 100)
    L.check(L.lib().cc_boost_create(e._e, n, C.byref(p), C.byref(b._b)))
    return b


@pytest.mark.parametrize("boost_type", [ev.BOOST_DISCRETE, ev.BOOST_GENTLE])
def test_depth_one_is_cc_boost_create(boost_type):
    """cc_boost_create_depth(..., 1) and cc_boost_create give identical records and state over six rounds, and
    cc_boost_last_tree returns the one node and two leaves of each stump."""
    imgs, labels = tc.noisy_samples(300, (8, 8), 9, dup=6)
    e = _evaluator(ev.HAAR, ev.BASIC, (8, 8), imgs, labels)
    a = cc.CascadeBoost(e, 300, boost_type=boost_type, max_depth=1)
    b = _booster_from_cc_boost_create(e, 300, boost_type=boost_type)
    for r in range(6):
        ra, rb = a.round(), b.round()
        assert "nodes" not in ra and set(ra) == set(rb)
        bw.assert_round_equal(ra, rb, a.state(), b.state(), ("depth 1", r))
        if not ra["trained"]:
            continue
        for booster in (a, b):
            nodes, leaves = booster.last_tree()
            assert len(nodes) == 1 and (nodes[0]["left"], nodes[0]["right"], nodes[0]["depth"]) == (0, -1, 0)
            assert all(nodes[0][k] == ra[k] for k in ("var_idx", "split_point", "quality", "ord_c")) and nodes[0]["n_samples"] == ra["n_active"]
            assert leaves.tolist() == [ra["left_value"], ra["right_value"]]


# ---- HOG -----------------------------------------------------------------------------------------------------------
def test_hog_trees_equal_the_witness():
    """HOG takes the ordered path: 16x16 window (one block, 36 variables), n = 300, max_depth 2, Gentle, three rounds, on
    the values the evaluator reports."""
    n, win = 300, (16, 16)
    imgs, labels = tc.noisy_samples(n, win, 11)
    e = _evaluator(ev.HOG, 0, win, imgs, labels)
    vals = e.calc_batch(0, e.getNumVariables(), n_samples=n)
    recs, _, _ = _run(e, vals, labels, 3, max_depth=2, categorical=False, exp=cc.device_exp, where="hog")
    assert recs[0]["trained"] and len(recs[0]["nodes"]) >= 2
