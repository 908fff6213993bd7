"""CPU only. The witness of the tree booster (tests/tree_witness.py) against the stump witness and against itself, the case
constants of the GPU tests, cc_cascade_from_trees (host only, no device) and what train_cascade(max_depth=...) does around
the device calls."""
import ctypes as C
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import cascadeclassifier_amd as cc
from cascadeclassifier_amd import _lib as L
from cascadeclassifier_amd import evaluator as ev
from cascadeclassifier_amd import trainer
from oracle import oracle as orc
from tests import boost_witness as bw
from tests import tree_cases as tc
from tests import tree_witness as tw
from tests.boost_witness import F32
from tests.test_gpu_split import _samples

SMALL = {"haar": (ev.HAAR, ev.BASIC, (8, 8)), "lbp": (ev.LBP, 0, (12, 12))}


def _small_case(name, n=200, seed=13):
    ftype, mode, win = SMALL[name]
    imgs, labels = _samples(n, win, seed, dup=6)
    return ftype, mode, win, imgs, labels, tc.values(ftype, mode, win, imgs)


@pytest.fixture(scope="module", params=sorted(SMALL))
def small(request):
    return _small_case(request.param)


# ---- witness against witness ------------------------------------------------------------------------------------
@pytest.mark.parametrize("boost_type", [ev.BOOST_DISCRETE, ev.BOOST_GENTLE])
def test_depth_one_is_the_stump_witness(small, boost_type):
    """At max_depth = 1 TreeWitness equals BoostWitness record for record and state for state over six rounds."""
    ftype, _, _, _, labels, vals = small
    kw = dict(boost_type=boost_type, categorical=ftype == ev.LBP, weight_trim_rate=0.95)
    a, b = tw.TreeWitness(vals, labels, max_depth=1, **kw), bw.BoostWitness(vals, labels, **kw)
    for r in range(6):
        got, want = a.round(), b.round()
        assert set(got) == set(want)  # no new keys at depth 1
        bw.assert_round_equal(got, want, a.state(), b.state(), ("depth 1", boost_type, r))
        if want["trained"]:
            nodes, leaves = tw.writer_layout(a.roots[-1])
            assert len(nodes) == 1 and (nodes[0]["left"], nodes[0]["right"]) == (0, -1)
            assert leaves.tolist() == [want["left_value"], want["right_value"]]
    assert a.n_weak == b.n_weak >= 2


# ---- witness self-checks -----------------------------------------------------------------------------------------
class _Recorded:
    """exp that hands its arguments through, so that weak_eval can be read before it is overwritten."""

    def __init__(self):
        self.args = []

    def __call__(self, a):
        self.args.append(np.array(a, np.float64))
        return bw.libm_exp(a)


def _trees_xml(path):
    """Per stage and tree of a saved cascade: (internalNodes tokens, leafValues tokens)."""
    casc = ET.parse(path).getroot().find("cascade")
    return [[(w.findtext("internalNodes").split(), w.findtext("leafValues").split()) for w in st.find("weakClassifiers") if w.tag == "_"]
            for st in casc.find("stages") if st.tag == "_"]


@pytest.mark.parametrize("depth", [2, 3])
def test_witness_trees_are_consistent(small, depth, tmp_path):
    """Children partition their parent in increasing order; an active sample's weak_eval is the value of the leaf direction
    sent it to; the predict walk over the witness's nodes gives the verdict of oracle.train_predict on the cascade that
    from_trees builds from the records, with the leaves compared as float32."""
    ftype, mode, win, imgs, labels, vals = small
    rec_exp = _Recorded()
    wit = tw.TreeWitness(vals, labels, max_depth=depth, boost_type=ev.BOOST_GENTLE, categorical=ftype == ev.LBP, exp=rec_exp)
    recs, sums32 = [], np.zeros(len(labels), np.float64)
    for r in range(4):
        mask = list(wit.mask)
        rec = wit.round()
        if not rec["trained"]:
            break
        recs.append(rec)
        root = wit.roots[-1]
        for node in tw.all_nodes(root):
            assert node["idx"] == sorted(node["idx"])
            if node["left"] is not None:
                assert sorted(node["left"]["idx"] + node["right"]["idx"]) == node["idx"]
                assert node["left"]["idx"] and node["right"]["idx"]
                assert node["left"]["depth"] == node["right"]["depth"] == node["depth"] + 1 <= depth
        weak_eval = rec_exp.args[-1] * np.array([-y for y in wit.y], np.float64)  # undoes `weak_eval *= -y`: y is +-1
        for i in range(wit.n):
            if mask[i]:
                assert wit.leaf_of[i]["left"] is None and weak_eval[i] == wit.leaf_of[i]["value"], (r, i)
        sums32 += [float(F32(wit._predict(root, i)["value"])) for i in range(wit.n)]
    assert len(recs) >= 2 and max(len(r["nodes"]) for r in recs) >= 2
    c = cc.CascadeClassifier.from_trees(ftype, win, [(recs[-1]["stage_threshold"], recs)], haar_mode=mode)
    assert c.info()["max_nodes_per_tree"] == max(len(r["nodes"]) for r in recs)
    path = str(tmp_path / "t.xml")
    c.save(path)
    o = orc.load_cascade_xml(path)
    want_leaves = np.concatenate([np.array([F32(v) for v in r["leaves"]], np.float32) for r in recs])
    assert o.leaves.dtype == np.float32 and (o.leaves == want_leaves).all()
    s, t, nf = orc.set_images(imgs, want_tilted=False, want_norm=ftype == ev.HAAR)
    got = np.array([orc.train_predict(o, s, t, nf, i, win[0], win[1]) for i in range(wit.n)], np.uint8)
    bound = float(F32(recs[-1]["stage_threshold"]) - F32(1e-5))
    want = np.array([0 if v < bound else 1 for v in sums32], np.uint8)
    assert (got == want).all() and 0 < want.sum() < wit.n


# ---- the case constants of the GPU tests ---------------------------------------------------------------------------------
def _tree_depth(node):
    return 0 if node["left"] is None else 1 + max(_tree_depth(node["left"]), _tree_depth(node["right"]))


def test_the_case_constants_are_worth_using():
    """tests/tree_cases.py's seeds of the depth sweep (n = 360, dup = 12; 12x12 Haar CORE seed 33, LBP 24x24 seed 32), run
    here with libm's exp at depth 3: some tree has at least three internal nodes, some tree's two sides differ in depth,
    leaves are made by sample_count <= 10, by the depth limit and by the purity / regression-accuracy rule, and trimming
    leaves at least 10 % of the samples inactive in at least two rounds, so the predict walk through two levels runs."""
    for name, boost_type in (("haar", ev.BOOST_GENTLE), ("lbp", ev.BOOST_REAL)):
        ftype, _, _, _, labels, vals = tc.sweep_case(name)
        wit = tw.TreeWitness(vals, labels, max_depth=3, boost_type=boost_type, categorical=ftype == ev.LBP, weight_trim_rate=tc.TRIM)
        inactive_rounds = deep_walks = 0
        for r in range(tc.SWEEP_ROUNDS[boost_type]):
            before = sum(wit.mask)
            if wit.round()["trained"] and before <= 0.9 * tc.N:
                inactive_rounds += 1
                deep_walks += _tree_depth(wit.roots[-1]) >= 2
        nodes = [n for root in wit.roots for n in tw.all_nodes(root)]
        assert max(sum(1 for n in tw.all_nodes(root) if n["left"] is not None) for root in wit.roots) >= 3, name
        assert any(_tree_depth(root["left"]) != _tree_depth(root["right"]) for root in wit.roots), name
        assert {tw.LEAF_MIN_SAMPLES, tw.LEAF_DEPTH, tw.LEAF_PURE} <= {n["leaf"] for n in nodes}, name
        assert inactive_rounds >= 2 and deep_walks >= 1, (name, inactive_rounds, deep_walks)


def test_the_exit_cases_split_where_they_should():
    """tests/tree_cases.exit_case: the root's split leaves an impure child of exactly 10 samples, which stays a leaf, or of
    11, which is searched and splits; the other child is pure and stays a leaf."""
    for n_left in (10, 11):
        imgs, labels = tc.exit_case(n_left)
        wit = tw.TreeWitness(tc.values(ev.HAAR, ev.BASIC, (8, 8), imgs), labels, max_depth=2, boost_type=ev.BOOST_DISCRETE)
        assert wit.round()["trained"]
        small, big = sorted((wit.roots[0]["left"], wit.roots[0]["right"]), key=lambda n: len(n["idx"]))
        assert len(small["idx"]) == n_left and small["cnt"][0] == 2 and big["leaf"] == tw.LEAF_PURE
        assert small["leaf"] == (tw.LEAF_MIN_SAMPLES if n_left == 10 else None)


# ---- cc_cascade_from_trees ----------------------------------------------------------------------------------------------------
def _random_stumps(n_vars, seed):
    rng = np.random.default_rng(seed)
    weaks = [{"trained": True, "var_idx": int(v), "left_value": float(rng.uniform(-1, 1)), "right_value": float(rng.uniform(-1, 1)),
              "ord_c": np.float32(rng.uniform(-0.5, 0.5)), "subset": rng.integers(-2**31, 2**31, 8).astype(np.int32)}
             for v in rng.choice(n_vars, 7)]
    return [(np.float32(-0.731), weaks[:3]), (np.float32(0.25), weaks[3:])]


@pytest.mark.parametrize("ftype,win,mode,n_vars", [(ev.HAAR, (20, 18), ev.CORE, 5000), (ev.LBP, (20, 18), 0, 2000), (ev.HOG, (32, 16), 0, 36 * 3)])
def test_stump_input_gives_the_model_of_from_stumps(ftype, win, mode, n_vars, tmp_path):
    stages = _random_stumps(n_vars, 5)
    a = cc.CascadeClassifier.from_stumps(ftype, win, stages, haar_mode=mode)
    b = cc.CascadeClassifier.from_trees(ftype, win, stages, haar_mode=mode)
    assert a.info() == b.info() and b.info()["max_nodes_per_tree"] == 1
    ma, mb = a.model(), b.model()
    for k in ("stage_first", "stage_ntrees", "stage_threshold", "stump_feature", "stump_threshold", "stump_left", "stump_right", "stump_subsets", "rects",
              "weights", "tilted"):
        x, y = getattr(ma, k), getattr(mb, k)
        assert (x is None) == (y is None) and (x is None or (x == y).all()), k
    pa, pb = str(tmp_path / "a.xml"), str(tmp_path / "b.xml")
    a.save(pa)
    b.save(pb)
    assert open(pa).read() == open(pb).read()


def _witness_records(ftype, depth):
    """Two stages of witness records at `depth`; HOG's values are seeded numbers (the witness does not care what is searched)."""
    if ftype == ev.HOG:
        win, mode = (16, 16), 0
        rng = np.random.default_rng(3)
        labels = rng.integers(0, 2, 150).astype(np.uint8)
        vals = (rng.random((36, 150)) * 0.5 + labels[None] * rng.random((36, 1)) * 0.2).astype(np.float32)
    else:
        name = "haar" if ftype == ev.HAAR else "lbp"
        _, mode, win, _, labels, vals = _small_case(name)
    stages = []
    for boost_type in (ev.BOOST_GENTLE, ev.BOOST_DISCRETE):
        wit = tw.TreeWitness(vals, labels, max_depth=depth, boost_type=boost_type, categorical=ftype == ev.LBP)
        recs = [wit.round() for _ in range(3)]
        recs = [r for r in recs if r["trained"]]
        stages.append((recs[-1]["stage_threshold"], recs))
    return win, mode, stages


@pytest.mark.parametrize("depth", [2, 3])
@pytest.mark.parametrize("ftype", [ev.HAAR, ev.LBP, ev.HOG])
def test_trees_are_written_in_the_writers_layout(ftype, depth, tmp_path):
    """save -> load -> save reproduces the file; its internalNodes / leafValues are the witness's writer layout with the
    used variables renumbered in catalog order; max_nodes_per_tree is the largest tree's node count."""
    win, mode, stages = _witness_records(ftype, depth)
    c = cc.CascadeClassifier.from_trees(ftype, win, stages, haar_mode=mode)
    recs = [r for _, rs in stages for r in rs]
    inf = c.info()
    assert inf["max_nodes_per_tree"] == max(len(r["nodes"]) for r in recs) > 1
    assert inf["n_nodes"] == sum(len(r["nodes"]) for r in recs) and inf["n_leaves"] == inf["n_nodes"] + inf["n_weak"] and inf["n_weak"] == len(recs)
    used = sorted({nd["var_idx"] for r in recs for nd in r["nodes"]})
    assert inf["n_features"] == len(used)
    p1, p2 = str(tmp_path / "1.xml"), str(tmp_path / "2.xml")
    c.save(p1)
    back = cc.CascadeClassifier(p1)
    assert not back.empty(), getattr(back, "load_error", "")
    assert back.info() == inf
    back.save(p2)
    assert open(p1).read() == open(p2).read()
    trees = [t for st in _trees_xml(p1) for t in st]
    assert len(trees) == len(recs)
    step = 3 + (8 if ftype == ev.LBP else 1)
    for (toks, leaf_toks), r in zip(trees, recs):
        assert len(toks) == step * len(r["nodes"]) and len(leaf_toks) == len(r["nodes"]) + 1
        for k, nd in enumerate(r["nodes"]):
            t = toks[k * step:(k + 1) * step]
            assert [int(t[0]), int(t[1]), int(t[2])] == [nd["left"], nd["right"], used.index(nd["var_idx"])]
            if ftype == ev.LBP:
                assert [int(v) for v in t[3:]] == [int(v) for v in nd["subset"]]
            else:
                assert F32(float(t[3])) == F32(nd["ord_c"])
        assert [F32(float(v)) for v in leaf_toks] == [F32(v) for v in r["leaves"]]


def _call_from_trees(ftype, win, n_weak, n_nodes, nodes, n_leaves=None, n_nodes_total=None):
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    n_weak, n_nodes = np.array(n_weak, np.int32), np.array(n_nodes, np.int32)
    flat = (L.TreeNode * max(1, len(nodes)))()
    for k, (left, right, var) in enumerate(nodes):
        flat[k].left, flat[k].right, flat[k].var_idx = left, right, var
    leaves = np.zeros(len(nodes) + len(n_nodes) + 4, np.float32)
    thr = np.zeros(len(n_weak), np.float32)
    out = C.c_void_p(1)  # must come back NULL from a refusal
    st = L.lib().cc_cascade_from_trees(ftype, 0, win[0], win[1], len(n_weak), vp(n_weak), len(n_nodes), vp(thr), vp(n_nodes),
                                       len(nodes) if n_nodes_total is None else n_nodes_total, flat, vp(leaves), C.byref(out))
    if st == L.CC_OK:
        L.lib().cc_cascade_destroy(out)
    return st, out.value, L.lib().cc_last_error().decode()


def test_from_trees_refusals():
    """A tree without nodes, child references the XML reader would refuse and variables outside the catalog: each returns its
    status and leaves *out == NULL."""
    win = (24, 24)
    n_cat = len(orc.lbp_catalog(24, 24))
    ok = [(1, 0, 5), (-1, 2, 6), (-2, -3, 7)]  # root -> node 1 -> node 2; four leaves
    st, out, _ = _call_from_trees(ev.LBP, win, [1], [3], ok)
    assert st == L.CC_OK and out
    cases = {
        "no nodes": (([2], [1, 0], [(0, -1, 5)]), L.CC_ERR_INVALID_ARG, "has 0 nodes"),
        "left child past the tree": (([1], [3], [(3, 0, 5), (-1, 2, 6), (-2, -3, 7)]), L.CC_ERR_OUT_OF_RANGE, "out of range"),
        "leaf past the tree's leaves": (([1], [3], [(1, 0, 5), (-1, 2, 6), (-2, -4, 7)]), L.CC_ERR_OUT_OF_RANGE, "out of range"),
        "child is the node itself": (([1], [3], [(1, 0, 5), (-1, 1, 6), (-2, -3, 7)]), L.CC_ERR_OUT_OF_RANGE, "does not increase"),
        "child before its parent": (([1], [3], [(1, 0, 5), (-1, 2, 6), (1, -3, 7)]), L.CC_ERR_OUT_OF_RANGE, "does not increase"),
        "variable past the catalog": (([1], [3], [(1, 0, 5), (-1, 2, n_cat), (-2, -3, 7)]), L.CC_ERR_OUT_OF_RANGE, "outside the catalog"),
        "negative variable": (([1], [3], [(1, 0, -1), (-1, 2, 6), (-2, -3, 7)]), L.CC_ERR_OUT_OF_RANGE, "outside the catalog"),
        "variable of an inner node only": (([1], [2], [(1, 0, 5), (-1, -2, n_cat)]), L.CC_ERR_OUT_OF_RANGE, "outside the catalog"),
    }
    for name, (args, status, text) in cases.items():
        st, out, msg = _call_from_trees(ev.LBP, win, *args)
        assert st == status and out is None and text in msg, (name, st, out, msg)
    st, out, msg = _call_from_trees(ev.LBP, win, [1], [3], ok, n_nodes_total=2)
    assert st == L.CC_ERR_INVALID_ARG and out is None and "adds up to 3 nodes" in msg
    st, out, msg = _call_from_trees(ev.LBP, win, [2], [3], ok)  # n_weak says two trees, one was given
    assert st == L.CC_ERR_INVALID_ARG and out is None and "adds up to 2" in msg
    with pytest.raises(cc.CascadeError, match="has 0 weak"):
        cc.CascadeClassifier.from_trees(ev.HAAR, win, [(0.5, [])])


# ---- train_cascade(max_depth=...) and the bindings ----------------------------------------------------------------------------
class _Fakes:
    """The device classes of cascadeclassifier_amd.trainer replaced by recorders: what the driver asks of them is all that runs."""

    def __init__(self, monkeypatch):
        self.ratios, self.boost_kw, self.built = [], [], []
        fakes = self

        class Evaluator:
            @staticmethod
            def create(ftype, device):
                return Evaluator()

            def init(self, *a):
                pass

            def fill_passed(self, cascade, positives, first, want, label):
                return want, want

            def presort(self, n):
                pass

        class Miner:
            def __init__(self, *a):
                pass

            empty = classmethod(lambda cls, *a: cls())

            def fill(self, e, images, first, want, **kw):
                fakes.ratios.append(kw["min_acceptance_ratio"])
                return {"n_filled": want, "n_consumed": 2 * want, "stop": L.CC_FILL_FILLED}

        class Boost:
            def __init__(self, e, n, **kw):
                fakes.boost_kw.append(kw)

            def train_stage(self):
                return [{"trained": True, "stage_threshold": np.float32(0.5)}]

        class Classifier:
            from_stumps = staticmethod(lambda *a, **kw: fakes.built.append("from_stumps") or "cascade")
            from_trees = staticmethod(lambda *a, **kw: fakes.built.append("from_trees") or "cascade")

        for name, fake in (("CvFeatureEvaluator", Evaluator), ("NegativeMiner", Miner), ("CascadeBoost", Boost), ("CascadeClassifier", Classifier)):
            monkeypatch.setattr(trainer, name, fake)


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_train_cascade_divides_the_leaf_rate_and_picks_the_constructor(monkeypatch, depth):
    """required_leaf_fa_rate = pow(maxFalseAlarm, num_stages) / max_depth (cascadeclassifier.cpp:209-210) reaches the fill; the
    booster gets the depth; the stage's cascade comes from from_trees when max_depth > 1 and from from_stumps otherwise."""
    f = _Fakes(monkeypatch)
    pos = np.zeros((4, 8, 8), np.uint8)
    bg = [np.random.default_rng(1).integers(0, 256, (40, 40), dtype=np.uint8)]
    cascade, records, end = trainer.train_cascade(pos, bg, 4, 4, 2, win=(8, 8), max_false_alarm=0.4, max_depth=depth)
    want = pow(float(np.float32(0.4)), 2.0) / float(depth)
    assert cascade == "cascade" and end == trainer.END_NUM_STAGES and len(records) == 2
    assert f.ratios == [want, want]
    assert [kw["max_depth"] for kw in f.boost_kw] == [depth, depth]
    assert f.built == ["from_trees" if depth > 1 else "from_stumps"] * 2
    with pytest.raises(ValueError):
        trainer.train_cascade(pos, bg, 4, 4, 2, win=(8, 8), max_depth=0)


def test_the_tree_entry_points_are_bound():
    """The three symbols bind with the declared argtypes and the struct mirrors cc_tree_node; without a device
    cc_boost_create_depth says CC_ERR_NO_DEVICE."""
    lib = L.lib()
    for name in ("cc_boost_create_depth", "cc_boost_last_tree", "cc_cascade_from_trees"):
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert C.sizeof(L.TreeNode) == 72 and L.TreeNode.value.offset == 64 and L.TreeNode.subset.offset == 32
    p = L.BoostParams(ev.BOOST_GENTLE, 0, 0.95, 0.995, 0.5, 100)
    b = C.c_void_p(1)
    st = lib.cc_boost_create_depth(None, 4, C.byref(p), 2, C.byref(b))
    assert b.value is None
    if lib.cc_device_count() > 0:
        assert st == L.CC_ERR_INVALID_ARG
        return
    assert st == L.CC_ERR_NO_DEVICE
    with pytest.raises(cc.CascadeError) as err:
        cc.train_cascade(np.zeros((2, 24, 24), np.uint8), [np.zeros((48, 64), np.uint8)], 2, 2, 1, max_depth=2)
    assert err.value.status == L.CC_ERR_NO_DEVICE
