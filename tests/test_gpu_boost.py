"""GPU tests of the device booster (section 6b of the C ABI; cc_boost.hip) against tests/boost_witness.py, the contract
restated in Python floats. Records and the full per-sample state are compared with tolerance 0.0 after every round; for
Gentle and Real AdaBoost the witness takes its vector exp from the device (cc_debug_exp64), whose distance from libm is
bounded by a test of its own."""
import math
import os

import numpy as np
import pytest

import cascadeclassifier_amd as cc
from cascadeclassifier_amd import _lib as L
from cascadeclassifier_amd import evaluator as ev
from oracle import oracle as orc
from tests import boost_witness as bw
from tests.test_gpu_split import _samples
from tests.test_gpu_training_sizes import HAAR_RANGE

pytestmark = pytest.mark.gpu

WIN = (24, 24)
N = 360
SEED = 31  # chosen on the CPU (witness with libm's exp): see test_gentle_and_real_rounds_equal_the_witness
BOOST_CHUNK = 512  # cc_boost.hip: samples staged per step of a serial sum (block_serial_sums)
APPLY_CHUNK = 1024  # cc_boost.hip: ranks per step of k_boost_apply_ord
EXP_ARGS = []  # every argument the witness handed to the device's exp in this session


def _device_exp(a):
    EXP_ARGS.append(np.array(a, np.float64))
    return cc.device_exp(a)


def _evaluator(ftype, mode, win, imgs, labels, var_range=None):
    e = cc.CvFeatureEvaluator.create(ftype)
    e.init(cc.CvFeatureParams(ftype, mode), len(imgs), win)
    e.setImages(imgs, labels)
    if var_range:
        e.presort(len(imgs), *var_range)
    else:
        e.presort()
    return e


def _values(ftype, mode, win, imgs, var_range=None):
    s, t, nf = orc.set_images(imgs, want_tilted=False, want_norm=ftype == ev.HAAR)
    cat = orc.haar_catalog(win[0], win[1], mode) if ftype == ev.HAAR else orc.lbp_catalog(*win)
    f0, f1 = var_range or (0, len(cat))
    if ftype == ev.HAAR:
        return orc.haar_eval_batch(cat, f0, f1, s, t, nf, win[0], win[1])
    return orc.lbp_eval_batch(cat, f0, f1, s, win[0], win[1])


def _case360(ftype, mode, win):
    imgs, labels = _samples(N, win, SEED, dup=12)
    return ftype, _evaluator(ftype, mode, win, imgs, labels), labels, _values(ftype, mode, win, imgs)


@pytest.fixture(scope="module")
def haar_core_24():
    return _case360(ev.HAAR, ev.CORE, WIN)


# The oracle's search of the 210 400 CORE variables of a 24x24 window takes seconds per round on the CPU; the ten-round
# cases run on the 13 168 variables of a 12x12 window (the same kernels: 206 groups of 64 variables) and on LBP 24x24.
@pytest.fixture(scope="module", params=["haar", "lbp"])
def case360(request):
    return _case360(ev.HAAR, ev.CORE, (12, 12)) if request.param == "haar" else _case360(ev.LBP, 0, WIN)


def _run(e, vals, labels, rounds, *, categorical, exp=bw.libm_exp, var0=0, where="", **params):
    """`rounds` rounds on the device and in the witness; every record and the whole state equal after each."""
    b = cc.CascadeBoost(e, len(labels), **params)
    wit = bw.BoostWitness(vals, labels, categorical=categorical, exp=exp, var0=var0, **params)
    recs, active = [], []
    for r in range(rounds):
        got, want = b.round(), wit.round()
        bw.assert_round_equal(got, want, b.state(), wit.state(), (where, r))
        recs.append(got)
        active.append(int(sum(wit.mask)))
    return recs, active, wit


def test_discrete_haar_core_24_equals_the_witness(haar_core_24):
    """Discrete AdaBoost, Haar CORE 24x24, n = 360, six rounds, trimming 0.95: every field of every record and the full
    state after every round equal the CPU witness; no device exp is involved."""
    ftype, e, labels, vals = haar_core_24
    recs, active, _ = _run(e, vals, labels, 6, categorical=False, boost_type=ev.BOOST_DISCRETE, weight_trim_rate=0.95, where="discrete 24x24")
    assert all(r["trained"] for r in recs) and min(active) < N  # trimming took samples out


def test_discrete_rounds_equal_the_witness(case360):
    """The same for the 12x12 Haar window and for LBP (categorical splits)."""
    ftype, e, labels, vals = case360
    recs, _, _ = _run(e, vals, labels, 6, categorical=ftype == ev.LBP, boost_type=ev.BOOST_DISCRETE, weight_trim_rate=0.95, where="discrete")
    assert all(r["trained"] for r in recs)


@pytest.mark.parametrize("boost_type", [ev.BOOST_GENTLE, ev.BOOST_REAL])
def test_gentle_and_real_rounds_equal_the_witness(case360, boost_type):
    """Ten rounds, the witness taking exp from cc_debug_exp64. The seed was picked with the CPU witness so that trimming
    deactivates at least 10 % of the samples in at least two rounds: the inactive-sample path of update_weights runs."""
    ftype, e, labels, vals = case360
    recs, active, _ = _run(e, vals, labels, 10, categorical=ftype == ev.LBP, exp=_device_exp, boost_type=boost_type, where=("exp", boost_type))
    assert sum(1 for a in active if a <= 0.9 * N) >= 2, active
    assert len({r["var_idx"] for r in recs if r["trained"]}) > 2


EDGE_SIZES = [63, 64, 65, BOOST_CHUNK - 1, BOOST_CHUNK, BOOST_CHUNK + 1, APPLY_CHUNK - 1, APPLY_CHUNK + 1]


@pytest.mark.parametrize("n", EDGE_SIZES)
def test_sizes_at_kernel_edges(n):
    """One wavefront more or less, and one sample below / above the chunk of the serial sums (BOOST_CHUNK) and of the
    split-apply pass (APPLY_CHUNK). 8x8 Haar BASIC, Gentle, three rounds."""
    win = (8, 8)
    imgs, labels = _samples(n, win, 7 + n, dup=4)
    e = _evaluator(ev.HAAR, ev.BASIC, win, imgs, labels)
    _run(e, _values(ev.HAAR, ev.BASIC, win, imgs), labels, 3, categorical=False, exp=_device_exp, where=("edge", n))


@pytest.mark.parametrize("n", [20480, 20481, 65537])
def test_sizes_where_the_tables_change_form(n):
    """20 480 is the last size whose node table fits LDS (8-byte entries), 20 481 the first with the table in global memory;
    65 537 the first with 32-bit sample numbers in the presorted tables. 8x8 window, the 192 variables of
    tests/test_gpu_training_sizes.py, three Gentle rounds."""
    win = (8, 8)
    imgs, labels = _samples(n, win, 17)
    e = _evaluator(ev.HAAR, ev.BASIC, win, imgs, labels, HAAR_RANGE)
    vals = _values(ev.HAAR, ev.BASIC, win, imgs, HAAR_RANGE)
    recs, _, _ = _run(e, vals, labels, 3, categorical=False, exp=_device_exp, var0=HAAR_RANGE[0], where=("form", n))
    assert all(HAAR_RANGE[0] <= r["var_idx"] < HAAR_RANGE[1] for r in recs)


def _small(n, labels, ftype=ev.HAAR, seed=3):
    imgs, _ = _samples(n, (8, 8), seed)
    return _evaluator(ftype, ev.BASIC, (8, 8), imgs, np.asarray(labels, np.uint8)), imgs


def test_exit_ten_active_samples():
    e, _ = _small(10, [1, 0] * 5)
    r = cc.CascadeBoost(e, 10).round()
    assert not r["trained"] and r["stop"] == 4 and r["n_active"] == 10  # min_sample_count, o_cvdtree.cpp:130


def test_exit_one_class_only():
    e, _ = _small(40, [1] * 40)
    b = cc.CascadeBoost(e, 40, boost_type=ev.BOOST_DISCRETE)
    before = b.state()
    r = b.round()
    assert not r["trained"] and r["stop"] == 4
    after = b.state()
    assert all((before[k] == after[k]).all() for k in before)  # state untouched


def test_exit_max_weak_count():
    labels = np.random.default_rng(2).integers(0, 2, 200)  # labels unrelated to the pixels: the false alarm stays up
    e, _ = _small(200, labels)
    recs = cc.CascadeBoost(e, 200, max_weak_count=2, max_false_alarm=1e-3).train_stage()
    assert [r["stop"] for r in recs] == [0, 2] and all(r["trained"] for r in recs)


def test_exit_separable_set_stops_after_one_tree():
    rng = np.random.default_rng(4)
    n = 120
    labels = (np.arange(n) % 2).astype(np.uint8)
    imgs = rng.integers(0, 20, (n, 8, 8)).astype(np.uint8)
    imgs[labels == 1, :, :4] += 200  # positives: bright left half; negatives: bright right half
    imgs[labels == 0, :, 4:] += 200
    e = _evaluator(ev.HAAR, ev.BASIC, (8, 8), imgs, labels)
    recs = cc.CascadeBoost(e, n).train_stage()
    assert len(recs) == 1 and recs[0]["stop"] == 1 and recs[0]["hit_rate"] == 1 and recs[0]["false_alarm"] == 0


def test_logit_is_unsupported_and_presort_invalidates():
    e, imgs = _small(40, [1, 0] * 20)
    with pytest.raises(cc.CascadeError) as ei:
        cc.CascadeBoost(e, 40, boost_type=ev.BOOST_LOGIT)
    assert ei.value.status == L.CC_ERR_UNSUPPORTED and "LOGIT" in str(ei.value)
    with pytest.raises(cc.CascadeError) as ei:
        cc.CascadeBoost(e, 39)  # not the presorted sample count
    assert ei.value.status == L.CC_ERR_INVALID_ARG
    b = cc.CascadeBoost(e, 40)
    assert b.round()["trained"]
    e.presort()
    with pytest.raises(cc.CascadeError) as ei:
        b.round()
    assert ei.value.status == L.CC_ERR_INVALID_ARG and "create a new booster" in str(ei.value)
    b = cc.CascadeBoost(e, 40)
    e.setImages(imgs[:1], first_idx=3)
    with pytest.raises(cc.CascadeError) as ei:
        b.round()
    assert ei.value.status == L.CC_ERR_INVALID_ARG


def test_hog_rounds_equal_the_witness():
    """HOG, 16x16 window (one block, 36 variables), n = 300, Gentle, five rounds. The witness searches the values the
    evaluator reports (tests/test_gpu_hog.py checks those against the restatement of HOGfeatures.cpp)."""
    n, win = 300, (16, 16)
    imgs, labels = _samples(n, win, 11)
    e = _evaluator(ev.HOG, 0, win, imgs, labels)
    vals = e.calc_batch(0, e.getNumVariables(), n_samples=n)
    _run(e, vals, labels, 5, categorical=False, exp=_device_exp, where="hog")


def test_transcript_shape_of_the_reference_run(repo_root):
    """traincascade/res/README.md:41-54: LBP, Gentle, 75x32, 100 positives and one negative: stage 0 ends after one weak
    classifier with hit rate 1 and false alarm 0. The positives are those of tests/golden/barcode.vec; the negative here
    is seeded noise, NOT the window the reference's reader cuts from its bg.png."""
    pos = cc.detector.vec_read(os.path.join(repo_root, "tests", "golden", "barcode.vec"))
    pos = np.asarray(pos, np.uint8).reshape(-1, 32, 75)[:100]
    assert len(pos) == 100
    neg = np.random.default_rng(9).integers(0, 256, (1, 32, 75), dtype=np.uint8)
    imgs = np.concatenate([pos, neg])
    labels = np.array([1] * 100 + [0], np.uint8)
    e = _evaluator(ev.LBP, 0, (75, 32), imgs, labels)
    recs = cc.CascadeBoost(e, 101, boost_type=ev.BOOST_GENTLE).train_stage()
    assert len(recs) == 1 and recs[0]["trained"] and recs[0]["stop"] == 1
    assert recs[0]["hit_rate"] == 1 and recs[0]["false_alarm"] == 0


def _stage_pass(model, vals_used):
    """Direct evaluation of a stump cascade's float model on values [used feature][sample]: per stage the double sum of
    the float leaves in tree order; a sample fails a stage iff sum < threshold (the model's, epsilon already taken off)."""
    alive = np.ones(vals_used.shape[1], bool)
    for s in range(len(model.stage_ntrees)):
        acc = np.zeros(vals_used.shape[1], np.float64)
        for t in range(model.stage_first[s], model.stage_first[s] + model.stage_ntrees[s]):
            v = vals_used[model.stump_feature[t]]
            acc = acc + np.where(v <= model.stump_threshold[t], np.float64(model.stump_left[t]), np.float64(model.stump_right[t]))
        alive &= ~(acc < np.float64(model.stage_threshold[s]))
    return alive.astype(np.uint8)


def test_the_training_loop_closes(tmp_path):
    """samples -> presort -> boost a stage -> cascade -> mine negatives -> next stage, all through the library."""
    n_pos, n_neg = 100, 100
    imgs, labels = _samples(2 * n_pos, WIN, 41)
    pos = imgs[labels == 1][:n_pos]
    rng = np.random.default_rng(42)
    neg = rng.integers(0, 256, (n_neg, 24, 24), dtype=np.uint8)
    stages = []
    cascade = None
    for stage in range(2):
        samples = np.concatenate([pos, neg])
        lab = np.array([1] * len(pos) + [0] * len(neg), np.uint8)
        e = _evaluator(ev.HAAR, ev.BASIC, WIN, samples, lab)
        recs = cc.CascadeBoost(e, len(samples)).train_stage()
        last = recs[-1]
        assert last["stop"] == 1 and last["false_alarm"] <= 0.5 and last["hit_rate"] >= np.float32(0.995), (stage, last)
        stages.append((last["stage_threshold"], recs))
        cascade = cc.CascadeClassifier.from_stumps(ev.HAAR, WIN, stages, haar_mode=ev.BASIC)
        if stage == 0:
            _, kept, _ = cc.NegativeMiner(cascade).run(rng.integers(0, 256, (150, 200), dtype=np.uint8), max_keep=n_neg)
            assert len(kept) > 10  # false positives of stage 0: the next stage's negatives
            neg = kept
    m = cascade.model()
    assert m.info["n_stages"] == 2
    path = str(tmp_path / "trained.xml")
    cascade.save(path)
    back = cc.CascadeClassifier(path)
    mb = back.model()
    for k in ("stage_first", "stage_ntrees", "stage_threshold", "stump_feature", "stump_threshold", "stump_left", "stump_right", "rects", "weights", "tilted"):
        assert (getattr(m, k) == getattr(mb, k)).all(), k
    # predict_cascade on the stored samples against the built model's float stumps
    used = sorted({w["var_idx"] for _, ws in stages for w in ws})
    vals_used = np.stack([e.calc_batch(v, v + 1, n_samples=len(samples))[0] for v in used])
    got = e.predict_cascade(cascade, n_samples=len(samples))
    assert (got == _stage_pass(m, vals_used)).all()
    assert got[:len(pos)].mean() >= 0.98  # two stages at hit rate >= 0.995 each
    rects = back.detectMultiScale(rng.integers(0, 256, (150, 200), dtype=np.uint8), 1.2, 1)
    assert rects.ndim == 2 or len(rects) == 0


def test_device_exp_within_two_ulp_of_libm():
    """The ROCm device library and glibc each document <= 1 ulp for double exp: at most 2 ulp between them. 10^5 points over
    [-40, 40] plus every argument the witness cases above produced (this test is the file's last)."""
    x = np.concatenate([np.random.default_rng(5).uniform(-40, 40, 100000)] + EXP_ARGS)
    got = cc.device_exp(x)
    want = np.array([math.exp(v) for v in x])
    ulps = np.abs(got - want) / np.spacing(want)
    print("device exp: max distance from libm %.3f ulp over %d points" % (ulps.max(), len(x)))
    assert ulps.max() <= 2.0
