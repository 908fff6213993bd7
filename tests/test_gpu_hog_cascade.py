"""HOG cascades on the device: the training-side stage predict on stored samples (cc_eval_predict_cascade) and the batched
negative mining (cc_negminer_*), both against numpy restatements of the reference: the HOG evaluator
(tests/hog_restatement.py), CvCascadeBoost::predict (boost.cpp:461-477) and the negative reader's window walk
(NegReader::nextImg / get, imagestorage.cpp:57-126, float32 arithmetic, levels by the oracle's INTER_LINEAR_EXACT resize).
Every mined window gets its own setImage, with the border taken from the window copy (HOGfeatures.cpp:173-183)."""
import ctypes as C
import os

import numpy as np
import pytest

import cascadeclassifier_amd as cc
from cascadeclassifier_amd import _lib as L
from cascadeclassifier_amd import evaluator as ev
from oracle import oracle as orc
from tests import cascade_factory as cf
from tests import hog_cascade_factory as hf
from tests import hog_lds_cases as lds
from tests import hog_mine_cases as mc
from tests import hog_restatement as hog
from tests.hog_mine_cases import BACKGROUNDS, predict_windows, reader_stream
from tests.hog_mine_cases import cascade_for as _cascade_for
from tests.hog_mine_cases import edges as _edges
from tests.util import frame_natural, frame_uniform, read_vec

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
# 24x24, 32x32, 75x32, then the windows at the edges of the miner's LDS classes (tests/hog_lds_cases.py): tall, either side of
# the 64 KiB opt-in, the largest the miner accepts. The inputs, the restatement and the conditions that make each case worth
# running (tests/test_hog_mine_cases_host.py) are in tests/hog_mine_cases.py.
WINS = mc.WINDOWS


def _id(win):
    return "%dx%d" % win


def _accept_all_haar(W, H):
    feat = orc.make_haar_feature(False, [(0, 0, 4, 4, -1.0), (0, 0, 2, 2, 4.0)])
    stages = [(-1e30, [([(0, -1, 0, 0.0)], [1.0, 1.0])])]
    return cf.haar_xml(np.array([feat]).reshape(1), stages, mode="BASIC", W=W, H=H)


def _classifier(xml, tmp_path, name):
    p = str(tmp_path / name)
    open(p, "w").write(xml)
    c = cc.CascadeClassifier(p)
    assert not c.empty(), getattr(c, "load_error", "")
    return c


# ---------------------------------------------------------------------------------------------- predict on stored samples
@pytest.mark.parametrize("depth", [1, 2], ids=["stumps", "trees"])
@pytest.mark.parametrize("win", WINS, ids=_id)
def test_predict_cascade_equals_stage_walk(win, depth, tmp_path):
    W, H = win
    rng = np.random.default_rng(W * 7 + depth)
    if win in lds.MINER_WINDOWS:  # 200 samples; the 10-90 % pass share is asserted in tests/test_hog_mine_cases_host.py
        samples, xml, feats, stages, want = mc.predict_case(win, depth)
    else:
        if win == (75, 32):
            samples = read_vec(os.path.join(ROOT, "tests", "golden", "barcode.vec"))
        elif win == (24, 24):
            samples = frame_uniform(24, 24 * 20000, 12).reshape(20000, 24, 24)
            samples[::3] = samples[::3] // 4 + 90  # lower-contrast third
        else:
            samples = np.stack([frame_natural(W * 3, H * 2, 5 + k)[k % H:k % H + H, (3 * k) % W:(3 * k) % W + W] for k in range(600)])
        calib = samples[rng.choice(len(samples), min(len(samples), 400), replace=False)]
        xml, feats, stages = hf.hog_cascade(calib, seed=W + depth, stage_sizes=(4, 6, 9), depth=depth, pass_share=0.7)
        want = predict_windows(feats, stages, samples)
    c = _classifier(xml, tmp_path, "hog.xml")
    n = len(samples)
    e = cc.CvFeatureEvaluator.create(ev.HOG)
    e.init(cc.CvFeatureParams.create(ev.HOG), n, win)
    e.setImages(samples)
    assert 0 < want.sum() < n
    got = e.predict_cascade(c)
    assert (got == want).all(), f"{(got != want).sum()} of {n} samples differ"
    idx = rng.permutation(n)[: n // 3].astype(np.int32)  # the sample_idx form
    assert (e.predict_cascade(c, sample_idx=idx) == want[idx]).all()


def test_predict_cascade_type_and_window_mismatch(tmp_path):
    xml, _, _ = hf.hog_cascade(np.stack([frame_natural(24, 24, k) for k in range(50)]), seed=1, stage_sizes=(2,))
    c = _classifier(xml, tmp_path, "hog.xml")
    e = cc.CvFeatureEvaluator.create(ev.HAAR)
    e.init(cc.CvFeatureParams(ev.HAAR), 4, (24, 24))
    with pytest.raises(cc.CascadeError) as err:
        e.predict_cascade(c, n_samples=4)
    assert err.value.status == L.CC_ERR_INVALID_ARG and "HOG" in str(err.value)
    e32 = cc.CvFeatureEvaluator.create(ev.HOG)
    e32.init(cc.CvFeatureParams.create(ev.HOG), 4, (32, 32))
    with pytest.raises(cc.CascadeError) as err:
        e32.predict_cascade(c, n_samples=4)
    assert err.value.status == L.CC_ERR_INVALID_ARG


# ---------------------------------------------------------------------------------------------- negative mining
@pytest.mark.parametrize("win", WINS, ids=_id)
def test_reader_restatement_matches_plan_and_oracle(win, tmp_path):
    """The test's reader walk is itself checked: its ladder is cc_negminer_plan's, and its windows are the pixels the
    oracle's literal reader loop keeps with an accept-all Haar cascade of the same window size."""
    W, H = win
    haar = _classifier(_accept_all_haar(W, H), tmp_path, "all.xml")
    o = orc.load_cascade_xml(str(tmp_path / "all.xml"))
    xml, _, _ = _cascade_for(W, H, 1, seed=3, stage_sizes=(2,))
    m = cc.NegativeMiner(_classifier(xml, tmp_path, "hog.xml"))
    for _, img, ox, oy, ladder, wins in mc.streams(win):
        plan = m.plan(img.shape[1], img.shape[0], ox, oy)
        assert plan["levels"] == ladder and plan["n_windows"] == len(wins)
        flags, pix, _ = orc.negmine_image(o, img, ox, oy, max_keep=len(wins) + 1)
        assert flags.all() and len(pix) == len(wins) and (pix == wins).all()
        assert len(cc.NegativeMiner(haar).run(img, ox, oy, max_keep=0)[0]) == len(wins)


def _assert_mined(m, win, flags):
    """The miner's flags, kept positions and kept pixels on every background of the window against the restatement's flags."""
    total = 0
    for (name, img, ox, oy, _, wins), want in zip(mc.streams(win), flags):
        keep = 25
        got_f, got_p, got_i = m.run(img, ox, oy, max_keep=keep)
        assert got_f.shape == want.shape and (got_f == want).all(), f"{name}: {(got_f != want).sum()} of {len(want)} windows differ"
        want_i = np.nonzero(want)[0][:keep]
        assert (got_i == want_i).all() and (got_p == wins[want_i]).all(), name
        total += int(want.sum())
    assert 0 < total < sum(len(f) for f in flags)


@pytest.mark.parametrize("depth", [1, 2], ids=["stumps", "trees"])
@pytest.mark.parametrize("win", WINS, ids=_id)
def test_negative_mining_matches_reader_loop(win, depth, tmp_path):
    xml, _, _, flags = mc.mining_case(win, depth)
    _assert_mined(cc.NegativeMiner(_classifier(xml, tmp_path, "hog.xml")), win, flags)


def test_negative_mining_with_long_stages(tmp_path):
    """Stages of 70 and 130 stumps: in the wavefront walk (the cascade is order-independent) every lane takes a second and a
    third stump of a stage. Both long stages reject and pass windows (tests/test_hog_mine_cases_host.py)."""
    xml, _, stages, flags, counts = mc.long_stage_case()
    assert hf.order_independent(stages) and all(p > 0 and e - p > 0 for e, p in counts[1:])
    _assert_mined(cc.NegativeMiner(_classifier(xml, tmp_path, "hog.xml")), (24, 24), flags)


def test_negative_mining_with_order_dependent_stumps(tmp_path):
    """A stump cascade whose leaves (+2^80, a1, -2^80, a3, then more small votes) fail the order-independence proof: the
    miner must walk it in one lane, in tree order. Summed in the order of a wavefront that shares the stumps
    (hf.wave_stage_sums) a3's vote is lost as well as a1's and the same windows get other flags, so a miner that took the
    wavefront walk here fails this test; so does one that sums in reversed order."""
    xml, feats, stages, fwd, rev, wave = mc.order_dependent_case()
    assert not hf.order_independent(stages)
    assert (np.concatenate(fwd) != np.concatenate(wave)).any() and (np.concatenate(fwd) != np.concatenate(rev)).any()
    assert (fwd[1] != wave[1]).any()  # also on the stored samples below
    c = _classifier(xml, tmp_path, "hog.xml")
    _assert_mined(cc.NegativeMiner(c), (24, 24), fwd)
    wins = mc.streams((24, 24))[1][5]  # k_hog_predict's walk of the same cascade on stored samples
    e = cc.CvFeatureEvaluator.create(ev.HOG)
    e.init(cc.CvFeatureParams.create(ev.HOG), len(wins), (24, 24))
    e.setImages(wins)
    assert (e.predict_cascade(c) == fwd[1]).all()


def test_window_border_is_the_copy_not_the_level():
    """On the edge background, gradients at a window's outer ring differ from those of the same pixels inside the level:
    planes shared level-wide would give these windows other values (the tests above would see it)."""
    W, H = 24, 24
    img = _edges(240, 160, 7)
    ladder, wins = reader_stream(img, W, H, 0, 0)
    lw, lh, nx, ny = ladder[-1]
    level = orc.resize_linear_exact(img, lw, lh)
    i = len(wins) - nx * ny + nx + 1  # last level, grid (1, 1): x = y = 12
    assert (wins[i] == level[12:12 + H, 12:12 + W]).all()
    hist_w, norm_w = hog.set_image(wins[i])
    hist_l, norm_l = hog.set_image(level[12:12 + H + 1, 12:12 + W + 1])  # the same pixels with the level's right / bottom context
    assert not (np.array_equal(hist_w[:, H, W], hist_l[:, H, W]) and norm_w[H, W] == norm_l[H, W])


@pytest.mark.parametrize("win,depth", [((24, 24), 1), ((32, 32), 2)], ids=["24x24_stumps", "32x32_trees"])
def test_batch_equals_one_call_per_image(win, depth, tmp_path):
    W, H = win
    xml, _, _ = _cascade_for(W, H, depth, seed=5 + depth)
    m = cc.NegativeMiner(_classifier(xml, tmp_path, "hog.xml"))
    for shape, n_img, ox, oy, keep in (((200, 300), 6, 7, 3, 40), ((480, 640), 40, 0, 0, 300)):  # 40 x 640x480: several pieces
        imgs = [frame_natural(shape[1], shape[0], 70 + k) if k % 3 else _edges(shape[1], shape[0], k) for k in range(n_img)]
        single = [m.run(im, ox, oy, max_keep=10 ** 6) for im in imgs]
        flags, pix, idx = m.run_batch(imgs, ox, oy, max_keep=keep)
        assert flags.shape == (n_img, len(single[0][0]))
        for k, (f1, _, _) in enumerate(single):
            assert (flags[k] == f1).all(), f"image {k}: {(flags[k] != f1).sum()} windows differ"
        want_idx = np.concatenate([i1 + k * flags.shape[1] for k, (_, _, i1) in enumerate(single)])[:keep]
        want_pix = np.concatenate([p1 for _, p1, _ in single])[:keep]
        assert len(want_idx) > 0 and (idx == want_idx).all() and (pix == want_pix).all()


def test_miner_flags_equal_evaluator_host_mirror(tmp_path):
    """CvFeatureEvaluator(HOG).setImage(window) -> operator() from the host mirror -> stage walk, for a few hundred stream
    windows: the trainer's own per-window path gives the miner's flag."""
    W, H = 24, 24
    xml, feats, stages = _cascade_for(W, H, 1, seed=17)
    m = cc.NegativeMiner(_classifier(xml, tmp_path, "hog.xml"))
    cat = hog.catalog(W, H)
    vi = np.array([np.nonzero((cat == f[:4]).all(1))[0][0] * 36 + f[4] for f in feats])
    e = cc.CvFeatureEvaluator.create(ev.HOG)
    e.init(cc.CvFeatureParams.create(ev.HOG), 1, (W, H))
    model = hf.parsed_model(stages)
    checked = 0
    for _, img, ox, oy in BACKGROUNDS:
        _, wins = reader_stream(img, W, H, ox, oy)
        flags = m.run(img, ox, oy, max_keep=0)[0]
        for i in range(0, len(wins), max(1, len(wins) // 120)):
            e.setImage(wins[i], 0, 0)
            vals = np.array([[e(int(v), 0)] for v in vi], np.float32)
            assert hf.stage_walk(model, vals)[0] == flags[i], i
            checked += 1
    assert checked >= 200


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals(tmp_path):
    xml, _, _ = hf.hog_cascade(np.stack([frame_natural(24, 24, k) for k in range(50)]), seed=2, stage_sizes=(2,))
    c = _classifier(xml, tmp_path, "hog.xml")
    d = C.c_void_p()
    assert L.lib().cc_detector_create(c._c, 0, 1, C.byref(d)) == L.CC_ERR_UNSUPPORTED
    n = C.c_size_t(0)
    assert L.lib().cc_cascade_compile_specialized(c._c, 2, b"gfx950", C.byref(n)) == L.CC_ERR_UNSUPPORTED
    img = frame_natural(64, 48, 1)
    for call in (lambda: c.detectMultiScale(img), lambda: c.detectMultiScale3(img), lambda: c.detect_batch(img[None]),
                 lambda: c.specialize(2), lambda: c.specialize_async(2)):
        with pytest.raises(cc.CascadeError) as err:
            call()
        assert err.value.status == L.CC_ERR_UNSUPPORTED and "HOG" in str(err.value)
    # a window whose planes do not fit the LDS of one workgroup
    big = hf.hog_xml(np.array([[0, 0, 8, 8, 0]], np.int32), [(-1.0, [([(0, -1, 0, 0.5)], [1.0, -1.0])])], 128, 96)
    cb = cc.CascadeClassifier()
    assert cb.load_from_string(big)
    with pytest.raises(cc.CascadeError) as err:
        cc.NegativeMiner(cb)
    assert err.value.status == L.CC_ERR_UNSUPPORTED and "LDS" in str(err.value)


def _one_stump(W, H):
    c = cc.CascadeClassifier()
    assert c.load_from_string(hf.hog_xml(np.array([[0, 0, 8, 8, 0]], np.int32), [(-1.0, [([(0, -1, 0, 0.5)], [1.0, -1.0])])], W, H))
    return c


def test_miner_refuses_the_first_window_past_its_lds(tmp_path):
    """The last windows whose planes fit 160 KiB of LDS are accepted, the next ones refused (tests/hog_lds_cases.py), and a
    refusal leaves the library able to mine. At height 40 the planes of 86, 87 and 88 columns fit (159 880, 161 720 and
    163 560 B of 163 840); 89 columns (165 400 B) are the first that do not."""
    for win in lds.MINER_LAST_ACCEPTED + [(86, 40), (87, 40)]:
        assert lds.miner_accepts(win)
        assert cc.NegativeMiner(_one_stump(*win)) is not None
    for win in lds.MINER_FIRST_REFUSED:
        assert not lds.miner_accepts(win)
        with pytest.raises(cc.CascadeError) as err:
            cc.NegativeMiner(_one_stump(*win))
        assert err.value.status == L.CC_ERR_UNSUPPORTED and "LDS" in str(err.value), win
    xml, _, _, flags = mc.mining_case((24, 24), 1)
    _assert_mined(cc.NegativeMiner(_classifier(xml, tmp_path, "hog.xml")), (24, 24), flags)


@pytest.mark.parametrize("order", ["large_first", "small_first"])
def test_miners_of_two_sizes_share_the_kernel(order, tmp_path):
    """k_negmine_hog's LDS opt-in belongs to the kernel, not to a miner: a 59x59 miner (161 405 B) and a 75x32 miner
    (112 320 B) created in either order both mine what the restatement says, the large one also after the small one ran."""
    large, small = (59, 59), (75, 32)
    assert lds.miner_opts_in(large) and lds.miner_opts_in(small) and lds.TABLE[large][3] > lds.TABLE[small][3]
    miners = {}
    for win in ((large, small) if order == "large_first" else (small, large)):
        miners[win] = cc.NegativeMiner(_classifier(mc.mining_case(win, 1)[0], tmp_path, "hog_%dx%d.xml" % win))
    for win in (large, small, large):
        _assert_mined(miners[win], win, mc.mining_case(win, 1)[3])
