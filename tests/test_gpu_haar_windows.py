"""Haar detection, negative mining and training-side predict at windows other than 24x24.

The window size selects code in the detector that a 24x24 cascade never runs: the non-compact squared-sum integral of odd
windows, the opt-in for more than 64 KiB of LDS (and the refusal above 160 KiB), row stride, plane split and bank skew of
the tile geometries that the Haar stump records are offsets into, the second (tilted) tile behind the first, the 16-bit
tile's eligibility test and strip form, the integer form of a stump, the miner's half-window ladder.

Same bar as tests/test_gpu_detect_variants.py: per-window result codes, stage sums (tolerance HAAR_SUM_TOL = 0), visited
flags, ungrouped candidates and grouped rectangles identical to the CPU oracle, which tests/test_haar_windows_host.py
checks against direct pixel summation at these windows. The cascades come from tests/haar_windows.py.

LDS bytes per block of the table-driven kernel (eval_lds_bytes of the larger of TileGeom<1> / TileGeom<2>, 8 window rows;
upright / with the tilted tile):
    20x20 28048 / 49056     19x23 29840 / 52640     25x24 31072 / 55104     24x25 31680 / 56320     14x28 32160 / 57280
    44x12 25840 / 44640     75x32 45776 / 84512*    128x40 63808 / 120576*  96x96 107392* / 207744 (refused)
    * = above 64 KiB: cc_detector_create asks for the larger dynamic LDS size.
"""
import re

import numpy as np
import pytest

import cascadeclassifier_amd as cc
from cascadeclassifier_amd import _lib as L
from cascadeclassifier_amd import evaluator as ev
from oracle import oracle as orc
from tests import haar_windows as hw
from tests.test_gpu_color import colourise, restated_gray
from tests.test_gpu_detect import HAAR_SUM_TOL
from tests.util import frame_natural, frame_uniform

pytestmark = pytest.mark.gpu

LDS_MESSAGE = r"needs (\d+) bytes of LDS per tile"


def _frames(W, H):
    return [(frame_natural(400, 300, 51), 1.1), (frame_natural(W + 3, H + 40, 52), 1.5), (frame_uniform(333, 127, 53), 1.25)]


def _classifier(xml_text, **kw):
    p = cc.CascadeClassifier(**kw)
    assert p.load_from_string(xml_text), getattr(p, "load_error", "")
    return p


def _check(p, o, cases, grouped=(0, 2), **size):
    """cases: (image, scale factor). Returns the candidates per case."""
    n_cand = []
    mn, mx = size.get("minSize"), size.get("maxSize")
    for img, sf in cases:
        ref = orc.detect_raw(o, img, sf, mn or (0, 0), mx or (0, 0), nthreads=8, full=True)
        codes, sums, vis = p.debug_windows(img, sf, mn, mx)
        assert len(codes) == ref.n_grid_windows
        bad = np.nonzero(codes != ref.codes)[0]
        assert len(bad) == 0, f"{len(bad)} of {len(codes)} window results differ, first at {bad[:5].tolist()}: {codes[bad[:5]].tolist()} for {ref.codes[bad[:5]].tolist()}"
        assert np.max(np.abs(sums - ref.sums), initial=0.0) <= HAAR_SUM_TOL
        assert (vis == ref.visited).all()
        raw = p.detect_raw(img, sf, mn, mx)
        assert raw.shape == ref.candidates.shape and (raw == ref.candidates).all()
        for g in grouped:
            a, b = p.detectMultiScale(img, sf, g, minSize=mn, maxSize=mx), orc.detect_multiscale(o, img, sf, g, mn or (0, 0), mx or (0, 0), nthreads=8)
            assert a.shape == b.shape and (a == b).all()
        n_cand.append(len(raw))
    return n_cand


# ------------------------------------------------------------------ table-driven kernel, every window
@pytest.mark.parametrize("pair", [p for p in hw.PAIRS if p != (96, 96, True)], ids=hw.pair_id)
def test_table_driven_kernel(tmp_path, pair):
    W, H, tilted = pair
    xml = hw.stump_xml(W, H, tilted)
    n = _check(_classifier(xml), hw.oracle_cascade(tmp_path, xml), _frames(W, H))
    assert n[0] > 0


def test_window_above_160_kib_is_refused(tmp_path):
    """96x96 with the tilted tile behind the sum tile: the detector says so instead of launching."""
    p = _classifier(hw.stump_xml(96, 96, True))
    with pytest.raises(cc.CascadeError, match=LDS_MESSAGE) as e:
        p.detectMultiScale(frame_natural(400, 300, 51), 1.1, 0)
    assert e.value.status == L.CC_ERR_UNSUPPORTED
    assert int(re.search(LDS_MESSAGE, str(e.value)).group(1)) > 160 * 1024 - 256
    # the same window without tilted features is served (more than 64 KiB: the opt-in path)
    xml = hw.stump_xml(96, 96, False)
    q, o = _classifier(xml), hw.oracle_cascade(tmp_path, xml)
    img = frame_natural(200, 150, 54)
    a, b = q.detectMultiScale(img, 1.2, 0), orc.detect_multiscale(o, img, 1.2, 0, nthreads=8)
    assert a.shape == b.shape and (a == b).all() and len(b) > 0


@pytest.mark.parametrize("pair", [p for p in hw.PAIRS if p != (96, 96, True)], ids=hw.pair_id)
def test_frames_of_about_one_window(tmp_path, pair):
    """Frames of exactly the window, one pixel more on either side, and one pixel short on either side."""
    W, H, tilted = pair
    xml = hw.stump_xml(W, H, tilted)
    p, o = _classifier(xml), hw.oracle_cascade(tmp_path, xml)
    src = frame_natural(640, 480, 3)
    # two calibration windows that the cascade accepts (about one in sixteen passes four stages calibrated at one half
    # each), so that the frames of one window are not all empty results, and one arbitrary place
    accepted = [(x, y) for (x, y) in hw.calibration_positions(W, H)[::3] if len(orc.detect_multiscale(o, src[y:y + H, x:x + W], 1.1, 0))][:2]
    assert len(accepted) == 2
    seen = 0
    for (x, y) in accepted + [(100, 50)]:
        for (w, h) in [(W, H), (W + 1, H), (W, H + 1), (W - 1, H + 30), (W + 30, H - 1)]:
            img = np.ascontiguousarray(src[y:y + h, x:x + w])
            a, b = p.detectMultiScale(img, 1.1, 0), orc.detect_multiscale(o, img, 1.1, 0)
            assert a.shape == b.shape and (a == b).all(), (x, y, w, h)
            if w < W or h < H:
                assert len(b) == 0
            seen += len(b)
    assert seen >= 6


@pytest.mark.parametrize("W,H", [(20, 20), (19, 23)])
@pytest.mark.parametrize("tilted", [False, True], ids=["upright", "tilted"])
def test_saturated_and_flat_frames(tmp_path, W, H, tilted):
    """400x400 of 255 with a lattice of zeros: the squared-sum integral wraps past 2^32 (19x23: through the non-compact
    addressing). A flat frame: every window fails the variance test."""
    xml = hw.stump_xml(W, H, tilted)
    p, o = _classifier(xml), hw.oracle_cascade(tmp_path, xml)
    sat = np.full((400, 400), 255, np.uint8)
    sat[::7, ::5] = 0
    assert int(orc.integral(sat, sqsum_f64=True)["sqsum_f64"][-1, -1]) > 2 ** 32
    _check(p, o, [(sat, 1.2)])
    flat = np.full((100, 120), 77, np.uint8)
    _check(p, o, [(flat, 1.1)])
    ref = orc.detect_raw(o, flat, 1.1, full=True)
    assert (ref.codes == -1).all() and len(ref.candidates) == 0


@pytest.mark.parametrize("tilted", [False, True], ids=["upright", "tilted"])
def test_min_and_max_size_odd_window(tmp_path, tilted):
    xml = hw.stump_xml(19, 23, tilted)
    p, o = _classifier(xml), hw.oracle_cascade(tmp_path, xml)
    img = hw.pasted_frame(19, 23, 55)
    assert _check(p, o, [(img, 1.1)], minSize=(40, 40))[0] > 0
    assert _check(p, o, [(img, 1.1)], maxSize=(60, 60))[0] > 0
    _check(p, o, [(img, 1.1)], minSize=(50, 50), maxSize=(50, 50))


def test_batch_and_colour_odd_window(tmp_path):
    xml = hw.stump_xml(19, 23, True)
    o = hw.oracle_cascade(tmp_path, xml)
    frames = np.stack([hw.pasted_frame(19, 23, 60 + i) for i in range(5)])
    p = _classifier(xml, max_batch=2)
    got = p.detect_batch(frames, 1.1, 2)
    total = 0
    for i in range(5):
        b = orc.detect_multiscale(o, frames[i], 1.1, 2, nthreads=8)
        assert got[i].shape == b.shape and (got[i] == b).all()
        total += len(b)
    assert total > 0
    bgr = colourise(frames[0], 71)
    want = orc.detect_multiscale(o, restated_gray(bgr, "bgr"), 1.1, 2, nthreads=8)
    a = p.detectMultiScale(bgr, 1.1, 2)
    assert a.shape == want.shape and (a == want).all() and len(want) > 0
    rgb = np.ascontiguousarray(bgr[..., ::-1])
    a = p.detectMultiScale(rgb, 1.1, 2, pixel_format="rgb")
    assert a.shape == want.shape and (a == want).all()


# ------------------------------------------------------------------ run-time specialised kernels
def _specialise_or_refusal(p, k):
    """cc_detector_specialize's contract: the number of compiled stages, or CascadeError with the LDS message (0 here)."""
    try:
        got = p.specialize(k)
    except cc.CascadeError as e:
        assert e.status == L.CC_ERR_UNSUPPORTED and re.search(r"bytes of LDS per tile", str(e)), str(e)
        assert p.specialized_stages() == 0
        return 0
    assert got == k
    return k


@pytest.mark.parametrize("pair", [(20, 20, False), (20, 20, True), (19, 23, False), (19, 23, True), (75, 32, False), (75, 32, True),
                                  (128, 40, False), (128, 40, True), (96, 96, False)], ids=hw.pair_id)
def test_specialised_kernels(tmp_path, pair):
    """Some stages and all stages compiled. Either the module is installed and every bit matches, or the library refuses
    with its LDS message and the detector goes on with the table-driven kernel -- and still matches."""
    W, H, tilted = pair
    xml = hw.stump_xml(W, H, tilted)
    o = hw.oracle_cascade(tmp_path, xml)
    outcomes = []
    for k in (2, o.nstages):
        p = _classifier(xml)
        outcomes.append(_specialise_or_refusal(p, k))
        n = _check(p, o, _frames(W, H)[:2], grouped=(2,))
        assert n[0] > 0
    print(f"specialize {W}x{H} {'tilted' if tilted else 'upright'}: stages in effect {outcomes}")


@pytest.mark.parametrize("W,H,min_area", [(20, 20, 16), (19, 23, 16), (75, 32, 16), (20, 20, 258)])
def test_tile16_kernels(tmp_path, monkeypatch, W, H, min_area):
    """CCAMD_SPEC_TILE16=1 with upright cascades. 20x20 and 19x23 are eligible (the variance rectangle's halves, 9 x 18
    and 9 x 21 pixels, sum below 2^16); 75x32 is not (37 x 30 x 255 > 2^16) and keeps the 32-bit tile without a word;
    min_area=258 makes every first rectangle take the strip form."""
    monkeypatch.setenv("CCAMD_SPEC_TILE16", "1")
    half = (W - 2 - (W - 2) // 2) * (H - 2) * 255
    assert (half < 65536) == ((W, H) != (75, 32))
    xml = hw.stump_xml(W, H, False, min_area)
    o = hw.oracle_cascade(tmp_path, xml)
    for k in (2, o.nstages):
        p = _classifier(xml)
        assert p.specialize(k) == k
        n = _check(p, o, _frames(W, H)[:2] if k == 2 else _frames(W, H)[:1], grouped=(2,))
        assert n[0] > 0


@pytest.mark.parametrize("env", [{"CCAMD_WAVE_BELOW": "0"}, {"CCAMD_WAVE_BELOW": "64"}, {"CCAMD_SPLIT_STUMPS": "0"},
                                 {"CCAMD_SPLIT_STUMPS": "1", "CCAMD_WAVE_BELOW": "64"}], ids=lambda e: ",".join(f"{k[6:]}={v}" for k, v in e.items()))
@pytest.mark.parametrize("pair", [(20, 20, True), (19, 23, False), (19, 23, True)], ids=hw.pair_id)
def test_wave_phase_and_split_stumps(tmp_path, monkeypatch, pair, env):
    """The wavefront-per-window phase (taken below CCAMD_WAVE_BELOW live windows of a tile) and the split of a stage's
    stumps over the wavefronts, on a frame whose pasted calibration windows keep the queues long into the last stage."""
    W, H, tilted = pair
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    xml = hw.stump_xml(W, H, tilted)
    o = hw.oracle_cascade(tmp_path, xml)
    img = hw.pasted_frame(W, H, 56)
    ref = orc.detect_raw(o, img, 1.1, nthreads=8, full=True)
    exits = hw.exit_stage_counts(ref.codes, o.nstages)
    assert exits[-2] > 100 and exits[-1] > 100, f"windows per exit stage {exits.tolist()}: too few reach the last stage"
    assert _check(_classifier(xml), o, [(img, 1.1)], grouped=(2,))[0] > 0


@pytest.mark.parametrize("W,H", [(20, 20), (19, 23)])
@pytest.mark.parametrize("tilted", [False, True], ids=["upright", "tilted"])
def test_trees_deeper_than_stumps(tmp_path, W, H, tilted):
    xml = hw.tree_xml(W, H, tilted)
    p, o = _classifier(xml), hw.oracle_cascade(tmp_path, xml)
    assert p.info()["max_nodes_per_tree"] == 4
    assert _check(p, o, _frames(W, H))[0] > 0
    with pytest.raises(cc.CascadeError, match="stump cascades only"):
        p.specialize(2)
    assert _check(p, o, _frames(W, H)[:1], grouped=())[0] > 0


# ------------------------------------------------------------------ negative mining, training-side predict
MINE = [(20, 20, False, "stumps"), (20, 20, True, "stumps"), (19, 23, False, "stumps"), (19, 23, True, "stumps"),
        (75, 32, False, "stumps"), (75, 32, True, "stumps"), (19, 23, False, "trees"), (19, 23, True, "trees")]


def _mine_id(c):
    return hw.pair_id(c) + "-" + c[3]


def _mine_xml(W, H, tilted, kind):
    return hw.stump_xml(W, H, tilted) if kind == "stumps" else hw.tree_xml(W, H, tilted)


@pytest.mark.parametrize("case", MINE, ids=_mine_id)
def test_negative_mining_matches_reader_loop(tmp_path, case):
    """NegativeMiner against the oracle's literal reader loop (tests/test_gpu_negmine.py) where the half-window step
    rounds: images that are no multiple of the half window in either direction, non-zero offsets."""
    W, H, tilted, kind = case
    path = hw.write_xml(tmp_path, _mine_xml(W, H, tilted, kind))
    o = orc.load_cascade_xml(path)
    c = cc.CascadeClassifier(path)
    assert not c.empty(), getattr(c, "load_error", "")
    m = cc.NegativeMiner(c)
    images = [(frame_natural(333, 211, 41), 5, 2), (frame_natural(7 * W + W // 2 + 3, 5 * H + H // 2 + 1, 43), 3, 7),
              (frame_uniform(2 * W + 5, 2 * H + 3, 42), 1, 1), (hw.pasted_frame(W, H, 44, 641, 479), 0, 17)]
    assert images[1][0].shape[1] % (W // 2) and images[1][0].shape[0] % (H // 2)
    total = 0
    for img, ox, oy in images:
        h, w = img.shape
        want_f, want_p, want_i = orc.negmine_image(o, img, ox, oy, max_keep=40)
        assert m.plan(w, h, ox, oy)["n_windows"] == len(want_f)
        got_f, got_p, got_i = m.run(img, ox, oy, max_keep=40)
        assert got_f.shape == want_f.shape and (got_f == want_f).all(), f"{(got_f != want_f).sum()} of {len(want_f)} windows differ"
        assert (got_i == want_i).all() and (got_p == want_p).all()
        total += int(want_f.sum())
    assert total > 0
    # run_batch of three = one call per image, and the oracle on the first and the last
    imgs = [hw.pasted_frame(W, H, 80 + k, 301, 203) for k in range(3)]
    single = [m.run(im, 3, 5, max_keep=10 ** 6) for im in imgs]
    flags, pix, idx = m.run_batch(imgs, 3, 5, max_keep=25)
    assert flags.shape == (3, len(single[0][0]))
    for k, (f1, p1, i1) in enumerate(single):
        assert (flags[k] == f1).all(), f"image {k}: {(flags[k] != f1).sum()} windows differ"
    want_idx = np.concatenate([i1 + k * flags.shape[1] for k, (f1, p1, i1) in enumerate(single)])[:25]
    want_pix = np.concatenate([p1 for f1, p1, i1 in single])[:25]
    assert (idx == want_idx).all() and (pix == want_pix).all() and len(want_idx) > 0
    for k in (0, 2):
        assert (flags[k] == orc.negmine_image(o, imgs[k], 3, 5, max_keep=1)[0]).all()


@pytest.mark.parametrize("case", MINE, ids=_mine_id)
def test_training_side_predict(tmp_path, case):
    """CvCascadeClassifier::predict over stored samples of the cascade's size against the oracle's stage walk."""
    W, H, tilted, kind = case
    path = hw.write_xml(tmp_path, _mine_xml(W, H, tilted, kind))
    o = orc.load_cascade_xml(path)
    c = cc.CascadeClassifier(path)
    imgs = np.concatenate([hw.calibration_windows(W, H)[5::7][:300], np.full((1, H, W), 77, np.uint8)])
    e = cc.CvFeatureEvaluator.create(ev.HAAR)
    e.init(cc.CvFeatureParams(ev.HAAR, ev.ALL if tilted else ev.BASIC), len(imgs), (W, H))
    e.setImages(imgs)
    got = e.predict_cascade(c)
    s, t, nf = orc.set_images(imgs, want_tilted=tilted)
    want = np.array([orc.train_predict(o, s, t, nf, i, W, H) for i in range(len(imgs))], np.uint8)
    assert (got == want).all() and 0 < want.sum() < len(imgs)
