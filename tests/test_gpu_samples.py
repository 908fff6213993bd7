"""Sample synthesis on the device against the recorded output of the reference's tool and against the numpy witness
(tests/sample_witness.py), byte for byte."""
import os

import numpy as np
import pytest

import cascadeclassifier_amd as cc
from cascadeclassifier_amd import samples as S
from tests import sample_witness as W
from tests.sample_cases import BARCODE, CASES, GOLDEN, barcode_image, bg_images, obj_image

pytestmark = pytest.mark.gpu


def test_readme_command_reproduces_the_recorded_vec(tmp_path):
    path = str(tmp_path / "barcode.vec")
    cc.create_training_samples(path, barcode_image(), 100, 75, 32, **BARCODE)
    got, want = open(path, "rb").read(), open(os.path.join(GOLDEN, "barcode.vec"), "rb").read()
    assert len(got) == len(want) == 480112
    diff = np.flatnonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))
    assert diff.size == 0, f"{diff.size} bytes differ, first at {diff[0]}"


def _both(sw, sh, ow, oh, kw, n, seed=12345, backgrounds=None, bg_list=None, max_batch=0, obj_seed=5):
    img = obj_image(sw, sh, obj_seed, kw.get("bgcolor", 0))
    want = W.generate(img, n, ow, oh, W.Params(**kw), W.RNG(seed), backgrounds=backgrounds, bg_images=bg_list)
    s = cc.Sampler(img, kw.get("bgcolor", 0), kw.get("bgthreshold", 80))
    if bg_list is not None:
        s.set_backgrounds(bg_list)
    rng = cc.CvRNG(seed)
    got = s.generate(n, (ow, oh), cc.SampleParams(**kw), rng, backgrounds=backgrounds, max_batch=max_batch)
    s.close()
    assert got.shape == want.shape == (n, oh, ow)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{len(bad)} pixels differ, first (sample, y, x) = {bad[0]}"
    return got


@pytest.mark.parametrize("name", sorted(CASES))
def test_generate_matches_witness(name):
    sw, sh, ow, oh, kw = CASES[name]
    got = _both(sw, sh, ow, oh, kw, 24)
    assert len(np.unique(got)) > 8


def test_generate_onto_caller_backgrounds():
    bg = np.random.RandomState(11).randint(0, 256, (24, 24, 24)).astype(np.uint8)
    _both(40, 24, 24, 24, {}, 24, backgrounds=bg)


def test_generate_onto_the_tools_background_windows():
    got = _both(40, 24, 24, 24, {}, 60, bg_list=bg_images())  # 60 windows: every image, several scales of image 0
    assert len(np.unique(got[:, 0, 0])) > 8  # corner pixels are background: they differ from sample to sample


def test_generate_one_sample():
    _both(40, 24, 24, 24, {}, 1)


def test_generate_one_more_than_a_batch():
    bg = np.random.RandomState(12).randint(0, 256, (9, 13, 20)).astype(np.uint8)
    _both(40, 24, 20, 13, {}, 9, backgrounds=bg, max_batch=8)
    _both(40, 24, 20, 13, {}, 9, bg_list=bg_images(), max_batch=4)


def test_sampler_prepare_matches_witness():
    """Mask and border extension alone: a zero-angle sample of an image whose background is noisy shows both."""
    for bgcolor in (0, 255, 100):
        _both(37, 29, 24, 24, dict(bgcolor=bgcolor, bgthreshold=20, maxxangle=0.0, maxyangle=0.0, maxzangle=0.0), 2, obj_seed=9)


QUADS = {
    "inside": [[10.5, 6.25], [50.0, 9.0], [46.5, 40.0], [8.0, 36.5]],
    "crossing_left_top": [[-12.0, -7.5], [40.0, -3.0], [36.0, 30.0], [-9.5, 26.0]],
    "past_right_bottom": [[20.0, 15.0], [75.5, 18.0], [72.0, 60.0], [24.0, 55.5]],
    "counter_clockwise": [[8.0, 36.5], [46.5, 40.0], [50.0, 9.0], [10.5, 6.25]],
}


@pytest.mark.parametrize("name", sorted(QUADS))
def test_warp_perspective_matches_dense_witness(name):
    src = obj_image(23, 17, 21)
    pattern = ((np.arange(48)[:, None] * 7 + np.arange(64)[None, :] * 3) % 251).astype(np.uint8)
    want = W.warp_perspective(src, pattern.copy(), QUADS[name])
    got = S.warp_perspective(src, pattern.copy(), QUADS[name])
    assert (got == want).all()
    changed = got != pattern
    assert changed.any() and not changed.all()  # the spans are there, and pixels outside them are untouched
    if name == "crossing_left_top":
        assert changed[1, 0] and not changed[0].any()  # clamped to column 0; the walk starts at row 1
    if name == "past_right_bottom":
        assert changed[47, 63 - 10:].any()


def test_command_line_writes_the_same_file(tmp_path):
    """The tool's options through main(): -img as .pgm, -bg list file, -randinv, -rngseed; equal to the Python call."""
    img, bgs = obj_image(40, 24, 5), bg_images()
    with open(tmp_path / "obj.pgm", "wb") as f:
        f.write(b"P5\n# object\n40 24\n255\n" + img.tobytes())
    for i, b in enumerate(bgs):
        np.save(tmp_path / f"bg{i}.npy", b)
    (tmp_path / "bg.txt").write_text("# backgrounds\nbg0.npy\nbg1.npy\nbg2.npy\n")
    a, b = str(tmp_path / "a.vec"), str(tmp_path / "b.vec")
    assert S.main(["-img", str(tmp_path / "obj.pgm"), "-vec", a, "-bg", str(tmp_path / "bg.txt"), "-num", "7", "-w", "20", "-h", "13",
                   "-randinv", "-maxidev", "25", "-maxzangle", "0.9", "-rngseed", "99"]) == 0
    cc.create_training_samples(b, img, 7, 20, 13, invert=S.RANDOM_INVERT, maxintensitydev=25, maxzangle=0.9, backgrounds=bgs, rngseed=99)
    assert open(a, "rb").read() == open(b, "rb").read()
    want = W.generate(img, 7, 20, 13, W.Params(invert=W.RANDOM_INVERT, maxintensitydev=25, maxzangle=0.9), W.RNG(99), bg_images=bgs)
    from cascadeclassifier_amd.detector import vec_read
    assert (vec_read(a).reshape(7, 13, 20) == want).all()
