"""The integral bands' column sums come from the pyramid kernel (k_resize) or, for a level the caller brings itself,
from k_band_colsums; k_integral_band scans them as one more row. Everything is integer arithmetic modulo 2^32, so every
comparison here is exact: integral() against numpy's cumsum in uint32, the resize-fed path (detector, negative miner)
against the CPU oracle, at sizes that reach every edge of those kernels (widths around multiples of 4 and of the
256-column chunk, heights around the 8-row band, levels whose width is a multiple of 4 -- the integral row then has a
quad the pyramid row lacks)."""
import os

import numpy as np
import pytest

import cascadeclassifier_amd as cc
from cascadeclassifier_amd import detector as det
from oracle import oracle as orc
from tests import cascade_factory as cf
from tests.front_cases import integral_witness as _cumsum_u32
from tests.test_gpu_negmine import _truncated
from tests.util import frame_natural, frame_uniform

pytestmark = pytest.mark.gpu


def _check_integral(img):
    g = det.integral(img, sqsum=True)
    assert g["sum"].shape == (img.shape[0] + 1, img.shape[1] + 1)
    assert (g["sum"] == _cumsum_u32(img, False)).all()
    assert (g["sqsum"] == _cumsum_u32(img, True)).all()


@pytest.mark.parametrize("h", [1, 7, 8, 9, 17])
@pytest.mark.parametrize("w", [1, 3, 4, 5, 255, 256, 257, 1021])
def test_integral_equals_cumsum(w, h):
    _check_integral(frame_uniform(w, h, 100 * w + h))
    _check_integral(np.full((h, w), 255, np.uint8))


def test_integral_of_saturated_full_hd_wraps():
    img = np.full((1080, 1920), 255, np.uint8)
    assert 255 * 255 * img.size > 2 ** 32
    _check_integral(img)


def _check_detector(path, frames, haar):
    """debug_windows / detect_raw of every frame and the rectangles of the frames as one batch against the oracle."""
    o = orc.load_cascade_xml(path)
    p = cc.CascadeClassifier(path, max_batch=len(frames))
    assert not p.empty(), getattr(p, "load_error", "")
    n_cand = 0
    for img in frames:
        ref = orc.detect_raw(o, img, 1.1, (0, 0), (0, 0), nthreads=8, full=True)
        codes, sums, vis = p.debug_windows(img, 1.1)
        assert len(codes) == ref.n_grid_windows
        assert (codes == ref.codes).all(), f"{(codes != ref.codes).sum()} window results differ"
        assert (sums == ref.sums).all()
        assert (vis == ref.visited).all()
        raw = p.detect_raw(img, 1.1)
        assert raw.shape == ref.candidates.shape and (raw == ref.candidates).all()
        n_cand += len(raw)
    got = p.detect_batch(np.stack(frames), 1.1, 2)
    for i, img in enumerate(frames):
        want = orc.detect_multiscale(o, img, 1.1, 2, nthreads=8)
        assert got[i].shape == want.shape and (got[i] == want).all(), i
    return n_cand


def _faces(img, seed):
    from tests.test_gpu_detect import _faces as paste
    return paste(img, seed)


@pytest.mark.parametrize("w,h", [(333, 251), (1283, 727)])
@pytest.mark.parametrize("kind", ["haar", "lbp"])
def test_resize_fed_integrals_in_the_detector(tmp_path, haar_xml, lbp_xml, kind, w, h):
    """Scaled sizes that are no multiples of 4 or 8, a batch of 3 frames; the LBP cascade runs without squared sums."""
    path = _truncated(haar_xml, 6, str(tmp_path)) if kind == "haar" else _truncated(lbp_xml, 4, str(tmp_path))
    frames = [_faces(frame_natural(w, h, 60 + i), i) for i in range(2)] + [frame_uniform(w, h, 63)]
    _check_detector(path, frames, kind == "haar")


def test_resize_fed_integrals_with_a_tilted_cascade(tmp_path):
    """The tilted kernels still read the pyramid the resize kernel wrote."""
    calib = frame_natural(320, 240, 3)
    wins = np.stack([calib[y:y + 24, x:x + 24] for y in range(0, 200, 9) for x in range(0, 280, 11)])
    path = os.path.join(str(tmp_path), "tilted.xml")
    open(path, "w").write(cf.tilted_stump_cascade(wins))
    frames = [frame_natural(333, 251, 70 + i) for i in range(3)]
    assert _check_detector(path, frames, True) > 0


@pytest.mark.parametrize("kind", ["haar3", "lbp4"])
@pytest.mark.parametrize("w,h", [(300, 200), (1283, 727)])
def test_negative_miner_on_resize_fed_integrals(tmp_path, haar_xml, lbp_xml, kind, w, h):
    path = _truncated(haar_xml, 3, str(tmp_path)) if kind == "haar3" else _truncated(lbp_xml, 4, str(tmp_path))
    o = orc.load_cascade_xml(path)
    m = cc.NegativeMiner(cc.CascadeClassifier(path))
    img = frame_natural(w, h, 80)
    for ox, oy in ((0, 0), (5, 2)):
        want_f, want_p, want_i = orc.negmine_image(o, img, ox, oy, max_keep=40)
        got_f, got_p, got_i = m.run(img, ox, oy, max_keep=40)
        assert got_f.shape == want_f.shape and (got_f == want_f).all(), f"{(got_f != want_f).sum()} of {len(want_f)} windows differ"
        assert (got_i == want_i).all() and (got_p == want_p).all()
