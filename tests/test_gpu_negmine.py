"""Batched negative mining (cc_negminer_*) against the reference's window-by-window loop as restated by the oracle
(NegReader::get + setImage + CvCascadeClassifier::predict; imagestorage.cpp:57-126, cascadeclassifier.cpp:329-357):
identical pass flags for every window of the reader's stream, identical pixels for the accepted windows."""
import os

import numpy as np
import pytest

import cascadeclassifier_amd as cc
from oracle import oracle as orc
from tests import cascade_factory as cf
from tests.util import frame_natural, frame_uniform
from tests.util import truncated_cascade as _truncated


def _reference_negative():  # test_integration.cpp:59-64
    r, c = np.mgrid[0:128, 0:256]
    return ((r * 7 + c * 13) & 0xFF).astype(np.uint8)


@pytest.mark.gpu
def test_plan_matches_reader_stream_length(haar_xml):
    """The ladder / window census equals the length of the oracle's literal reader loop."""
    o = orc.load_cascade_xml(haar_xml)
    m = cc.NegativeMiner(cc.CascadeClassifier(haar_xml))
    for (w, h, ox, oy) in [(256, 128, 0, 0), (256, 128, 5, 3), (100, 75, 0, 0), (640, 480, 23, 23), (24, 24, 0, 0), (31, 200, 7, 0)]:
        flags, _, _ = orc.negmine_image(o, frame_uniform(w, h, 1), ox, oy, max_keep=0)
        assert m.plan(w, h, ox, oy)["n_windows"] == len(flags)


def test_haar9_takes_the_wave_walk(tmp_path, haar_xml):
    """CPU only. The bundled Haar cascade cut to 9 stages is a stump cascade whose stage sums are exact in any order (the
    miner's condition for one wavefront per window), and its last stages hold more than 64 stumps, so lanes of the wave
    walk take a second stump; haar3 and haar6 stop short of that."""
    from tests import cascade_edges as ce
    sizes = {n: [sl.stop - sl.start for sl in ce.stage_slices(orc.load_cascade_xml(_truncated(haar_xml, n, str(tmp_path))))] for n in (6, 9)}
    assert max(sizes[6]) <= 64 < max(sizes[9]) and len(sizes[9]) == 9
    assert ce.order_independent(orc.load_cascade_xml(_truncated(haar_xml, 9, str(tmp_path))), 1)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["haar3", "haar6", "haar9", "lbp4", "lbp_full", "haar_tilted", "haar_trees", "lbp_trees"])
def test_negative_mining_matches_reader_loop(tmp_path, haar_xml, lbp_xml, kind):
    """haar9: stages of more than 64 stumps, the second round of lanes of the wave walk (test_haar9_takes_the_wave_walk)."""
    tmp = str(tmp_path)
    calib = frame_natural(320, 240, 3)
    wins = np.stack([calib[y:y + 24, x:x + 24] for y in range(0, 200, 9) for x in range(0, 280, 11)])
    if kind.startswith("haar") and kind[4:].isdigit():
        path = _truncated(haar_xml, int(kind[4:]), tmp)
    elif kind == "lbp4":
        path = _truncated(lbp_xml, 4, tmp)
    elif kind == "lbp_full":
        path = lbp_xml
    else:
        xml = {"haar_tilted": lambda: cf.tilted_stump_cascade(wins), "haar_trees": lambda: cf.haar_tree_cascade(wins, with_tilted=True),
               "lbp_trees": cf.lbp_tree_cascade}[kind]()
        path = os.path.join(tmp, kind + ".xml")
        open(path, "w").write(xml)
    o = orc.load_cascade_xml(path)
    c = cc.CascadeClassifier(path)
    assert not c.empty(), getattr(c, "load_error", "")
    m = cc.NegativeMiner(c)
    images = [(_reference_negative(), 0, 0), (frame_natural(333, 211, 41), 5, 2), (frame_uniform(100, 64, 42), 23, 23),
              (frame_natural(640, 480, 43), 0, 17)]
    total_pass = 0
    for img, ox, oy in images:
        want_f, want_p, want_i = orc.negmine_image(o, img, ox, oy, max_keep=40)
        got_f, got_p, got_i = m.run(img, ox, oy, max_keep=40)
        assert got_f.shape == want_f.shape and (got_f == want_f).all(), f"{(got_f != want_f).sum()} of {len(want_f)} windows differ"
        assert (got_i == want_i).all() and (got_p == want_p).all()
        total_pass += int(want_f.sum())
    if kind not in ("lbp_full",):
        assert total_pass > 0


@pytest.mark.gpu
def test_haar9_through_training_side_predict(tmp_path, haar_xml):
    """The cascade that takes the miner's wave walk, through the evaluator's serial walk on stored samples: both walks are
    held to the oracle on the same cascade."""
    from cascadeclassifier_amd import evaluator as ev
    path = _truncated(haar_xml, 9, str(tmp_path))
    tm = np.load(os.path.join(os.path.dirname(haar_xml), "face_template_24x24.npy"))
    rng = np.random.default_rng(5)
    near = np.clip(tm[None].astype(np.float64) + rng.normal(0, 6, (60, 24, 24)), 0, 255).astype(np.uint8)
    calib = frame_natural(320, 240, 3)
    wins = np.stack([calib[y:y + 24, x:x + 24] for y in range(0, 200, 9) for x in range(0, 280, 11)])
    imgs = np.concatenate([near, wins[:240]])
    e = cc.CvFeatureEvaluator.create(ev.HAAR)
    e.init(cc.CvFeatureParams(ev.HAAR, ev.BASIC), len(imgs), (24, 24))
    e.setImages(imgs)
    got = e.predict_cascade(cc.CascadeClassifier(path))
    o = orc.load_cascade_xml(path)
    s, t, nf = orc.set_images(imgs)
    want = np.array([orc.train_predict(o, s, t, nf, i, 24, 24) for i in range(len(imgs))], np.uint8)
    assert (got == want).all() and 0 < want.sum() < len(imgs)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["haar3", "lbp4", "haar_tilted", "haar_trees"])
def test_batch_of_images_equals_one_call_per_image(tmp_path, haar_xml, lbp_xml, kind):
    """cc_negminer_run_batch over several images of one size and offset = cc_negminer_run on each (and the oracle's reader
    loop on the first and last): flags per image, and the kept windows are the first max_keep passing ones in stream order
    across the images. Calls with other sizes / offsets in between exercise the plan cache."""
    tmp = str(tmp_path)
    calib = frame_natural(320, 240, 3)
    wins = np.stack([calib[y:y + 24, x:x + 24] for y in range(0, 200, 9) for x in range(0, 280, 11)])
    if kind == "haar3":
        path = _truncated(haar_xml, 3, tmp)
    elif kind == "lbp4":
        path = _truncated(lbp_xml, 4, tmp)
    else:
        xml = {"haar_tilted": lambda: cf.tilted_stump_cascade(wins), "haar_trees": lambda: cf.haar_tree_cascade(wins, with_tilted=True)}[kind]()
        path = os.path.join(tmp, kind + ".xml")
        open(path, "w").write(xml)
    o = orc.load_cascade_xml(path)
    m = cc.NegativeMiner(cc.CascadeClassifier(path))
    imgs = [frame_natural(300, 200, 70 + k) for k in range(5)] + [frame_uniform(300, 200, 90)]
    for ox, oy, keep in ((0, 0, 37), (7, 3, 500), (0, 0, 0)):
        m.run(frame_natural(123, 77, 5), 1, 1)  # another plan in between
        single = [m.run(im, ox, oy, max_keep=10 ** 6) for im in imgs]
        flags, pix, idx = m.run_batch(imgs, ox, oy, max_keep=keep)
        assert flags.shape == (len(imgs), len(single[0][0]))
        for k, (f1, p1, i1) in enumerate(single):
            assert (flags[k] == f1).all(), f"image {k}: {(flags[k] != f1).sum()} windows differ"
        want_idx = np.concatenate([i1 + k * flags.shape[1] for k, (f1, p1, i1) in enumerate(single)])[:keep]
        want_pix = np.concatenate([p1 for f1, p1, i1 in single])[:keep]
        assert (idx == want_idx).all() and (pix == want_pix).all()
        for k in (0, len(imgs) - 1):
            assert (flags[k] == orc.negmine_image(o, imgs[k], ox, oy, max_keep=1)[0]).all()
    with pytest.raises(ValueError):
        m.run_batch([imgs[0], frame_natural(301, 200, 1)])


@pytest.mark.gpu
def test_negative_miner_argument_checks(haar_xml):
    m = cc.NegativeMiner(cc.CascadeClassifier(haar_xml))
    with pytest.raises(cc.CascadeError):
        m.run(frame_uniform(64, 64, 1), ox=50, oy=0)  # offset leaves no room for the window (nextImg would skip it)
    with pytest.raises(cc.CascadeError):
        m.run(frame_uniform(20, 64, 1))


# ---- batches that do not fit one staging piece -------------------------------------------------------------------
# mine_images stages a batch in pieces of at least 8 MiB and launches every kernel once per piece at the piece's first
# image: source, pyramid, integrals, band sums, diagonal sums, segment totals and pass flags are all offset by it. The
# batches above are one piece each; these are two, and the first piece is staged by several threads.
# The library does not report how it cut a batch, so _pieces is a copy by hand of mine_images' arithmetic (8 MiB per piece,
# at most 4 staging threads, one per 2 MiB): its assertions guard this copy. Whoever changes those constants in
# cc_negmine.hip changes them here, and the image counts below with them, or these batches silently become one piece.
STAGING_PIECE_BYTES = 8 << 20


def _pieces(w, h, k):
    """(images per piece, pieces, staging threads of the first piece) as mine_images derives them."""
    src_bytes = (w + 3) // 4 * 4 * h
    per = max(1, STAGING_PIECE_BYTES // src_bytes)
    n = min(per, k)
    return per, (k + per - 1) // per, min(4, n, max(1, (n * src_bytes) >> 21))


def _check_multi_piece_batch(path, imgs, expect_threads):
    o = orc.load_cascade_xml(path)
    c = cc.CascadeClassifier(path)
    assert not c.empty(), getattr(c, "load_error", "")
    m = cc.NegativeMiner(c)
    h, w = imgs[0].shape
    k = len(imgs)
    per, n_pieces, threads = _pieces(w, h, k)
    assert n_pieces >= 2 and threads == expect_threads, (per, n_pieces, threads)
    wins = m.plan(w, h)["n_windows"]
    single = [m.run(im, max_keep=wins) for im in imgs]
    # a stale offset would hand an image the flags of a neighbour, or of the image at the same place of the other piece
    for a in range(k - 1):
        assert (single[a][0] != single[a + 1][0]).any(), a
    for a in range(per, k):
        assert (single[a][0] != single[a - per][0]).any(), a
    passed = [int(f.sum()) for f, _, _ in single]
    first, second = sum(passed[:per]), sum(passed[per:])
    assert first > 0 and second >= 2
    keep = first + (second + 1) // 2  # the kept windows start in piece one and end inside piece two
    flags, pix, idx = m.run_batch(imgs, max_keep=keep)
    assert flags.shape == (k, wins)
    for a, (f1, _, _) in enumerate(single):
        assert (flags[a] == f1).all(), f"image {a}: {(flags[a] != f1).sum()} windows differ"
    want_idx = np.concatenate([i1 + a * wins for a, (_, _, i1) in enumerate(single)])[:keep]
    want_pix = np.concatenate([p1 for _, p1, _ in single])[:keep]
    assert len(idx) == keep and idx[0] < per * wins <= idx[-1]
    assert (idx == want_idx).all() and (pix == want_pix).all()
    for a in sorted({0, per - 1, per, k - 1}):
        want_f, want_p, _ = orc.negmine_image(o, imgs[a], 0, 0, max_keep=wins)
        assert (flags[a] == want_f).all(), a
        assert (single[a][1] == want_p).all(), a


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["haar3", "haar_tilted"])
def test_batch_of_two_pieces_staged_by_four_threads(tmp_path, haar_xml, kind):
    """9 images of 1024x1024: 1 MiB each, pieces of 8 and 1, the first staged by 4 threads with whole-image copies (the
    width is a multiple of 4). haar3 runs the wave kernel; the tilted cascade also offsets the diagonal sums and the
    segment totals."""
    if kind == "haar3":
        path = _truncated(haar_xml, 3, str(tmp_path))
    else:
        calib = frame_natural(320, 240, 3)
        wins = np.stack([calib[y:y + 24, x:x + 24] for y in range(0, 200, 9) for x in range(0, 280, 11)])
        path = os.path.join(str(tmp_path), "tilted.xml")
        open(path, "w").write(cf.tilted_stump_cascade(wins))
    assert _pieces(1024, 1024, 9)[:2] == (8, 2)
    _check_multi_piece_batch(path, [frame_natural(1024, 1024, 500 + a) for a in range(9)], 4)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["lbp4", "haar_trees"])
def test_batch_of_256_images_in_two_pieces_staged_row_by_row(tmp_path, lbp_xml, kind):
    """256 images (the most a call takes) of 190x176: the pitch is 192, so rows are copied one by one; 248 images fit a
    piece, which 3 threads stage, and 8 are left for the second. The tree cascade runs the thread-per-window kernel."""
    if kind == "lbp4":
        path = _truncated(lbp_xml, 4, str(tmp_path))
    else:
        calib = frame_natural(320, 240, 3)
        wins = np.stack([calib[y:y + 24, x:x + 24] for y in range(0, 200, 9) for x in range(0, 280, 11)])
        path = os.path.join(str(tmp_path), "trees.xml")
        open(path, "w").write(cf.haar_tree_cascade(wins))
    assert _pieces(190, 176, 256)[:2] == (248, 2)
    _check_multi_piece_batch(path, [frame_natural(190, 176, 600 + a) for a in range(256)], 3)


@pytest.mark.gpu
def test_batch_refusals_leave_the_miner_usable(tmp_path, haar_xml):
    """Through the C ABI: more than 256 images and a flag buffer one entry short are refused, the latter still reports the
    windows per image, and the next valid call returns the bits it returned before."""
    import ctypes as C
    from cascadeclassifier_amd import _lib as L
    m = cc.NegativeMiner(cc.CascadeClassifier(_truncated(haar_xml, 3, str(tmp_path))))
    w, h, k = 100, 75, 3
    imgs = [frame_natural(w, h, 700 + a) for a in range(k)]
    before = m.run_batch(imgs, max_keep=50)
    wins = before[0].shape[1]
    assert before[0].sum() > 0

    def call(images, cap):
        ptrs = (C.c_void_p * len(images))(*[im.ctypes.data for im in images])
        flags = np.zeros(max(wins * len(images), 1), np.uint8)
        pix, idx = np.zeros((50, 24, 24), np.uint8), np.zeros(50, np.int64)
        nw, nk = C.c_int64(-1), C.c_int(0)
        st = L.lib().cc_negminer_run_batch(m._m, ptrs, len(images), w, h, w, 0, 0, flags.ctypes.data_as(C.c_void_p), cap, C.byref(nw),
                                           pix.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p), 50, C.byref(nk))
        return st, nw.value

    def same_as_before():
        again = m.run_batch(imgs, max_keep=50)
        assert all((a == b).all() for a, b in zip(again, before))

    assert call([imgs[a % k] for a in range(257)], wins * 257)[0] == L.CC_ERR_INVALID_ARG
    same_as_before()
    assert call([imgs[a % k] for a in range(256)], wins * 256)[0] == L.CC_OK
    same_as_before()
    assert call(imgs, wins * k - 1) == (L.CC_ERR_BUFFER_TOO_SMALL, wins)
    same_as_before()
    assert call(imgs, wins * k)[0] == L.CC_OK
