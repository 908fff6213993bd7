"""Colour frames on the device: the COLOR_BGR2GRAY conversion (cc_to_gray_u8, k_to_gray) and every detection entry point
that takes colour frames. Expected values come from the integer restatement below (OpenCV's 8-bit RGB2Gray: B2Y 1868,
G2Y 9617, R2Y 4899, shift 14) fed to the CPU oracle; colour results must also equal the gray path on the converted
frames, bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

import cascadeclassifier_amd as cc
from cascadeclassifier_amd import _lib as L
from cascadeclassifier_amd import detector as det
from oracle import oracle as orc
from tests.util import frame_natural

pytestmark = pytest.mark.gpu

DATA = os.path.join(os.path.dirname(__file__), "..", "data")
HAAR = os.path.join(DATA, "haarcascade_frontalface_synthetic.xml")
LBP = os.path.join(DATA, "lbpcascade_frontalface.xml")
FMT = {"gray": 0, "bgr": 1, "bgra": 2, "rgb": 3, "rgba": 4, "rgb_planar": 5}


def restated_gray(img, fmt):
    """gray = (B*1868 + G*9617 + R*4899 + 8192) >> 14 of an (H, W, C) array, or of (3, H, W) planes R, G, B."""
    a = np.asarray(img).astype(np.uint32)
    if fmt == "rgb_planar":
        r, g, b = a[0], a[1], a[2]
    elif fmt in ("bgr", "bgra"):
        b, g, r = a[..., 0], a[..., 1], a[..., 2]
    else:
        r, g, b = a[..., 0], a[..., 1], a[..., 2]
    return ((b * 1868 + g * 9617 + r * 4899 + 8192) >> 14).astype(np.uint8)


def colourise(gray, seed, channels=3):
    """A colour image whose channels differ, built around a natural gray frame (faces included)."""
    rng = np.random.default_rng(seed)
    g = gray.astype(np.int32)
    out = np.stack([np.clip(g + rng.integers(-40, 41, g.shape), 0, 255) for _ in range(channels)], -1).astype(np.uint8)
    return out


def _faces(img, seed, ks=(1.0, 1.7, 2.6, 4.0)):
    tm = np.load(os.path.join(DATA, "face_template_24x24.npy"))
    rng = np.random.default_rng(seed)
    out = img.copy()
    h, w = out.shape
    for k in ks:
        s = int(24 * k)
        if s >= min(h, w):
            continue
        y, x = int(rng.integers(0, h - s)), int(rng.integers(0, w - s))
        out[y:y + s, x:x + s] = orc.resize_linear_exact(tm, s, s)
    return out


def colour_frame(w, h, seed, channels=3):
    """BGR(A) frame whose conversion keeps the pasted faces detectable: every channel carries the face, noise differs."""
    base = _faces(frame_natural(w, h, seed), seed)
    c = colourise(base, seed + 1, channels)
    return c


def _to_gray(src, fmt, w, h, row_stride, ptr=None):
    dst = np.zeros((h, w), np.uint8)
    p = ptr if ptr is not None else src.ctypes.data
    L.check(L.lib().cc_to_gray_u8(0, C.c_void_p(p), FMT[fmt], w, h, row_stride, dst.ctypes.data_as(C.c_void_p), w))
    return dst


def _same_lists(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.shape == y.shape and (x == y).all(), (x, y)


# ---- 1. the conversion ---------------------------------------------------------------------------------------------
def test_to_gray_exhaustive_bgr_triples():
    v = np.arange(1 << 24, dtype=np.uint32)
    img = np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)  # B, G, R
    got = _to_gray(img, "bgr", 4096, 4096, 4096 * 3)
    want = restated_gray(img, "bgr")
    assert (got == want).all()
    # PIL's convert("L") is another formula: it must differ somewhere
    a = img.astype(np.uint32)
    pil = ((a[..., 2] * 19595 + a[..., 1] * 38470 + a[..., 0] * 7471 + 0x8000) >> 16).astype(np.uint8)
    assert (got != pil).any()
    known = {(255, 0, 0): 29, (0, 255, 0): 150, (0, 0, 255): 76, (255, 255, 255): 255, (0, 0, 0): 0}  # (B, G, R)
    for (b, g, r), y in known.items():
        assert got.reshape(-1)[(b << 16) | (g << 8) | r] == y
        assert pil.reshape(-1)[(b << 16) | (g << 8) | r] == y  # the two agree on these five


@pytest.mark.parametrize("fmt", ["gray", "bgr", "bgra", "rgb", "rgba", "rgb_planar"])
def test_to_gray_formats_odd_geometry(fmt):
    rng = np.random.default_rng(FMT[fmt])
    bpp = {"gray": 1, "bgr": 3, "bgra": 4, "rgb": 3, "rgba": 4, "rgb_planar": 1}[fmt]
    for w in (1, 3, 5, 17, 1921):
        for h in (1, 7):
            for offset in (0, 1, 7, 15):
                rs = w * bpp + int(rng.integers(0, 12))
                rs += 1 - rs % 2  # odd row strides
                rows = 3 * h if fmt == "rgb_planar" else h
                buf = rng.integers(0, 256, offset + rs * rows + 16, dtype=np.uint8)  # alpha bytes random too
                view = np.lib.stride_tricks.as_strided(buf[offset:], (rows, w * bpp), (rs, 1))
                if fmt == "gray":
                    want = view.copy()
                elif fmt == "rgb_planar":
                    want = restated_gray(view.reshape(3, h, w), fmt)
                else:
                    want = restated_gray(view.reshape(h, w, bpp), fmt)
                got = _to_gray(buf, fmt, w, h, rs, ptr=buf.ctypes.data + offset)
                assert (got == want).all(), (fmt, w, h, offset, rs)
                if fmt != "gray":
                    assert (det.to_gray(view.reshape((3, h, w) if fmt == "rgb_planar" else (h, w, bpp)), fmt) == want).all()


# ---- 3. single images ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xml", [HAAR, LBP], ids=["haar", "lbp"])
@pytest.mark.parametrize("size", [(640, 480), (1920, 1080)])
@pytest.mark.parametrize("sf,mn", [(1.1, 3), (4.0, 50)])
def test_detect_multiscale_colour(xml, size, sf, mn):
    w, h = size
    bgr = colour_frame(w, h, 7 + w)
    gray = restated_gray(bgr, "bgr")
    p = cc.CascadeClassifier(xml)
    want = orc.detect_multiscale(orc.load_cascade_xml(xml), gray, sf, mn, nthreads=8)
    got = p.detectMultiScale(bgr, sf, mn)
    assert got.shape == want.shape and (got == want).all()
    assert (p.detectMultiScale(gray, sf, mn) == got).all()
    if size == (640, 480):
        rgb = np.ascontiguousarray(bgr[..., ::-1])
        assert (p.detectMultiScale(rgb, sf, mn, pixel_format="rgb") == want).all()
        bgra = np.concatenate([bgr, np.random.default_rng(3).integers(0, 256, (h, w, 1), dtype=np.uint8)], -1)
        assert (p.detectMultiScale(bgra, sf, mn) == want).all()
        rgba = np.ascontiguousarray(bgra[..., [2, 1, 0, 3]])
        assert (p.detectMultiScale(rgba, sf, mn, pixel_format="rgba") == want).all()
        planar = np.ascontiguousarray(rgb.transpose(2, 0, 1))
        assert (p.detectMultiScale(planar, sf, mn, pixel_format="rgb_planar") == want).all()
        r3, l3, w3 = p.detectMultiScale3(bgr, sf, mn)
        rg, lg, wg = p.detectMultiScale3(gray, sf, mn)
        assert (r3 == rg).all() and (l3 == lg).all() and (w3 == wg).all()
        ro, lo, wo = orc.detect_multiscale_levels(orc.load_cascade_xml(xml), gray, sf, mn, nthreads=8)
        assert (r3 == ro).all() and (l3 == lo).all()


# ---- 4. batches ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch11():
    bgr = np.stack([colour_frame(320, 240, 900 + i) for i in range(11)])
    gray = restated_gray(bgr, "bgr")
    return bgr, gray


@pytest.mark.parametrize("n", [1, 2, 5, 11])
def test_detect_batch_host_colour(batch11, n):
    bgr, gray = batch11[0][:n], batch11[1][:n]
    p = cc.CascadeClassifier(HAAR, max_batch=4)
    want = p.detect_batch(gray, 1.1, 2)
    o = orc.load_cascade_xml(HAAR)
    for i in range(min(n, 2)):
        assert (want[i] == orc.detect_multiscale(o, gray[i], 1.1, 2, nthreads=8)).all()
    _same_lists(p.detect_batch(bgr, 1.1, 2), want)
    bgra = np.concatenate([bgr, np.full(bgr.shape[:3] + (1,), 77, np.uint8)], -1)
    _same_lists(p.detect_batch(bgra, 1.1, 2), want)
    _same_lists(p.detect_batch(np.ascontiguousarray(bgr[..., ::-1]), 1.1, 2, pixel_format="rgb"), want)
    if n == 11:  # pinned caller memory takes the copy without the staging area
        import torch
        pinned = torch.from_numpy(bgr).pin_memory()
        _same_lists(p.detect_batch(pinned.numpy(), 1.1, 2), want)


def test_detect_batch_device_colour(batch11):
    import torch
    bgr, gray = batch11
    p = cc.CascadeClassifier(LBP, max_batch=4)
    want = p.detect_batch(gray, 1.1, 2)
    t = torch.from_numpy(bgr).cuda()
    _same_lists(p.detect_batch(None, 1.1, 2, device_ptr=t.data_ptr(), shape=t.shape), want)
    planar = torch.from_numpy(np.ascontiguousarray(bgr[..., ::-1].transpose(0, 3, 1, 2))).cuda()  # (n, 3, H, W) R, G, B
    _same_lists(p.detect_batch(None, 1.1, 2, device_ptr=planar.data_ptr(), shape=planar.shape, pixel_format="rgb_planar"), want)
    # a slice of a wider tensor: padded rows (in bytes)
    wide = torch.zeros((11, 240, 333, 3), dtype=torch.uint8, device="cuda")
    wide[:, :, :320] = t
    _same_lists(p.detect_batch(None, 1.1, 2, device_ptr=wide.data_ptr(), shape=(11, 240, 320, 3), row_stride=333 * 3,
                               frame_stride=333 * 3 * 240), want)
    # odd byte offset and an odd row stride
    n, h, w = 11, 240, 320
    rs, fs = w * 3 + 5, (w * 3 + 5) * h + 3
    flat = torch.zeros(fs * n + 16, dtype=torch.uint8, device="cuda")
    host = np.zeros(fs * n + 16, np.uint8)
    for f in range(n):
        for y in range(h):
            o = 3 + f * fs + y * rs
            host[o:o + w * 3] = bgr[f, y].reshape(-1)
    flat.copy_(torch.from_numpy(host))
    _same_lists(p.detect_batch(None, 1.1, 2, device_ptr=flat.data_ptr() + 3, shape=(n, h, w, 3), row_stride=rs,
                               frame_stride=fs), want)
    torch.cuda.synchronize()


# ---- 5. candidate-list overflow ---------------------------------------------------------------------------------
def test_colour_survives_overflow_redo(batch11, monkeypatch):
    import torch
    bgr, gray = batch11
    ref = cc.CascadeClassifier(HAAR, max_batch=4)
    want = ref.detect_batch(gray, 1.1, 2)
    monkeypatch.setenv("CCAMD_CAND_CAP", "16")
    p = cc.CascadeClassifier(HAAR, max_batch=4)
    _same_lists(p.detect_batch(bgr, 1.1, 2), want)
    t = torch.from_numpy(bgr).cuda()
    q = cc.CascadeClassifier(HAAR, max_batch=4)
    _same_lists(q.detect_batch(None, 1.1, 2, device_ptr=t.data_ptr(), shape=t.shape), want)
    r = cc.CascadeClassifier(HAAR, max_batch=4)
    assert (r.detectMultiScale(bgr[0], 1.1, 2) == want[0]).all()


# ---- 6. submit / collect ---------------------------------------------------------------------------------------
def test_submit_collect_gray_and_colour_interleaved(batch11):
    bgr, gray = batch11
    p = cc.CascadeClassifier(HAAR, max_batch=4)
    want_a = p.detect_batch(gray[:7], 1.1, 2)
    want_b = p.detect_batch(gray[4:], 1.1, 2)
    for first, second in (("gray", "colour"), ("colour", "gray")):
        src = {"gray": (gray[:7], gray[4:]), "colour": (bgr[:7], bgr[4:])}
        t1 = p.detect_batch_submit(src[first][0], 1.1, 2)
        t2 = p.detect_batch_submit(src[second][1], 1.1, 2)  # retires t1's last pass while its own first pass runs
        t3 = p.detect_batch_submit(src[first][1], 1.1, 2)
        _same_lists(p.detect_batch_collect(t1), want_a)
        _same_lists(p.detect_batch_collect(t2), want_b)
        _same_lists(p.detect_batch_collect(t3), want_b)


def test_pending_pass_of_one_format_survives_a_submit_of_the_other():
    """A submitted batch's last pass stays pending while the next submit stages its own frames into the pinned staging
    area. Here the pending pass's copy to the device is held back (the front stream waits for work queued on the caller's
    stream), so a staging slot of the other format that overlapped the pending pass's slot would be overwritten before that
    copy reads it. Both orders, at every position of the slot round-robin: every result must be right."""
    import torch
    bgr = np.stack([colour_frame(640, 480, 7100 + i) for i in range(2)])
    bgra = np.concatenate([bgr, np.full(bgr.shape[:3] + (1,), 200, np.uint8)], -1)
    gray = restated_gray(bgr, "bgr")
    p = cc.CascadeClassifier(HAAR, max_batch=1)
    want = [p.detectMultiScale(gray[i], 1.1, 2) for i in range(2)]
    assert all(len(w) for w in want)
    p.detect_batch(bgra, 1.1, 2)  # the staging area reaches its colour size (growing it waits for the device)
    s = torch.cuda.Stream()
    a = torch.randn(4096, 4096, device="cuda")
    p.set_stream(s.cuda_stream)
    p.set_profiling(True)  # single frames take the ordinary pass path (not the single-image graph), so they stay pending
    try:
        for shift in range(3):
            for first, second in ((gray, bgra), (bgra, gray)):
                with torch.cuda.stream(s):
                    for _ in range(150):  # ~0.1 s of work ahead of the first submit's copy on the caller's stream
                        a = torch.tanh(a @ a * 1e-4)
                t1 = p.detect_batch_submit(first[:1], 1.1, 2)
                t2 = p.detect_batch_submit(second[1:], 1.1, 2)
                _same_lists(p.detect_batch_collect(t1), want[:1])
                _same_lists(p.detect_batch_collect(t2), want[1:])
            p.detect_batch(gray[:1], 1.1, 2)  # moves the round-robin on by one slot
    finally:
        p.set_profiling(False)
        s.synchronize()
        p.set_stream(None)


# ---- 7. graphs ---------------------------------------------------------------------------------------------------
def test_single_image_graphs_per_format():
    bgr = colour_frame(640, 480, 4242)
    gray = restated_gray(bgr, "bgr")
    p = cc.CascadeClassifier(HAAR)
    want = orc.detect_multiscale(orc.load_cascade_xml(HAAR), gray, 1.1, 3, nthreads=8)
    active, captures = [], []
    for img in (gray, bgr, gray, bgr, gray, bgr, gray, bgr):
        got = p.detectMultiScale(img, 1.1, 3)
        assert got.shape == want.shape and (got == want).all()
        active.append(p.graph_active())
        captures.append(p.graph_captures())
    assert active[2:] == [True] * 6, active
    # one capture per format (calls 3 and 4); every later call replays its format's graph without capturing again
    assert captures == [0, 0, 1, 2, 2, 2, 2, 2], captures


# ---- 8. a caller stream -------------------------------------------------------------------------------------------
def test_caller_stream_colour_frames(batch11):
    import torch
    bgr, gray = batch11
    p = cc.CascadeClassifier(HAAR, max_batch=4)
    want = p.detect_batch(gray, 1.1, 2)
    s = torch.cuda.Stream()
    src = torch.from_numpy(bgr).pin_memory()
    with torch.cuda.stream(s):
        t = torch.empty(bgr.shape, dtype=torch.uint8, device="cuda")
        t.copy_(src, non_blocking=True)
        planar = t.flip(-1).permute(0, 3, 1, 2).contiguous()
        p.set_stream(s.cuda_stream)
        got = p.detect_batch(None, 1.1, 2, device_ptr=t.data_ptr(), shape=t.shape)
        got_p = p.detect_batch(None, 1.1, 2, device_ptr=planar.data_ptr(), shape=planar.shape, pixel_format="rgb_planar")
    s.synchronize()
    _same_lists(got, want)
    _same_lists(got_p, want)


# ---- 9. errors -----------------------------------------------------------------------------------------------------
def test_colour_errors():
    from tests.hog_cascade_factory import hog_cascade
    p = cc.CascadeClassifier(HAAR)
    with pytest.raises(cc.CascadeError) as e:
        p.detectMultiScale(np.zeros((48, 64, 2), np.uint8))
    assert e.value.status == L.CC_ERR_INVALID_ARG
    with pytest.raises(cc.CascadeError) as e:
        p.detectMultiScale(np.zeros((48, 64, 3), np.uint8), pixel_format="yuv")
    assert e.value.status == L.CC_ERR_INVALID_ARG
    d = p._detector()
    prm = L.DetectParams(1.1, 3, 0, 0, 0, 0)
    img = np.zeros((48, 64, 3), np.uint8)
    out = np.zeros((16, 4), np.int32)
    n = C.c_int(0)
    for fmt, rs in ((9, 64 * 3), (-1, 64 * 3), (1, 64 * 3 - 1), (2, 64 * 3), (5, 63)):  # unknown formats, short rows
        st = L.lib().cc_detect_multiscale_fmt(d, img.ctypes.data_as(C.c_void_p), 64, 48, rs, fmt, C.byref(prm),
                                              out.ctypes.data_as(C.c_void_p), 16, C.byref(n))
        assert st == L.CC_ERR_INVALID_ARG, (fmt, rs)
    offs = np.zeros(3, np.int32)
    frames = np.zeros((2, 48, 64, 3), np.uint8)
    st = L.lib().cc_detect_batch_fmt(d, frames.ctypes.data_as(C.c_void_p), 0, 2, 64, 48, 64 * 3, 64 * 3 * 48 - 1, 1, C.byref(prm),
                                     out.ctypes.data_as(C.c_void_p), 16, offs.ctypes.data_as(C.c_void_p))
    assert st == L.CC_ERR_INVALID_ARG  # frame stride shorter than a BGR frame
    st = L.lib().cc_detect_batch_fmt(d, frames.ctypes.data_as(C.c_void_p), 0, 2, 64, 48, 64, 64 * 48 * 3 - 1, 5, C.byref(prm),
                                     out.ctypes.data_as(C.c_void_p), 16, offs.ctypes.data_as(C.c_void_p))
    assert st == L.CC_ERR_INVALID_ARG  # ... and than a planar one
    dst = np.zeros((48, 64), np.uint8)
    assert L.lib().cc_to_gray_u8(0, img.ctypes.data_as(C.c_void_p), 6, 64, 48, 64 * 4, dst.ctypes.data_as(C.c_void_p), 64) == L.CC_ERR_INVALID_ARG
    assert L.lib().cc_to_gray_u8(0, img.ctypes.data_as(C.c_void_p), 2, 64, 48, 64 * 3, dst.ctypes.data_as(C.c_void_p), 64) == L.CC_ERR_INVALID_ARG
    rng = np.random.default_rng(1)
    xml, _, _ = hog_cascade(rng.integers(0, 256, (40, 24, 24), dtype=np.uint8))
    h = cc.CascadeClassifier()
    assert h.load_from_string(xml)
    with pytest.raises(cc.CascadeError) as e:
        h.detectMultiScale(img)
    assert e.value.status == L.CC_ERR_UNSUPPORTED
