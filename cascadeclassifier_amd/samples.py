"""Sample synthesis: the trainer's positives from one object image, as the reference's createsamples tool makes them
(tools/createsamples/utility.cpp: cvCreateTrainingSamples). The random draws and the sequential arithmetic run on the host
(cc_sample_plan), the pixels in one HIP kernel per batch of samples (cc_sampler_render); section 8 of the header.

    python -m cascadeclassifier_amd.samples -img object.pgm -vec out.vec -num 1000 -w 24 -h 24

takes the tool's options with the tool's defaults. Images are read as binary .pgm or .npy (no image decoder here).

The tool's test mode (cvCreateTestSamples: one distorted copy pasted into a random rectangle of each background, with the
ground truth in an info file) is cc_testset_plan + cc_sampler_render_testset, create_test_samples here and

    python -m cascadeclassifier_amd.samples -img object.pgm -bg bg.txt -info out/info.dat [-maxscale 4]

The tool's -info mode (cvCreateTrainingSamplesFromInfo: every rectangle an info file annotates, cut out of its image and
resized to the window, INTER_AREA when it shrinks on both axes and INTER_LINEAR_EXACT otherwise) is scan_info +
cc_samples_from_info, create_samples_from_info here and

    python -m cascadeclassifier_amd.samples -info annotations.dat -vec positives.vec -w 24 -h 24
"""
from __future__ import annotations

import ctypes as C
import os
import re
import sys

import numpy as np

from . import _lib as L
from .detector import vec_write

RANDOM_INVERT = L.CC_SAMPLE_RANDOM_INVERT


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


class CvRNG:
    """State of cv::RNG between calls: the tool seeds it with 12345; a seed of 0 becomes 0xffffffff."""

    def __init__(self, seed: int = 12345):
        self.state = (int(seed) & 0xFFFFFFFFFFFFFFFF) or 0xFFFFFFFF


class SampleParams:
    """Options of cvCreateTrainingSamples with the tool's defaults. invert: 0, 1 or RANDOM_INVERT. inscribe / maxshift /
    maxscale are the three values the training mode passes as 0 (cvCreateTestSamples does not)."""

    def __init__(self, bgcolor=0, bgthreshold=80, invert=0, maxintensitydev=40, maxxangle=1.1, maxyangle=1.1, maxzangle=0.5,
                 inscribe=0, maxshift=0.0, maxscale=0.0):
        self.bgcolor, self.bgthreshold, self.invert, self.maxintensitydev = bgcolor, bgthreshold, invert, maxintensitydev
        self.maxxangle, self.maxyangle, self.maxzangle = maxxangle, maxyangle, maxzangle
        self.inscribe, self.maxshift, self.maxscale = inscribe, maxshift, maxscale

    def _c(self) -> L.SampleParams:
        return L.SampleParams(self.bgcolor, self.bgthreshold, self.invert, self.maxintensitydev, self.maxxangle, self.maxyangle,
                              self.maxzangle, int(self.inscribe), 0, self.maxshift, self.maxscale)


class _BgReader:
    """The tool's background reader over a list of image sizes (kept across plan calls)."""

    def __init__(self, sizes):
        self.sizes = np.ascontiguousarray(sizes, np.int32).reshape(-1, 2)
        self.c = L.SampleBgReader()
        self.c.sizes = self.sizes.ctypes.data
        self.c.n_images = len(self.sizes)


def plan(src_w: int, src_h: int, win, params: SampleParams, rng: CvRNG, n: int, bg_sizes=None, _reader=None):
    """Host only. (records, spans): n cc_sample_record structures (a ctypes array) and the (n, canvas rows, 2) int32 row
    spans. bg_sizes: (width, height) of the tool's background images, for records that name their window."""
    out_w, out_h = win
    recs = (L.SampleRecord * max(n, 1))()
    ch = src_h + 2 * (src_h // 2)
    spans = np.zeros((n, ch, 2), np.int32)
    state = C.c_uint64(rng.state)
    reader = _reader if _reader is not None else (_BgReader(bg_sizes) if bg_sizes is not None else None)
    p = params._c()
    L.check(L.lib().cc_sample_plan(src_w, src_h, out_w, out_h, C.byref(p), C.byref(state), C.byref(reader.c) if reader else None, n,
                                   C.cast(recs, C.c_void_p), _vp(spans)))
    rng.state = state.value
    return recs, spans


class TestsetState:
    """What cvCreateTestSamples carries from one iteration to the next, between calls of plan_testset: the background
    reader, the sticky maxscale (negative: taken from the first image drawn) and the iterations made so far."""
    __test__ = False  # not a test class, whatever the name starts with

    def __init__(self, bg_sizes, maxscale: float = -1.0):
        self.reader = _BgReader(bg_sizes)
        self.maxscale = float(maxscale)
        self.iterations = 0


def plan_testset(src_w: int, src_h: int, win, params: SampleParams, rng: CvRNG, num: int, state: TestsetState):
    """Host only: up to num more iterations of cvCreateTestSamples' loop (cc_testset_plan). (items, records, spans) of the
    emitted samples: items is a list of (iteration, bg_index, x, y, width, height), records a ctypes array of
    cc_sample_record, spans (n, canvas rows, 2) int32. rng and state are carried on."""
    win_w, win_h = win
    cap = max(min(num, len(state.reader.sizes)), 1)  # the loop runs MIN(num, images) times in all
    items = (L.TestsetItem * cap)()
    recs = (L.SampleRecord * cap)()
    ch = src_h + 2 * (src_h // 2)
    spans = np.zeros((cap, ch, 2), np.int32)
    rs, ms, done, n = C.c_uint64(rng.state), C.c_double(state.maxscale), C.c_int32(state.iterations), C.c_int32(0)
    p = params._c()
    L.check(L.lib().cc_testset_plan(src_w, src_h, win_w, win_h, C.byref(p), C.byref(rs), C.byref(state.reader.c), C.byref(ms),
                                    C.byref(done), num, C.byref(n), C.cast(items, C.c_void_p),
                                    C.cast(recs, C.c_void_p), _vp(spans)))
    rng.state, state.maxscale, state.iterations = rs.value, ms.value, done.value
    out = [(it.iteration, it.bg_image, it.x, it.y, it.width, it.height) for it in items[:n.value]]
    return out, recs, spans[:n.value]


class Sampler:
    """One object image on the device (icvStartSampleDistortion): generate() turns it into training samples,
    generate_testset() into detection test images."""

    def __init__(self, image, bgcolor: int = 0, bgthreshold: int = 80, device: int = 0):
        image = np.ascontiguousarray(image, np.uint8)
        if image.ndim != 2:
            raise ValueError("Sampler: a gray image (h, w) is required")
        self.h, self.w = image.shape
        self.bgcolor, self.bgthreshold, self.device = bgcolor, bgthreshold, device
        self._s = C.c_void_p()
        self._reader = None
        self._reader_win = None
        self._bg_sizes = None
        self._testset = None
        L.check(L.lib().cc_sampler_create(device, _vp(image), self.w, self.h, self.w, bgcolor, bgthreshold, C.byref(self._s)))

    def close(self):
        if self._s:
            L.lib().cc_sampler_destroy(self._s)
            self._s = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    def set_backgrounds(self, images):
        """The tool's -bg images: samples are then blended onto windows the tool's reader takes from them."""
        imgs = [np.ascontiguousarray(i, np.uint8) for i in images]
        if any(i.ndim != 2 for i in imgs):
            raise ValueError("set_backgrounds: gray images (h, w) are required")
        ptrs = (C.c_void_p * max(len(imgs), 1))(*[i.ctypes.data for i in imgs])
        ws = np.array([i.shape[1] for i in imgs], np.int32)
        hs = np.array([i.shape[0] for i in imgs], np.int32)
        L.check(L.lib().cc_sampler_set_backgrounds(self._s, C.cast(ptrs, C.c_void_p), _vp(ws), _vp(hs), len(imgs)))
        self._reader = _BgReader(np.stack([ws, hs], axis=1)) if imgs else None
        self._reader_win = None
        self._bg_sizes = np.stack([ws, hs], axis=1) if imgs else None
        self._testset = None

    def plan(self, n: int, win, params: SampleParams, rng: CvRNG):
        if self._reader is not None:
            if self._reader_win not in (None, tuple(win)):
                raise ValueError("the background reader was started with another window size")
            self._reader_win = tuple(win)
        self._check(params)
        return plan(self.w, self.h, win, params, rng, n, _reader=self._reader)

    def _check(self, params):
        if (params.bgcolor, params.bgthreshold) != (self.bgcolor, self.bgthreshold):
            raise ValueError("params.bgcolor / bgthreshold differ from the Sampler's")

    def generate(self, n: int, win, params: SampleParams, rng: CvRNG, backgrounds=None, max_batch: int = 0) -> np.ndarray:
        """n samples as (n, h, w) uint8 for the window win = (w, h). backgrounds: (n, h, w) windows to blend onto; None: the
        set_backgrounds images if any, else bgcolor. max_batch > 0 caps the samples per kernel launch."""
        out_w, out_h = win
        recs, spans = self.plan(n, win, params, rng)
        out = np.empty((n, out_h, out_w), np.uint8)
        bg = None
        if backgrounds is not None:
            bg = np.ascontiguousarray(backgrounds, np.uint8)
            if bg.shape != out.shape:
                raise ValueError(f"backgrounds must have shape {out.shape}")
        L.check(L.lib().cc_sampler_render(self._s, C.cast(recs, C.c_void_p), _vp(spans), n, out_w, out_h,
                                          _vp(bg) if bg is not None else None, max_batch, _vp(out)))
        return out

    def restart_testset(self):
        """Forget the test mode's reader and iteration count: the next generate_testset starts the tool's loop again."""
        self._testset = None

    def generate_testset(self, num: int, win, params: SampleParams, rng: CvRNG, maxscale: float = -1.0, max_batch: int = 0,
                         device_out=None, frame_stride: int = 0):
        """Up to num more iterations of cvCreateTestSamples over the set_backgrounds images (MIN(num, images) in all; the
        reader and the iteration count stay in the Sampler until set_backgrounds or restart_testset, so calls of a and b
        equal one of a + b). Returns (samples, maxscale): samples is a list of (image, (x, y, w, h), iteration, bg_index),
        the image a fresh copy of background bg_index with the object in the rectangle; maxscale is the value to pass to
        the next call (a negative one is replaced by the first image's and then kept).
        device_out: a device pointer that receives the images as an (n, rows, cols) stack, frame_stride bytes apart (0:
        rows * cols), with room for MIN(num, images) frames; every image must then have one size, and the list's images
        are None (nothing comes back to the host)."""
        if getattr(self, "_bg_sizes", None) is None:
            raise ValueError("generate_testset: set_backgrounds first")
        self._check(params)
        st = self._testset
        if st is None:
            st = self._testset = TestsetState(self._bg_sizes)
        before = (rng.state, st.maxscale, st.iterations, bytes(st.reader.c))
        st.maxscale = float(maxscale)
        try:
            return self._generate_testset(num, win, params, rng, st, max_batch, device_out, frame_stride)
        except Exception:  # a refused call leaves the stream of draws where it was
            rng.state, st.maxscale, st.iterations = before[:3]
            C.memmove(C.byref(st.reader.c), before[3], len(before[3]))
            raise

    def _generate_testset(self, num, win, params, rng, st, max_batch, device_out, frame_stride):
        items, recs, spans = plan_testset(self.w, self.h, win, params, rng, num, st)
        n = len(items)
        its = (L.TestsetItem * max(n, 1))(*[L.TestsetItem(*it) for it in items])
        images, ptrs = [None] * n, None
        if device_out is None:
            images = [np.empty((int(self._bg_sizes[b][1]), int(self._bg_sizes[b][0])), np.uint8) for _, b, *_ in items]
            ptrs = C.cast((C.c_void_p * max(n, 1))(*[i.ctypes.data for i in images]), C.c_void_p)
        L.check(L.lib().cc_sampler_render_testset(self._s, C.cast(its, C.c_void_p), C.cast(recs, C.c_void_p), _vp(spans), n, max_batch,
                                                  ptrs, C.c_void_p(device_out) if device_out is not None else None, frame_stride))
        return [(images[k], tuple(items[k][2:6]), items[k][0], items[k][1]) for k in range(n)], st.maxscale


def create_training_samples(vec_path: str, image, num: int = 1000, w: int = 24, h: int = 24, *, bgcolor=0, bgthreshold=80,
                            invert=0, maxintensitydev=40, maxxangle=1.1, maxyangle=1.1, maxzangle=0.5, backgrounds=None,
                            rngseed=12345, device=0) -> np.ndarray:
    """cvCreateTrainingSamples: writes num w x h samples of `image` to vec_path and returns them. backgrounds: the images
    of the tool's -bg list."""
    s = Sampler(image, bgcolor, bgthreshold, device)
    try:
        if backgrounds is not None:
            s.set_backgrounds(backgrounds)
        p = SampleParams(bgcolor, bgthreshold, invert, maxintensitydev, maxxangle, maxyangle, maxzangle)
        out = s.generate(num, (w, h), p, CvRNG(rngseed))
    finally:
        s.close()
    vec_write(vec_path, out, w, h)
    return out


def write_gray(path: str, image) -> None:
    """A gray image as a binary .pgm (P5, 8 bit)."""
    image = np.ascontiguousarray(image, np.uint8)
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (image.shape[1], image.shape[0]))
        f.write(image.tobytes())


def write_info(path: str, entries) -> None:
    """The tool's info file (a detection test set's ground truth, or the -info input): per line an image name, a count and
    count rectangles x y w h. entries: (name, rectangles) pairs."""
    with open(path, "w") as f:
        for name, rects in entries:
            rects = [tuple(int(v) for v in r) for r in rects]
            f.write(" ".join([name, str(len(rects))] + ["%d %d %d %d" % r for r in rects]) + "\n")


def read_info(path: str):
    """The entries of an info file as a list of (name, (count, 4) int32 array); names are as written, relative to the file."""
    entries = []
    for line_no, line in enumerate(open(path), 1):
        tok = line.split()
        if not tok:
            continue
        if len(tok) < 2 or not tok[1].isdigit() or len(tok) != 2 + 4 * int(tok[1]):
            raise ValueError(f"{path}:{line_no}: expected 'name count' and count times 'x y w h'")
        entries.append((tok[0], np.array(tok[2:], np.int32).reshape(-1, 4)))
    return entries


def create_test_samples(info_path: str, image, backgrounds, num: int = 1000, w: int = 24, h: int = 24, *, maxscale=-1.0, bgcolor=0,
                        bgthreshold=80, invert=0, maxintensitydev=40, maxxangle=1.1, maxyangle=1.1, maxzangle=0.5, rngseed=12345,
                        device=0):
    """cvCreateTestSamples: MIN(num, len(backgrounds)) times one distorted copy of `image` is pasted into a random rectangle
    of a randomly drawn background (scale 1..maxscale of the w x h window; maxscale < 0: 0.7 of the first image drawn).
    Each image is written next to info_path as "%04d_%04d_%04d_%04d_%04d.pgm" % (iteration, x, y, width, height) (the tool
    writes .jpg, and cuts the name short) with the line "<name> 1 x y width height" in info_path. Returns (images, rects):
    a list of (rows, cols) uint8 arrays and an (n, 4) int32 array."""
    s = Sampler(image, bgcolor, bgthreshold, device)
    try:
        s.set_backgrounds(backgrounds)
        p = SampleParams(bgcolor, bgthreshold, invert, maxintensitydev, maxxangle, maxyangle, maxzangle)
        samples, _ = s.generate_testset(num, (w, h), p, CvRNG(rngseed), maxscale)
    finally:
        s.close()
    base = os.path.dirname(info_path)
    if base:
        os.makedirs(base, exist_ok=True)
    entries = []
    for img, rect, iteration, _ in samples:
        name = "%04d_%04d_%04d_%04d_%04d.pgm" % ((iteration,) + rect)
        write_gray(os.path.join(base, name), img)
        entries.append((name, [rect]))
    write_info(info_path, entries)
    return [smp[0] for smp in samples], np.array([smp[1] for smp in samples], np.int32).reshape(-1, 4)


def area_tab(ssize: int, dsize: int):
    """Host only (cc_area_tab): one axis of cv::resize INTER_AREA from ssize to dsize pixels as (scale, iscale, integer,
    dst_index, src_index, alpha): entry k adds alpha[k] * source[src_index[k]] to destination dst_index[k]."""
    cap = 2 * max(int(ssize), 1)
    di, si, al = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.float32)
    scale, iscale, integer, n = C.c_double(0.0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
    L.check(L.lib().cc_area_tab(ssize, dsize, C.byref(scale), C.byref(iscale), C.byref(integer), _vp(di), _vp(si), _vp(al), cap,
                                C.byref(n)))
    return scale.value, iscale.value, bool(integer.value), di[:n.value], si[:n.value], al[:n.value]


class _Scanner:
    """The token stream fscanf sees: "%s" takes a run of non-blank characters, "%d" an optional sign and digits from the
    front of one and leaves the rest (and anything that does not start like a number) where it is."""
    _INT = re.compile(r"[+-]?\d+")

    def __init__(self, text: str):
        self.tok, self.pos = text.split(), 0

    def word(self):
        if self.pos >= len(self.tok):
            return None
        self.pos += 1
        return self.tok[self.pos - 1]

    def integer(self):
        if self.pos >= len(self.tok):
            return None
        t = self.tok[self.pos]
        m = self._INT.match(t)
        if not m:
            return None
        if m.end() < len(t):
            self.tok[self.pos] = t[m.end():]
        else:
            self.pos += 1
        return int(m.group())


def scan_info(info_path: str, num: int = 1000):
    """The fscanf walk of cvCreateTrainingSamplesFromInfo (utility.cpp:1189-1226) over an info file, without its pixels:
    (entries, bad). entries: (name, [(x, y, w, h), ...]) per entry the walk visits, names as written, `num` rectangles in
    all at most (a count that runs past num is cut). bad: None, or the 1-based number of the entry whose rectangles did
    not parse (end of file inside an entry included); that entry's earlier rectangles are kept and the walk ends there, as
    the tool's does. Unlike read_info this is a token stream: white space of any kind separates, lines mean nothing.
    Where the tool's loop would spin for ever -- the file ends before num rectangles -- the walk ends."""
    sc = _Scanner(open(info_path).read())
    entries, total, entry = [], 0, 1
    while total < num:
        name = sc.word()
        if name is None:  # end of file: the tool reads count = 0 again and again
            break
        count = sc.integer()
        rects = []
        bad = False
        for _ in range(count or 0):  # a name without a count has none, as fscanf(...) != 2 leaves count at 0
            if total >= num:
                break
            r = [sc.integer() for _ in range(4)]
            if None in r:  # fscanf stops at the first field that fails
                bad = True
                break
            rects.append(tuple(r))
            total += 1
        entries.append((name, rects))
        if bad:
            return entries, entry
        entry += 1
    return entries, None


def samples_from_info(images, records, win, device: int = 0, max_batch: int = 0, device_out=None, host: bool = True):
    """cc_samples_from_info: records (image, x, y, width, height) cut out of `images` (gray (h, w) uint8 arrays; rows may be
    strided) and resized to the window win = (w, h): INTER_AREA when the rectangle is at least the window on both axes,
    else INTER_LINEAR_EXACT, the rectangle alone being the source. Returns (n, h, w) uint8, or None when host is False.
    device_out: a device pointer that receives the same (n, h, w) stack. max_batch > 0 caps the records per launch."""
    w, h = win
    imgs = []
    for a in images:
        a = np.asarray(a)
        if a.ndim != 2 or a.dtype != np.uint8:
            raise ValueError("samples_from_info: gray images (h, w) of uint8 are required")
        if a.shape[1] > 1 and a.strides[1] != 1 or a.strides[0] < a.shape[1]:
            a = np.ascontiguousarray(a)
        imgs.append(a)
    recs = np.ascontiguousarray(records, np.int32).reshape(-1, 5)
    n = len(recs)
    ptrs = (C.c_void_p * max(len(imgs), 1))(*[a.ctypes.data for a in imgs])
    ws = np.array([a.shape[1] for a in imgs], np.int32)
    hs = np.array([a.shape[0] for a in imgs], np.int32)
    strides = np.array([a.strides[0] for a in imgs], np.uintp)
    out = np.empty((n, h, w), np.uint8) if host and w > 0 and h > 0 else None
    L.check(L.lib().cc_samples_from_info(device, C.cast(ptrs, C.c_void_p), _vp(ws), _vp(hs), _vp(strides), len(imgs), _vp(recs), n, w, h,
                                         max_batch, _vp(out) if out is not None else None,
                                         C.c_void_p(device_out) if device_out is not None else None))
    return out


def create_samples_from_info(vec_path: str, info_path: str, num: int = 1000, w: int = 24, h: int = 24, device: int = 0,
                             max_batch: int = 0) -> np.ndarray:
    """cvCreateTrainingSamplesFromInfo: the first `num` annotated rectangles of info_path, each cut out of its image (.pgm or
    .npy, named relative to the info file) and resized to w x h, written to vec_path and returned as (n, h, w) uint8.
    A malformed entry ends the run as in the tool: what precedes it is kept and "<info>(<entry>) : parse error" goes to
    stderr. Three deliberate differences: the run ends at the end of the file (the tool's loop spins there for ever); the
    .vec header holds the number of samples written (the tool writes num whatever it made); an image that is missing or
    unreadable raises, naming the file (the tool asserts). An image is read only when a rectangle needs it."""
    entries, bad = scan_info(info_path, num)
    base = os.path.dirname(info_path)
    index, images, records = {}, [], []
    for name, rects in entries:
        if not rects:
            continue
        path = os.path.join(base, name)
        if path not in index:
            try:
                img = read_gray(path)
            except Exception as e:
                raise ValueError(f"{info_path}: image {path} cannot be read: {e}") from e
            index[path] = len(images)
            images.append(img)
        records += [(index[path],) + r for r in rects]
    if bad is not None:
        sys.stderr.write(f"{info_path}({bad}) : parse error")
    out = samples_from_info(images, np.array(records, np.int64).reshape(-1, 5).clip(-2 ** 31, 2 ** 31 - 1), (w, h), device, max_batch)
    if os.path.dirname(vec_path):
        os.makedirs(os.path.dirname(vec_path), exist_ok=True)  # icvMkDir
    vec_write(vec_path, out, w, h)
    return out


def warp_perspective(src, dst, quad, device: int = 0) -> np.ndarray:
    """cvWarpPerspective of the tool: src mapped into the quadrangle quad (4 x 2, x y) of dst, in place; returns dst."""
    src = np.ascontiguousarray(src, np.uint8)
    if not (isinstance(dst, np.ndarray) and dst.dtype == np.uint8 and dst.ndim == 2 and dst.flags.c_contiguous):
        raise ValueError("warp_perspective: dst must be a contiguous (h, w) uint8 array")
    q = np.ascontiguousarray(quad, np.float64).reshape(8)
    L.check(L.lib().cc_warp_perspective_u8(device, _vp(src), src.shape[1], src.shape[0], src.shape[1], _vp(dst), dst.shape[1],
                                           dst.shape[0], dst.shape[1], _vp(q)))
    return dst


def read_gray(path: str) -> np.ndarray:
    """A gray image from a binary .pgm (P5, 8 bit) or a .npy file."""
    if path.endswith(".npy"):
        a = np.load(path)
        if a.ndim != 2 or a.dtype != np.uint8:
            raise ValueError(f"{path}: a (h, w) uint8 array is required")
        return a
    data = open(path, "rb").read()
    tok, pos = [], 0
    while len(tok) < 4:  # magic, width, height, maxval; '#' starts a comment
        while data[pos:pos + 1].isspace():
            pos += 1
        if data[pos:pos + 1] == b"#":
            pos = data.index(b"\n", pos)
            continue
        end = pos
        while end < len(data) and not data[end:end + 1].isspace():
            end += 1
        tok.append(data[pos:end])
        pos = end
    if tok[0] != b"P5" or int(tok[3]) > 255:
        raise ValueError(f"{path}: only 8-bit binary PGM (P5) and .npy are read")
    w, h = int(tok[1]), int(tok[2])
    return np.frombuffer(data, np.uint8, w * h, pos + 1).reshape(h, w).copy()


def read_background_list(path: str):
    """The tool's -bg file: one image path per line, relative to the file; '#' lines are comments."""
    base = os.path.dirname(path)
    names = [l.strip() for l in open(path) if l.strip() and not l.startswith("#")]
    return [read_gray(os.path.join(base, n)) for n in names]


def parse_args(argv=None):
    """(mode, options) of a command line: the mode is chosen as createsamples.cpp:184-212 does -- "training" (-img and
    -vec: a .vec of distorted copies) before "test" (-img, -bg and -info: test images and their info file) before
    "from_info" (-info and -vec without -img: a .vec of annotated rectangles)."""
    import argparse
    ap = argparse.ArgumentParser(prog="python -m cascadeclassifier_amd.samples", add_help=False,
                                 description="createsamples: a .vec of distorted copies of one image (-img -vec), test "
                                             "images with one copy pasted into each background (-img -bg -info), or a .vec "
                                             "of the rectangles an info file annotates (-info -vec)")
    ap.add_argument("--help", action="help")
    ap.add_argument("-img")
    ap.add_argument("-vec")
    ap.add_argument("-info")
    ap.add_argument("-maxscale", type=float, default=-1.0)
    ap.add_argument("-bg")
    ap.add_argument("-num", type=int, default=1000)
    ap.add_argument("-bgcolor", type=int, default=0)
    ap.add_argument("-bgthresh", type=int, default=80)
    ap.add_argument("-inv", action="store_true")
    ap.add_argument("-randinv", action="store_true")
    ap.add_argument("-maxidev", type=int, default=40)
    ap.add_argument("-maxxangle", type=float, default=1.1)
    ap.add_argument("-maxyangle", type=float, default=1.1)
    ap.add_argument("-maxzangle", type=float, default=0.5)
    ap.add_argument("-w", type=int, default=24)
    ap.add_argument("-h", type=int, default=24)
    ap.add_argument("-rngseed", type=int, default=12345)
    a = ap.parse_args(argv)
    if a.img and a.vec:
        return "training", a
    if a.img and a.bg and a.info:
        return "test", a
    if a.info and a.vec:
        return "from_info", a
    ap.error("nothing to do: give -img and -vec (training samples), -img, -bg and -info (test images), or -info and -vec "
             "(samples from annotated images)")


def main(argv=None) -> int:
    mode, a = parse_args(argv)
    invert = RANDOM_INVERT if a.randinv else 1 if a.inv else 0
    if mode == "from_info":
        out = create_samples_from_info(a.vec, a.info, a.num, a.w, a.h)
        print(f"{a.vec}: {len(out)} samples of {a.w} x {a.h}")
        return 0
    if mode == "test":
        images, _ = create_test_samples(a.info, read_gray(a.img), read_background_list(a.bg), a.num, a.w, a.h, maxscale=a.maxscale,
                                        bgcolor=a.bgcolor, bgthreshold=a.bgthresh, invert=invert, maxintensitydev=a.maxidev,
                                        maxxangle=a.maxxangle, maxyangle=a.maxyangle, maxzangle=a.maxzangle, rngseed=a.rngseed)
        print(f"{a.info}: {len(images)} test images")
        return 0
    out = create_training_samples(a.vec, read_gray(a.img), a.num, a.w, a.h, bgcolor=a.bgcolor, bgthreshold=a.bgthresh, invert=invert,
                                  maxintensitydev=a.maxidev, maxxangle=a.maxxangle, maxyangle=a.maxyangle, maxzangle=a.maxzangle,
                                  backgrounds=read_background_list(a.bg) if a.bg else None, rngseed=a.rngseed)
    print(f"{a.vec}: {len(out)} samples of {a.w} x {a.h}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
