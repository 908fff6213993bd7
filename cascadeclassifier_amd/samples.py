"""Sample synthesis: the trainer's positives from one object image, as the reference's createsamples tool makes them
(tools/createsamples/utility.cpp: cvCreateTrainingSamples). The random draws and the sequential arithmetic run on the host
(cc_sample_plan), the pixels in one HIP kernel per batch of samples (cc_sampler_render); section 8 of the header.

    python -m cascadeclassifier_amd.samples -img object.pgm -vec out.vec -num 1000 -w 24 -h 24

takes the tool's options with the tool's defaults. Images are read as binary .pgm or .npy (no image decoder here).
"""
from __future__ import annotations

import ctypes as C
import os
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


class Sampler:
    """One object image on the device (icvStartSampleDistortion): generate() turns it into training samples."""

    def __init__(self, image, bgcolor: int = 0, bgthreshold: int = 80, device: int = 0):
        image = np.ascontiguousarray(image, np.uint8)
        if image.ndim != 2:
            raise ValueError("Sampler: a gray image (h, w) is required")
        self.h, self.w = image.shape
        self.bgcolor, self.bgthreshold, self.device = bgcolor, bgthreshold, device
        self._s = C.c_void_p()
        self._reader = None
        self._reader_win = None
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


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m cascadeclassifier_amd.samples", add_help=False,
                                 description="createsamples: a .vec of distorted copies of one image")
    ap.add_argument("--help", action="help")
    ap.add_argument("-img", required=True)
    ap.add_argument("-vec", required=True)
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
    invert = RANDOM_INVERT if a.randinv else 1 if a.inv else 0
    out = create_training_samples(a.vec, read_gray(a.img), a.num, a.w, a.h, bgcolor=a.bgcolor, bgthreshold=a.bgthresh, invert=invert,
                                  maxintensitydev=a.maxidev, maxxangle=a.maxxangle, maxyangle=a.maxyangle, maxzangle=a.maxzangle,
                                  backgrounds=read_background_list(a.bg) if a.bg else None, rngseed=a.rngseed)
    print(f"{a.vec}: {len(out)} samples of {a.w} x {a.h}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
