"""Python host mirror of the detection boundary: a CascadeClassifier with the call shape of cv2.CascadeClassifier as
the reference's Python tool uses it (tools/detection/Python/detect.py:16,22), on top of the C ABI."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib as L


def _params(scale_factor, min_neighbors, min_size, max_size) -> L.DetectParams:
    mn = min_size or (0, 0)
    mx = max_size or (0, 0)
    return L.DetectParams(float(scale_factor), int(min_neighbors), int(mn[0]), int(mn[1]), int(mx[0]), int(mx[1]))


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _view(ptr, ctype, n):
    if not ptr or n == 0:
        return np.zeros(0, np.dtype(ctype))
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(n,)).copy()


@dataclass
class CascadeModel:
    info: dict
    stage_first: np.ndarray
    stage_ntrees: np.ndarray
    stage_threshold: np.ndarray
    stump_feature: np.ndarray | None
    stump_threshold: np.ndarray | None
    stump_left: np.ndarray | None
    stump_right: np.ndarray | None
    stump_subsets: np.ndarray | None
    rects: np.ndarray
    weights: np.ndarray | None
    tilted: np.ndarray | None


def scale_plan(win_w, win_h, width, height, scale_factor=1.1, min_size=None, max_size=None) -> np.ndarray:
    p = _params(scale_factor, 3, min_size, max_size)
    n = C.c_int(0)
    buf = (L.ScaleInfo * 4096)()
    L.check(L.lib().cc_scale_plan(win_w, win_h, width, height, C.byref(p), buf, 4096, C.byref(n)))
    dt = np.dtype([("scale", "<f4"), ("w", "<i4"), ("h", "<i4"), ("ystep", "<i4"), ("nx", "<i4"), ("ny", "<i4"),
                   ("win_w", "<i4"), ("win_h", "<i4")])
    return np.frombuffer(bytes(buf), dt, n.value).copy()


def _all_or_none(what, *args):
    """True when every one of `args` is given, False when none is; anything in between is a ValueError."""
    given = [a is not None for a in args]
    if any(given) and not all(given):
        raise ValueError(f"{what} go together: give all of them or none")
    return all(given)


def group_rectangles(rects, group_threshold, eps=0.2, levels=None, weights=None):
    """cv::groupRectangles on the host. With levels (n,) int32 and weights (n,) float64 -- both or neither -- the
    rejectLevels / levelWeights form (cc_group_rectangles_levels), which returns (rects, levels, weights)."""
    rects = np.ascontiguousarray(rects, np.int32).reshape(-1, 4)
    out = np.zeros((max(len(rects), 1), 4), np.int32)
    n = C.c_int(0)
    if not _all_or_none("levels and weights", levels, weights):
        L.check(L.lib().cc_group_rectangles(_vp(rects), len(rects), int(group_threshold), float(eps), _vp(out), len(out), C.byref(n)))
        return out[:n.value].copy()
    levels = np.ascontiguousarray(levels, np.int32).reshape(-1)
    weights = np.ascontiguousarray(weights, np.float64).reshape(-1)
    if len(levels) != len(rects) or len(weights) != len(rects):
        raise ValueError("levels and weights need one entry per rectangle")
    out_l, out_w = np.zeros(len(out), np.int32), np.zeros(len(out), np.float64)
    L.check(L.lib().cc_group_rectangles_levels(_vp(rects), _vp(levels), _vp(weights), len(rects), int(group_threshold), float(eps),
                                               _vp(out), _vp(out_l), _vp(out_w), len(out), C.byref(n)))
    return out[:n.value].copy(), out_l[:n.value].copy(), out_w[:n.value].copy()


def _raise_with_count(status, needed):
    """CascadeError of a failed call; CC_ERR_BUFFER_TOO_SMALL carries the count the buffer must hold as .needed."""
    err = L.CascadeError(status, L.lib().cc_last_error().decode("utf-8", "replace"))
    if status == L.CC_ERR_BUFFER_TOO_SMALL:
        err.needed = int(needed)
    raise err


def group_rectangles_device(rects_ptr, offsets_ptr, n_frames, group_threshold, out_ptr, cap, out_offsets_ptr, eps=0.2,
                            device=0, levels_ptr=None, weights_ptr=None, out_levels_ptr=None, out_weights_ptr=None) -> int:
    """cv::groupRectangles on every frame of a batch, in device memory (cc_group_rectangles_device). All pointers are plain
    integers (e.g. tensor.data_ptr()) into memory of `device`: rects int32 (n, 4), offsets int32 (n_frames + 1), out int32
    (cap, 4), out_offsets int32 (n_frames + 1). Returns the number of rectangles over all frames; raises CascadeError with
    CC_ERR_BUFFER_TOO_SMALL (.needed = that number) when it exceeds cap -- out_offsets are complete then, out holds the
    first cap. levels_ptr -> int32 (n), weights_ptr -> float64 (n), out_levels_ptr -> int32 (cap), out_weights_ptr -> float64
    (cap), all four or none: the grouping with levels and weights (cc_group_rectangles_device_levels)."""
    n = C.c_int(0)
    if _all_or_none("levels_ptr, weights_ptr, out_levels_ptr and out_weights_ptr", levels_ptr, weights_ptr, out_levels_ptr, out_weights_ptr):
        st = L.lib().cc_group_rectangles_device_levels(int(device), C.c_void_p(rects_ptr or 0), C.c_void_p(levels_ptr or 0),
                                                       C.c_void_p(weights_ptr or 0), C.c_void_p(offsets_ptr or 0), int(n_frames),
                                                       int(group_threshold), float(eps), C.c_void_p(out_ptr or 0),
                                                       C.c_void_p(out_levels_ptr or 0), C.c_void_p(out_weights_ptr or 0), int(cap),
                                                       C.c_void_p(out_offsets_ptr or 0), C.byref(n))
        if st != L.CC_OK:
            _raise_with_count(st, n.value)
        return n.value
    st = L.lib().cc_group_rectangles_device(int(device), C.c_void_p(rects_ptr or 0), C.c_void_p(offsets_ptr or 0), int(n_frames),
                                            int(group_threshold), float(eps), C.c_void_p(out_ptr or 0), int(cap),
                                            C.c_void_p(out_offsets_ptr or 0), C.byref(n))
    if st != L.CC_OK:
        _raise_with_count(st, n.value)
    return n.value


# pixel_format keywords -> CC_PIX_* (include/cascadeclassifier_amd.h). 3- and 4-channel arrays default to cv2's BGR / BGRA.
PIXEL_FORMATS = {"gray": L.CC_PIX_GRAY8, "bgr": L.CC_PIX_BGR8, "bgra": L.CC_PIX_BGRA8, "rgb": L.CC_PIX_RGB8,
                 "rgba": L.CC_PIX_RGBA8, "rgb_planar": L.CC_PIX_RGB8_PLANAR}
_CHANNELS = {L.CC_PIX_GRAY8: 1, L.CC_PIX_BGR8: 3, L.CC_PIX_BGRA8: 4, L.CC_PIX_RGB8: 3, L.CC_PIX_RGBA8: 4,
             L.CC_PIX_RGB8_PLANAR: 3}


def frame_layout(shape, pixel_format=None, batched=False):
    """Shape of one image or of a batch of frames -> (n, height, width, CC_PIX_* code, row_stride, frame_stride), the
    strides in bytes of a dense uint8 array of that shape. One image: (H, W) gray, (H, W, 3) / (H, W, 4) colour, or
    (3, H, W) with pixel_format="rgb_planar". A batch: the same with a leading n. pixel_format (None = what the shape
    says: gray, "bgr" or "bgra") must agree with the shape; anything else raises CascadeError(CC_ERR_INVALID_ARG)."""
    def bad(why):
        return L.CascadeError(L.CC_ERR_INVALID_ARG, f"frame shape {tuple(shape)}, pixel_format {pixel_format!r}: {why}")

    shape = tuple(int(v) for v in shape)
    if pixel_format is not None and pixel_format not in PIXEL_FORMATS:
        raise bad(f"unknown pixel format (one of {sorted(PIXEL_FORMATS)})")
    if batched and len(shape) < 1:
        raise bad("no frame count")
    dims = shape[1:] if batched else shape
    n = shape[0] if batched else 1
    if len(dims) == 2:
        fmt = PIXEL_FORMATS[pixel_format or "gray"]
        if fmt != L.CC_PIX_GRAY8:
            raise bad("a 2-d frame is gray")
        h, w = dims
        rs = w
    elif len(dims) == 3 and pixel_format == "rgb_planar":
        c, h, w = dims
        if c != 3:
            raise bad("planar frames are (3, H, W)")
        fmt, rs = L.CC_PIX_RGB8_PLANAR, w
    elif len(dims) == 3:
        h, w, c = dims
        if c not in (3, 4):
            raise bad("colour frames have 3 or 4 channels")
        fmt = PIXEL_FORMATS[pixel_format or ("bgr" if c == 3 else "bgra")]
        if _CHANNELS[fmt] != c or fmt == L.CC_PIX_RGB8_PLANAR:
            raise bad(f"{c} channels do not match the pixel format")
        rs = w * c
    else:
        raise bad("expected (H, W), (H, W, C) or (3, H, W) per frame")
    if n < 0 or h < 1 or w < 1:
        raise bad("empty frame")
    rows = 3 * h if fmt == L.CC_PIX_RGB8_PLANAR else h
    return n, h, w, fmt, rs, rs * rows


def to_gray(img, pixel_format=None, device=0):
    """Colour -> gray on the device with the detector's conversion (cc_to_gray_u8): one image as detectMultiScale takes it."""
    img = np.ascontiguousarray(img, np.uint8)
    _, h, w, fmt, rs, _ = frame_layout(img.shape, pixel_format)
    dst = np.empty((h, w), np.uint8)
    L.check(L.lib().cc_to_gray_u8(device, _vp(img), fmt, w, h, rs, _vp(dst), w))
    return dst


def integral(img, device=0, sqsum=False, tilted=False):
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    out = {"sum": np.empty((h + 1, w + 1), np.int32)}
    if sqsum:
        out["sqsum"] = np.empty((h + 1, w + 1), np.int32)
    if tilted:
        out["tilted"] = np.empty((h + 1, w + 1), np.int32)
    L.check(L.lib().cc_integral_u8(device, _vp(img), w, h, w, _vp(out["sum"]), _vp(out.get("sqsum")), _vp(out.get("tilted"))))
    return out


def resize_linear_exact(img, dw, dh, device=0):
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    dst = np.empty((dh, dw), np.uint8)
    L.check(L.lib().cc_resize_linear_exact_u8(device, _vp(img), w, h, w, _vp(dst), dw, dh, dw))
    return dst


def resize_area(img, dw, dh, device=0):
    """cv::resize INTER_AREA of a gray (h, w) uint8 image to dw x dh (cc_resize_area_u8: neither side may grow). Rows may be
    strided (a view of a wider array): the stride is passed on as it is."""
    img = np.asarray(img)
    if img.ndim != 2 or img.dtype != np.uint8 or (img.shape[1] > 1 and img.strides[1] != 1) or img.strides[0] < img.shape[1]:
        img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    dst = np.empty((max(dh, 0), max(dw, 0)), np.uint8)
    L.check(L.lib().cc_resize_area_u8(device, _vp(img), w, h, img.strides[0], _vp(dst), dw, dh))
    return dst


class CascadeClassifier:
    """cv2.CascadeClassifier-shaped front end. load()/empty()/detectMultiScale() as the reference's tools call them."""

    def __init__(self, filename: str | None = None, device: int = 0, max_batch: int = 1):
        self._c = C.c_void_p()
        self._d = C.c_void_p()
        self.device = device
        self.max_batch = max_batch
        if filename is not None and not self.load(filename):
            pass  # like cv2: constructor does not throw; empty() reports it

    # -- model ----------------------------------------------------------------------------------
    def load(self, filename: str) -> bool:
        self._release()
        st = L.lib().cc_cascade_load_xml(filename.encode(), C.byref(self._c))
        if st != L.CC_OK:
            self.load_error = L.lib().cc_last_error().decode()
            self._c = C.c_void_p()
            return False
        return True

    def load_from_string(self, text: str | bytes) -> bool:
        self._release()
        b = text.encode() if isinstance(text, str) else text
        st = L.lib().cc_cascade_load_xml_mem(b, len(b), C.byref(self._c))
        if st != L.CC_OK:
            self.load_error = L.lib().cc_last_error().decode()
            self._c = C.c_void_p()
            return False
        return True

    @classmethod
    def from_stumps(cls, feature_type, win, stages, haar_mode=L.CC_HAAR_BASIC, device: int = 0, max_batch: int = 1):
        """The cascade CvCascadeClassifier::save would write for trained stumps: `stages` is a list of
        (stage_threshold, [weak dicts]) with the dicts CascadeBoost.train_stage returns (var_idx, ord_c or subset,
        left_value, right_value; records with trained == False are skipped) and the threshold of the stage's last record.
        Leaves and thresholds are cast to float here, as the writer does; the used variables are renumbered in catalog
        order."""
        weaks = [[w for w in ws if w.get("trained", True)] for _, ws in stages]
        n_weak = np.array([len(ws) for ws in weaks], np.int32)
        flat = [w for ws in weaks for w in ws]
        thr = np.array([np.float32(t) for t, _ in stages], np.float32)
        var = np.array([w["var_idx"] for w in flat], np.int32)
        lbp = feature_type == L.CC_FEATURE_LBP
        ord_c = None if lbp else np.array([np.float32(w["ord_c"]) for w in flat], np.float32)
        subsets = np.array([np.asarray(w["subset"], np.int64).astype(np.int32) for w in flat], np.int32).reshape(-1) if lbp else None
        left = np.array([np.float32(w["left_value"]) for w in flat], np.float32)
        right = np.array([np.float32(w["right_value"]) for w in flat], np.float32)
        self = cls(None, device, max_batch)
        L.check(L.lib().cc_cascade_from_stumps(int(feature_type), int(haar_mode), int(win[0]), int(win[1]), len(n_weak), _vp(n_weak),
                                               len(var), _vp(thr), _vp(var), _vp(ord_c), _vp(subsets), _vp(left), _vp(right), C.byref(self._c)))
        return self

    @classmethod
    def from_trees(cls, feature_type, win, stages, haar_mode=L.CC_HAAR_BASIC, device: int = 0, max_batch: int = 1):
        """from_stumps for weak trees of any depth (CvCascadeBoostTree::write): `stages` as from_stumps takes them, every
        trained record with "nodes" and "leaves" as CascadeBoost(max_depth > 1) returns them; a record without them is
        the stump of its own fields."""
        weaks = [[w for w in ws if w.get("trained", True)] for _, ws in stages]
        n_weak = np.array([len(ws) for ws in weaks], np.int32)
        thr = np.array([np.float32(t) for t, _ in stages], np.float32)
        n_nodes, flat, leaves = L.pack_trees([w for ws in weaks for w in ws])
        self = cls(None, device, max_batch)
        L.check(L.lib().cc_cascade_from_trees(int(feature_type), int(haar_mode), int(win[0]), int(win[1]), len(n_weak), _vp(n_weak), len(n_nodes),
                                              _vp(thr), _vp(n_nodes), int(n_nodes.sum()), flat, _vp(leaves), C.byref(self._c)))
        return self

    def empty(self) -> bool:
        return not self._c

    def save(self, filename: str, baseFormat: bool = False, params=None):
        """Write the model back as a cascade.xml: the new-format layout of CvCascadeClassifier::save, or with
        baseFormat=True its legacy "opencv-haar-classifier" layout (cascadeclassifier.cpp:439-531; Haar only). params (a
        traincascade.TrainParams or a dict of its fields, as train_params() returns it): the new-format file carries the
        whole <stageParams> / <featureParams> block of writeParams (cc_cascade_save_xml_params); the legacy layout has no
        place for it."""
        if baseFormat or params is None:
            fn = L.lib().cc_cascade_save_xml_legacy if baseFormat else L.lib().cc_cascade_save_xml
            L.check(fn(self._c, filename.encode()))
            return
        fields = params if isinstance(params, dict) else params.as_dict()
        p = L.TrainParams(**{n: fields[n] for n, _ in L.TrainParams._fields_})
        L.check(L.lib().cc_cascade_save_xml_params(self._c, C.byref(p), filename.encode()))

    def train_params(self):
        """The training parameters the loaded cascade.xml carried, as a dict of cc_train_params' fields, or None when the
        file had none (cc_cascade_train_params)."""
        p = L.TrainParams()
        st = L.lib().cc_cascade_train_params(self._c, C.byref(p))
        if st == L.CC_ERR_NO_TRAIN_PARAMS:
            return None
        L.check(st)
        return {n: getattr(p, n) for n, _ in p._fields_}

    def info(self) -> dict:
        ci = L.CascadeInfo()
        L.check(L.lib().cc_cascade_info_get(self._c, C.byref(ci)))
        return {n: getattr(ci, n) for n, _ in ci._fields_}

    def model(self) -> CascadeModel:
        inf = self.info()
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        L.check(L.lib().cc_cascade_stages(self._c, C.byref(a), C.byref(b), C.byref(c)))
        ns, nw, nf = inf["n_stages"], inf["n_weak"], inf["n_features"]
        sf, sn, sthr = _view(a, C.c_int32, ns), _view(b, C.c_int32, ns), _view(c, C.c_float, ns)
        stump = [None] * 5
        if inf["max_nodes_per_tree"] == 1:
            p = [C.c_void_p() for _ in range(5)]
            L.check(L.lib().cc_cascade_stumps(self._c, *[C.byref(x) for x in p]))
            stump = [_view(p[0], C.c_int32, nw), _view(p[1], C.c_float, nw), _view(p[2], C.c_float, nw),
                     _view(p[3], C.c_float, nw),
                     _view(p[4], C.c_int32, nw * inf["subset_size"]).reshape(nw, -1) if inf["subset_size"] else None]
        r, w, t = C.c_void_p(), C.c_void_p(), C.c_void_p()
        L.check(L.lib().cc_cascade_features(self._c, C.byref(r), C.byref(w), C.byref(t)))
        if inf["feature_type"] == L.CC_FEATURE_HAAR:
            rects = _view(r, C.c_int32, nf * 12).reshape(nf, 3, 4)
            weights = _view(w, C.c_float, nf * 3).reshape(nf, 3)
            tilted = _view(t, C.c_int32, nf)
        elif inf["feature_type"] == L.CC_FEATURE_HOG:  # cell 0 of the block (x y w h) and the component in [0, 36)
            rects, weights, tilted = _view(r, C.c_int32, nf * 5).reshape(nf, 5), None, None
        else:
            rects, weights, tilted = _view(r, C.c_int32, nf * 4).reshape(nf, 4), None, None
        return CascadeModel(inf, sf, sn, sthr, *stump, rects, weights, tilted)

    def wave_int_tables(self):
        """(q, thr_q, left_q, right_q) of cc_debug_wave_int_tables: per stage the quantum of the wave phase's integer vote
        sums (0 = that stage sums in double) and the integer stage threshold, per stump the leaves in quanta. Host only."""
        inf = self.info()
        q, thr_q = np.zeros(inf["n_stages"], np.float64), np.zeros(inf["n_stages"], np.int32)
        left_q, right_q = np.zeros(inf["n_weak"], np.int32), np.zeros(inf["n_weak"], np.int32)
        L.check(L.lib().cc_debug_wave_int_tables(self._c, _vp(q), _vp(thr_q), _vp(left_q), _vp(right_q)))
        return q, thr_q, left_q, right_q

    # -- detector -------------------------------------------------------------------------------
    def _detector(self):
        if not self._c:
            raise L.CascadeError(L.CC_ERR_INVALID_ARG, "CascadeClassifier is empty")
        if not self._d:
            L.check(L.lib().cc_detector_create(self._c, self.device, self.max_batch, C.byref(self._d)))
        return self._d

    def set_stream(self, hip_stream: int | None):
        L.check(L.lib().cc_detector_set_stream(self._detector(), C.c_void_p(hip_stream or 0)))

    def detectMultiScale(self, image, scaleFactor=1.1, minNeighbors=3, flags=0, minSize=None, maxSize=None,
                         pixel_format=None) -> np.ndarray:
        """image: HxW uint8 (gray), or HxWx3 / HxWx4 colour -- BGR / BGRA as cv2 takes them, pixel_format="rgb" / "rgba"
        for the other order, or 3xHxW with pixel_format="rgb_planar" -- converted to gray on the device.
        Returns an (n, 4) int32 array of (x, y, w, h) like cv2 does."""
        image = np.ascontiguousarray(image, np.uint8)
        _, h, w, fmt, rs, _ = frame_layout(image.shape, pixel_format)
        p = _params(scaleFactor, minNeighbors, minSize, maxSize)
        cap = 1024
        while True:
            out = np.zeros((cap, 4), np.int32)
            n = C.c_int(0)
            st = L.lib().cc_detect_multiscale_fmt(self._detector(), _vp(image), w, h, rs, fmt, C.byref(p), _vp(out), cap,
                                                  C.byref(n))
            if st == L.CC_ERR_BUFFER_TOO_SMALL:
                cap = n.value
                continue
            L.check(st)
            return out[:n.value].copy()

    @staticmethod
    def _batch_frames(frames, device_ptr, shape, row_stride, frame_stride, pixel_format):
        """-> (keep-alive array or None, pointer, on_device, n, h, w, format, row_stride, frame_stride)"""
        if device_ptr is None:
            frames = np.ascontiguousarray(frames, np.uint8)
            n, h, w, fmt, rs, fs = frame_layout(frames.shape, pixel_format, batched=True)
            return frames, _vp(frames), 0, n, h, w, fmt, rs, fs
        n, h, w, fmt, rs, fs = frame_layout(shape, pixel_format, batched=True)
        rs = row_stride or rs
        fs = frame_stride or rs * (3 * h if fmt == L.CC_PIX_RGB8_PLANAR else h)
        return None, C.c_void_p(device_ptr), 1, n, h, w, fmt, rs, fs

    def detect_batch(self, frames, scaleFactor=1.1, minNeighbors=3, minSize=None, maxSize=None, device_ptr=None,
                     shape=None, row_stride=None, frame_stride=None, pixel_format=None):
        """frames: (n, H, W) uint8 numpy array in host memory -- or (n, H, W, C) colour, BGR / BGRA unless pixel_format
        says "rgb" / "rgba" -- or device_ptr + shape=(n, H, W[, C]) for frames already in HBM (shape=(n, 3, H, W) with
        pixel_format="rgb_planar"); row_stride / frame_stride in bytes. Returns a list of (k_i, 4) arrays."""
        p = _params(scaleFactor, minNeighbors, minSize, maxSize)
        frames, ptr, on_dev, n, h, w, fmt, rs, fs = self._batch_frames(frames, device_ptr, shape, row_stride, frame_stride,
                                                                         pixel_format)
        cap = max(256 * n, 1024)
        while True:
            out = np.zeros((cap, 4), np.int32)
            offs = np.zeros(n + 1, np.int32)
            st = L.lib().cc_detect_batch_fmt(self._detector(), ptr, on_dev, n, w, h, rs, fs, fmt, C.byref(p), _vp(out), cap,
                                             _vp(offs))
            if st == L.CC_ERR_BUFFER_TOO_SMALL:
                cap = int(offs[n])
                continue
            L.check(st)
            return [out[offs[i]:offs[i + 1]].copy() for i in range(n)]

    def detect_batch3(self, frames, scaleFactor=1.1, minNeighbors=3, minSize=None, maxSize=None, device_ptr=None,
                      shape=None, row_stride=None, frame_stride=None, pixel_format=None):
        """detect_batch with scores, as detectMultiScale3 is detectMultiScale with scores (cc_detect_batch_levels_fmt): a list
        of (rects (k_i, 4) int32, rejectLevels (k_i,) int32, levelWeights (k_i,) float64), one per frame. Frames as
        detect_batch takes them."""
        p = _params(scaleFactor, minNeighbors, minSize, maxSize)
        frames, ptr, on_dev, n, h, w, fmt, rs, fs = self._batch_frames(frames, device_ptr, shape, row_stride, frame_stride,
                                                                         pixel_format)
        cap = max(256 * n, 1024)
        while True:
            out = np.zeros((cap, 4), np.int32)
            levels = np.zeros(cap, np.int32)
            weights = np.zeros(cap, np.float64)
            offs = np.zeros(n + 1, np.int32)
            st = L.lib().cc_detect_batch_levels_fmt(self._detector(), ptr, on_dev, n, w, h, rs, fs, fmt, C.byref(p), _vp(out),
                                                    _vp(levels), _vp(weights), cap, _vp(offs))
            if st == L.CC_ERR_BUFFER_TOO_SMALL:
                cap = int(offs[n])
                continue
            L.check(st)
            return [(out[offs[i]:offs[i + 1]].copy(), levels[offs[i]:offs[i + 1]].copy(), weights[offs[i]:offs[i + 1]].copy())
                    for i in range(n)]

    def detect_batch_to_device(self, frames, scaleFactor=1.1, minNeighbors=3, minSize=None, maxSize=None, *, out_ptr, cap,
                               offsets_ptr, device_ptr=None, shape=None, row_stride=None, frame_stride=None,
                               pixel_format=None, levels_ptr=None, weights_ptr=None) -> int:
        """detect_batch whose result stays on the device (cc_detect_batch_to_device): out_ptr -> int32 (cap, 4) and
        offsets_ptr -> int32 (n + 1) in memory of the detector's device, as plain integers (tensor.data_ptr()); frame i's
        rectangles are out[offsets[i]:offsets[i + 1]], the same and in the same order as detect_batch returns. Frames as
        detect_batch takes them. Returns the number of rectangles over all frames; raises CascadeError with
        CC_ERR_BUFFER_TOO_SMALL (.needed = that number) when it exceeds cap -- the offsets are complete then, out holds
        the first cap. levels_ptr -> int32 (cap) and weights_ptr -> float64 (cap), both or neither: the scores of
        detect_batch3 beside the rectangles (cc_detect_batch_to_device_levels)."""
        scored = _all_or_none("levels_ptr and weights_ptr", levels_ptr, weights_ptr)
        p = _params(scaleFactor, minNeighbors, minSize, maxSize)
        keep, ptr, on_dev, n, h, w, fmt, rs, fs = self._batch_frames(frames, device_ptr, shape, row_stride, frame_stride,
                                                                       pixel_format)
        total = C.c_int(0)
        if scored:
            st = L.lib().cc_detect_batch_to_device_levels(self._detector(), ptr, on_dev, n, w, h, rs, fs, fmt, C.byref(p),
                                                          C.c_void_p(out_ptr or 0), C.c_void_p(levels_ptr or 0),
                                                          C.c_void_p(weights_ptr or 0), int(cap), C.c_void_p(offsets_ptr or 0),
                                                          C.byref(total))
        else:
            st = L.lib().cc_detect_batch_to_device(self._detector(), ptr, on_dev, n, w, h, rs, fs, fmt, C.byref(p),
                                                   C.c_void_p(out_ptr or 0), int(cap), C.c_void_p(offsets_ptr or 0), C.byref(total))
        del keep  # host frames were staged inside the call
        if st != L.CC_OK:
            _raise_with_count(st, total.value)
        return total.value

    def detect_batch_submit(self, frames, scaleFactor=1.1, minNeighbors=3, minSize=None, maxSize=None, device_ptr=None,
                            shape=None, row_stride=None, frame_stride=None, pixel_format=None):
        """First half of detect_batch (cc_detect_batch_submit): launches the batch and returns a ticket while its last pass
        still runs. Submit the next batch before collecting this one to overlap them. The frames must stay alive until
        detect_batch_collect(ticket). Frames, shapes and pixel formats as detect_batch takes them."""
        p = _params(scaleFactor, minNeighbors, minSize, maxSize)
        keep, ptr, on_dev, n, h, w, fmt, rs, fs = self._batch_frames(frames, device_ptr, shape, row_stride, frame_stride,
                                                                       pixel_format)
        t = C.c_void_p()
        L.check(L.lib().cc_detect_batch_submit_fmt(self._detector(), ptr, on_dev, n, w, h, rs, fs, fmt, C.byref(p),
                                                   C.byref(t)))
        return {"ticket": t, "n": n, "frames": keep}

    def detect_batch_collect(self, ticket):
        """Second half: waits for the batch and returns what detect_batch returns (a list of (k_i, 4) arrays)."""
        n = ticket["n"]
        cap = max(256 * n, 1024)
        while True:
            out = np.zeros((cap, 4), np.int32)
            offs = np.zeros(n + 1, np.int32)
            st = L.lib().cc_detect_batch_collect(self._detector(), ticket["ticket"], _vp(out), cap, _vp(offs))
            if st == L.CC_ERR_BUFFER_TOO_SMALL:  # the ticket is still valid
                cap = int(offs[n])
                continue
            ticket["ticket"] = None
            ticket["frames"] = None
            L.check(st)
            return [out[offs[i]:offs[i + 1]].copy() for i in range(n)]

    def detect_batch_discard(self, ticket):
        """Ends a submitted batch whose results are not wanted (cc_detect_batch_discard)."""
        t, ticket["ticket"], ticket["frames"] = ticket["ticket"], None, None
        if t is not None:
            L.check(L.lib().cc_detect_batch_discard(self._detector(), t))

    def run_device_only(self, device_ptr, shape, scaleFactor=1.1, minSize=None, maxSize=None, row_stride=None,
                        frame_stride=None):
        n, h, w = shape
        p = _params(scaleFactor, 3, minSize, maxSize)
        rs = row_stride or w
        fs = frame_stride or rs * h
        L.check(L.lib().cc_detect_batch_device_only(self._detector(), C.c_void_p(device_ptr), 1, n, w, h, rs, fs, C.byref(p)))

    def detectMultiScale3(self, image, scaleFactor=1.1, minNeighbors=3, flags=0, minSize=None, maxSize=None, outputRejectLevels=True,
                          pixel_format=None):
        """cv2.CascadeClassifier.detectMultiScale3: (rects (n, 4) int32, rejectLevels (n,) int32, levelWeights (n,) float64).
        Images as detectMultiScale takes them."""
        if not outputRejectLevels:
            r = self.detectMultiScale(image, scaleFactor, minNeighbors, flags, minSize, maxSize, pixel_format=pixel_format)
            return r, np.zeros(0, np.int32), np.zeros(0, np.float64)
        image = np.ascontiguousarray(image, np.uint8)
        _, h, w, fmt, rs, _ = frame_layout(image.shape, pixel_format)
        p = _params(scaleFactor, minNeighbors, minSize, maxSize)
        cap = 1024
        while True:
            rects = np.zeros((cap, 4), np.int32)
            levels = np.zeros(cap, np.int32)
            weights = np.zeros(cap, np.float64)
            n = C.c_int(0)
            st = L.lib().cc_detect_multiscale_levels_fmt(self._detector(), _vp(image), w, h, rs, fmt, C.byref(p), _vp(rects),
                                                         _vp(levels), _vp(weights), cap, C.byref(n))
            if st == L.CC_ERR_BUFFER_TOO_SMALL:
                cap = n.value
                continue
            L.check(st)
            return rects[:n.value].copy(), levels[:n.value].copy(), weights[:n.value].copy()

    def detect_raw(self, image, scaleFactor=1.1, minSize=None, maxSize=None) -> np.ndarray:
        image = np.ascontiguousarray(image, np.uint8)
        h, w = image.shape
        p = _params(scaleFactor, 0, minSize, maxSize)
        cap = 4096
        while True:
            out = np.zeros((cap, 7), np.int32)
            n = C.c_int(0)
            st = L.lib().cc_detect_raw(self._detector(), _vp(image), w, h, w, C.byref(p), _vp(out), cap, C.byref(n))
            if st == L.CC_ERR_BUFFER_TOO_SMALL:
                cap = n.value
                continue
            L.check(st)
            return out[:n.value].copy()

    def debug_windows(self, image, scaleFactor=1.1, minSize=None, maxSize=None):
        image = np.ascontiguousarray(image, np.uint8)
        h, w = image.shape
        p = _params(scaleFactor, 0, minSize, maxSize)
        inf = self.info()
        sc = scale_plan(inf["win_w"], inf["win_h"], w, h, scaleFactor, minSize, maxSize)
        tot = int((sc["nx"].astype(np.int64) * sc["ny"]).sum())
        codes = np.zeros(max(tot, 1), np.int32)
        sums = np.zeros(max(tot, 1), np.float64)
        vis = np.zeros(max(tot, 1), np.uint8)
        n = C.c_int64(0)
        L.check(L.lib().cc_detect_debug_windows(self._detector(), _vp(image), w, h, w, C.byref(p), _vp(codes), _vp(sums),
                                                _vp(vis), tot, C.byref(n)))
        assert n.value == tot
        return codes[:tot], sums[:tot], vis[:tot]

    def specialize(self, n_stages: int = 4) -> int:
        """Compile the first n_stages stages of this cascade into the cascade kernel (hiprtc, a few seconds; Haar stump
        cascades). Results are unchanged; returns the number of stages in effect. n_stages <= 0 switches back."""
        L.check(L.lib().cc_detector_specialize(self._detector(), int(n_stages)))
        return self.specialized_stages()

    def specialize_async(self, n_stages: int = 4):
        """Start the same build on a background thread; detection keeps using the table-driven kernel until a later call
        finds the module ready (specialized_stages() then becomes non-zero)."""
        L.check(L.lib().cc_detector_specialize_async(self._detector(), int(n_stages)))

    def specialized_stages(self) -> int:
        return L.lib().cc_detector_specialized_stages(self._detector())

    def graph_active(self) -> bool:
        """True if the last single-image detectMultiScale call was one hipGraph launch (cc_detector_graph_active)."""
        return L.lib().cc_detector_graph_active(self._detector()) == 1

    def graph_captures(self) -> int:
        """hipGraph captures this detector has made (cc_detector_graph_captures); replays do not count."""
        return int(L.lib().cc_detector_graph_captures(self._detector()))

    def set_profiling(self, on: bool):
        L.check(L.lib().cc_detector_set_profiling(self._detector(), 1 if on else 0))

    def timings(self, reset=False) -> dict:
        t = L.DetectorTimings()
        L.check(L.lib().cc_detector_get_timings(self._detector(), C.byref(t), 1 if reset else 0))
        return {n: getattr(t, n) for n, _ in t._fields_}

    def candidate_capacity(self) -> int:
        """Entries of the per-pass candidate lists: 0 before a first pass has sized them, larger after an overflowing pass
        was redone (cc_detector_candidate_capacity)."""
        return int(L.lib().cc_detector_candidate_capacity(self._detector()))

    # -- lifetime -------------------------------------------------------------------------------
    def _release(self):
        if getattr(self, "_d", None):
            L.lib().cc_detector_destroy(self._d)
            self._d = C.c_void_p()
        if getattr(self, "_c", None):
            L.lib().cc_cascade_destroy(self._c)
            self._c = C.c_void_p()

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass


def vec_read(path: str, max_samples: int | None = None) -> np.ndarray:
    """Samples of a .vec file as (n, width*height) uint8 (PosReader semantics, imagestorage.cpp:138-182)."""
    cnt, vs = C.c_int32(0), C.c_int32(0)
    L.check(L.lib().cc_vec_read(path.encode(), C.byref(cnt), C.byref(vs), None, 0))
    n = cnt.value if max_samples is None else min(cnt.value, max_samples)
    out = np.zeros((max(n, 1), vs.value), np.uint8)
    L.check(L.lib().cc_vec_read(path.encode(), C.byref(cnt), C.byref(vs), _vp(out), n))
    return out[:n]


def vec_write(path: str, samples: np.ndarray, width: int, height: int):
    samples = np.ascontiguousarray(samples, np.uint8).reshape(-1, width * height)
    L.check(L.lib().cc_vec_write(path.encode(), _vp(samples), len(samples), width, height))
