"""Python host mirror of the training-side plugin surface CvFeatureEvaluator / CvHaarEvaluator / CvLBPEvaluator
(traincascade/lib/include/traincascade_features.h:155-188) on top of the C ABI: same method names, argument meaning
and error behaviour (CV_Assert failures surface as CascadeError instead of cv::Exception)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

HAAR, LBP, HOG = L.CC_FEATURE_HAAR, L.CC_FEATURE_LBP, L.CC_FEATURE_HOG
BASIC, CORE, ALL = L.CC_HAAR_BASIC, L.CC_HAAR_CORE, L.CC_HAAR_ALL


BOOST_DISCRETE, BOOST_REAL, BOOST_LOGIT, BOOST_GENTLE = 0, 1, 2, 3  # CvBoost types (boost.h)
SPLIT_DEFAULT, SPLIT_GINI, SPLIT_MISCLASS, SPLIT_SQERR = 0, 1, 3, 4


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def presort_plan(feature_type, n_vars, n_samples, budget_bytes):
    """cc_presort_plan (host arithmetic; no device unless budget_bytes is 0 = the device's free memory): how a presort of
    n_vars variables over n_samples fits budget_bytes of device memory. Returns (resident_vars, chunk_vars, bytes_needed);
    chunk_vars is 0 when every table fits. Raises CascadeError (CC_ERR_UNSUPPORTED) for a budget below one chunk of 64
    variables, naming the smallest budget that works, and for LBP tables that do not fit."""
    r, c, b = C.c_int(0), C.c_int(0), C.c_uint64(0)
    L.check(L.lib().cc_presort_plan(int(feature_type), int(n_vars), int(n_samples), int(budget_bytes), C.byref(r), C.byref(c), C.byref(b)))
    return r.value, c.value, b.value


class CvFeatureParams:
    """CvFeatureParams / CvHaarFeatureParams / CvLBPFeatureParams / CvHOGFeatureParams (haarfeatures.h:31-51,
    lbpfeatures.h:22-26, HOGfeatures.cpp:9-14)."""

    def __init__(self, feature_type=HAAR, mode=BASIC):
        self.feature_type = feature_type
        self.mode = mode
        self.maxCatCount = 256 if feature_type == LBP else 0
        self.featSize = 36 if feature_type == HOG else 1  # HOG: N_BINS * N_CELLS variables per feature

    @staticmethod
    def create(feature_type):
        return CvFeatureParams(feature_type) if feature_type in (HAAR, LBP, HOG) else None


class CvFeatureEvaluator:
    def __init__(self, feature_type, device=0):
        self.feature_type = feature_type
        self.device = device
        self._e = C.c_void_p()
        self.winSize = None

    @staticmethod
    def create(feature_type, device=0):
        """features.cpp:91-97: unknown type -> empty Ptr (None here). For HOG every feature index of the value methods
        (__call__, calc_list, calc_batch*, presort, find_best_split's var_idx) is a variable index in
        [0, getNumFeatures() * getFeatureSize())."""
        return CvFeatureEvaluator(feature_type, device) if feature_type in (HAAR, LBP, HOG) else None

    def init(self, featureParams: CvFeatureParams, maxSampleCount: int, winSize):
        self._release()
        w, h = winSize
        L.check(L.lib().cc_eval_create(self.feature_type, featureParams.mode, int(w), int(h), int(maxSampleCount), self.device,
                                       C.byref(self._e)))
        self.winSize = (int(w), int(h))
        self.featureParams = featureParams
        self.maxSampleCount = int(maxSampleCount)

    def setImage(self, img, clsLabel: int, idx: int):
        img = np.ascontiguousarray(img, np.uint8)
        if img.shape != (self.winSize[1], self.winSize[0]):  # features.cpp:85-86
            raise L.CascadeError(L.CC_ERR_INVALID_ARG, f"setImage: image {img.shape[::-1]} != winSize {self.winSize}")
        L.check(L.lib().cc_eval_set_image(self._e, _vp(img), img.shape[1], int(clsLabel), int(idx)))

    def setImages(self, imgs, labels=None, first_idx=0):
        imgs = np.ascontiguousarray(imgs, np.uint8)
        if imgs.ndim != 3 or imgs.shape[1:] != (self.winSize[1], self.winSize[0]):
            raise L.CascadeError(L.CC_ERR_INVALID_ARG, "setImages: images do not match winSize")
        lab = None if labels is None else np.ascontiguousarray(labels, np.uint8)
        L.check(L.lib().cc_eval_set_images(self._e, _vp(imgs), imgs.shape[0], int(first_idx), _vp(lab)))

    def __call__(self, featureIdx: int, sampleIdx: int) -> float:
        out = C.c_float(0)
        L.check(L.lib().cc_eval_calc(self._e, int(featureIdx), int(sampleIdx), C.byref(out)))
        return out.value

    def calc_list(self, feature_idx, sample_idx: int) -> np.ndarray:
        """operator()(fi, sample_idx) for an arbitrary list of features and one stored sample, one launch (cc_eval_calc_list)."""
        fi = np.ascontiguousarray(feature_idx, np.int32)
        out = np.empty(len(fi), np.float32)
        L.check(L.lib().cc_eval_calc_list(self._e, _vp(fi), len(fi), int(sample_idx), _vp(out)))
        return out

    def calc_batch(self, fi_begin, fi_end, sample_idx=None, n_samples=None) -> np.ndarray:
        idx = None if sample_idx is None else np.ascontiguousarray(sample_idx, np.int32)
        ns = len(idx) if idx is not None else (self.maxSampleCount if n_samples is None else n_samples)
        out = np.empty((fi_end - fi_begin, ns), np.float32)
        L.check(L.lib().cc_eval_calc_batch(self._e, int(fi_begin), int(fi_end), _vp(idx), ns, _vp(out), 0))
        return out

    def calc_batch_sorted(self, fi_begin, fi_end, n_samples=None, idx_bytes=None):
        """Values and per-feature argsort of the samples (the sorted-index half of precalculate)."""
        ns = self.maxSampleCount if n_samples is None else n_samples
        if idx_bytes is None:
            idx_bytes = 2 if ns < 65536 else 4  # is_buf_16u, o_cvcascadeboosttraindata.cpp:250-251
        vals = np.empty((fi_end - fi_begin, ns), np.float32)
        idx = np.empty((fi_end - fi_begin, ns), np.uint16 if idx_bytes == 2 else np.int32)
        L.check(L.lib().cc_eval_calc_batch_sorted(self._e, int(fi_begin), int(fi_end), ns, _vp(vals), _vp(idx), idx_bytes))
        return vals, idx

    def calc_batch_device(self, fi_begin, fi_end, out_ptr, sample_idx=None, n_samples=None, pitch=0):
        """Values into device memory at out_ptr, rows `pitch` floats apart (0 = densely packed)."""
        idx = None if sample_idx is None else np.ascontiguousarray(sample_idx, np.int32)
        ns = len(idx) if idx is not None else (self.maxSampleCount if n_samples is None else n_samples)
        L.check(L.lib().cc_eval_calc_batch_device(self._e, int(fi_begin), int(fi_end), _vp(idx), ns, C.c_void_p(out_ptr), int(pitch)))

    def calc_custom_haar(self, feats, normalized=False, sample_idx=None, n_samples=None) -> np.ndarray:
        """feats: list of (tilted, [(x, y, w, h, weight), ...]) — Feature::calc on stored samples."""
        arr = (L.HaarFeatureC * len(feats))()
        for i, (tilted, rects) in enumerate(feats):
            arr[i].tilted = 1 if tilted else 0
            for j, r in enumerate(rects):
                for k in range(4):
                    arr[i].r[j][k] = int(r[k])
                arr[i].w[j] = float(r[4])
        idx = None if sample_idx is None else np.ascontiguousarray(sample_idx, np.int32)
        ns = len(idx) if idx is not None else (self.maxSampleCount if n_samples is None else n_samples)
        out = np.empty((len(feats), ns), np.float32)
        L.check(L.lib().cc_eval_calc_custom_haar(self._e, arr, len(feats), 1 if normalized else 0, _vp(idx), ns, _vp(out)))
        return out

    def predict_cascade(self, cascade, sample_idx=None, n_samples=None) -> np.ndarray:
        idx = None if sample_idx is None else np.ascontiguousarray(sample_idx, np.int32)
        ns = len(idx) if idx is not None else (self.maxSampleCount if n_samples is None else n_samples)
        out = np.empty(ns, np.uint8)
        L.check(L.lib().cc_eval_predict_cascade(self._e, cascade._c, _vp(idx), ns, _vp(out)))
        return out

    def fill_passed(self, cascade, imgs, first_idx, want, label=1):
        """fillPassedSamples for packed candidates (the positives, cascadeclassifier.cpp:312): the candidates that pass
        `cascade` (None: all) fill slots first_idx .. in order, at most `want`. Returns (n_filled, n_consumed)."""
        imgs = np.ascontiguousarray(imgs, np.uint8)
        if imgs.ndim != 3 or imgs.shape[1:] != (self.winSize[1], self.winSize[0]):
            raise L.CascadeError(L.CC_ERR_INVALID_ARG, "fill_passed: images do not match winSize")
        nf, nc = C.c_int(0), C.c_int64(0)
        L.check(L.lib().cc_eval_fill_passed(self._e, None if cascade is None else cascade._c, _vp(imgs), imgs.shape[0], int(first_idx),
                                            int(want), int(label), C.byref(nf), C.byref(nc)))
        return nf.value, nc.value

    # ---- best-split search of a boosted-tree node (CvDTree::find_best_split, o_cvdtree.cpp:313-357)
    def presort(self, n_samples=None, fi_begin=0, fi_end=None, *, resident_vars=None, chunk_vars=None, budget_bytes=None):
        """Evaluate features [fi_begin, fi_end) (default: all) on stored samples [0, n_samples) and keep the sorted
        order (Haar, HOG) / the category codes (LBP) resident on the device; call again whenever the stored samples change.

        Past the memory limit (ordered variables; cc_eval_presort_split): resident_vars of the range's variables keep
        their tables, the others are evaluated, sorted and searched chunk_vars at a time at every node, with results
        bit-identical to the resident presort. budget_bytes plans the two numbers (presort_plan; 0: the free device
        memory plus what this evaluator already holds for tables). Returns (resident_vars, chunk_vars) as used, or None
        for the plain call with all three left at None."""
        n = self.maxSampleCount if n_samples is None else int(n_samples)
        self._presorted = (int(fi_begin), self.getNumVariables() if fi_end is None else int(fi_end))
        f0, f1 = self._presorted
        if resident_vars is None and chunk_vars is None and budget_bytes is None:
            L.check(L.lib().cc_eval_presort_range(self._e, f0, f1, n))
            return None
        if budget_bytes is not None:
            if resident_vars is not None or chunk_vars is not None:
                raise ValueError("presort: budget_bytes plans resident_vars and chunk_vars; give either the budget or the two")
            resident_vars, chunk_vars, _ = self.presort_plan(n, f1 - f0, budget_bytes)
        if resident_vars is None:
            raise ValueError("presort: chunk_vars needs resident_vars")
        if chunk_vars is None:
            chunk_vars = 64
        L.check(L.lib().cc_eval_presort_split(self._e, f0, f1, n, int(resident_vars), int(chunk_vars)))
        return int(resident_vars), int(chunk_vars)

    def presort_plan(self, n_samples, n_vars=None, budget_bytes=0):
        """cc_presort_plan for this evaluator's feature type: (resident_vars, chunk_vars, bytes_needed) of a presort of
        n_vars variables (default: all) over n_samples within budget_bytes; chunk_vars is 0 when everything fits.
        budget_bytes = 0: the free device memory plus table_bytes()."""
        nv = self.getNumVariables() if n_vars is None else int(n_vars)
        budget = C.c_uint64(int(budget_bytes))
        if budget.value == 0:
            L.check(L.lib().cc_eval_presort_budget(self._e, C.byref(budget)))
        return presort_plan(self.feature_type, nv, n_samples, budget.value)

    def table_bytes(self) -> int:
        """Device bytes held for sorted tables plus streaming scratch (cc_eval_table_bytes)."""
        b = C.c_uint64(0)
        L.check(L.lib().cc_eval_table_bytes(self._e, C.byref(b)))
        return b.value

    STREAM_PHASES = ("evaluate", "sort", "interleave", "search", "winner")

    def stream_profile(self, enable=True):
        """Events between the steps of every streamed chunk (cc_eval_stream_profile); read them with stream_phase_ms."""
        L.check(L.lib().cc_eval_stream_profile(self._e, 1 if enable else 0))

    def stream_phase_ms(self) -> dict:
        """Device time of the last streamed search by step, summed over its chunks (cc_eval_stream_phase_ms)."""
        ms = np.zeros(len(self.STREAM_PHASES), np.float64)
        k = C.c_int(0)
        L.check(L.lib().cc_eval_stream_phase_ms(self._e, _vp(ms), len(ms), C.byref(k)))
        return dict(zip(self.STREAM_PHASES, ms.tolist()))

    def find_best_split(self, weights, *, responses=None, class_labels=None, sample_idx=None, node_value=0.0,
                        boost_type=BOOST_GENTLE, split_criteria=0, per_var=False):
        """weights: n + 2 doubles (CvBoostTree::calc_node_value's subtree weights: per sample, then the totals).
        Returns a dict (found, var_idx, quality, ord_c, split_point, subset); with per_var=True also the per-variable
        best qualities (float64) and split points."""
        w = np.ascontiguousarray(weights, np.float64)
        n = len(w) - 2
        idx = None if sample_idx is None else np.ascontiguousarray(sample_idx, np.int32)
        if idx is not None and len(idx) != n:
            raise ValueError("weights must hold len(sample_idx) + 2 values")
        resp = None if responses is None else np.ascontiguousarray(responses, np.float32)
        lab = None if class_labels is None else np.ascontiguousarray(class_labels, np.int32)
        for a in (resp, lab):
            if a is not None and len(a) != n:
                raise ValueError("responses / class_labels must hold one value per node sample")
        sp = L.Split()
        nf = self._presorted[1] - self._presorted[0] if getattr(self, "_presorted", None) else self.getNumVariables()
        q = np.empty(nf, np.float64) if per_var else None
        pt = np.empty(nf, np.int32) if per_var else None
        L.check(L.lib().cc_eval_find_best_split(self._e, _vp(idx), n, _vp(w), _vp(resp), _vp(lab), float(node_value), int(boost_type),
                                                int(split_criteria), C.byref(sp), _vp(q), _vp(pt)))
        out = {"found": bool(sp.found), "var_idx": sp.var_idx, "quality": np.float32(sp.quality), "ord_c": np.float32(sp.ord_c),
               "split_point": sp.split_point, "subset": np.array(sp.subset[:], np.int32)}
        return (out, q, pt) if per_var else out

    def getNumFeatures(self) -> int:
        return L.lib().cc_eval_num_features(self._e)

    def getNumVariables(self) -> int:
        """The trainer's variable count, getNumFeatures() * getFeatureSize() (o_cvcascadeboosttraindata.cpp:246-247)."""
        return self.getNumFeatures() * self.getFeatureSize()

    def getMaxCatCount(self) -> int:
        return L.lib().cc_eval_max_cat_count(self._e)

    def getFeatureSize(self) -> int:
        return L.lib().cc_eval_feature_size(self._e)

    def getCls(self, si=None):
        p = L.lib().cc_eval_labels(self._e)
        a = np.ctypeslib.as_array(p, shape=(self.maxSampleCount,))
        return a if si is None else float(a[si])

    def feature_geometry(self, fi):
        """Haar: (rects[3][4], weights[3], tilted); LBP: (cell,); HOG: cells[4][4] (x, y, w, h of cells 0..3)."""
        if self.feature_type == HOG:
            cells = np.zeros((4, 4), np.int32)
            L.check(L.lib().cc_eval_hog_feature_geometry(self._e, int(fi), _vp(cells)))
            return cells
        rects = np.zeros((3, 4), np.int32)
        w = np.zeros(3, np.float32)
        t = C.c_int(0)
        L.check(L.lib().cc_eval_feature_geometry(self._e, int(fi), _vp(rects), _vp(w), C.byref(t)))
        return (rects[0].copy(),) if self.feature_type == LBP else (rects, w, t.value)

    def get_sample(self, idx):
        """Haar / LBP: (sum, tilted or None, norm factor or None); HOG: (hist[9, H+1, W+1], norm[H+1, W+1])."""
        if self.feature_type == HOG:
            shape = (self.winSize[1] + 1, self.winSize[0] + 1)
            hist = np.empty((9,) + shape, np.float32)
            norm = np.empty(shape, np.float32)
            L.check(L.lib().cc_eval_get_hog_sample(self._e, int(idx), _vp(hist), _vp(norm)))
            return hist, norm
        cols = (self.winSize[0] + 1) * (self.winSize[1] + 1)
        s = np.empty(cols, np.int32)
        haar = self.feature_type == HAAR
        t = np.empty(cols, np.int32) if haar and self.featureParams.mode == ALL else None
        nf = np.empty(1, np.float32) if haar else None
        L.check(L.lib().cc_eval_get_sample(self._e, int(idx), _vp(s), _vp(t), _vp(nf)))
        return s, t, (float(nf[0]) if nf is not None else None)

    def last_kernel_ms(self) -> float:
        ms = C.c_double(0)
        L.check(L.lib().cc_eval_last_kernel_ms(self._e, C.byref(ms)))
        return ms.value

    def _release(self):
        if getattr(self, "_e", None):
            L.lib().cc_eval_destroy(self._e)
            self._e = C.c_void_p()

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass


def _weak_dict(w: L.Weak) -> dict:
    return {"trained": bool(w.trained), "stop": w.stop, "n_active": w.n_active, "var_idx": w.var_idx, "split_point": w.split_point,
            "quality": np.float32(w.quality), "ord_c": np.float32(w.ord_c), "subset": np.array(w.subset[:], np.int32),
            "left_value": w.left_value, "right_value": w.right_value, "stage_threshold": np.float32(w.stage_threshold),
            "hit_rate": np.float32(w.hit_rate), "false_alarm": np.float32(w.false_alarm)}


class CascadeBoost:
    """One stage of CvCascadeBoost::train (boost.cpp:409-459) on the device, with weak trees of at most max_depth levels
    of splits (1: stumps): weights, subsample mask, weak responses and stage sums stay there; the split of every node is
    the evaluator's presorted search. The evaluator must have been presorted over exactly n_samples; presorting or setting
    images again invalidates the booster. With max_depth > 1 a trained record also carries the tree in the writer's order
    (CvCascadeBoostTree::write): "nodes", a list of dicts (left, right, depth, n_samples, var_idx, split_point, quality,
    ord_c, subset, value), and "leaves", len(nodes) + 1 values."""

    STOP_GO_ON, STOP_FALSE_ALARM, STOP_MAX_WEAK, STOP_NO_ACTIVE, STOP_NOT_TRAINED = 0, 1, 2, 3, 4
    ROUND_PARTS = ("node_table_root", "split_search", "winner", "apply_split", "leaves", "update_weights", "trim", "stage_status")

    def __init__(self, evaluator: CvFeatureEvaluator, n_samples: int, boost_type=BOOST_GENTLE, split_criteria=SPLIT_DEFAULT,
                 weight_trim_rate=0.95, min_hit_rate=0.995, max_false_alarm=0.5, max_weak_count=100, max_depth=1):
        self._b = C.c_void_p()
        self._evaluator = evaluator  # keep the evaluator alive
        self.n_samples = int(n_samples)
        self.max_weak_count = int(max_weak_count)
        self.max_depth = int(max_depth)
        p = L.BoostParams(int(boost_type), int(split_criteria), float(weight_trim_rate), float(min_hit_rate), float(max_false_alarm),
                          int(max_weak_count))
        L.check(L.lib().cc_boost_create_depth(evaluator._e, self.n_samples, C.byref(p), self.max_depth, C.byref(self._b)))

    def last_tree(self):
        """(nodes, leaves) of the last trained round's tree (cc_boost_last_tree)."""
        k = C.c_int(0)
        st = L.lib().cc_boost_last_tree(self._b, None, 0, None, 0, C.byref(k))
        if st != L.CC_ERR_BUFFER_TOO_SMALL:
            L.check(st)
        nodes = (L.TreeNode * k.value)()
        leaves = np.empty(k.value + 1, np.float64)
        L.check(L.lib().cc_boost_last_tree(self._b, nodes, k.value, _vp(leaves), len(leaves), C.byref(k)))
        names = [n for n, _ in L.TreeNode._fields_ if n != "subset"]
        return [dict({n: getattr(nd, n) for n in names}, subset=np.array(list(nd.subset), np.int32)) for nd in nodes], leaves

    def round(self) -> dict:
        """One weak classifier: the record of cc_boost_round as a dict."""
        w = L.Weak()
        L.check(L.lib().cc_boost_round(self._b, C.byref(w)))
        rec = _weak_dict(w)
        if self.max_depth > 1 and rec["trained"]:
            rec["nodes"], rec["leaves"] = self.last_tree()
        return rec

    def train_stage(self) -> list:
        """Rounds until one says stop; the records of all of them (the last one carries the stage threshold)."""
        if self.max_depth > 1:  # a round's tree has to be fetched before the next round replaces it
            recs = []
            while len(recs) <= self.max_weak_count:
                recs.append(self.round())
                if recs[-1]["stop"] != 0:
                    break
            return recs
        cap = self.max_weak_count + 1
        arr = (L.Weak * cap)()
        k = C.c_int(0)
        L.check(L.lib().cc_boost_train_stage(self._b, arr, cap, C.byref(k)))
        return [_weak_dict(arr[i]) for i in range(k.value)]

    def state(self) -> dict:
        n = self.n_samples
        w, we, ss = (np.empty(n, np.float64) for _ in range(3))
        m = np.empty(n, np.uint8)
        L.check(L.lib().cc_boost_get_state(self._b, _vp(w), _vp(we), _vp(m), _vp(ss)))
        return {"weights": w, "weak_eval": we, "mask": m, "stage_sum": ss}

    def last_round_ms(self) -> dict:
        """Device time of the last round's kernels, by part."""
        ms = np.zeros(len(self.ROUND_PARTS), np.float64)
        k = C.c_int(0)
        L.check(L.lib().cc_boost_last_round_ms(self._b, _vp(ms), len(ms), C.byref(k)))
        return dict(zip(self.ROUND_PARTS, ms.tolist()))

    def _release(self):
        if getattr(self, "_b", None):
            L.lib().cc_boost_destroy(self._b)
            self._b = C.c_void_p()

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass


def device_exp(x, device=0) -> np.ndarray:
    """The device's exp(double) (cc_debug_exp64): what update_weights applies to the weak responses."""
    a = np.ascontiguousarray(x, np.float64)
    out = np.empty(a.shape, np.float64)
    L.check(L.lib().cc_debug_exp64(int(device), _vp(a), a.size, _vp(out)))
    return out


class NegativeMiner:
    """Batched form of the negative branch of CvCascadeClassifier::fillPassedSamples (cascadeclassifier.cpp:329-357):
    one call runs the reader's whole window stream of one background image (imagestorage.cpp:57-126) through the
    trained stages on the device."""

    def __init__(self, cascade, device=0):
        self._m = C.c_void_p()
        self._cascade = cascade  # keep the model alive
        L.check(L.lib().cc_negminer_create(cascade._c, device, C.byref(self._m)))
        inf = cascade.info()
        self.win = (inf["win_w"], inf["win_h"])

    @classmethod
    def empty(cls, feature_type, win, device=0):
        """A miner with no trained stage (stage 0 of training): every window of the stream passes."""
        self = cls.__new__(cls)
        self._m = C.c_void_p()
        self._cascade = None
        L.check(L.lib().cc_negminer_create_empty(int(feature_type), int(win[0]), int(win[1]), device, C.byref(self._m)))
        self.win = (int(win[0]), int(win[1]))
        return self

    def fill(self, evaluator, imgs, first_idx, want, *, start=0, got=0, consumed=0, min_acceptance_ratio=0.0, ox=0, oy=0,
             want_keep_index=False):
        """cc_negminer_fill: the negative branch of fillPassedSamples over the window stream of `imgs` (one size, one offset),
        from stream position `start`, straight into the evaluator's slots first_idx ..; `got` / `consumed` are the stage's
        counts so far. Returns a dict: n_filled, n_consumed, stop (CC_FILL_*), and keep_index if asked for."""
        imgs = [np.ascontiguousarray(im, np.uint8) for im in imgs]
        if not imgs:
            raise ValueError("fill: no image")
        h, w = imgs[0].shape
        if any(im.shape != (h, w) for im in imgs):
            raise ValueError("fill: images of one size only")
        k = len(imgs)
        ptrs = (C.c_void_p * k)(*[im.ctypes.data for im in imgs])
        keep = np.zeros(max(int(want), 1), np.int64) if want_keep_index else None
        nf, nc, stop = C.c_int(0), C.c_int64(0), C.c_int(0)
        L.check(L.lib().cc_negminer_fill(self._m, evaluator._e, ptrs, k, w, h, w, int(ox), int(oy), int(start), int(first_idx), int(want),
                                         int(got), int(consumed), float(min_acceptance_ratio), C.byref(nf), C.byref(nc), C.byref(stop),
                                         _vp(keep)))
        out = {"n_filled": nf.value, "n_consumed": nc.value, "stop": stop.value}
        if want_keep_index:
            out["keep_index"] = keep[:nf.value].copy()
        return out

    def plan(self, width, height, ox=0, oy=0):
        lw, lh, nx, ny = (np.zeros(64, np.int32) for _ in range(4))
        nl, nw = C.c_int(0), C.c_int64(0)
        L.check(L.lib().cc_negminer_plan(self._m, width, height, ox, oy, _vp(lw), _vp(lh), _vp(nx), _vp(ny), 64, C.byref(nl), C.byref(nw)))
        k = nl.value
        return {"levels": list(zip(lw[:k].tolist(), lh[:k].tolist(), nx[:k].tolist(), ny[:k].tolist())), "n_windows": nw.value}

    def run(self, img, ox=0, oy=0, max_keep=64):
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        cap = self.plan(w, h, ox, oy)["n_windows"]
        flags = np.zeros(max(cap, 1), np.uint8)
        pix = np.zeros((max(max_keep, 1), self.win[1], self.win[0]), np.uint8)
        idx = np.zeros(max(max_keep, 1), np.int64)
        nw, nk = C.c_int64(0), C.c_int(0)
        L.check(L.lib().cc_negminer_run(self._m, _vp(img), w, h, w, ox, oy, _vp(flags), cap, C.byref(nw), _vp(pix), _vp(idx),
                                        max_keep, C.byref(nk)))
        return flags[:nw.value].copy(), pix[:nk.value].copy(), idx[:nk.value].copy()

    def run_batch(self, imgs, ox=0, oy=0, max_keep=64):
        """cc_negminer_run_batch: several images of one size, one offset (consecutive images of a background set). Returns
        (flags [n_images][n_windows], kept pixels, kept indices as image * n_windows + stream index)."""
        imgs = [np.ascontiguousarray(im, np.uint8) for im in imgs]
        h, w = imgs[0].shape
        if any(im.shape != (h, w) for im in imgs):
            raise ValueError("run_batch: images of one size only")
        k = len(imgs)
        per = self.plan(w, h, ox, oy)["n_windows"]
        flags = np.zeros(max(per * k, 1), np.uint8)
        pix = np.zeros((max(max_keep, 1), self.win[1], self.win[0]), np.uint8)
        idx = np.zeros(max(max_keep, 1), np.int64)
        ptrs = (C.c_void_p * k)(*[im.ctypes.data for im in imgs])
        nw, nk = C.c_int64(0), C.c_int(0)
        L.check(L.lib().cc_negminer_run_batch(self._m, ptrs, k, w, h, w, ox, oy, _vp(flags), per * k, C.byref(nw), _vp(pix), _vp(idx),
                                              max_keep, C.byref(nk)))
        return flags[:nw.value * k].reshape(k, nw.value).copy(), pix[:nk.value].copy(), idx[:nk.value].copy()

    def __del__(self):
        try:
            if self._m:
                L.lib().cc_negminer_destroy(self._m)
                self._m = C.c_void_p()
        except Exception:
            pass
