"""Witness of one boosted stage of stumps: the contract of the C ABI's section 6b restated operation by operation in
plain Python floats (IEEE doubles; numpy.float32 where the reference computes in float), citing the reference's lines.

Only two things are taken from elsewhere: the split of a node comes from oracle.find_best_split (the CPU oracle of the
split search, as tests/test_gpu_split.py uses it), and `exp`, the vector exponential of update_weights, is a parameter:
math.exp for CPU tests, the device's exp on the GPU (the reference's cvExp is OpenCV's own routine; parity of these n
exponentials with it is unpinned)."""
import math

import numpy as np

from oracle import oracle as orc

DISCRETE, REAL, LOGIT, GENTLE = 0, 1, 2, 3
FLT_EPSILON = float(np.finfo(np.float32).eps)
DBL_MAX = float(np.finfo(np.float64).max)
F32 = np.float32


def libm_exp(a):
    return np.array([math.exp(float(v)) for v in a], np.float64)


def log_ratio(val):
    """o_cvboostree.cpp:11-17 / boost.cpp:28-36"""
    eps = 1e-5
    val = max(val, eps)
    val = min(val, 1. - eps)
    return math.log(val / (1. - val))


def trim_walk(weights, rate):
    """CvBoost::trim_weights (o_cvboost.cpp:113-134) for 0 < rate < 1: (mask, threshold)."""
    srt = sorted(float(w) for w in weights)
    count = len(srt)
    s = 1. - rate
    i = 0
    while i < count:
        if s <= 0:
            break
        s -= srt[i]
        i += 1
    threshold = srt[i] if i < count else DBL_MAX
    mask = np.array([1 if float(w) >= threshold else 0 for w in weights], np.uint8)
    return mask, threshold


def is_err_desired(stage_sum, labels, min_hit_rate, max_false_alarm):
    """CvCascadeBoost::isErrDesired (boost.cpp:479-518) in the reference's types: (threshold, hitRate, falseAlarm, done)."""
    ev = sorted(F32(stage_sum[i]) for i in range(len(labels)) if labels[i] == 1)  # predict(i, true) returns (float)sum
    num_pos = len(ev)
    threshold_idx = int((F32(1.0) - F32(min_hit_rate)) * F32(num_pos))
    threshold = ev[threshold_idx]
    num_pos_true = num_pos - threshold_idx
    for i in range(threshold_idx - 1, -1, -1):
        if abs(F32(ev[i] - threshold)) < FLT_EPSILON:
            num_pos_true += 1
    hit = F32(num_pos_true) / F32(num_pos)
    num_neg = num_false = 0
    bound = float(F32(threshold - F32(0.00001)))  # threshold - CV_THRESHOLD_EPS, a float; the sum is a double
    for i in range(len(labels)):
        if labels[i] == 0:
            num_neg += 1
            if not (float(stage_sum[i]) < bound):
                num_false += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        fa = F32(num_false) / F32(num_neg)
    return F32(threshold), hit, fa, bool(fa <= F32(max_false_alarm))


class BoostWitness:
    def __init__(self, vals, labels, boost_type=GENTLE, categorical=False, exp=libm_exp, split_criteria=0, weight_trim_rate=0.95,
                 min_hit_rate=0.995, max_false_alarm=0.5, max_weak_count=100, var0=0):
        """vals: [F][n] float32 values of every searched variable on every sample; labels: n values 0 / 1."""
        self.vals = np.ascontiguousarray(vals, np.float32)
        self.n = self.vals.shape[1]
        self.labels = [int(v) for v in labels]
        self.boost_type, self.categorical, self.exp, self.split_criteria = boost_type, categorical, exp, split_criteria
        self.rate, self.min_hit_rate, self.max_false_alarm, self.max_weak_count = weight_trim_rate, min_hit_rate, max_false_alarm, max_weak_count
        self.var0 = var0
        self.classifier = boost_type in (DISCRETE, REAL)
        n = self.n
        # boost.cpp:190-265: orig_response = 2 * class - 1, every sample active, weights 1./n; Gentle responses (float)y
        self.y = [2 * c - 1 for c in self.labels]
        self.weights = [1. / n] * n
        self.mask = [1] * n
        self.weak_eval = [0.0] * n
        self.stage_sum = [0.0] * n
        self.have_subsample = False
        self.n_weak = 0
        self.threshold, self.hit_rate, self.false_alarm = F32(0), F32(0), F32(0)
        self.exp_args = []  # every argument the vector exp saw

    def state(self):
        return {"weights": np.array(self.weights), "weak_eval": np.array(self.weak_eval), "mask": np.array(self.mask, np.uint8),
                "stage_sum": np.array(self.stage_sum)}

    def _node_value(self, idx):
        """calc_node_value (o_cvboostree.cpp:657-732) over samples idx in order: (value, rcw, sum, risk, class counts)."""
        w, y = self.weights, self.y
        rcw = [0.0, 0.0]
        if self.classifier:
            cnt = [0, 0]
            for i in idx:
                r = self.labels[i]
                rcw[r] += w[i]
                cnt[r] += 1
            if self.boost_type == DISCRETE:
                value = float((1 if rcw[1] > rcw[0] else 0) * 2 - 1)
            else:
                value = 0.5 * log_ratio(rcw[1] / (rcw[0] + rcw[1]))
            return value, rcw, 0.0, 0.0, cnt
        s = s2 = 0.0
        for i in idx:
            t = float(F32(y[i]))
            rcw[0] += w[i]
            s += t * w[i]
            s2 += t * t * w[i]
        n = len(idx)
        iw = 1. / rcw[0]
        value = s * iw
        risk = s2 - (s * iw) * s
        risk *= n * iw * n * iw
        return value, rcw, s, risk, None

    def _left_by_predict(self, i, rec):
        """CvCascadeBoostTree::predict (o_cvcascadeboosttree.cpp:16-39)"""
        v = self.vals[rec["var_idx"] - self.var0][i]
        if not self.categorical:
            return bool(v <= rec["ord_c"])
        c = int(v)
        return bool((int(rec["subset"][c >> 5]) >> (c & 31)) & 1)

    def round(self):
        n, w, y = self.n, self.weights, self.y
        rec = {"trained": False, "stop": 4, "var_idx": -1, "split_point": -1, "quality": F32(-1), "ord_c": F32(0), "subset": np.zeros(8, np.int32),
               "left_value": 0.0, "right_value": 0.0, "stage_threshold": self.threshold, "hit_rate": self.hit_rate, "false_alarm": self.false_alarm}
        active = [i for i in range(n) if self.mask[i]]  # cvPreprocessIndexArray of the mask: increasing sample order
        na = len(active)
        rec["n_active"] = na
        # 1. root calc_node_value; 2. no tree (o_cvdtree.cpp:130-145)
        if na == 0:
            return rec
        value, rcw, _, risk, cnt = self._node_value(active)
        if na <= 10:
            return rec
        if self.classifier:
            if (cnt[0] != 0) + (cnt[1] != 0) == 1:
                return rec
        elif risk >= 0 and math.sqrt(risk) / na < float(F32(0.01)):
            return rec
        # 3. best split
        W = np.array([w[i] for i in active] + [rcw[0], rcw[1]], np.float64)
        sub = self.vals[:, active]
        if self.classifier:
            sp = orc.find_best_split(sub, W, categorical=self.categorical, class_labels=np.array([self.labels[i] for i in active], np.int32),
                                     node_value=value, boost_type=self.boost_type, split_criteria=self.split_criteria)
        else:
            sp = orc.find_best_split(sub, W, categorical=self.categorical, responses=np.array([F32(y[i]) for i in active], np.float32),
                                     node_value=value, boost_type=self.boost_type, split_criteria=self.split_criteria)
        if not sp["found"]:
            return rec
        var = int(sp["var_idx"])
        rec.update(trained=True, var_idx=self.var0 + var, quality=F32(sp["quality"]))
        # 4. directions (calc_node_dir, o_cvboostree.cpp:87-149)
        left = {}
        if self.categorical:
            rec["subset"] = np.array(sp["subset"], np.int32)
            for i in active:
                c = int(self.vals[var][i])
                left[i] = bool((int(rec["subset"][c >> 5]) >> (c & 31)) & 1)
        else:
            rec["ord_c"], rec["split_point"] = F32(sp["ord_c"]), int(sp["split_point"])
            order = np.argsort(sub[var], kind="stable")  # ties in presort (increasing sample) order
            for rank, k in enumerate(order):
                left[active[int(k)]] = rank <= rec["split_point"]
        # 5. leaves: calc_node_value of each child over its samples in increasing order
        lv = self._node_value([i for i in active if left[i]])[0]
        rv = self._node_value([i for i in active if not left[i]])[0]
        for i in active:
            self.weak_eval[i] = lv if left[i] else rv
        # 6. update_weights(tree) (boost.cpp:266-406)
        if self.have_subsample:
            for i in range(n):
                if not self.mask[i]:
                    self.weak_eval[i] = lv if self._left_by_predict(i, rec) else rv
        sum_w = 0.0
        we = self.weak_eval
        scale_c = 1.0
        if self.boost_type == DISCRETE:
            err = 0.0
            for i in range(n):
                sum_w += w[i]
                err += w[i] * (1 if we[i] != y[i] else 0)
            if sum_w != 0:
                err /= sum_w
            scale_c = err = -log_ratio(err)
            scale = [1., math.exp(err)]
            sum_w = 0.0
            for i in range(n):
                w[i] = w[i] * scale[1 if we[i] != y[i] else 0]
                sum_w += w[i]
            lv *= scale_c  # tree->scale(C)
            rv *= scale_c
        else:
            for i in range(n):
                we[i] *= -y[i]
            self.exp_args.extend(we)
            ex = self.exp(np.array(we, np.float64))
            for i in range(n):
                we[i] = float(ex[i])
                w[i] = w[i] * we[i]
                sum_w += w[i]
        if sum_w > FLT_EPSILON:
            sum_w = 1. / sum_w
            for i in range(n):
                w[i] *= sum_w
        rec["left_value"], rec["right_value"] = lv, rv
        self.n_weak += 1
        # 7. stage sums: predict(i)->value of the new tree, by the threshold rule (boost.cpp:461-473)
        for i in range(n):
            self.stage_sum[i] += lv if self._left_by_predict(i, rec) else rv
        # 8. trim_weights
        if 0. < self.rate < 1.:
            m, _ = trim_walk(w, self.rate)
            self.mask = [int(v) for v in m]
            self.have_subsample = sum(self.mask) < n
        if sum(self.mask) == 0:  # boost.cpp:444
            rec["stop"] = 3
            return rec
        # 9. isErrDesired
        self.threshold, self.hit_rate, self.false_alarm, done = is_err_desired(self.stage_sum, self.labels, self.min_hit_rate, self.max_false_alarm)
        rec.update(stage_threshold=self.threshold, hit_rate=self.hit_rate, false_alarm=self.false_alarm)
        rec["stop"] = 1 if done else (2 if self.n_weak >= self.max_weak_count else 0)
        return rec


RECORD_FIELDS = ("trained", "stop", "n_active", "var_idx", "split_point", "quality", "ord_c", "left_value", "right_value", "stage_threshold",
                 "hit_rate", "false_alarm")


def assert_round_equal(got, want, got_state, want_state, where):
    """Every field of the record and the full state, tolerance 0.0."""
    for k in RECORD_FIELDS:
        g, x = got[k], want[k]
        same = (g == x) or (isinstance(g, (float, np.floating)) and math.isnan(float(g)) and math.isnan(float(x)))
        assert same, (where, k, g, x)
    assert (np.asarray(got["subset"]) == np.asarray(want["subset"])).all(), (where, "subset")
    if not want["trained"]:
        return
    for k in ("weights", "weak_eval", "mask", "stage_sum"):
        bad = np.nonzero(got_state[k] != want_state[k])[0]
        assert len(bad) == 0, (where, k, len(bad), int(bad[0]), got_state[k][bad[0]], want_state[k][bad[0]])
