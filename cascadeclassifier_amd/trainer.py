"""The cascade driver: CvCascadeClassifier::train with updateTrainingSet / fillPassedSamples
(traincascade/lib/src/cascadeclassifier.cpp:203-284, :308-357) and the background reader CvCascadeImageReader::NegReader
(imagestorage.cpp:57-126) over images held in memory. Every arithmetic step runs on the device: the positives through
CvFeatureEvaluator.fill_passed, the negatives through NegativeMiner.fill, a stage through CascadeBoost."""
from __future__ import annotations

import math
import time

import numpy as np

from . import _lib as L
from .detector import CascadeClassifier
from .evaluator import (BASIC, BOOST_GENTLE, HAAR, CascadeBoost, CvFeatureEvaluator, CvFeatureParams, NegativeMiner)

_F = np.float32
_SCALE_FACTOR = _F(1.4142135623730950488016887242097)
_STEP_FACTOR = _F(0.5)

END_NUM_STAGES = "all stages trained"
END_CANNOT_FILL = "train dataset for temp stage can not be filled"
END_LEAF_FA_RATE = "required leaf false alarm rate achieved"
END_ACCEPTANCE_BREAK = "acceptanceRatioBreakValue reached"
END_STAGE_NOT_TRAINED = "stage could not be trained"


def stream_ladder(win, cols, rows, ox, oy):
    """The levels of one image's window stream as (width, height, nx, ny), in the reader's float arithmetic
    (imagestorage.cpp:82-85, :105-117): level 0 first; nx * ny windows per level, rows top to bottom."""
    W, H = win
    scale = max((_F(W) + _F(ox)) / _F(cols), (_F(H) + _F(oy)) / _F(rows))
    lw, lh = int(scale * _F(cols) + _F(0.5)), int(scale * _F(rows) + _F(0.5))
    out = []
    while True:
        x, nx = ox, 1
        while int(_F(x) + (_F(1.0) + _STEP_FACTOR) * _F(W)) < lw:
            x += int(_STEP_FACTOR * _F(W))
            nx += 1
        y, ny = oy, 1
        while int(_F(y) + (_F(1.0) + _STEP_FACTOR) * _F(H)) < lh:
            y += int(_STEP_FACTOR * _F(H))
            ny += 1
        out.append((lw, lh, nx, ny))
        scale = scale * _SCALE_FACTOR
        if not scale <= _F(1.0):
            return out
        lw, lh = int(scale * _F(cols)), int(scale * _F(rows))


class BackgroundReader:
    """The state of NegReader over a list of 2-D uint8 images: `last` (the next image of the list), `round` (which
    chooses the offset), the image that is open with its offset, and the position inside that image's window stream,
    which persists from one stage to the next. Windows are handed out in runs (next_batch) and accounted for afterwards
    (advance), where the reference hands them out one at a time."""

    def __init__(self, images, win):
        self.images = [np.ascontiguousarray(im, np.uint8) for im in images]
        self.win = (int(win[0]), int(win[1]))
        if any(im.ndim != 2 for im in self.images):
            raise ValueError("BackgroundReader: 2-D gray images only")
        if not any(im.shape[1] >= self.win[0] and im.shape[0] >= self.win[1] for im in self.images):
            raise ValueError("BackgroundReader: no image holds a %dx%d window" % self.win)
        self.last = 0
        self.round = 0
        self.current = None  # index of the open image; None until the first window is asked for
        self.offset = (0, 0)
        self.position = 0
        self._wins = {}

    def _step(self, last, rnd):
        """nextImg (imagestorage.cpp:57-81) from the state (last, round): the state behind it, the image it opens and
        the offset. The round changes when the LAST image of the list is opened; images too small for the window at
        the offset are skipped."""
        W, H = self.win
        count = len(self.images)
        for _ in range(count):
            idx = last
            last += 1
            rnd += last // count
            rnd %= W * H
            last %= count
            rows, cols = self.images[idx].shape
            ox, oy = min(rnd % W, cols - W), min(rnd // W, rows - H)
            if ox >= 0 and oy >= 0:
                return last, rnd, idx, (ox, oy)
        raise AssertionError("an image that holds a window was checked for at construction")

    def _next_img(self):
        self.last, self.round, self.current, self.offset = self._step(self.last, self.round)
        self.position = 0

    def stream_length(self, idx, offset):
        rows, cols = self.images[idx].shape
        key = (cols, rows) + tuple(offset)
        if key not in self._wins:
            self._wins[key] = sum(nx * ny for _, _, nx, ny in stream_ladder(self.win, cols, rows, *offset))
        return self._wins[key]

    def next_batch(self, max_images=256):
        """The run of consecutive images, at most max_images, that the reader visits from here with one size and one
        offset. The first is the open image, whose stream continues at `start`. The state does not change."""
        if self.current is None:
            self._next_img()
        idx = [self.current]
        shape = self.images[self.current].shape
        last, rnd = self.last, self.round
        while len(idx) < max_images:
            last, rnd, nxt, off = self._step(last, rnd)
            if off != self.offset or self.images[nxt].shape != shape:
                break
            idx.append(nxt)
        return {"images": [self.images[i] for i in idx], "indices": idx, "ox": self.offset[0], "oy": self.offset[1],
                "start": self.position, "n_windows": self.stream_length(self.current, self.offset)}

    def advance(self, n_consumed):
        """Moves the state over n_consumed windows. Behind an image's last window the next image is opened at once, as
        NegReader::get does (imagestorage.cpp:118-121)."""
        if self.current is None:
            if n_consumed == 0:
                return
            self._next_img()
        position = self.position + int(n_consumed)
        while position >= self.stream_length(self.current, self.offset):
            position -= self.stream_length(self.current, self.offset)
            self._next_img()
        self.position = position

    def state(self):
        return {"last": self.last, "round": self.round, "current": self.current, "offset": self.offset, "position": self.position}

    def restore(self, state):
        """The inverse of state(), for a reader over the same list and window: afterwards the reader hands out the windows
        the reader that gave `state` would have handed out next. ValueError for a state that cannot belong to this list:
        `last` or `round` out of range, an open image that does not follow from them (`last` stands behind the open image,
        and `round` fixes its offset), an image too small for the window at that offset, or a position behind the image's
        stream. Nothing changes when it raises."""
        try:
            last, rnd, position = int(state["last"]), int(state["round"]), int(state["position"])
            current = None if state["current"] is None else int(state["current"])
            offset = tuple(int(v) for v in state["offset"])
        except (KeyError, TypeError, ValueError) as err:
            raise ValueError("BackgroundReader.restore: malformed state (%s)" % err) from None
        W, H = self.win
        count = len(self.images)
        if not 0 <= last < count or not 0 <= rnd < W * H or len(offset) != 2:
            raise ValueError("BackgroundReader.restore: last %d / round %d do not fit %d images and a %dx%d window" % (last, rnd, count, W, H))
        if current is None:
            if (last, rnd, offset, position) != (0, 0, (0, 0), 0):
                raise ValueError("BackgroundReader.restore: a reader that has opened no image stands at its start")
        else:
            if not 0 <= current < count or last != (current + 1) % count:
                raise ValueError("BackgroundReader.restore: image %d is not the one in front of last = %d" % (current, last))
            rows, cols = self.images[current].shape
            if offset != (min(rnd % W, cols - W), min(rnd // W, rows - H)) or min(offset) < 0:
                raise ValueError("BackgroundReader.restore: offset %s is not the one of round %d in image %d (%dx%d)" % (offset, rnd, current, cols, rows))
            if not 0 <= position < self.stream_length(current, offset):
                raise ValueError("BackgroundReader.restore: position %d behind the %d windows of image %d" %
                                 (position, self.stream_length(current, offset), current))
        self.last, self.round, self.current, self.offset, self.position = last, rnd, current, offset, position


# ---- the transcript: the lines the reference prints while it trains, as std::cout prints their numbers ----

def format_number(x) -> str:
    """operator<< of a float or double at the stream's defaults: %g, 6 significant digits."""
    return "%g" % float(x)


def loaded_lines(n_loaded):
    """cascadeclassifier.cpp:203-207"""
    if n_loaded > 1:
        return ["", "Stages 0-%d are loaded" % (n_loaded - 1)]
    return ["", "Stage 0 is loaded"] if n_loaded == 1 else []


def stage_begin_lines(i):
    """cascadeclassifier.cpp:215-216"""
    return ["", "===== TRAINING %d-stage =====" % i, "<BEGIN"]


def fill_lines(record):
    """updateTrainingSet's two lines (cascadeclassifier.cpp:315, :325); the second only when the set could be filled."""
    out = ["POS count : consumed   %d : %d" % (record["pos_count"], record["pos_consumed"])]
    if record["acceptance_ratio"] is not None:
        out.append("NEG count : acceptanceRatio    %d : %s" % (record["neg_count"], format_number(record["acceptance_ratio"])))
    return out


END_MESSAGES = {
    END_CANNOT_FILL: "Train dataset for temp stage can not be filled. Branch training terminated.",
    END_LEAF_FA_RATE: "Required leaf false alarm rate achieved. Branch training terminated.",
    END_ACCEPTANCE_BREAK: "The required acceptanceRatio for the model has been reached to avoid overfitting of trainingdata. "
                          "Branch training terminated.",
}
_TABLE_RULE = "+----+---------+---------+"
_STOP_NO_ACTIVE = 3  # CascadeBoost.STOP_NO_ACTIVE: the round ended before isErrDesired, which prints the row


def boost_lines(weak, precalc_seconds=0):
    """What CvCascadeBoost::train prints for one stage: the presort's whole seconds (o_cvcascadeboosttraindata.cpp), the table of
    isErrDesired (boost.cpp:429-431, :511-515) with one row per round that reached it, and END> (cascadeclassifier.cpp:240)."""
    out = ["Precalculation time: %s" % format_number(int(precalc_seconds)), _TABLE_RULE, "|  N |    HR   |    FA   |", _TABLE_RULE]
    n = 0
    for w in weak:
        if not w["trained"]:
            continue
        n += 1
        if w["stop"] != _STOP_NO_ACTIVE:
            out += ["|%4d|%9s|%9s|" % (n, format_number(w["hit_rate"]), format_number(w["false_alarm"])), _TABLE_RULE]
    return out + ["END>"]


def time_line(seconds):
    """cascadeclassifier.cpp:278-283"""
    s = int(seconds)
    return "Training until now has taken %d days %d hours %d minutes %d seconds." % (s // 86400, s // 3600 % 24, s // 60 % 60, s % 60)


def train_cascade(positives, backgrounds, num_pos, num_neg, num_stages, *, feature_type=HAAR, win=(24, 24), haar_mode=BASIC,
                  boost_type=BOOST_GENTLE, min_hit_rate=0.995, max_false_alarm=0.5, weight_trim_rate=0.95, max_weak_count=100,
                  acceptance_ratio_break_value=-1.0, device=0, max_batch=256, on_stage=None, max_depth=1, table_budget_bytes=None,
                  initial_stages=None, reader=None, log=None):
    """CvCascadeClassifier::train (cascadeclassifier.cpp:203-284) for stages of weak trees with at most max_depth levels of
    splits (the reference's -maxDepth; 1: stumps). positives: [n][win_h][win_w]
    uint8, taken from the first one again for every stage; backgrounds: 2-D uint8 images, read as NegReader reads its list.
    Returns (cascade or None, stage records, end reason); a record holds pos_count, pos_consumed, neg_count, neg_consumed,
    acceptance_ratio and, for a trained stage, weak (the records of CascadeBoost.train_stage). on_stage(i, record, cascade)
    is called after every trained stage. Raises ValueError when the positives run out before num_pos of them pass.
    table_budget_bytes: device memory every stage's presort may use for sorted tables and streaming scratch (0: what is
    free); variables whose tables do not fit are evaluated and sorted again at every node, and the trained cascade is the
    same. None: all tables resident, or an error when they do not fit. The reference's -precalcValBufSize and
    -precalcIdxBufSize size two host caches in MB, one for values and one for sorted indices; here one budget in bytes
    covers both.
    initial_stages: the stages an earlier run trained, a list of (stage_threshold, [weak dicts]) as from_stumps / from_trees
    take them (traincascade.read_stage returns one). The loop starts behind them, like startNumStages (:203-213); with
    num_stages of them or more nothing is trained and the cascade of the first num_stages is returned. The records cover the
    iterations of this call only. reader: a BackgroundReader over `backgrounds` to go on with instead of a fresh one (its
    state() inside on_stage is the state behind that stage). log: a callable that gets the reference's transcript, line by
    line, at the points where the reference prints it."""
    def say(make, *args):  # the lines are made only for a caller who reads them
        if log is not None:
            for line in make(*args):
                log(line)

    t0 = time.monotonic()
    positives = np.ascontiguousarray(positives, np.uint8)
    win = (int(win[0]), int(win[1]))
    if num_pos < 1 or num_neg < 0 or max_batch < 1 or max_depth < 1:
        raise ValueError("train_cascade: num_pos >= 1, num_neg >= 0, max_batch >= 1, max_depth >= 1")
    if reader is None:
        reader = BackgroundReader(backgrounds, win)
    e = CvFeatureEvaluator.create(feature_type, device)
    e.init(CvFeatureParams(feature_type, haar_mode), num_pos + num_neg, win)
    stages = list(initial_stages or [])[:max(num_stages, 0)]

    def build(stages):  # a record with "nodes" is a tree; one without is the stump of its own fields, for either builder
        deep = max_depth > 1 or any("nodes" in w for _, ws in stages for w in ws)
        return (CascadeClassifier.from_trees if deep else CascadeClassifier.from_stumps)(feature_type, win, stages, haar_mode=haar_mode, device=device)

    cascade = build(stages) if stages else None
    miner = NegativeMiner(cascade, device) if stages else NegativeMiner.empty(feature_type, win, device)
    say(loaded_lines, len(stages))
    required_leaf_fa_rate = math.pow(float(np.float32(max_false_alarm)), float(num_stages)) / float(max_depth)  # cascadeclassifier.cpp:209-210
    records = []
    end = END_NUM_STAGES
    for i in range(len(stages), num_stages):
        say(stage_begin_lines, i)
        # updateTrainingSet (:308-327)
        pos_count, pos_consumed = e.fill_passed(cascade, positives, 0, num_pos, 1)
        if pos_count < num_pos:  # PosReader::get raises when the file ends (imagestorage.cpp:173-174)
            raise ValueError("Can not get new positive sample. vec-file is over.")
        pro_num_neg = int(round((float(num_neg) * float(pos_count)) / num_pos))  # cvRound: half to even
        neg_count = neg_consumed = 0
        while neg_count < pro_num_neg:
            b = reader.next_batch(max_batch)
            r = miner.fill(e, b["images"], pos_count + neg_count, pro_num_neg - neg_count, start=b["start"], got=neg_count,
                           consumed=neg_consumed, min_acceptance_ratio=required_leaf_fa_rate, ox=b["ox"], oy=b["oy"])
            neg_count += r["n_filled"]
            neg_consumed += r["n_consumed"]
            reader.advance(r["n_consumed"])
            if r["stop"] != L.CC_FILL_EXHAUSTED:
                break
        record = {"pos_count": pos_count, "pos_consumed": pos_consumed, "neg_count": neg_count, "neg_consumed": neg_consumed,
                  "acceptance_ratio": None, "weak": None}
        records.append(record)
        if neg_count == 0 and not (neg_consumed > 0 and (float(neg_count) + 1) / float(neg_consumed) <= required_leaf_fa_rate):
            end = END_CANNOT_FILL
        else:
            acceptance = 0.0 if neg_consumed == 0 else float(neg_count) / float(neg_consumed)
            record["acceptance_ratio"] = acceptance
            if acceptance <= required_leaf_fa_rate:
                end = END_LEAF_FA_RATE
            elif acceptance <= acceptance_ratio_break_value and acceptance_ratio_break_value >= 0:
                end = END_ACCEPTANCE_BREAK
        say(fill_lines, record)
        if end != END_NUM_STAGES:
            say(lambda: [END_MESSAGES[end]])
            break
        n = pos_count + neg_count
        t_presort = time.monotonic()
        if table_budget_bytes is None:
            e.presort(n)
        else:
            e.presort(n, budget_bytes=table_budget_bytes)
        t_presort = time.monotonic() - t_presort
        weak = CascadeBoost(e, n, boost_type=boost_type, weight_trim_rate=weight_trim_rate, min_hit_rate=min_hit_rate,
                            max_false_alarm=max_false_alarm, max_weak_count=max_weak_count, max_depth=max_depth).train_stage()
        say(boost_lines, weak, t_presort)
        if not any(w["trained"] for w in weak):
            end = END_STAGE_NOT_TRAINED
            break
        record["weak"] = weak
        stages.append((weak[-1]["stage_threshold"], weak))
        cascade = build(stages)
        miner = NegativeMiner(cascade, device)
        if on_stage is not None:
            on_stage(i, record, cascade)
        say(lambda: [time_line(time.monotonic() - t0)])
    return cascade, records, end
