"""The traincascade tool: CvCascadeClassifier::train around train_cascade (traincascade/lib/src/cascadeclassifier.cpp:137-295,
:534-564) with its data directory -- params.xml, stage<i>.xml, cascade.xml -- and its command line (traincascade.cpp:39-166):

    python -m cascadeclassifier_amd.traincascade -data <dir> -vec <file.vec> -bg <list.txt> [-numPos ...] ...

The files are written and read by the C ABI (section 6d of include/cascadeclassifier_amd.h); tags and values follow the
reference's writers, the byte layout of OpenCV's FileStorage is not pinned. Beside the reference's files the directory
holds resume.json, the background reader's state behind every finished stage: with it a run that was killed goes on exactly
where it stopped, where the reference reopens its reader at the first image."""
from __future__ import annotations

import ctypes as C
import json
import os
import sys
from dataclasses import asdict, dataclass

import numpy as np

from . import _lib as L
from . import trainer as T
from .detector import CascadeClassifier, vec_read
from .evaluator import (ALL, BASIC, BOOST_DISCRETE, BOOST_GENTLE, BOOST_LOGIT, BOOST_REAL, CORE, HAAR, HOG, LBP, CvFeatureEvaluator,
                        CvFeatureParams)
from .samples import read_background_list

FEATURE_NAMES = {"HAAR": HAAR, "LBP": LBP, "HOG": HOG}
BOOST_NAMES = {"DAB": BOOST_DISCRETE, "RAB": BOOST_REAL, "LB": BOOST_LOGIT, "GAB": BOOST_GENTLE}
MODE_NAMES = {"BASIC": BASIC, "CORE": CORE, "ALL": ALL}
PARAMS_FILENAME, CASCADE_FILENAME, RESUME_FILENAME = "params.xml", "cascade.xml", "resume.json"
LOGIT_MESSAGE = "cc_boost_create: LOGIT boost is not supported (its responses change every round)"
BASE_FORMAT_MESSAGE = "old file format is used for Haar-like features only"
NOT_TRAINED_MESSAGE = "Cascade classifier can't be trained. Check the used training parameters."
BANNER = ["---------------------------------------------------------------------------------",
          "Training parameters are pre-loaded from the parameter file in data folder!",
          "Please empty this folder if you want to use a NEW set of training parameters.",
          "---------------------------------------------------------------------------------"]


def _name_of(names, value):
    return next(k for k, v in names.items() if v == value)


def _f32(x) -> float:
    return float(np.float32(x))


@dataclass
class TrainParams:
    """cc_train_params: what params.xml holds. minHitRate and maxFalseAlarm are floats in the reference and are narrowed
    here; weightTrimRate is a double and kept. max_cat_count / feat_size None: the feature type's (LBP 256 / 1, HAAR 0 / 1,
    HOG 0 / 36)."""
    feature_type: int = HAAR
    win_w: int = 24
    win_h: int = 24
    boost_type: int = BOOST_GENTLE
    min_hit_rate: float = 0.995
    max_false_alarm: float = 0.5
    weight_trim_rate: float = 0.95
    max_depth: int = 1
    max_weak_count: int = 100
    max_cat_count: int | None = None
    feat_size: int | None = None
    haar_mode: int = BASIC

    def __post_init__(self):
        self.min_hit_rate, self.max_false_alarm = _f32(self.min_hit_rate), _f32(self.max_false_alarm)
        self.weight_trim_rate = float(self.weight_trim_rate)
        if self.max_cat_count is None:
            self.max_cat_count = 256 if self.feature_type == LBP else 0
        if self.feat_size is None:
            self.feat_size = 36 if self.feature_type == HOG else 1
        if self.feature_type != HAAR:
            self.haar_mode = BASIC

    def as_dict(self) -> dict:
        return asdict(self)

    def _c(self) -> L.TrainParams:
        return L.TrainParams(**{n: getattr(self, n) for n, _ in L.TrainParams._fields_})

    @classmethod
    def _from_c(cls, p: L.TrainParams) -> "TrainParams":
        return cls(**{n: getattr(p, n) for n, _ in p._fields_})


def write_params(path: str, params: TrainParams, object_name: str | None = None):
    """params.xml (cc_train_params_save_xml). object_name: the top-level element; None: named after the file."""
    L.check(L.lib().cc_train_params_save_xml(C.byref(params._c()), path.encode(), None if object_name is None else object_name.encode()))


def read_params(path: str):
    """The parameters of a params.xml or of a cascade.xml (cc_train_params_load_xml); None for a cascade file that holds no
    training parameters. CascadeError (CC_ERR_PARSE, the tag named) for a value one of the reference's read()s refuses."""
    p = L.TrainParams()
    st = L.lib().cc_train_params_load_xml(path.encode(), C.byref(p))
    if st == L.CC_ERR_NO_TRAIN_PARAMS:
        return None
    L.check(st)
    return TrainParams._from_c(p)


def _max_cat_count(feature_type) -> int:
    return 256 if feature_type == LBP else 0


def write_stage(path: str, stage, feature_type, object_name: str | None = None):
    """stage<i>.xml (cc_stage_save_xml) from (stage_threshold, [weak dicts]) as from_stumps / from_trees take it: records with
    trained == False are skipped, one with "nodes" and "leaves" is a tree, any other the stump of its own fields. Variable
    indices are written as they are (catalog indices); leaves and thresholds are cast to float as the writer does."""
    thr, weak = stage
    n_nodes, flat, leaves = L.pack_trees([w for w in weak if w.get("trained", True)])
    L.check(L.lib().cc_stage_save_xml(path.encode(), None if object_name is None else object_name.encode(), _max_cat_count(feature_type),
                                      float(np.float32(thr)), len(n_nodes), n_nodes.ctypes.data_as(C.c_void_p), int(n_nodes.sum()), flat,
                                      leaves.ctypes.data_as(C.c_void_p)))


def read_stage(path: str, feature_type, n_variables: int = 0):
    """(stage_threshold, [weak dicts]) of a stage<i>.xml (cc_stage_load_xml), as from_stumps / from_trees and train_cascade's
    initial_stages take it. A tree of one node comes back as a stump (var_idx, ord_c or subset, left_value, right_value), a
    deeper one with "nodes" (left, right, var_idx, ord_c, subset) and "leaves". n_variables > 0: the catalog size, which
    every featureIdx must stay below."""
    lbp = feature_type == LBP
    thr, n_weak, n_total = C.c_float(0), C.c_int(0), C.c_int(0)
    st = L.lib().cc_stage_load_xml(path.encode(), _max_cat_count(feature_type), int(n_variables), C.byref(thr), C.byref(n_weak), None, 0,
                                   C.byref(n_total), None, 0, None)
    if st != L.CC_ERR_BUFFER_TOO_SMALL:
        L.check(st)
    n_nodes = np.zeros(n_weak.value, np.int32)
    nodes = (L.TreeNode * n_total.value)()
    leaves = np.zeros(n_total.value + n_weak.value, np.float32)
    L.check(L.lib().cc_stage_load_xml(path.encode(), _max_cat_count(feature_type), int(n_variables), C.byref(thr), C.byref(n_weak),
                                      n_nodes.ctypes.data_as(C.c_void_p), len(n_nodes), C.byref(n_total), nodes, len(nodes),
                                      leaves.ctypes.data_as(C.c_void_p)))

    def split(nd):
        return {"var_idx": nd.var_idx, "subset": np.array(nd.subset[:], np.int32)} if lbp else {"var_idx": nd.var_idx, "ord_c": np.float32(nd.ord_c)}

    weak, k = [], 0
    for t, nn in enumerate(int(v) for v in n_nodes):
        lv = leaves[k + t:k + t + nn + 1]
        if nn == 1:
            weak.append(dict(split(nodes[k]), left_value=np.float32(lv[0]), right_value=np.float32(lv[1])))
        else:
            weak.append({"nodes": [dict(split(nodes[k + j]), left=nodes[k + j].left, right=nodes[k + j].right) for j in range(nn)],
                         "leaves": lv.copy()})
        k += nn
    return np.float32(thr.value), weak


# ---- the transcript (stdout of the reference's tool) -----------------------------------------------------------------

def parameters_lines(*, data_dir, vec_name, bg_name, num_pos, num_neg, num_stages, params: TrainParams, n_features,
                     precalc_val_buf_size=1024, precalc_idx_buf_size=1024, acceptance_ratio_break_value=-1.0):
    """The PARAMETERS: block (cascadeclassifier.cpp:188-201 with the printAttrs of cascadeclassifier.cpp:99-105,
    boost.cpp:111-124 and haarfeatures.cpp:61-68; LBP and HOG parameters print nothing)."""
    g = T.format_number
    out = ["PARAMETERS:", "cascadeDirName: %s" % data_dir, "vecFileName: %s" % vec_name, "bgFileName: %s" % bg_name,
           "numPos: %d" % num_pos, "numNeg: %d" % num_neg, "numStages: %d" % num_stages,
           "precalcValBufSize[Mb] : %d" % precalc_val_buf_size, "precalcIdxBufSize[Mb] : %d" % precalc_idx_buf_size,
           "acceptanceRatioBreakValue : %s" % g(acceptance_ratio_break_value),
           "stageType: BOOST", "featureType: %s" % _name_of(FEATURE_NAMES, params.feature_type),
           "sampleWidth: %d" % params.win_w, "sampleHeight: %d" % params.win_h,
           "boostType: %s" % _name_of(BOOST_NAMES, params.boost_type), "minHitRate: %s" % g(params.min_hit_rate),
           "maxFalseAlarmRate: %s" % g(params.max_false_alarm), "weightTrimRate: %s" % g(params.weight_trim_rate),
           "maxDepth: %d" % params.max_depth, "maxWeakCount: %d" % params.max_weak_count]
    if params.feature_type == HAAR:
        out.append("mode: %s" % _name_of(MODE_NAMES, params.haar_mode))
    out.append("Number of unique features given windowSize [%d,%d] : %d" % (params.win_w, params.win_h, n_features))
    return out


def transcript(*, data_dir, vec_name, bg_name, num_pos, num_neg, num_stages, params: TrainParams, n_features, n_loaded=0, records=(),
               end=T.END_NUM_STAGES, preloaded=False, precalc_val_buf_size=1024, precalc_idx_buf_size=1024,
               acceptance_ratio_break_value=-1.0, precalc_seconds=0, seconds=0):
    """Every line a run prints on stdout, from what it was given and what it returned: the banner when the parameters came
    from params.xml, the PARAMETERS block, the loaded stages, per iteration the lines train_cascade logs, and the closing
    line of a run that trained nothing. The two lines that tell time take precalc_seconds and seconds. Pure: no device."""
    out = list(BANNER) if preloaded else []
    out += parameters_lines(data_dir=data_dir, vec_name=vec_name, bg_name=bg_name, num_pos=num_pos, num_neg=num_neg, num_stages=num_stages,
                            params=params, n_features=n_features, precalc_val_buf_size=precalc_val_buf_size,
                            precalc_idx_buf_size=precalc_idx_buf_size, acceptance_ratio_break_value=acceptance_ratio_break_value)
    out += T.loaded_lines(n_loaded)
    for k, rec in enumerate(records):
        out += T.stage_begin_lines(n_loaded + k) + T.fill_lines(rec)
        if rec["weak"] is not None:
            out += T.boost_lines(rec["weak"], precalc_seconds) + [T.time_line(seconds)]
        elif end in T.END_MESSAGES:
            out.append(T.END_MESSAGES[end])
        else:  # the stage could not be trained: no round reached isErrDesired
            out += T.boost_lines([], precalc_seconds)
    if n_loaded == 0 and not any(rec["weak"] is not None for rec in records):
        out.append(NOT_TRAINED_MESSAGE)
    return out


# ---- the data directory ----------------------------------------------------------------------------------------------

def _replace_into(path, write):
    """write(tmp) to a temporary name beside `path`, then move it into place: a killed run never leaves half a file."""
    tmp = path + ".tmp"
    write(tmp)
    os.replace(tmp, path)


def _stage_path(data_dir, i):
    return os.path.join(data_dir, "stage%d.xml" % i)


def _note(text):
    print("traincascade: " + text, file=sys.stderr)


def _load_stages(data_dir, params, num_stages, device):
    """stage0.xml, stage1.xml, ... while they exist, at most num_stages (cascadeclassifier.cpp:547-562). A file that exists
    and does not parse, or names a variable outside the catalog, is an error that names it."""
    stages = []
    win = (params.win_w, params.win_h)
    while len(stages) < num_stages and os.path.exists(_stage_path(data_dir, len(stages))):
        path = _stage_path(data_dir, len(stages))
        stage = read_stage(path, params.feature_type)
        try:  # the catalog is the builder's: it refuses a variable it does not hold
            CascadeClassifier.from_trees(params.feature_type, win, [stage], haar_mode=params.haar_mode, device=device)
        except L.CascadeError as err:
            raise L.CascadeError(err.status, "%s: %s" % (path, err)) from None
        stages.append(stage)
    return stages


def _restored_reader(data_dir, backgrounds, win, n_loaded):
    """The reader behind n_loaded stages from resume.json, or a fresh one -- the reference's reader -- with a note on stderr."""
    reader = T.BackgroundReader(backgrounds, win)
    path = os.path.join(data_dir, RESUME_FILENAME)
    try:
        saved = json.load(open(path))
        if not isinstance(saved, dict):
            raise ValueError("not an object")
    except FileNotFoundError:
        saved, why = {}, "%s is missing" % path
    except (OSError, ValueError) as err:
        saved, why = {}, "%s does not read (%s)" % (path, err)
    else:
        why = None
        if saved.get("backgrounds") != len(reader.images) or list(saved.get("window") or []) != list(win):
            why = "%s was written for another background list or window" % path
        elif str(n_loaded) not in saved:
            why = "%s has no entry for %d stages" % (path, n_loaded)
        else:
            try:
                reader.restore(saved[str(n_loaded)])
            except ValueError as err:
                why = str(err)
    if why is not None:
        _note("%s: the background reader starts at the first image, as the reference's does; the run does not continue the "
              "interrupted one exactly" % why)
        return T.BackgroundReader(backgrounds, win), {}
    return reader, {k: v for k, v in saved.items() if k.isdigit() and int(k) <= n_loaded}


def train_cascade_dir(data_dir, positives, backgrounds, num_pos, num_neg, num_stages, *, feature_type=HAAR, win=(24, 24), haar_mode=BASIC,
                      boost_type=BOOST_GENTLE, min_hit_rate=0.995, max_false_alarm=0.5, weight_trim_rate=0.95, max_weak_count=100,
                      max_depth=1, acceptance_ratio_break_value=-1.0, base_format_save=False, device=0, max_batch=256,
                      table_budget_bytes=None, on_stage=None, log=None, vec_name="", bg_name="", precalc_val_buf_size=1024,
                      precalc_idx_buf_size=1024):
    """CvCascadeClassifier::train with its data directory. Returns (cascade or None, stages loaded, records of this call, end
    reason); the arguments are train_cascade's.

    Start: data_dir is created when missing. A params.xml in it replaces the parameters given (the reference's banner says
    so), and stage0.xml, stage1.xml, ... are then read while they exist, at most num_stages; a stage file that does not
    parse is an error (the reference trains that stage again without a word). Stage files without params.xml are ignored
    and overwritten. resume.json restores the background reader behind the loaded stages, so the run continues the
    interrupted one exactly; without a usable entry the reader starts afresh, as the reference's does, with a note on stderr.
    Per trained stage, in this order: resume.json, params.xml (after stage 0), stage<i>.xml, each through a temporary name
    and os.replace; then on_stage. End: cascade.xml with the parameters, or with base_format_save the legacy layout (Haar
    only: anything else fails before a file is touched). With no stage at all nothing is written and the cascade is None.
    log gets stdout's lines (default: print); vec_name, bg_name and the two buffer sizes are only printed."""
    say = log if log is not None else (lambda line: print(line, flush=True))
    params = TrainParams(feature_type, int(win[0]), int(win[1]), boost_type, min_hit_rate, max_false_alarm, weight_trim_rate, max_depth,
                         max_weak_count, haar_mode=haar_mode)
    ppath = os.path.join(data_dir, PARAMS_FILENAME)
    preloaded = os.path.exists(ppath)
    if preloaded:
        params = read_params(ppath)
        if params is None:
            raise L.CascadeError(L.CC_ERR_PARSE, "%s holds no training parameters" % ppath)
    if params.boost_type == BOOST_LOGIT:
        raise L.CascadeError(L.CC_ERR_UNSUPPORTED, LOGIT_MESSAGE)
    if base_format_save and params.feature_type != HAAR:
        raise L.CascadeError(L.CC_ERR_UNSUPPORTED, BASE_FORMAT_MESSAGE)
    win = (params.win_w, params.win_h)
    os.makedirs(data_dir, exist_ok=True)
    if preloaded:
        for line in BANNER:
            say(line)
        initial = _load_stages(data_dir, params, num_stages, device)
    else:
        initial = []
        if os.path.exists(_stage_path(data_dir, 0)):
            _note("%s holds stage files but no %s: they are ignored and will be overwritten" % (data_dir, PARAMS_FILENAME))
    probe = CvFeatureEvaluator.create(params.feature_type, device)
    probe.init(CvFeatureParams(params.feature_type, params.haar_mode), 1, win)
    n_features = probe.getNumFeatures()
    probe._release()
    for line in parameters_lines(data_dir=data_dir, vec_name=vec_name, bg_name=bg_name, num_pos=num_pos, num_neg=num_neg, num_stages=num_stages,
                                 params=params, n_features=n_features, precalc_val_buf_size=precalc_val_buf_size,
                                 precalc_idx_buf_size=precalc_idx_buf_size, acceptance_ratio_break_value=acceptance_ratio_break_value):
        say(line)
    if initial:
        reader, states = _restored_reader(data_dir, backgrounds, win, len(initial))
    else:
        reader, states = T.BackgroundReader(backgrounds, win), {}
    states.update(backgrounds=len(reader.images), window=list(win))

    def save_stage(i, record, cascade):
        state = reader.state()
        states[str(i + 1)] = dict(state, offset=list(state["offset"]))
        _replace_into(os.path.join(data_dir, RESUME_FILENAME), lambda tmp: json.dump(states, open(tmp, "w"), indent=1, sort_keys=True))
        if i == 0:
            _replace_into(ppath, lambda tmp: write_params(tmp, params, "params"))
        _replace_into(_stage_path(data_dir, i), lambda tmp: write_stage(tmp, (record["weak"][-1]["stage_threshold"], record["weak"]),
                                                                       params.feature_type, "stage%d" % i))
        if on_stage is not None:
            on_stage(i, record, cascade)

    cascade, records, end = T.train_cascade(positives, backgrounds, num_pos, num_neg, num_stages, feature_type=params.feature_type, win=win,
                                            haar_mode=params.haar_mode, boost_type=params.boost_type, min_hit_rate=params.min_hit_rate,
                                            max_false_alarm=params.max_false_alarm, weight_trim_rate=params.weight_trim_rate,
                                            max_weak_count=params.max_weak_count, max_depth=params.max_depth,
                                            acceptance_ratio_break_value=acceptance_ratio_break_value, device=device, max_batch=max_batch,
                                            on_stage=save_stage, table_budget_bytes=table_budget_bytes, initial_stages=initial, reader=reader,
                                            log=say)
    if cascade is None:
        say(NOT_TRAINED_MESSAGE)
        return None, len(initial), records, end
    cpath = os.path.join(data_dir, CASCADE_FILENAME)
    if base_format_save:
        _replace_into(cpath, lambda tmp: cascade.save(tmp, baseFormat=True))
    else:
        _replace_into(cpath, lambda tmp: cascade.save(tmp, params=params))
    return cascade, len(initial), records, end


# ---- the command line ------------------------------------------------------------------------------------------------

def parse_args(argv=None):
    """The flags of traincascade.cpp:44-51, :64-149 and the three scanAttrs (cascadeclassifier.cpp:107-133, boost.cpp:126-163,
    haarfeatures.cpp:70-85) with their defaults. -h is the sample height, --help the usage. The three rates pass through
    float, as the reference's (float) atof does. An unknown flag or value ends with status 2; the reference skips it."""
    import argparse
    ap = argparse.ArgumentParser(prog="python -m cascadeclassifier_amd.traincascade", add_help=False, allow_abbrev=False,
                                 description="traincascade: train a boosted cascade of HAAR, LBP or HOG features on the device, "
                                             "with the reference tool's data directory; a directory that holds finished stages "
                                             "is continued")
    ap.add_argument("--help", action="help")
    ap.add_argument("-data", required=True)
    ap.add_argument("-vec", required=True)
    ap.add_argument("-bg", required=True)
    ap.add_argument("-numPos", type=int, default=2000)
    ap.add_argument("-numNeg", type=int, default=1000)
    ap.add_argument("-numStages", type=int, default=20)
    ap.add_argument("-precalcValBufSize", type=int, default=None)
    ap.add_argument("-precalcIdxBufSize", type=int, default=None)
    ap.add_argument("-baseFormatSave", action="store_true")
    ap.add_argument("-numThreads", type=int, default=None)  # accepted and ignored: the work runs on the device
    ap.add_argument("-acceptanceRatioBreakValue", type=float, default=-1.0)
    ap.add_argument("-stageType", choices=["BOOST"], default="BOOST")
    ap.add_argument("-featureType", choices=sorted(FEATURE_NAMES), default="HAAR")
    ap.add_argument("-w", type=int, default=24)
    ap.add_argument("-h", type=int, default=24)
    ap.add_argument("-bt", choices=sorted(BOOST_NAMES), default="GAB")
    ap.add_argument("-minHitRate", type=lambda s: _f32(float(s)), default=_f32(0.995))
    ap.add_argument("-maxFalseAlarmRate", type=lambda s: _f32(float(s)), default=_f32(0.5))
    ap.add_argument("-weightTrimRate", type=lambda s: _f32(float(s)), default=0.95)
    ap.add_argument("-maxDepth", type=int, default=1)
    ap.add_argument("-maxWeakCount", type=int, default=100)
    ap.add_argument("-mode", choices=sorted(MODE_NAMES), default="BASIC")
    argv = sys.argv[1:] if argv is None else list(argv)
    known = {s for action in ap._actions for s in action.option_strings}
    for tok in argv:  # argparse would take "-numP" for "-numPos"
        if len(tok) > 1 and tok[0] == "-" and not (tok[1].isdigit() or tok[1] == ".") and tok not in known:
            ap.error("unknown flag %s" % tok)
    a = ap.parse_args(argv)
    # the reference sizes two host caches in MB; here their sum is the presort's one budget, 0 (what is free) when neither is given
    if a.precalcValBufSize is None and a.precalcIdxBufSize is None:
        a.table_budget_bytes = 0
    else:
        a.table_budget_bytes = ((1024 if a.precalcValBufSize is None else a.precalcValBufSize) +
                                (1024 if a.precalcIdxBufSize is None else a.precalcIdxBufSize)) << 20
    a.precalcValBufSize = 1024 if a.precalcValBufSize is None else a.precalcValBufSize
    a.precalcIdxBufSize = 1024 if a.precalcIdxBufSize is None else a.precalcIdxBufSize
    return a


def main(argv=None) -> int:
    a = parse_args(argv)
    try:
        if BOOST_NAMES[a.bt] == BOOST_LOGIT:  # before the data directory is touched
            raise L.CascadeError(L.CC_ERR_UNSUPPORTED, LOGIT_MESSAGE)
        positives = vec_read(a.vec)
        if positives.shape[1] != a.w * a.h:
            raise ValueError("%s holds samples of %d values, -w %d -h %d needs %d" % (a.vec, positives.shape[1], a.w, a.h, a.w * a.h))
        cascade, _, _, _ = train_cascade_dir(
            a.data, positives.reshape(-1, a.h, a.w), read_background_list(a.bg), a.numPos, a.numNeg, a.numStages,
            feature_type=FEATURE_NAMES[a.featureType], win=(a.w, a.h), haar_mode=MODE_NAMES[a.mode], boost_type=BOOST_NAMES[a.bt],
            min_hit_rate=a.minHitRate, max_false_alarm=a.maxFalseAlarmRate, weight_trim_rate=a.weightTrimRate, max_weak_count=a.maxWeakCount,
            max_depth=a.maxDepth, acceptance_ratio_break_value=a.acceptanceRatioBreakValue, base_format_save=a.baseFormatSave,
            table_budget_bytes=a.table_budget_bytes, vec_name=a.vec, bg_name=a.bg, precalc_val_buf_size=a.precalcValBufSize,
            precalc_idx_buf_size=a.precalcIdxBufSize)
    except Exception as err:  # the reference ends with an uncaught cv::Exception here
        print("traincascade: %s" % err, file=sys.stderr)
        return 1
    return 0 if cascade is not None else 1


if __name__ == "__main__":
    sys.exit(main())
