"""HOG training end to end: the inputs of tests/test_gpu_train_cascade_hog.py and a witness of CvCascadeClassifier::train
(cascadeclassifier.cpp:203-284, :308-357) in which the library decides nothing:

* the window stream comes from fill_witness.NegReaderWitness (the order) and hog_mine_cases.reader_stream (the pixels);
* every value from hog_restatement.set_images + eval_vars over hog_restatement.catalog(W, H);
* the stage walk from hog_cascade_factory.stage_walk: float32 leaves and thresholds, double sums in tree order, stage
  threshold (float)t - 1e-5f;
* a stage from boost_witness.BoostWitness (max_depth 1) or tree_witness.TreeWitness on those values, ordered variables; the
  vector exponential is a parameter (libm's on the host, the device's in the GPU test).

tests/test_train_cascade_hog_host.py runs the witness with libm's exp and asserts what makes the inputs worth training on."""
import math

import numpy as np

from cascadeclassifier_amd.trainer import END_CANNOT_FILL, END_LEAF_FA_RATE, END_NUM_STAGES, END_STAGE_NOT_TRAINED
from tests import boost_witness as bw
from tests import fill_witness as fw
from tests import hog_cascade_factory as hf
from tests import hog_mine_cases as mc
from tests import hog_restatement as hog
from tests import tree_witness as tw
from tests.util import frame_natural

NUM_POS = NUM_NEG = 60
NUM_STAGES = 3
PARAMS = dict(boost_type=bw.GENTLE, min_hit_rate=0.995, max_false_alarm=0.5, weight_trim_rate=0.95, max_weak_count=4)
# (window, max_depth, stripe amplitude of the positives). At 32x24 amplitude 30 is separated by the first stage's stumps and
# the second stage finds nothing to fill with; 22 trains three stages.
CASES = [((24, 24), 1, 30), ((24, 24), 2, 30), ((32, 24), 1, 22)]


def case_id(case):
    return "%dx%d_depth%d" % (case[0] + (case[1],))


def positives(win, amplitude, n=80, seed=17):
    """Crops of a natural frame with diagonal stripes over the middle three quarters of the width and noise of sigma 6.
    Fainter patterns (the Haar / LBP tests' recipe) leave HOG stumps nothing to reject in three rounds; stripes over the
    whole window at amplitude 60 are separated by one stump and training ends after the first stage."""
    W, H = win
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    pattern = np.where(np.abs(xx - W / 2) < 0.375 * W, amplitude * np.sign(np.sin((xx + yy) / 24 * 9)), 0.0)
    frame = frame_natural(400, 300, seed).astype(np.float64)
    out = []
    for _ in range(n):
        x, y = int(rng.integers(0, 400 - W)), int(rng.integers(0, 300 - H))
        out.append(np.clip(frame[y:y + H, x:x + W] + pattern + rng.normal(0, 6, (H, W)), 0, 255))
    return np.stack(out).astype(np.uint8)


def backgrounds():
    return [frame_natural(176, 132, 31), frame_natural(120, 100, 32), frame_natural(176, 132, 33), frame_natural(120, 100, 34)]


def all_values(windows, cat):
    """values[variable][window] of every catalog variable."""
    return hog.eval_vars(cat, *hog.set_images(windows))


def model_of(stages):
    """The stages of weak records as hog_cascade_factory's walk takes them; a node's feature index is its variable."""
    out = []
    for thr, weak in stages:
        weaks = []
        for w in (w for w in weak if w["trained"]):
            if "nodes" in w:
                weaks.append(([(nd["left"], nd["right"], nd["var_idx"], nd["ord_c"]) for nd in w["nodes"]], list(w["leaves"])))
            else:
                weaks.append(([(0, -1, w["var_idx"], w["ord_c"])], [w["left_value"], w["right_value"]]))
        out.append((thr, weaks))
    return hf.parsed_model(out)


def witness_train(pos, bgs, win, max_depth, exp, num_pos=NUM_POS, num_neg=NUM_NEG, num_stages=NUM_STAGES, params=PARAMS):
    """Returns (stages, records, end reason, notes): stages as from_stumps / from_trees take them; a note per stage says how
    many images its negatives came from and whether it resumed in the middle of one."""
    W, H = win
    cat = hog.catalog(W, H)
    reader = fw.NegReaderWitness(bgs, win)
    required = math.pow(float(np.float32(params["max_false_alarm"])), float(num_stages)) / float(max_depth)  # :209-210
    pos_vals = all_values(pos, cat)
    stages, records, notes = [], [], []
    images, flags_of = {}, {}

    def windows_of(idx, off):  # values of every window of the image's stream, and their flags under the stages so far
        if (idx, off) not in images:
            images[(idx, off)] = all_values(mc.reader_stream(bgs[idx], W, H, off[0], off[1])[1], cat)
        key = (len(stages), idx, off)
        if key not in flags_of:
            vals = images[(idx, off)]
            flags_of[key] = hf.stage_walk(model_of(stages), vals) if stages else np.ones(vals.shape[1], np.uint8)
        return flags_of[key], images[(idx, off)]

    end = END_NUM_STAGES
    for _ in range(num_stages):
        flags = hf.stage_walk(model_of(stages), pos_vals) if stages else np.ones(len(pos), np.uint8)
        pos_count, pos_consumed, _, keep = fw.fill_select(flags, 0, num_pos)
        if pos_count < num_pos:
            raise ValueError("Can not get new positive sample. vec-file is over.")
        pro_num_neg = int(round((float(num_neg) * float(pos_count)) / num_pos))
        note = {"resumed_mid_image": reader.img is not None and reader.i != 0, "images": 0}
        got, consumed, neg, last_image = 0, 0, [], None
        for _ in range(pro_num_neg):  # fillPassedSamples, :329-357
            by_ratio = False
            while True:
                if consumed != 0 and float(got + 1) / float(consumed) <= required:
                    by_ratio = True
                    break
                idx, off, wi, _, _ = reader.get()
                consumed += 1
                if (idx, off) != last_image or wi == 0:
                    note["images"] += 1
                    last_image = (idx, off)
                f, vals = windows_of(idx, off)
                if f[wi]:
                    neg.append(vals[:, wi])
                    got += 1
                    break
            if by_ratio:
                break
        notes.append(note)
        record = {"pos_count": pos_count, "pos_consumed": pos_consumed, "neg_count": got, "neg_consumed": consumed, "acceptance_ratio": None,
                  "weak": None}
        records.append(record)
        if got == 0 and not (consumed > 0 and (float(got) + 1) / float(consumed) <= required):
            end = END_CANNOT_FILL
            break
        record["acceptance_ratio"] = 0.0 if consumed == 0 else float(got) / float(consumed)
        if record["acceptance_ratio"] <= required:
            end = END_LEAF_FA_RATE
            break
        vals = np.concatenate([pos_vals[:, keep], np.stack(neg, axis=1)], axis=1)
        labels = np.array([1] * pos_count + [0] * got, np.uint8)
        if max_depth == 1:
            wit = bw.BoostWitness(vals, labels, categorical=False, exp=exp, **params)
        else:
            wit = tw.TreeWitness(vals, labels, max_depth=max_depth, categorical=False, exp=exp, **params)
        weak = []
        while not weak or weak[-1]["stop"] == 0:
            weak.append(wit.round())
        if not any(w["trained"] for w in weak):
            end = END_STAGE_NOT_TRAINED
            break
        record["weak"] = weak
        stages.append((weak[-1]["stage_threshold"], weak))
    return stages, records, end, notes


def saved_text(cascade):
    """What cascade.save writes."""
    import os
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cascade.xml")
        cascade.save(path)
        return open(path).read()


def assert_xml_is_the_witness(text, win, stages):
    """The saved cascade against the witness's records, without the library: every node's <rect> is catalog[var_idx // 36]
    followed by var_idx % 36, the <features> list holds each used variable once, thresholds and leaves are the float32
    values of the records."""
    f32 = np.float32
    W, H, feats, parsed = hf.parse_hog_xml(text)
    assert (W, H) == tuple(win) and len(parsed) == len(stages)
    cat = hog.catalog(W, H)
    used = set()
    for s, ((thr, weaks), (w_thr, w_weak)) in enumerate(zip(parsed, stages)):
        assert thr == f32(w_thr), (s, thr, w_thr)
        trained = [w for w in w_weak if w["trained"]]
        assert len(weaks) == len(trained), s
        for k, ((nodes, leaves), w) in enumerate(zip(weaks, trained)):
            if "nodes" in w:
                want_nodes = [(nd["left"], nd["right"], nd["var_idx"], nd["ord_c"]) for nd in w["nodes"]]
                want_leaves = list(w["leaves"])
            else:
                want_nodes, want_leaves = [(0, -1, w["var_idx"], w["ord_c"])], [w["left_value"], w["right_value"]]
            assert len(nodes) == len(want_nodes) and len(leaves) == len(want_leaves), (s, k)
            for (l, r, fi, t), (wl, wr, var, wt) in zip(nodes, want_nodes):
                assert (l, r) == (wl, wr), (s, k)
                assert tuple(feats[fi]) == tuple(int(v) for v in cat[var // 36]) + (var % 36,), (s, k, feats[fi], var)
                assert t == f32(wt), (s, k, t, wt)
                used.add(var)
            assert [f32(v) for v in leaves] == [f32(v) for v in want_leaves], (s, k)
    rects = [tuple(int(v) for v in f) for f in feats]
    assert len(set(rects)) == len(rects) == len(used)


def assert_worth_training(records, notes):
    """At least two stages are trained; some stage rejects windows, some stage draws from more than one image, some stage
    after the first resumes in the middle of an image."""
    summary = [(r["neg_count"], r["neg_consumed"], None if r["weak"] is None else len(r["weak"])) for r in records]
    assert sum(r["weak"] is not None for r in records) >= 2, summary
    assert any(r["neg_consumed"] > r["neg_count"] > 0 for r in records), summary
    assert any(n["images"] > 1 for n in notes), notes
    assert any(n["resumed_mid_image"] for n in notes[1:]), notes
