"""Witness of one boosted stage of weak trees: tests/boost_witness.py with a tree of up to max_depth levels of splits where
that one grows a stump. Three things are added, each restated from the reference's lines in plain Python:

  - the recursion of CvDTree::try_split_node (o_cvdtree.cpp:122-187) with its leaf rules and CvBoostTree::try_split_node's
    weak_eval of an unsplit node's samples (o_cvboostree.cpp:71-85);
  - the children's sample lists, which keep increasing sample order (split_node_data, o_cvcascadeboosttree.cpp:300-338);
  - the numbering of internal nodes and leaves by CvCascadeBoostTree::write (o_cvcascadeboosttree.cpp:41-93).

The split of a node still comes from oracle.find_best_split on the node's columns, and `exp` stays a parameter."""
import math

import numpy as np

from oracle import oracle as orc
from tests import boost_witness as bw
from tests.boost_witness import DISCRETE, F32, FLT_EPSILON

MIN_SAMPLE_COUNT = 10  # o_cvdtreeparams.cpp:8
REGRESSION_ACCURACY = float(F32(0.01))  # o_cvdtreeparams.cpp:9
LEAF_MIN_SAMPLES, LEAF_DEPTH, LEAF_PURE, LEAF_NO_SPLIT = "sample_count <= 10", "depth >= max_depth", "pure / regression accuracy", "no split"

NODE_FIELDS = ("left", "right", "depth", "n_samples", "var_idx", "split_point", "quality", "ord_c", "value")


class TreeWitness(bw.BoostWitness):
    def __init__(self, vals, labels, max_depth=1, **params):
        super().__init__(vals, labels, **params)
        if max_depth < 1:
            raise ValueError("max_depth >= 1")
        self.max_depth = min(int(max_depth), 25)  # o_cvdtreetraindata.cpp:105
        self.roots = []  # the root of every trained round's tree

    # ---- CvDTree::try_split_node ------------------------------------------------------------------------------
    def _new_node(self, idx, depth):
        value, rcw, _, risk, cnt = self._node_value(idx)
        return {"idx": idx, "depth": depth, "value": value, "rcw": rcw, "risk": risk, "cnt": cnt, "left": None, "right": None, "leaf": None,
                "var_idx": -1, "split_point": -1, "quality": F32(-1), "ord_c": F32(0), "subset": np.zeros(8, np.int32)}

    def _leaf_rule(self, node):
        """o_cvdtree.cpp:130-145: the reason the node is not searched, or None."""
        n = len(node["idx"])
        if n <= MIN_SAMPLE_COUNT:
            return LEAF_MIN_SAMPLES
        if node["depth"] >= self.max_depth:
            return LEAF_DEPTH
        if self.classifier:
            if (node["cnt"][0] != 0) + (node["cnt"][1] != 0) == 1:
                return LEAF_PURE
        elif node["risk"] >= 0 and math.sqrt(node["risk"]) / n < REGRESSION_ACCURACY:
            return LEAF_PURE
        return None

    def _find_split(self, node):
        idx, w = node["idx"], self.weights
        W = np.array([w[i] for i in idx] + [node["rcw"][0], node["rcw"][1]], np.float64)
        sub = self.vals[:, idx]
        if self.classifier:
            kind = {"class_labels": np.array([self.labels[i] for i in idx], np.int32)}
        else:
            kind = {"responses": np.array([F32(self.y[i]) for i in idx], np.float32)}
        return sub, orc.find_best_split(sub, W, categorical=self.categorical, node_value=node["value"], boost_type=self.boost_type,
                                        split_criteria=self.split_criteria, **kind)

    def _try_split_node(self, node):
        idx = node["idx"]
        node["leaf"] = self._leaf_rule(node)
        if node["leaf"] is None:
            sub, sp = self._find_split(node)
            if not sp["found"]:
                node["leaf"] = LEAF_NO_SPLIT
        if node["leaf"] is not None:
            for i in idx:  # o_cvboostree.cpp:74-84
                self.weak_eval[i] = node["value"]
                self.leaf_of[i] = node
            return
        var = int(sp["var_idx"])
        node["var_idx"], node["quality"] = self.var0 + var, F32(sp["quality"])
        # calc_node_dir (o_cvboostree.cpp:87-149)
        left = {}
        if self.categorical:
            node["subset"] = np.array(sp["subset"], np.int32)
            for i in idx:
                c = int(self.vals[var][i])
                left[i] = bool((int(node["subset"][c >> 5]) >> (c & 31)) & 1)
        else:
            node["ord_c"], node["split_point"] = F32(sp["ord_c"]), int(sp["split_point"])
            order = np.argsort(sub[var], kind="stable")  # the presorted order restricted to the node; ties by sample index
            for rank, k in enumerate(order):
                left[idx[int(k)]] = rank <= node["split_point"]
        # split_node_data: the children's samples in the parent's (increasing) order; calc_node_value of each
        node["left"] = self._new_node([i for i in idx if left[i]], node["depth"] + 1)
        node["right"] = self._new_node([i for i in idx if not left[i]], node["depth"] + 1)
        self._try_split_node(node["left"])
        self._try_split_node(node["right"])

    # ---- CvCascadeBoostTree::predict (o_cvcascadeboosttree.cpp:16-39) ---------------------------------------------------
    def _predict(self, root, i):
        node = root
        while node["left"] is not None:
            node = node["left"] if self._left_by_predict(i, node) else node["right"]
        return node

    def round(self):
        n, w, y = self.n, self.weights, self.y
        rec = {"trained": False, "stop": 4, "var_idx": -1, "split_point": -1, "quality": F32(-1), "ord_c": F32(0), "subset": np.zeros(8, np.int32),
               "left_value": 0.0, "right_value": 0.0, "stage_threshold": self.threshold, "hit_rate": self.hit_rate, "false_alarm": self.false_alarm}
        active = [i for i in range(n) if self.mask[i]]  # cvPreprocessIndexArray of the mask: increasing sample order
        rec["n_active"] = len(active)
        if not active:
            return rec
        root = self._new_node(active, 0)
        if self._leaf_rule(root) is not None:  # no tree (o_cvdtree.cpp:106, boost.cpp:436-440): nothing changes
            return rec
        saved = list(self.weak_eval)
        self.leaf_of = {}
        self._try_split_node(root)
        if root["left"] is None:
            self.weak_eval = saved
            return rec
        rec.update(trained=True, **{k: root[k] for k in ("var_idx", "quality", "ord_c", "split_point", "subset")})
        # update_weights(tree) (boost.cpp:266-406)
        we = self.weak_eval
        if self.have_subsample:
            for i in range(n):
                if not self.mask[i]:
                    we[i] = self._predict(root, i)["value"]
        sum_w = 0.0
        if self.boost_type == DISCRETE:
            err = 0.0
            for i in range(n):
                sum_w += w[i]
                err += w[i] * (1 if we[i] != y[i] else 0)
            if sum_w != 0:
                err /= sum_w
            scale_c = err = -bw.log_ratio(err)
            scale = [1., math.exp(err)]
            sum_w = 0.0
            for i in range(n):
                w[i] = w[i] * scale[1 if we[i] != y[i] else 0]
                sum_w += w[i]
            for node in all_nodes(root):  # tree->scale(C)
                node["value"] *= scale_c
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
        rec["left_value"], rec["right_value"] = root["left"]["value"], root["right"]["value"]
        if self.max_depth > 1:
            rec["nodes"], rec["leaves"] = writer_layout(root)
        self.roots.append(root)
        self.n_weak += 1
        # stage sums: predict(i)->value of the new tree (boost.cpp:461-473)
        for i in range(n):
            self.stage_sum[i] += self._predict(root, i)["value"]
        # trim_weights
        if 0. < self.rate < 1.:
            m, _ = bw.trim_walk(w, self.rate)
            self.mask = [int(v) for v in m]
            self.have_subsample = sum(self.mask) < n
        if sum(self.mask) == 0:  # boost.cpp:444
            rec["stop"] = 3
            return rec
        self.threshold, self.hit_rate, self.false_alarm, done = bw.is_err_desired(self.stage_sum, self.labels, self.min_hit_rate, self.max_false_alarm)
        rec.update(stage_threshold=self.threshold, hit_rate=self.hit_rate, false_alarm=self.false_alarm)
        rec["stop"] = 1 if done else (2 if self.n_weak >= self.max_weak_count else 0)
        return rec


def all_nodes(root):
    out, todo = [], [root]
    while todo:
        node = todo.pop()
        out.append(node)
        if node["left"] is not None:
            todo += [node["right"], node["left"]]
    return out


def writer_layout(root):
    """CvCascadeBoostTree::write (o_cvcascadeboosttree.cpp:41-93): the internal nodes breadth-first from the root; a child
    that splits gets the next internal number when its parent is written, a leaf the next leaf number (0, -1, ...)."""
    queue, nodes, leaves = [root], [], []
    next_node = 1
    for node in queue:  # grows while it is walked
        refs = []
        for child in (node["left"], node["right"]):
            if child["left"] is None:
                refs.append(-len(leaves))
                leaves.append(child["value"])
            else:
                queue.append(child)
                refs.append(next_node)
                next_node += 1
        nodes.append({"left": refs[0], "right": refs[1], "depth": node["depth"], "n_samples": len(node["idx"]), "var_idx": node["var_idx"],
                      "split_point": node["split_point"], "quality": node["quality"], "ord_c": node["ord_c"], "subset": node["subset"],
                      "value": node["value"]})
    return nodes, np.array(leaves, np.float64)


def assert_tree_equal(got, want, where):
    """Every node and every leaf of a trained record, tolerance 0.0."""
    assert len(got["nodes"]) == len(want["nodes"]), (where, "n_nodes", len(got["nodes"]), len(want["nodes"]))
    for k, (g, x) in enumerate(zip(got["nodes"], want["nodes"])):
        for f in NODE_FIELDS:
            assert g[f] == x[f], (where, "node", k, f, g[f], x[f])
        assert (np.asarray(g["subset"]) == np.asarray(x["subset"])).all(), (where, "node", k, "subset")
    assert (np.asarray(got["leaves"]) == np.asarray(want["leaves"])).all(), (where, "leaves", got["leaves"], want["leaves"])
