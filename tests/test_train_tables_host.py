"""Host-only parts of csrc/cc_train_device.h under AddressSanitizer + UBSan: tests/cpp/train_tables_host.cpp, a stand-alone
program (own main, no device call) that builds the plain-offset catalogs and the node records of k_predict and checks every
offset and child index. CPU only."""
import os
import subprocess

import numpy as np

from tests import cascade_factory as cf
from tests.host_build import build_program
from tests.util import frame_natural, truncated_cascade


def test_train_tables_host_program_runs_clean(tmp_path, haar_xml, lbp_xml):
    exe = build_program("train_tables_host", tmp_path, hip_host_only=True)
    img = frame_natural(320, 240, 3)
    wins = np.stack([img[y:y + 24, x:x + 24] for y in range(0, 200, 9) for x in range(0, 280, 11)])
    made = {"haar_trees.xml": cf.haar_tree_cascade(wins, with_tilted=True), "lbp_trees.xml": cf.lbp_tree_cascade(),
            "haar_tilted.xml": cf.tilted_stump_cascade(wins)}
    paths = [haar_xml, lbp_xml, truncated_cascade(haar_xml, 9, str(tmp_path))]
    for name, xml in made.items():
        paths.append(os.path.join(str(tmp_path), name))
        open(paths[-1], "w").write(xml)
    r = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-2000:], r.stderr[-3000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr
    # The miner's own predicate (stage_sums_order_independent, as mine_begin calls it) on the cascade of the haar9 cases of
    # tests/test_gpu_negmine.py: it takes the wave walk, and its widest stage gives lanes a second stump.
    haar9 = [l for l in r.stdout.splitlines() if l.startswith(paths[2] + ":")]
    assert len(haar9) == 1 and "9 stages" in haar9[0] and "widest stage 83," in haar9[0] and haar9[0].endswith("wave walk 1"), haar9
