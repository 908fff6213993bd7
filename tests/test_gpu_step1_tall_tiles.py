"""Tall tiles of the run-time specialised Haar kernel's STEP-1 module (lean LDS layout: rotated norm-factor rows, queue
tables that grow towards each other with the split phase's partial sums and the wave phase's lists between them; a
wave_below of the module's own): at 12, 16, 20 and 24 window rows per tile every window's result code, exit stage, stage
sum, visited flag and every rectangle equal the CPU oracle's.

One process per height (the height is read from CCAMD_SPEC_TILE_Y1 when the module is built): tests/step1_tall.py is the
worker and says which shapes and cases it runs -- frames whose STEP-1 scales have ny = TILE_Y - 1, TILE_Y, TILE_Y + 1 and
4 k + 3 rows in the last tile, nx = 63, 64, 65 (derived from cc.scale_plan); windows of 24x24, 20x20 and 25x24; two and all
stages compiled; CCAMD_WAVE_BELOW 0 and 64 with CCAMD_SPLIT_STUMPS 0 and 1; a batch of three frames; and a frame of face
templates tiled edge to edge, which leaves hundreds of one tile's windows alive at a table-driven stage."""
import os
import subprocess
import sys

import pytest

from tests import step1_tall as t

pytestmark = pytest.mark.gpu


@pytest.mark.timeout(300)
@pytest.mark.parametrize("rows", t.HEIGHTS)
def test_step1_module_at_every_height(rows, repo_root):
    env = dict(os.environ)
    for k in ("CCAMD_SPEC_TILE_Y", "CCAMD_SPEC_TILE_Y2", "CCAMD_SPEC_ONE_MODULE", "CCAMD_WAVE_BELOW", "CCAMD_WAVE_BELOW1", "CCAMD_SPLIT_STUMPS"):
        env.pop(k, None)
    env["CCAMD_SPEC_TILE_Y1"] = str(rows)
    r = subprocess.run([sys.executable, "-m", "tests.step1_tall", str(rows)], cwd=repo_root, env=env, capture_output=True, text=True, timeout=280)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "STEP1_TALL_OK rows=%d " % rows in r.stdout
