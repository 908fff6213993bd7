"""Inputs shared by the test-mode tests of sample synthesis (tests/test_testset_plan_host.py, tests/test_gpu_testset.py):
background lists, the cases of the plan and the cases of the renderer with what each is there for. The condition a render
case exists for is asserted on the witness on the host (test_render_case_meets_its_condition), so a case cannot stop
covering its edge unnoticed."""
import numpy as np

from tests import sample_witness as W
from tests import testset_witness as TW
from tests.sample_cases import obj_image

# ---- host plan: (window, background sizes, Params kwargs, num, maxscale, seed) ----
# With an automatic maxscale every later image must hold 0.7 of the first one's smaller side: sides 100..140 do.
SIZES_AUTO = [(100 + (7 * i) % 41, 100 + (11 * i) % 41) for i in range(12)]
SIZES_MIXED = [(61, 80), (400, 300), (90, 60), (127, 64), (75, 333), (64, 64), (200, 100), (63, 97)]  # all hold 2.5 x 24
SIZES_WITH_9 = [(9, 50), (120, 110), (50, 9), (101, 131), (9, 9), (140, 100), (10, 9), (111, 117)]  # four are drawn again
PLAN_CASES = {
    "auto": ((24, 24), SIZES_AUTO, {}, 12, -1.0, 12345),
    "auto_20x13": ((20, 13), SIZES_AUTO, {}, 12, -1.0, 12345),
    "maxscale_1": ((24, 24), SIZES_MIXED, {}, 8, 1.0, 12345),
    "maxscale_2.5": ((24, 24), SIZES_MIXED, {}, 8, 2.5, 12345),
    "randinv": ((24, 24), SIZES_MIXED, dict(invert=W.RANDOM_INVERT), 8, 2.5, 12345),
    "seed_0": ((24, 24), SIZES_AUTO, {}, 12, -1.0, 0),
    "seed_past_32_bits": ((24, 24), SIZES_AUTO, {}, 12, -1.0, 2 ** 32 + 7),
    "sides_of_9": ((24, 24), SIZES_WITH_9, {}, 8, 2.0, 12345),
    "num_clamped": ((24, 24), SIZES_MIXED, {}, 50, 2.5, 12345),
}
DRAWS_PER_SAMPLE = 21  # background 1, scale 1, x 2, y 2, quad 8, xshift 2, yshift 2, randscale 2, forecolordev 1

# Sticky skip: at seed 0 the first image drawn is the 14 x 11 one, the automatic maxscale 0.7 * 11 / 24 < 1 stays for the
# whole run and nothing is emitted, though two images would hold the window.
SKIP_SIZES, SKIP_SEED = [(12, 12), (300, 200), (14, 11), (200, 300)], 0
# Refusal: at seed 20 the first image drawn is the 400 x 300 one (maxscale 8.75), the second a 30-pixel one that the
# 24 x 24 window scaled by the draw does not fit into.
REFUSAL_SIZES, REFUSAL_SEED, REFUSAL_ITERATION = [(400, 300), (30, 30), (31, 33), (30, 34)], 20, 2


class CountingRNG(W.RNG):
    def __init__(self, seed=12345):
        super().__init__(seed)
        self.draws = 0

    def next(self):
        self.draws += 1
        return super().next()


# ---- renderer: name -> (object w, h, window, background sizes, Params kwargs, num, maxscale, seed) ----
RENDER_CASES = {
    "rect_256": (40, 24, (16, 16), [(21, 19), (30, 26), (45, 61)], {}, 3, 1.0, 12345),           # exactly one full tile
    "rect_257_row": (40, 24, (257, 1), [(263, 11), (300, 12), (301, 10)], {}, 3, 1.0, 12345),    # one tile and one pixel; a row > 256
    "from_1x1_window": (40, 24, (1, 1), [(10 + i, 13 + (3 * i) % 7) for i in range(16)], {}, 16, 7.99, 12345),  # 1 x 1 .. 7 x 7
    "whole_image": (40, 24, (10, 10), [(10, 10)] * 3, {}, 3, 1.0, 12345),                         # the rectangle is the image
    "odd_widths": (41, 23, (20, 13), [(45, 61), (101, 53), (70, 52), (83, 47), (66, 39)], {}, 5, 2.0, 12345),  # device pitches 48, 104, ...
    "mixed_sizes": (40, 24, (24, 16), [(400, 300), (397, 290), (350, 299), (333, 222), (399, 231), (345, 267)], {}, 6, 12.5, 32),  # 25 x 16 next to 284 x 189
    "same_image_twice": (40, 24, (24, 24), [(70, 52), (61, 66), (90, 55)], {}, 3, 2.0, 12345),     # each copy is fresh
    "randinv": (40, 24, (24, 24), [(70, 52), (61, 66), (90, 55), (64, 64), (81, 49), (77, 77)], dict(invert=W.RANDOM_INVERT), 6, 2.0, 12345),
    "idev_clamps": (40, 24, (24, 24), [(70, 52), (61, 66), (90, 55), (64, 64), (81, 49), (77, 77)], dict(maxintensitydev=255), 6, 2.0, 12345),
    "equal_sizes": (40, 24, (24, 24), [(128, 96)] * 5, {}, 5, -1.0, 12345),                        # for the device-output path
}


def backgrounds(sizes, seed=91):
    r = np.random.RandomState(seed)
    return [r.randint(0, 256, (h, w)).astype(np.uint8) for w, h in sizes]


def render_inputs(name):
    """(object image, background images, Params kwargs) of a RENDER_CASES row."""
    sw, sh, _, sizes, kw, _, _, _ = RENDER_CASES[name]
    return obj_image(sw, sh, 5, kw.get("bgcolor", 0)), backgrounds(sizes), kw


_render_witness_cache = {}


def render_witness(name):
    """(images, samples, maxscale) of the sparse witness for a row (computed once per process; do not modify)."""
    if name not in _render_witness_cache:
        _, _, win, _, kw, num, maxscale, seed = RENDER_CASES[name]
        img, bgs, _ = render_inputs(name)
        images, samples, ms = TW.generate(img, bgs, win[0], win[1], W.Params(**kw), W.RNG(seed), num, maxscale)
        for i in images:
            i.setflags(write=False)
        _render_witness_cache[name] = (images, samples, ms)
    return _render_witness_cache[name]
