"""Tall tiles of the specialised Haar kernel's STEP-1 module, shared by tests/test_step1_tall_tiles_host.py and
tests/test_gpu_step1_tall_tiles.py: the restated LDS request, the frame shapes at the tile edges, and the worker that
tests/test_gpu_step1_tall_tiles.py starts once per tile height (`python -m tests.step1_tall <rows>`; the height is read
from CCAMD_SPEC_TILE_Y1 when a module is built, so every height gets a process of its own).

Shapes. A STEP-1 scale (scale factor above 2) of nx x ny window origins is cut into tiles of 64 x TILE_Y. The rows of a
tile are dealt to the block's four wavefronts, TILE_Y / 4 each (three to six: an odd number at 12 and 20 rows). The frames
below give STEP-1 scales with ny = TILE_Y - 1, TILE_Y and TILE_Y + 1 (a tile short of one row, a full one, a second tile
of one row), 4 k + 3 rows in the last tile (one row more than an odd multiple of a pair of rows: wavefronts with all,
some and none of their rows inside the grid), and nx = 63, 64 and 65 (the tile's column edge). They are found from
cc.scale_plan, not written down."""
import os
import sys

import numpy as np

HEIGHTS = (12, 16, 20, 24)
SCALE_FACTOR = 1.1
TILE_X = 64


# ---- the LDS request, restated (cc_eval_common.h: TileGeom<1>, eval_lds_bytes with lean = true) ----
def tile_words_step1(W, H, rows):
    cols = (TILE_X - 1) + W + 1
    stride = (cols + 3) // 4 * 4
    if stride % 16 == 0:
        stride += 4
    return ((rows - 1) + H + 1) * stride


def lean_lds_bytes(W, H, rows):
    """Integral tile (16-byte multiple) + norm factors float[rows][64] + two queue tables u16[rows * 64] + 3 x 32 counters."""
    tile = (tile_words_step1(W, H, rows) + 3) // 4 * 4 * 4
    return tile + rows * TILE_X * 4 + 2 * rows * TILE_X * 2 + 3 * 32 * 4


def blocks_per_cu(lds_bytes):
    return min(8, (160 * 1024) // lds_bytes)


def default_rows(W, H, want):
    rows = want
    while rows - 4 >= 8 and blocks_per_cu(lean_lds_bytes(W, H, rows)) < 4:
        rows -= 4
    return rows


# ---- frame shapes ----
def step1_grids(W, H, w, h):
    import cascadeclassifier_amd as cc
    sc = cc.scale_plan(W, H, w, h, SCALE_FACTOR)
    return [(int(s["nx"]), int(s["ny"])) for s in sc if s["ystep"] == 1]


def ny_targets(rows):
    return {"short": lambda ny: ny == rows - 1, "full": lambda ny: ny == rows, "plus1": lambda ny: ny == rows + 1,
            "odd_pair": lambda ny: ny % rows % 4 == 3}


def nx_targets():
    return {"nx63": lambda nx: nx == 63, "nx64": lambda nx: nx == 64, "nx65": lambda nx: nx == 65}


def edge_frames(W, H, rows):
    """[(w, h)]: few frames between 150x90 and 220x160 whose STEP-1 scales cover every ny and nx target. A scale's ny depends on
    the frame's height and its nx on the width, so heights and widths are searched on their own and then paired; what the
    paired frames cover is checked again by the caller (covered_targets)."""
    def cover(targets, values_of, candidates):
        chosen, missing = [], dict(targets)
        for c in candidates:
            got = [k for k, f in missing.items() if any(f(v) for v in values_of(c))]
            if got:
                chosen.append(c)
                for k in got:
                    del missing[k]
            if not missing:
                break
        assert not missing, sorted(missing)
        return chosen
    hs = cover(ny_targets(rows), lambda h: [ny for _, ny in step1_grids(W, H, 200, h)], range(90, 161))
    ws = cover(nx_targets(), lambda w: [nx for nx, _ in step1_grids(W, H, w, 120)], range(150, 221))
    return [(ws[i % len(ws)], hs[i % len(hs)]) for i in range(max(len(ws), len(hs)))]


def covered_targets(W, H, rows, frames):
    got = set()
    for (w, h) in frames:
        for nx, ny in step1_grids(W, H, w, h):
            got |= {k for k, f in ny_targets(rows).items() if f(ny)}
            got |= {k for k, f in nx_targets().items() if f(nx)}
    return got


def dense_template_frame(haar_xml):
    """Face templates of 2.2 to 3 window sizes tiled edge to edge: at the STEP-1 scales whole tiles of windows sit on a face
    or next to one, and far more than 24 of a tile's windows are still alive in the late, table-driven stages."""
    from tests.util import frame_natural, upscale
    tm = np.load(os.path.join(os.path.dirname(haar_xml), "face_template_24x24.npy"))
    img = frame_natural(220, 160, 71)
    y = 0
    for s in (53, 60, 47):
        if y + s > 160:
            break
        for x in range(0, 220 - s + 1, s):
            img[y:y + s, x:x + s] = upscale(tm, s)
        y += s
    return img


def late_windows_per_tile(o, img, rows, stage, W=24, H=24):
    """Largest number of windows of one 64 x rows tile of a STEP-1 scale that are still in the cascade when stage `stage`
    starts, by the oracle's result codes."""
    import cascadeclassifier_amd as cc
    from oracle import oracle as orc
    ref = orc.detect_raw(o, img, SCALE_FACTOR, nthreads=8, full=True)
    sc = cc.scale_plan(W, H, img.shape[1], img.shape[0], SCALE_FACTOR)
    most, ofs = 0, 0
    for s in sc:
        nx, ny = int(s["nx"]), int(s["ny"])
        codes = ref.codes[ofs:ofs + nx * ny].reshape(ny, nx)
        ofs += nx * ny
        if s["ystep"] != 1:
            continue
        reached = (codes == 1) | (codes <= -stage)  # passed everything, or rejected by `stage` or a later one
        if stage <= 1:
            reached &= ~((codes == -1) & (ref.sums[ofs - nx * ny:ofs].reshape(ny, nx) == 0.0))
        for ty in range(0, ny, rows):
            for tx in range(0, nx, TILE_X):
                most = max(most, int(reached[ty:ty + rows, tx:tx + TILE_X].sum()))
    return most


# ---- the worker ----
def same_as_oracle(p, o, img, sf=SCALE_FACTOR):
    from oracle import oracle as orc
    ref = orc.detect_raw(o, img, sf, nthreads=8, full=True)
    codes, sums, vis = p.debug_windows(img, sf)
    bad = np.nonzero(codes != ref.codes)[0]
    assert len(bad) == 0, f"{len(bad)} of {len(codes)} window results differ, first {bad[:5].tolist()}: {codes[bad[:5]].tolist()} for {ref.codes[bad[:5]].tolist()}"
    assert (sums == ref.sums).all(), "stage sums differ"
    assert (vis == ref.visited).all(), "visited flags differ"
    raw = p.detect_raw(img, sf)
    assert raw.shape == ref.candidates.shape and (raw == ref.candidates).all(), "candidates differ"
    a, b = p.detectMultiScale(img, sf, 2), orc.detect_multiscale(o, img, sf, 2, nthreads=8)
    assert a.shape == b.shape and (a == b).all(), "rectangles differ"
    return len(raw)


def worker(rows):
    import tempfile
    import cascadeclassifier_amd as cc
    from oracle import oracle as orc
    from tests import haar_windows as hw
    from tests.util import frame_natural
    assert os.environ.get("CCAMD_SPEC_TILE_Y1") == str(rows)
    tmp = tempfile.mkdtemp(prefix="step1_tall_")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    haar_xml = os.path.join(root, "data", "haarcascade_frontalface_synthetic.xml")
    n_cand = 0

    def classifier(text, k, **env):
        for kk in ("CCAMD_WAVE_BELOW", "CCAMD_SPLIT_STUMPS"):
            os.environ.pop(kk, None)
        os.environ.update(env)
        p = cc.CascadeClassifier()
        assert p.load_from_string(text)
        assert p.specialize(k) == k
        return p

    # 1. tile edges, three window sizes, every stage compiled
    for (W, H) in ((24, 24), (20, 20), (25, 24)):
        text = hw.stump_xml(W, H, False)
        o = hw.oracle_cascade(tmp, text, "c%dx%d.xml" % (W, H))
        frames = edge_frames(W, H, rows)
        assert covered_targets(W, H, rows, frames) == set(ny_targets(rows)) | set(nx_targets())
        p = classifier(text, 4)
        for i, (w, h) in enumerate(frames):
            n_cand += same_as_oracle(p, o, hw.pasted_frame(W, H, 60 + i, w=w, h=h, scales=(2.2, 2.6, 3.1)))
        print("edges %dx%d: frames %s" % (W, H, frames), flush=True)
        if (W, H) != (24, 24):
            continue
        # 2. two stages compiled (the rest table-driven), and the switches that choose between the late-stage paths
        frame = hw.pasted_frame(W, H, 64, w=frames[-1][0], h=frames[0][1], scales=(2.2, 2.6, 3.1))
        for wb, split in ((0, 1), (64, 1), (0, 0), (64, 0)):
            p = classifier(text, 2, CCAMD_WAVE_BELOW=str(wb), CCAMD_SPLIT_STUMPS=str(split))
            n_cand += same_as_oracle(p, o, frame)
        print("switches ok", flush=True)
    for kk in ("CCAMD_WAVE_BELOW", "CCAMD_SPLIT_STUMPS"):
        os.environ.pop(kk, None)
    # 3. the stock-profile cascade: a batch of three frames, and tiles that stay crowded into the table-driven stages
    o = orc.load_cascade_xml(haar_xml)
    text = open(haar_xml).read()
    p = classifier(text, 7)
    batch = np.stack([frame_natural(200, 150, 80 + i) for i in range(3)])
    batch[1, 20:73, 30:83] = dense_template_frame(haar_xml)[0:53, 0:53]
    got = p.detect_batch(batch, SCALE_FACTOR, 2)
    for f in range(3):
        want = orc.detect_multiscale(o, batch[f], SCALE_FACTOR, 2, nthreads=8)
        assert got[f].shape == want.shape and (got[f] == want).all(), "batch frame %d differs" % f
    print("batch ok", flush=True)
    crowded = dense_template_frame(haar_xml)
    p = classifier(text, 2)
    most = late_windows_per_tile(o, crowded, rows, 2)
    assert most > 24, most  # more than the default wave_below at the first table-driven stage
    n_cand += same_as_oracle(p, o, crowded)
    print("crowded ok: %d windows of one tile enter stage 2" % most, flush=True)
    assert n_cand > 0
    print("STEP1_TALL_OK rows=%d candidates=%d" % (rows, n_cand), flush=True)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    worker(int(sys.argv[1]))
