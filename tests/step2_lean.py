"""The specialised Haar kernel's STEP-2 module in the lean LDS layout, shared by tests/test_step2_lean_host.py and
tests/test_gpu_step2_lean_tiles.py: the layout's arithmetic restated from cc_eval_common.h / cc_eval_kernel.inc (tile
words, the LDS sum and the blocks it runs per CU, norm-factor slots, queue tables, what lives between them, row ownership of the
dense phase), the frame shapes at the tile edges, and the cascade whose first stages pass every window.

Shapes. A STEP-2 scale (scale factor up to 2) of nx x ny window origins is cut into tiles of 64 x TILE_Y. The frames give the
largest STEP-2 scale (scale 1) ny = 1, 9, 10, 11, 19, 20, 21 window rows (around one and two tiles of 10 rows: a ragged last
tile, a ragged last round of the row ownership, one row more than a full tile) and nx = 1, 63, 64, 65 window columns. Widths
24, 148, 150, 152 give those columns; the rows of a scale depend on the frame's height AND, through the scan's stripes, on
its width, so for every width the heights are found from cc.scale_plan (edge_frame_sizes), and the heights 24, 40, 42, 44,
60, 62, 64 are run at every width besides. The largest of these frames is 152 x 65."""
import numpy as np

HEIGHTS = (8, 9, 10, 11, 12)
WINDOWS = ((20, 20), (24, 24), (32, 32))
FRAME_HEIGHTS = (24, 40, 42, 44, 60, 62, 64)
FRAME_WIDTHS = (24, 148, 150, 152)
NY_TARGETS = (1, 9, 10, 11, 19, 20, 21)
NX_TARGETS = (1, 63, 64, 65)
SCALE_FACTOR = 1.1
TILE_X = 64
WAVES = 4          # wavefronts of a block
THREADS = 256
CU_LDS = 160 * 1024
PART_BYTES = 3 * 64 * 8   # four slices' partial sums: slices 1..3, 64 doubles each


ALLOC = 1280              # LDS allocation unit: 1 / 128 of a CU's 160 KiB (lds_blocks_resident)


# ---- tile and LDS sum (TileGeom<2>, eval_lds_bytes with lean = true, lds_blocks_resident) ----
def row_stride_step2(W):
    cols = (TILE_X - 1) * 2 + W + 1
    plane = ((cols + 3) // 4 * 4 // 2 + 1) // 2 * 2
    stride = 2 * plane
    while ((2 * stride) & 31) % 8 == 0:
        stride += 2
    return stride


def tile_words_step2(W, H, rows):
    return ((rows - 1) * 2 + H + 1) * row_stride_step2(W)


def skew_step2(W):
    return (2 * row_stride_step2(W)) & 31


def blocks_per_cu(lds_bytes):
    """Blocks of 256 threads a CU runs by the LDS request alone, the request rounded up to allocation units."""
    units = -(-lds_bytes // ALLOC)
    return min(8, (CU_LDS // ALLOC) // units)


def blocks_by_bytes(lds_bytes):
    """The count without allocation units (what the runtime's occupancy query answers)."""
    return min(8, CU_LDS // lds_bytes)


def lean_lds_bytes(W, H, rows):
    """Integral tile (16-byte multiple) + norm factors float[rows][64] + two queue tables u16[rows * 64] + 3 x 32 counters."""
    tile = (tile_words_step2(W, H, rows) + 3) // 4 * 4 * 4
    return tile + rows * TILE_X * 4 + 2 * rows * TILE_X * 2 + 3 * 32 * 4


def padded_lds_bytes(W, H, rows=8):
    """The request of the module this one replaces: s_part and norm-factor rows of pitch 96."""
    tile = (tile_words_step2(W, H, rows) + 3) // 4 * 4 * 4
    return tile + PART_BYTES + rows * 96 * 4 + 2 * rows * TILE_X * 2 + 3 * 32 * 4


def default_rows(W, H):
    want = blocks_per_cu(lean_lds_bytes(W, H, 8))
    return max(r for r in HEIGHTS if blocks_per_cu(lean_lds_bytes(W, H, r)) >= want)


# ---- index arithmetic of the layout ----
def vnf_slot(ids, skew):
    return (ids & ~63) | (((ids & 63) + skew * (ids >> 6)) & 63)


def win_class(ids, skew):
    return ((ids & 63) + skew * (ids >> 6)) & 31


def queue_entries(rows):
    """u16 entries of the queue area: two tables of 64 * rows ids."""
    return 2 * rows * TILE_X


def q_index(g, row, c, entries):
    """Table 0 grows from the front of the area, table 1 backwards from its end."""
    return entries - 32 - row * 32 + c if g & 1 else row * 32 + c


def table_entries(g, R, entries):
    return {q_index(g, row, c, entries) for row in range(R) for c in range(32)}


def gap_bytes(rows_ty, R, extra=0):
    """Bytes between the tables while neither holds more than R rows (extra: bytes the area does not have, for mutations)."""
    return 2 * rows_ty * TILE_X * 2 + extra - 2 * R * 32 * 2


def split_need_bytes(ns):
    return (ns - 1) * (THREADS // ns) * 8


def slices_chosen(rows_ty, R, extra=0):
    """{ns} the thread phase can end up with at R queued rows: the leftover row groups ask for 4, 2 or 1 slices (one, two or
    three leftover groups), and the layout halves that until the partial sums fit the gap."""
    groups = (R + 1) // 2
    rem = groups % WAVES
    if rem == 0:
        return set()
    ns = 1
    while ns * 2 * rem <= WAVES:
        ns *= 2
    while ns > 1 and split_need_bytes(ns) > gap_bytes(rows_ty, R, extra):
        ns >>= 1
    return {ns}


def split_entries(R, ns):
    """u16 entries the partial sums occupy: from behind row R of table 0."""
    return set(range(R * 32, R * 32 + split_need_bytes(ns) // 2))


def wave_list_entries(qg, entries):
    """Four lists of 64 ids in the far end of the table that group qg does not read."""
    lo = 0 if qg & 1 else entries - WAVES * 64
    return set(range(lo, lo + WAVES * 64))


# ---- row ownership of the staging and dense phases ----
def rows_per_thread(rows_ty):
    return (rows_ty + WAVES - 1) // WAVES


def owned_rows(wave, rows_ty):
    """Tile rows wavefront `wave` evaluates, round by round (a round beyond the tile is skipped)."""
    per = rows_per_thread(rows_ty)
    if rows_ty % WAVES == 0:
        cand = [wave * per + k for k in range(per)]
    else:
        cand = [wave + k * WAVES for k in range(per)]
    return [r for r in cand if r < rows_ty]


# ---- frames and cascades of the GPU tests ----
def grid_at_scale_1(w, h, W=24, H=24):
    import cascadeclassifier_amd as cc
    s0 = cc.scale_plan(W, H, w, h, SCALE_FACTOR)[0]
    assert float(s0["scale"]) == 1.0 and int(s0["ystep"]) == 2
    return int(s0["nx"]), int(s0["ny"])


def edge_frame_sizes():
    """[(w, h)]: for every width of FRAME_WIDTHS the smallest height that gives each ny of NY_TARGETS at scale 1, and the
    heights of FRAME_HEIGHTS at every width; no size twice."""
    sizes = []
    for w in FRAME_WIDTHS:
        for ny in NY_TARGETS:
            h = next(h for h in range(24, 66) if grid_at_scale_1(w, h)[1] == ny)
            sizes.append((w, h))
        sizes += [(w, h) for h in FRAME_HEIGHTS]
    return sorted(set(sizes))


def pass_all_then_thin_xml(windows, n_pass_all=4, n_thin=16, stumps=8, keep=0.8, seed=5):
    """24x24 upright stump cascade: `n_pass_all` stages whose threshold lies below every possible sum, then `n_thin` stages
    each calibrated to keep about `keep` of the calibration windows that reach it. Leaves are multiples of 1/64, so stage
    sums are exact in any order (stump-split and wave phase allowed)."""
    from oracle import oracle as orc
    from tests import cascade_factory as cf
    rng = np.random.default_rng(seed)
    cat = orc.haar_catalog(24, 24, 0)
    ui = np.nonzero((cat["tilted"] == 0) & (cat["r"][:, 0, 2] * cat["r"][:, 0, 3] >= 16))[0]
    n_stages = n_pass_all + n_thin
    n = n_stages * stumps
    feats = cat[rng.choice(ui, n, replace=False)].copy()
    v = cf.calibration_values(feats, windows, 24, 24)
    thr = np.median(v, axis=1).astype(np.float32)
    a = (rng.integers(16, 65, n) / 64.0).astype(np.float32)
    sign = rng.choice([-1.0, 1.0], n).astype(np.float32)
    stages, k = [], 0
    alive = np.ones(v.shape[1], bool)
    for s in range(n_stages):
        sl = slice(k, k + stumps)
        votes = np.where(v[sl] < thr[sl, None], (a * sign)[sl, None], (-a * sign)[sl, None]).astype(np.float64)
        sums = votes.sum(0)
        if s < n_pass_all:
            st = np.float32(-float(a[sl].sum()) - 1.0)
        else:
            pool = sums[alive] if alive.sum() > 20 else sums
            st = np.float32(np.quantile(pool, 1.0 - keep))
            alive &= sums >= st
        weaks = [([(0, -1, k + i, thr[k + i])], [a[k + i] * sign[k + i], -a[k + i] * sign[k + i]]) for i in range(stumps)]
        stages.append((st, weaks))
        k += stumps
    return cf.haar_xml(feats, stages, mode="BASIC", W=24, H=24)


def late_counts_per_tile(codes, nx, ny, rows_ty, n_stages):
    """{stage: set of window counts over the tiles} of one STEP-2 scale: the windows of a tile still alive when the stage
    starts, by the oracle's result codes (what the kernel compares with wave_below)."""
    codes = codes.reshape(ny, nx)
    out = {}
    for s in range(2, n_stages):
        reached = (codes == 1) | (codes <= -s)
        out[s] = {int(reached[ty:ty + rows_ty, tx:tx + TILE_X].sum()) for ty in range(0, ny, rows_ty) for tx in range(0, nx, TILE_X)}
    return out


def late_rows_per_tile(codes, nx, ny, rows_ty, skew, n_stages):
    """{stage: set of queue-table row counts over the tiles} of one STEP-2 scale: the rows of the table a stage reads = the
    most windows of one bank class still alive when the stage starts, by the oracle's result codes."""
    codes = codes.reshape(ny, nx)
    out = {}
    for s in range(1, n_stages):
        reached = (codes == 1) | (codes <= -s)
        seen = set()
        for ty in range(0, ny, rows_ty):
            for tx in range(0, nx, TILE_X):
                t = reached[ty:ty + rows_ty, tx:tx + TILE_X]
                yy, xx = np.nonzero(t)
                if len(yy) == 0:
                    seen.add(0)
                    continue
                cls = (xx + skew * yy) & 31
                seen.add(int(np.bincount(cls, minlength=32).max()))
        out[s] = seen
    return out
