"""Witnesses for filling a stage's training set (section 6c of the C ABI, cascadeclassifier_amd/trainer.py), in plain
Python ints and floats:

* fill_select: the loop of CvCascadeClassifier::fillPassedSamples (cascadeclassifier.cpp:329-357) over given pass flags;
* NegReaderWitness / reader_stream: CvCascadeImageReader::NegReader (imagestorage.cpp:23-126) window by window, with images
  held in memory where the reference reads files. It keeps the reference's members (last, round, point, offset, scale)
  and resizes nothing: a window is named by its image, the image's offset, the level's size and its corner."""
import numpy as np

FILLED, RATIO, EXHAUSTED = 0, 1, 2
f32 = np.float32


def fill_select(flags, start, want, got_before=0, consumed_before=0, ratio=0.0):
    """(n_filled, n_consumed, stop, keep list) of the loop from stream position `start` over flags[start:]."""
    n = len(flags)
    got = consumed = 0
    j = int(start)
    keep = []
    while True:
        if got == want:  # the for-loop over the slots ends (:333)
            stop = FILLED
            break
        c, g = consumed_before + consumed, got_before + got
        if c != 0 and float(g + 1) / float(c) <= ratio:  # :337
            stop = RATIO
            break
        if j == n:  # no further window in this stream (:342)
            stop = EXHAUSTED
            break
        consumed += 1
        if flags[j]:
            keep.append(j)
            got += 1
        j += 1
    return got, consumed, stop, keep


def fill_select_np(flags, start, want, got_before=0, consumed_before=0, ratio=0.0):
    """fill_select for streams too long for a Python loop: the same three conditions at every position at once, in exact
    int64 counts and IEEE double division. tests/test_trainer_host.py holds it to the loop."""
    flags = np.asarray(flags, np.uint8)
    m = len(flags) - int(start)
    P = np.concatenate([[0], np.cumsum(flags[start:], dtype=np.int64)])  # flags set before position start + k
    k = np.arange(m + 1, dtype=np.int64)
    c = consumed_before + k
    filled = P >= want
    by_ratio = (c != 0) & ((got_before + P + 1).astype(np.float64) / np.where(c == 0, 1, c).astype(np.float64) <= ratio)
    at = int(np.argmax(filled | by_ratio | (k == m)))
    stop = FILLED if filled[at] else RATIO if by_ratio[at] else EXHAUSTED
    keep = (np.nonzero(flags[start:start + at])[0] + start).tolist()
    return int(P[at]), at, stop, keep


DENSITIES = (("none", 0.0), ("all", 1.0), ("one_percent", 0.01), ("half", 0.5))


def flag_arrays(n, seed=0):
    """name -> n pass flags at each of the densities."""
    rng = np.random.default_rng(seed + n)
    return {name: (rng.random(n) < p).astype(np.uint8) for name, p in DENSITIES}


def ratio_cases(flags, start):
    """(got_before, consumed_before, ratio, name). The ties sit at the middle of flags[start:]: the ratio is the very
    quotient the loop forms there, so `<=` holds with equality; one ulp below it does not hold there, one above does."""
    m = len(flags) - start
    k = max(m // 2, 1)
    g = int(np.asarray(flags[start:start + k], np.int64).sum())
    tie = float(g + 1) / float(k)
    yield 0, 0, 0.0, "zero"
    yield 0, 0, tie, "tie"
    yield 0, 0, float(np.nextafter(tie, np.inf)), "above"
    yield 0, 0, float(np.nextafter(tie, -np.inf)), "below"
    g0, c0 = 2 ** 30 + 3, 2 ** 31 + 7  # counts of a long stage: past 32 bits
    tie64 = float(g0 + g + 1) / float(c0 + k)
    yield g0, c0, tie64, "tie64"
    yield g0, c0, float(np.nextafter(tie64, -np.inf)), "below64"
    yield 0, 0, 10.0, "guard"  # consumed == 0 at the first position: the ratio must not be looked at there


def select_cases(flags, starts=None, ratios=None):
    """(start, want, got_before, consumed_before, ratio, name) over start in {0, 1, mid, n}, want in {0, 1, exact, exact + 1}."""
    n = len(flags)
    for start in sorted({0, min(1, n), n // 2, n}) if starts is None else starts:
        count = int(np.asarray(flags[start:], np.int64).sum())
        for want in sorted({0, 1, count, count + 1}):
            for g0, c0, ratio, name in ratio_cases(flags, start):
                if ratios is None or name in ratios:
                    yield start, want, g0, c0, ratio, name


class NegReaderWitness:
    def __init__(self, images, win):
        self.images = images
        self.W, self.H = win
        self.last = self.round = 0
        self.scale_factor = f32(1.4142135623730950488016887242097)
        self.step_factor = f32(0.5)
        self.img = None  # size (cols, rows) of the current ladder level; None: img.empty()
        self.index = None
        self.i = 0  # windows handed out from the open image

    def next_img(self):  # imagestorage.cpp:57-88
        count = len(self.images)
        ok = False
        for _ in range(count):
            index = self.last
            src = self.images[index]
            self.last += 1
            self.round += self.last // count
            self.round = self.round % (self.W * self.H)
            self.last %= count
            rows, cols = src.shape
            ox = min(self.round % self.W, cols - self.W)
            oy = min(self.round // self.W, rows - self.H)
            if ox >= 0 and oy >= 0:
                ok = True
                break
        assert ok, "no image of the list holds a window"
        self.index, self.src = index, (cols, rows)
        self.offset = (ox, oy)
        self.point = [ox, oy]
        self.scale = max((f32(self.W) + f32(ox)) / f32(cols), (f32(self.H) + f32(oy)) / f32(rows))
        self.img = (int(self.scale * f32(cols) + f32(0.5)), int(self.scale * f32(rows) + f32(0.5)))
        self.i = 0
        return True

    def get(self):  # imagestorage.cpp:90-126
        """(image index, (ox, oy), window number in the image's stream, level size, corner) of the next window."""
        if self.img is None:
            self.next_img()
        out = (self.index, self.offset, self.i, self.img, tuple(self.point))
        self.i += 1
        if int(f32(self.point[0]) + (f32(1.0) + self.step_factor) * f32(self.W)) < self.img[0]:
            self.point[0] += int(self.step_factor * f32(self.W))
        else:
            self.point[0] = self.offset[0]
            if int(f32(self.point[1]) + (f32(1.0) + self.step_factor) * f32(self.H)) < self.img[1]:
                self.point[1] += int(self.step_factor * f32(self.H))
            else:
                self.point[1] = self.offset[1]
                self.scale = self.scale * self.scale_factor
                if self.scale <= f32(1.0):
                    self.img = (int(self.scale * f32(self.src[0])), int(self.scale * f32(self.src[1])))
                else:
                    self.next_img()
        return out


def reader_stream(images, win, n):
    """The first n windows of the reader over `images`, as NegReaderWitness.get names them."""
    r = NegReaderWitness(images, win)
    return [r.get() for _ in range(n)]
