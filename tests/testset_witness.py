"""numpy restatement of the reference's test mode of createsamples (tools/createsamples/utility.cpp:1031-1123,
cvCreateTestSamples), written from those lines: per iteration a background image from the reader (window 10 x 10), the
sticky maxscale, the float uniform for the scale, the rectangle, the inverse draw and icvPlaceDistortedSample with
inscribe = 1, maxshift = maxscale = 0 into src(Rect(x, y, width, height)). The random numbers, the reader, the placement
and the pixels are tests/sample_witness.py's; this file adds cv::RNG's float overload and the loop."""
import numpy as np

from tests import sample_witness as W

F32 = np.float32


def uniform_float(rng, a, b):
    """cv::RNG::uniform(float a, float b) = ((float)*this) * (b - a) + a with operator float() = next() *
    2.3283064365386962890625e-10f: ONE draw, every operation rounded to float."""
    a, b = F32(a), F32(b)
    f = F32(rng.next()) * F32(2.3283064365386962890625e-10)
    return F32(F32(f * F32(b - a)) + a)


def new_reader(sizes):
    """icvInitBackgroundReaders(bgfilename, Size(10, 10)) (:1055) over image sizes (width, height)."""
    return W.BgReader(sizes, 10, 10)


def plan(src_w, src_h, win_w, win_h, p, rng, num, reader, maxscale=-1.0, done=0):
    """Iterations done .. MIN(done + num, images) - 1 of the loop (:1078-1101). Returns (samples, maxscale, done): samples is
    a list of dicts (iteration, bg_index, rect = (x, y, width, height), rec = the placement's record as W.plan makes it).
    Raises ValueError where the reference asserts: no usable background, a rectangle that leaves its image."""
    maxscale = float(maxscale)
    count = min(done + num, len(reader.sizes))
    place = W.Params(p.bgcolor, p.bgthreshold, p.invert, p.maxintensitydev, p.maxxangle, p.maxyangle, p.maxzangle,
                     inscribe=1, maxshift=0.0, maxscale=0.0)
    out = []
    for i in range(done, count):
        reader._next_image(rng)  # icvGetNextFromBackgroundData (:1081)
        cols, rows = reader.sizes[reader.last]
        if maxscale < 0.0:  # MIN(0.7F * cols / winwidth, 0.7F * rows / winheight), float, assigned once (:1082-1085)
            maxscale = float(min(F32(F32(0.7) * F32(cols)) / F32(win_w), F32(F32(0.7) * F32(rows)) / F32(win_h)))
        if maxscale < 1.0:
            continue
        with np.errstate(all="ignore"):
            scale = uniform_float(rng, 1.0, F32(maxscale))
            fw, fh = scale * F32(win_w), scale * F32(win_h)
        if not (1 <= fw < 4097 and 1 <= fh < 4097):
            raise ValueError(f"iteration {i + 1}: rectangle sides outside 1..4096")
        width, height = int(fw), int(fh)
        x = int(rng.uniform(0.1, 0.8) * (cols - width))
        y = int(rng.uniform(0.1, 0.8) * (rows - height))
        if x < 0 or y < 0 or x + width > cols or y + height > rows:  # src(Rect(x, y, width, height)) asserts (:1099)
            raise ValueError(f"iteration {i + 1}: the rectangle leaves its image")
        # the inverse draw (:1096-1098) is the first thing W.plan does without a reader; then icvPlaceDistortedSample
        rec = W.plan(src_w, src_h, width, height, place, rng, 1)[0]
        out.append(dict(iteration=i + 1, bg_index=reader.last, rect=(x, y, width, height), rec=rec))
    return out, maxscale, max(done, count)


def render(image, bg_images, p, samples, dense=False):
    """The images the tool would hand to imwrite (:1111): per sample a fresh copy of its background with the placement
    blended into the rectangle."""
    src, mask = W.start_distortion(image, p.bgcolor, p.bgthreshold)
    f = W.render_dense if dense else W.render_sparse
    out = []
    for s in samples:
        img = np.array(bg_images[s["bg_index"]], np.uint8, copy=True)
        x, y, w, h = s["rect"]
        img[y:y + h, x:x + w] = f(src, mask, p.bgcolor, s["rec"], w, h, img[y:y + h, x:x + w].copy())
        out.append(img)
    return out


def generate(image, bg_images, win_w, win_h, p, rng, num, maxscale=-1.0, dense=False):
    """(images, samples, maxscale) of one run of cvCreateTestSamples."""
    image = np.asarray(image, np.uint8)
    reader = new_reader([(b.shape[1], b.shape[0]) for b in bg_images])
    samples, maxscale, _ = plan(image.shape[1], image.shape[0], win_w, win_h, p, rng, num, reader, maxscale)
    return render(image, bg_images, p, samples, dense), samples, maxscale
