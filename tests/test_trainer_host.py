"""CPU only. The background reader of the cascade driver (cascadeclassifier_amd/trainer.py) against NegReader written window
by window (tests/fill_witness.py), the witness of the fill loop on cases worked out by hand, and the bindings of section 6c."""
import ctypes as C

import numpy as np
import pytest

import cascadeclassifier_amd as cc
from cascadeclassifier_amd import _lib as L
from cascadeclassifier_amd.trainer import stream_ladder
from tests import fill_witness as fw

WIN = (3, 2)  # round wraps at 6: after six passes over the list


def _img(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


LISTS = {
    "one": [_img(9, 7, 1)],
    "two": [_img(9, 7, 1), _img(5, 4, 2)],
    "five_mixed": [_img(9, 7, 1), _img(2, 9, 2), _img(9, 7, 3), _img(4, 3, 4), _img(3, 2, 5)],  # [1] holds no window
    "equal_sizes": [_img(8, 6, k) for k in range(4)],
}


def _window_of(reader, idx, offset, pos):
    """(level size, corner) of stream position pos, from the reader's ladder."""
    rows, cols = reader.images[idx].shape
    sx, sy = int(0.5 * WIN[0]), int(0.5 * WIN[1])
    for lw, lh, nx, ny in stream_ladder(WIN, cols, rows, *offset):
        if pos < nx * ny:
            return (lw, lh), (offset[0] + (pos % nx) * sx, offset[1] + (pos // nx) * sy)
        pos -= nx * ny
    raise AssertionError("position behind the image's stream")


def _expand(reader, batch):
    """The windows a batch stands for, named as the witness names them."""
    out = []
    for k, idx in enumerate(batch["indices"]):
        first = batch["start"] if k == 0 else 0
        for pos in range(first, batch["n_windows"]):
            out.append((idx, (batch["ox"], batch["oy"]), pos) + _window_of(reader, idx, (batch["ox"], batch["oy"]), pos))
    return out


@pytest.mark.parametrize("name", sorted(LISTS))
@pytest.mark.parametrize("max_images", [1, 3, 256])
def test_batches_are_the_reader_stream(name, max_images):
    """Whole batches, one after the other, over enough windows for `round` to wrap past W * H more than once."""
    images = LISTS[name]
    r = cc.BackgroundReader(images, WIN)
    per_pass = sum(r.stream_length(i, (0, 0)) for i in range(len(images)) if images[i].shape[1] >= WIN[0] and images[i].shape[0] >= WIN[1])
    n = per_pass * (2 * WIN[0] * WIN[1] + 3)
    want = fw.reader_stream(images, WIN, n)
    rounds = set()
    got = []
    while len(got) < n:
        b = r.next_batch(max_images)
        assert 1 <= len(b["indices"]) <= max_images
        wins = _expand(r, b)
        got += wins
        r.advance(len(wins))
        rounds.add(r.round)
    assert got[:n] == want
    assert rounds == set(range(WIN[0] * WIN[1]))  # every offset was in use, so the wrap happened
    if name == "equal_sizes" and max_images > 1:
        assert len(cc.BackgroundReader(images, WIN).next_batch(max_images)["indices"]) > 1


@pytest.mark.parametrize("name", sorted(LISTS))
def test_a_stop_at_every_position(name):
    """advance(k) for every k up to the end of the second image (mid-row, last window of a level, last window of an image),
    then on in steps that are no multiple of anything: state and next window equal the witness's."""
    images = LISTS[name]
    probe = cc.BackgroundReader(images, WIN)
    b0 = probe.next_batch(1)
    probe.advance(b0["n_windows"])
    two = b0["n_windows"] + probe.next_batch(1)["n_windows"]
    ladder = stream_ladder(WIN, images[0].shape[1], images[0].shape[0], 0, 0)
    assert len(ladder) >= 2 and any(nx >= 2 and ny >= 2 for _, _, nx, ny in ladder)  # mid-row stops and level boundaries in image 0
    for k in range(two + 2):
        r = cc.BackgroundReader(images, WIN)
        w = fw.NegReaderWitness(images, WIN)
        done = 0
        for step in (k, 1, 7, two, 5):
            if done == 0 and step == 0:
                r.advance(0)  # nothing consumed: the reader stays unopened
                assert r.state()["current"] is None
                continue
            r.next_batch(2)  # looking ahead changes nothing
            r.advance(step)
            for _ in range(step):
                w.get()
            done += step
            assert (r.last, r.round, r.current, r.offset, r.position) == (w.last, w.round, w.index, w.offset, w.i), (k, step)
            nxt = fw.NegReaderWitness(images, WIN)  # a second witness, so that looking at the next window consumes nothing
            for _ in range(done):
                nxt.get()
            b = r.next_batch(1)
            assert (b["indices"][0], (b["ox"], b["oy"]), b["start"]) == nxt.get()[:3]


def test_reader_refuses_a_list_without_a_window():
    with pytest.raises(ValueError):
        cc.BackgroundReader([_img(2, 9, 1), _img(9, 1, 2)], WIN)
    with pytest.raises(ValueError):
        cc.BackgroundReader([], WIN)


def test_fill_select_witness_by_hand():
    f = [0, 1, 0, 0, 1, 1, 0]
    assert fw.fill_select(f, 0, 2) == (2, 5, fw.FILLED, [1, 4])
    assert fw.fill_select(f, 0, 0) == (0, 0, fw.FILLED, [])
    assert fw.fill_select(f, 2, 5) == (2, 5, fw.EXHAUSTED, [4, 5])
    assert fw.fill_select(f, 7, 1) == (0, 0, fw.EXHAUSTED, [])
    # (g + 1) / c == 0.25 at g = 0, c = 4 with flags 0 0 0 0: a tie stops
    assert fw.fill_select([0] * 8, 0, 3, ratio=0.25) == (0, 4, fw.RATIO, [])
    assert fw.fill_select([0] * 8, 0, 3, ratio=float(np.nextafter(0.25, 0))) == (0, 5, fw.RATIO, [])
    # c == 0: the ratio is not looked at before the first window, whatever it is
    assert fw.fill_select([1], 0, 1, ratio=10.0) == (1, 1, fw.FILLED, [0])
    assert fw.fill_select([1, 1], 0, 2, ratio=10.0) == (1, 1, fw.RATIO, [0])
    # counts carried over from earlier calls of the stage
    assert fw.fill_select([0, 0], 0, 1, got_before=1, consumed_before=6, ratio=0.25) == (0, 2, fw.RATIO, [])


def test_vector_form_of_the_witness_equals_the_loop():
    """fill_select_np, which the GPU tests use for the longest stream, on every case they run at the short lengths; and the
    cases really hold ties, stops by ratio past 32 bits and all three reasons."""
    seen, names = set(), set()
    for n in (0, 1, 63, 64, 65, 300, 1025):
        for flags in fw.flag_arrays(n).values():
            for start, want, g0, c0, ratio, name in fw.select_cases(flags):
                a = fw.fill_select(flags, start, want, g0, c0, ratio)
                assert fw.fill_select_np(flags, start, want, g0, c0, ratio) == a, (n, start, want, name)
                seen.add(a[2])
                if a[2] == fw.RATIO:
                    names.add(name)
                if name == "guard":
                    assert a[1] >= 1 or want == 0 or start == n
    assert seen == {fw.FILLED, fw.RATIO, fw.EXHAUSTED}
    assert {"tie", "above", "tie64", "guard"} <= names
    zeros = np.zeros(40, np.uint8)
    (g0, c0, tie, _), = [c for c in fw.ratio_cases(zeros, 0) if c[3] == "tie"]
    assert fw.fill_select(zeros, 0, 1, g0, c0, tie)[1] == 20 < fw.fill_select(zeros, 0, 1, g0, c0, float(np.nextafter(tie, 0)))[1]


def test_section_6c_is_bound():
    """The symbols exist with the declared signatures; without a device the compute entry points say so."""
    lib = L.lib()
    for name in ("cc_negminer_create_empty", "cc_negminer_fill", "cc_eval_fill_passed", "cc_debug_fill_select", "cc_debug_fill_scan_tile"):
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert lib.cc_debug_fill_scan_tile() >= 64 and lib.cc_debug_fill_scan_tile() % 64 == 0
    assert (L.CC_FILL_FILLED, L.CC_FILL_RATIO, L.CC_FILL_EXHAUSTED) == (fw.FILLED, fw.RATIO, fw.EXHAUSTED)
    for attr in ("fill", "empty"):
        assert hasattr(cc.NegativeMiner, attr)
    assert hasattr(cc.CvFeatureEvaluator, "fill_passed") and callable(cc.train_cascade)
    if lib.cc_device_count() > 0:
        return
    flags = np.ones(4, np.uint8)
    nf, nc, stop = C.c_int(0), C.c_int64(0), C.c_int(0)
    st = lib.cc_debug_fill_select(0, flags.ctypes.data_as(C.c_void_p), 4, 0, 2, 0, 0, 0.0, C.byref(nf), C.byref(nc), C.byref(stop), None)
    assert st == L.CC_ERR_NO_DEVICE
    with pytest.raises(cc.CascadeError) as err:
        cc.NegativeMiner.empty(0, (24, 24))
    assert err.value.status == L.CC_ERR_NO_DEVICE
    with pytest.raises(cc.CascadeError) as err:
        cc.train_cascade(np.zeros((2, 24, 24), np.uint8), [_img(64, 48, 1)], 2, 2, 1)
    assert err.value.status == L.CC_ERR_NO_DEVICE
