"""The LDS classes of HOG windows: which windows the evaluator's setImage kernel (k_hog_set_images) and the negative miner's
window kernel (k_negmine_hog) accept, with how many planes per pass and how many bytes. TABLE is written out by hand; the host
test (tests/test_hog_lds_host.py) holds it to the library's own report (cc_debug_hog_lds) and to `restated`, the formulas in
plain Python. The GPU tests take their windows from the lists below, so a change of a budget or of a formula fails on the CPU
before a window silently moves to another class."""
import ctypes as C

KIB = 1024
DEFAULT_KIB, MAX_KIB = 64, 160  # LDS a kernel gets without asking; LDS of one CU of gfx950, the most a workgroup can ask for

# (W, H): (planes per setImage pass (0: refused), setImage budget in KiB, setImage bytes, miner bytes)
TABLE = {
    (24, 24): (10, 64, 26880, 27880),
    (32, 32): (10, 64, 47360, 48680),
    (75, 32): (5, 64, 60640, 112320),
    (32, 75): (5, 64, 61500, 112320),     # tall
    (24, 60): (9, 64, 61200, 68200),      # tall
    (70, 40): (4, 64, 59440, 130440),
    (37, 37): (10, 64, 63085, 64605),     # last window with ten planes per pass; last miner window inside 64 KiB
    (38, 38): (9, 64, 60572, 68060),      # first with nine; first miner window that opts in
    (59, 59): (3, 64, 59885, 161405),     # largest square the miner accepts
    (60, 59): (3, 64, 60888, 164100),     # first the miner refuses
    (86, 40): (3, 64, 58960, 159880),
    (40, 86): (3, 64, 59512, 159880),
    (87, 40): (3, 64, 59640, 161720),
    (88, 40): (3, 64, 60320, 163560),     # largest of height 40 the miner accepts
    (40, 88): (3, 64, 60896, 163560),
    (89, 40): (3, 64, 61000, 165400),     # first of height 40 the miner refuses
    (85, 85): (1, 64, 65365, 331965),     # one plane per pass inside 64 KiB: ten passes, no opt-in
    (86, 85): (4, 160, 154870, 335830),   # first window of the 160 KiB branch: passes of 4, 4 and 2 planes
    (128, 64): (3, 160, 140032, 376360),
    (96, 96): (3, 160, 157824, 422440),
    (128, 128): (1, 160, 147968, 747560),
    (134, 135): (1, 160, 163350, 824850),  # last window the evaluator accepts
    (135, 134): (1, 160, 163346, 824850),
    (135, 135): (0, 160, 164565, 830965),  # refused: one plane per pass does not fit 160 KiB
    (136, 134): (0, 160, 164552, 830920),
    (160, 160): (0, 160, 231040, 1164840),
    (128, 96): (2, 160, 160512, 561960),
}


def set_bytes(W, H, P):
    """k_hog_set_images: magnitudes [H][W] float, row sums of P planes [P][H][W + 1] float, bins [H][W] bytes."""
    return W * H * 4 + P * H * (W + 1) * 4 + W * H


def mine_bytes(W, H):
    """k_negmine_hog: ten planes [H + 1][W + 1] float, magnitudes [H][W] float, bins [H][W] bytes."""
    return 10 * (W + 1) * (H + 1) * 4 + W * H * 5


def restated(W, H):
    """The row of TABLE from the formulas: all ten planes inside 64 KiB where they fit, else as many as fit, else as many as
    160 KiB holds; a refused window reports the bytes of one plane per pass."""
    for kib in (DEFAULT_KIB, MAX_KIB):
        P = 10
        while P > 0 and set_bytes(W, H, P) > kib * KIB:
            P -= 1
        if P > 0:
            break
    return P, kib, set_bytes(W, H, max(P, 1)), mine_bytes(W, H)


def exported(W, H):
    """The row of TABLE as the library reports it (host only, no device)."""
    from cascadeclassifier_amd import _lib as L
    p, kib, sb, mb = C.c_int(-1), C.c_int(-1), C.c_int64(-1), C.c_int64(-1)
    L.check(L.lib().cc_debug_hog_lds(W, H, C.byref(p), C.byref(kib), C.byref(sb), C.byref(mb)))
    return p.value, kib.value, sb.value, mb.value


def eval_accepts(win):
    return TABLE[win][0] > 0


def miner_accepts(win):
    return TABLE[win][3] <= MAX_KIB * KIB


def miner_opts_in(win):
    return DEFAULT_KIB * KIB < TABLE[win][3] <= MAX_KIB * KIB


def eval_opts_in(win):
    return eval_accepts(win) and TABLE[win][2] > DEFAULT_KIB * KIB


# The windows of the GPU tests, by what they are there for. Each list is asserted against TABLE's classes in the host test.
MINER_WINDOWS = [(32, 75), (37, 37), (38, 38), (59, 59), (86, 40), (40, 86), (88, 40), (40, 88)]
MINER_LARGE = [(59, 59), (86, 40), (40, 86), (88, 40), (40, 88)]   # mined on one small background: a few dozen windows
MINER_LAST_ACCEPTED = [(59, 59), (88, 40), (40, 88)]
MINER_FIRST_REFUSED = [(60, 59), (89, 40)]
EVAL_WINDOWS = [(37, 37), (38, 38), (24, 60), (32, 75), (85, 85), (86, 85), (134, 135), (135, 134)]
EVAL_LAST_ACCEPTED = [(134, 135), (135, 134)]
EVAL_FIRST_REFUSED = [(135, 135), (136, 134)]
