"""The named inputs of the image-preparation tests (tests/test_images_truth_cpu.py, tests/test_gpu_images.py): CASES[name] = (image uint8 [h,w,C], (W, H)),
from a generator seeded by the name.  Sizes are small and chosen for the path they take; the strip sizes are read from gsrast.images."""
import zlib

import numpy as np

from gsrast.images import H_STRIP, V_STRIP

SIZES = {                                                 # name: ((w, h), (W, H))
    "down": ((37, 23), (16, 10)),                         # non-integer downscale
    "up": ((13, 9), (40, 27)),                            # fs clamps to 1: five taps
    "v_only": ((64, 48), (64, 20)),                       # the horizontal pass does not run
    "h_only": ((50, 31), (7, 31)),                        # the vertical pass does not run
    "copy": ((33, 17), (33, 17)),
    "one_pixel": ((129, 65), (1, 1)),
    "taps_401": ((300, 7), (3, 9)),                       # 401 taps on one axis, an upscale on the other
    "taps_chunks": ((9000, 3), (2, 2)),                   # more taps than one staged chunk of the horizontal pass holds
    "strips": ((1031, 517), (400, 201)),                  # many strips; 3 w no multiple of 4: rows at every byte alignment
    "hstrip_below": ((613, 9), (H_STRIP - 1, 4)),
    "hstrip": ((613, 9), (H_STRIP, 4)),
    "hstrip_above": ((613, 9), (H_STRIP + 1, 4)),
    "vstrip_two": ((301, 5), (2 * V_STRIP + 3, 6)),       # an upscale over more than two strips of the vertical pass
}
GOLDEN_MAX = (64, 48)                                     # tests/golden/images_pillow.npz holds the cases whose input is no larger


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _build():
    cases = {}
    for name, ((w, h), size) in SIZES.items():
        for C in (1, 3, 4):
            cases[f"{name}_C{C}"] = (_rng(f"{name}_C{C}").integers(0, 256, (h, w, C), dtype=np.uint8), size)
    # a strided, non-contiguous view: every second column of an image twice as wide
    wide = _rng("strided").integers(0, 256, (24, 80, 3), dtype=np.uint8)
    cases["strided_C3"] = (wide[:, ::2], (17, 11))
    # 16-pixel blocks of 0 and 255, upscaled: the bicubic overshoot leaves [0, 255] on both sides in both passes
    yy, xx = np.mgrid[0:24, 0:40]
    for C in (1, 3, 4):
        img = np.repeat((((xx // 16 + yy // 16) % 2) * 255).astype(np.uint8)[..., None], C, axis=2)
        if C == 4:
            img[..., 3] = 255
        cases[f"clip_C{C}"] = (np.ascontiguousarray(img), (130, 77))
    # RGBA whose alpha has columns of 0, of 255 and of random values
    img = _rng("alpha_columns").integers(0, 256, (20, 36, 4), dtype=np.uint8)
    img[:, :12, 3] = 0
    img[:, 12:24, 3] = 255
    cases["alpha_columns_C4"] = (img, (15, 9))
    # an [h,w] image of mode L
    cases["flat_L"] = (_rng("flat_L").integers(0, 256, (23, 37), dtype=np.uint8), (16, 10))
    return cases


CASES = _build()
GOLDEN = sorted(n for n, (img, _) in CASES.items() if img.shape[1] <= GOLDEN_MAX[0] and img.shape[0] <= GOLDEN_MAX[1])


def random_pairs(count=50, seed=0):
    """Seeded random (image, size) pairs: sizes 1..70 on either side, 1, 3 or 4 channels."""
    r = np.random.default_rng(seed)
    for _ in range(count):
        w, h, W, H = (int(x) for x in r.integers(1, 71, 4))
        C = (1, 3, 4)[int(r.integers(0, 3))]
        yield r.integers(0, 256, (h, w, C), dtype=np.uint8), (W, H)
