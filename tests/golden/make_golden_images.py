"""Writes tests/golden/images_pillow.npz: for every case of tests/images_cases.py whose input is at most 64 x 48, the input and what
PIL.Image.resize returns for it with its defaults, and the version of the Pillow that said so.

    python tests/golden/make_golden_images.py

Keys: "<case>/in", "<case>/size" (W, H), "<case>/out", and "pillow_version"."""
import os
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "gs-sr_amd"))
import images_cases as cases  # noqa: E402


def pillow_resize(img, size):
    """uint8 [h,w,C] or [h,w] -> the same layout resized by Pillow (mode L, RGB or RGBA by the channel count)."""
    flat = img.ndim == 2 or img.shape[2] == 1
    pil = Image.fromarray(np.ascontiguousarray(img.reshape(img.shape[:2]) if flat else img))
    out = np.array(pil.resize(size))
    return out.reshape(out.shape[:2] + (1,)) if flat and img.ndim == 3 else out


def main():
    doc = {"pillow_version": np.array(PIL.__version__)}
    for name in cases.GOLDEN:
        img, size = cases.CASES[name]
        doc[f"{name}/in"] = np.ascontiguousarray(img)
        doc[f"{name}/size"] = np.array(size, dtype=np.int64)
        doc[f"{name}/out"] = pillow_resize(img, size)
    path = os.path.join(HERE, "images_pillow.npz")
    np.savez_compressed(path, **doc)
    print(f"{path}: {len(cases.GOLDEN)} cases, Pillow {PIL.__version__}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
