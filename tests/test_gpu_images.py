"""GPU tests (pytest -m gpu) of gsrast.images (gsr_image_resample of the C ABI, csrc/gsr_image.hip) against the numpy restatement of
tests/images_truth.py on the named inputs of tests/images_cases.py, and directly against what Pillow returned (tests/golden/images_pillow.npz).
Everything is an integer algorithm or a float32 operation rounded on its own: every comparison is of bytes, and no element is excused."""
import functools
import os

import numpy as np
import pytest
import torch

import images_cases as cases
import images_truth as truth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = np.load(os.path.join(ROOT, "tests", "golden", "images_pillow.npz"))
NAMES = sorted(cases.CASES)
COLOUR = [n for n in NAMES if cases.CASES[n][0].ndim == 3 and cases.CASES[n][0].shape[2] >= 3]


@functools.lru_cache(maxsize=None)
def _truth(name):
    img, size = cases.CASES[name]
    out = truth.resize(img, size)
    out.setflags(write=False)
    return out


def _dev(img):
    """The image on the device with the strides it has on the host (a non-contiguous case stays non-contiguous)."""
    if img.flags.c_contiguous:
        return torch.from_numpy(img).to(DEV)
    base = torch.from_numpy(np.ascontiguousarray(img.base)).to(DEV)
    view = base[:, ::2]
    assert not view.is_contiguous() and np.array_equal(view.cpu().numpy(), img)
    return view


def _bytes_equal(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    bad = np.flatnonzero(got.reshape(-1).view(np.uint8 if got.dtype == np.uint8 else np.uint32) != want.reshape(-1).view(np.uint8 if want.dtype == np.uint8 else np.uint32))
    print(f"{what}: {want.size} elements, {len(bad)} differ")
    assert len(bad) == 0, (what, bad[:8], got.reshape(-1)[bad[:8]], want.reshape(-1)[bad[:8]])


@pytest.mark.parametrize("name", NAMES)
def test_resize_u8(name):
    from gsrast import images
    img, size = cases.CASES[name]
    d = _dev(img)
    got = images.resize_u8(d, size)
    again = images.resize_u8(d, size)
    assert got.dtype == torch.uint8 and got.device == d.device and got.is_contiguous()
    _bytes_equal(got, _truth(name), name)
    assert torch.equal(got, again), "two runs differ"
    if (size[0], size[1]) == (img.shape[1], img.shape[0]):
        assert got.data_ptr() != d.data_ptr()             # a copy, not the input


@pytest.mark.parametrize("name", cases.GOLDEN)
def test_the_device_equals_what_pillow_returned(name):
    from gsrast import images
    img, size = cases.CASES[name]
    _bytes_equal(images.resize_u8(torch.from_numpy(FIXTURE[f"{name}/in"]).to(DEV), size), FIXTURE[f"{name}/out"], f"{name} (Pillow {FIXTURE['pillow_version']})")


@pytest.mark.parametrize("name", NAMES)
def test_pil_to_torch(name):
    from gsrast import images
    img, size = cases.CASES[name]
    d = _dev(img)
    got = images.pil_to_torch(d, size)
    want = truth.quotients(_truth(name))
    want = np.ascontiguousarray((want[..., None] if want.ndim == 2 else want).transpose(2, 0, 1))
    assert got.is_contiguous()
    _bytes_equal(got, want, name)
    assert torch.equal(got, images.PILtoTorch(d, size)), "two runs differ"


@pytest.mark.parametrize("alpha_mask", (False, True))
@pytest.mark.parametrize("name", COLOUR)
def test_camera_images(name, alpha_mask):
    from gsrast import images
    img, size = cases.CASES[name]
    d = _dev(img)
    got = images.camera_images(d, size, alpha_mask=alpha_mask)
    want = truth.camera_images(img, size, alpha_mask)
    assert (got[2] is None) == (want[2] is None) == (not (alpha_mask and img.shape[2] == 4))
    again = images.camera_images(d, size, alpha_mask=alpha_mask)
    for g, a, w, what in zip(got, again, want, ("original_image", "gray_image", "gt_alpha_mask")):
        if w is not None:
            _bytes_equal(g, np.ascontiguousarray(w), f"{name} {what}")
            assert torch.equal(g, a), "two runs differ"


def test_every_quotient():
    """All 256 values through the float path (a copy-sized call): the correctly rounded v / 255, not v * (1 / 255)."""
    from gsrast import images
    img = np.arange(256, dtype=np.uint8).reshape(16, 16, 1)
    _bytes_equal(images.pil_to_torch(torch.from_numpy(img).to(DEV), (16, 16)), truth.quotients(img).transpose(2, 0, 1).copy(), "quotients")


def test_host_inputs_and_a_view_inside_a_dword():
    from gsrast import images
    img, size = cases.CASES["down_C4"]
    want = _truth("down_C4")
    _bytes_equal(images.resize_u8(img, size, device=DEV), want, "numpy input")
    _bytes_equal(images.resize_u8(torch.from_numpy(img), size, device=DEV), want, "host tensor input")
    buf = torch.empty(img.size + 1, dtype=torch.uint8, device=DEV)
    view = buf[1:].view(img.shape)
    view.copy_(torch.from_numpy(img))
    assert view.data_ptr() % 4 == 1
    _bytes_equal(images.resize_u8(view, size), want, "RGBA view that begins inside a dword")
    flat, fsize = cases.CASES["flat_L"]
    assert images.resize_u8(torch.from_numpy(flat).to(DEV), fsize).shape == (fsize[1], fsize[0])
    Image = pytest.importorskip("PIL.Image")
    _bytes_equal(images.resize_u8(Image.fromarray(img), size, device=DEV), want, "PIL input")
    _bytes_equal(images.PILtoTorch(Image.fromarray(flat), fsize, device=DEV), truth.pil_to_torch(flat, fsize), "PIL mode L")


def test_load_camera_images():
    from gsrast import images
    img = np.random.default_rng(3).integers(0, 256, (5, 1700, 3), dtype=np.uint8)
    size = images.load_resolution(1700, 5, 1.0)
    assert size[1] == 4 and size[0] in (1599, 1600)
    got = images.load_camera_images(torch.from_numpy(img).to(DEV), 1.0)
    want = truth.camera_images(img, size)
    _bytes_equal(got[0], np.ascontiguousarray(want[0]), "original_image")
    _bytes_equal(got[1], np.ascontiguousarray(want[1]), "gray_image")
    assert got[2] is None


def test_on_another_stream_with_a_dependent_operation():
    from gsrast import images
    img, size = cases.CASES["strips_C3"]
    d = torch.from_numpy(img).to(DEV)
    want = images.camera_images(d, size)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        rgb, gray, _ = images.camera_images(d, size)
        total = rgb.double().sum() + gray.double().sum()                  # enqueued behind the call on the same stream
        u8 = images.resize_u8(d, size)
        wide = u8.to(torch.int32)
    s.synchronize()
    assert torch.equal(rgb, want[0]) and torch.equal(gray, want[1])
    assert total.item() == (want[0].double().sum() + want[1].double().sum()).item()
    _bytes_equal(wide.cpu().numpy().astype(np.uint8), _truth("strips_C3"), "resize_u8 on a stream")
