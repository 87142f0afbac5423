"""Without a GPU: holds tests/images_truth.py, the numpy restatement of the image preparation of include/gsrast.h, to Pillow itself -- the fixture
tests/golden/images_pillow.npz and, where Pillow imports, the live library -- and to the reference's torch expressions on the host; holds
gsrast.images.load_resolution to a table; and checks the argument errors of gsrast.images, which are raised before the library is touched."""
import os

import numpy as np
import pytest
import torch

import abi_header
import images_cases as cases
import images_truth as truth
from gsrast import images

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = np.load(os.path.join(ROOT, "tests", "golden", "images_pillow.npz"))


def _pillow(img, size):
    from PIL import Image
    flat = img.ndim == 2 or img.shape[2] == 1
    out = np.array(Image.fromarray(np.ascontiguousarray(img.reshape(img.shape[:2]) if flat else img)).resize(size))
    return out.reshape(out.shape[:2] + (1,)) if flat and img.ndim == 3 else out


def test_the_fixture_holds_every_small_case():
    assert str(FIXTURE["pillow_version"])
    assert len(cases.GOLDEN) >= 20
    for name in cases.GOLDEN:
        img, size = cases.CASES[name]
        assert np.array_equal(FIXTURE[f"{name}/in"], img) and tuple(FIXTURE[f"{name}/size"]) == size, name
        assert FIXTURE[f"{name}/out"].shape[:2] == (size[1], size[0]), name


@pytest.mark.parametrize("name", cases.GOLDEN)
def test_truth_equals_the_fixture(name):
    img, size = cases.CASES[name]
    assert np.array_equal(truth.resize(img, size), FIXTURE[f"{name}/out"])


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_truth_equals_live_pillow(name):
    pytest.importorskip("PIL")
    img, size = cases.CASES[name]
    assert np.array_equal(truth.resize(img, size), _pillow(img, size))


def test_truth_equals_live_pillow_on_random_sizes():
    pytest.importorskip("PIL")
    n = 0
    for img, size in cases.random_pairs(50, seed=0):
        assert np.array_equal(truth.resize(img, size), _pillow(img, size)), (img.shape, size)
        n += 1
    assert n == 50


def test_the_cases_reach_what_they_are_named_for():
    for C in (1, 3, 4):
        img, size = cases.CASES[f"clip_C{C}"]
        _, sums = truth.resize(img, size, sums=True)
        for which in ("h", "v"):
            s = sums[which] >> truth.PRECISION_BITS
            print(f"clip_C{C} {which}: unclipped range [{s.min()}, {s.max()}]")
            assert s.min() < 0 and s.max() > 255, (C, which)
    img, size = cases.CASES["alpha_columns_C4"]
    a = truth.resize(img, size)[..., 3]
    assert (a == 0).any() and (a == 255).any() and ((a > 0) & (a < 255)).any()
    assert not cases.CASES["strided_C3"][0].flags.c_contiguous
    taps = lambda name, axis: max(len(k) for _, k in truth.coefficients(cases.CASES[name][0].shape[axis], cases.CASES[name][1][1 - axis]))
    assert taps("taps_401_C3", 1) == 300 and taps("up_C3", 1) <= 5 and taps("taps_chunks_C3", 1) > 4096
    img, size = cases.CASES["copy_C4"]
    assert np.array_equal(truth.resize(img, size), img)                  # a copy: no premultiplied round trip


def test_quotients_and_gray_equal_the_references_torch_expressions():
    v = np.arange(256, dtype=np.uint8)
    want = (torch.from_numpy(v) / 255.0).numpy()                          # PILtoTorch, general_utils.py:23
    assert want.dtype == np.float32 and np.array_equal(truth.quotients(v).view(np.uint32), want.view(np.uint32))
    by_reciprocal = v.astype(np.float32) * (np.float32(1.0) / np.float32(255.0))
    print("values where a product with the float32 reciprocal differs:", int((by_reciprocal != want).sum()))
    assert (by_reciprocal != want).sum() == 126
    r = np.random.default_rng(5)
    rgb = truth.quotients(r.integers(0, 256, (3, 64, 96), dtype=np.uint8))
    t = torch.from_numpy(rgb)
    want = (0.2989 * t[0] + 0.587 * t[1] + 0.114 * t[2]).unsqueeze(0).numpy()      # torchvision's rgb_to_grayscale, which transforms.Grayscale() calls
    assert np.array_equal(truth.gray(rgb).view(np.uint32), want.view(np.uint32))
    try:
        import torchvision.transforms as transforms
    except Exception:
        return
    assert np.array_equal(transforms.Grayscale()(t).numpy().view(np.uint32), truth.gray(rgb).view(np.uint32))


def test_camera_images_of_the_truth_are_the_references_steps():
    """Camera.__init__ lines 59-77 in torch on the host, on the truth's resized bytes, with the mask loadCam means to pass and with none."""
    img, size = cases.CASES["alpha_columns_C4"]
    chw = torch.from_numpy(truth.resize(img, size)) / 255.0
    chw = chw.permute(2, 0, 1)
    for alpha_mask in (False, True):
        original = chw[:3].clamp(0.0, 1.0).clone()
        g = (0.2989 * original[0] + 0.587 * original[1] + 0.114 * original[2]).unsqueeze(0)
        original *= chw[3:4] if alpha_mask else torch.ones((1,) + tuple(original.shape[1:]))
        rgb, gray, mask = truth.camera_images(img, size, alpha_mask)
        assert np.array_equal(rgb.view(np.uint32), original.numpy().view(np.uint32)) and np.array_equal(gray.view(np.uint32), g.numpy().view(np.uint32))
        assert (mask is None) == (not alpha_mask) and (mask is None or np.array_equal(mask, chw[3:4].numpy()))


RESOLUTIONS = [                                            # (orig_w, orig_h, resolution_scale, input_resolution) -> (W, H)
    ((5472, 3648, 1.0, -1), (1600, 1066)),
    ((1601, 1000, 1.0, -1), (1599, 999)),
    ((1600, 1200, 1.0, -1), (1600, 1200)),
    ((1001, 667, 1.0, 2), (500, 334)),
    ((1003, 669, 1.0, 2), (502, 334)),
    ((5472, 3648, 2.0, -1), (800, 533)),
    ((6000, 4000, 1.0, 1024), (1024, 682)),
    ((4000, 3000, 1.0, -1), (1600, 1200)),
    ((1920, 1080, 1.0, -1), (1600, 900)),
    ((1920, 1080, 1, 1), (1920, 1080)),
    ((1920, 1080, 2.0, 4), (240, 135)),
]


@pytest.mark.parametrize("args,want", RESOLUTIONS)
def test_load_resolution(args, want):
    got = images.load_resolution(*args)
    assert got == want and all(type(x) is int for x in got)


def test_load_resolution_float64_quotients():
    """orig_w / (orig_w / 1600) is not always 1600.0: the integer part is 1599 for 464 of the widths 1601..8000, and 1601 is one of them."""
    short = [w for w in range(1601, 8001) if images.load_resolution(w, 1000, 1.0)[0] == 1599]
    assert all(images.load_resolution(w, 1000, 1.0)[0] in (1599, 1600) for w in range(1601, 8001))
    assert len(short) == 464 and short[0] == 1601


def test_constants_equal_the_header():
    consts = abi_header.constants(abi_header.source("gsrast.h"))
    assert images.H_STRIP == consts["GSR_IMG_HSTRIP"] and images.V_STRIP == consts["GSR_IMG_VSTRIP"]


def test_the_module_does_not_import_pillow():
    src = open(images.__file__).read()
    assert "import PIL" not in src and "from PIL" not in src


def test_argument_errors_need_no_device():
    ok = np.zeros((5, 6, 3), dtype=np.uint8)
    for bad, match in ((ok.astype(np.float32), "uint8"), (torch.zeros(5, 6, 3), "uint8"), (np.zeros((5, 6, 2), np.uint8), "shape"), (np.zeros(5, np.uint8), "shape"),
                       (np.zeros((1, 5, 6, 3), np.uint8), "shape"), (np.zeros((0, 6, 3), np.uint8), "empty"), ([[1, 2]], "PIL image, a numpy array")):
        for fn in (images.resize_u8, images.pil_to_torch, images.PILtoTorch):
            with pytest.raises(ValueError, match=match):
                fn(bad, (4, 4))
    for size in ((0, 4), (4, -1), (4,), 4, (2.5, 4), (1 << 20, 1 << 20)):
        with pytest.raises(ValueError, match="size"):
            images.resize_u8(ok, size)
    with pytest.raises(ValueError, match="3 or 4 channels"):
        images.camera_images(ok[..., :1], (4, 4))
    with pytest.raises(ValueError, match="3 or 4 channels"):
        images.load_camera_images(ok[..., 0], 1.0)
    for device in ("cpu", torch.device("cpu")):
        with pytest.raises(RuntimeError, match="no CPU path"):
            images.resize_u8(ok, (4, 4), device=device)
        with pytest.raises(RuntimeError, match="no CPU path"):
            images.camera_images(ok, (4, 4), device=device)


def test_pillow_modes_that_are_not_offered():
    Image = pytest.importorskip("PIL.Image")
    for mode in ("P", "1", "I;16", "F", "LA", "CMYK"):
        with pytest.raises(ValueError, match=f"mode '{mode}'"):
            images.PILtoTorch(Image.new(mode, (6, 5)), (3, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):           # an accepted mode gets as far as the device
        images.PILtoTorch(Image.new("RGB", (6, 5)), (3, 3), device="cpu")


def test_entry_point_argument_errors_without_a_device():
    """gsr_image_resample refuses bad sizes, strides, alignments, output combinations and a short scratch before it launches anything."""
    import ctypes as C
    import gsrast
    L = gsrast.lib()
    assert L.gsr_image_resample_scratch_bytes(37, 23, 3, 16, 10) > 0
    for bad in ((0, 23, 3, 16, 10), (37, 23, 2, 16, 10), (37, 23, 3, 0, 10), (1 << 16, 1 << 15, 1, 4, 4), (4, 4, 3, 1 << 15, 1 << 15)):
        assert L.gsr_image_resample_scratch_bytes(*bad) == 0, bad
    buf = (C.c_uint8 * 4096)()
    addr = (C.addressof(buf) + 15) & ~15
    need = L.gsr_image_resample_scratch_bytes(8, 8, 4, 4, 4)

    def run(w=8, h=8, ch=4, stride=32, image=addr, planes=0, gray=None, mask=None, scratch_bytes=need):
        return L.gsr_image_resample(image, w, h, ch, stride, 4, 4, addr, addr if planes else None, planes, gray, mask, addr, scratch_bytes, None)
    for kw, text in ((dict(ch=2), "channels"), (dict(w=0), "sizes"), (dict(stride=31), "row stride"), (dict(image=addr + 1), "multiples of 4"),
                     (dict(stride=34), "multiples of 4"), (dict(planes=5), "planes"), (dict(ch=1, stride=8, gray=addr), "gray"),
                     (dict(ch=3, stride=24, mask=addr), "mask"), (dict(planes=4, mask=addr), "mask"), (dict(scratch_bytes=need - 1), "scratch"),
                     (dict(image=None), "null")):
        assert run(**kw) != 0 and text in gsrast.last_error(), (kw, gsrast.last_error())
