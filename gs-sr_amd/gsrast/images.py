"""The training photographs prepared on the device: Pillow's bicubic resize bit for bit, the division by 255, PGSR's gray image and the alpha mask
(include/gsrast.h, "image preparation"; kernels in csrc/gsr_image.hip).  This is what the reference does on the host for every
camera and every resolution scale: loadCam (gssr/cameras/utils.py:20-54) chooses a size, PILtoTorch (gssr/utils/general_utils.py:21-27) runs
Image.resize and divides by 255, Camera.__init__ (gssr/cameras/__init__.py:59-77) clamps, makes the gray image and applies the mask.

    resize_u8           PIL.Image.resize((W, H)) with its defaults on a uint8 [h,w,C] image: uint8 [H,W,C], the same bytes
    pil_to_torch        PILtoTorch: float32 [C,H,W], every value the correctly rounded v / 255
    camera_images       (original_image [3,H,W], gray_image [1,H,W], gt_alpha_mask [1,H,W] or None) as Camera.__init__ leaves them
    load_resolution     the (W, H) loadCam chooses, operation for operation (host only)
    PILtoTorch          pil_to_torch under the reference's name
    load_camera_images  load_resolution + camera_images: loadCam up to the Camera(...) call

An image is a PIL.Image of mode L, RGB or RGBA, a numpy array or a torch tensor, uint8 [h,w,C] with C = 1, 3, 4 (or [h,w]); Pillow is imported by
nobody here -- an image object brings it along -- so the module imports without it.  Decoding the file stays on the host; host inputs are copied
to the device, strided device tensors are made contiguous.  There is no CPU path: a device that is not a HIP device raises, like gsrast.chamfer.
Host synchronisations per call on a device tensor: 0; launches: 3."""
import numpy as np
import torch

from . import call, lib, scratch

H_STRIP = 256                                             # GSR_IMG_HSTRIP: output columns per workgroup of the horizontal pass
V_STRIP = 256                                             # GSR_IMG_VSTRIP
MODES = {"L": 1, "RGB": 3, "RGBA": 4}


def _is_pil(image):
    return type(image).__module__.split(".")[0] == "PIL" and hasattr(image, "mode")


def _source(image):
    """An image of any accepted kind -> (a uint8 torch tensor [h,w,C] on whatever device it is, whether it came as [h,w]); ValueError for the rest."""
    if _is_pil(image):
        if image.mode not in MODES:
            raise ValueError(f"image mode {image.mode!r} is not offered: L, RGB and RGBA are (Pillow would resample this mode by nearest neighbour)")
        image = np.array(image)
    if isinstance(image, np.ndarray):
        if image.dtype != np.uint8:
            raise ValueError(f"image: expected uint8 but found {image.dtype}")
        t = torch.from_numpy(np.ascontiguousarray(image) if image.flags.writeable else image.copy())
    elif isinstance(image, torch.Tensor):
        if image.dtype != torch.uint8:
            raise ValueError(f"image: expected uint8 but found {image.dtype}")
        t = image.detach()
    else:
        raise ValueError(f"image: expected a PIL image, a numpy array or a torch tensor but found {type(image).__name__}")
    flat = t.dim() == 2
    if flat:
        t = t.unsqueeze(-1)
    if t.dim() != 3 or t.shape[2] not in (1, 3, 4):
        raise ValueError(f"image: expected shape [h, w, C] with C = 1, 3 or 4, or [h, w], but found {list(image.shape)}")
    if t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"image: an empty image of shape {list(image.shape)}")
    if t.numel() >= 1 << 31:
        raise ValueError(f"image: {t.numel()} bytes reach 2^31")
    return t, flat


def _size(size, C):
    try:
        W, H = size
        ok = int(W) == W and int(H) == H
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"size: expected (W, H) as two integers but found {size!r}")
    W, H = int(W), int(H)
    if W < 1 or H < 1:
        raise ValueError(f"size: width and height must be at least 1 but found {(W, H)}")
    if W * H * C >= 1 << 31:
        raise ValueError(f"size: {W * H * C} output bytes reach 2^31")
    return W, H


def _device(t, device):
    """Where the call runs: the tensor's device if it is on one, else `device`; anything but a HIP device raises."""
    dev = t.device if t.is_cuda else torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"gsrast.images has no CPU path: device {str(dev)!r} is not a HIP device")
    return dev


def _resample(image, size, device, u8=False, planes=0, gray=False, mask=False):
    """One gsr_image_resample call -> (out_u8 or None, out_planes or None, out_gray or None, out_mask or None, came as [h,w])."""
    t, flat = _source(image)
    h, w, C = (int(x) for x in t.shape)
    W, H = _size(size, C)
    if (gray and C < 3) or (mask and C != 4) or planes > C:
        raise ValueError(f"image: {C} channel{'s' if C > 1 else ''} cannot give what was asked for (the gray image needs 3, the mask 4)")
    dev = _device(t, device)
    t = t.to(dev).contiguous()
    if C == 4 and t.data_ptr() % 4:                       # a view that begins inside a dword: for 4 channels a pixel is one dword
        t = t.clone()
    new = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)
    out_u8 = new(H, W, C, dtype=torch.uint8) if u8 else None
    out_planes = new(planes, H, W) if planes else None
    out_gray = new(1, H, W) if gray else None
    out_mask = new(1, H, W) if mask else None
    nbytes = int(lib().gsr_image_resample_scratch_bytes(w, h, C, W, H))
    if nbytes == 0:
        raise ValueError(f"gsrast.images: [{h}, {w}, {C}] -> [{H}, {W}]: sizes out of range")
    call("gsr_image_resample", dev, t, w, h, C, w * C, W, H, out_u8, out_planes, planes, out_gray, out_mask, scratch(nbytes, dev), nbytes)
    return out_u8, out_planes, out_gray, out_mask, flat


def resize_u8(image, size, device="cuda"):
    """-> uint8 [H,W,C] ([H,W] for an [h,w] input) on the device: the bytes of PIL.Image.resize((W, H)) with its defaults (bicubic, no box, no
    reducing_gap) on an image of mode L, RGB or RGBA; (W, H) == (w, h) gives a copy.  size is (W, H), Pillow's order."""
    out, _, _, _, flat = _resample(image, size, device, u8=True)
    return out[:, :, 0] if flat else out


def pil_to_torch(image, size, device="cuda"):
    """-> float32 [C,H,W] on the device: the resized image over 255, each value the correctly rounded float32 quotient, what
    torch.from_numpy(np.array(resized)) / 255.0 gives on the host."""
    t, _ = _source(image)
    return _resample(t, size, device, planes=int(t.shape[2]))[1]


PILtoTorch = pil_to_torch


def camera_images(image, size, alpha_mask=False, device="cuda"):
    """-> (original_image [3,H,W], gray_image [1,H,W], gt_alpha_mask [1,H,W] or None), float32 on the device, as Camera.__init__ leaves them for
    an image of 3 or 4 channels: rgb = the quotients clamped to [0,1]; gray = (0.2989 r + 0.587 g) + 0.114 b in float32, every operation rounded,
    of the image BEFORE the mask; original_image = rgb * mask.
    alpha_mask=False is what the reference does for every real image: loadCam tests shape[1] == 4 of a CHW tensor -- the height -- so the alpha
    channel is dropped, the mask is None and the image is multiplied by ones.  alpha_mask=True is what that line means to do for an RGBA image:
    gt_alpha_mask = channel 3 / 255 and original_image = rgb * gt_alpha_mask."""
    t, _ = _source(image)
    if t.shape[2] < 3:
        raise ValueError(f"image: a camera image needs 3 or 4 channels but found {int(t.shape[2])}")
    _, rgb, gray, mask, _ = _resample(t, size, device, planes=3, gray=True, mask=bool(alpha_mask) and t.shape[2] == 4)
    return rgb, gray, mask


def load_resolution(orig_w, orig_h, resolution_scale, input_resolution=-1):
    """-> (W, H) as loadCam lines 23-40 compute it, in the same float64 operations: Python's round (ties to even) of orig / (resolution_scale *
    input_resolution) for input_resolution in {1, 2, 4, 8}; else the integer part of orig / (float(global_down) * float(resolution_scale)), with
    global_down = orig_w / 1600 for a width above 1600 (1 below) where input_resolution is -1 and orig_w / input_resolution otherwise.  The
    quotient of a quotient is why a width of 1601 comes out as 1599 and not 1600."""
    if input_resolution in (1, 2, 4, 8):
        down = resolution_scale * input_resolution
        return round(orig_w / down), round(orig_h / down)
    if input_resolution == -1:
        global_down = orig_w / 1600 if orig_w > 1600 else 1
    else:
        global_down = orig_w / input_resolution
    scale = float(global_down) * float(resolution_scale)
    return int(orig_w / scale), int(orig_h / scale)


def load_camera_images(image, resolution_scale, input_resolution=-1, device="cuda", alpha_mask=False):
    """loadCam up to the Camera(...) call: the size from load_resolution on the image's own, then camera_images."""
    if _is_pil(image):
        w, h = image.size
    else:
        t, _ = _source(image)
        h, w = int(t.shape[0]), int(t.shape[1])
    return camera_images(image, load_resolution(w, h, resolution_scale, input_resolution), alpha_mask=alpha_mask, device=device)
