"""A numpy restatement of the image preparation of include/gsrast.h ("image preparation"), written from that definition: Pillow's 8-bit bicubic
resize as a float64 coefficient table and two integer passes, the premultiplied alpha of RGBA, the division by 255, PGSR's gray image, the mask.
Every floating-point operation is a numpy / Python float64 or float32 operation of its own; the sums of the weights run in ascending order in a
loop (np.sum adds pairwise).  resize() also returns each pass's sums before they are shifted and clipped."""
import numpy as np

PRECISION_BITS = 22


def bicubic(t):
    t = abs(t)
    if t < 1.0:
        return ((1.5 * t - 2.5) * t) * t + 1.0
    if t < 2.0:
        return (((t - 5.0) * t + 8.0) * t - 4.0) * -0.5
    return 0.0


def coefficients(in_size, out_size):
    """-> [(xmin, k int64 [n])] per output coordinate of one axis."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ss = 1.0 / fs
    rows = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        w = [bicubic(((x + xmin) - center + 0.5) * ss) for x in range(xmax - xmin)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        k = [int(v * float(1 << PRECISION_BITS) + 0.5) if v >= 0 else int(v * float(1 << PRECISION_BITS) - 0.5) for v in w]      # int() truncates toward zero
        rows.append((xmin, np.array(k, dtype=np.int64)))
    return rows


def pass_sums(img, out_size, axis):
    """The sums (1 << 21) + sum k * pixel of one pass along `axis` (0: vertical, 1: horizontal) of a uint8 [h,w,C] image, int64, unclipped."""
    rows = coefficients(img.shape[axis], out_size)
    src = np.moveaxis(img.astype(np.int64), axis, 0)
    out = np.empty((out_size,) + src.shape[1:], dtype=np.int64)
    for xx, (xmin, k) in enumerate(rows):
        out[xx] = (src[xmin:xmin + len(k)] * k.reshape((-1,) + (1,) * (src.ndim - 1))).sum(axis=0) + (1 << (PRECISION_BITS - 1))
    assert np.abs(out).max() < 1 << 31, "a sum leaves the signed 32-bit accumulator"
    return np.moveaxis(out, 0, axis)


def clip8(sums):
    return np.clip(sums >> PRECISION_BITS, 0, 255).astype(np.uint8)


def premultiply(img):
    out = img.copy()
    a = img[..., 3].astype(np.int64)
    for c in range(3):
        t = img[..., c].astype(np.int64) * a + 128
        out[..., c] = ((t >> 8) + t) >> 8
    return out


def unpremultiply(img):
    out = img.copy()
    a = img[..., 3].astype(np.int64)
    keep = (a == 0) | (a == 255)
    div = np.where(keep, 1, a)
    for c in range(3):
        out[..., c] = np.where(keep, img[..., c], np.minimum(255 * img[..., c].astype(np.int64) // div, 255))
    return out


def resize(img, size, sums=False):
    """PIL.Image.resize((W, H)) on a uint8 [h,w,C] (or [h,w]) image -> uint8 [H,W,C] ([H,W]); with sums=True also {"h": ..., "v": ...}, the
    unclipped sums of the passes that ran."""
    img = np.asarray(img)
    assert img.dtype == np.uint8
    flat = img.ndim == 2
    x = img[..., None] if flat else img
    h, w, C = x.shape
    W, H = size
    seen = {}
    if (W, H) == (w, h):
        out = x.copy()
    else:
        out = premultiply(x) if C == 4 else x
        if W != w:
            seen["h"] = pass_sums(out, W, 1)
            out = clip8(seen["h"])
        if H != h:
            seen["v"] = pass_sums(out, H, 0)
            out = clip8(seen["v"])
        if C == 4:
            out = unpremultiply(out)
    out = out[..., 0] if flat else out
    return (out, seen) if sums else out


def quotients(u8):
    """v / 255 as the correctly rounded float32 quotient."""
    return np.asarray(u8).astype(np.float32) / np.float32(255.0)


def pil_to_torch(img, size):
    out = resize(img, size)
    out = out[..., None] if out.ndim == 2 else out
    return np.ascontiguousarray(quotients(out).transpose(2, 0, 1))


def gray(rgb):
    """float32 [3,H,W] -> [1,H,W]: (0.2989 r + 0.587 g) + 0.114 b, every product and sum a float32 operation."""
    g = (np.float32(0.2989) * rgb[0] + np.float32(0.587) * rgb[1]) + np.float32(0.114) * rgb[2]
    assert g.dtype == np.float32
    return g[None]


def camera_images(img, size, alpha_mask=False):
    """-> (original_image [3,H,W], gray_image [1,H,W], gt_alpha_mask [1,H,W] or None)."""
    chw = pil_to_torch(img, size)
    rgb = np.clip(chw[:3], np.float32(0.0), np.float32(1.0))
    g = gray(rgb)
    if alpha_mask and chw.shape[0] == 4:
        mask = chw[3:4]
        return rgb * mask, g, mask
    return rgb * np.ones((1,) + rgb.shape[1:], dtype=np.float32), g, None
