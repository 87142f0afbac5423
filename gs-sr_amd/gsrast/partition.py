"""The VastGaussian scene split, on the device (include/gsrast.h "scene partition", csrc/gsr_partition.hip).

Replaces what split_scene.py:39-53 runs through gssr/utils/vastgaussian_utils.py:89-286 with one Python loop over every point, image and id per tile,
a scipy hull and a shapely intersection per (tile, image), and distCUDA2 called from inside the loop:

    point_tiles, tile_z_range, visibility, coverage      tensors in, tensors out, one status word per op, a fixed number of host reads
    partition_tensors                                     steps 2 to 4 in a row on tensors
    camera_position_based_region_division, position_based_data_selection, visibility_based_camera_selection, coverage_based_point_selection
                                                          the reference's names, arguments (its keyword `threshod` included) and structures
    partition_scene, write_box                            the four steps in a row; box.txt byte for byte as split_scene.py:70-73

A tile mask is W = ceil(T / 32) int32 words per row: bit t & 31 of word t >> 5 says "in tile t".  At most 1024 tiles (GSR_PART_MAX_TILES: the boxes
and their counters are held in LDS).  Step 1 -- which cameras found a tile -- stays numpy on the host: C log C on a few thousand centres, and it needs
Python's stable order.  Camera centres are np.linalg.inv(w2c)[:3, -1] exactly as the reference's get_cam_center, not -R^T t: a camera on the edge of the
box that was made from its own centre must compare equal.

Deviations.  Where the reference crashes, a RuntimeError names the cause: fewer than four points in a tile's box or no distance inside the 3-sigma band
(an empty .min()), a non-finite coordinate (a NaN threshold), a box corner with camera-space z exactly 0 or a non-finite projection (a Qhull error), a
point id that a tile's image observes and points3D lacks (KeyError).  One result differs: a hull of zero area (all eight projections collinear) gives
ratio 0 here and a QhullError in the reference.  The 3-sigma thresholds are float64 here and float32 in numpy: a distance within a relative 1e-6 of a
threshold may fall on the other side."""
import ctypes as C

import numpy as np
import torch

from . import call, lib, raise_status, scratch, status_text, typed_tensor as _tensor

ERR_FEW, ERR_NONFINITE, ERR_ZERO_Z, ERR_ABSENT, ERR_TABLE, ERR_OFFSETS, ERR_COUNT = 1, 2, 4, 8, 16, 32, 64
MAX_TILES = 1024                                          # GSR_PART_MAX_TILES
BLOCK = 256                                               # GSR_PART_BLOCK: points per workgroup of the box pass
PINHOLE_ASSERT = "Colmap camera model not handled: only undistorted datasets (PINHOLE or SIMPLE_PINHOLE cameras) supported!"


STATUS = {
    ERR_FEW: "a tile has fewer than four points in its box, or no point's neighbour distance lies inside mean +- 3 std (the reference fails on an empty min())",
    ERR_NONFINITE: "a non-finite value: a box bound, a point coordinate (as float32), a 3-sigma threshold or a term of a projection is NaN or infinite",
    ERR_ZERO_Z: "a box corner has camera-space z exactly 0 (the reference gets a Qhull error)",
    ERR_ABSENT: "a point id that an image of a tile observes is absent from the point table (the reference's KeyError)",
    ERR_TABLE: "point_ids does not ascend strictly",
    ERR_OFFSETS: "obs_offsets does not ascend from 0 to len(obs_ids)",
    ERR_COUNT: "counts does not hold the number of bits of mask",
}


def status_message(op, status):
    """The text of a status word of the scene partition."""
    return status_text(op, status, STATUS)


def _tiles(T, op):
    if T < 1 or T > MAX_TILES:
        raise RuntimeError(f"{op}: {T} tiles out of range [1, {MAX_TILES}] (the boxes and their counters are held in LDS)")
    return (T + 31) // 32


def _raise(op, status):
    raise_status(op, int(status.item()) & 0xFFFFFFFF, STATUS)      # the host read


# ---------------------------------------------------------------------------------------------------------------- tensor level
def point_tiles(xy, boxes):
    """-> (mask int32 [N,W], counts int32 [T]): the tiles whose box holds each row, and the rows per tile.

    xy float64 [N,2] or [N,3] (x, y are the first two columns; points and camera centres alike), boxes float64 [T,4] = (mx, Mx, my, My), T <= 1024.
    Bounds are inside, compared in float64; a NaN coordinate is in no tile; a NaN bound raises.  One pass over the rows whatever T.
    Exactly one host synchronisation: the status word."""
    op = "point_tiles"
    if not isinstance(xy, torch.Tensor) or xy.dim() != 2 or xy.shape[1] not in (2, 3):
        raise RuntimeError(f"xy: expected a tensor of shape ['*', 2] or ['*', 3] but found {list(getattr(xy, 'shape', []))}")
    xy = _tensor(xy, "xy", torch.float64, (None, xy.shape[1]))
    bx = _tensor(boxes, "boxes", torch.float64, (None, 4), xy.device)
    N, T = xy.shape[0], bx.shape[0]
    W = _tiles(T, op)
    dev = xy.device
    mask = torch.empty(N, W, dtype=torch.int32, device=dev)
    counts = torch.empty(T, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    call("gsr_partition_boxes", dev, xy if N else None, N, xy.shape[1], bx, T, mask if N else None, counts, status, what=op)
    _raise(op, status)
    return mask, counts


def tile_z_range(xyz, mask, counts):
    """-> (zrange float32 [T,2] = (mz, Mz), stats float64 [T,2] = (mean, std) of the neighbour distances).

    xyz float64 [N,3]; mask, counts: point_tiles' results for these rows.  Per tile: the float32 xyz of its rows, distCUDA2 on that subset, the
    population std and mean in float64 (a fixed order: two calls give the same bits), and min / max of float32 z over mean - 3 std < dist < mean + 3 std.
    Raises where the reference crashes: fewer than four rows in a tile or none inside the band, a non-finite coordinate.
    Exactly two host synchronisations, whatever N and T: the counts (they size the per-tile nearest-neighbour calls) and the status word."""
    op = "tile_z_range"
    xyz = _tensor(xyz, "xyz", torch.float64, (None, 3))
    dev = xyz.device
    N = xyz.shape[0]
    cnt = _tensor(counts, "counts", torch.int32, (None,), dev)
    T = cnt.shape[0]
    W = _tiles(T, op)
    mask = _tensor(mask, "mask", torch.int32, (N, W), dev)
    L = lib()
    zrange = torch.zeros(T, 2, dtype=torch.float32, device=dev)
    stats = torch.zeros(T, 2, dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    host = [int(c) & 0xFFFFFFFF for c in cnt.cpu().tolist()]      # host read 1
    n_max = max(host)
    if n_max > N:
        raise RuntimeError(status_message(op, ERR_COUNT))
    nbytes = int(L.gsr_partition_zrange_scratch_bytes(N, n_max))
    work = scratch(nbytes, dev)
    for t, n in enumerate(host):
        call("gsr_partition_zrange", dev, xyz if N else None, N, mask if N else None, T, t, n, n_max, zrange, stats, work, nbytes, status, what=op)
    _raise(op, status)                                # host read 2
    return zrange, stats


def visibility(boxes, zrange, w2c, centers, intr, member, threshold):
    """-> (ratio float64 [T,C], dist float64 [T,C], md float64 [T], add uint8 [T,C]).

    boxes float64 [T,4] (NOT expanded), zrange float32 [T,2], w2c float64 [C,3,4] (the rows [R | t]), centers float64 [C,3], intr float64 [C,4] =
    (fx, fy, width, height), member int32 [C,W]: the tile mask of the images (point_tiles on the centres with the expanded boxes).
    ratio = area(hull of the eight projected box corners, cut to the image) / (width height), the principal point at the image's middle and corners
    behind the camera mirrored, as in the reference; dist = the mean L1 distance from the centre to the corners; md = 1.2 x the mean over the tile's
    members of the largest Euclidean corner distance (NaN for a tile without members: nothing is added); add = ratio > threshold and dist < md and
    the image is no member.  A hull of zero area gives ratio 0.  Raises on a corner with camera-space z exactly 0 and on non-finite terms.
    Exactly one host synchronisation: the status word."""
    op = "visibility"
    bx = _tensor(boxes, "boxes", torch.float64, (None, 4))
    dev = bx.device
    T = bx.shape[0]
    W = _tiles(T, op)
    zr = _tensor(zrange, "zrange", torch.float32, (T, 2), dev)
    cen = _tensor(centers, "centers", torch.float64, (None, 3), dev)
    Cn = cen.shape[0]
    if Cn < 1:
        raise RuntimeError(f"{op}: expected at least one image")
    E = _tensor(w2c, "w2c", torch.float64, (Cn, 3, 4), dev)
    K = _tensor(intr, "intr", torch.float64, (Cn, 4), dev)
    mem = _tensor(member, "member", torch.int32, (Cn, W), dev)
    threshold = float(threshold)
    if not np.isfinite(threshold):
        raise RuntimeError(f"{op}: threshold must be finite")
    ratio = torch.empty(T, Cn, dtype=torch.float64, device=dev)
    dist = torch.empty(T, Cn, dtype=torch.float64, device=dev)
    md = torch.empty(T, dtype=torch.float64, device=dev)
    add = torch.empty(T, Cn, dtype=torch.uint8, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    call("gsr_partition_visibility", dev, bx, zr, T, E, cen, K, Cn, mem, threshold, ratio, dist, md, add, status, what=op)
    _raise(op, status)
    return ratio, dist, md, add


def pack_mask(flags):
    """uint8 / bool [T,C] -> the tile mask int32 [C,W] (on the device, no host read)."""
    T, Cn = flags.shape
    W = (T + 31) // 32
    bits = torch.zeros(Cn, W * 32, dtype=torch.int64, device=flags.device)
    bits[:, :T] = flags.t().to(torch.int64)
    words = (bits.view(Cn, W, 32) << torch.arange(32, device=flags.device, dtype=torch.int64)).sum(dim=2)
    return torch.where(words >= (1 << 31), words - (1 << 32), words).to(torch.int32)


def coverage(obs_offsets, obs_ids, image_mask, point_ids, num_tiles):
    """-> (tile_offsets int64 [T + 1] on the HOST, rows int64 [tile_offsets[T]]): tile t's points are rows[tile_offsets[t]:tile_offsets[t + 1]] of the
    point table, ascending -- the order np.unique gives the ids.

    obs_ids int64 [M]: the images' point ids one image after the other (-1: none; repeats allowed), image a in [obs_offsets[a], obs_offsets[a + 1]),
    obs_offsets int64 [C + 1]; image_mask int32 [C,W]: the tiles of each image; point_ids int64 [Np] ascending strictly (any int64: no 32-bit limit).
    Raises when an image of at least one tile observes an id that point_ids lacks (the reference's KeyError); the ids of an image of no tile are never
    looked up.  Exactly one host synchronisation: the per-tile counts and the status word, read together."""
    op = "coverage"
    T = int(num_tiles)
    W = _tiles(T, op)
    off = _tensor(obs_offsets, "obs_offsets", torch.int64, (None,))
    dev = off.device
    Cn = off.shape[0] - 1
    if Cn < 1:
        raise RuntimeError(f"{op}: expected at least one image")
    ids = _tensor(obs_ids, "obs_ids", torch.int64, (None,), dev)
    im = _tensor(image_mask, "image_mask", torch.int32, (Cn, W), dev)
    pid = _tensor(point_ids, "point_ids", torch.int64, (None,), dev)
    M, Np = ids.shape[0], pid.shape[0]
    L = lib()
    pmask = torch.empty(Np, W, dtype=torch.int32, device=dev)
    rec = torch.empty(T + 1, dtype=torch.int32, device=dev)      # counts, then the status word
    call("gsr_partition_coverage_mask", dev, off, ids if M else None, M, im, Cn, pid if Np else None, Np, T, pmask if Np else None, rec, rec[T:], what=op)
    host = [int(v) & 0xFFFFFFFF for v in rec.cpu().tolist()]      # the one host read
    raise_status(op, host[T], STATUS)
    offsets = np.zeros(T + 1, np.int64)
    np.cumsum(host[:T], out=offsets[1:])
    rows = torch.empty(int(offsets[T]), dtype=torch.int64, device=dev)
    nbytes = int(L.gsr_partition_coverage_rows_scratch_bytes(Np))
    work = scratch(nbytes, dev)
    call("gsr_partition_coverage_rows", dev, pmask if Np else None, Np, T, offsets.ctypes.data_as(C.POINTER(C.c_int64)), rows if offsets[T] else None,
         work, nbytes, what=op)
    return torch.from_numpy(offsets), rows


def partition_tensors(boxes, centers, w2c, intr, xyz, obs_offsets, obs_ids, point_ids, ratio=0.2, threshold=0.25):
    """Steps 2 to 4 in a row at the tensor level, for step 1's boxes float64 [T,4]: -> dict(member int32 [C,W] (the images inside the expanded boxes),
    in_box int32 [N,W] and in_box_counts int32 [T] (the points inside them), zrange, stats, ratio, dist, md, add (visibility's results),
    image_mask int32 [C,W] (members and added images), tile_offsets int64 [T + 1] on the host and rows int64 (coverage's CSR into point_ids)).
    centers, w2c, intr: per image as for visibility; xyz float64 [N,3] in any order; point_ids ascending strictly.
    Six host synchronisations whatever N, M, C and T: 1 + 1 (the two box passes) + 2 (z-range) + 1 (visibility) + 1 (coverage)."""
    bx = _tensor(boxes, "boxes", torch.float64, (None, 4))
    dw = (bx[:, 1] - bx[:, 0]) * float(ratio) / 2.0           # the reference's expression, operation by operation
    dh = (bx[:, 3] - bx[:, 2]) * float(ratio) / 2.0
    grown = torch.stack([bx[:, 0] - dw, bx[:, 1] + dw, bx[:, 2] - dh, bx[:, 3] + dh], dim=1)
    member, _ = point_tiles(centers, grown)
    in_box, counts = point_tiles(xyz, grown)
    zrange, stats = tile_z_range(xyz, in_box, counts)
    vis_ratio, dist, md, add = visibility(bx, zrange, w2c, centers, intr, member, threshold)
    image_mask = member | pack_mask(add)
    tile_offsets, rows = coverage(obs_offsets, obs_ids, image_mask, point_ids, bx.shape[0])
    return dict(member=member, in_box=in_box, in_box_counts=counts, zrange=zrange, stats=stats, ratio=vis_ratio, dist=dist, md=md, add=add, image_mask=image_mask,
                tile_offsets=tile_offsets, rows=rows)


# ---------------------------------------------------------------------------------------------------------------- the reference's structures
def _rotmat(q):
    w, x, y, z = (np.float64(v) for v in q)
    return np.array([[1 - 2 * y**2 - 2 * z**2, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
                     [2 * x * y + 2 * w * z, 1 - 2 * x**2 - 2 * z**2, 2 * y * z - 2 * w * x],
                     [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x**2 - 2 * y**2]])


def w2c_matrix(extr):
    """The 4x4 world-to-camera matrix of an image (.qvec, real part first, and .tvec)."""
    m = np.zeros((4, 4))
    m[:3, :3] = _rotmat(extr.qvec)
    m[:3, -1] = np.array(extr.tvec)
    m[3, 3] = 1.0
    return m


def cam_center(extr):
    """np.linalg.inv(w2c)[:3, -1], as the reference's get_cam_center."""
    return np.linalg.inv(w2c_matrix(extr))[:3, -1]


def _box_of(centers):
    c = np.vstack(centers)
    return np.array([np.min(c[:, 0]), np.max(c[:, 0]), np.min(c[:, 1]), np.max(c[:, 1])])


def camera_position_based_region_division(images, num_col=None, num_row=None, max_num_images=150):
    """The reference's step 1 (vastgaussian_utils.py:89-147), on the host.  images: {id: image}.  -> [{"images": [{"image": image, "center": centre}, ...],
    "box": float64 [mx, Mx, my, My]}, ...].  Quadtree mode (num_col or num_row None): halves along the longer x / y extent of the centres (equal
    extents: y), in Python's stable sorted order, until a half has fewer than max_num_images images.  Grid mode: num_col columns by x, each cut into
    num_row tiles by y, with the reference's integer-division slices: the images left over at the end of a column or row belong to no tile."""
    items = [{"image": img, "center": cam_center(img)} for img in images.values()]
    tiles = []
    if num_col is None or num_row is None:
        if int(max_num_images) < 2:
            raise RuntimeError(f"camera_position_based_region_division: max_num_images must be at least 2, not {max_num_images} (the halving would never end)")
        if not items:
            raise RuntimeError("camera_position_based_region_division: expected at least one image")
        def split(part):                                  # depth log2(C); the lower half's subtree comes before the upper half's
            mx, Mx, my, My = _box_of([it["center"] for it in part])
            axis = 0 if (Mx - mx) > (My - my) else 1
            srt = sorted(part, key=lambda it: it["center"][axis])
            for half in (srt[:len(srt) // 2], srt[len(srt) // 2:]):
                if len(half) < max_num_images:
                    tiles.append(half)
                else:
                    split(half)
        split(items)
    else:
        num_col, num_row = int(num_col), int(num_row)
        if num_col < 1 or num_row < 1:
            raise RuntimeError(f"camera_position_based_region_division: num_col and num_row must be positive, not {num_col} and {num_row}")
        n = len(items)
        per_col = n // num_col
        srt = sorted(items, key=lambda it: it["center"][0])
        for i in range(num_col):
            col = srt[i * per_col:((i + 1) * per_col if (i + 1) * per_col < n else n)]
            per_tile = len(col) // num_row
            cs = sorted(col, key=lambda it: it["center"][1])
            for j in range(num_row):
                tiles.append(cs[j * per_tile:((j + 1) * per_tile if (j + 1) * per_tile < len(col) else len(col))])
    for k, tile in enumerate(tiles):
        if not tile:
            raise RuntimeError(f"camera_position_based_region_division: tile {k} is empty (fewer images than tiles in a column or row)")
    return [{"images": tile, "box": _box_of([it["center"] for it in tile])} for tile in tiles]


def _on(device, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _members(mask_cpu, t):
    """The rows of a host tile mask [n,W] with bit t, ascending."""
    return np.nonzero((mask_cpu[:, t >> 5] >> (t & 31)) & 1)[0]


def _host_mask(rows_per_tile, n):
    """int32 [n,W] from per-tile row lists."""
    T = len(rows_per_tile)
    m = np.zeros((n, (T + 31) // 32), np.uint32)
    for t, rows in enumerate(rows_per_tile):
        if len(rows):
            m[np.asarray(rows, np.int64), t >> 5] |= np.uint32(1 << (t & 31))
    return m.view(np.int32)


def _expanded(boxes, ratio):
    out = []
    for mx, Mx, my, My in boxes:
        dw = (Mx - mx) * ratio / 2.0
        dh = (My - my) * ratio / 2.0
        out.append(np.array([mx - dw, Mx + dw, my - dh, My + dh]))
    return np.array(out, np.float64).reshape(-1, 4)


def position_based_data_selection(tiles, images, points3D, ratio=0.2, device="cuda"):
    """The reference's step 2 (vastgaussian_utils.py:150-178): every tile's box grows by ratio / 2 of its width and height per side; the tile gets the
    images whose centre and the points whose x, y lie inside (bounds included, float64), each in the order of its dict, and KEEPS its un-expanded box.
    -> [{"images": [image, ...], "box": box, "points3D": [point, ...]}, ...].  Two box passes on the device (centres, points): two host
    synchronisations, plus one copy of each mask to the host to build the lists."""
    if not tiles:
        return []
    boxes = _expanded([np.asarray(t["box"], np.float64) for t in tiles], ratio)
    imgs, pts = list(images.values()), list(points3D.values())
    cen = np.array([cam_center(i) for i in imgs], np.float64).reshape(-1, 3)
    xyz = np.array([np.asarray(p.xyz, np.float64).reshape(3) for p in pts], np.float64).reshape(-1, 3)
    bx = _on(device, boxes)
    im_mask = point_tiles(_on(device, cen), bx)[0].cpu().numpy()
    pt_mask = point_tiles(_on(device, xyz), bx)[0].cpu().numpy()
    return [{"images": [imgs[i] for i in _members(im_mask, t)], "box": tile["box"], "points3D": [pts[i] for i in _members(pt_mask, t)]}
            for t, tile in enumerate(tiles)]


def _intrinsics(intr):
    if intr.model == "SIMPLE_PINHOLE":
        fx = fy = intr.params[0]
    elif intr.model == "PINHOLE":
        fx, fy = intr.params[0], intr.params[1]
    else:
        assert False, PINHOLE_ASSERT
    return [float(fx), float(fy), float(intr.width), float(intr.height)]


def visibility_based_camera_selection(tiles, images, cameras, threshod=0.25, device="cuda", return_tensors=False):
    """The reference's step 3 (vastgaussian_utils.py:216-271), its misspelled keyword included.  Per tile: the z-range of its points3D (3-sigma filter on
    distCUDA2 of the float32 subset), the eight corners of (box, z-range), and every image of `images` that is not in the tile is added when the hull
    of the projected corners covers more than `threshod` of the image and its mean L1 corner distance is below md.  New images go in front of the
    tile's own, in the order of `images`.  Every image's camera model is checked (the reference asserts only on the images it projects).
    tile_z_range and visibility on the device: three host synchronisations, plus one copy of the decisions to the host.
    return_tensors: also the dict of device results (zrange, stats, ratio, dist, md, add)."""
    if not tiles:
        return ([], {}) if return_tensors else []
    imgs = list(images.values())
    index = {img.id: k for k, img in enumerate(imgs)}
    members = []
    for k, tile in enumerate(tiles):
        for img in tile["images"]:
            if img.id not in index:
                raise RuntimeError(f"visibility_based_camera_selection: image {img.id} of tile {k} is not in images")
        members.append(sorted({index[img.id] for img in tile["images"]}))
    pts, rows, at = [], [], 0
    for tile in tiles:
        pts += [np.asarray(p.xyz, np.float64).reshape(3) for p in tile["points3D"]]
        rows.append(np.arange(at, at + len(tile["points3D"])))
        at += len(tile["points3D"])
    xyz = np.array(pts, np.float64).reshape(-1, 3)
    intr = np.array([_intrinsics(cameras[img.camera_id]) for img in imgs], np.float64).reshape(-1, 4)
    E = np.array([w2c_matrix(img)[:3] for img in imgs], np.float64).reshape(-1, 3, 4)
    cen = np.array([cam_center(img) for img in imgs], np.float64).reshape(-1, 3)
    boxes = np.array([np.asarray(t["box"], np.float64) for t in tiles], np.float64).reshape(-1, 4)
    mask = _on(device, _host_mask(rows, len(xyz)))
    counts = _on(device, np.array([len(r) for r in rows], np.int32))
    zrange, stats = tile_z_range(_on(device, xyz), mask, counts)
    ratio, dist, md, add = visibility(_on(device, boxes), zrange, _on(device, E), _on(device, cen), _on(device, intr), _on(device, _host_mask(members, len(imgs))),
                                      threshod)
    add_cpu = add.cpu().numpy()
    out = [{"images": [imgs[c] for c in np.nonzero(add_cpu[t])[0]] + list(tile["images"]), "box": tile["box"], "points3D": tile["points3D"]}
           for t, tile in enumerate(tiles)]
    return (out, dict(zrange=zrange, stats=stats, ratio=ratio, dist=dist, md=md, add=add)) if return_tensors else out


def coverage_based_point_selection(tiles, points3D, device="cuda"):
    """The reference's step 4 (vastgaussian_utils.py:274-286): a tile's points become the points its images observe -- the ascending distinct
    point3D_ids != -1 of its images, each looked up in points3D.  An id that points3D lacks raises RuntimeError (the reference's KeyError).
    One host synchronisation on the device, plus one copy of the rows to the host."""
    if not tiles:
        return []
    imgs, index = [], {}
    per_tile = []
    for tile in tiles:
        mine = []
        for img in tile["images"]:
            if id(img) not in index:
                index[id(img)] = len(imgs)
                imgs.append(img)
            mine.append(index[id(img)])
        per_tile.append(sorted(set(mine)))
    if not imgs:
        raise RuntimeError("coverage_based_point_selection: no tile holds an image")
    arrays = [np.asarray(img.point3D_ids).reshape(-1).astype(np.int64, copy=False) for img in imgs]
    offsets = np.zeros(len(arrays) + 1, np.int64)
    np.cumsum([len(a) for a in arrays], out=offsets[1:])
    ids = np.concatenate(arrays) if arrays else np.zeros(0, np.int64)
    pid = np.fromiter(points3D.keys(), np.int64, len(points3D))
    pid.sort()
    off, rows = coverage(_on(device, offsets), _on(device, ids), _on(device, _host_mask(per_tile, len(imgs))), _on(device, pid), len(tiles))
    off, rows = off.numpy(), rows.cpu().numpy()
    return [{"images": tile["images"], "box": tile["box"], "points3D": [points3D[int(i)] for i in pid[rows[off[t]:off[t + 1]]]]} for t, tile in enumerate(tiles)]


def partition_scene(cameras, images, points3D, num_col=None, num_row=None, max_num_images=200, extend_ratio=0.1, visibility_threshold=0.5, device="cuda"):
    """What split_scene.py:39-53 computes, with its defaults: the four steps in a row.  cameras {id: .model .width .height .params}, images {id: .id
    .qvec .tvec .camera_id .name .point3D_ids}, points3D {id: .xyz}.  -> [{"images": [...], "box": float64 [4], "points3D": [...]}, ...], tile k being
    the reference's tile_%04d % k."""
    tiles = camera_position_based_region_division(images, num_col, num_row, max_num_images)
    tiles = position_based_data_selection(tiles, images, points3D, ratio=extend_ratio, device=device)
    tiles = visibility_based_camera_selection(tiles, images, cameras, threshod=visibility_threshold, device=device)
    return coverage_based_point_selection(tiles, points3D, device=device)


def write_box(path, box):
    """box.txt as split_scene.py:70-73 writes it, byte for byte: a header line, then the four bounds as str() prints them, no newline at the end."""
    with open(path, "w") as f:
        f.write("mx Mx my My\n")
        f.write(f"{box[0]} {box[1]} {box[2]} {box[3]}")
