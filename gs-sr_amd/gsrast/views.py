"""The PGSR neighbour views, on the device (include/gsrast.h "neighbour views", csrc/gsr_views.hip).

Replaces `view_selection` / `calc_score` (gssr/utils/mvsnet_utils.py:306-343), which `PGSRDataLoader.__init__` runs when the scene has no pair.txt: it
scores every pair of training images by the SfM points they share -- one list search per element, len_i * len_j comparisons per pair, C (C - 1) / 2
pairs over a process pool -- and keeps each image's `num_views` best partners as `cam.near_ids`.  Here the same sums run over the point TRACKS:

    select_views       tensors in, tensors out, everything on the device, one host read (the status word)
    view_selection     the reference's arguments and its list of lists of (index, score)
    write_pairs, read_pairs, assign_near_ids      the reference's pair.txt, byte for byte, and what pgsr_dataloader.py:44-46 does with the lists

Scores are float64 sums in ascending point id.  That is not the reference's order (it walks the lower-indexed image's keypoints), so a score agrees
with the reference's to rounding (relative 1e-10 for angles above 0.1 degree), not bit for bit; two calls here give identical bits and
scores[a, b] == scores[b, a] exactly.

Ties.  The reference ranks a row with np.argsort(score)[::-1], an unstable sort: the order of equal scores is whatever it leaves.  Here the rule is
fixed: descending score, and among EQUAL scores the HIGHER index first (what a stable ascending sort, reversed, gives; what numpy's own sort
leaves depends on its version and SIMD dispatch).  The image's own index competes with its score 0, as in the reference, so it is selected when
C <= num_views or fewer than num_views partners score above 0.

Deviation.  In the reference a cosine that rounds above 1 gives NaN and silently poisons that pair's score (the row is then ranked with a NaN in it).
Here any non-finite term, or a non-finite camera centre, raises RuntimeError."""
import numpy as np
import torch

from . import call, lib, one_device, raise_status, scratch, status_text, typed_tensor as _tensor

ERR_NONFINITE, ERR_ABSENT, ERR_TABLE, ERR_OFFSETS, ERR_ID_RANGE = 1, 2, 4, 8, 16
MAX_IMAGES = 16384                                        # GSR_VIEWS_MAX_IMAGES: a row of scores is held in LDS


STATUS = {
    ERR_NONFINITE: "a non-finite value: a camera centre or a term of a score is NaN or infinite (a point that coincides with a centre, or a cosine "
                   "that rounds above 1)",
    ERR_ABSENT: "a point id that two or more images observe is absent from the point table",
    ERR_TABLE: "point_ids does not ascend strictly",
    ERR_OFFSETS: "obs_offsets does not ascend from 0 to len(obs_ids)",
    ERR_ID_RANGE: "wide_ids=False but an id has bits above 2^32",
}


def status_message(status):
    """The text of the status word of gsr_view_select."""
    return status_text("select_views", status, STATUS)


def _params(theta0, sigma1, sigma2, num_views):
    theta0, sigma1, sigma2 = float(theta0), float(sigma1), float(sigma2)
    if not (np.isfinite(theta0) and np.isfinite(sigma1) and np.isfinite(sigma2) and sigma1 > 0 and sigma2 > 0):
        raise RuntimeError("select_views: theta0 must be finite and sigma1, sigma2 positive finite numbers")
    if int(num_views) != num_views or int(num_views) < 1:
        raise RuntimeError(f"select_views: num_views must be a positive integer, not {num_views}")
    return theta0, sigma1, sigma2, int(num_views)


def select_views(centers, obs_offsets, obs_ids, point_ids, point_xyz, theta0=5, sigma1=1, sigma2=10, num_views=10, return_scores=False, wide_ids=True):
    """-> (near_ids int32 [C,k], near_scores float64 [C,k]) and, with return_scores, scores float64 [C,C]; k = min(num_views, C).

    centers float64 [C,3]; obs_ids int64 [M]: the images' COLMAP point ids (-1: none; repeats allowed) one image after the other, image a in
    [obs_offsets[a], obs_offsets[a + 1]), obs_offsets int64 [C + 1]; point_ids int64 [Np] ascending strictly with point_xyz float64 [Np,3].  All on one
    device.  wide_ids=False promises that every id fits 32 bits, which saves the sort its high-word passes (a broken promise raises).
    Row a of near_ids ranks the images by descending score[a], the higher index first among equal scores, a itself included with score 0 (module
    docstring).  Raises RuntimeError when an id that two or more images observe is absent from point_ids (the reference's KeyError; an absent id that
    one image observes is no error) and -- unlike the reference, which leaves a NaN in the scores -- when a centre or a term is not finite.
    At most 16384 images.  Exactly one host synchronisation: the status word."""
    theta0, sigma1, sigma2, num_views = _params(theta0, sigma1, sigma2, num_views)
    cen = _tensor(centers, "centers", torch.float64, (None, 3))
    Cn = cen.shape[0]
    if Cn < 1:
        raise RuntimeError("select_views: expected at least one image")
    if Cn > MAX_IMAGES:
        raise RuntimeError(f"select_views: {Cn} images exceed the limit of {MAX_IMAGES} (a row of scores is held in LDS)")
    off = _tensor(obs_offsets, "obs_offsets", torch.int64, (Cn + 1,))
    ids = _tensor(obs_ids, "obs_ids", torch.int64, (None,))
    pid = _tensor(point_ids, "point_ids", torch.int64, (None,))
    xyz = _tensor(point_xyz, "point_xyz", torch.float64, (pid.shape[0], 3))
    dev = one_device(("centers", cen), ("obs_offsets", off), ("obs_ids", ids), ("point_ids", pid), ("point_xyz", xyz))
    M, Np, k = ids.shape[0], pid.shape[0], min(num_views, Cn)
    near_ids = torch.empty(Cn, k, dtype=torch.int32, device=dev)
    near_scores = torch.empty(Cn, k, dtype=torch.float64, device=dev)
    scores = torch.empty(Cn, Cn, dtype=torch.float64, device=dev) if return_scores else None
    status = torch.empty(1, dtype=torch.int32, device=dev)
    nbytes = int(lib().gsr_view_select_scratch_bytes(M, Cn))
    work = scratch(nbytes, dev)
    call("gsr_view_select", dev, cen, Cn, off, ids if M else None, M, pid if Np else None, xyz if Np else None, Np, theta0, sigma1, sigma2, k,
         64 if wide_ids else 32, near_ids, near_scores, scores, work, nbytes, status)
    raise_status("select_views", int(status.item()) & 0xFFFFFFFF, STATUS)      # the one host read
    return (near_ids, near_scores, scores) if return_scores else (near_ids, near_scores)


def flatten_observations(camera_point3D_ids):
    """-> (obs_offsets int64 [C + 1], obs_ids int64 [M]) numpy arrays from the reference's list of per-image id arrays."""
    arrays = [np.asarray(a).reshape(-1).astype(np.int64, copy=False) for a in camera_point3D_ids]
    offsets = np.zeros(len(arrays) + 1, np.int64)
    np.cumsum([len(a) for a in arrays], out=offsets[1:])
    return offsets, (np.concatenate(arrays) if arrays else np.zeros(0, np.int64))


def point_table(points3d):
    """-> (point_ids int64 [Np] ascending, point_xyz float64 [Np,3]) numpy arrays from the reference's {id: object with .xyz}."""
    ids = np.fromiter(points3d.keys(), np.int64, len(points3d))
    ids.sort()
    xyz = np.array([np.asarray(points3d[int(i)].xyz, np.float64).reshape(3) for i in ids], np.float64).reshape(-1, 3)
    return ids, xyz


def view_selection(camera_centers, camera_point3D_ids, points3d, theta0=5, sigma1=1, sigma2=10, num_views=10, device="cuda"):
    """The reference's view_selection (mvsnet_utils.py:322-343), its arguments and its result: per image the list of its min(num_views, C) best
    partners as (index, score), best first.  camera_centers: C float64 3-vectors; camera_point3D_ids: C integer arrays (-1: no point); points3d:
    {id: object with .xyz}.  Ties and non-finite values: see the module docstring.  To use it in the reference's data loader, which imports the name
    directly, rebind gssr.dataloader.pgsr_dataloader.view_selection."""
    if len(camera_centers) != len(camera_point3D_ids):
        raise RuntimeError(f"view_selection: {len(camera_centers)} centres but {len(camera_point3D_ids)} id arrays")
    if len(camera_centers) == 0:
        return []
    centers = np.array([np.asarray(c, np.float64).reshape(3) for c in camera_centers], np.float64)
    offsets, ids = flatten_observations(camera_point3D_ids)
    pid, xyz = point_table(points3d)
    wide = bool(ids.size) and bool(((ids != -1) & ((ids < 0) | (ids >= (1 << 32)))).any())
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    near_ids, near_scores = select_views(t(centers), t(offsets), t(ids), t(pid), t(xyz), theta0, sigma1, sigma2, num_views, wide_ids=wide)
    return [list(zip(row_i, row_s)) for row_i, row_s in zip(near_ids.cpu().tolist(), near_scores.cpu().tolist())]


def write_pairs(file, view_sel):
    """Writes the pair.txt the reference's data loader reads back (the format of mvsnet_utils.py:345-352, byte for byte).  Line 1: the number of
    images.  Then two lines per image: its index, and the fields `n id_0 score_0 ... id_{n-1} score_{n-1}` -- integers in decimal, a score truncated
    towards zero as %d prints it -- each field FOLLOWED by one blank, the last one too."""
    lines = [str(len(view_sel))]
    for index, partners in enumerate(view_sel):
        fields = [len(partners)]
        for partner, score in partners:
            fields += [int(partner), int(score)]
        lines += [str(index), "".join(f"{v} " for v in fields)]
    with open(file, "w") as f:
        f.write("".join(line + "\n" for line in lines))


def read_pairs(file):
    """Reads a pair.txt as the reference's read_pairs does (mvsnet_utils.py:354-362), its HALF LIST included: of the n (id, score) pairs of an image's
    line the reference returns only the first ceil(n / 2) -- it advances two pairs per step while consuming one -- and that shorter list is what the
    data loader then uses for a scene that already has a pair.txt.  -> list of lists of (int, float)."""
    with open(file, "r") as f:
        lines = f.read().split("\n")
    out = []
    for image in range(int(lines[0])):
        fields = lines[2 + 2 * image].rstrip().split(" ")          # lines[1 + 2 * image] holds the image's index
        n = int(fields[0])
        pairs = list(zip(fields[1:1 + 2 * n:2], fields[2:2 + 2 * n:2]))
        out.append([(int(k), float(v)) for k, v in pairs[:(n + 1) // 2]])
    return out


def assign_near_ids(train_dataset_by_scale, view_sel):
    """What pgsr_dataloader.py:44-46 leaves on the cameras: at every resolution scale, camera i gets near_ids = the indices of view_sel[i], best first."""
    near = [[index for index, _ in partners] for partners in view_sel]
    for cameras in train_dataset_by_scale.values():
        if len(cameras) > len(near):
            raise IndexError(f"assign_near_ids: {len(cameras)} cameras but {len(near)} lists of neighbours")
        for camera, ids in zip(cameras, near):
            camera.near_ids = list(ids)
