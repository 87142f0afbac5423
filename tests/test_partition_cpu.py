"""CPU: the VastGaussian scene split away from the device (gsrast.partition; gs-sr_amd/csrc/gsr_partition.hip).  The numpy restatement the GPU tests use
as their truth (tests/ref_partition.py) is held to the fixtures the reference's own four functions produced (tests/golden/make_golden_partition.py),
exactly; step 1, which stays on the host, is held to the fixtures in both modes and to the restatement at its edges; write_box to the reference's
bytes; and every argument error is raised before a device is touched."""
import os
import types

import numpy as np
import pytest
import torch

import partition_cases as pc
import ref_partition as rp


def test_the_two_scenes_are_there():
    assert pc.SCENES == ["grid", "quad"]
    for name in pc.SCENES:
        assert os.path.getsize(os.path.join(pc.GOLDEN, f"ref_partition_{name}.npz")) <= 65536
    assert pc.load("quad")["cfg"]["num_col"] is None and pc.load("grid")["cfg"]["num_col"] == 2


@pytest.mark.parametrize("name", pc.SCENES)
def test_restatement_equals_the_reference_exactly(name):
    z, rs = pc.load(name), pc.restated(name)
    ids = z["image_ids"]
    assert np.array_equal(rs["cen"], z["centers"]), "centres: np.linalg.inv, bit for bit"
    assert rs["boxes"].tobytes() == z["boxes"].tobytes(), "box bits"
    assert [ids[t].tolist() for t in rs["first"]] == z["s1"], "step 1: tiles, membership and order"
    assert [ids[t].tolist() for t in rs["members"]] == z["s2"], "step 2: images in dict order"
    assert [z["point_ids"][p].tolist() for p in rs["in_box"]] == z["s2p"], "step 2: points in dict order"
    assert np.array_equal(rs["zr"], z["zrange"]), "mz, Mz as the reference's corner arrays held them"
    assert [ids[t].tolist() for t in rs["images"]] == z["s3"], "step 3: the added images in front, in dict order"
    assert [p.tolist() for p in rs["points"]] == z["s4"], "step 4: ascending distinct ids"
    # what the scenes were drawn for
    added = [len(a) - len(b) for a, b in zip(z["s3"], z["s2"])]
    assert sum(added) >= 1 and max(np.bincount(np.concatenate([np.searchsorted(np.sort(ids), t) for t in z["s3"]]))) >= 2
    assert (z["obs_ids"] == -1).any() and (np.diff(np.sort(z["point_ids"])) > 1).any() and (np.diff(z["point_ids"]) < 0).any()
    if name == "grid":
        assert sum(len(t) for t in z["s1"]) < len(ids), "grid mode drops the leftovers"


@pytest.mark.parametrize("name", pc.SCENES)
def test_region_division_equals_the_fixtures(name):
    from gsrast import partition
    z = pc.load(name)
    c = z["cfg"]
    tiles = partition.camera_position_based_region_division(z["images"], c["num_col"], c["num_row"], c["max_num_images"])
    assert [[it["image"].id for it in t["images"]] for t in tiles] == z["s1"]
    assert np.array([t["box"] for t in tiles]).tobytes() == z["boxes"].tobytes()
    assert all(t["box"].dtype == np.float64 and t["box"].shape == (4,) for t in tiles)
    by_id = {int(i): k for k, i in enumerate(z["image_ids"])}
    assert all(np.array_equal(it["center"], z["centers"][by_id[it["image"].id]]) for t in tiles for it in t["images"])


def _division(cen, **kw):
    from gsrast import partition
    images = {10 + k: pc.image_at(c, 10 + k) for k, c in enumerate(cen)}
    tiles = partition.camera_position_based_region_division(images, **kw)
    want, boxes = rp.region_division(np.asarray(cen, np.float64), kw.get("num_col"), kw.get("num_row"), kw.get("max_num_images", 150))
    assert [[it["image"].id - 10 for it in t["images"]] for t in tiles] == want
    assert np.array([t["box"] for t in tiles]).reshape(-1, 4).tobytes() == boxes.tobytes()
    return want


def test_region_division_edges():
    r = np.random.default_rng(0)
    cen = np.concatenate([r.uniform(0, 8, (14, 2)), np.zeros((14, 1))], axis=1)
    # halves of 7: final with max_num_images = 8 (len == max - 1), split again with 7 (len == max)
    assert [len(t) for t in _division(cen, max_num_images=8)] == [7, 7]
    assert [len(t) for t in _division(cen, max_num_images=7)] == [3, 4, 3, 4]
    # equal extents: the tie goes to axis 1
    sq = np.array([[0, 0, 0], [4, 1, 0], [1, 4, 0], [3, 3, 0]], np.float64)
    assert _division(sq, max_num_images=3) == [[0, 1], [3, 2]]
    # equal coordinates: Python's stable order keeps the dict's
    same = np.array([[k % 2, 5.0, 0] for k in range(6)], np.float64)          # extent 1 in x, 0 in y: axis 0; three images at x = 0, three at x = 1
    assert _division(same, max_num_images=4) == [[0, 2, 4], [1, 3, 5]]
    flat = np.array([[2.0, 2.0, 0]] * 5, np.float64)                          # all equal: axis 1, order untouched
    assert _division(flat, max_num_images=4) == [[0, 1], [2, 3, 4]]
    # grid mode: 11 images, 2 columns of 5 (the last image by x is dropped), each 2 rows of 2 (the last by y of each column is dropped)
    g = np.concatenate([r.uniform(0, 8, (11, 2)), np.zeros((11, 1))], axis=1)
    tiles = _division(g, num_col=2, num_row=2)
    assert [len(t) for t in tiles] == [2, 2, 2, 2]
    assert int(np.argmax(g[:, 0])) not in sum(tiles, [])
    tiles = _division(g[:10], num_col=2, num_row=5)                            # nothing left over
    assert sorted(sum(tiles, [])) == list(range(10))


def test_write_box_matches_the_reference_bytes(tmp_path):
    from gsrast import partition
    for name in pc.SCENES:
        z = pc.load(name)
        path = str(tmp_path / "box.txt")
        partition.write_box(path, z["boxes"][0])
        assert open(path, "rb").read() == z["box_txt"].tobytes()


def test_argument_errors_are_raised_before_a_device_is_touched():
    from gsrast import partition
    d = torch.zeros(5, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="xy: expected a tensor of shape"):
        partition.point_tiles(np.zeros((5, 3)), d)
    with pytest.raises(RuntimeError, match="xy must be a CUDA tensor"):
        partition.point_tiles(d, torch.zeros(2, 4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="xyz must be a CUDA tensor"):
        partition.tile_z_range(d, torch.zeros(5, 1, dtype=torch.int32), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="boxes must be a CUDA tensor"):
        partition.visibility(torch.zeros(2, 4, dtype=torch.float64), None, None, None, None, None, 0.25)
    with pytest.raises(RuntimeError, match="obs_offsets must be a CUDA tensor"):
        partition.coverage(torch.zeros(3, dtype=torch.int64), None, None, None, 2)
    with pytest.raises(RuntimeError, match="0 tiles out of range"):
        partition.coverage(None, None, None, None, 0)
    with pytest.raises(RuntimeError, match="1025 tiles out of range"):
        partition.coverage(None, None, None, None, 1025)
    with pytest.raises(RuntimeError, match="max_num_images must be at least 2"):
        partition.camera_position_based_region_division({1: pc.image_at([0, 0, 0], 1)}, max_num_images=1)
    with pytest.raises(RuntimeError, match="expected at least one image"):
        partition.camera_position_based_region_division({})
    with pytest.raises(RuntimeError, match="num_col and num_row must be positive"):
        partition.camera_position_based_region_division({1: pc.image_at([0, 0, 0], 1)}, num_col=0, num_row=1)
    with pytest.raises(RuntimeError, match="tile 0 is empty"):
        partition.camera_position_based_region_division({1: pc.image_at([0, 0, 0], 1), 2: pc.image_at([1, 0, 0], 2)}, num_col=1, num_row=3)
    # the reference's assertion keeps its text, and is raised before any device work
    img = pc.image_at([0, 0, 1], 1)
    tiles = [{"images": [img], "box": np.array([0.0, 1.0, 0.0, 1.0]), "points3D": []}]
    cams = {1: types.SimpleNamespace(model="OPENCV", width=4, height=4, params=np.ones(8))}
    with pytest.raises(AssertionError, match="Colmap camera model not handled: only undistorted datasets \\(PINHOLE or SIMPLE_PINHOLE cameras\\) supported!"):
        partition.visibility_based_camera_selection(tiles, {1: img}, cams)
    assert partition.position_based_data_selection([], {}, {}) == [] and partition.coverage_based_point_selection([], {}) == []
