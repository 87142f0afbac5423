"""CPU: the first anchors (gsrast.init, csrc/gsr_init.hip).  The plain restatement tests/ref_create_anchors.py reproduces, with ==, every array the
reference's own create_from_data left in tests/golden/ref_create_anchors_*.npz; the ABI carries the new entry points; torch.quantile's float32 rank
rule is pinned where it parts from the float64 rank."""
import glob
import os
import re

import numpy as np
import pytest
import torch

import ref_create_anchors as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
OCTREE = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "ref_create_anchors_octree_*.npz")))
SCAFFOLD = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "ref_create_anchors_scaffold_*.npz")))
NEW = ["gsr_cam_dist_quantiles_scratch_bytes", "gsr_cam_dist_quantiles", "gsr_select_lerp_scratch_bytes", "gsr_select_lerp",
       "gsr_voxel_unique_scratch_bytes", "gsr_voxel_unique_count", "gsr_voxel_unique_emit"]


def test_golden_set_is_complete():
    assert len(OCTREE) == 3 and len(SCAFFOLD) == 4
    z = {n: np.load(os.path.join(GOLDEN, n)) for n in OCTREE}
    assert sorted(int(v["dist2level"]) for v in z.values()) == [0, 1, 2]                       # floor, round, ceil
    assert sorted({int(v["fork"]) for v in z.values()}) == [2, 3]
    assert {int(v["cfg_levels"]) for v in z.values()} == {-1, 4}
    assert any(v["scales"].shape[0] == 2 for v in z.values())
    neg = z["ref_create_anchors_octree_round.npz"]
    assert neg["points"].min() > 0 and (np.round((neg["points"] - neg["init_pos"]) / neg["voxel_size"]) < 0).any()      # keys go negative
    s = {n: np.load(os.path.join(GOLDEN, n)) for n in SCAFFOLD}
    assert sorted(str(v["points"].dtype) for v in s.values()) == ["float32", "float32", "float64", "float64"]
    assert sorted(float(v["cfg_voxel_size"]) > 0 for v in s.values()) == [False, False, True, True]
    for n in OCTREE + SCAFFOLD:
        assert os.path.getsize(os.path.join(GOLDEN, n)) < 128 * 1024


@pytest.mark.parametrize("name", OCTREE)
def test_restatement_reproduces_the_reference_octree(name):
    z = np.load(os.path.join(GOLDEN, name))
    cams = np.concatenate([np.concatenate([z[f"centres_{i}"], np.full((z[f"centres_{i}"].shape[0], 1), s, np.float32)], 1)
                           for i, s in enumerate(z["scales"])]).astype(np.float32)
    assert np.array_equal(cams, z["cam_infos"])
    got = ref.octree_create(z["points"], cams, dist_ratio=float(z["dist_ratio"]), fork=int(z["fork"]), extend=float(z["extend"]),
                            levels=int(z["cfg_levels"]), init_level=int(z["cfg_init_level"]), base_layer=int(z["cfg_base_layer"]),
                            visible_threshold=float(z["cfg_visible_threshold"]), dist2level=ref.MODES[int(z["dist2level"])])
    for k in ("all_dist", "standard_dist", "voxel_size", "init_pos", "positions0", "level0", "anchor", "level"):
        assert got[k].dtype == z[k].dtype and np.array_equal(got[k], z[k]), k
    for k in ("levels", "init_level", "base_layer"):
        assert got[k] == int(z[k]), k
    if float(z["cfg_visible_threshold"]) < 0:
        assert np.array_equal(got["positions1"], z["positions1"]) and np.array_equal(got["level1"], z["level1"])
    else:
        assert "positions1" not in z.files and got["visible_threshold"] == float(z["cfg_visible_threshold"])
    # a tenth of the generator's asserted margin (1e-5 between any visible fraction and the threshold): it cannot flip a keep decision
    assert abs(got["visible_threshold"] - float(z["visible_threshold"])) <= 1e-6
    import glue_truth
    assert np.array_equal(ref.scaling_of(glue_truth.dist2_bruteforce(z["anchor"])).numpy(), z["scaling"])


@pytest.mark.parametrize("name", SCAFFOLD)
def test_restatement_reproduces_the_reference_scaffold(name):
    z = np.load(os.path.join(GOLDEN, name))
    vs, anchor = ref.scaffold_create(z["points"], float(z["cfg_voxel_size"]))
    assert vs == float(z["voxel_size"])
    assert anchor.dtype == np.float32 and np.array_equal(anchor, z["anchor"])


def test_new_symbols_are_declared_exported_and_built():
    """Fails without the feature: the entry points of csrc/gsr_init.hip."""
    import gsrast
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsrast.h")).read(), flags=re.S)
    decl = set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", src))
    L = gsrast.lib()
    for s in NEW:
        assert s in decl, f"include/gsrast.h does not declare {s}"
        assert s in gsrast.EXPORTS, f"gsrast.EXPORTS lacks {s}"
        assert hasattr(L, s) and getattr(L, s).argtypes is not None, f"libgsrast_hip.so does not export {s} with a signature"
    assert re.search(r"#define\s+GSR_ABI_VERSION\s+8\b", src) and gsrast.ABI_VERSION == 8 and L.gsr_abi_version() == 8
    # scratch: O(C) for the camera quantiles (no C x N array), O(1) for an array, O(N L) for the voxels
    a, b = L.gsr_cam_dist_quantiles_scratch_bytes(1000, 300), L.gsr_cam_dist_quantiles_scratch_bytes(5000000, 300)
    assert a == b and 0 < a <= 300 * 4 * 256 * 4 + 3 * 4096 and L.gsr_cam_dist_quantiles_scratch_bytes(5000000, 3000) < 3000 * 4400 + 8192
    assert 0 < L.gsr_select_lerp_scratch_bytes(1 << 30) <= 4096 + 2 * 256
    assert L.gsr_voxel_unique_scratch_bytes(1000000, 12) < 1000000 * (12 * 4 + 24) + (1 << 20)
    assert L.gsr_voxel_unique_scratch_bytes(0, 1) == 0 and L.gsr_voxel_unique_scratch_bytes(10, 33) == 0 and L.gsr_cam_dist_quantiles_scratch_bytes(10, 0) == 0


def test_argument_errors_without_a_device():
    """The entry points validate before they touch the device."""
    import ctypes as C
    import gsrast
    L = gsrast.lib()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    one = lambda *v: (C.c_int64 * len(v))(*v)
    w = (C.c_float * 2)(0.0, 0.0)
    assert L.gsr_cam_dist_quantiles(a, 10, a, 1, one(0, 10), one(0, 10), w, a, a, 1 << 20, a, None) != 0 and "ranks" in gsrast.last_error()
    assert L.gsr_cam_dist_quantiles(a, 10, a, 1, one(0, 3), one(2, 3), w, a, a, 1 << 20, a, None) != 0 and "one apart" in gsrast.last_error()
    assert L.gsr_cam_dist_quantiles(a, 10, a, 1, one(0, 3), one(1, 3), w, a, a, 16, a, None) != 0 and "scratch" in gsrast.last_error()
    assert L.gsr_cam_dist_quantiles(a, 0, a, 1, one(0, 0), one(0, 0), w, a, a, 1 << 20, a, None) != 0 and "points" in gsrast.last_error()
    assert L.gsr_select_lerp(a, 5, None, 3, one(0), one(0), w, a, a, 1 << 20, a, None) != 0 and "targets" in gsrast.last_error()
    assert L.gsr_select_lerp(a, 5, None, 1, one(5), one(5), w, a, a, 1 << 20, a, None) != 0 and "ranks" in gsrast.last_error()
    ip, cell = (C.c_double * 3)(0, 0, 0), (C.c_double * 1)(0.0)
    assert L.gsr_voxel_unique_count(a, 5, 1, ip, cell, 0, a, 1 << 20, a, None) != 0 and "cell size" in gsrast.last_error()
    cell[0] = 1.0
    assert L.gsr_voxel_unique_count(a, 5, 1, ip, cell, 2, a, 1 << 20, a, None) != 0 and "mode" in gsrast.last_error()
    assert L.gsr_voxel_unique_count(a, 5, 1, ip, cell, 0, a, 16, a, None) != 0 and "scratch" in gsrast.last_error()
    rec = (C.c_uint32 * 2)(2, 5)
    assert L.gsr_voxel_unique_emit(a, 5, 1, ip, cell, 0, a, 1 << 20, rec, a, a, None) != 0 and "status 2" in gsrast.last_error()
    rec = (C.c_uint32 * 2)(0, 6)
    assert L.gsr_voxel_unique_emit(a, 5, 1, ip, cell, 0, a, 1 << 20, rec, a, a, None) != 0 and "record" in gsrast.last_error()
    from gsrast import init
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        init.camera_dist_quantiles(torch.zeros(4, 3), torch.zeros(1, 4), 0.999)
    with pytest.raises(RuntimeError, match="out of range"):
        init.kthvalue(torch.zeros(4), 0)
    assert "int32" in init.status_message("x", 2) and "non-finite" in init.status_message("x", 1)


def test_the_quantile_case_past_the_block_cap_makes_a_workgroup_take_a_second_chunk():
    """k_cq_hist's grid is (min(chunks, max(1, CQ_BLOCKS / batches)), batches) and a workgroup walks chunk = blockIdx.x, += gridDim.x: the loop turns
    a second time only where the chunks outnumber grid.x.  The constants the GPU tests mirror are the source's, and the case crosses the cap with a
    partial last batch and a partial last chunk."""
    import test_gpu_create_anchors as G
    src = open(os.path.join(ROOT, "gs-sr_amd", "csrc", "gsr_init.hip")).read()
    define = lambda name: re.search(r"^#define %s\s+(\S+(?: \* \S+\))?)" % name, src, flags=re.M).group(1)
    assert define("CQ_CB") == str(G.BATCH) and define("CQ_BLOCKS") == f"{G.BLOCKS}u"
    assert define("CQ_CHUNK") == "(SEL_BLOCK * CQ_PPT)" and int(define("SEL_BLOCK")) * int(define("CQ_PPT")) == G.CHUNK
    assert "std::min(gsr_div_up((uint32_t)N, CQ_CHUNK), std::max(1u, CQ_BLOCKS / batches)), batches)" in src and "chunk += gridDim.x" in src
    div_up = lambda a, b: -(-a // b)
    grid_x = lambda C, N: min(div_up(N, G.CHUNK), max(1, G.BLOCKS // div_up(C, G.BATCH)))
    make_p, make_c, r = G.QUANTILE_CASES["past_the_block_cap"]
    C, N = make_c().shape[0], make_p().shape[0]
    assert (C, N) == G.PAST_CAP and r == 0.999
    assert div_up(N, G.CHUNK) > max(1, G.BLOCKS // div_up(C, G.BATCH)) and C % G.BATCH != 0 and N % G.CHUNK != 0
    assert (div_up(C, G.BATCH), grid_x(C, N), div_up(N, G.CHUNK), C % G.BATCH, N % G.CHUNK) == (512, 8, 10, 2, 5)
    assert len(set(make_c()[:, 3].tolist())) == 4                                             # cameras of mixed scales
    for name, (mp, mc, _) in G.QUANTILE_CASES.items():                                        # no other case gets there
        if name != "past_the_block_cap":
            assert grid_x(mc().shape[0], mp().shape[0]) == div_up(mp().shape[0], G.CHUNK), name


def _lerp_fused(a, b, w):
    a, b, w = np.float32(a), np.float32(b), np.float32(w)
    d = np.float64(np.float32(b - a))                       # the product of two float32 is exact in float64; the one rounding to float32 follows
    return np.float32(np.float64(w) * d + np.float64(a)) if abs(w) < 0.5 else np.float32(np.float64(np.float32(w - np.float32(1))) * d + np.float64(b))


@pytest.mark.parametrize("n", [4099, 100003])
def test_quantile_ranks_are_float32(n):
    """torch.quantile computes rank = q * (n - 1) in the input's dtype.  set_level asks for q = dist_ratio and 1 - dist_ratio at every size; at
    n = 100003, q = 0.999 the float32 rank is 99902 exactly (one element, weight 0) where the float64 rank is 99901.998 (two elements), and torch
    follows the float32 one.  gsrast.init.ranks (what the kernels are handed) and the restatement agree with torch itself at both sizes: the elements
    through torch.quantile's 'lower' / 'higher' modes, the linear mode with either of ATen's two lerp evaluations (fused at the AVX2 / AVX512 dispatch
    levels, Lerp.h operation by operation at the DEFAULT level, which is the form this project pins)."""
    from gsrast import init
    x = torch.exp(torch.arange(n, dtype=torch.float64) * 1e-4).float()         # sorted, distinct, gaps far above a float32 step
    assert bool((x[1:] > x[:-1]).all())
    shuffled = x[torch.randperm(n, generator=torch.Generator().manual_seed(n))]
    parted = 0
    for q in (0.999, 1 - 0.999):
        lo, hi, w = init.ranks(q, n)
        assert (lo, hi, np.float32(w)) == ref.ranks(q, n)
        assert torch.quantile(shuffled, q, interpolation="lower") == x[lo] and torch.quantile(shuffled, q, interpolation="higher") == x[hi]
        want = float(torch.quantile(shuffled, q))
        assert want in (float(ref.lerp32(x[lo], x[hi], w)), float(_lerp_fused(x[lo], x[hi], w)))
        r64 = q * (n - 1)
        lo64, hi64 = int(np.floor(r64)), int(np.ceil(r64))
        if (lo64, hi64) != (lo, hi):
            parted += 1
            assert want != float(ref.lerp32(x[lo64], x[hi64], np.float32(r64 - lo64)))
    assert parted == (1 if n == 100003 else 0)


def test_lerp_is_lerp_h_at_atens_default_level():
    """The restatement's lerp (Lerp.h, every operation rounded on its own) is torch.quantile's at ATen's DEFAULT dispatch level, in a process of its own
    (the level is fixed when torch loads); in this process torch.quantile equals the unfused or the fused form, whichever level the machine runs at."""
    import subprocess
    import sys
    code = ("import sys, numpy as np, torch\n"
            "sys.path.insert(0, sys.argv[1])\n"
            "import ref_create_anchors as ref\n"
            "g = torch.Generator().manual_seed(5)\n"
            "bad = 0\n"
            "for n in (37, 1000, 4099):\n"
            "    for q in (0.999, 0.3, 0.77, 0.5):\n"
            "        for _ in range(12):\n"
            "            x = torch.rand(n, generator=g) * 10\n"
            "            bad += float(torch.quantile(x, q)) != float(ref.quantile(x.numpy(), q))\n"
            "print('mismatches', bad)\n")
    env = dict(os.environ, ATEN_CPU_CAPABILITY="default")
    out = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "tests")], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout + out.stderr
    g = torch.Generator().manual_seed(6)
    for n in (37, 1000):
        for q in (0.999, 0.3, 0.77):
            x = torch.rand(n, generator=g) * 10
            s = np.sort(x.numpy())
            lo, hi, w = ref.ranks(q, n)
            assert float(torch.quantile(x, q)) in (float(ref.lerp32(s[lo], s[hi], w)), float(_lerp_fused(s[lo], s[hi], w)))
