"""CPU: the register budgets of the splat-parallel blend backward, read off the gfx950 code object's metadata (hipcc cross-compiles without a GPU).

k_blend_bwd_sp<V> is built for a fixed number of waves per SIMD (SP_WPE_*: EWA 6, PLANE 5, SURFEL 4), i.e. at most 80 / 96 / 128 VGPRs of the 512 per
SIMD lane, and a change that pushes a variant over its budget shows up as spilled registers (scratch traffic in the hot loop), which nothing else in
the suite would notice.  Compiled with the flags the Makefile gives gsr_blend_sp.hip (tools/kernel_resources.py keeps them)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

# variant id (include/gsrast.h: GSR_EWA 0, GSR_SURFEL 1, GSR_PLANE 2) -> (VGPR budget, spilled VGPRs allowed)
# PLANE's spill figure is the one read off a build of the commit before the zero-record fetch of the empty lanes went in: 0 (no scratch at all).
BUDGET = {"ewa": (0, 80, 0), "surfel": (1, 128, 0), "plane": (2, 96, 0)}


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    mk = open(os.path.join(kr.SRC, "Makefile")).read()
    blend = re.search(r"^BLEND_FLAGS = \$\(COMMON\) (.*) \$\(BLEND_EXTRA\)$", mk, re.M).group(1).split()
    assert blend == kr.BLEND, "tools/kernel_resources.py no longer has the Makefile's blend flags"
    out = str(tmp_path_factory.mktemp("sp") / "gsr_blend_sp.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc"] + kr.COMMON + kr.BLEND + ["-o", out, os.path.join(kr.SRC, "gsr_blend_sp.hip")], stderr=subprocess.DEVNULL)
    txt = open(out).read()
    return re.split(r"\n  - ", txt[txt.index("amdhsa.kernels:"):])


@pytest.mark.parametrize("variant", sorted(BUDGET))
def test_blend_backward_keeps_its_register_budget(records, variant):
    vid, vgprs, spills = BUDGET[variant]
    recs = [r for r in records if re.search(r"\.name:\s+_Z14k_blend_bwd_spILi%dEEv11BlendParams\s" % vid, r)]
    assert len(recs) == 1
    g = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, recs[0]).group(1))
    assert g("vgpr_count") <= vgprs and g("vgpr_spill_count") <= spills and g("private_segment_fixed_size") == 0, \
        (g("vgpr_count"), g("vgpr_spill_count"), g("private_segment_fixed_size"))
