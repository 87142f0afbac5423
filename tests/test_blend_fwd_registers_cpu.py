"""CPU: the register budget of the surfel blend forward, read off the gfx950 code object's metadata (hipcc cross-compiles without a GPU).

k_blend_fwd<SURFEL> runs eight waves per SIMD, the most its 20 KB of LDS per workgroup allow, as long as it needs at most 64 VGPRs (512 per SIMD lane); one
register more costs a wave per SIMD, and nothing else in the suite would notice.  Compiled with the flags the Makefile gives gsr_blend.hip
(tools/kernel_resources.py keeps them; without -fno-slp-vectorize the kernel needs 83)."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402


def test_surfel_forward_keeps_eight_waves_per_simd(tmp_path):
    mk = open(os.path.join(kr.SRC, "Makefile")).read()
    blend = re.search(r"^BLEND_FLAGS = \$\(COMMON\) (.*) \$\(BLEND_EXTRA\)$", mk, re.M).group(1).split()
    assert blend == kr.BLEND, "tools/kernel_resources.py no longer has the Makefile's blend flags"
    out = str(tmp_path / "gsr_blend.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc"] + kr.COMMON + kr.BLEND + ["-o", out, os.path.join(kr.SRC, "gsr_blend.hip")], stderr=subprocess.DEVNULL)
    txt = open(out).read()
    recs = [r for r in re.split(r"\n  - ", txt[txt.index("amdhsa.kernels:"):]) if re.search(r"\.name:\s+_Z11k_blend_fwdILi1EEv11BlendParams\s", r)]
    assert len(recs) == 1
    g = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, recs[0]).group(1))
    assert g("vgpr_count") <= 64 and g("vgpr_spill_count") == 0, (g("vgpr_count"), g("vgpr_spill_count"))
