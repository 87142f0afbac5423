"""gsrast -- ctypes binding of libgsrast_hip.so (include/gsrast.h) and the shared autograd bridge used by the
drop-in packages diff_gaussian_rasterization / diff_surfel_rasterization / diff_plane_rasterization /
scaffold_filter / simple_knn that sit next to this package.

There is NO CPU or PyTorch fallback: every entry point raises if the HIP library is missing or a tensor is not on
a HIP device (the reference's extensions are CUDA-only in exactly the same way, e.g. CHECK_INPUT in
diff-surfel-rasterization/rasterize_points.cu:27-29).
"""
import ctypes as C
import os

import torch

from ._abi import FUNCTIONS, bind
from ._abi import gsr_cfg as Cfg, gsr_inputs as Inputs, gsr_outputs as Outputs, gsr_out_grads as OutGrads, gsr_in_grads as InGrads  # noqa: F401
from ._abi import gsr_mv_cfg as MvCfg, gsr_tsdf_sparse as TsdfSparse, gsr_lod_cfg as LodCfg  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GSR_LIB_PATH") or os.path.join(os.path.dirname(_HERE), "libgsrast_hip.so")   # override: experiments only

EWA, SURFEL, PLANE = 0, 1, 2                              # include/gsrast.h enum gsr_variant
ABI_VERSION = 8
PROF_LABELS = ["preprocess", "depth_order", "binning", "blend_fwd", "bwd_memset", "blend_bwd", "preprocess_bwd", "_"]      # enum gsr_prof_label
EXPORTS = [name for name, _, _ in FUNCTIONS if name.startswith("gsr_")]

_lib = None


def lib():
    """Loads libgsrast_hip.so and gives every entry point of both headers its signature (_abi.FUNCTIONS); fails loudly when the library has not been
    built (python __graft_entry__.py build) or is not the one this binding was written for."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"gsrast: HIP library not built: {LIB_PATH} (run `make -C gs-sr_amd/csrc` or "
                           f"`python -c 'import __graft_entry__ as g; g.build()'`); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    if L.gsr_abi_version() != ABI_VERSION:                # first: int32_t (void) is what ctypes assumes of an unbound function
        raise RuntimeError("gsrast: ABI version mismatch between python binding and libgsrast_hip.so")
    bind(L, LIB_PATH)
    _lib = L
    return L


def profile_enable(on=True, stages=None):
    """Starts (and resets) / stops the stage profiler.  stages: names out of PROF_LABELS to time only those (each timed stage costs ~10 us
    of stream idle time per launch: two HIP event records)."""
    if not on:
        lib().gsr_profile_enable(0)
    elif stages is None:
        lib().gsr_profile_enable(1)
    else:
        lib().gsr_profile_enable(sum(1 << PROF_LABELS.index(n) for n in stages) << 8)


def profile_read():
    """-> {label: (total_ms, launches)} accumulated since profile_enable(True)."""
    ms = (C.c_double * len(PROF_LABELS))(); n = (C.c_uint64 * len(PROF_LABELS))()
    lib().gsr_profile_read(ms, n)
    return {PROF_LABELS[i]: (ms[i], int(n[i])) for i in range(7)}


def last_error():
    return lib().gsr_last_error().decode("utf-8", "replace")


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"gsrast {what}: {last_error()}")


def stream_ptr(device=None):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def dev_f32(t, name, allow_empty=True):
    """The reference does x.contiguous().data<float>(): float32 required, empty tensor == 'not provided'."""
    if t is None or t.numel() == 0:
        if not allow_empty:
            raise RuntimeError(f"{name} must be provided")
        return None
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")          # CHECK_INPUT message of the surfel extension
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name}: expected scalar type Float but found {t.dtype}")
    return t.contiguous()


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def make_cfg(variant, P, settings, D, M, render_geo, keep):
    cfg = Cfg()
    cfg.variant = variant; cfg.P = P; cfg.D = int(D); cfg.M = int(M)
    cfg.W = int(settings.image_width); cfg.H = int(settings.image_height)
    cfg.tanfovx = float(settings.tanfovx); cfg.tanfovy = float(settings.tanfovy)
    cfg.scale_modifier = float(settings.scale_modifier)
    cfg.prefiltered = int(bool(settings.prefiltered)); cfg.debug = int(bool(settings.debug))
    cfg.render_geo = int(bool(render_geo))
    for name, attr in (("bg", "bg"), ("viewmatrix", "viewmatrix"), ("projmatrix", "projmatrix"), ("campos", "campos")):
        t = dev_f32(getattr(settings, attr), name, allow_empty=False)
        keep.append(t)
        setattr(cfg, name, t.data_ptr())
    return cfg


from .mesh import cluster_connected_triangles, post_process_mesh  # noqa: E402,F401  (gsrast.mesh needs the helpers above)
from .unbounded import extract_mesh_unbounded  # noqa: E402,F401
