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


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)      # private, but what torch's own generated code reads the stream with


def stream_ptr(device=None):
    """The current stream of `device` (None: of the current device) as a pointer.  Read through torch's raw-stream getter where this torch has
    it: torch.cuda.current_stream() builds a Stream object per call, 2 us of a 7 us call (EXPERIMENTS.md (94)); it is the fallback."""
    if device is not None and not isinstance(device, torch.device):
        device = torch.device(device)
    if _raw_stream is None:
        return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    index = None if device is None else device.index
    if index is None:
        index = torch.cuda.current_device()
    return C.c_void_p(_raw_stream(index))


# ---- the gate: the one place that knows how a call into the library is made.  Every entry point that enqueues work takes its stream last
# (_abi.FUNCTIONS: restype cint, last argtype vp); the library launches on that stream and keeps per-device state under hipGetDevice(), so the
# tensors' device must be the current one while the call runs, and every pointer must lie on it.
def enqueue(name, dev, *args):
    """-> rc of entry point `name`, called with `dev` current (made so for the call where it is not) and stream_ptr(dev) appended.  A torch.Tensor
    among args must be contiguous and on `dev` and travels as its data pointer; None stays None; everything else (numbers, ctypes arrays and
    structs, byref(), raw c_void_p) is passed as it is.  The entry point is looked up only once the arguments have passed.  Tensors whose
    pointers sit inside a struct are invisible here: their caller holds them to one device with one_device()."""
    current = torch.cuda.current_device()
    if dev.index is None and dev.type == "cuda":
        dev = torch.device("cuda", current)
    argv = list(args)
    for i, a in enumerate(argv):
        if isinstance(a, torch.Tensor):
            if a.device != dev:
                raise RuntimeError(f"gsrast {name}: argument {i} is a tensor on {a.device}, the call runs on {dev}")
            if not a.is_contiguous():
                raise RuntimeError(f"gsrast {name}: argument {i} is not contiguous")
            argv[i] = C.c_void_p(a.data_ptr())
    fn = getattr(lib(), name)
    if dev.index == current:                              # the common case, without the cost of entering and leaving the context
        return fn(*argv, stream_ptr(dev))
    with torch.cuda.device(dev):
        return fn(*argv, stream_ptr(dev))


def call(name, dev, *args, what=None):
    """enqueue(), then check(): `what` labels the error where it is not the entry point's name without its gsr_ / gsd_ prefix."""
    check(enqueue(name, dev, *args), what or name[4:])


def scratch(nbytes, dev):
    """A scratch block for a *_scratch_bytes figure: never empty, so that its pointer is never null."""
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)


def one_device(*named):
    """(name, tensor or None) pairs -> the device of the first tensor; every other one must share it.  For tensors that reach the library inside
    a struct, where enqueue() cannot see them."""
    first = dev = None
    for name, t in named:
        if t is None:
            continue
        if dev is None:
            first, dev = name, t.device
        elif t.device != dev:
            raise RuntimeError(f"{name} must be on the device of {first}")
    return dev


def status_text(op, word, table):
    """The text of a status word a kernel left: `table` is {bit: text}."""
    parts = [text for bit, text in table.items() if word & bit]
    return f"gsrast {op}: status {word}: " + "; ".join(parts or ["unknown bits"])


def raise_status(op, word, table):
    if word:
        raise RuntimeError(status_text(op, word, table))


def typed_tensor(t, name, dtype, shape, device=None):
    """A contiguous HIP tensor of `dtype` and `shape` (None: any size, printed as '*'), optionally on `device`, or a RuntimeError that names it."""
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"{name} must be a tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")
    if t.dtype != dtype:
        raise RuntimeError(f"{name}: expected {dtype} but found {t.dtype}")
    if t.dim() != len(shape) or any(s is not None and t.shape[i] != s for i, s in enumerate(shape)):
        raise RuntimeError(f"{name}: expected shape {[s if s is not None else '*' for s in shape]} but found {list(t.shape)}")
    if device is not None and t.device != device:
        raise RuntimeError(f"{name} must be on the device of {device}")
    return t.detach().contiguous()


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


from .mesh import cluster_connected_triangles, post_process_mesh, simplify_vertex_clustering  # noqa: E402,F401  (gsrast.mesh needs the helpers above)
from .mesh import vertex_adjacency, compute_triangle_normals, compute_vertex_normals  # noqa: E402,F401
from .mesh import filter_smooth_simple, filter_smooth_laplacian, filter_smooth_taubin  # noqa: E402,F401
from .mesh import MeshRaster, rasterize_mesh, triangle_view_counts, cull_unseen_triangles  # noqa: E402,F401
from .unbounded import extract_mesh_unbounded  # noqa: E402,F401
from . import chamfer  # noqa: E402,F401
from .chamfer import nearest_points, sample_surface, voxel_downsample, surface_distance  # noqa: E402,F401
from .chamfer import NearestGrid  # noqa: E402,F401
from . import register  # noqa: E402,F401
from .register import transform_points, correspondence_sums, solve_transform, fit_transform, icp, evaluate_registration, crop_polygon_volume  # noqa: E402,F401
from .register import RegistrationResult  # noqa: E402,F401
from . import images  # noqa: E402,F401
from .images import resize_u8, pil_to_torch, camera_images, load_resolution, PILtoTorch, load_camera_images  # noqa: E402,F401
