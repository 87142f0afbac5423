"""Drop-in replacement for `simple_knn._C` (submodules/simple-knn/ext.cpp:15-17):
    distCUDA2(points float32 [P,3]) -> float32 [P]   mean squared distance to the 3 nearest neighbours."""
import torch

from gsrast import lib, call, scratch, dev_f32


def distCUDA2(points):
    pts = dev_f32(points, "points", allow_empty=True)
    P = int(points.size(0))
    out = torch.zeros((P,), dtype=torch.float32, device=points.device)
    if P == 0:
        return out
    work = scratch(lib().gsr_dist2_scratch_bytes(P), points.device)
    call("gsr_dist2", points.device, P, pts, out, work, work.numel(), what="distCUDA2")
    return out
