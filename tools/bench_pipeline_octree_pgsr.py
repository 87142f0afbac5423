"""End-to-end octree-pgsr iteration after step 7000 on synthetic anchors (BASELINE.json configs[2]), for the view camera AND the neighbour
camera: gsrast.methods.octree_pgsr, where the iteration is described.  Na anchors x k=10 offsets on 6 octree levels, sized so that ~300k
Gaussians reach the rasterizer per camera at 1920x1080.  One JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gs-sr_amd"))
from gsrast import methods             # noqa: E402
from bench_pipeline import timed       # noqa: E402


def build(a, dev, seed=0):
    """-> (step, st): one octree-pgsr training iteration (step > 7000); a has .Na and optionally .static."""
    return methods.octree_pgsr(dev, a.Na, static=bool(getattr(a, "static", False)), seed=seed)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--static", action="store_true", help="sync-free static-shape iteration (decode static_rows)")
    ap.add_argument("--graph", action="store_true", help="record the (static) iteration into a HIP graph and replay it")
    ap.add_argument("--Na", type=int, default=methods.SIZES["octree-pgsr"]["Na"])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    st, dt = timed(a, build)
    print(json.dumps({"pipeline": "octree-pgsr (step > 7000: LOD mask + prefilter + decode + plane render, twice; single-view + multi-view losses)",
                      "mode": st["mode"], "Na": a.Na, "Nv": st["Nv"], "P": st["P"], "steps": a.steps, "ms_per_iter": round(1e3 * dt / a.steps, 3),
                      "iters_per_s": round(a.steps / dt, 1)}))


if __name__ == "__main__":
    main()
