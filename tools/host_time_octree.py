"""Host time per octree-pgsr iteration with the device queue never full: python tools/host_time_octree.py
(eager gsrast.methods.octree_pgsr; every iteration is synchronised, then profiled by cumulative host time)."""
import os, sys, time, cProfile, pstats
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gs-sr_amd"))
import torch
from gsrast import methods
step, st = methods.build("octree-pgsr", torch.device("cuda:0"))
for _ in range(10):
    step()
torch.cuda.synchronize()
pr = cProfile.Profile(); pr.enable()
t0 = time.perf_counter()
for _ in range(30):
    step(); torch.cuda.synchronize()
dt = time.perf_counter() - t0
pr.disable()
print("ms per synchronised iteration", round(1e3 * dt / 30, 3))
pstats.Stats(pr).sort_stats("cumulative").print_stats(28)
