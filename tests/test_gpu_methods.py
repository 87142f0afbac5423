"""GPU: each of the four complete method iterations of gsrast.methods runs, eager, at a small size."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["scaffold-2dgs", "octree-2dgs", "octree-pgsr", "pgsr"])
def test_three_eager_iterations_leave_finite_parameters(name):
    from gsrast import methods
    step, st = methods.build(name, torch.device("cuda:0"), **({"P": 20000} if name == "pgsr" else {"Na": 9000}))
    for _ in range(3):
        step()
    assert st["P"] > 0
    if name != "pgsr":
        assert st["Nv"] > 0
    opt, = st["optimizers"]
    for p in (p for g in opt.param_groups for p in g["params"]):
        assert bool(torch.isfinite(p).all()), tuple(p.shape)
        assert float(opt.state[p]["step"]) == 3
