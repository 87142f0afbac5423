"""The method iterations are product code: gsrast.methods, and bench.py's method leg through the tools, load nothing from tests/ (and
gsrast.methods nothing from tools/).  No GPU: imports only."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _under(mod, *dirs):
    f = getattr(mod, "__file__", None)
    return bool(f) and os.path.abspath(f).startswith(tuple(os.path.join(ROOT, d) + os.sep for d in dirs))


def test_gsrast_methods_imports_with_only_the_package_tree_on_the_path(tmp_path):
    code = ("import os, sys, gsrast.methods\n"
            "bad = [n for n, m in sys.modules.items() for f in [getattr(m, '__file__', None)] if f and\n"
            "       os.path.abspath(f).startswith((os.path.join(sys.argv[1], 'tests') + os.sep, os.path.join(sys.argv[1], 'tools') + os.sep))]\n"
            "print('LOADED', sorted(bad))\n")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "gs-sr_amd"))
    r = subprocess.run([sys.executable, "-c", code, ROOT], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "LOADED []" in r.stdout, r.stdout


def test_the_method_leg_of_bench_loads_no_module_from_tests():
    before = set(sys.modules)
    import bench  # noqa: F401
    tools = os.path.join(ROOT, "tools")
    sys.path.insert(0, tools)                    # what bench.method_iteration does before its imports
    try:
        import iter_breakdown, bench_pipeline, bench_pipeline_octree_pgsr, bench_pipeline_pgsr  # noqa: F401
    finally:
        sys.path.remove(tools)
    new = sorted(n for n in set(sys.modules) - before if _under(sys.modules[n], "tests"))
    assert new == [], new
