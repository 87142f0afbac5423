"""The gate every call from the Python packages into libgsrast_hip.so goes through (gsrast.enqueue / call / scratch / one_device / raise_status),
against a stand-in library: no device and no built library is needed."""
import ast
import ctypes as C
import glob
import os

import pytest
import torch

import gsrast
from gsrast import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENQUEUEING = {name for name, restype, argtypes in _abi.FUNCTIONS if restype is _abi.cint and argtypes and argtypes[-1] is _abi.vp}


class _FakeLib:
    """Records every call in `log` and every entry point that is looked up in `lookups`; gsr_probe / gsd_probe return `rc`."""

    def __init__(self, log, rc=0):
        self.log, self.rc, self.lookups = log, rc, []

    def _probe(self, *args):
        self.log.append(("entry", args))
        return self.rc

    def __getattr__(self, name):
        self.lookups.append(name)
        return {"gsr_probe": self._probe, "gsd_probe": self._probe, "gsr_last_error": lambda: b"the last error"}[name]


@pytest.fixture
def gate(monkeypatch):
    """-> (log, fake library): torch.cuda.device and the stream lookup record into the log instead of touching a device."""
    log = []
    fake = _FakeLib(log)
    monkeypatch.setattr(gsrast, "_lib", fake)

    class _Device:
        def __init__(self, dev):
            self.dev = dev

        def __enter__(self):
            log.append(("enter", self.dev))

        def __exit__(self, *exc):
            log.append(("exit", self.dev))

    monkeypatch.setattr(torch.cuda, "device", _Device)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 7)      # some other device is current
    monkeypatch.setattr(gsrast, "stream_ptr", lambda dev=None: ("stream of", dev))
    return log, fake


def test_gate_calls_inside_device_context_with_stream_last(gate):
    log, fake = gate
    dev = torch.device("cpu")
    t = torch.zeros(5)
    arr = (C.c_float * 3)(1, 2, 3)
    word = C.c_uint32(7)
    ref = C.byref(word)
    raw = C.c_void_p(1234)
    fake.rc = 0
    assert gsrast.enqueue("gsr_probe", dev, 3, t, None, 2.5, arr, ref, raw) == 0
    assert [e[0] for e in log] == ["enter", "entry", "exit"]          # the entry point ran inside the device context ...
    assert log[0][1] == dev and log[2][1] == dev                      # ... of dev
    args = log[1][1]
    assert args[-1] == ("stream of", dev)                             # the stream came last
    assert isinstance(args[1], C.c_void_p) and args[1].value == t.data_ptr()
    assert args[2] is None
    assert args[0] == 3 and args[3] == 2.5 and args[4] is arr and args[5] is ref and args[6] is raw
    assert len(args) == 8
    fake.rc = 5
    assert gsrast.enqueue("gsr_probe", dev) == 5                      # enqueue hands the return code back


def test_gate_leaves_a_current_device_alone(gate, monkeypatch):
    log, _ = gate
    dev = torch.device("cpu")
    monkeypatch.setattr(torch.cuda, "current_device", lambda: dev.index)      # dev is the current device already
    t = torch.zeros(3)
    assert gsrast.enqueue("gsr_probe", dev, t, 4) == 0
    assert len(log) == 1 and log[0][0] == "entry"                    # no context entered; the same call is made
    args = log[0][1]
    assert args[0].value == t.data_ptr() and args[1] == 4 and args[2] == ("stream of", dev) and len(args) == 3


def test_call_raises_with_the_label_and_the_last_error(gate):
    log, fake = gate
    dev = torch.device("cpu")
    gsrast.call("gsr_probe", dev, 1)                                  # rc 0: nothing raised
    fake.rc = 1
    with pytest.raises(RuntimeError) as e:
        gsrast.call("gsr_probe", dev, 1)
    assert str(e.value) == "gsrast probe: the last error"             # the name without its prefix
    with pytest.raises(RuntimeError) as e:
        gsrast.call("gsd_probe", dev, 1)
    assert str(e.value) == "gsrast probe: the last error"
    with pytest.raises(RuntimeError) as e:
        gsrast.call("gsr_probe", dev, 1, what="forward")
    assert str(e.value) == "gsrast forward: the last error"


@pytest.mark.parametrize("bad, word", [(lambda: torch.zeros(4, device="meta"), "meta"), (lambda: torch.zeros(4, 4).t(), "contiguous")])
def test_gate_refuses_before_the_entry_point(gate, bad, word):
    log, fake = gate
    for fn in (gsrast.enqueue, gsrast.call):
        with pytest.raises(RuntimeError) as e:
            fn("gsr_probe", torch.device("cpu"), 9, torch.zeros(2), bad())
        msg = str(e.value)
        assert "gsr_probe" in msg and "argument 2" in msg and word in msg
    assert log == []                                                  # neither the device context nor the entry point was reached ...
    assert fake.lookups == []                                         # ... and the entry point was not even looked up on the library


def test_one_device():
    a, b, m = torch.zeros(2), torch.zeros(3), torch.zeros(2, device="meta")
    assert gsrast.one_device(("a", a), ("none", None), ("b", b)) == torch.device("cpu")
    assert gsrast.one_device(("none", None), ("m", m)) == torch.device("meta")
    assert gsrast.one_device() is None and gsrast.one_device(("none", None)) is None
    with pytest.raises(RuntimeError) as e:
        gsrast.one_device(("none", None), ("centers", a), ("obs_ids", b), ("point_ids", m))
    assert str(e.value) == "point_ids must be on the device of centers"


def test_scratch_is_never_empty():
    for n, want in ((0, 1), (1, 1), (8, 8), (4097, 4097)):
        s = gsrast.scratch(n, torch.device("cpu"))
        assert s.dtype == torch.uint8 and s.numel() == want


# What the three status_message functions returned at the commit before the tables, bit by bit.
_VIEWS = {
    1: "a non-finite value: a camera centre or a term of a score is NaN or infinite (a point that coincides with a centre, or a cosine that rounds above 1)",
    2: "a point id that two or more images observe is absent from the point table",
    4: "point_ids does not ascend strictly",
    8: "obs_offsets does not ascend from 0 to len(obs_ids)",
    16: "wide_ids=False but an id has bits above 2^32",
}
_PARTITION = {
    1: "a tile has fewer than four points in its box, or no point's neighbour distance lies inside mean +- 3 std (the reference fails on an empty min())",
    2: "a non-finite value: a box bound, a point coordinate (as float32), a 3-sigma threshold or a term of a projection is NaN or infinite",
    4: "a box corner has camera-space z exactly 0 (the reference gets a Qhull error)",
    8: "a point id that an image of a tile observes is absent from the point table (the reference's KeyError)",
    16: "point_ids does not ascend strictly",
    32: "obs_offsets does not ascend from 0 to len(obs_ids)",
    64: "counts does not hold the number of bits of mask",
}
_INIT = {
    1: "a non-finite value (NaN or infinity) in the input",
    2: "a voxel key outside int32: (point - init_pos) / cell exceeds 2^31",
    4: "a rank beyond the number of elements",
}


def _cases(table):
    """(word, text) for every single bit, all bits together, an unknown bit alone and an unknown bit beside a known one."""
    top = 2 * max(table)
    return [(b, t) for b, t in table.items()] + [(top - 1, "; ".join(table.values())), (top, "unknown bits"), (top | 1, table[1])]


def test_status_messages_are_the_parents():
    from gsrast import init, partition, views
    for word, text in _cases(_VIEWS):
        assert views.status_message(word) == f"gsrast select_views: status {word}: {text}"
    for word, text in _cases(_PARTITION):
        assert partition.status_message("tile_z_range", word) == f"gsrast tile_z_range: status {word}: {text}"
    for word, text in _cases(_INIT):
        assert init.status_message("quantile", word) == f"gsrast quantile: status {word}: {text}"


def test_raise_status():
    table = {1: "one", 4: "four"}
    gsrast.raise_status("op", 0, table)                               # zero does not raise
    for word, text in ((1, "one"), (5, "one; four"), (2, "unknown bits"), (6, "four")):
        with pytest.raises(RuntimeError) as e:
            gsrast.raise_status("op", word, table)
        assert str(e.value) == f"gsrast op: status {word}: {text}"


def test_nobody_goes_around_the_gate():
    assert len(ENQUEUEING) >= 76 and "gsr_profile_enable" not in ENQUEUEING and "gsr_last_error" not in ENQUEUEING
    files = sorted(glob.glob(os.path.join(ROOT, "gs-sr_amd", "**", "*.py"), recursive=True))
    assert len(files) >= 30
    around = []
    for path in files:
        rel = os.path.relpath(path, ROOT)
        for node in ast.walk(ast.parse(open(path).read(), path)):
            if isinstance(node, ast.Attribute) and node.attr in ENQUEUEING:
                around.append(f"{rel}:{node.lineno}: .{node.attr}")
            name = node.attr if isinstance(node, ast.Attribute) else node.id if isinstance(node, ast.Name) else \
                [a.name for a in node.names] if isinstance(node, ast.ImportFrom) else None
            if (name == "stream_ptr" or (isinstance(name, list) and "stream_ptr" in name)) and rel != os.path.join("gs-sr_amd", "gsrast", "__init__.py"):
                around.append(f"{rel}:{node.lineno}: stream_ptr")
    assert not around, "calls that do not go through gsrast.enqueue / gsrast.call:\n" + "\n".join(around)
