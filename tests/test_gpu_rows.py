"""The row mover (csrc/gsr_rows.hip) through gsrast.anchors.rows_compact: the cases its two clients' own suites do not reach -- a table that needs a
second launch, the 4- and 8-byte unit paths on rows the 16-byte path would take, a block boundary inside a row, and a device-side map of no rows.
Every result is compared with torch.cat((x[keep], tail)) on the host for exact equality."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _check(keep, xs, tails, dev_xs=None):
    from gsrast import anchors
    dev_tails = [t.to(DEV) if torch.is_tensor(t) else t for t in tails]
    outs = anchors.rows_compact(keep.to(DEV), dev_xs if dev_xs is not None else [x.to(DEV) for x in xs], dev_tails)
    assert len(outs) == len(xs)
    for i, (x, t, o) in enumerate(zip(xs, tails, outs)):
        tail = t if torch.is_tensor(t) else torch.zeros((t,) + tuple(x.shape[1:]), dtype=x.dtype)
        want = torch.cat((x[keep], tail))
        assert o.shape == want.shape and o.dtype == want.dtype and torch.equal(o.cpu(), want), i


def test_table_split():
    """25 tensors: the table of a launch holds 24, the last one goes in a second launch."""
    g = torch.Generator().manual_seed(25)
    N = 1000
    xs = [torch.randn(N, 1, generator=g) for _ in range(25)]
    _check(torch.rand(N, generator=g) < 0.7, xs, [37] * 25)


@pytest.mark.parametrize("tail", ["tensor", "zeros"])
def test_unit_fallback(tail):
    """Rows of 16 bytes whose storage starts 4 and 8 bytes off a 16-byte boundary, beside an aligned one, in one table."""
    g = torch.Generator().manual_seed(16)
    N = 1000
    bases = [torch.randn(4 * N + off, generator=g) for off in (1, 2, 0)]
    xs = [b[off:].view(N, 4) for b, off in zip(bases, (1, 2, 0))]
    dev_xs = [b.to(DEV)[off:].view(N, 4) for b, off in zip(bases, (1, 2, 0))]
    assert [x.data_ptr() % 16 for x in dev_xs] == [4, 8, 0]
    tails = [torch.randn(37, 4, generator=g) for _ in xs] if tail == "tensor" else [37] * 3
    _check(torch.rand(N, generator=g) < 0.7, xs, tails, dev_xs)


@pytest.mark.parametrize("n_tail", [0, 1])
def test_chunk_edge_inside_a_row(n_tail):
    """683 rows of 12 bytes are 2049 units of 4 bytes: the 2048-unit block boundary falls inside the last row."""
    g = torch.Generator().manual_seed(683)
    N = 683
    _check(torch.ones(N, dtype=torch.bool), [torch.randn(N, 3, generator=g)], [torch.randn(n_tail, 3, generator=g)])


@pytest.mark.parametrize("N", [0, 1000])
def test_no_row_kept_tail_only(N):
    """The device-side number of mapped rows is 0: nothing kept of N rows, and N = 0; a tensor tail and a tail of zeros."""
    g = torch.Generator().manual_seed(N + 1)
    xs = [torch.randn(N, 3, generator=g), torch.randint(-9, 9, (N, 2), generator=g, dtype=torch.int32), torch.randn(N, 4, generator=g)]
    keep = torch.zeros(N, dtype=torch.bool)
    _check(keep, xs, [torch.randn(37, 3, generator=g), torch.randint(-9, 9, (37, 2), generator=g, dtype=torch.int32), torch.randn(5, 4, generator=g)])
    _check(keep, xs, [37, 37, 5])
