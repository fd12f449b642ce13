"""The search kernel (csrc/nearest.hip) and the precision / recall / density / coverage kernels (csrc/prdc.hip) walk rows
with one function (csrc/rowdist.h), so what they compute from one distance is decided by the same bits.  The first four
tests compare the kernels with each other on generic bf16 rows (uniform in [-1, 1], where another order of summation shows
in the last place): no tolerance and no float64.  Every output sits between guard bands that must stay untouched; every
launch is repeated once and must be bit-identical.

Shapes: (Q, N) = a lone pair; a ragged tile with one row past a block; three tiles and three blocks, so that the chain of
rows loaded ahead wraps across tiles.  D = a row shorter than the wave stride of 512; one turn plus 64 elements; a second
LDS chunk of 64 elements; two full chunks with the wrap to chunk 0."""
import functools

import numpy as np
import pytest
import torch

import biggan_tensorflow_amd  # noqa: F401
from biggan_tensorflow_amd import functional as Fn
from tests import nn_ref as R

pytestmark = pytest.mark.gpu

BAND = 4096
FILL = {torch.float32: 12345.0, torch.int32: 12345}
PAIRS = [(1, 1), (13, 17), (19, 35)]
DIMS = [64, 576, 2112, 4096]


def _guarded(shape, dtype=torch.float32):
    """(buffer, view): the view sits between two bands of FILL."""
    n = int(np.prod(shape))
    buf = torch.full((BAND + n + BAND,), FILL[dtype], dtype=dtype, device="cuda")
    return buf, buf[BAND:BAND + n].view(*shape)


def _twice(launch, *shapes_dtypes):
    """Run ``launch(*outs)`` twice into guarded outputs: the same bits both times, the bands untouched.  The outputs."""
    made = [_guarded(shape, dtype) for shape, dtype in shapes_dtypes]
    outs = [view for _, view in made]
    launch(*outs)
    first = [o.clone() for o in outs]
    launch(*outs)
    for (buf, view), one in zip(made, first):
        fill = FILL[buf.dtype]
        assert torch.equal(one, view) and bool((buf[:BAND] == fill).all()) and bool((buf[-BAND:] == fill).all())
    return first


def _bf16(a):
    """float64 array of bf16-representable values -> bf16 tensor on the device, exactly."""
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).cuda().to(torch.bfloat16)


def _distances(q, s):
    return _twice(lambda out: Fn.nn_distances(q, s, out=out), ((len(q), len(s)), torch.float32))[0]


@functools.lru_cache(maxsize=None)
def _pair_once(Q, N, D):
    q, s = R.random_operands(np.random.RandomState(Q + N + D), Q, N, D)
    q, s = _bf16(q), _bf16(s)
    return q, s, _distances(q, s)


def _pair(Q, N, D):
    """(q, set, d): generic rows on the device and the search kernel's matrix, computed once per shape.  The matrix is
    handed out as a copy, so that no test can change what another reads."""
    q, s, d = _pair_once(Q, N, D)
    return q, s, d.clone()


# ---------------------------------------------------------------- the cover pass against the matrix
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("Q,N", PAIRS)
def test_cover_minimum_is_the_column_minimum_of_the_matrix(Q, N, D):
    q, s, d = _pair(Q, N, D)
    dmin, = _twice(lambda out: Fn.prdc_cover(q, None, s, count=None, dmin=out), ((N,), torch.float32))
    assert torch.equal(dmin, d.min(dim=0).values)
    assert torch.equal(Fn.prdc_cover(q, None, s, count=None)[1], dmin)


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("Q,N", PAIRS)
def test_counts_are_decided_by_the_same_bits(Q, N, D):
    q, s, d = _pair(Q, N, D)
    i = torch.arange(Q, device="cuda")
    radius = d[i, (7 * i) % N]                               # every query has one pair exactly at its radius
    if Q > 1:
        radius[0], radius[Q - 1] = float("inf"), 0.0         # the last query equals a set row: 0 <= 0 counts
    count, dmin = _twice(lambda c, m: Fn.prdc_cover(q, radius, s, count=c, dmin=m), ((N,), torch.int32), ((N,), torch.float32))
    want = (d <= radius[:, None]).sum(0)                     # the pairs at their radius are in: <= of equal numbers
    assert torch.equal(count.long(), want)                   # the same fp32 numbers on both sides: no pair is undecided
    assert torch.equal(dmin, d.min(dim=0).values)


# ---------------------------------------------------------------- the radii against the matrix
@functools.lru_cache(maxsize=None)
def _self_matrix_once(N, D):
    x = R.random_operands(np.random.RandomState(3 * N + D), 1, N, D)[1]
    x[5] = x[2]
    x = _bf16(x)
    d = _distances(x, x)
    n = torch.arange(N, device="cuda")
    d[n, n] = float("inf")
    return x, d


def _self_matrix(N, D):
    """(x, d): generic rows, row 5 a copy of row 2, and the search kernel's matrix of x against itself with the diagonal
    set to +inf by index, computed once per shape; the matrix is handed out as a copy."""
    x, d = _self_matrix_once(N, D)
    return x, d.clone()


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("D", [64, 2112])
@pytest.mark.parametrize("N", [9, 17, 35])
def test_radii_are_the_kth_off_diagonal_entry_of_the_matrix(N, D, k):
    x, d = _self_matrix(N, D)
    got, = _twice(lambda out: Fn.prdc_radii(x, k, out=out), ((N,), torch.float32))
    assert torch.equal(got, d.sort(dim=1).values[:, k - 1])
    if k == 1:
        assert got[2] == 0.0 and got[5] == 0.0               # an equal row elsewhere counts, at distance 0


# ---------------------------------------------------------------- the search kernel alone
@pytest.mark.parametrize("D", [576, 2112])
def test_search_kernel_is_symmetric_bit_for_bit(D):
    x, y, xy = _pair(19, 35, D)
    assert torch.equal(xy, _distances(y, x).T)


def test_exact_operands_over_two_full_chunks_bit_for_bit():
    """The exact-operand test of test_gpu_nn.py at D = 4096: two full LDS chunks and the wrap of the rows loaded ahead to
    chunk 0, which no shape of nn_ref.SHAPES has."""
    Q, N, D = 13, 17, 4096
    q, s = R.exact_operands(np.random.RandomState(Q * N + D), Q, N, D)
    q[Q - 1] = s[N // 2]                                     # a query equal to a set row: exactly 0
    got, want = _distances(_bf16(q), _bf16(s)).cpu().numpy(), R.distances(q, s)
    assert np.array_equal(got.astype(np.float64), want)
    assert got[Q - 1, N // 2] == 0.0
