"""The scrunch kernels' summation order (aux_kernels.hip: np_pairwise_leaf,
np_pairwise_sum, scrunch_kernel), restated in numpy float32 operations and
compared with the reference's scrunch, data[:N].reshape(-1, f).mean(axis=1)
(oracle.scrunch), bit for bit.  No device: this is how the order is checked
where there is no GPU; tests/test_gpu_dered.py holds the kernels to the same
oracle."""
import numpy as np
import pytest

import dered_common as dc

F32 = np.float32
NP_BUFSIZE = 8192          # kNpBufSize (dered_host.hpp)


def leaf(a):
    """np_pairwise_leaf over the rows of a [rows, n <= 128]: fewer than 8
    addends in turn from 0; else 8 accumulators over the multiples of 8,
    combined pairwise, then the rest in turn."""
    n = a.shape[1]
    if n < 8:
        r = np.zeros(a.shape[0], F32)
        for i in range(n):
            r = r + a[:, i]
        return r
    r = [a[:, k].copy() for k in range(8)]
    i = 8
    while i < n - n % 8:
        for k in range(8):
            r[k] = r[k] + a[:, i + k]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for j in range(i, n):
        res = res + a[:, j]
    return res


def pairwise(a):
    """np_pairwise_sum: halving at multiples of 8 down to leaves of <= 128"""
    n = a.shape[1]
    if n <= 128:
        return leaf(a)
    n2 = n // 2
    n2 -= n2 % 8
    return pairwise(a[:, :n2]) + pairwise(a[:, n2:])


def kernel_sum(a):
    """scrunch_kernel: the pairwise sums of consecutive runs of 8192 samples
    (the last one shorter), added in turn"""
    acc = pairwise(a[:, :NP_BUFSIZE])
    for off in range(NP_BUFSIZE, a.shape[1], NP_BUFSIZE):
        acc = acc + pairwise(a[:, off:off + NP_BUFSIZE])
    return acc


def kernel_scrunch(x, f):
    a = x[:x.size // f * f].reshape(-1, f)
    s = kernel_sum(a)
    assert s.dtype == F32
    return (s.astype(np.float64) / float(f)).astype(F32)


# the factors of the device cases, the leaf's edges and factors further past the buffer size
FACTORS = sorted(set(dc.FACTORS) | {1, 6, 9, 15, 17, 127, 130, 153, 154, 8191, 8200, 9000, 16384, 20000, 24577, 40001})


@pytest.mark.parametrize("rows", [1, 37])
def test_kernel_summation_order_is_numpys(oracle, rows):
    assert np.getbufsize() == NP_BUFSIZE, \
        f"numpy's ufunc buffer holds {np.getbufsize()} elements, not {NP_BUFSIZE}: the scrunch kernels follow the latter"
    rs = np.random.RandomState(rows)
    bad = []
    for f in FACTORS:
        x = (rs.normal(size=rows * f + min(5, f - 1)) * 3.0 + 100.0).astype(F32)
        ref = oracle.scrunch(x, f)
        got = kernel_scrunch(x, f)
        assert ref.dtype == F32 and ref.shape == got.shape == (rows,)
        if not np.array_equal(ref.view(np.uint32), got.view(np.uint32)):
            bad.append(f)
    assert not bad, f"factors whose sums differ from numpy's: {bad}"


def test_one_recursion_differs_above_the_buffer_size(oracle):
    """What the chunking is for: a single pairwise recursion over the whole
    block is numpy's sum up to 8192 addends (and at 16384, whose first split
    falls on 8192) and not above."""
    rs = np.random.RandomState(3)
    same = {}
    for f in (4097, 8192, 8193, 10007, 16384, 16385):
        x = (rs.normal(size=37 * f) * 3.0 + 100.0).astype(F32)
        one = (pairwise(x.reshape(-1, f)).astype(np.float64) / float(f)).astype(F32)
        same[f] = bool(np.array_equal(one, oracle.scrunch(x, f)))
    assert same == {4097: True, 8192: True, 8193: False, 10007: False, 16384: True, 16385: False}
