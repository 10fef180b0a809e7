"""The order in which numpy sums a contiguous (n, 1) array over axis 0, restated in plain Python.

np.mean / np.var over axis 0 of an (n, D) array with D >= 2 add the rows one after another, feature by feature.  A ONE-feature
array is coalesced into a single inner reduce of n contiguous elements, and that loop is numpy's pairwise sum:

    n < 8      the elements one after another;
    n <= 128   eight running sums r[k] over the elements k, k + 8, k + 16, ... of the first n - n % 8, combined as
               ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the n % 8 tail elements one after another;
    n > 128    sum(x[:n2]) + sum(x[n2:]) with n2 = n // 2 rounded down to a multiple of 8, each half by the same rule;
    n > 8192   numpy hands that loop at most 8192 elements at a time (its buffer size) and adds the chunks' sums to the result one
               after another: ((0 + sum(x[:8192])) + sum(x[8192:16384])) + ...

This is what csrc/norm_math.h's norm_pairwise_sum does for a normaliser of one feature (a 1-D goal, say); the functions here are its
definition, and tests/test_numpy_pairwise_ref.py pins them against numpy itself, so a numpy that changed the order would show there.
Every operation is carried out in the array's own dtype (numpy scalars), so the results can be compared bit for bit."""
import numpy as np


CHUNK = 8192


def pairwise_sum(x):
    """Sum of the 1-D array x in numpy's order, as a scalar of x's dtype."""
    x = np.asarray(x)
    res = x.dtype.type(0)
    for base in range(0, len(x), CHUNK):
        res = res + _chunk_sum(x[base:base + CHUNK])
    return res


def _chunk_sum(x):
    n = len(x)
    if n < 8:
        res = x.dtype.type(0)
        for v in x:
            res = res + v
        return res
    if n <= 128:
        r = [x[k] for k in range(8)]
        i = 8
        while i < n - n % 8:
            for k in range(8):
                r[k] = r[k] + x[i + k]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        while i < n:
            res = res + x[i]
            i += 1
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return _chunk_sum(x[:n2]) + _chunk_sum(x[n2:])


def mean_var_one_feature(x):
    """(np.mean(x, axis=0), np.var(x, axis=0)) of a contiguous (n, 1) array, operation by operation: the sum over the rows, / n,
    the squared deviations, their sum, / n, all in x's dtype."""
    x = np.asarray(x)
    assert x.ndim == 2 and x.shape[1] == 1
    col, t = x[:, 0], x.dtype.type
    mean = pairwise_sum(col) / t(len(col))
    d = col - mean
    var = pairwise_sum(d * d) / t(len(col))
    return np.array([mean]), np.array([var])


def sequential_sum(x):
    """What a feature of a D >= 2 array gets: the rows one after another."""
    x = np.asarray(x)
    res = x.dtype.type(0)
    for v in x:
        res = res + v
    return res
