"""The summation scheme of the parameter-gradient kernels (include/flatland_param_grads.h, policy._tn) restated in numpy, and the
a-priori error bounds the tests hold the kernels and this restatement to.

Scheme: the rows go in blocks of REDUCE_BLOCK = 256; a block's product dZ^T X is formed in float32; the blocks of a slice are added
in float64 in block order, the last block ragged; a slice is ceil(blocks / slices) whole blocks; the slices' float64 sums are added
in slice order and rounded to float32 once.  A bias is the float64 column sum of dZ taken in the same block and slice order.

Bounds, per element, with u = 2^-24 (float32's unit roundoff), valid for ANY order of the additions inside a block -- derived, not
measured.  A block's float32 sum of at most 256 products carries at most 255 additions and one rounding of each product, to first
order 256 u sum_r |dZ[r,p] X[r,q]| over the block, so over all blocks

    |g - g64| <= 256 u sum_r |dZ[r,p] X[r,q]| + u |g64|

the last term being the one rounding of the total to float32 (the float64 additions of the block sums are 2^-29 of that and are
not counted).  A bias is n numbers added in float64 and rounded once:

    |b - b64| <= u |b64| + n 2^-53 sum_r |dZ[r,p]|

The bound functions work on numpy arrays and on torch tensors alike (float64 operands expected).
"""
import numpy as np

REDUCE_BLOCK = 256
U = 2.0 ** -24


def slice_blocks(n_rows, slices):
    """[(first block, block behind the last)] of every slice: ceil(blocks / slices) whole blocks each, the late ones empty"""
    blocks = -(-n_rows // REDUCE_BLOCK)
    per = -(-blocks // slices)
    return [(min(s * per, blocks), min((s + 1) * per, blocks)) for s in range(slices)]


def _blockwise(n_rows, slices, term, shape):
    total = None
    for b0, b1 in slice_blocks(n_rows, slices):
        acc = np.zeros(shape, dtype=np.float64)
        for b in range(b0, b1):
            acc = acc + term(slice(b * REDUCE_BLOCK, min(n_rows, (b + 1) * REDUCE_BLOCK)))
        total = acc if total is None else total + acc
    return total.astype(np.float32)


def tn(dz, x, slices=1):
    """sum over the rows of dZ^T X: dz f32 [n, p], x f32 [n, q] -> f32 [p, q]"""
    assert dz.dtype == np.float32 and x.dtype == np.float32 and dz.shape[0] == x.shape[0]
    return _blockwise(dz.shape[0], slices, lambda rows: np.matmul(dz[rows].T, x[rows]).astype(np.float64), (dz.shape[1], x.shape[1]))


def colsum(dz, slices=1):
    """the float64 column sum of dZ in block order: dz f32 [n, p] -> f32 [p]"""
    assert dz.dtype == np.float32
    return _blockwise(dz.shape[0], slices, lambda rows: dz[rows].astype(np.float64).sum(0), (dz.shape[1],))


def weight_bound(dz64, x64, g64):
    """the per-element bound of a weight gradient: dz64 [n, p], x64 [n, q], g64 [p, q], all float64"""
    return REDUCE_BLOCK * U * (abs(dz64).T @ abs(x64)) + U * abs(g64)


def bias_bound(dz64, g64):
    """the per-element bound of a bias gradient: dz64 [n, p], g64 [p], float64"""
    return U * abs(g64) + dz64.shape[0] * 2.0 ** -53 * abs(dz64).sum(0)


def fraction(g, g64, bound):
    """the largest |g - g64| / bound over the elements (0 where both are 0; inf where the bound is 0 and the error is not)"""
    err = abs(g - g64)
    worst = 0.0
    nz = bound > 0
    if bool(nz.any()):
        worst = float((err[nz] / bound[nz]).max())
    if bool((err[~nz] > 0).any()):
        worst = float("inf")
    return worst
