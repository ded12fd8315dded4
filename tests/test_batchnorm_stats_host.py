"""The forward statistics of dn_batchnorm_rows_* (csrc/dn_norm.hip) restated in NumPy fp32, without a GPU: (count, mean, M2) per 64-row
chunk, each chunk's sums about a shift of its own (its first row), merged by Chan's formula in its k-way form -- mean = sum n_k mean_k
/ N, M2 = sum M2_k + sum n_k (mean_k - mean)^2 -- in the kernel's fixed order (8 slices of chunks slice, slice + 8, ..., then the slices).  Held to the tolerances of tests/test_gpu_kernels.py::
test_batch_norm_rows_matches_torch on the same inputs: the draw of that test with row 0 moved K standard deviations off the column mean and
column 0 constant except for row 0.  The form the kernel had before -- ONE shift for the whole matrix (row 0), var = s2 / N - d * d -- is
restated next to it: it loses the variance on these inputs, which is what the test inputs are for."""
import numpy as np
import pytest

f32 = np.float32
CHUNK, BLOCK, SLICES = 64, 256, 8


def _inputs(N, C, K):
    rng = np.random.default_rng(N + C)
    x = rng.standard_normal((N, C)) * 2.0 + 30.0 * rng.standard_normal(C)
    if K:
        x0 = x.copy()
        x[0] = x0.mean(0) + K * 2.0
        x[1:, 0] = x0[1, 0]
    return x.astype(f32)


def _chunk_sums(x, r0, r1, shift):
    """(sum d, sum d^2), d = x - shift, over rows r0 .. r1 as a workgroup adds them: row groups r0 + g, r0 + g + GPB, ..., then the groups in order"""
    C = x.shape[1]
    gpb = BLOCK // (C // 4)
    t1, t2 = np.zeros(C, f32), np.zeros(C, f32)
    for g in range(gpb):
        a, b = np.zeros(C, f32), np.zeros(C, f32)
        for r in range(r0 + g, r1, gpb):
            d = x[r] - shift
            a = a + d
            b = b + d * d
        t1, t2 = t1 + a, t2 + b
    return t1, t2


def _sliced(terms):
    """sum of per-chunk terms in the kernel's order: slice j adds chunks j, j + 8, ..., then the slices in order"""
    sl = []
    for j in range(SLICES):
        a = np.zeros_like(terms[0])
        for k in range(j, len(terms), SLICES):
            a = a + terms[k]
        sl.append(a)
    t = sl[0]
    for j in range(1, SLICES):
        t = t + sl[j]
    return t


def stats_chunked(x):
    """mean, biased variance as the kernel forms them now: mean = sum n_k mean_k / N (about chunk 0's mean), M2 = sum M2_k + sum
    n_k (mean_k - mean)^2 -- Chan's merge in its k-way form, every term of M2 >= 0"""
    N, C = x.shape
    nchunks = -(-N // CHUNK)
    part = []
    for k in range(nchunks):
        r0, r1 = k * CHUNK, min(N, (k + 1) * CHUNK)
        t1, t2 = _chunk_sums(x, r0, r1, x[r0])
        d = t1 * f32(1.0 / (r1 - r0))
        part.append((f32(r1 - r0), x[r0] + d, np.maximum(t2 - t1 * d, f32(0))))
    ref = part[0][1]
    mean = ref + _sliced([n * (m - ref) for n, m, _ in part]) / f32(N)
    m2 = _sliced([q + n * (m - mean) * (m - mean) for n, m, q in part])
    return mean, np.maximum(m2 / f32(N), f32(0))


def stats_one_shift(x):
    """... and as it formed them before: every chunk about row 0, plain sums, var = s2 / N - d * d"""
    N, C = x.shape
    s1, s2 = np.zeros(C, f32), np.zeros(C, f32)
    parts = [_chunk_sums(x, k * CHUNK, min(N, (k + 1) * CHUNK), x[0]) for k in range(-(-N // CHUNK))]
    sl = []
    for j in range(SLICES):
        a, b = np.zeros(C, f32), np.zeros(C, f32)
        for k in range(j, len(parts), SLICES):
            a, b = a + parts[k][0], b + parts[k][1]
        sl.append((a, b))
    for a, b in sl:
        s1, s2 = s1 + a, s2 + b
    inv = f32(1.0 / N)
    d = s1 * inv
    return x[0] + d, np.maximum(s2 * inv - d * d, f32(0))


@pytest.mark.parametrize("K", [0, 30, 300, 1000])
@pytest.mark.parametrize("N,C", [(5000, 128), (20181, 256), (300, 40)])
def test_chunked_chan_statistics_hold_the_projects_tolerances(N, C, K):
    x = _inputs(N, C, K)
    mean, var = stats_chunked(x)
    x64 = x.astype(np.float64)
    np.testing.assert_allclose(mean, x64.mean(0), rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(var, x64.var(0), rtol=2e-4, atol=1e-5)


def test_one_shift_statistics_lose_the_variance_when_row_0_is_far_out():
    """What the inputs are for: the earlier form misses the 2e-4 of the variance at (20181, 256) once row 0 lies 300 deviations out."""
    x = _inputs(20181, 256, 300)
    v64 = x.astype(np.float64).var(0)
    err_old = float(np.max(np.abs(stats_one_shift(x)[1] - v64) / v64))
    err_new = float(np.max(np.abs(stats_chunked(x)[1] - v64) / v64))
    assert err_old > 2e-4 > 10 * err_new, (err_old, err_new)
