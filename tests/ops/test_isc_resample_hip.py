"""GPU tests for the ISC resampling kernel (``ops.isc_resample_stat`` /
``k_isc_resample_stat``), its dispatch from ``isc._resample_stat`` and
the ``device="cuda"`` path of the public tests.

Oracle: the torch twin run on the CPU on the same tensors.

* ``'median'``: ``torch.equal`` on the values, NaN positions equal.  No
  tolerance: only selection and one exact halving are involved.
* ``'mean'``: ``atol=1e-12``.  Inputs stay within |x| <= 0.999, where
  atanh is below 3.8 and a few ulp of it is ~3e-15; the mean does not
  grow that and tanh is 1-Lipschitz.
* the time-shift test end to end: ``atol=1e-12`` for both statistics,
  since the lag table comes from two different FFT libraries (measured
  CPU FFT against the direct sum: ~3e-16).
"""

import numpy as np
import pytest
import torch

from brainiak_amd import isc as isc_mod
from brainiak_amd.isc import (bootstrap_isc, isc, permutation_isc,
                              timeshift_isc)

pytestmark = pytest.mark.gpu

STATS = ['median', 'mean']


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from brainiak_amd import ops as _ops
    if _ops.load_extension() is None:
        pytest.fail("HIP extension not built — GPU box must load it")
    return _ops


def _case(n_draws, n_rows, n_lags, n_voxels, seed, n_table=6):
    """Table and draws with everything that can go wrong in a column:
    a NaN row, an all-NaN voxel, ties, signs 0 and -1, a draw with
    every sign 0, lags at both ends."""
    rng = np.random.RandomState(seed)
    table = rng.uniform(-0.999, 0.999, size=(n_table, n_lags, n_voxels))
    table[2] = np.nan
    if n_voxels > 1:
        table[:, :, n_voxels // 2] = np.nan
    rows = rng.randint(0, n_table, size=(n_draws, n_rows))
    lags = rng.randint(0, n_lags, size=(n_draws, n_rows))
    lags[:, 0] = 0
    lags[:, -1] = n_lags - 1
    signs = rng.choice([-1, 0, 1], size=(n_draws, n_rows),
                       p=[0.3, 0.2, 0.5])
    signs[0, 0] = 1
    if n_draws > 1:
        rows[1, :] = rows[1, 0]                # the same row R times
        lags[1, :] = lags[1, 0]
        signs[1, :] = 1
    if n_draws > 2:
        signs[2, :] = 0                        # nothing survives
    return (torch.from_numpy(table), torch.from_numpy(rows).int(),
            torch.from_numpy(lags).int(), torch.from_numpy(signs).to(
                torch.int8))


def _oracle(table, rows, lags, signs, stat):
    return isc_mod._resample_stat(table, rows, lags, signs, stat)


def _kernel(ops, table, rows, lags, signs, stat):
    out = ops.isc_resample_stat(
        table.cuda(), rows.cuda(), None if lags is None else lags.cuda(),
        signs.cuda(), stat)
    torch.cuda.synchronize()
    return out.cpu()


def _check(out, ref, stat, atol_median=None):
    assert out.dtype == torch.float64 and out.shape == ref.shape
    assert torch.equal(torch.isnan(out), torch.isnan(ref))
    diff = float((out - ref).nan_to_num().abs().max()) if out.numel() \
        else 0.0
    print(f"{stat}: max|diff|={diff:.3e}")
    if stat == 'median' and atol_median is None:
        assert torch.equal(out.nan_to_num(), ref.nan_to_num())
    else:
        assert diff <= 1e-12


def _resolve_rows(ops, n_rows):
    cap = ops.isc_resample_max_rows()
    return {"cap-1": cap - 1, "cap": cap}.get(n_rows, n_rows)


def test_row_cap_covers_128_subjects(ops):
    assert ops.isc_resample_max_rows() >= 128


@pytest.mark.parametrize("stat", STATS)
@pytest.mark.parametrize("n_rows", [1, 2, 3, 8, "cap-1", "cap"])
@pytest.mark.parametrize("n_voxels", [1, 63, 64, 65, 130])
def test_kernel_equals_cpu_oracle(ops, n_voxels, n_rows, stat):
    n_rows = _resolve_rows(ops, n_rows)
    for n_draws in (1, 3):
        for n_lags in (1, 5):
            table, rows, lags, signs = _case(
                n_draws, n_rows, n_lags, n_voxels,
                seed=n_voxels * 1000 + n_rows * 10 + n_draws + n_lags)
            ref = _oracle(table, rows, lags, signs, stat)
            _check(_kernel(ops, table, rows, lags, signs, stat), ref, stat)
            if n_draws > 2:
                assert torch.isnan(ref[2]).all()
            if n_lags == 1:
                _check(_kernel(ops, table, rows, None, signs, stat), ref,
                       stat)


@pytest.mark.parametrize("stat", STATS)
def test_kernel_many_draws_subject_counts(ops, stat):
    """Several hundred blocks at a real subject count, no entry left
    out: every column is full."""
    table, rows, lags, signs = _case(70, 32, 7, 200, seed=9, n_table=32)
    signs = torch.where(signs == 0, torch.ones_like(signs), signs)
    ref = _oracle(table, rows, lags, signs, stat)
    _check(_kernel(ops, table, rows, lags, signs, stat), ref, stat)


def test_kernel_even_count_and_lone_one(ops):
    table = torch.tensor([0.1, 0.4, 0.2, 0.8, 1.0, -1.0],
                         dtype=torch.float64).reshape(6, 1, 1)
    rows = torch.tensor([[0, 1, 2, 3], [0, 1, 2, 3], [4, 4, 4, 4],
                         [5, 0, 0, 0], [4, 5, 0, 0]], dtype=torch.int32)
    signs = torch.tensor([[1, 1, 1, 1], [1, 1, 1, 0], [1, 0, 0, 0],
                          [-1, 0, 0, 0], [1, 1, 0, 0]], dtype=torch.int8)
    med = _kernel(ops, table, rows, None, signs, 'median')[:, 0]
    assert med[0] == (0.2 + 0.4) / 2 and med[1] == 0.2
    mean = _kernel(ops, table, rows, None, signs, 'mean')[:, 0]
    # atanh(+-1) = +-inf: a lone 1 is exactly 1, +inf with -inf is NaN
    assert mean[2] == 1.0 and mean[3] == 1.0 and torch.isnan(mean[4])
    for stat in STATS:
        _check(_kernel(ops, table, rows, None, signs, stat),
               _oracle(table, rows, None, signs, stat), stat)


def test_kernel_offsets_beyond_2_to_31(ops):
    """A table of more than 2^31 elements: the offset (row * L + lag) * V
    + v has to be formed in 64 bits.  Only the two gathered rows are
    ever written or read."""
    n_table, n_lags, n_voxels = 16385, 2, 65536
    assert (n_table - 1) * n_lags * n_voxels >= 2 ** 31
    g = torch.Generator().manual_seed(3)
    small = torch.rand((2, 1, n_voxels), generator=g,
                       dtype=torch.float64) * 1.9 - 0.95
    try:
        big = torch.empty((n_table, n_lags, n_voxels), dtype=torch.float64,
                          device="cuda")
    except torch.OutOfMemoryError:
        pytest.fail("needs 17 GB of device memory")
    big[0, 0] = small[0, 0].cuda()
    big[n_table - 1, 1] = small[1, 0].cuda()
    rows = torch.tensor([[0, n_table - 1]], dtype=torch.int32)
    lags = torch.tensor([[0, 1]], dtype=torch.int32)
    signs = torch.tensor([[1, -1]], dtype=torch.int8)
    small_rows = torch.tensor([[0, 1]], dtype=torch.int32)
    for stat in STATS:
        out = ops.isc_resample_stat(big, rows.cuda(), lags.cuda(),
                                    signs.cuda(), stat).cpu()
        _check(out, _oracle(small, small_rows, None, signs, stat), stat)
    del big
    torch.cuda.empty_cache()


def test_kernel_empty_shapes(ops):
    table = torch.zeros((3, 2, 5), dtype=torch.float64)
    rows = torch.zeros((0, 4), dtype=torch.int32)
    signs = torch.zeros((0, 4), dtype=torch.int8)
    assert _kernel(ops, table, rows, None, signs, 'median').shape == (0, 5)
    # no rows per draw: nothing survives
    rows = torch.zeros((2, 0), dtype=torch.int32)
    signs = torch.zeros((2, 0), dtype=torch.int8)
    for stat in STATS:
        out = _kernel(ops, table, rows, None, signs, stat)
        assert out.shape == (2, 5) and torch.isnan(out).all()


def test_binding_rejects_bad_arguments(ops):
    cap = ops.isc_resample_max_rows()
    table, rows, lags, signs = (t.cuda() for t in _case(2, 3, 2, 10, 0))
    with pytest.raises(RuntimeError):
        ops.isc_resample_stat(table.cpu(), rows, lags, signs, 'median')
    with pytest.raises(RuntimeError):
        ops.isc_resample_stat(table.float(), rows, lags, signs, 'median')
    with pytest.raises(RuntimeError):
        ops.isc_resample_stat(table, rows.long(), lags, signs, 'median')
    with pytest.raises(RuntimeError):
        ops.isc_resample_stat(table, rows, lags[:, :2].contiguous(), signs,
                              'median')
    with pytest.raises(RuntimeError):
        ops.isc_resample_stat(table, rows, lags, signs.int(), 'median')
    with pytest.raises(RuntimeError):
        ops.isc_resample_stat(table.transpose(1, 2), rows, lags, signs,
                              'median')
    with pytest.raises(RuntimeError):
        ops.isc_resample_stat(table, rows, lags, signs, 'max')
    wide = torch.zeros((2, cap + 1), dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError):
        ops.isc_resample_stat(table, wide, None, wide.to(torch.int8),
                              'median')


# -- dispatch ---------------------------------------------------------------

@pytest.fixture
def kernel_calls(ops, monkeypatch):
    """Counts calls of ops.isc_resample_stat (still running it)."""
    monkeypatch.delenv("BRAINIAK_ISC_RESAMPLE", raising=False)
    calls = []
    real = ops.isc_resample_stat

    def counted(*args):
        calls.append(1)
        return real(*args)

    monkeypatch.setattr(ops, "isc_resample_stat", counted)
    return calls


@pytest.mark.parametrize("stat", STATS)
def test_dispatch_uses_kernel_on_gpu(kernel_calls, stat):
    table, rows, lags, signs = _case(3, 8, 5, 65, seed=1)
    ref = _oracle(table, rows, lags, signs, stat)
    out = isc_mod._resample_stat(table.cuda(), rows, lags, signs, stat)
    assert len(kernel_calls) == 1 and out.is_cuda
    _check(out.cpu(), ref, stat)
    # numpy indices are taken as well
    out = isc_mod._resample_stat(table.cuda(), rows.numpy(), lags.numpy(),
                                 signs.numpy(), stat)
    assert len(kernel_calls) == 2
    _check(out.cpu(), ref, stat)


@pytest.mark.parametrize("stat", STATS)
def test_dispatch_env_forces_torch(kernel_calls, monkeypatch, stat):
    monkeypatch.setenv("BRAINIAK_ISC_RESAMPLE", "torch")
    table, rows, lags, signs = _case(3, 8, 5, 65, seed=1)
    ref = _oracle(table, rows, lags, signs, stat)
    out = isc_mod._resample_stat(table.cuda(), rows, lags, signs, stat)
    assert len(kernel_calls) == 0 and out.is_cuda
    _check(out.cpu(), ref, stat)


def test_dispatch_rows_above_cap(ops, kernel_calls):
    """'median' beyond the cap stays on the torch twin (on the GPU) and
    still matches; 'mean' has no cap."""
    n_rows = ops.isc_resample_max_rows() + 1
    table, rows, lags, signs = _case(3, n_rows, 5, 65, seed=2)
    ref = _oracle(table, rows, lags, signs, 'median')
    out = isc_mod._resample_stat(table.cuda(), rows, lags, signs, 'median')
    assert len(kernel_calls) == 0 and out.is_cuda
    _check(out.cpu(), ref, 'median')
    ref = _oracle(table, rows, lags, signs, 'mean')
    out = isc_mod._resample_stat(table.cuda(), rows, lags, signs, 'mean')
    assert len(kernel_calls) == 1
    _check(out.cpu(), ref, 'mean')


def test_dispatch_checks_ranges_before_the_kernel(kernel_calls):
    table, rows, lags, signs = _case(2, 3, 2, 10, seed=0)
    bad = rows.clone()
    bad[0, 0] = 6
    with pytest.raises(ValueError):
        isc_mod._resample_stat(table.cuda(), bad, lags, signs, 'median')
    bad = lags.clone()
    bad[1, 1] = 2
    with pytest.raises(ValueError):
        isc_mod._resample_stat(table.cuda(), rows, bad, signs, 'median')
    assert len(kernel_calls) == 0


# -- end to end: device="cuda" against device="cpu" --------------------------

def _data(n_TRs, n_voxels, n_subjects, seed):
    rng = np.random.RandomState(seed)
    data = rng.randn(n_TRs, n_voxels, 1) \
        + 1.5 * rng.randn(n_TRs, n_voxels, n_subjects)
    data[:, 2, :] = np.nan
    return data


def _iscs(n_subjects, pairwise, seed):
    iscs = isc(_data(60, 7, n_subjects, seed), pairwise=pairwise)
    iscs[1, 4] = np.nan
    return iscs


def _check_np(got, want, stat, exact_median=True):
    _check(torch.from_numpy(np.asarray(got, dtype=np.float64)),
           torch.from_numpy(np.asarray(want, dtype=np.float64)), stat,
           atol_median=None if exact_median else 1e-12)


@pytest.mark.parametrize("stat", STATS)
@pytest.mark.parametrize("pairwise", [False, True],
                         ids=["loo", "pairwise"])
def test_bootstrap_cuda_equals_cpu(kernel_calls, pairwise, stat):
    iscs = _iscs(5, pairwise, seed=3)
    kw = dict(pairwise=pairwise, summary_statistic=stat, n_bootstraps=50,
              random_state=11)
    obs_c, ci_c, p_c, dist_c = bootstrap_isc(iscs, device="cpu", **kw)
    obs, ci, p, dist = bootstrap_isc(iscs, device="cuda", **kw)
    assert len(kernel_calls) == 1
    assert isinstance(dist, np.ndarray) and dist.shape == (50, 7)
    _check_np(dist, dist_c, stat)
    assert np.array_equal(obs, obs_c, equal_nan=True)
    assert np.array_equal(p, p_c)
    for got, want in zip(ci, ci_c):
        _check_np(got, want, stat)


@pytest.mark.parametrize("stat", STATS)
@pytest.mark.parametrize("pairwise", [False, True],
                         ids=["loo", "pairwise"])
@pytest.mark.parametrize("n_subjects,n_perm,groups,seed,launches", [
    pytest.param(12, 40, None, 19, 1, id="one-sample-random"),
    pytest.param(4, 16, None, 7, 1, id="one-sample-exact"),
    pytest.param(5, 40, [0, 0, 0, 1, 1], 7, 2, id="two-sample-random"),
    pytest.param(5, 120, [0, 0, 0, 1, 1], 7, 2, id="two-sample-exact"),
])
def test_permutation_cuda_equals_cpu(kernel_calls, n_subjects, n_perm,
                                     groups, seed, launches, pairwise,
                                     stat):
    iscs = _iscs(n_subjects, pairwise, seed=5)
    kw = dict(group_assignment=groups, pairwise=pairwise,
              summary_statistic=stat, n_permutations=n_perm,
              random_state=seed)
    obs_c, p_c, dist_c = permutation_isc(iscs, device="cpu", **kw)
    obs, p, dist = permutation_isc(iscs, device="cuda", **kw)
    assert len(kernel_calls) == launches
    assert isinstance(dist, np.ndarray) and dist.shape == (n_perm, 7)
    _check_np(dist, dist_c, stat)
    assert np.array_equal(obs, obs_c, equal_nan=True)
    # equal distributions give equal p; under 'mean' only the randomised
    # one-sample inputs are free of ties with the observed statistic
    # (asserted by the CPU test), the others tie by construction
    if stat == 'median' or launches == 1 and n_perm == 40:
        assert np.array_equal(p, p_c)


@pytest.mark.parametrize("stat", STATS)
@pytest.mark.parametrize("n_TRs", [37, 40], ids=["odd-T", "even-T"])
def test_timeshift_cuda_equals_cpu(kernel_calls, n_TRs, stat):
    data = _data(n_TRs, 11, 5, seed=2)
    kw = dict(summary_statistic=stat, n_shifts=20, random_state=13)
    obs_c, p_c, dist_c = timeshift_isc(data, device="cpu", **kw)
    obs, p, dist = timeshift_isc(data, device=torch.device("cuda"), **kw)
    assert len(kernel_calls) == 1
    assert isinstance(dist, np.ndarray) and dist.shape == (20, 11)
    assert np.isnan(dist[:, 2]).all()
    _check_np(dist, dist_c, stat, exact_median=False)
    assert np.array_equal(obs, obs_c, equal_nan=True)
    # the CPU test asserts that these inputs leave no null value within
    # 1e-9 of the observed statistic
    assert np.array_equal(p, p_c)


def test_timeshift_pairwise_cuda_raises(ops):
    with pytest.raises(ValueError, match="leave-one-out"):
        timeshift_isc(_data(20, 3, 4, seed=0), pairwise=True, n_shifts=2,
                      device="cuda")
