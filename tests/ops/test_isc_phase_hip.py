"""GPU tests for the phase-randomisation kernel (``ops.isc_phase_stat`` /
``k_isc_phase_stat``), its dispatch from ``isc._phase_stat`` and the
``device="cuda"`` path of ``phaseshift_isc``.

Oracle: the torch twin (a batched matmul, then the statistic) run on the
CPU on the same tensors.

``atol=1e-12`` for both statistics, NaN positions equal.  The kernel adds
the K products of a row in k order with one fused multiply-add each, the
matmul in whatever order its BLAS takes, so nothing is bit-equal: the two
sums differ by a few ulp of values below 1, ~1e-15.  The inputs keep
every sum within |x| <= 0.9 (tables within +-0.9 / K, coefficients within
+-1), where atanh grows that by at most 1 / (1 - 0.81) = 5.3.  End to
end the spectra come from two FFT libraries as well (the time-shift test
measured ~3e-16 between them) and |x| stays below 0.7 at the 37 and 40
TRs used.
"""

import numpy as np
import pytest
import torch

from brainiak_amd import isc as isc_mod
from brainiak_amd.isc import phaseshift_isc

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


def _case(n_draws, n_rows, n_cols, n_voxels, seed):
    """Table and coefficients with everything that can go wrong in a
    column: a NaN row, an all-NaN voxel, and two identical rows with
    identical coefficients (ties, and an even count where the rest is
    odd)."""
    rng = np.random.RandomState(seed)
    table = rng.uniform(-0.9 / n_cols, 0.9 / n_cols,
                        size=(n_rows, n_cols, n_voxels))
    coef = rng.uniform(-1.0, 1.0, size=(n_draws, n_rows, n_cols))
    if n_rows >= 2:
        table[-1] = table[0]
        coef[:, -1] = coef[:, 0]
    if n_rows >= 4:
        table[1] = np.nan
    if n_voxels > 1:
        table[:, :, n_voxels // 2] = np.nan
    return torch.from_numpy(table), torch.from_numpy(coef)


def _oracle(table, coef, stat):
    return isc_mod._phase_stat_torch(table, coef, stat)


def _kernel(ops, table, coef, stat):
    out = ops.isc_phase_stat(table.cuda(), coef.cuda(), stat)
    torch.cuda.synchronize()
    return out.cpu()


def _check(out, ref, stat):
    assert out.dtype == torch.float64 and out.shape == ref.shape
    assert torch.equal(torch.isnan(out), torch.isnan(ref))
    diff = float((out - ref).nan_to_num().abs().max()) if out.numel() \
        else 0.0
    print(f"{stat}: max|diff|={diff:.3e}")
    assert diff <= 1e-12


def test_row_cap_covers_128_rows(ops):
    assert ops.isc_phase_max_rows() >= 128


# Rows on both sides of each draw-tile switch of the median path (4 draws
# per block up to 32 rows, 2 up to 64, 1 up to the cap), voxels below / at /
# above one wave and in several waves, columns around the unroll of 8
# (tails of 1..7, one full group, one group and a tail), draws around the
# tiles of 1, 2, 4 ('median') and 8 ('mean').  A thinned product: every
# value of every axis appears with both statistics.
VOXELS = [1, 63, 64, 65, 130]
ROWS = [1, 2, 3, 8, 32, 33, 64, 65, "cap"]
COLS = [1, 2, 3, 5, 9, 8, 17]
DRAWS = [1, 3, 5, 9]
SHAPES = sorted({(VOXELS[(i + s) % len(VOXELS)], ROWS[i % len(ROWS)],
                  COLS[(i + 2 * s) % len(COLS)],
                  DRAWS[(i + 3 * s) % len(DRAWS)])
                 for s in range(3) for i in range(len(ROWS))},
                key=str)


def test_thinned_product_covers_every_value():
    for axis, values in enumerate((VOXELS, ROWS, COLS, DRAWS)):
        assert {shape[axis] for shape in SHAPES} == set(values)


@pytest.mark.parametrize("stat", STATS)
@pytest.mark.parametrize("n_voxels,n_rows,n_cols,n_draws", SHAPES)
def test_kernel_matches_cpu_twin(ops, n_voxels, n_rows, n_cols, n_draws,
                                 stat):
    if n_rows == "cap":
        n_rows = ops.isc_phase_max_rows()
    table, coef = _case(n_draws, n_rows, n_cols, n_voxels,
                        seed=n_voxels * 1000 + n_rows * 10 + n_cols)
    ref = _oracle(table, coef, stat)
    if n_voxels > 1:
        assert torch.isnan(ref[:, n_voxels // 2]).all()
        assert torch.isfinite(ref[:, 0]).all()
    _check(_kernel(ops, table, coef, stat), ref, stat)


@pytest.mark.parametrize("stat", STATS)
def test_kernel_many_blocks_real_shape(ops, stat):
    """Several hundred blocks at a real subject count and series length
    (200 TRs: 199 columns, a row is 24 full groups and a tail of 7)."""
    table, coef = _case(70, 32, 199, 200, seed=9)
    _check(_kernel(ops, table, coef, stat), _oracle(table, coef, stat),
           stat)


def test_kernel_even_count_and_lone_one(ops):
    nan = float("nan")
    columns = torch.tensor([[0.1, 0.4, 0.2, 0.8], [0.1, 0.4, 0.2, nan],
                            [nan, nan, nan, nan], [1.0, nan, nan, nan],
                            [1.0, -1.0, nan, nan]], dtype=torch.float64)
    table = columns.T[:, None, :].contiguous()          # [4, 1, 5]
    coef = torch.ones((1, 4, 1), dtype=torch.float64)
    med = _kernel(ops, table, coef, 'median')[0]
    assert med[0] == (0.2 + 0.4) / 2 and med[1] == 0.2
    assert torch.isnan(med[2]) and med[3] == 1.0 and med[4] == 0.0
    mean = _kernel(ops, table, coef, 'mean')[0]
    # atanh(+-1) = +-inf: a lone 1 is exactly 1, +inf with -inf is NaN
    assert mean[3] == 1.0 and torch.isnan(mean[2]) and torch.isnan(mean[4])
    for stat in STATS:
        _check(_kernel(ops, table, coef, stat), _oracle(table, coef, stat),
               stat)


def test_kernel_offsets_beyond_2_to_31(ops):
    """A table of more than 2^31 elements: the offset (r * K + k) * V + v
    has to be formed in 64 bits.  All rows but the last are zero, so
    'mean' is tanh(atanh(x_last) / R) of the last row's sum."""
    n_rows, n_cols, n_voxels = 16385, 2, 65536
    assert (n_rows * n_cols - 1) * n_voxels >= 2 ** 31
    g = torch.Generator().manual_seed(3)
    last = torch.rand((n_cols, n_voxels), generator=g,
                      dtype=torch.float64) * 0.9 - 0.45
    try:
        big = torch.zeros((n_rows, n_cols, n_voxels), dtype=torch.float64,
                          device="cuda")
    except torch.OutOfMemoryError:
        pytest.fail("needs 17 GB of device memory")
    big[n_rows - 1] = last.cuda()
    coef = torch.ones((1, n_rows, n_cols), dtype=torch.float64)
    out = ops.isc_phase_stat(big, coef.cuda(), 'mean').cpu()
    ref = torch.tanh(torch.atanh(last.sum(dim=0)) / n_rows)[None, :]
    _check(out, ref, 'mean')
    assert float(ref.abs().max()) > 1e-6
    del big
    torch.cuda.empty_cache()


def test_kernel_no_draws(ops):
    table, coef = _case(0, 3, 2, 5, seed=0)
    for stat in STATS:
        assert _kernel(ops, table, coef, stat).shape == (0, 5)


def test_binding_rejects_bad_arguments(ops):
    cap = ops.isc_phase_max_rows()
    table, coef = (t.cuda() for t in _case(2, 3, 4, 10, 0))
    with pytest.raises(RuntimeError):
        ops.isc_phase_stat(table.cpu(), coef, 'median')
    with pytest.raises(RuntimeError):
        ops.isc_phase_stat(table, coef.cpu(), 'median')
    with pytest.raises(RuntimeError):
        ops.isc_phase_stat(table.float(), coef, 'median')
    with pytest.raises(RuntimeError):
        ops.isc_phase_stat(table, coef.float(), 'median')
    with pytest.raises(RuntimeError):
        ops.isc_phase_stat(table.transpose(1, 2), coef.transpose(1, 2),
                           'median')                   # not contiguous
    with pytest.raises(RuntimeError):
        ops.isc_phase_stat(table, coef[:, :, ::2], 'median')
    with pytest.raises(RuntimeError):
        ops.isc_phase_stat(table, coef[:, :2].contiguous(), 'median')
    with pytest.raises(RuntimeError):
        ops.isc_phase_stat(table, coef[:, :, :3].contiguous(), 'median')
    with pytest.raises(RuntimeError):
        ops.isc_phase_stat(table, coef[0], 'median')
    with pytest.raises(RuntimeError):
        ops.isc_phase_stat(table, coef, 'max')
    with pytest.raises(RuntimeError):
        ops.isc_phase_stat(table[:, :0], coef[:, :, :0], 'mean')
    wide_t, wide_c = (t.cuda() for t in _case(2, cap + 1, 2, 10, 0))
    with pytest.raises(RuntimeError):
        ops.isc_phase_stat(wide_t, wide_c, 'median')


# -- dispatch ---------------------------------------------------------------

@pytest.fixture
def kernel_calls(ops, monkeypatch):
    """Counts calls of ops.isc_phase_stat (still running it)."""
    monkeypatch.delenv("BRAINIAK_ISC_RESAMPLE", raising=False)
    calls = []
    real = ops.isc_phase_stat

    def counted(*args):
        calls.append(1)
        return real(*args)

    monkeypatch.setattr(ops, "isc_phase_stat", counted)
    return calls


@pytest.mark.parametrize("stat", STATS)
def test_dispatch_uses_kernel_on_gpu(kernel_calls, stat):
    table, coef = _case(3, 8, 5, 65, seed=1)
    out = isc_mod._phase_stat(table.cuda(), coef.cuda(), stat)
    assert len(kernel_calls) == 1 and out.is_cuda
    _check(out.cpu(), _oracle(table, coef, stat), stat)
    # a CPU table stays on the twin
    out = isc_mod._phase_stat(table, coef, stat)
    assert len(kernel_calls) == 1 and not out.is_cuda


@pytest.mark.parametrize("stat", STATS)
def test_dispatch_env_forces_torch(ops, kernel_calls, monkeypatch, stat):
    table, coef = _case(5, 8, 5, 65, seed=1)
    kernel = _kernel(ops, table, coef, stat)
    monkeypatch.setenv("BRAINIAK_ISC_RESAMPLE", "torch")
    out = isc_mod._phase_stat(table.cuda(), coef.cuda(), stat)
    assert len(kernel_calls) == 1 and out.is_cuda      # _kernel's own call
    _check(out.cpu(), kernel, stat)
    _check(out.cpu(), _oracle(table, coef, stat), stat)


def test_dispatch_rows_above_cap(ops, kernel_calls):
    """'median' beyond the cap stays on the torch twin (on the GPU) and
    still matches; the raw op refuses it; 'mean' has no cap."""
    n_rows = ops.isc_phase_max_rows() + 1
    table, coef = _case(3, n_rows, 5, 65, seed=2)
    out = isc_mod._phase_stat(table.cuda(), coef.cuda(), 'median')
    assert len(kernel_calls) == 0 and out.is_cuda
    _check(out.cpu(), _oracle(table, coef, 'median'), 'median')
    with pytest.raises(RuntimeError, match="rows"):
        ops.isc_phase_stat(table.cuda(), coef.cuda(), 'median')
    out = isc_mod._phase_stat(table.cuda(), coef.cuda(), 'mean')
    assert len(kernel_calls) == 2
    _check(out.cpu(), _oracle(table, coef, 'mean'), 'mean')


# -- end to end: device="cuda" against device="cpu" --------------------------

def _data(n_TRs, n_voxels, n_subjects, seed):
    rng = np.random.RandomState(seed)
    data = rng.randn(n_TRs, n_voxels, 1) \
        + 1.5 * rng.randn(n_TRs, n_voxels, n_subjects)
    data[:, 2, :] = np.nan
    data[:, 5, 1] = np.nan
    return data


@pytest.mark.parametrize("stat", STATS)
@pytest.mark.parametrize("pairwise", [False, True],
                         ids=["loo", "pairwise"])
@pytest.mark.parametrize("n_TRs", [37, 40], ids=["odd-T", "even-T"])
def test_phaseshift_cuda_equals_cpu(kernel_calls, n_TRs, pairwise, stat):
    data = _data(n_TRs, 70, 5, seed=2)
    kw = dict(pairwise=pairwise, summary_statistic=stat, n_shifts=20,
              random_state=13)
    obs_c, p_c, dist_c = phaseshift_isc(data, device="cpu", **kw)
    obs, p, dist = phaseshift_isc(data, device=torch.device("cuda"), **kw)
    assert len(kernel_calls) == 1
    assert isinstance(dist, np.ndarray) and dist.shape == (20, 70)
    assert np.isnan(dist[:, 2]).all()
    assert np.isnan(dist[:, 5]).all() == (not pairwise)
    assert np.isfinite(np.delete(dist, [2, 5], axis=1)).all()
    _check(torch.from_numpy(dist), torch.from_numpy(dist_c), stat)
    assert np.array_equal(obs, obs_c, equal_nan=True)
    # p is equal where no null value lies within 1e-9 of the observed
    # statistic: nowhere, for these inputs
    with np.errstate(invalid="ignore"):
        near = np.abs(dist_c - obs_c) <= 1e-9
    print(f"null values within 1e-9 of the observed statistic: "
          f"{int(near.sum())}")
    assert near.sum() == 0
    assert np.array_equal(p, p_c, equal_nan=True)
