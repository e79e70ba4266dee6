"""GPU tests for the observed-ISC kernels (``ops.isc_loo`` /
``ops.isc_pairwise``: ``k_isc_totals``, ``k_isc_loo``, ``k_isc_pairwise``,
``k_isc_drop``), their dispatch from ``isc._isc_corr`` and the
``device="cuda"`` path of ``isc()``.

Oracles: the torch twin on the CPU (``device="cpu"``) and the numpy path
(``device=None``) on the same inputs.  NaN positions equal and
``atol=1e-12, rtol=0`` on the finite values: all three are centred
two-pass fp64 correlations of |r| <= 1 (the kernels are compiled without
multiply-add contraction, so products and sums round as on the host)
that differ in summation order only, a few ulp of 1.  Measured on the
MI355X: at most 6.7e-14 without a statistic and under 'median'; 2.6e-13
under 'mean' at 3 TRs, where correlations within 1e-4 of +-1 go through
atanh with a slope of 1 / (1 - r^2).
"""

import warnings

import numpy as np
import pytest
import torch

from brainiak_amd import isc as isc_mod
from brainiak_amd.isc import isc

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1, 2), (3, 63, 3), (31, 65, 5), (60, 130, 8), (60, 70, 17),
          (40, 66, 33)]
TOLERATE = [True, False, 0.8, 0.0]
STATS = [None, 'median', 'mean']


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from brainiak_amd import ops as _ops
    if _ops.load_extension() is None:
        pytest.fail("HIP extension not built — GPU box must load it")
    return _ops


def _case(n_TRs, n_voxels, n_subjects, offset, seed=0):
    """Shared signal plus noise, with (where there is room) a voxel that
    is NaN everywhere, a single NaN, a subject that is constant at one
    voxel, and a voxel whose only NaN-free subject is the last."""
    rng = np.random.RandomState(seed)
    data = rng.randn(n_TRs, n_voxels, 1) \
        + 1.5 * rng.randn(n_TRs, n_voxels, n_subjects) + offset
    if n_voxels > 5:
        data[:, 1, :] = np.nan
        data[n_TRs // 2, 2, n_subjects - 1] = np.nan
        data[:, 3, 0] = 2.0
        if n_subjects > 3:
            data[0, 4, :-1] = np.nan
    return data


def _check(got, want, label):
    assert isinstance(got, np.ndarray) and got.dtype == np.float64
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), label
    diff = float(np.nanmax(np.abs(got - want), initial=0.0))
    print(f"{label}: max|diff|={diff:.3e}")
    assert diff <= 1e-12, label


def _numpy_isc(data, **kw):
    """The numpy path, without its all-NaN-slice and 0/0 warnings."""
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return isc(data, **kw)


@pytest.fixture
def kernel_calls(ops, monkeypatch):
    """Counts calls of ops.isc_loo / ops.isc_pairwise (still running
    them)."""
    monkeypatch.delenv("BRAINIAK_ISC_CORR", raising=False)
    calls = {"loo": 0, "pairwise": 0}

    def counted(name, real):
        def wrapper(*args):
            calls[name] += 1
            return real(*args)
        return wrapper

    monkeypatch.setattr(ops, "isc_loo", counted("loo", ops.isc_loo))
    monkeypatch.setattr(ops, "isc_pairwise",
                        counted("pairwise", ops.isc_pairwise))
    return calls


def test_subject_cap_covers_32_subjects(ops):
    assert ops.isc_pairwise_max_subjects() >= 32


@pytest.mark.parametrize("pairwise", [False, True], ids=["loo", "pairwise"])
@pytest.mark.parametrize("offset", [0.0, 100.0])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cuda_equals_twin_and_numpy(kernel_calls, shape, offset, pairwise):
    data = _case(*shape, offset)
    name = "pairwise" if pairwise or shape[2] == 2 else "loo"
    n = 0
    for tolerate in TOLERATE:
        for stat in STATS:
            kw = dict(pairwise=pairwise, summary_statistic=stat,
                      tolerate_nans=tolerate)
            got = isc(data, device="cuda", **kw)
            n += 1
            assert kernel_calls[name] == n
            label = f"tolerate_nans={tolerate} stat={stat}"
            _check(got, isc(data, device="cpu", **kw), label + " vs twin")
            _check(got, _numpy_isc(data.copy(), **kw), label + " vs numpy")
    assert sum(kernel_calls.values()) == n


@pytest.mark.parametrize("pairwise,shape", [
    pytest.param(False, (12, 70, 70), id="loo-two-subject-slices"),
    pytest.param(False, (12, 70, 64), id="loo-64"),
    pytest.param(True, (12, 9, 64), id="pairwise-at-the-cap"),
    pytest.param(True, (20, 258, 4), id="pairwise-256-voxels-a-block"),
])
def test_cuda_at_the_kernels_other_paths(kernel_calls, pairwise, shape):
    data = _case(*shape, 100.0)
    for tolerate in (True, False):
        kw = dict(pairwise=pairwise, tolerate_nans=tolerate)
        got = isc(data, device="cuda", **kw)
        _check(got, isc(data, device="cpu", **kw),
               f"tolerate_nans={tolerate} vs twin")
        _check(got, _numpy_isc(data.copy(), **kw),
               f"tolerate_nans={tolerate} vs numpy")
    assert sum(kernel_calls.values()) == 2


@pytest.mark.parametrize("pairwise", [False, True], ids=["loo", "pairwise"])
def test_cuda_many_blocks_real_subject_count(kernel_calls, pairwise):
    data = _case(200, 1000, 32, 100.0)
    for stat in STATS:
        kw = dict(pairwise=pairwise, summary_statistic=stat)
        got = isc(data, device="cuda", **kw)
        _check(got, isc(data, device="cpu", **kw), f"stat={stat} vs twin")
        _check(got, _numpy_isc(data.copy(), **kw), f"stat={stat} vs numpy")
    assert kernel_calls["pairwise" if pairwise else "loo"] == 3


def test_pairwise_above_the_cap_takes_the_twin(ops, kernel_calls):
    n_subjects = ops.isc_pairwise_max_subjects() + 1
    data = _case(10, 7, n_subjects, 0.0)
    got = isc(data, pairwise=True, device="cuda")
    assert sum(kernel_calls.values()) == 0
    _check(got, isc(data, pairwise=True, device="cpu"), "above the cap")


@pytest.mark.parametrize("pairwise", [False, True], ids=["loo", "pairwise"])
def test_env_forces_the_twin(kernel_calls, monkeypatch, pairwise):
    monkeypatch.setenv("BRAINIAK_ISC_CORR", "torch")
    data = _case(31, 65, 5, 100.0)
    got = isc(data, pairwise=pairwise, device="cuda")
    assert sum(kernel_calls.values()) == 0
    _check(got, isc(data, pairwise=pairwise, device="cpu"), "twin on GPU")


def test_twin_median_above_the_row_cap_sorts_gpu_nans_last(kernel_calls,
                                                           monkeypatch):
    """136 pair rows take the statistic's torch twin, whose sort runs on
    the GPU; the NaNs that GPU arithmetic propagates may have their sign
    bit set and must still count as the largest values."""
    monkeypatch.setenv("BRAINIAK_ISC_CORR", "torch")
    data = _case(60, 70, 17, 0.0)
    kw = dict(pairwise=True, summary_statistic='median')
    got = isc(data, device="cuda", **kw)
    assert sum(kernel_calls.values()) == 0
    _check(got, isc(data, device="cpu", **kw), "median, twin on GPU")


@pytest.mark.parametrize("stat", STATS)
@pytest.mark.parametrize("pairwise", [False, True], ids=["loo", "pairwise"])
@pytest.mark.parametrize("resident", [False, True],
                         ids=["ndarray", "cuda-tensor"])
def test_chunked_equals_unchunked_bitwise(kernel_calls, monkeypatch,
                                          resident, pairwise, stat):
    """Host arrays are uploaded a chunk at a time; a tensor on the GPU is
    read in place, a window at a time."""
    data = _case(60, 130, 8, 100.0)
    arg = torch.from_numpy(data).cuda() if resident else data
    kw = dict(pairwise=pairwise, summary_statistic=stat, device="cuda")
    whole = isc(arg, **kw)
    monkeypatch.setattr(isc_mod, "_ISC_CHUNK_BYTES", 1)
    chunked = isc(arg, **kw)
    assert sum(kernel_calls.values()) == 1 + 3
    assert np.array_equal(chunked, whole, equal_nan=True)
    print("chunked vs whole: max|diff|=0 (bitwise)")


@pytest.mark.parametrize("pairwise", [False, True], ids=["loo", "pairwise"])
def test_cuda_tensor_input(kernel_calls, pairwise):
    data = _case(31, 65, 5, 100.0)
    kw = dict(pairwise=pairwise, device="cuda")
    want = isc(data, **kw)
    assert np.array_equal(isc(torch.from_numpy(data).cuda(), **kw), want,
                          equal_nan=True)
    # a host tensor, and a non-contiguous one on the GPU
    assert np.array_equal(isc(torch.from_numpy(data), **kw), want,
                          equal_nan=True)
    swapped = torch.from_numpy(data).cuda().permute(1, 0, 2).contiguous()
    assert np.array_equal(isc(swapped.permute(1, 0, 2), **kw), want,
                          equal_nan=True)
    data32 = data.astype(np.float32)
    got32 = isc(torch.from_numpy(data32).cuda(), **kw)
    assert got32.dtype == np.float64
    assert np.array_equal(got32, isc(data32.astype(np.float64), **kw),
                          equal_nan=True)
    assert sum(kernel_calls.values()) == 6
    print("tensor vs ndarray input: max|diff|=0 (bitwise)")


def test_window_offsets_beyond_2_to_31(ops):
    """A window at the end of an array of more than 2^31 elements: the
    offset t * V * S + v * S + s has to be formed in 64 bits.  Only the
    window is ever written or read."""
    n_TRs, n_voxels, n_subjects, nv = 3, 34_000_000, 32, 70
    assert (n_TRs - 1) * n_voxels * n_subjects >= 2 ** 31
    small = torch.from_numpy(_case(n_TRs, nv, n_subjects, 100.0)).cuda()
    try:
        big = torch.empty((n_TRs, n_voxels, n_subjects),
                          dtype=torch.float64, device="cuda")
    except torch.OutOfMemoryError:
        pytest.fail("needs 27 GB of device memory")
    v0 = n_voxels - nv
    big[:, v0:, :] = small
    for tolerant in (True, False):
        got = ops.isc_loo(big, tolerant, -1.0, v0, nv)
        want = ops.isc_loo(small, tolerant)
        assert got.shape == (n_subjects, nv)
        assert torch.equal(got.nan_to_num(2.0), want.nan_to_num(2.0))
    got = ops.isc_pairwise(big, 0.8 * n_subjects, v0, nv)
    want = ops.isc_pairwise(small, 0.8 * n_subjects)
    assert torch.equal(got.nan_to_num(2.0), want.nan_to_num(2.0))
    print("window at 2^31 vs small array: max|diff|=0 (bitwise)")
    del big
    torch.cuda.empty_cache()


def test_binding_rejects_bad_arguments(ops):
    data = torch.from_numpy(_case(31, 65, 5, 0.0)).cuda()
    cap = ops.isc_pairwise_max_subjects()
    for call in (lambda d, *w: ops.isc_loo(d, True, -1.0, *w),
                 lambda d, *w: ops.isc_pairwise(d, -1.0, *w)):
        assert call(data).shape[1] == 65
        assert call(data, 60, 0).shape[1] == 0
        with pytest.raises(RuntimeError):
            call(data.cpu())
        with pytest.raises(RuntimeError):
            call(data.float())
        with pytest.raises(RuntimeError):
            call(data.transpose(0, 1))
        with pytest.raises(RuntimeError):
            call(data[:, :, :1].contiguous())            # S < 2
        with pytest.raises(RuntimeError):
            call(data[:0])                               # T < 1
        with pytest.raises(RuntimeError):
            call(data[0])                                # 2-D
        with pytest.raises(RuntimeError):
            call(data, 60, 6)                            # window past V
        with pytest.raises(RuntimeError):
            call(data, -1, 5)
    wide = torch.zeros((4, 3, cap + 1), dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError):
        ops.isc_pairwise(wide)


def test_observed_from_the_device_feeds_the_null(kernel_calls):
    from brainiak_amd.isc import timeshift_isc
    data = _case(37, 11, 5, 0.0)
    obs = isc(data, summary_statistic='median', device="cuda")
    kw = dict(summary_statistic='median', n_shifts=20, random_state=13,
              device="cuda")
    got = timeshift_isc(data, observed=obs, **kw)
    want = timeshift_isc(data, **kw)
    assert np.array_equal(got[0], obs, equal_nan=True)
    _check(got[0], want[0], "observed")
    assert np.array_equal(got[2], want[2], equal_nan=True)
