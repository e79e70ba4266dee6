"""``isc(..., device="cpu")``: the torch twin of the observed-ISC device
path against the numpy path, and the ``observed=`` keyword of
``timeshift_isc`` / ``phaseshift_isc``.

Tolerance: NaN positions equal and ``atol=1e-12, rtol=0`` on the finite
values, the bound of the project's other ISC device tests.  Both paths
are centred two-pass fp64 correlations of |r| <= 1 that differ in
summation order only, a few ulp of 1.  Measured on these inputs: at
most 1e-14 without a statistic and under 'median'; 2.6e-13 under 'mean'
at 3 TRs, where correlations within 1e-4 of +-1 go through atanh with a
slope of 1 / (1 - r^2).
"""

import warnings

import numpy as np
import pytest
import torch

from brainiak_amd import isc as isc_mod
from brainiak_amd.isc import isc, phaseshift_isc, timeshift_isc

SHAPES = [(2, 1, 2), (3, 63, 3), (31, 65, 5), (60, 130, 8), (60, 70, 17),
          (40, 66, 33)]
TOLERATE = [True, False, 0.8, 0.0]
STATS = [None, 'median', 'mean']


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
    assert got.shape == want.shape and want.dtype == np.float64
    assert np.array_equal(np.isnan(got), np.isnan(want)), label
    diff = float(np.nanmax(np.abs(got - want), initial=0.0))
    print(f"{label}: max|diff|={diff:.3e}")
    assert diff <= 1e-12, label


def _numpy_isc(data, **kw):
    """The numpy path, without its all-NaN-slice and 0/0 warnings."""
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return isc(data, **kw)


@pytest.mark.parametrize("pairwise", [False, True], ids=["loo", "pairwise"])
@pytest.mark.parametrize("offset", [0.0, 100.0])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_device_cpu_equals_numpy(shape, offset, pairwise):
    data = _case(*shape, offset)
    for tolerate in TOLERATE:
        for stat in STATS:
            kw = dict(pairwise=pairwise, summary_statistic=stat,
                      tolerate_nans=tolerate)
            want = _numpy_isc(data.copy(), **kw)
            got = isc(data, device="cpu", **kw)
            _check(got, want, f"tolerate_nans={tolerate} stat={stat}")


def test_planted_voxels_behave_as_documented():
    data = _case(60, 130, 8, 100.0)
    out = isc(data, device=torch.device("cpu"))
    assert np.isnan(out[:, 1]).all()            # NaN everywhere: dropped
    assert np.isnan(out[7, 2]) and not np.isnan(out[:7, 2]).any()
    assert np.isnan(out[0, 3]) and not np.isnan(out[1:, 3]).any()
    assert not np.isnan(np.delete(out, [1, 2, 3, 4], axis=1)).any()
    # plain means: the single NaN reaches every row of its voxel
    assert np.isnan(isc(data, tolerate_nans=False, device="cpu")[:, 2]).all()
    # 7 of 8 clean subjects pass 0.8, 1 of 8 does not
    out = isc(data, tolerate_nans=0.8, device="cpu")
    assert not np.isnan(out[:7, 2]).any() and np.isnan(out[:, 4]).all()


@pytest.mark.parametrize("stat", STATS)
@pytest.mark.parametrize("pairwise", [False, True], ids=["loo", "pairwise"])
def test_chunked_equals_unchunked_bitwise(monkeypatch, pairwise, stat):
    data = _case(60, 130, 8, 100.0)
    kw = dict(pairwise=pairwise, summary_statistic=stat, device="cpu")
    whole = isc(data, **kw)
    windows = []
    real = isc_mod._isc_chunk_to_device

    def recording(x, a, b, *rest):
        windows.append((a, b))
        return real(x, a, b, *rest)

    monkeypatch.setattr(isc_mod, "_isc_chunk_to_device", recording)
    monkeypatch.setattr(isc_mod, "_ISC_CHUNK_BYTES", 1)
    chunked = isc(data, **kw)
    assert windows == [(0, 64), (64, 128), (128, 130)]
    assert np.array_equal(chunked, whole, equal_nan=True)
    print("chunked vs whole: max|diff|=0 (bitwise)")


@pytest.mark.parametrize("pairwise", [False, True], ids=["loo", "pairwise"])
def test_tensor_input(pairwise):
    data = _case(31, 65, 5, 100.0)
    kw = dict(pairwise=pairwise, device="cpu")
    want = isc(data, **kw)
    got = isc(torch.from_numpy(data), **kw)
    assert np.array_equal(got, want, equal_nan=True)
    data32 = data.astype(np.float32)
    want32 = isc(data32.astype(np.float64), **kw)
    got32 = isc(torch.from_numpy(data32), **kw)
    assert got32.dtype == np.float64
    assert np.array_equal(got32, want32, equal_nan=True)
    # an fp32 ndarray is computed in fp64 as well
    assert np.array_equal(isc(data32, **kw), want32, equal_nan=True)
    print("tensor vs ndarray input: max|diff|=0 (bitwise)")
    with pytest.raises(ValueError):
        isc(torch.from_numpy(data)[0], **kw)


def test_list_and_2d_input():
    data = _case(31, 65, 5, 0.0)
    as_list = [data[..., s] for s in range(5)]
    _check(isc(list(as_list), device="cpu"), _numpy_isc(list(as_list)),
           "list of [T, V]")
    series = [data[:, 0, s] for s in range(5)]
    _check(isc(list(series), device="cpu"), _numpy_isc(list(series)),
           "list of [T]")
    flat = data[:, 0, :]
    for pairwise in (False, True):
        got = isc(flat, pairwise=pairwise, device="cpu")
        assert got.shape == ((10, 1) if pairwise else (5, 1))
        _check(got, _numpy_isc(flat, pairwise=pairwise),
               f"2-D pairwise={pairwise}")
    got = isc(flat, summary_statistic='median', device="cpu")
    assert got.shape == (1,)
    _check(got, _numpy_isc(flat, summary_statistic='median'),
           "2-D median")


def test_two_subjects_ignore_the_summary():
    data = _case(31, 65, 2, 100.0)
    got = isc(data, summary_statistic='mean', device="cpu")
    assert got.shape == (65,)
    _check(got, _numpy_isc(data, summary_statistic='mean'), "two subjects")


def test_bad_arguments_raise():
    data = _case(31, 7, 5, 0.0)
    for bad in (1.5, -0.1):
        with pytest.raises(ValueError, match="between 0.0 and 1.0"):
            isc(data, tolerate_nans=bad, device="cpu")
    with pytest.raises(ValueError, match="'mean' or 'median'"):
        isc(data, summary_statistic='max', device="cpu")


# -- observed= of the null tests ---------------------------------------------

def _same_triple(got, want):
    assert len(got) == len(want) == 3
    for g, w in zip(got, want):
        assert np.array_equal(g, w, equal_nan=True)


@pytest.mark.parametrize("pairwise", [False, True], ids=["loo", "pairwise"])
@pytest.mark.parametrize("null", [timeshift_isc, phaseshift_isc],
                         ids=["timeshift", "phaseshift"])
def test_observed_keyword_replaces_the_internal_call(null, pairwise):
    data = _case(31, 7, 5, 0.0)
    kw = dict(pairwise=pairwise, summary_statistic='median', n_shifts=5,
              random_state=4)
    obs = isc(data, pairwise=pairwise, summary_statistic='median')
    _same_triple(null(data, observed=obs, **kw), null(data, **kw))
    # the device path of the null takes it as well
    if not (pairwise and null is timeshift_isc):
        _same_triple(null(data, observed=obs, device="cpu", **kw),
                     null(data, device="cpu", **kw))
    # what is passed is what comes back
    marked = obs + 0.25
    assert np.array_equal(null(data, observed=marked, **kw)[0], marked,
                          equal_nan=True)
    print("observed= vs internal isc: max|diff|=0 (bitwise)")


@pytest.mark.parametrize("null", [timeshift_isc, phaseshift_isc],
                         ids=["timeshift", "phaseshift"])
def test_observed_of_the_wrong_shape_raises(null):
    data = _case(31, 7, 5, 0.0)
    kw = dict(summary_statistic='median', n_shifts=2, random_state=0)
    with pytest.raises(ValueError, match="observed"):
        null(data, observed=np.zeros(6), **kw)
    with pytest.raises(ValueError, match="observed"):
        null(data, observed=isc(data), **kw)         # [5, 7], not [7]
    with pytest.raises(ValueError, match="observed"):
        null(data, pairwise=True, device=None,
             observed=isc(data, pairwise=True), **kw)
