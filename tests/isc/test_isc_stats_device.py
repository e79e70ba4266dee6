"""The device path of the ISC resampling nulls, run on the CPU
(``device="cpu"``: the torch twin of the HIP kernel), against the numpy
path with the same seed.

Comparison rules:

* ``'median'``: the null distribution is EQUAL, NaN positions included —
  the same draws select the same values and only selection and one exact
  halving are involved.
* ``'mean'`` and the time-shift test: ``atol=1e-12``.  With |x| <= 0.999,
  atanh is below 3.8, a few ulp of which is ~3e-15; averaging does not
  grow that and tanh is 1-Lipschitz.  The time-shift statistics move by
  at most the lag table's error, and the FFT table differs from the
  direct one by ~3e-16.
* ``p`` is equal wherever no null value lies within 1e-9 of the value it
  is compared with, which the seeded inputs guarantee for the bootstrap,
  the randomised one-sample permutation test and the time-shift test
  (asserted).  The exact tests and the two-sample test contain the
  observed grouping itself (the identity sign pattern; every label order
  that keeps the groups), so their nulls tie with the observed statistic
  by construction; there the two p-values may differ by no more than
  those tied entries, which for ``'median'`` (equal distributions) is
  again equality.

Every test prints the measured max |diff|.
"""

from itertools import combinations

import numpy as np
import pytest
import torch

from brainiak_amd import isc as isc_mod
from brainiak_amd.isc import (bootstrap_isc, isc, permutation_isc,
                              timeshift_isc)

STATS = ['median', 'mean']
SIDES = ['right', 'left', 'two-sided']
NAN_VOXEL = 2


def _data(n_TRs, n_voxels, n_subjects, seed):
    """Shared signal plus subject noise; one voxel NaN in every
    subject."""
    rng = np.random.RandomState(seed)
    signal = rng.randn(n_TRs, n_voxels, 1)
    data = signal + 1.5 * rng.randn(n_TRs, n_voxels, n_subjects)
    data[:, NAN_VOXEL, :] = np.nan
    return data


def _iscs(n_subjects, pairwise, seed, n_voxels=7):
    """ISCs of the seeded data, with a NaN voxel and one more missing
    entry (so the surviving count differs between voxels)."""
    iscs = isc(_data(60, n_voxels, n_subjects, seed), pairwise=pairwise)
    iscs[1, 4] = np.nan
    assert np.nanmax(np.abs(iscs)) < 0.999
    return iscs


def _max_diff(a, b):
    both = np.isfinite(a) & np.isfinite(b)
    return float(np.max(np.abs(a[both] - b[both]))) if both.any() else 0.0


def _check_null(stat, dist_dev, dist_np):
    assert dist_dev.shape == dist_np.shape
    assert isinstance(dist_dev, np.ndarray)
    assert dist_dev.dtype == np.float64
    assert np.array_equal(np.isnan(dist_dev), np.isnan(dist_np))
    assert np.isnan(dist_np[:, NAN_VOXEL]).all()
    assert np.isfinite(dist_np).any()
    print(f"{stat}: null max|diff|={_max_diff(dist_dev, dist_np):.3e}")
    if stat == 'median':
        assert np.array_equal(dist_dev, dist_np, equal_nan=True)
    else:
        np.testing.assert_allclose(dist_dev, dist_np, rtol=0, atol=1e-12)


def _check_p(side, p_dev, p_np, compared, observed, denom, ties_expected):
    """``compared`` is the numpy-path array that p_from_null holds
    against ``observed``."""
    if side == 'two-sided':
        compared, observed = np.abs(compared), np.abs(observed)
    with np.errstate(invalid="ignore"):
        near = np.abs(compared - observed) <= 1e-9
    n_near = near.sum(axis=0)
    print(f"side={side}: null values within 1e-9 of the observed "
          f"statistic: {int(n_near.sum())}")
    if not ties_expected:
        assert n_near.sum() == 0
    p_dev, p_np = np.ravel(p_dev), np.ravel(p_np)
    assert p_dev.shape == p_np.shape == np.ravel(n_near).shape
    # counts are integers: allow half a count of rounding
    assert np.all(np.abs(p_dev - p_np) * denom <= np.ravel(n_near) + 0.5)
    if not n_near.any():
        assert np.array_equal(p_dev, p_np)


# -- bootstrap ---------------------------------------------------------------

@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("stat", STATS)
@pytest.mark.parametrize("pairwise", [False, True],
                         ids=["loo", "pairwise"])
def test_bootstrap_matches_numpy_path(pairwise, stat, side):
    iscs = _iscs(5, pairwise, seed=3)
    kw = dict(pairwise=pairwise, summary_statistic=stat, n_bootstraps=50,
              side=side, random_state=11)
    obs_np, ci_np, p_np, dist_np = bootstrap_isc(iscs, **kw)
    obs, ci, p, dist = bootstrap_isc(iscs, device="cpu", **kw)
    assert dist.shape == (50, 7)
    _check_null(stat, dist, dist_np)
    assert np.array_equal(obs, obs_np, equal_nan=True)
    for got, want in zip(ci, ci_np):
        if stat == 'median':
            assert np.array_equal(got, want, equal_nan=True)
        else:
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    _check_p(side, p, p_np, dist_np - obs_np, obs_np, 51,
             ties_expected=False)


# -- permutation -------------------------------------------------------------

@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("stat", STATS)
@pytest.mark.parametrize("pairwise", [False, True],
                         ids=["loo", "pairwise"])
@pytest.mark.parametrize("n_subjects,n_perm,groups,exact,seed", [
    # seed 19: no flipped median happens to land on the observed one
    pytest.param(12, 40, None, False, 19, id="one-sample-random"),
    pytest.param(4, 16, None, True, 7, id="one-sample-exact"),
    pytest.param(5, 40, [0, 0, 0, 1, 1], False, 7, id="two-sample-random"),
    pytest.param(5, 120, [0, 0, 0, 1, 1], True, 7, id="two-sample-exact"),
])
def test_permutation_matches_numpy_path(n_subjects, n_perm, groups, exact,
                                        seed, pairwise, stat, side):
    iscs = _iscs(n_subjects, pairwise, seed=5)
    kw = dict(group_assignment=groups, pairwise=pairwise,
              summary_statistic=stat, n_permutations=n_perm, side=side,
              random_state=seed)
    obs_np, p_np, dist_np = permutation_isc(iscs, **kw)
    obs, p, dist = permutation_isc(iscs, device="cpu", **kw)
    assert dist.shape == (n_perm, 7)
    _check_null(stat, dist, dist_np)
    assert np.array_equal(obs, obs_np, equal_nan=True)
    _check_p(side, p, p_np, dist_np, obs_np,
             n_perm if exact else n_perm + 1,
             ties_expected=exact or groups is not None)


def test_permutation_two_sample_takes_array_assignment():
    iscs = _iscs(5, False, seed=5)
    kw = dict(summary_statistic='median', n_permutations=40,
              random_state=7)
    _, p_np, dist_np = permutation_isc(
        iscs, group_assignment=np.array([1, 2, 1, 2, 1]), **kw)
    _, p, dist = permutation_isc(
        iscs, group_assignment=np.array([1, 2, 1, 2, 1]), device="cpu",
        **kw)
    assert np.array_equal(dist, dist_np, equal_nan=True)
    assert np.array_equal(p, p_np)


# -- time shift --------------------------------------------------------------

@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("stat", STATS)
@pytest.mark.parametrize("n_TRs", [37, 40], ids=["odd-T", "even-T"])
def test_timeshift_matches_numpy_path(n_TRs, stat, side):
    data = _data(n_TRs, 11, 5, seed=2)
    kw = dict(pairwise=False, summary_statistic=stat, n_shifts=20,
              side=side, random_state=13)
    obs_np, p_np, dist_np = timeshift_isc(data, **kw)
    obs, p, dist = timeshift_isc(data, device="cpu", **kw)
    assert dist.shape == (20, 11)
    assert np.array_equal(np.isnan(dist), np.isnan(dist_np))
    assert np.isnan(dist[:, NAN_VOXEL]).all()
    assert np.isfinite(np.delete(dist, NAN_VOXEL, axis=1)).all()
    print(f"{stat}: null max|diff|={_max_diff(dist, dist_np):.3e}")
    np.testing.assert_allclose(dist, dist_np, rtol=0, atol=1e-12)
    assert np.array_equal(obs, obs_np, equal_nan=True)
    _check_p(side, p, p_np, dist_np, obs_np, 21, ties_expected=False)


def test_timeshift_voxel_chunks_share_the_draws(monkeypatch):
    """A byte budget that forces several voxel chunks changes nothing."""
    data = _data(37, 150, 5, seed=4)
    kw = dict(summary_statistic='median', n_shifts=6, random_state=1,
              device="cpu")
    _, _, whole = timeshift_isc(data, **kw)
    monkeypatch.setattr(isc_mod, "_TIMESHIFT_CHUNK_BYTES", 1)
    calls = []
    real = isc_mod._resample_stat

    def counted(*args):
        calls.append(args[0].shape[2])
        return real(*args)

    monkeypatch.setattr(isc_mod, "_resample_stat", counted)
    _, _, chunked = timeshift_isc(data, **kw)
    assert calls == [64, 64, 22]
    assert np.array_equal(whole, chunked, equal_nan=True)


def test_timeshift_lag_table_is_the_rolled_correlation():
    """C[s, k, v] against np.roll + np.corrcoef, every lag."""
    data = _data(9, 4, 3, seed=6)[:, [0, 1, 3], :]
    x = torch.from_numpy(data).permute(2, 0, 1).contiguous()
    table = isc_mod._timeshift_lag_table(x).numpy()
    assert table.shape == (3, 9, 3)
    worst = 0.0
    for s in range(3):
        others = np.delete(data, s, axis=2).mean(axis=2)
        for k in range(9):
            for v in range(3):
                r = np.corrcoef(np.roll(data[:, v, s], k),
                                others[:, v])[0, 1]
                worst = max(worst, abs(r - table[s, k, v]))
    print(f"lag table max|diff|={worst:.3e}")
    assert worst <= 1e-12


def test_timeshift_pairwise_device_raises():
    data = _data(20, 3, 4, seed=0)
    with pytest.raises(ValueError, match="leave-one-out"):
        timeshift_isc(data, pairwise=True, n_shifts=2, device="cpu")


# -- _resample_stat on the CPU against a plain numpy loop ---------------------

def _loop_oracle(table, rows, lags, signs, stat):
    n_draws, n_rows = rows.shape
    n_voxels = table.shape[2]
    out = np.full((n_draws, n_voxels), np.nan)
    for i in range(n_draws):
        for v in range(n_voxels):
            vals = []
            for r in range(n_rows):
                if signs[i, r] == 0:
                    continue
                lag = 0 if lags is None else lags[i, r]
                x = signs[i, r] * table[rows[i, r], lag, v]
                if not np.isnan(x):
                    vals.append(x)
            if not vals:
                continue
            if stat == 'median':
                out[i, v] = np.median(np.array(vals))
            else:
                with np.errstate(divide="ignore", invalid="ignore"):
                    out[i, v] = np.tanh(np.mean(np.arctanh(
                        np.array(vals))))
    return out


def _run(table, rows, lags, signs, stat):
    out = isc_mod._resample_stat(torch.from_numpy(table), rows, lags,
                                 signs, stat)
    assert out.dtype == torch.float64 and out.device.type == "cpu"
    assert out.shape == (rows.shape[0], table.shape[2])
    return out.numpy()


def _compare(got, want, stat):
    assert np.array_equal(np.isnan(got), np.isnan(want))
    print(f"{stat}: max|diff|={_max_diff(got, want):.3e}")
    if stat == 'median':
        assert np.array_equal(got, want, equal_nan=True)
    else:
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("stat", STATS)
@pytest.mark.parametrize("n_rows", [1, 2, 3, 8])
@pytest.mark.parametrize("n_lags", [1, 5])
def test_resample_stat_matches_loop(n_lags, n_rows, stat):
    rng = np.random.RandomState(n_rows * 10 + n_lags)
    table = rng.uniform(-0.999, 0.999, size=(6, n_lags, 9))
    table[:, :, 3] = np.nan                    # a NaN column
    table[2, :, :] = np.nan                    # a NaN row
    rows = rng.randint(0, 6, size=(7, n_rows))
    rows[1, :] = rows[1, 0]                    # ties
    lags = rng.randint(0, n_lags, size=(7, n_rows))
    lags[0, :] = 0
    lags[1, :] = n_lags - 1
    signs = rng.choice([-1, 0, 1], size=(7, n_rows), p=[0.3, 0.2, 0.5])
    signs[4, :] = 0                            # nothing survives
    signs[5, :] = 1
    got = _run(table, rows, lags, signs, stat)
    want = _loop_oracle(table, rows, lags, signs, stat)
    assert np.isnan(got[4]).all() and np.isnan(got[:, 3]).all()
    assert np.isfinite(got[5]).any()
    _compare(got, want, stat)
    if n_lags == 1:
        _compare(_run(table, rows, None, signs, stat), want, stat)


def test_resample_stat_even_count_takes_the_mean_of_the_middle():
    table = np.array([0.1, 0.4, 0.2, 0.8]).reshape(4, 1, 1)
    rows = np.arange(4)[None, :]
    got = _run(table, rows, None, np.ones((1, 4), dtype=np.int8),
               'median')
    assert got[0, 0] == (0.2 + 0.4) / 2
    # leaving one out makes the count odd
    got = _run(table, rows, None, np.array([[1, 1, 1, 0]]), 'median')
    assert got[0, 0] == 0.2
    # a sign flip moves the entry to the other end
    got = _run(table, rows, None, np.array([[1, 1, 1, -1]]), 'median')
    assert got[0, 0] == (0.1 + 0.2) / 2


def test_resample_stat_mean_of_a_lone_one_is_exactly_one():
    table = np.array([1.0, -1.0, 0.5]).reshape(3, 1, 1)
    one = np.ones((1, 1), dtype=np.int8)
    assert _run(table, np.array([[0]]), None, one, 'mean')[0, 0] == 1.0
    assert _run(table, np.array([[1]]), None, one, 'mean')[0, 0] == -1.0
    assert _run(table, np.array([[1]]), None, -one, 'mean')[0, 0] == 1.0
    # +inf outweighs any finite atanh; +inf with -inf is NaN
    both = np.ones((1, 2), dtype=np.int8)
    assert _run(table, np.array([[0, 2]]), None, both, 'mean')[0, 0] == 1.0
    assert np.isnan(_run(table, np.array([[0, 1]]), None, both,
                         'mean')[0, 0])


def test_resample_stat_chunks_over_draws(monkeypatch):
    rng = np.random.RandomState(0)
    table = rng.uniform(-0.9, 0.9, size=(5, 3, 10))
    rows = rng.randint(0, 5, size=(9, 4))
    lags = rng.randint(0, 3, size=(9, 4))
    signs = rng.choice([-1, 0, 1], size=(9, 4))
    for stat in STATS:
        whole = _run(table, rows, lags, signs, stat)
        # two draws per chunk: 4 rows x 10 voxels x 8 B x copies each
        monkeypatch.setattr(
            isc_mod, "_RESAMPLE_CHUNK_BYTES",
            2 * 4 * 10 * 8 * isc_mod._RESAMPLE_CHUNK_COPIES)
        assert np.array_equal(_run(table, rows, lags, signs, stat),
                              whole, equal_nan=True)
        monkeypatch.undo()


@pytest.mark.parametrize("bad", ["row-high", "row-negative", "lag-high",
                                 "lag-negative", "sign", "shape",
                                 "stat", "float-rows"])
def test_resample_stat_rejects_bad_arguments(bad):
    table = torch.zeros((3, 4, 5), dtype=torch.float64)
    rows = np.zeros((2, 3), dtype=np.int64)
    lags = np.zeros((2, 3), dtype=np.int64)
    signs = np.ones((2, 3), dtype=np.int8)
    stat = 'median'
    if bad == "row-high":
        rows[1, 2] = 3
    elif bad == "row-negative":
        rows[0, 0] = -1
    elif bad == "lag-high":
        lags[1, 0] = 4
    elif bad == "lag-negative":
        lags[0, 1] = -1
    elif bad == "sign":
        signs[0, 0] = 2
    elif bad == "shape":
        signs = signs[:, :2]
    elif bad == "stat":
        stat = 'max'
    else:
        rows = rows.astype(float)
    with pytest.raises(ValueError):
        isc_mod._resample_stat(table, rows, lags, signs, stat)


def test_bootstrap_pair_index_is_combinations_order(monkeypatch):
    """The condensed index the pairwise bootstrap computes is the
    position of the pair in itertools.combinations."""
    n = 6
    order = {pair: k for k, pair in enumerate(combinations(range(n), 2))}
    seen = {}

    def capture(iscs, rows, signs, stat, device):
        seen["rows"], seen["signs"] = rows, signs
        return np.zeros((rows.shape[0], iscs.shape[1]))

    draws = np.sort(np.random.RandomState(0).randint(0, n, size=(30, n)),
                    axis=1)
    iscs = np.zeros((len(order), 2))
    monkeypatch.setattr(isc_mod, "_rows_null_device", capture)
    isc_mod._bootstrap_null_device(iscs, draws, n, True, 'median', "cpu")
    for b in range(30):
        for k, (i, j) in enumerate(combinations(range(n), 2)):
            a, c = draws[b, i], draws[b, j]
            if a == c:
                assert seen["signs"][b, k] == 0
            else:
                assert seen["signs"][b, k] == 1
                assert seen["rows"][b, k] == order[(a, c)]
