"""The device path of the phase-randomisation null, run on the CPU
(``phaseshift_isc(device="cpu")``: the torch twin of the HIP kernel
``k_isc_phase_stat``), against the numpy path with the same seed.

Comparison rules:

* the null distribution: NaN positions equal and ``atol=1e-12``,
  ``rtol=0`` for both statistics.  'median' is not bit-equal here: the
  selected values themselves come from a different summation (a dot
  product with the spectra instead of an FFT round trip and a
  correlation).  Both routes carry a few ulp of O(1) quantities, ~1e-15;
  1e-12 is the tolerance the time-shift test already applies.
* 'mean': atanh grows an input error by 1 / (1 - x^2), so every value
  that enters the statistic has to stay within |x| <= 0.99 (a factor of
  at most 50, asserted on the twin's own pre-statistic values).  The
  seeds below were chosen so that this holds; at 3 TRs a null value is
  cos(phase + const) and exceeds 0.99 for 9 % of the phases, hence the
  few draws at 3 and 4 TRs (``_n_shifts``).
* ``observed`` is equal, and ``p`` is equal wherever no null value lies
  within 1e-9 of the value it is compared with (asserted to be
  everywhere).

Every test prints the measured max |diff|.
"""

from itertools import combinations

import numpy as np
import pytest
import torch

from brainiak_amd import isc as isc_mod
from brainiak_amd.isc import isc, phaseshift_isc
from brainiak_amd.utils.utils import array_correlation, phase_randomize

STATS = ['median', 'mean']
SIDES = ['right', 'left', 'two-sided']
N_VOXELS = 5
NAN_VOXEL = 2          # NaN in every subject
NAN_ONE_VOXEL = 3      # NaN in subject 1 only
DATA_SEED = 2

# random_state per (n_TRs, n_subjects, pairwise): the first seed for
# which every pre-statistic value of the twin stays within 0.99
SEEDS = {
    (3, 3, False): 3, (3, 3, True): 3,
    (3, 5, False): 40, (3, 5, True): 634,
    (4, 3, False): 0, (4, 3, True): 0,
    (4, 5, False): 4, (4, 5, True): 16,
    (5, 3, False): 2, (5, 3, True): 2,
    (5, 5, False): 0, (5, 5, True): 2,
    (37, 3, False): 0, (37, 3, True): 0,
    (37, 5, False): 0, (37, 5, True): 0,
    (40, 3, False): 0, (40, 3, True): 0,
    (40, 5, False): 0, (40, 5, True): 0,
}


def _n_shifts(n_TRs):
    """Draws per test: few enough at 3 and 4 TRs that a seed exists for
    which no value of the ten pairs of five subjects exceeds 0.99."""
    return {3: 2, 4: 6}.get(n_TRs, 20)


def _data(n_TRs, n_voxels, n_subjects, seed):
    """Shared signal plus subject noise; one voxel NaN in every subject,
    one voxel NaN in a single subject."""
    rng = np.random.RandomState(seed)
    signal = rng.randn(n_TRs, n_voxels, 1)
    data = signal + 1.5 * rng.randn(n_TRs, n_voxels, n_subjects)
    data[:, NAN_VOXEL, :] = np.nan
    data[:, NAN_ONE_VOXEL, 1] = np.nan
    return data


def _max_diff(a, b):
    both = np.isfinite(a) & np.isfinite(b)
    return float(np.max(np.abs(a[both] - b[both]))) if both.any() else 0.0


@pytest.fixture
def twin_values(monkeypatch):
    """Largest |x| that reaches the twin's statistic, per call."""
    seen = []
    real = isc_mod._stat_over_rows

    def spy(x, stat):
        seen.append(float(x.nan_to_num().abs().max()))
        return real(x, stat)

    monkeypatch.setattr(isc_mod, "_stat_over_rows", spy)
    return seen


def _check_p(side, p_dev, p_np, dist_np, observed, denom):
    compared = dist_np
    if side == 'two-sided':
        compared, observed = np.abs(compared), np.abs(observed)
    with np.errstate(invalid="ignore"):
        near = np.abs(compared - observed) <= 1e-9
    print(f"side={side}: null values within 1e-9 of the observed "
          f"statistic: {int(near.sum())}")
    assert near.sum() == 0
    assert np.array_equal(np.ravel(p_dev), np.ravel(p_np), equal_nan=True)
    assert np.ravel(p_np).shape == (dist_np.shape[1],)
    assert denom == dist_np.shape[0] + 1


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("stat", STATS)
@pytest.mark.parametrize("pairwise", [False, True],
                         ids=["loo", "pairwise"])
@pytest.mark.parametrize("n_subjects", [3, 5])
@pytest.mark.parametrize("n_TRs", [3, 4, 5, 37, 40])
def test_phaseshift_matches_numpy_path(twin_values, n_TRs, n_subjects,
                                       pairwise, stat, side):
    data = _data(n_TRs, N_VOXELS, n_subjects, DATA_SEED)
    n_shifts = _n_shifts(n_TRs)
    kw = dict(pairwise=pairwise, summary_statistic=stat,
              n_shifts=n_shifts, side=side,
              random_state=SEEDS[n_TRs, n_subjects, pairwise])
    with np.errstate(all="ignore"):
        obs_np, p_np, dist_np = phaseshift_isc(data, **kw)
    assert not twin_values
    obs, p, dist = phaseshift_isc(data, device="cpu", **kw)
    assert len(twin_values) == 1
    print(f"largest |x| before the statistic: {twin_values[0]:.6f}")
    if stat == 'mean':
        assert twin_values[0] <= 0.99

    assert isinstance(dist, np.ndarray) and dist.dtype == np.float64
    assert dist.shape == dist_np.shape == (n_shifts, N_VOXELS)
    assert np.array_equal(np.isnan(dist), np.isnan(dist_np))
    assert np.isnan(dist[:, NAN_VOXEL]).all()
    # a NaN in one subject: every leave-one-out mean is NaN, while the
    # pairs without that subject survive
    assert np.isnan(dist[:, NAN_ONE_VOXEL]).all() == (not pairwise)
    finite = [v for v in range(N_VOXELS)
              if v not in (NAN_VOXEL, NAN_ONE_VOXEL)]
    assert np.isfinite(dist[:, finite]).all()
    print(f"{stat}: null max|diff|={_max_diff(dist, dist_np):.3e}")
    np.testing.assert_allclose(dist, dist_np, rtol=0, atol=1e-12)
    assert np.array_equal(obs, obs_np, equal_nan=True)
    _check_p(side, p, p_np, dist_np, obs_np, n_shifts + 1)


def test_phaseshift_takes_a_random_state_and_a_torch_device():
    data = _data(12, N_VOXELS, 4, seed=3)
    kw = dict(summary_statistic='median', n_shifts=5)
    _, _, a = phaseshift_isc(data, random_state=7, device="cpu", **kw)
    _, _, b = phaseshift_isc(data, random_state=np.random.RandomState(7),
                             device=torch.device("cpu"), **kw)
    assert np.array_equal(a, b, equal_nan=True)


# -- the tables against the definition ---------------------------------------

def _numpy_tables(data, pairwise):
    """[R, K, V] from the formula, with numpy's FFT."""
    n_TRs, _, n_subjects = data.shape
    F = (n_TRs - 1) // 2

    def spectrum(a):
        a = a - a.mean(axis=0)
        return np.fft.fft(a / np.sqrt((a * a).sum(axis=0)), axis=0)

    if pairwise:
        P = [spectrum(data[..., a]) * np.conj(spectrum(data[..., b]))
             for a, b in combinations(range(n_subjects), 2)]
    else:
        P = [spectrum(data[..., s]) * np.conj(spectrum(
            np.delete(data, s, axis=2).mean(axis=2)))
            for s in range(n_subjects)]
    P = np.stack(P)                                     # [R, T, V]
    parts = [2 / n_TRs * P.real[:, 1:F + 1],
             -2 / n_TRs * P.imag[:, 1:F + 1]]
    if n_TRs % 2 == 0:
        parts.append(P.real[:, n_TRs // 2][:, None] / n_TRs)
    return np.concatenate(parts, axis=1)


@pytest.mark.parametrize("pairwise", [False, True],
                         ids=["loo", "pairwise"])
@pytest.mark.parametrize("n_TRs", [4, 5])
def test_tables_and_coefficients_follow_the_definition(n_TRs, pairwise):
    n_subjects, seed = 4, 11
    data = _data(n_TRs, 6, n_subjects, seed=5)[:, [0, 1, 4, 5], :]
    F = (n_TRs - 1) // 2
    K = 2 * F + (1 if n_TRs % 2 == 0 else 0)
    pairs = list(combinations(range(n_subjects), 2))
    R = len(pairs) if pairwise else n_subjects

    x = torch.from_numpy(data).permute(2, 0, 1).contiguous()
    table = isc_mod._phase_tables(x, pairwise)
    assert table.shape == (R, K, 4) and table.is_contiguous()
    assert table.dtype == torch.float64
    want = _numpy_tables(data, pairwise)
    print(f"table max|diff|={np.abs(table.numpy() - want).max():.3e}")
    np.testing.assert_allclose(table.numpy(), want, rtol=0, atol=1e-14)

    # the phases that phase_randomize draws from this seed
    phases = np.random.RandomState(seed).rand(F, 1, n_subjects)[:, 0, :] \
        * 2 * np.pi
    coef = isc_mod._phase_coef(torch.from_numpy(phases[None]), pairwise,
                               n_TRs)
    assert coef.shape == (1, R, K) and coef.is_contiguous()
    ph = phases.T                                       # [S, F]
    if pairwise:
        ph = np.stack([ph[a] - ph[b] for a, b in pairs])
    want = [np.cos(ph), np.sin(ph)]
    if n_TRs % 2 == 0:
        want.append(np.ones((R, 1)))
    np.testing.assert_allclose(coef[0].numpy(), np.concatenate(want, 1),
                               rtol=0, atol=1e-15)

    # contracting them is the correlation of the surrogate
    got = torch.einsum("rk,rkv->rv", coef[0], table).numpy()
    surrogate = phase_randomize(data, random_state=seed)
    if pairwise:
        want = np.stack([array_correlation(surrogate[..., a],
                                           surrogate[..., b])
                         for a, b in pairs])
    else:
        want = np.stack([array_correlation(
            surrogate[..., s], np.delete(data, s, axis=2).mean(axis=2))
            for s in range(n_subjects)])
    print(f"single draw max|diff|={np.abs(got - want).max():.3e}")
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)


# -- chunking -----------------------------------------------------------------

# A chunk changes the shape of the matmul, and with it possibly the order
# in which a BLAS adds the K <= 37 products of magnitude <= 1: a few ulp,
# K * 1.1e-16 < 1e-14.
CHUNK_ATOL = 1e-14


@pytest.mark.parametrize("pairwise", [False, True],
                         ids=["loo", "pairwise"])
def test_voxel_chunks_share_the_draws(monkeypatch, pairwise):
    """A byte budget that forces three voxel chunks changes nothing, and
    every chunk is contracted with the same coefficient block."""
    data = _data(37, 130, 4, seed=4)
    kw = dict(pairwise=pairwise, summary_statistic='median', n_shifts=6,
              random_state=1, device="cpu")
    _, _, whole = phaseshift_isc(data, **kw)
    monkeypatch.setattr(isc_mod, "_PHASESHIFT_CHUNK_BYTES", 1)
    calls = []
    real = isc_mod._phase_stat

    def counted(table, coef, stat):
        calls.append((table.shape[2], coef))
        return real(table, coef, stat)

    monkeypatch.setattr(isc_mod, "_phase_stat", counted)
    _, _, chunked = phaseshift_isc(data, **kw)
    assert [c[0] for c in calls] == [64, 64, 2]
    assert all(c[1] is calls[0][1] for c in calls)
    assert np.array_equal(np.isnan(whole), np.isnan(chunked))
    print(f"chunked max|diff|={_max_diff(whole, chunked):.3e}")
    np.testing.assert_allclose(chunked, whole, rtol=0, atol=CHUNK_ATOL)


@pytest.mark.parametrize("stat", STATS)
def test_twin_chunks_over_draws(monkeypatch, stat):
    rng = np.random.RandomState(0)
    table = torch.from_numpy(rng.uniform(-0.1, 0.1, size=(4, 9, 10)))
    table[1, :, 3] = float("nan")
    coef = torch.from_numpy(rng.uniform(-1, 1, size=(7, 4, 9)))
    whole = isc_mod._phase_stat(table, coef, stat)
    calls = []
    real = isc_mod._stat_over_rows

    def counted(x, s):
        calls.append(x.shape[0])
        return real(x, s)

    monkeypatch.setattr(isc_mod, "_stat_over_rows", counted)
    # two draws per chunk: 4 rows x 10 voxels x 8 B x copies each
    monkeypatch.setattr(isc_mod, "_RESAMPLE_CHUNK_BYTES",
                        2 * 4 * 10 * 8 * isc_mod._RESAMPLE_CHUNK_COPIES)
    chunked = isc_mod._phase_stat(table, coef, stat)
    assert calls == [2, 2, 2, 1]
    assert torch.equal(torch.isnan(whole), torch.isnan(chunked))
    np.testing.assert_allclose(chunked.numpy(), whole.numpy(), rtol=0,
                               atol=CHUNK_ATOL)


# -- NaN policy ---------------------------------------------------------------

@pytest.mark.parametrize("stat", STATS)
def test_pairwise_threshold_drops_the_voxel(stat):
    """tolerate_nans=0.8 with 5 subjects: a voxel with two NaN subjects
    (60 % clean) is dropped - NaN in the whole column, although three of
    its pairs are finite - and one with a single NaN subject stays."""
    data = _data(37, N_VOXELS, 5, seed=6)
    data[:, 0, 3] = np.nan
    data[:, 0, 4] = np.nan
    kw = dict(pairwise=True, summary_statistic=stat, n_shifts=8,
              tolerate_nans=0.8, random_state=3)
    with np.errstate(all="ignore"):
        obs_np, p_np, dist_np = phaseshift_isc(data, **kw)
    obs, p, dist = phaseshift_isc(data, device="cpu", **kw)
    assert np.isnan(dist_np[:, 0]).all() and np.isnan(dist[:, 0]).all()
    assert np.isfinite(dist[:, NAN_ONE_VOXEL]).all()
    assert np.array_equal(np.isnan(dist), np.isnan(dist_np))
    np.testing.assert_allclose(dist, dist_np, rtol=0, atol=1e-12)
    assert np.array_equal(obs, obs_np, equal_nan=True)
    # without the threshold the three clean pairs of voxel 0 survive
    _, _, kept = phaseshift_isc(data, device="cpu",
                                **dict(kw, tolerate_nans=True))
    assert np.isfinite(kept[:, 0]).all()
    np.testing.assert_array_equal(kept[:, 1:], dist[:, 1:])


# -- _phase_stat on hand-made tables ------------------------------------------

def _stat_of_columns(columns, stat):
    """Each column as the rows of a K = 1 table under a coefficient 1."""
    table = torch.tensor(columns, dtype=torch.float64).T[:, None, :]
    coef = torch.ones((1, table.shape[0], 1), dtype=torch.float64)
    out = isc_mod._phase_stat(table.contiguous(), coef, stat)
    assert out.dtype == torch.float64 and out.shape == (1, len(columns))
    return out[0].numpy()


def test_phase_stat_semantics():
    nan = float("nan")
    med = _stat_of_columns([[0.1, 0.4, 0.2, 0.8],     # even count
                            [0.1, 0.4, 0.2, nan],     # odd count
                            [nan, nan, nan, nan],     # nothing survives
                            [0.4, nan, nan, 0.1]], 'median')
    assert med[0] == (0.2 + 0.4) / 2 and med[1] == 0.2
    assert np.isnan(med[2]) and med[3] == (0.1 + 0.4) / 2
    mean = _stat_of_columns([[1.0, nan], [-1.0, nan], [1.0, 0.5],
                             [1.0, -1.0], [nan, nan], [0.3, 0.3]], 'mean')
    # atanh(+-1) = +-inf: a lone 1 is exactly 1, +inf with -inf is NaN
    assert mean[0] == 1.0 and mean[1] == -1.0 and mean[2] == 1.0
    assert np.isnan(mean[3]) and np.isnan(mean[4])
    assert abs(mean[5] - 0.3) <= 1e-15


def test_phase_stat_contracts_over_k():
    rng = np.random.RandomState(1)
    table = rng.uniform(-0.2, 0.2, size=(3, 4, 5))
    coef = rng.uniform(-1, 1, size=(2, 3, 4))
    x = np.einsum("irk,rkv->irv", coef, table)
    for stat, want in (('median', np.median(x, axis=1)),
                       ('mean', np.tanh(np.arctanh(x).mean(axis=1)))):
        got = isc_mod._phase_stat(torch.from_numpy(table),
                                  torch.from_numpy(coef), stat).numpy()
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-15)


@pytest.mark.parametrize("bad", ["stat", "dtype", "rows", "columns",
                                 "dims", "empty"])
def test_phase_stat_rejects_bad_arguments(bad):
    table = torch.zeros((3, 4, 5), dtype=torch.float64)
    coef = torch.zeros((2, 3, 4), dtype=torch.float64)
    stat = 'median'
    if bad == "stat":
        stat = 'max'
    elif bad == "dtype":
        table = table.float()
    elif bad == "rows":
        coef = coef[:, :2]
    elif bad == "columns":
        coef = coef[:, :, :3]
    elif bad == "dims":
        coef = coef[0]
    else:
        table, coef = table[:, :0], coef[:, :, :0]
    with pytest.raises(ValueError):
        isc_mod._phase_stat(table, coef, stat)


def test_device_path_rejects_a_single_tr():
    with pytest.raises(ValueError):
        phaseshift_isc(np.ones((1, 3, 4)), n_shifts=2, device="cpu")


def test_observed_is_the_host_isc():
    data = _data(20, N_VOXELS, 4, seed=8)
    obs, _, _ = phaseshift_isc(data, summary_statistic='mean', n_shifts=2,
                               random_state=0, device="cpu")
    assert np.array_equal(obs, isc(data, summary_statistic='mean'),
                          equal_nan=True)
