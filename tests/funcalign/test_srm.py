import numpy as np
import pytest

from brainiak_amd.funcalign import srm as srm_mod
from brainiak_amd.funcalign.srm import SRM, DetSRM, load


def _synthetic_subjects(rng, subjects=4, voxels=60, samples=40, features=5,
                        noise=0.1):
    """Shared low-rank latent + per-subject orthogonal mixing + noise."""
    S = rng.randn(features, samples)
    data, W = [], []
    for _ in range(subjects):
        q, _ = np.linalg.qr(rng.randn(voxels, features))
        W.append(q)
        data.append(q @ S + noise * rng.randn(voxels, samples))
    return data, W, S


def test_detsrm_fit_recovers_shared_space(seeded_rng):
    data, _, S = _synthetic_subjects(seeded_rng)
    model = DetSRM(n_iter=15, features=5, rand_seed=0, device="cpu")
    model.fit(data)
    assert len(model.w_) == 4
    for w in model.w_:
        assert w.shape == (60, 5)
        # orthogonality
        assert np.allclose(w.T @ w, np.eye(5), atol=1e-8)
    assert model.s_.shape == (5, 40)
    # transformed data should correlate across subjects much more than raw
    projected = model.transform(data)
    c = np.corrcoef(projected[0].ravel(), projected[1].ravel())[0, 1]
    assert abs(c) > 0.9


def test_detsrm_objective_decreases(seeded_rng):
    data, _, _ = _synthetic_subjects(seeded_rng)
    m2 = DetSRM(n_iter=2, features=5, rand_seed=0, device="cpu").fit(data)
    m10 = DetSRM(n_iter=12, features=5, rand_seed=0, device="cpu").fit(data)
    obj2 = m2._objective_function(data, m2.w_, m2.s_)
    obj10 = m10._objective_function(data, m10.w_, m10.s_)
    assert obj10 <= obj2 + 1e-9


def test_srm_fit_basic(seeded_rng):
    data, _, _ = _synthetic_subjects(seeded_rng, subjects=3)
    model = SRM(n_iter=8, features=5, rand_seed=0, device="cpu")
    model.fit(data)
    assert model.s_.shape == (5, 40)
    assert model.sigma_s_.shape == (5, 5)
    assert model.rho2_.shape == (3,)
    assert np.all(model.rho2_ > 0)
    for w, mu in zip(model.w_, model.mu_):
        assert w.shape == (60, 5)
        assert np.allclose(w.T @ w, np.eye(5), atol=1e-8)
        assert mu.shape == (60,)
    # eigenvalues of sigma_s positive
    assert np.all(np.linalg.eigvalsh(model.sigma_s_) > -1e-10)


def test_srm_errors(seeded_rng):
    data, _, _ = _synthetic_subjects(seeded_rng, subjects=2, samples=40)
    with pytest.raises(ValueError):
        SRM(device="cpu").fit([data[0]])  # too few subjects
    with pytest.raises(ValueError):
        SRM(features=50, device="cpu").fit(data)  # samples < features
    bad = [data[0], data[1][:, :30]]
    with pytest.raises(ValueError):
        SRM(features=5, device="cpu").fit(bad)  # unequal samples
    nan_data = [d.copy() for d in data]
    nan_data[0][0, 0] = np.nan
    with pytest.raises(ValueError):
        SRM(features=5, device="cpu").fit(nan_data)
    with pytest.raises(srm_mod.NotFittedError):
        SRM(device="cpu").transform(data)


def test_srm_transform_and_new_subject(seeded_rng):
    data, _, _ = _synthetic_subjects(seeded_rng, subjects=4)
    model = SRM(n_iter=8, features=5, rand_seed=0, device="cpu").fit(data[:3])
    with pytest.raises(ValueError):
        model.transform(data)  # 4 subjects vs model's 3
    proj = model.transform(data[:3])
    assert proj[0].shape == (5, 40)
    w_new = model.transform_subject(data[3])
    assert w_new.shape == (60, 5)
    assert np.allclose(w_new.T @ w_new, np.eye(5), atol=1e-6)
    with pytest.raises(ValueError):
        model.transform_subject(data[3][:, :20])


def test_srm_save_load_roundtrip(tmp_path, seeded_rng):
    data, _, _ = _synthetic_subjects(seeded_rng, subjects=3)
    model = SRM(n_iter=5, features=5, rand_seed=3, device="cpu").fit(data)
    f = tmp_path / "model.npz"
    model.save(f)
    loaded = load(f)
    assert loaded.features == 5 and loaded.n_iter == 5
    assert np.allclose(loaded.s_, model.s_)
    assert np.allclose(loaded.sigma_s_, model.sigma_s_)
    for a, b in zip(loaded.w_, model.w_):
        assert np.allclose(a, b)


def test_srm_seed_determinism(seeded_rng):
    data, _, _ = _synthetic_subjects(seeded_rng, subjects=3)
    m1 = SRM(n_iter=4, features=5, rand_seed=7, device="cpu").fit(data)
    m2 = SRM(n_iter=4, features=5, rand_seed=7, device="cpu").fit(data)
    assert np.allclose(m1.s_, m2.s_)
    m3 = SRM(n_iter=4, features=5, rand_seed=8, device="cpu").fit(data)
    assert not np.allclose(m1.w_[0], m3.w_[0])


def test_polar_orthogonal_matches_svd(seeded_rng):
    import torch
    A = torch.tensor(seeded_rng.randn(30, 5))
    W = srm_mod._polar_orthogonal(A, perturb=0.0).numpy()
    U, _, Vt = np.linalg.svd(A.numpy(), full_matrices=False)
    assert np.allclose(W, U @ Vt, atol=1e-10)


@pytest.mark.gpu
def test_detsrm_gpu(seeded_rng, gpu_device):
    data, _, _ = _synthetic_subjects(seeded_rng)
    model = DetSRM(n_iter=10, features=5, rand_seed=0,
                   device="cuda").fit(data)
    for w in model.w_:
        assert np.allclose(w.T @ w, np.eye(5), atol=1e-4)
    projected = model.transform(data)
    c = np.corrcoef(projected[0].ravel(), projected[1].ravel())[0, 1]
    assert abs(c) > 0.9


def test_srm_loads_frozen_v0_1_model():
    """Backward-compat: the npz schema written by v0.1 keeps loading
    (the reference's sr_v0_4.npz compat test, ref
    tests/funcalign/test_srm.py)."""
    from pathlib import Path
    path = Path(__file__).parent / "data" / "srm_v0_1.npz"
    from brainiak_amd.funcalign.srm import load
    m = load(str(path))
    assert m.s_.shape == (5, 30)
    assert len(m.w_) == 3 and m.w_[0].shape == (40, 5)
    # transform with the loaded bases works
    rng = np.random.RandomState(7)
    S = rng.randn(5, 30)
    q, _ = np.linalg.qr(rng.randn(40, 5))
    x = q @ S
    proj = m.transform([x, None, None])
    assert proj[0].shape == (5, 30)


# -- round-2 depth (ref tests/funcalign/test_srm.py:1-319) -------------------

def test_srm_batched_polar_many_matches_loop(seeded_rng):
    """The ragged-batch Procrustes helper equals per-matrix polar
    factors."""
    import torch

    from brainiak_amd.funcalign.srm import (
        _polar_orthogonal,
        _polar_orthogonal_many,
    )
    mats = [torch.tensor(seeded_rng.randn(v, 5)) for v in (30, 17, 44)]
    batched = _polar_orthogonal_many([m.clone() for m in mats],
                                     perturb=0.001)
    for m, w in zip(mats, batched):
        ref = _polar_orthogonal(m.clone(), perturb=0.001)
        assert torch.allclose(w, ref, atol=1e-8)
        # orthonormal columns
        assert torch.allclose(w.T @ w, torch.eye(5, dtype=w.dtype),
                              atol=1e-8)


def test_srm_w_orthogonality_and_shapes(seeded_rng):
    from brainiak_amd.funcalign.srm import SRM
    data = [seeded_rng.randn(30 + 5 * i, 40) for i in range(3)]
    m = SRM(n_iter=6, features=4, rand_seed=0, device="cpu")
    m.fit(data)
    assert m.s_.shape == (4, 40)
    for i, w in enumerate(m.w_):
        assert w.shape == (30 + 5 * i, 4)
        assert np.allclose(w.T @ w, np.eye(4), atol=1e-8)
    assert m.sigma_s_.shape == (4, 4)
    # sigma_s symmetric positive semi-definite
    assert np.allclose(m.sigma_s_, m.sigma_s_.T)
    assert np.all(np.linalg.eigvalsh(m.sigma_s_) > -1e-10)
    assert m.rho2_.shape == (3,)
    assert np.all(m.rho2_ > 0)


def test_srm_transform_errors(seeded_rng):
    from brainiak_amd.funcalign.srm import SRM, NotFittedError
    data = [seeded_rng.randn(20, 30) for _ in range(3)]
    m = SRM(n_iter=4, features=3, rand_seed=0)
    with pytest.raises(NotFittedError):
        m.transform(data)
    m.fit(data)
    with pytest.raises(ValueError):
        m.transform(data[:2])     # subject count mismatch
    with pytest.raises(ValueError):
        m.transform_subject(seeded_rng.randn(20, 25))  # TR mismatch


def test_detsrm_matches_reference_complexity_contract(seeded_rng):
    """DetSRM with orthonormal planted W and noiseless data recovers
    X_i = W_i S exactly-ish."""
    from brainiak_amd.funcalign.srm import DetSRM
    k, t = 3, 40
    S = seeded_rng.randn(k, t)
    data, ws = [], []
    for _ in range(3):
        w = np.linalg.qr(seeded_rng.randn(25, k))[0]
        ws.append(w)
        data.append(w @ S)
    m = DetSRM(n_iter=30, features=k, rand_seed=0)
    m.fit(data)
    for i in range(3):
        recon = m.w_[i] @ m.s_
        assert np.allclose(recon, data[i], atol=1e-3)


def test_srm_features_exceed_samples_error(seeded_rng):
    from brainiak_amd.funcalign.srm import SRM
    data = [seeded_rng.randn(30, 5) for _ in range(2)]   # 5 TRs < 10
    with pytest.raises(ValueError):
        SRM(n_iter=3, features=10).fit(data)


def test_rsrm_outliers_land_in_s(seeded_rng):
    """RSRM: spike outliers are absorbed by the sparse S_i term, not
    the shared response (the model's defining property)."""
    from brainiak_amd.funcalign.rsrm import RSRM
    k, t, v = 3, 50, 40
    R = seeded_rng.randn(k, t)
    data = []
    for _ in range(3):
        w = np.linalg.qr(seeded_rng.randn(v, k))[0]
        x = w @ R + 0.01 * seeded_rng.randn(v, t)
        data.append(x)
    # subject 0 gets heavy sparse corruption
    data[0][5, ::7] += 20.0
    m = RSRM(n_iter=12, features=k, gamma=1.0, rand_seed=0)
    m.fit(data)
    # the outlier entries appear in s_[0]
    assert np.abs(m.s_[0][5, ::7]).mean() > 1.0
    # other entries stay mostly sparse-zero
    mask = np.ones_like(m.s_[0], dtype=bool)
    mask[5, ::7] = False
    assert np.abs(m.s_[0][mask]).mean() < 0.5
