"""Batched path of the activity-based voxel selector on the CPU:
``ops.searchlight_gram`` (torch twin) against a brute-force loop, and
``MVPAVoxelSelector.run(clf, device="cpu")`` against the host path."""

import numpy as np
import pytest
import torch
from sklearn import svm

from brainiak_amd import ops
from brainiak_amd.fcma import mvpa_voxelselector as mvs_mod
from brainiak_amd.fcma.mvpa_voxelselector import MVPAVoxelSelector
from brainiak_amd.parallel import spawn_ranks
from brainiak_amd.searchlight import Ball, Cube, Searchlight


# ---------------------------------------------------------------------------
# ops.searchlight_gram
# ---------------------------------------------------------------------------

def _brute_force(x, mask, shape, centres):
    """Per-centre boolean gather and X^T X in fp64; also |X|^T |X| and
    the in-light voxel count, which the rounding bound needs."""
    B, X, Y, Z, E = x.shape
    rad = shape.shape[0] // 2
    xs = x.astype(np.float64)
    G = np.zeros((len(centres), E, E))
    A = np.zeros((len(centres), E, E))
    nv = np.zeros(len(centres), dtype=int)
    for n, c in enumerate(centres):
        b, i, j, k = np.unravel_index(c, (B, X, Y, Z))
        sl = np.s_[i - rad:i + rad + 1, j - rad:j + rad + 1,
                   k - rad:k + rad + 1]
        sel = mask[b][sl] & shape
        rows = xs[b][sl][sel]                    # [nv, E]
        G[n] = rows.T @ rows
        A[n] = np.abs(rows).T @ np.abs(rows)
        nv[n] = rows.shape[0]
    return G, A, nv


def _inner_centres(mask, rad):
    B, X, Y, Z = mask.shape
    inner = np.zeros_like(mask)
    inner[:, rad:X - rad, rad:Y - rad, rad:Z - rad] = True
    return np.flatnonzero(inner & mask)


def _check_gram(G, x, mask, shape, centres):
    ref, absref, nv = _brute_force(x, mask, shape, centres)
    G = G.numpy().astype(np.float64)
    bound = (nv[:, None, None] + 2) * 2.0 ** -24 * absref
    assert np.all(np.abs(G - ref) <= bound)
    assert np.array_equal(G, G.transpose(0, 2, 1))


@pytest.mark.parametrize("dims,rad,shape_cls", [
    ((6, 5, 7), 1, Cube),
    ((7, 7, 8), 2, Ball),
])
def test_twin_matches_brute_force(dims, rad, shape_cls):
    rng = np.random.RandomState(3)
    B, E = 2, 5
    x = rng.randn(B, *dims, E).astype(np.float32)
    mask = rng.rand(B, *dims) < 0.6
    shape = shape_cls(rad).mask_
    # one centre whose ball holds only itself
    lone = (1, rad, rad, rad)
    mask[1, :2 * rad + 1, :2 * rad + 1, :2 * rad + 1] = False
    mask[lone] = True
    centres = _inner_centres(mask, rad)
    lone_idx = np.ravel_multi_index(lone, mask.shape)
    assert lone_idx in centres
    G = ops.searchlight_gram(torch.as_tensor(x), torch.as_tensor(mask),
                             torch.as_tensor(shape),
                             torch.as_tensor(centres))
    assert G.dtype == torch.float32 and G.shape == (len(centres), E, E)
    _check_gram(G, x, mask, shape, centres)
    n = int(np.flatnonzero(centres == lone_idx)[0])
    v = x[lone].astype(np.float64)
    assert np.allclose(G[n].numpy(), np.outer(v, v), rtol=1e-6, atol=0)


def test_twin_chunks_over_centres(monkeypatch):
    rng = np.random.RandomState(4)
    x = rng.randn(1, 5, 5, 5, 3).astype(np.float32)
    mask = rng.rand(1, 5, 5, 5) < 0.6
    shape = Cube(1).mask_
    centres = _inner_centres(mask, 1)
    args = (torch.as_tensor(x), torch.as_tensor(mask),
            torch.as_tensor(shape), torch.as_tensor(centres))
    whole = ops.searchlight_gram(*args)
    monkeypatch.setattr(ops, "_SL_GRAM_TWIN_BYTES", 1)
    assert torch.equal(ops.searchlight_gram(*args), whole)


def _small_case():
    x = torch.zeros((2, 4, 5, 6, 3))
    mask = torch.ones((2, 4, 5, 6), dtype=torch.bool)
    shape = torch.ones((3, 3, 3), dtype=torch.bool)
    return x, mask, shape


def _lin(b, i, j, k):
    return ((b * 4 + i) * 5 + j) * 6 + k


@pytest.mark.parametrize("centre", [
    _lin(0, 0, 2, 2), _lin(0, 3, 2, 2), _lin(1, 1, 0, 2), _lin(1, 1, 4, 2),
    _lin(0, 1, 2, 0), _lin(1, 2, 2, 5),       # on a block face
    -1, 2 * 4 * 5 * 6,                        # out of range
])
def test_gram_rejects_bad_centre(centre):
    x, mask, shape = _small_case()
    with pytest.raises(ValueError):
        ops.searchlight_gram(x, mask, shape, torch.tensor([_lin(0, 1, 1, 1),
                                                           centre]))


@pytest.mark.parametrize("shape_dims", [(3, 3, 5), (2, 2, 2), (11, 11, 11)])
def test_gram_rejects_bad_shape(shape_dims):
    x = torch.zeros((1, 12, 12, 12, 2))
    mask = torch.ones((1, 12, 12, 12), dtype=torch.bool)
    with pytest.raises(ValueError):
        ops.searchlight_gram(x, mask,
                             torch.ones(shape_dims, dtype=torch.bool),
                             torch.tensor([(5 * 12 + 5) * 12 + 5]))


def test_gram_no_centres():
    x, mask, shape = _small_case()
    G = ops.searchlight_gram(x, mask, shape,
                             torch.empty(0, dtype=torch.int64))
    assert G.shape == (0, 3, 3) and G.dtype == torch.float32


# ---------------------------------------------------------------------------
# MVPAVoxelSelector.run(clf, device="cpu")
# ---------------------------------------------------------------------------

CONFIGS = [
    # dims, rad, shape, E, seed
    ((7, 7, 7), 1, Cube, 16, 0),
    ((8, 7, 9), 2, Ball, 12, 1),
    ((7, 7, 7), 1, Cube, 24, 2),
]


def _selector(dims, rad, shape_cls, E, seed, proportion=0, comm=None,
              rank0_only=False):
    rng = np.random.RandomState(seed)
    mask = rng.rand(*dims) < 0.7
    labels = np.array([e % 2 for e in range(E)])
    data = rng.randn(*dims, E).astype(np.float32)
    data[3, 3, 3, :] += 3.0 * labels
    data[3, 3, 2, :] += 3.0 * labels
    sl = Searchlight(sl_rad=rad, max_blk_edge=4, shape=shape_cls,
                     min_active_voxels_proportion=proportion, comm=comm,
                     pool_size=1)
    if rank0_only and sl.comm.rank != 0:
        data = None
    return MVPAVoxelSelector(data, mask, labels, num_folds=4, sl=sl)


def _linear_svc():
    return svm.SVC(kernel='linear', shrinking=False, C=1)


def _is_none(volume):
    return np.array([v is None for v in volume.ravel()]).reshape(
        volume.shape)


def _assert_same(got, want):
    vol_g, ranked_g = got
    vol_w, ranked_w = want
    assert vol_g.shape == vol_w.shape and vol_g.dtype == object
    none_g = _is_none(vol_g)
    none_w = _is_none(vol_w)
    assert np.array_equal(none_g, none_w)
    assert np.array_equal(vol_g[~none_g].astype(float),
                          vol_w[~none_w].astype(float))
    assert ranked_g == ranked_w


@pytest.mark.parametrize("dims,rad,shape_cls,E,seed", CONFIGS)
def test_run_cpu_device_equals_host_path(dims, rad, shape_cls, E, seed):
    want = _selector(dims, rad, shape_cls, E, seed).run(_linear_svc())
    got = _selector(dims, rad, shape_cls, E, seed).run(_linear_svc(),
                                                       device="cpu")
    assert any(acc is not None for acc in want[0].ravel())
    _assert_same(got, want)


@pytest.mark.parametrize("proportion", [0.5, 0.7])
def test_run_cpu_device_min_active_proportion(proportion):
    dims, rad, shape_cls, E, seed = CONFIGS[0]
    want = _selector(dims, rad, shape_cls, E, seed, proportion).run(
        _linear_svc())
    got = _selector(dims, rad, shape_cls, E, seed, proportion).run(
        _linear_svc(), device=torch.device("cpu"))
    none_want = _is_none(want[0])
    if proportion == 0.7:
        # 19 of 27 voxels of a 70 % mask: the threshold drops centres
        free = _selector(dims, rad, shape_cls, E, seed).run(_linear_svc())
        assert none_want.sum() > _is_none(free[0]).sum()
    assert np.array_equal(_is_none(got[0]), none_want)
    _assert_same(got, want)


def test_gram_chunking_leaves_result_unchanged(monkeypatch):
    dims, rad, shape_cls, E, seed = CONFIGS[0]
    whole = _selector(dims, rad, shape_cls, E, seed).run(_linear_svc(),
                                                         device="cpu")
    monkeypatch.setattr(mvs_mod, "_GRAM_CHUNK_BYTES", E * E * 4)
    calls = []
    real = ops.searchlight_gram

    def counted(x, mask, shape, centres):
        calls.append(int(centres.shape[0]))
        return real(x, mask, shape, centres)

    monkeypatch.setattr(ops, "searchlight_gram", counted)
    chunked = _selector(dims, rad, shape_cls, E, seed).run(_linear_svc(),
                                                           device="cpu")
    assert calls and max(calls) == 1
    _assert_same(chunked, whole)


@pytest.mark.parametrize("make_clf", [
    lambda: svm.SVC(kernel='rbf', C=10, gamma='auto'),
    lambda: svm.SVC(kernel='precomputed'),
    lambda: svm.SVC(kernel='linear', class_weight='balanced'),
], ids=["rbf", "precomputed", "balanced"])
def test_device_path_rejects_other_classifiers(make_clf):
    dims, rad, shape_cls, E, seed = CONFIGS[0]
    with pytest.raises(ValueError, match="device=None"):
        _selector(dims, rad, shape_cls, E, seed).run(make_clf(),
                                                     device="cpu")


@pytest.mark.parametrize("make_clf", [
    lambda: svm.SVC(kernel='rbf', C=10, gamma='auto'),
    lambda: svm.SVC(kernel='linear', class_weight='balanced'),
], ids=["rbf", "balanced"])
def test_host_path_still_runs_other_classifiers(make_clf):
    mvs = _selector((5, 5, 5), 1, Cube, 12, 0)
    volume, ranked = mvs.run(make_clf())
    assert len(ranked) == int(mvs.mask.sum())
    assert all(0.0 <= acc <= 1.0 for _, acc in ranked)


def test_host_path_still_runs_precomputed_classifier():
    # a 'precomputed' SVC needs square inputs: the host path hands the
    # classifier to sklearn as it is, so the failure is sklearn's own
    mvs = _selector((5, 5, 5), 1, Cube, 12, 0)
    with pytest.raises(ValueError) as err:
        mvs.run(svm.SVC(kernel='precomputed'))
    assert "device=None" not in str(err.value)


def test_three_classes():
    dims, rad, shape_cls, E, seed = (5, 5, 5), 1, Cube, 12, 0
    mvs = _selector(dims, rad, shape_cls, E, seed)
    mvs.labels = np.array([e % 3 for e in range(E)])
    with pytest.raises(ValueError, match="device=None"):
        mvs.run(_linear_svc(), device="cpu")
    volume, ranked = mvs.run(_linear_svc())
    assert len(ranked) == int(mvs.mask.sum())


def _two_rank_run(ctx, outfile):
    dims, rad, shape_cls, E, seed = CONFIGS[1]
    mvs = _selector(dims, rad, shape_cls, E, seed, comm=ctx,
                    rank0_only=True)
    volume, ranked = mvs.run(_linear_svc(), device="cpu")
    if ctx.rank == 0:
        np.save(outfile, volume.astype(float))
        np.save(outfile + ".ranked.npy", np.asarray(ranked))


def test_two_ranks_equal_serial(tmp_path):
    out = str(tmp_path / "vol.npy")
    spawn_ranks(_two_rank_run, world_size=2, args=(out,))
    dims, rad, shape_cls, E, seed = CONFIGS[1]
    volume, ranked = _selector(dims, rad, shape_cls, E, seed).run(
        _linear_svc(), device="cpu")
    assert np.array_equal(np.load(out), volume.astype(float),
                          equal_nan=True)
    assert np.array_equal(np.load(out + ".ranked.npy"), np.asarray(ranked))
