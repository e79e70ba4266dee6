"""The shared-tile SVM CV kernel against the one-wave-per-QP kernel.

``ops.svm_cv(variant="shared")`` (one workgroup per voxel, the folds share
one staged K tile, pair search by DPP + ballot, pair update by readlane)
must reproduce ``variant="wave"`` exactly: the int32 ``correct`` counts
are compared for equality at the default ``max_iter`` and at
``max_iter`` in {1, 2, 7}, so the whole SMO trajectory is checked, not
only its fixed point.  A different tie-break among equal scores or a
differently rounded update changes the pair picked within the first few
iterations and with it the truncated runs' predictions.

What the two kernels share (bias rule, box slack, eta clamp, fp16 tile,
prediction chain, ``max_iter`` exit) is invisible here; both are held to
an fp64 sklearn optimum, decision value by decision value, by
``test_svm_cv_oracle.py``.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ITERS = (None, 1, 2, 7)     # None = the default max_iter


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from brainiak_amd import ops as _ops
    if _ops.load_extension() is None:
        pytest.fail("HIP extension not built — GPU box must load it")
    return _ops


class _Plan:
    """Stratified folds without sklearn: sample e of a class goes to the
    test set of fold (rank within its class) mod F; a fold trains on the
    rest, in index order."""

    def __init__(self, labels, F):
        labels = np.asarray(labels)
        E = len(labels)
        fold_of = np.zeros(E, dtype=np.int64)
        for cls in np.unique(labels):
            idx = np.nonzero(labels == cls)[0]
            fold_of[idx] = np.arange(len(idx)) % F
        tr = np.zeros((F, E), dtype=np.int32)
        te = np.zeros((F, E), dtype=np.int32)
        ntr = np.zeros(F, dtype=np.int32)
        nte = np.zeros(F, dtype=np.int32)
        for f in range(F):
            t = np.nonzero(fold_of == f)[0]
            r = np.nonzero(fold_of != f)[0]
            te[f, :len(t)] = t
            tr[f, :len(r)] = r
            nte[f], ntr[f] = len(t), len(r)
        self.F = F
        self.max_n = int(max(ntr.max(), nte.max()))
        self.n_test = nte
        self.args = (
            torch.tensor(np.where(labels == labels.max(), 1.0, -1.0)
                         .astype(np.float32)).cuda(),
            torch.tensor(tr).cuda(), torch.tensor(te).cuda(),
            torch.tensor(ntr).cuda(), torch.tensor(nte).cuda())


def _alternating(E):
    return np.arange(E) % 2


def _features_kernels(E, C, labels, seed, dim=10):
    """K = X X^T of noisy class-shifted features, as the sklearn test
    of the wave kernel builds them."""
    g = torch.Generator().manual_seed(seed)
    yy = torch.tensor(labels, dtype=torch.float32)[:, None]
    out = []
    for i in range(C):
        X = torch.randn((E, dim), generator=g) + (2.0 * i / C) * yy
        out.append(X @ X.T)
    return torch.stack(out).float().contiguous()


def _gram_kernels(E, C, labels, seed, V=512):
    """Gram-like kernels at the magnitude the pipeline hands the CV:
    Z Z^T over V z-scored columns, scaled up to a whole-brain column
    count and put through the magnitude shrink."""
    from brainiak_amd.fcma.core import _shrink_
    g = torch.Generator().manual_seed(seed)
    yy = torch.tensor(labels, dtype=torch.float32)[:, None]
    Z = torch.randn((C, E, V), generator=g) + 0.15 * yy
    G = torch.bmm(Z, Z.transpose(1, 2)) * (34470.0 / V)
    return _shrink_(G.float().contiguous())


def _run(ops, K, plan, variant, max_iter=None, tol=1e-3):
    kw = {} if max_iter is None else {"max_iter": max_iter}
    out = ops.svm_cv(K, *plan.args, C=1.0, tol=tol, max_n=plan.max_n,
                     variant=variant, **kw)
    torch.cuda.synchronize()
    return out.cpu()


def _assert_same(ops, K, plan, tol=1e-3, iters=ITERS):
    K = K.cuda().contiguous()
    for it in iters:
        wave = _run(ops, K, plan, "wave", it, tol)
        shared = _run(ops, K, plan, "shared", it, tol)
        assert wave.dtype == torch.int32 and shared.dtype == torch.int32
        assert shared.shape == (K.shape[0], plan.F)
        assert int(shared.min()) >= 0
        assert bool((shared <= torch.tensor(plan.n_test)[None, :]).all())
        diff = int((wave != shared).sum())
        assert diff == 0, (
            f"max_iter={it}: {diff} of {wave.numel()} counts differ; "
            f"first rows wave {wave[:2].tolist()} "
            f"shared {shared[:2].tolist()}")
    return shared       # the last one: max_iter = iters[-1]


# (E, F, C): the smallest instance, the headline instance with one and
# with several blocks, uneven folds with idle lanes, more folds than the
# eight waves of a block, the two-variables-per-lane fp16 tile full
# (E=128: n=96) and partly filled (E=96 F=4: n=72), and E=96 F=3, whose
# 64-sample folds are the largest the one-variable path takes.
SHAPES = [(8, 2, 5), (64, 4, 1), (64, 4, 37), (30, 4, 9), (40, 20, 6),
          (128, 4, 5), (96, 3, 5), (96, 4, 5)]


@pytest.mark.parametrize("E,F,C", SHAPES)
def test_shared_equals_wave_feature_kernels(ops, E, F, C):
    labels = _alternating(E)
    plan = _Plan(labels, F)
    _assert_same(ops, _features_kernels(E, C, labels, seed=100 + E + F),
                 plan)


@pytest.mark.parametrize("E,F,C", [(64, 4, 37), (128, 4, 5), (30, 4, 9)])
def test_shared_equals_wave_gram_scale(ops, E, F, C):
    labels = _alternating(E)
    plan = _Plan(labels, F)
    _assert_same(ops, _gram_kernels(E, C, labels, seed=200 + E), plan)


def test_shared_separable_kernels_score_high(ops):
    """Guard against the two variants agreeing on nonsense: a cleanly
    separable kernel is classified correctly in every fold."""
    E, F = 64, 4
    labels = _alternating(E)
    plan = _Plan(labels, F)
    yy = torch.tensor(labels, dtype=torch.float32)[:, None] * 2 - 1
    g = torch.Generator().manual_seed(7)
    X = 0.1 * torch.randn((3, E, 6), generator=g) + yy
    K = torch.bmm(X, X.transpose(1, 2)).float().contiguous().cuda()
    got = _run(ops, K, plan, "shared")
    assert torch.equal(got, torch.tensor(plan.n_test)[None, :]
                       .expand(3, F).to(torch.int32))


def test_shared_equals_wave_unbalanced_labels(ops):
    E, F = 64, 4
    labels = (np.arange(E) % 4 == 0).astype(np.int64)      # 3 : 1
    plan = _Plan(labels, F)
    _assert_same(ops, _features_kernels(E, 9, labels, seed=31), plan)


def _tie_kernels(E, labels):
    """Three kernels full of exact ties: identity, a constant block per
    class, and duplicated rows/columns."""
    same = torch.tensor(labels[:, None] == labels[None, :]).float()
    g = torch.Generator().manual_seed(41)
    X = torch.randn((E // 4, 5), generator=g).repeat_interleave(4, dim=0)
    X = X + torch.tensor(labels, dtype=torch.float32)[:, None]
    return torch.stack([torch.eye(E), same, X @ X.T]).float().contiguous()


@pytest.mark.parametrize("E,F", [(64, 4), (128, 4), (30, 4)])
def test_shared_equals_wave_tie_heavy(ops, E, F):
    labels = _alternating(E)
    plan = _Plan(labels, F)
    if E % 4:
        K = _tie_kernels(E + 2, _alternating(E + 2))[:, :E, :E].contiguous()
    else:
        K = _tie_kernels(E, labels)
    _assert_same(ops, K, plan)


def test_shared_equals_wave_loose_tol(ops):
    E, F = 64, 4
    labels = _alternating(E)
    plan = _Plan(labels, F)
    _assert_same(ops, _features_kernels(E, 11, labels, seed=51), plan,
                 tol=1e-2)


def test_shared_raises_where_it_does_not_fit(ops):
    E, F = 160, 2
    labels = _alternating(E)
    plan = _Plan(labels, F)
    K = _features_kernels(E, 2, labels, seed=61).cuda()
    with pytest.raises(RuntimeError, match="shared"):
        ops.svm_cv(K, *plan.args, max_n=plan.max_n, variant="shared")
    with pytest.raises(RuntimeError, match="variant"):
        ops.svm_cv(K, *plan.args, max_n=plan.max_n, variant="bogus")


def test_auto_falls_back_to_wave(ops):
    E, F = 160, 2
    labels = _alternating(E)
    plan = _Plan(labels, F)
    assert not ops._ext().svm_cv_shared_fits(E, plan.max_n)
    assert ops._ext().svm_cv_shared_fits(64, 48)
    K = _features_kernels(E, 3, labels, seed=71).cuda()
    auto = _run(ops, K, plan, "auto")
    wave = _run(ops, K, plan, "wave")
    assert torch.equal(auto, wave)
    assert int(auto.max()) > 0


def test_svm_cv_device_reads_the_environment(ops, monkeypatch):
    """BRAINIAK_SVM_CV switches the kernel under svm_cv_device; an
    explicit argument wins."""
    from types import SimpleNamespace

    from brainiak_amd.fcma.svm import svm_cv_device
    E = 160
    labels = _alternating(E)
    p = _Plan(labels, 2)
    plan = SimpleNamespace(
        y=p.args[0], train_idx=p.args[1], test_idx=p.args[2],
        n_train=p.args[3], n_test=p.args[4],
        n_test_f=p.args[4].to(torch.float32), max_n=p.max_n)
    K = _features_kernels(E, 2, labels, seed=81).cuda()
    monkeypatch.setenv("BRAINIAK_SVM_CV", "shared")
    with pytest.raises(RuntimeError, match="shared"):
        svm_cv_device(K, plan, 1.0, 1e-3)
    acc = svm_cv_device(K, plan, 1.0, 1e-3, variant="wave")
    monkeypatch.setenv("BRAINIAK_SVM_CV", "wave")
    assert torch.equal(acc, svm_cv_device(K, plan, 1.0, 1e-3))
