"""The SVM CV kernels against an fp64 dual-optimum oracle.

``ops.svm_cv_trace`` returns, next to the int32 ``correct`` counts of
``ops.svm_cv``, the decision value of every test sample and the number of
SMO iterations each (voxel, fold) QP ran.  Both kernels (``"wave"`` and
``"shared"``) are held here to three independent references:

* ``d*``: ``sklearn.svm.SVC(kernel='precomputed', tol=1e-8,
  shrinking=False)`` trained in fp64 on each fold's training block, its
  ``decision_function`` on the test rows (``y=+1`` is ``classes[1]``, as
  in ``FoldPlan``).  When the plan's largest fold (train or test) is over
  64 samples the kernels keep Q in an fp16 tile and predict with the fp32
  rows (header of ``svm_kernels.hip``); the oracle of such a case trains
  on the training block rounded to fp16 and predicts with the unrounded
  rows.  The two magnitude families (``big``, ``small``) leave the range
  in which that contract can be stated with a plain fp16 cast, so their
  oracle trains on the unrounded block.
* the fp32 twin: ``fcma.svm.smo_batch_train`` on the CPU with the
  kernel's ``C``, ``tol`` and ``max_iter`` on the same (rounded) block:
  the same algorithm and stopping rule in independent code.  It gives the
  distance ``dev = max |d_twin - d*|`` that two solutions stopped at
  ``gap < tol`` can have, and it says which QPs converge at all.
* ``ops.svm_cv`` itself, whose counts must equal the trace form's.

A family's bound on ``|dec - d*|`` is ``4 * dev`` rounded up to two
significant digits: a factor 2 for the kernel stopping on the other side
of the optimum, another 2 for its different tie-break and rounding
order.  ``dev`` is measured on the references alone, never on the kernel;
for the magnitude families it is the twin's distance from ``d*`` on the
unrounded block plus the twin's own shift when the block is rescaled by a
power of two into the fp16 range, rounded and scaled back.  Each bound
below carries the ``dev`` it came from; ``test_bound_not_stale`` recomputes
``dev`` and fails when it exceeds half the bound.  The table is printed by

    PYTHONPATH=. python tests/ops/test_svm_cv_oracle.py [-v] [family ...]

from the repository root.  The rank-10 family at C = 1 is split by tile
type (``feat10``: every fold up to 64, fp32 tile; ``feat10_h``: fp16 tile),
because the rounded training block doubles ``dev``.
"""

import functools
import math
import sys
from collections import namedtuple

import numpy as np
import pytest
import torch

MAX_ITER = 10000            # the default of ops.svm_cv

# recipe: the kernels' construction, times scale; sep: class shift of the
# first voxel's features (later voxels are shifted further); seed; C; tol;
# bound on |dec - d*|.  Each bound is 4 * dev rounded up to two significant
# digits, dev as printed by the command above (CPU only: the fp32 twin
# against the fp64 oracle).
Family = namedtuple("Family", "recipe scale sep seed C tol bound")
FAMILIES = {
    # X X^T of 10-d features, folds up to 64 (fp32 tile)   dev 0.00624
    "feat10": Family("feat10", 1.0, 0.0, 0, 1.0, 1e-3, 0.025),
    # the same, plans with a fold over 64 (fp16 tile)      dev 0.0138
    "feat10_h": Family("feat10", 1.0, 0.0, 0, 1.0, 1e-3, 0.056),
    # X X^T of 40-d features                               dev 0.00701
    "feat40": Family("feat40", 1.0, 0.0, 0, 1.0, 1e-3, 0.029),
    # shrunk Gram-like kernels at pipeline magnitude       dev 0.000398
    "gram": Family("gram", 1.0, 0.0, 0, 1.0, 1e-3, 0.0016),
    # (class shift 1: without one, some QPs of the fp32 twin are not at
    # the gap after MAX_ITER iterations at C = 10)         dev 0.0172
    "feat10_C10": Family("feat10", 1.0, 1.0, 1, 10.0, 1e-3, 0.069),
    #                                                      dev 0.00567
    "feat10_C01": Family("feat10", 1.0, 0.0, 0, 0.1, 1e-3, 0.023),
    #                                                      dev 0.124
    "feat40_tol2": Family("feat40", 1.0, 0.0, 0, 1.0, 1e-2, 0.5),
    #                                                      dev 0.00479
    "gram_tol2": Family("gram", 1.0, 0.0, 0, 1.0, 1e-2, 0.02),
    # feature kernels with diagonals of 2e5 to 2e6, past the fp16 maximum,
    # classes shifted apart by 3.  (Without the shift the classes overlap,
    # and at C = 1 a kernel of this size is all but a hard-margin problem
    # on data no hyperplane separates: the fp32 twin is still at a gap of
    # several units after MAX_ITER iterations, so there is no bound to
    # measure.)                                            dev 0.00455
    "big": Family("feat10", 2.0e4, 3.0, 0, 1.0, 1e-3, 0.019),
    # feature kernels times 1e-4: entries in the fp16 subnormal range
    #                                                      dev 4.56e-06
    "small": Family("feat10", 1.0e-4, 0.0, 0, 1.0, 1e-3, 1.9e-5),
}
MAGNITUDE = ("big", "small")


# ---------------------------------------------------------------------------
# fold plans
# ---------------------------------------------------------------------------

class Plan:
    """Index tables in the layout ``ops.svm_cv`` takes, from explicit
    (train, test) index lists per fold."""

    def __init__(self, labels, folds):
        labels = np.asarray(labels)
        E, F = len(labels), len(folds)
        self.E, self.F = E, F
        self.y = np.where(labels == labels.max(), 1.0, -1.0).astype(
            np.float32)
        self.train_idx = np.zeros((F, E), dtype=np.int32)
        self.test_idx = np.zeros((F, E), dtype=np.int32)
        self.n_train = np.zeros(F, dtype=np.int32)
        self.n_test = np.zeros(F, dtype=np.int32)
        for f, (tr, te) in enumerate(folds):
            assert len(set(self.y[tr])) == 2, "one-class training fold"
            self.train_idx[f, :len(tr)] = tr
            self.test_idx[f, :len(te)] = te
            self.n_train[f], self.n_test[f] = len(tr), len(te)
        self.max_n = int(max(self.n_train.max(), self.n_test.max()))
        # the kernels switch to the fp16 tile by the plan's largest fold
        self.fp16 = self.max_n > 64

    def folds(self):
        for f in range(self.F):
            yield (f, self.train_idx[f, :self.n_train[f]],
                   self.test_idx[f, :self.n_test[f]])


def _alternating(E):
    return np.arange(E) % 2


def _stratified(labels, F, descending=False):
    """Sample e of a class tests in fold (rank within its class) mod F and
    trains in the others, in index order (or in descending order)."""
    labels = np.asarray(labels)
    fold_of = np.zeros(len(labels), dtype=np.int64)
    for cls in np.unique(labels):
        idx = np.nonzero(labels == cls)[0]
        fold_of[idx] = np.arange(len(idx)) % F
    folds = []
    for f in range(F):
        tr = np.nonzero(fold_of != f)[0]
        folds.append((tr[::-1] if descending else tr,
                      np.nonzero(fold_of == f)[0]))
    return Plan(labels, folds)


def _contiguous(labels, F):
    """Hand-built: fold f tests the f-th contiguous run of each class."""
    labels = np.asarray(labels)
    E = len(labels)
    fold_of = np.zeros(E, dtype=np.int64)
    for cls in np.unique(labels):
        idx = np.nonzero(labels == cls)[0]
        fold_of[idx] = (np.arange(len(idx)) * F) // len(idx)
    return Plan(labels, [(np.nonzero(fold_of != f)[0],
                          np.nonzero(fold_of == f)[0]) for f in range(F)])


def _small_train(labels, n_train, F, seed):
    """Hand-built: each fold trains on n_train samples (half per class) and
    tests on all the others."""
    labels = np.asarray(labels)
    rng = np.random.RandomState(seed)
    folds = []
    for _ in range(F):
        tr = np.concatenate([
            rng.permutation(np.nonzero(labels == cls)[0])[:n_train // 2]
            for cls in np.unique(labels)])
        tr = np.sort(tr)
        folds.append((tr, np.setdiff1d(np.arange(len(labels)), tr)))
    return Plan(labels, folds)


# name -> (labels, plan, the shared kernel covers the shape)
def _shape(name):
    alt = _alternating
    table = {
        # n_train = 2, and the smallest instance of the equality tests
        "e4f2": lambda: (alt(4), 2, True),
        "e8f2": lambda: (alt(8), 2, True),
        # idle lanes; E=31 puts odd voxels off 16-byte alignment, so the
        # shared kernel's scalar staging loop and its EE % 4 tail run
        "e30f4": lambda: (alt(30), 4, True),
        "e31f4": lambda: (alt(31), 4, True),
        "e64f4": lambda: (alt(64), 4, True),          # the headline instance
        "e96f3": lambda: (alt(96), 3, True),          # n = 64, last fp32 fold
        "e98f3": lambda: (alt(98), 3, True),          # n = 66, first fp16 fold
        "e127f4": lambda: (alt(127), 4, True),        # n = 95, 96
        "e128f4": lambda: (alt(128), 4, True),        # n = 96
        "e128f16": lambda: (alt(128), 16, True),      # n = 120, F > 8 waves
        "e170f4": lambda: (alt(170), 4, False),       # n = 128, wave only
        # n_train = n_test = 65: the prediction loop's second pass
        "e130f2": lambda: (alt(130), 2, False),
    }
    if name in table:
        labels, F, shared = table[name]()
        return labels, _stratified(labels, F), shared
    if name == "e128_tr40":     # fp16 tile with n < 64 and m = 88 > 64
        labels = alt(128)
        return labels, _small_train(labels, 40, 2, seed=5), True
    if name == "e64_desc":      # training indices in descending order
        labels = alt(64)
        return labels, _stratified(labels, 4, descending=True), True
    if name == "e64_3to1":      # labels 3:1 unbalanced
        labels = (np.arange(64) % 4 == 0).astype(np.int64)
        return labels, _stratified(labels, 4), True
    if name == "e64_blocked":   # first half one class
        labels = (np.arange(64) >= 32).astype(np.int64)
        return labels, _contiguous(labels, 4), True
    raise KeyError(name)


# ---------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------

def _feature_kernels(E, C, labels, seed, dim, sep=0.0):
    """K = X X^T of noisy class-shifted features, the recipe of
    test_svm_cv_shared.py; the shift grows with the voxel index."""
    g = torch.Generator().manual_seed(seed)
    yy = torch.tensor(labels, dtype=torch.float32)[:, None]
    out = []
    for i in range(C):
        X = torch.randn((E, dim), generator=g) + (sep + 2.0 * i / C) * yy
        out.append(X @ X.T)
    return torch.stack(out).float().contiguous()


def _gram_kernels(E, C, labels, seed, V=512):
    """Gram-like kernels at the magnitude the pipeline hands the CV, the
    recipe of test_svm_cv_shared.py."""
    from brainiak_amd.fcma.core import _shrink_
    g = torch.Generator().manual_seed(seed)
    yy = torch.tensor(labels, dtype=torch.float32)[:, None]
    Z = torch.randn((C, E, V), generator=g) + 0.15 * yy
    G = torch.bmm(Z, Z.transpose(1, 2)) * (34470.0 / V)
    return _shrink_(G.float().contiguous())


CASES = (
    [("feat10", s) for s in ("e4f2", "e8f2", "e30f4", "e31f4", "e64f4",
                             "e96f3", "e64_desc", "e64_3to1", "e64_blocked")]
    + [("feat10_h", s) for s in ("e98f3", "e127f4", "e128f4", "e128f16",
                                 "e170f4", "e130f2", "e128_tr40")]
    + [("feat40", s) for s in ("e31f4", "e64f4", "e128f4")]
    + [("gram", s) for s in ("e30f4", "e64f4", "e98f3", "e128f4")]
    + [(fam, s) for fam in ("feat10_C10", "feat10_C01", "feat40_tol2",
                            "gram_tol2")
       for s in ("e64f4", "e128f4")]
    + [(fam, s) for fam in MAGNITUDE
       for s in ("e64f4", "e128f4", "e170f4")])
N_VOXELS = 4


def _round_fp16(K):
    return K.astype(np.float16).astype(np.float64)


def _round_fp16_scaled(K):
    """K [E, E] rounded to 11 bits after an exact power-of-two rescaling
    that puts its largest magnitude into [2^14, 2^15), and scaled back."""
    qe = int(np.frexp(np.abs(K).max())[1]) - 1 - 14
    return np.ldexp(_round_fp16(np.ldexp(K, -qe)), qe)


# ---------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------

def _oracle(K64, Ktrain64, plan, C):
    """d* [C, F, E]: sklearn's fp64 optimum trained on Ktrain64's training
    blocks, predicting with K64's rows."""
    from sklearn.svm import SVC
    d = np.zeros((K64.shape[0], plan.F, plan.E))
    for c in range(K64.shape[0]):
        for f, tr, te in plan.folds():
            clf = SVC(kernel="precomputed", C=C, tol=1e-8, shrinking=False)
            clf.fit(Ktrain64[c][np.ix_(tr, tr)], plan.y[tr])
            assert clf.classes_[1] == 1.0
            d[c, f, :len(te)] = clf.decision_function(
                K64[c][np.ix_(te, tr)])
    return d


def _twin(K64, Ktrain64, plan, C, tol, dtype=torch.float32, max_iter=MAX_ITER):
    """smo_batch_train on the CPU: (d_twin [C, F, E], converged [C, F]).
    Folds of equal size go through one batch.  ``converged`` is the gap
    test recomputed in fp64 from the returned alpha."""
    from brainiak_amd.fcma.svm import smo_batch_train
    nv = K64.shape[0]
    d = np.zeros((nv, plan.F, plan.E))
    conv = np.zeros((nv, plan.F), dtype=bool)
    for n in np.unique(plan.n_train):
        fs = [f for f in range(plan.F) if plan.n_train[f] == n]
        trs = [plan.train_idx[f, :n] for f in fs]
        Kb = np.stack([Ktrain64[c][np.ix_(tr, tr)]
                       for tr in trs for c in range(nv)])
        yb = np.stack([plan.y[tr] for tr in trs for c in range(nv)])
        alpha, b = smo_batch_train(
            torch.as_tensor(Kb, dtype=dtype), torch.as_tensor(yb, dtype=dtype),
            C=C, tol=tol, max_iter=max_iter)
        alpha = alpha.double().numpy()
        b = b.double().numpy()
        yb = yb.astype(np.float64)
        score = -yb * (np.einsum("bij,bj->bi", Kb * yb[:, :, None]
                                 * yb[:, None, :], alpha) - 1.0)
        up = ((yb > 0) & (alpha < C - 1e-12)) | ((yb < 0) & (alpha > 1e-12))
        lo = ((yb > 0) & (alpha > 1e-12)) | ((yb < 0) & (alpha < C - 1e-12))
        gap = (np.where(up, score, -np.inf).max(1)
               - np.where(lo, score, np.inf).min(1))
        for k, f in enumerate(fs):
            te = plan.test_idx[f, :plan.n_test[f]]
            for c in range(nv):
                q = k * nv + c
                d[c, f, :len(te)] = (K64[c][np.ix_(te, trs[k])]
                                     @ (alpha[q] * yb[q]) + b[q])
                conv[c, f] = gap[q] < tol
    return d, conv


Case = namedtuple("Case", "family shape plan shared K valid y_test d_star "
                          "conv dev")


@functools.lru_cache(maxsize=None)
def _case(family, shape):
    """Inputs and references of one case, computed once per process."""
    fam = FAMILIES[family]
    labels, plan, shared = _shape(shape)
    seed = 1000 * (fam.seed + 1) + sum(map(ord, family + shape))
    if fam.recipe == "gram":
        K = _gram_kernels(plan.E, N_VOXELS, labels, seed)
    else:
        K = _feature_kernels(plan.E, N_VOXELS, labels, seed,
                             dim=int(fam.recipe[4:]), sep=fam.sep)
    K = (K * fam.scale).float().contiguous()
    K64 = K.double().numpy()
    valid = np.arange(plan.E)[None, :] < plan.n_test[:, None]      # [F, E]
    y_test = np.where(valid, plan.y[plan.test_idx], 0.0)
    if family in MAGNITUDE:
        d_star = _oracle(K64, K64, plan, fam.C)
        d_twin, conv = _twin(K64, K64, plan, fam.C, fam.tol)
        dev = np.abs(d_twin - d_star)[:, valid].max()
        if plan.fp16:
            Kr = np.stack([_round_fp16_scaled(k) for k in K64])
            d_r, conv = _twin(K64, Kr, plan, fam.C, fam.tol)
            dev += np.abs(d_r - d_twin)[:, valid].max()
    else:
        Kr = _round_fp16(K64) if plan.fp16 else K64
        d_star = _oracle(K64, Kr, plan, fam.C)
        d_twin, conv = _twin(K64, Kr, plan, fam.C, fam.tol)
        dev = np.abs(d_twin - d_star)[:, valid].max()
    return Case(family, shape, plan, shared, K, valid, y_test, d_star, conv,
                float(dev))


def _family_cases(family):
    return [_case(f, s) for f, s in CASES if f == family]


def _round_up_2(x):
    e = math.floor(math.log10(x)) - 1
    return math.ceil(x / 10 ** e - 1e-9) * 10 ** e


def _unsafe_share(cases, bound):
    unsafe = sum(int((np.abs(c.d_star)[:, c.valid] <= bound).sum())
                 for c in cases)
    total = sum(int(c.valid.sum()) * c.K.shape[0] for c in cases)
    return unsafe / total


# ---------------------------------------------------------------------------
# CPU tests: the references against each other
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("family", list(FAMILIES))
def test_bound_not_stale(family):
    """The family's bound still is at least twice the distance between the
    fp32 twin and the fp64 oracle, and at most a tenth of the family's
    test samples lie within the bound of the boundary."""
    cases = _family_cases(family)
    dev = max(c.dev for c in cases)
    bound = FAMILIES[family].bound
    print(f"{family}: dev {dev:.3g} bound {bound:.3g}")
    assert dev <= bound / 2
    assert _unsafe_share(cases, bound) <= 0.10


@pytest.mark.parametrize("family,shape", [("feat10", "e30f4"),
                                          ("gram", "e64f4")])
def test_oracle_agrees_with_fp64_smo(family, shape):
    """sklearn's optimum against smo_batch_train in fp64 at tol 1e-9."""
    c = _case(family, shape)
    K64 = c.K.double().numpy()
    d, conv = _twin(K64, K64, c.plan, FAMILIES[family].C, 1e-9,
                    dtype=torch.float64, max_iter=200000)
    assert conv.all()
    err = np.abs(d - c.d_star)[:, c.valid].max()
    print(f"{family}-{shape}: |d_smo64 - d*| {err:.3g}")
    assert err <= 1e-5


# ---------------------------------------------------------------------------
# GPU tests: the kernels against the references
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from brainiak_amd import ops as _ops
    if _ops.load_extension() is None:
        pytest.fail("HIP extension not built — GPU box must load it")
    return _ops


def _check(ops, c, variant):
    fam = FAMILIES[c.family]
    plan = c.plan
    args = (c.K.cuda(), torch.tensor(plan.y).cuda(),
            torch.tensor(plan.train_idx).cuda(),
            torch.tensor(plan.test_idx).cuda(),
            torch.tensor(plan.n_train).cuda(),
            torch.tensor(plan.n_test).cuda())
    kw = dict(C=fam.C, tol=fam.tol, max_iter=MAX_ITER, max_n=plan.max_n,
              variant=variant)
    correct, dec, n_iter = ops.svm_cv_trace(*args, **kw)
    plain = ops.svm_cv(*args, **kw)
    torch.cuda.synchronize()
    correct = correct.cpu().numpy()
    dec = dec.cpu().numpy().astype(np.float64)
    n_iter = n_iter.cpu().numpy()
    nv = c.K.shape[0]
    assert dec.shape == (nv, plan.F, plan.E)
    assert n_iter.shape == correct.shape == (nv, plan.F)

    err = np.abs(dec - c.d_star)[:, c.valid]
    print(f"{c.family}-{c.shape}-{variant}: max |dec - d*| "
          f"{np.nanmax(err):.3g} (bound {fam.bound:.3g}), max n_iter "
          f"{n_iter.max()}, twin unconverged "
          f"{int((~c.conv).sum())}, kernel at max_iter "
          f"{int((n_iter >= MAX_ITER).sum())}")
    assert np.isfinite(dec).all()
    assert (dec[:, ~c.valid] == 0).all()
    assert err.max() <= fam.bound

    # the counts are the signs of the decision values
    right = ((dec > 0) == (c.y_test > 0)[None]) & c.valid[None]
    assert (correct == right.sum(axis=2)).all()
    assert (plain.cpu().numpy() == correct).all()

    # count interval against the oracle: a sample within the bound of the
    # boundary may go either way, every other one as d* says
    safe = (np.abs(c.d_star) > fam.bound) & c.valid[None]
    sure = (safe & ((c.d_star > 0) == (c.y_test > 0)[None])).sum(axis=2)
    unsafe = (~safe & c.valid[None]).sum(axis=2)
    assert (sure <= correct).all() and (correct <= sure + unsafe).all()

    # the kernel converges wherever the fp32 twin does
    assert (n_iter >= 0).all() and (n_iter <= MAX_ITER).all()
    assert (n_iter[c.conv] < MAX_ITER).all()


@pytest.mark.gpu
@pytest.mark.parametrize("family,shape", CASES)
def test_wave_kernel_matches_oracle(ops, family, shape):
    _check(ops, _case(family, shape), "wave")


@pytest.mark.gpu
@pytest.mark.parametrize("family,shape",
                         [(f, s) for f, s in CASES if _shape(s)[2]])
def test_shared_kernel_matches_oracle(ops, family, shape):
    _check(ops, _case(family, shape), "shared")


@pytest.mark.gpu
def test_shared_flags_match_the_dispatcher(ops):
    """The table's 'shared' column is the dispatcher's own rule, so no
    shape the shared kernel covers is left to the wave kernel alone."""
    for s in sorted({s for _, s in CASES}):
        _, plan, shared = _shape(s)
        assert bool(ops._ext().svm_cv_shared_fits(plan.E, plan.max_n)) \
            == shared, s


if __name__ == "__main__":
    print(f"{'family':12s} {'dev':>9s} {'4*dev^':>9s} {'bound':>9s} "
          f"{'unsafe':>7s} {'med|d*|':>8s} twin-unconverged")
    for family in [a for a in sys.argv[1:] if a in FAMILIES] or FAMILIES:
        cases = _family_cases(family)
        dev = max(c.dev for c in cases)
        bound = FAMILIES[family].bound or _round_up_2(4 * dev)
        med = np.median(np.concatenate(
            [np.abs(c.d_star)[:, c.valid].ravel() for c in cases]))
        unconv = [(c.shape, int((~c.conv).sum())) for c in cases
                  if not c.conv.all()]
        print(f"{family:12s} {dev:9.3g} {_round_up_2(4 * dev):9.3g} "
              f"{bound:9.3g} {_unsafe_share(cases, bound):7.3f} "
              f"{med:8.3g} {unconv}")
        if "-v" in sys.argv:
            for c in cases:
                print(f"    {c.shape:12s} dev {c.dev:.3g}")
