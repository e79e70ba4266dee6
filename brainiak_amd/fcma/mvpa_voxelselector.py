"""Activity-based voxel selection via Searchlight (API parity:
ref src/brainiak/fcma/mvpa_voxelselector.py:34-136).

The per-searchlight statistic here runs the stratified k-fold loop
explicitly (clone → fit → score per split) rather than delegating to
``cross_val_score``: the explicit loop skips sklearn's indexing/
cloning scaffolding per fold and keeps the hot path obvious.

``run(clf, device=...)`` is the batched path for a linear ``SVC``: a
linear SVM sees a searchlight only through the [E, E] Gram matrix of
its activity vectors, so every centre of a block stack is scored from
``ops.searchlight_gram`` (one HIP launch per chunk of centres) and the
batched precomputed-kernel cross-validation the correlation-based
selector already uses, instead of ``num_folds`` libsvm fits per centre
under a triple Python loop.
"""

import logging

import numpy as np
from sklearn import model_selection
from sklearn.base import clone

from ..utils.timing import stage_timer

logger = logging.getLogger(__name__)

__all__ = ["MVPAVoxelSelector"]

# upper bound on the bytes of Gram matrices (N * E * E * 4) held per
# chunk of searchlight centres on the device path
_GRAM_CHUNK_BYTES = 1 << 30


def _sl_accuracy(data, mask, myrad, bcast_var):
    """Mean stratified-CV accuracy of one searchlight's activity
    vectors.  ``bcast_var`` unpacks to (labels, num_folds, clf)."""
    labels, num_folds, clf = bcast_var
    samples = data[0][mask, :].T          # [epoch, in-light voxel]
    labels = np.asarray(labels)
    folds = model_selection.StratifiedKFold(n_splits=num_folds,
                                            shuffle=False)
    scores = []
    for fit_idx, eval_idx in folds.split(samples, labels):
        member = clone(clf)
        member.fit(samples[fit_idx], labels[fit_idx])
        scores.append(member.score(samples[eval_idx],
                                   labels[eval_idx]))
    return float(np.mean(scores))


class MVPAVoxelSelector:
    """Searchlight-driven activity-based voxel selection.

    Parameters: data [x, y, z, epoch] (from
    prepare_searchlight_mvpa_data), mask 3-D, labels per epoch,
    num_folds, and a Searchlight instance.
    """

    def __init__(self, data, mask, labels, num_folds, sl):
        self.data = data
        self.mask = np.asarray(mask).astype(bool)
        if not self.mask.any():
            raise ValueError('Zero processed voxels')
        self.labels = labels
        self.num_folds = num_folds
        self.sl = sl

    def run(self, clf, device=None):
        """Returns (result_volume, [(voxel_id, accuracy)] sorted desc).

        device=None runs ``clf`` (any sklearn classifier) once per fold
        and searchlight on the host.  device="cpu", "cuda" or a
        ``torch.device`` scores every searchlight from its Gram matrix
        in batches on that device; this takes only an
        ``sklearn.svm.SVC`` with ``kernel='linear'`` and
        ``class_weight=None`` and two-class labels, and uses the
        classifier's ``C`` and ``tol``.
        """
        ctx = self.sl.comm
        if ctx.is_root:
            logger.info('activity-based selection: searchlight sweep '
                        'starting')
        if device is None:
            self.sl.distribute([self.data], self.mask)
            self.sl.broadcast((self.labels, self.num_folds, clf))
            volume = self.sl.run_searchlight(_sl_accuracy)
        else:
            volume = self._run_device(clf, device)

        ranked = []
        if ctx.is_root:
            in_mask = volume[self.mask]
            ranked = [(vid, acc if acc is not None else 0)
                      for vid, acc in enumerate(in_mask)]
            ranked.sort(key=lambda pair: pair[1], reverse=True)
            logger.info('activity-based selection: sweep finished '
                        '(%d voxels scored)', len(ranked))
        return volume, ranked

    # -- batched device path -----------------------------------------------

    def _linear_svc_params(self, clf):
        """(C, tol) of a classifier the Gram path reproduces; ValueError
        for anything else."""
        from sklearn.svm import SVC
        why = None
        if not isinstance(clf, SVC):
            why = 'the classifier is not an sklearn.svm.SVC'
        elif clf.kernel != 'linear':
            why = "the SVC kernel is %r, not 'linear'" % (clf.kernel,)
        elif clf.class_weight is not None:
            why = 'class_weight is set'
        elif len(np.unique(np.asarray(self.labels))) != 2:
            why = 'labels do not hold exactly two classes'
        if why is not None:
            raise ValueError(
                'MVPAVoxelSelector.run(device=...) scores searchlights '
                'from their Gram matrices, which covers a linear SVC on '
                'two classes only (%s); use device=None to run this '
                'classifier on the host path' % why)
        return float(clf.C), float(clf.tol)

    def _run_device(self, clf, device):
        import torch

        from .. import ops
        from .svm import (FoldPlan, cross_validate_voxels, stratified_folds,
                          svm_cv_device)

        C, tol = self._linear_svc_params(clf)
        sl = self.sl
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            # every rank on its own device
            device = sl.comm.device if sl.comm.device.type == 'cuda' \
                else torch.device('cuda', torch.cuda.current_device())
        labels = np.asarray(self.labels)
        num_folds = self.num_folds
        proportion = sl.min_active_voxels_proportion

        plan = None
        if device.type == 'cuda' and ops.require_hip():
            folds = stratified_folds(labels, num_folds)
            if max(max(len(tr), len(te)) for tr, te in folds) <= 128:
                plan = FoldPlan(labels, num_folds, device)

        def score(gram):
            if plan is not None:
                return svm_cv_device(gram, plan, C, tol).to(torch.float64)
            accs = cross_validate_voxels(gram, labels, num_folds, C=C,
                                         tol=tol, process_num=0)
            return torch.as_tensor(np.asarray(accs, dtype=np.float64),
                                   device=gram.device)

        def batch_fn(stacks, mask_stack, rad, bcast_var, extra):
            x = torch.as_tensor(stacks[0]).to(
                device=device, dtype=torch.float32).contiguous()
            msk = torch.as_tensor(mask_stack).to(device=device,
                                                 dtype=torch.bool)
            shape = torch.as_tensor(sl.shape).to(device=device,
                                                 dtype=torch.bool)
            B, bx, by, bz = msk.shape
            E = x.shape[-1]
            K = 2 * rad + 1
            active = msk[:, rad:bx - rad, rad:by - rad,
                         rad:bz - rad].clone()
            if proportion != 0:
                # in-light voxel counts: exact small integers in fp32
                if device.type == 'cuda':
                    counts = ops.stencil3d(msk.float().contiguous(),
                                           shape.float().contiguous())
                else:
                    counts = torch.nn.functional.conv3d(
                        msk.float()[:, None], shape.float()[None, None]
                    )[:, 0]
                active &= counts.double() / float(K ** 3) > proportion
            where = active.nonzero()
            centres = ((where[:, 0] * bx + where[:, 1] + rad) * by
                       + where[:, 2] + rad) * bz + where[:, 3] + rad
            n_total = int(centres.shape[0])
            accs = torch.empty(n_total, dtype=torch.float64, device=device)
            step = max(1, _GRAM_CHUNK_BYTES // (E * E * 4))
            mask_u8 = msk.to(torch.uint8)
            shape_u8 = shape.to(torch.uint8)
            for lo in range(0, n_total, step):
                with stage_timer('searchlight Gram', logger,
                                 sync_device=device):
                    gram = ops.searchlight_gram(x, mask_u8, shape_u8,
                                                centres[lo:lo + step])
                with stage_timer('searchlight cross validation', logger,
                                 sync_device=device):
                    accs[lo:lo + step] = score(gram)
            out = torch.full(active.shape, float('nan'),
                             dtype=torch.float64, device=device)
            out[active] = accs
            return out.cpu().numpy()

        sl.distribute([self.data], self.mask)
        # the block stacks cached on a device belong to the previous
        # distribute() call
        sl._device_group_cache = None
        sl.broadcast(None)
        if device.type == 'cuda':
            volume = sl.run_batched_block_function_device(batch_fn, device)
        else:
            volume = sl.run_batched_block_function(batch_fn)
        # NaN marks the centres the sweep left out: None, as on the host
        # (None also reads as NaN in the float view)
        volume[np.isnan(volume.astype(np.float64))] = None
        return volume
