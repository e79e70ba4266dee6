"""Intersubject correlation (ISC/ISFC) and its nonparametric statistics.

API parity with the reference isc module (ref src/brainiak/isc.py:81-1551):
``isc``, ``isfc``, ``compute_summary_statistic``, ``squareform_isfc``,
``bootstrap_isc`` (subject bootstrap with Hall-Wilson shift),
``permutation_isc`` (one-sample sign-flip / two-sample label shuffle, exact
tests when the permutation space is small), ``timeshift_isc`` (circular
shifts), ``phaseshift_isc`` (FFT phase randomization).

The implementations are vectorized rather than per-iteration loops:
pairwise ISC is one einsum over z-scored series, leave-one-out means
use the sum trick (total minus subject) instead of ``np.delete``, the
bootstrap resamples all iterations with one fancy-index, and the
one-sample permutation test applies every sign-flip as a single
matrix product.

MI355X additions:
 - the heavy ISFC gemms run through torch (rocBLAS/MFMA on GPU tensors);
 - ``isfc_distributed``: subject-sharded leave-one-out ISFC over RCCL —
   each rank holds a subset of subjects, the across-subject (nan-aware)
   sum rides ONE all-reduce, and each rank correlates its subjects
   against the leave-one-out mean on its own GPU (BASELINE config 4:
   50k voxels x 32 subjects over xGMI);
 - ``isc`` itself takes ``device=``: per voxel, the correlation of every
   subject with its leave-one-out mean, or of every subject pair, as a
   centred two-pass fp64 correlation straight from the [TR, voxel,
   subject] layout, in voxel chunks (``_isc_corr``: the HIP kernels
   ``ops.isc_loo`` / ``ops.isc_pairwise`` on a GPU, a torch twin
   elsewhere), under the NaN policy of the numpy path; the summary
   statistic is ``_resample_stat`` with one identity draw.
   ``timeshift_isc`` / ``phaseshift_isc`` take its result as
   ``observed=`` and then skip their host ``isc`` call;
 - ``bootstrap_isc`` / ``permutation_isc`` / leave-one-out
   ``timeshift_isc`` take ``device=``: the null distribution is then a
   per-draw gather + median / Fisher mean over a fixed table
   (``_resample_stat``: the HIP kernel ``ops.isc_resample_stat`` on a
   GPU, its torch twin elsewhere) from the same draws as the numpy
   path;
 - ``phaseshift_isc`` takes ``device=`` too (leave-one-out and
   pairwise): the correlation of a phase-randomised series with a fixed
   one is linear in the cosines and sines of the drawn phases, so the
   null is one contraction of a per-draw coefficient block with a fixed
   spectral table followed by the same statistic (``_phase_stat``: the
   HIP kernel ``ops.isc_phase_stat`` on a GPU, a batched-matmul twin
   elsewhere), without any per-draw FFT.

Citations as in the reference: [Hasson2004], [Simony2016], [Chen2016],
[HallWilson1991], [PhipsonSmyth2010], [SilverDunlap1987].
"""

import logging
import math
import os
from itertools import combinations, permutations

import numpy as np
from scipy.spatial.distance import squareform

from .fcma.util import compute_correlation
from .utils.utils import (
    _check_timeseries_input,
    array_correlation,
    p_from_null,
    phase_randomize,
)

logger = logging.getLogger(__name__)

MAX_RANDOM_SEED = 2 ** 32 - 1

__all__ = [
    "bootstrap_isc",
    "compute_summary_statistic",
    "isc",
    "isfc",
    "isfc_distributed",
    "permutation_isc",
    "phaseshift_isc",
    "squareform_isfc",
    "timeshift_isc",
]


def _as_rng(random_state):
    """Coerce None / int seed / RandomState into a RandomState."""
    if isinstance(random_state, np.random.RandomState):
        return random_state
    return np.random.RandomState(random_state)


def _drop_bad_voxels(data, tolerate_nans):
    """Voxel NaN policy shared by isc/isfc.

    A voxel is dropped when every subject has a NaN somewhere in its
    series; a float policy in [0, 1] additionally requires that
    fraction of subjects to be NaN-free.  Returns (filtered data,
    keep mask over voxels).
    """
    nan_somewhere = np.any(np.isnan(data), axis=0)      # [voxel, subject]
    keep = ~np.all(nan_somewhere, axis=1)
    if tolerate_nans is True:
        logger.info("ISC: averaging will tolerate all NaNs")
    elif isinstance(tolerate_nans, float):
        if not 0.0 <= tolerate_nans <= 1.0:
            raise ValueError("If threshold to tolerate NaNs is a float, "
                             "it must be between 0.0 and 1.0; got "
                             f"{tolerate_nans}")
        clean_subjects = np.sum(~nan_somewhere, axis=1)
        keep &= clean_subjects >= data.shape[-1] * tolerate_nans
        logger.info("ISC: voxels need a %s fraction of NaN-free "
                    "subjects; %d voxels dropped", tolerate_nans,
                    int(np.sum(~keep)))
    else:
        logger.info("ISC: averaging will not tolerate NaNs")
    return data[:, keep, :], keep


def _loo_means(data, use_nanmean):
    """Leave-one-out across-subject means, [TR, voxel, subject], via
    the sum trick (one pass instead of n_subjects ``np.delete``s)."""
    n = data.shape[-1]
    if use_nanmean:
        finite = np.isfinite(data)
        totals = np.nansum(data, axis=2, keepdims=True)
        counts = finite.sum(axis=2, keepdims=True)
        num = totals - np.where(finite, data, 0.0)
        den = counts - finite
        with np.errstate(invalid="ignore", divide="ignore"):
            return num / den
    totals = data.sum(axis=2, keepdims=True)
    return (totals - data) / (n - 1)


def _pairwise_voxel_correlations(data):
    """r for every subject pair at every voxel in one einsum.

    data [TR, voxel, subject] → [pair, voxel] with pairs in
    ``combinations`` (row-major upper-triangle) order.
    """
    centered = data - data.mean(axis=0)
    norms = np.sqrt(np.einsum("tvs,tvs->vs", centered, centered))
    with np.errstate(invalid="ignore", divide="ignore"):
        unit = centered / norms
    gram = np.einsum("tvi,tvj->vij", unit, unit)        # [voxel, s, s]
    iu = np.triu_indices(data.shape[-1], k=1)
    return gram[:, iu[0], iu[1]].T


def isc(data, pairwise=False, summary_statistic=None, tolerate_nans=True,
        device=None):
    """Intersubject correlation per voxel (leave-one-out or pairwise).

    ``device`` (``"cpu"``, ``"cuda"``, a ``torch.device``): compute on
    that device (``_isc_corr``: the HIP kernels ``ops.isc_loo`` /
    ``ops.isc_pairwise`` on a GPU, their torch twin elsewhere), in voxel
    chunks; ``None`` keeps the numpy path.  The device path returns the
    same shapes and type (numpy float64) under the same NaN policy.  Its
    arithmetic is fp64 whatever the input dtype.  There ``data`` may
    also be a 3-D ``torch.Tensor`` [TR, voxel, subject] (fp32 or fp64,
    on any device); one that already lives on the compute device is not
    copied through the host.
    """
    if device is not None:
        return _isc_device(data, pairwise, summary_statistic,
                           tolerate_nans, device)
    data, n_TRs, n_voxels, n_subjects = _check_timeseries_input(data)

    if n_subjects == 2:
        logger.info("Only two subjects! Simply computing Pearson "
                    "correlation.")
        summary_statistic = None

    data, keep = _drop_bad_voxels(data, tolerate_nans)

    if n_subjects == 2:
        rows = array_correlation(data[..., 0], data[..., 1])[None, :]
    elif pairwise:
        rows = _pairwise_voxel_correlations(data)
    else:
        loo = _loo_means(data, use_nanmean=bool(tolerate_nans))
        rows = np.stack([array_correlation(data[..., s], loo[..., s])
                         for s in range(n_subjects)])

    iscs = np.full((rows.shape[0], n_voxels), np.nan)
    iscs[:, keep] = rows

    if summary_statistic:
        iscs = compute_summary_statistic(
            iscs, summary_statistic=summary_statistic, axis=0)[None, :]
    return iscs[0] if iscs.shape[0] == 1 else iscs


def _resolve_targets(targets, data):
    """ISFC target handling: no targets → self-ISFC (symmetric)."""
    if not isinstance(targets, (np.ndarray, list)):
        t, v, s = data.shape
        return data, t, v, s, True
    targets, n_TRs, n_voxels, n_subjects = (
        _check_timeseries_input(targets))
    if data.shape[0] != n_TRs:
        raise ValueError("Targets array must have same number of "
                         "TRs as input data")
    if data.shape[2] != n_subjects:
        raise ValueError("Targets array must have same number of "
                         "subjects as input data")
    return targets, n_TRs, n_voxels, n_subjects, False


def isfc(data, targets=None, pairwise=False, summary_statistic=None,
         vectorize_isfcs=True, tolerate_nans=True):
    """Intersubject functional correlation: correlations between each
    voxel's time series and every (target) voxel in other subjects."""
    data, n_TRs, n_voxels, n_subjects = _check_timeseries_input(data)
    targets, _, _, _, symmetric = _resolve_targets(targets, data)
    if not symmetric:
        pairwise = False
    data, keep = _drop_bad_voxels(data, tolerate_nans)
    targets, keep_t = _drop_bad_voxels(targets, tolerate_nans)

    def corr(a, b):
        return compute_correlation(np.ascontiguousarray(a.T),
                                   np.ascontiguousarray(b.T),
                                   return_nans=True)

    if symmetric and n_subjects == 2:
        logger.info("Only two subjects! Computing ISFC between them.")
        m = corr(data[..., 0], data[..., 1])
        mats = [(m + m.T) / 2]
        summary_statistic = None
    elif pairwise:
        mats = []
        for a, b in combinations(range(n_subjects), 2):
            m = corr(data[..., a], targets[..., b])
            mats.append((m + m.T) / 2 if symmetric else m)
    else:
        use_nan = bool(tolerate_nans)
        loo = _loo_means(targets, use_nanmean=use_nan)
        mats = []
        for s in range(n_subjects):
            m = corr(data[..., s], loo[..., s])
            mats.append((m + m.T) / 2 if symmetric else m)

    expanded = np.full((len(mats), len(keep), len(keep_t)), np.nan)
    expanded[np.ix_(np.arange(len(mats)), keep, keep_t)] = \
        np.stack(mats)
    isfcs = expanded

    if summary_statistic:
        isfcs = compute_summary_statistic(
            isfcs, summary_statistic=summary_statistic, axis=0)
    if isfcs.shape[0] == 1:
        isfcs = isfcs[0]
    if vectorize_isfcs and symmetric:
        return squareform_isfc(isfcs)
    return isfcs


def isfc_distributed(local_data, comm, summary_statistic=None,
                     row_tile=4096, device=None, precision='fp32',
                     return_tensor=False):
    """Subject-sharded leave-one-out ISFC over RCCL/xGMI.

    Parameters
    ----------
    local_data : list of [n_TRs, n_voxels] arrays — THIS rank's subjects.
    comm : DistContext.
    summary_statistic : None | 'mean' | 'median'.  With 'mean' the
        across-subject reduction rides the same collective pass and the
        full per-subject stack is never materialized.
    row_tile : accepted for API stability; the full-matrix GEMM path
        is used — at the benchmark scale (50k voxels) the [V, V]
        matrices fit 288 GB HBM several times over.
    device : torch device override.

    Returns (on every rank)
    -----------------------
    summary_statistic None  → [n_subjects_total, V, V] stacked ISFCs
    summary_statistic given → [V, V] collapsed ISFC matrix

    precision 'bf16' runs the [T,V]x[T,V] correlation GEMMs on the
    MFMA bf16 path (~0.4 % relative error on r; fp32 is the default
    and matches the serial oracle).  ``return_tensor=True`` keeps the
    collapsed result on the compute device (the D2H of a [V, V]
    matrix dominates the GPU step otherwise).
    """
    import torch

    dev = torch.device(device) if device is not None else comm.device
    local = [d.to(device=dev, dtype=torch.float32)
             if isinstance(d, torch.Tensor)
             else torch.as_tensor(np.ascontiguousarray(d),
                                  dtype=torch.float32).to(dev)
             for d in local_data]
    V = local[0].shape[1] if local else 0
    T = local[0].shape[0] if local else 0
    meta = comm.all_gather_object((len(local), V, T))
    n_total = sum(m[0] for m in meta)
    V = max(m[1] for m in meta)
    T = max(m[2] for m in meta)

    # z-score each subject once (so correlation = dot of unit columns)
    def _norm(d):
        d = d - d.mean(dim=0)
        denom = d.norm(dim=0).clamp_min(1e-30)
        return d / denom

    # ONE all-reduce carries the across-subject sum for the LOO mean
    total = torch.zeros((T, V), dtype=torch.float32, device=dev)
    for d in local:
        total += d
    total = comm.all_reduce(total)

    normed_local = [_norm(d) for d in local]

    def _corr(a, b, keep_bf16=False):
        if precision == 'bf16':
            m = a.T.to(torch.bfloat16) @ b.to(torch.bfloat16)
            return m if keep_bf16 else m.float()
        return a.T @ b                          # [V, V]

    if summary_statistic == 'mean':
        from . import ops as _ops
        use_hip = dev.type == 'cuda' and _ops.require_hip()
        acc = torch.zeros((V, V), dtype=torch.float32, device=dev)
        if use_hip and precision == 'bf16' and local \
                and os.environ.get("BRAINIAK_ISFC_FUSED"):
            # fully fused path (OPT-IN): correlation tile pairs,
            # symmetrize, atanh and accumulation in ONE kernel — the
            # per-subject [V, V] matrix never touches HBM.  Measured
            # 270 vs 259 ms against the GEMM+accum pipeline at 50k x
            # 32: the hand MFMA schedule gives back more than the M
            # round trip saves (hipBLASLt's GEMM is ~3x our MFMA
            # utilization), so the GEMM path stays the default —
            # profiles/NEXT.md lists the tiling work that would flip
            # it.
            Zs = torch.stack([nd.T.contiguous().to(torch.bfloat16)
                              for nd in normed_local])
            Zm = torch.stack([
                _norm((total - d) / (n_total - 1)).T.contiguous()
                .to(torch.bfloat16) for d in local])
            _ops.isfc_fused_(acc, Zs, Zm)
            del Zs, Zm
        elif use_hip:
            # subjects stream through the fused sym+atanh+accumulate
            # kernel in stacks of up to 4: the [V, V] accumulator's
            # read-modify-write happens once per stack instead of once
            # per subject (acc traffic dominates at V=50k).  GEMMs
            # write straight into the stack buffer slices — no copies.
            nb = min(4, max(1, len(local)))
            gdt = (torch.bfloat16 if precision == 'bf16'
                   else torch.float32)
            stackbuf = torch.empty((nb, V, V), dtype=gdt, device=dev)
            pairs = list(zip(local, normed_local))
            j = 0
            for i, (d, nd) in enumerate(pairs):
                loo = _norm((total - d) / (n_total - 1))
                torch.matmul(nd.T.to(gdt), loo.to(gdt),
                             out=stackbuf[j])
                j += 1
                if j == nb or i == len(pairs) - 1:
                    _ops.isfc_accum_(acc, stackbuf[:j])
                    j = 0
            del stackbuf
        else:
            for d, nd in zip(local, normed_local):
                loo = _norm((total - d) / (n_total - 1))
                m = _corr(nd, loo)
                m = (m + m.T) / 2
                acc += torch.atanh(m.clamp(-1 + 1e-7, 1 - 1e-7))
        acc = comm.all_reduce(acc)
        out = torch.tanh(acc / n_total)
        if return_tensor:
            # device-resident result for GPU consumers: the pageable
            # D2H of a [50k, 50k] fp32 matrix costs ~1 s — more than
            # the whole on-device computation (profiles/README.md r2)
            return out
        if out.is_cuda:
            host = torch.empty_like(out, device="cpu",
                                    pin_memory=True)
            host.copy_(out)
            return host.numpy()
        return out.cpu().numpy()

    stacks = []
    for d, nd in zip(local, normed_local):
        loo = _norm((total - d) / (n_total - 1))
        m = _corr(nd, loo)
        stacks.append(((m + m.T) / 2).cpu().numpy())
    gathered = comm.all_gather_object(stacks)
    flat = [m for part in gathered for m in part]
    out = np.stack(flat)
    if summary_statistic == 'median':
        return np.nanmedian(out, axis=0)
    return out


def compute_summary_statistic(iscs, summary_statistic='mean', axis=None):
    """'mean' (Fisher-Z mean: tanh(mean(arctanh))) or 'median' of ISCs."""
    reducers = {
        'mean': lambda a: np.tanh(np.nanmean(np.arctanh(a), axis=axis)),
        'median': lambda a: np.nanmedian(a, axis=axis),
    }
    if summary_statistic not in reducers:
        raise ValueError("Summary statistic must be 'mean' or 'median'")
    return reducers[summary_statistic](iscs)


def squareform_isfc(isfcs, iscs=None):
    """Square ↔ condensed ISFC conversion retaining the ISC diagonal.

    Square [.., V, V] input (no iscs) → (condensed off-diagonals,
    diagonal ISCs); condensed input + iscs → square matrices.
    """
    have_iscs = isinstance(iscs, np.ndarray)
    square_in = not have_iscs and isfcs.shape[-2] == isfcs.shape[-1]

    if square_in:
        stack = isfcs[None] if isfcs.ndim == 2 else isfcs
        if stack.ndim != 3:
            raise ValueError("Square (redundant) ISFCs must be square "
                             "with multiple subjects or pairs of "
                             "subjects indexed by the first dimension")
        V = stack.shape[-1]
        iu = np.triu_indices(V, k=1)
        condensed = stack[:, iu[0], iu[1]]
        diags = np.diagonal(stack, axis1=1, axis2=2)
        if condensed.shape[0] == 1:
            return condensed[0], diags[0]
        return condensed, diags

    flat = isfcs[None] if isfcs.ndim == 1 else isfcs
    diag = iscs[None] if iscs.ndim == 1 else iscs
    V = diag.shape[-1]
    iu = np.triu_indices(V, k=1)
    squares = np.zeros((flat.shape[0], V, V), dtype=flat.dtype)
    squares[:, iu[0], iu[1]] = flat
    squares += np.transpose(squares, (0, 2, 1))
    squares[:, np.arange(V), np.arange(V)] = diag
    return squares[0] if squares.shape[0] == 1 else squares


# --------------------------------------------------------------------------
# nonparametric statistics
# --------------------------------------------------------------------------

def _coerce_iscs(iscs, pairwise):
    """Normalize ISC input to [row, voxel] and infer subject count."""
    iscs = np.asarray(iscs)
    if iscs.ndim == 1:
        iscs = iscs[:, None]
    if pairwise:
        try:
            n_subjects = squareform(iscs[:, 0],
                                    force='tomatrix').shape[0]
        except ValueError:
            raise ValueError("For pairwise input, ISCs must be the "
                             "vectorized triangle of a square matrix.")
    else:
        n_subjects = iscs.shape[0]
    logger.info("Nonparametric ISC test: %d subjects, %d voxel(s)/"
                "ROI(s)", n_subjects, iscs.shape[1])
    return iscs, n_subjects, iscs.shape[1]


# --------------------------------------------------------------------------
# device path of the resampling nulls
#
# Per draw and per voxel, every variant of the bootstrap, sign-flip,
# label-shuffle and time-shift tests gathers one value per subject (or
# pair) from a fixed table, optionally flips its sign or leaves it out,
# and takes the NaN-skipping median or Fisher mean of what it gathered.
# ``_resample_stat`` is that step: the HIP kernel
# ``ops.isc_resample_stat`` on a GPU table, a chunked torch twin
# anywhere else.
# --------------------------------------------------------------------------

# byte budget of the torch twin's [chunk, R, V] intermediates
_RESAMPLE_CHUNK_BYTES = 512 << 20
# live [chunk, R, V]-sized tensors at the twin's peak (gathered values,
# signed values, sorted values and the sort's int64 indices)
_RESAMPLE_CHUNK_COPIES = 4
# byte budget of one voxel chunk of the time-shift lag table with its
# FFT temporaries
_TIMESHIFT_CHUNK_BYTES = 2 << 30
# table-sized tensors alive while a lag table is built (series, LOO
# means, their unit forms, two half-spectra of complex128, the table)
_TIMESHIFT_CHUNK_COPIES = 8
# byte budget of one voxel chunk of the phase-shift table with its FFT
# temporaries
_PHASESHIFT_CHUNK_BYTES = 2 << 30
# table-sized tensors alive while a phase table is built (series, LOO
# means, their unit forms, two half-spectra of complex128 or the pair
# products, the table)
_PHASESHIFT_CHUNK_COPIES = 8


def _host_tensor(a, name):
    """Index / sign array (numpy or torch, any device) → int64 tensor
    on the host."""
    import torch
    t = a.detach().cpu() if isinstance(a, torch.Tensor) \
        else torch.from_numpy(np.ascontiguousarray(a))
    if t.dtype.is_floating_point or t.dtype.is_complex \
            or t.dtype == torch.bool:
        raise ValueError(f"{name} must be an integer array")
    return t.to(torch.int64)


def _stat_over_rows(x, stat):
    """NaN-skipping median (numpy's nanmedian) or Fisher mean over dim 1
    of x [c, R, V] -> [c, V]; NaN where nothing survives."""
    import torch
    R = x.shape[1]
    nan = torch.tensor(float("nan"), dtype=torch.float64, device=x.device)
    if stat == 'median':
        n = (~torch.isnan(x)).sum(dim=1)            # [c, V]
        # NaNs sort last; numpy's rule for an even count is the
        # mean of the two middle values (torch.nanmedian takes
        # the lower one)
        # (a GPU sort orders by bit pattern and puts a NaN whose sign bit
        # is set first, and arithmetic on the GPU does produce those: all
        # NaNs are made the positive one)
        xs = torch.sort(torch.where(torch.isnan(x), nan, x), dim=1).values
        hi = (n // 2).clamp(max=R - 1)
        lo = ((n - 1) // 2).clamp(min=0)
        v_hi = torch.gather(xs, 1, hi[:, None, :])[:, 0, :]
        v_lo = torch.gather(xs, 1, lo[:, None, :])[:, 0, :]
        med = torch.where(lo == hi, v_hi, (v_lo + v_hi) / 2)
        return torch.where(n > 0, med, nan)
    z = torch.atanh(x)
    ok = ~torch.isnan(z)
    total = torch.where(ok, z, torch.zeros_like(z)).sum(dim=1)
    return torch.tanh(total / ok.sum(dim=1))


def _resample_stat_torch(table, rows, lags, signs, stat):
    """Torch twin of ``ops.isc_resample_stat`` on any device, chunked
    over draws.  rows / lags / signs are tensors on the table's device;
    lags may be None."""
    import torch
    N, L, V = table.shape
    n_draws, R = rows.shape
    out = torch.full((n_draws, V), float("nan"), dtype=torch.float64,
                     device=table.device)
    if R == 0 or V == 0:
        return out
    flat = table.reshape(N * L, V)
    index = rows.long() * L
    if lags is not None:
        index = index + lags.long()
    per_draw = R * V * 8 * _RESAMPLE_CHUNK_COPIES
    chunk = max(1, _RESAMPLE_CHUNK_BYTES // per_draw)
    nan = torch.tensor(float("nan"), dtype=torch.float64,
                       device=table.device)
    for a in range(0, n_draws, chunk):
        b = min(n_draws, a + chunk)
        sg = signs[a:b].to(torch.float64)[:, :, None]
        x = torch.where(sg != 0, flat[index[a:b]] * sg, nan)  # [c, R, V]
        out[a:b] = _stat_over_rows(x, stat)
    return out


def _resample_stat(table, rows, lags, signs, stat):
    """out[i, v] = stat over the r with signs[i, r] != 0 and a non-NaN
    value of signs[i, r] * table[rows[i, r], lags[i, r], v].

    table : fp64 tensor [N, L, V] on the compute device.
    rows, lags, signs : integer arrays [I, R] (numpy or torch); lags may
        be None (all zero); signs hold +1 / -1 / 0 (0 leaves the entry
        out).  They are range-checked here, on the host, before any
        upload.
    stat : 'median' (numpy's nanmedian, even-count rule included) or
        'mean' (tanh(mean(atanh(x))); atanh results that are NaN are
        skipped, infinities are not).

    A GPU table goes through the HIP kernel ``ops.isc_resample_stat``
    (for 'median' while R is within ``ops.isc_resample_max_rows()``);
    everything else, and everything under
    ``BRAINIAK_ISC_RESAMPLE=torch``, takes the torch twin.  Returns an
    fp64 tensor [I, V] on the table's device.
    """
    import torch
    from . import ops
    if stat not in ('mean', 'median'):
        raise ValueError("Summary statistic must be 'mean' or 'median'")
    if not isinstance(table, torch.Tensor) or table.dim() != 3 \
            or table.dtype != torch.float64:
        raise ValueError("table must be an fp64 tensor [N, L, V]")
    N, L, V = table.shape
    rows_h = _host_tensor(rows, "rows")
    signs_h = _host_tensor(signs, "signs")
    lags_h = None if lags is None else _host_tensor(lags, "lags")
    if rows_h.dim() != 2:
        raise ValueError("rows must be [I, R]")
    if signs_h.shape != rows_h.shape or (
            lags_h is not None and lags_h.shape != rows_h.shape):
        raise ValueError("rows, lags and signs must have the same shape")
    if rows_h.numel():
        if int(rows_h.min()) < 0 or int(rows_h.max()) >= N:
            raise ValueError(f"rows must lie in [0, {N})")
        if lags_h is not None and (int(lags_h.min()) < 0
                                   or int(lags_h.max()) >= L):
            raise ValueError(f"lags must lie in [0, {L})")
        if L < 1:
            raise ValueError("table has no lags to gather from")
        if int(signs_h.abs().max()) > 1:
            raise ValueError("signs must be +1, -1 or 0")
    R = rows_h.shape[1]

    dev = table.device
    table = table.contiguous()
    rows_d = rows_h.to(torch.int32).to(dev)
    signs_d = signs_h.to(torch.int8).to(dev)
    lags_d = None if lags_h is None else lags_h.to(torch.int32).to(dev)

    if (table.is_cuda
            and os.environ.get("BRAINIAK_ISC_RESAMPLE", "") != "torch"
            and ops.require_hip()
            and (stat == 'mean' or R <= ops.isc_resample_max_rows())):
        return ops.isc_resample_stat(table, rows_d, lags_d, signs_d, stat)
    return _resample_stat_torch(table, rows_d, lags_d, signs_d, stat)


def _rows_null_device(iscs, rows, signs, summary_statistic, device):
    """Null distribution [I, voxel] (numpy) of a test whose draws pick
    rows of the ISC matrix itself (bootstrap, permutation)."""
    import torch
    table = torch.from_numpy(
        np.ascontiguousarray(iscs, dtype=np.float64))[:, None, :]
    out = _resample_stat(table.to(torch.device(device)), rows, None,
                         signs, summary_statistic)
    return out.cpu().numpy()


def _bootstrap_null_device(iscs, draws, n_subjects, pairwise,
                           summary_statistic, device):
    """Bootstrap null from the sorted subject draws [boot, subject]."""
    if not pairwise:
        return _rows_null_device(iscs, draws, np.ones_like(draws),
                                 summary_statistic, device)
    # the resampled pair (a, b), a < b, is the condensed pair of
    # subjects (draws[a], draws[b]); draws are sorted, so the first
    # is never the larger, and equal ones are left out
    iu = np.triu_indices(n_subjects, k=1)
    first, second = draws[:, iu[0]], draws[:, iu[1]]
    distinct = first != second
    pair = (first * n_subjects - first * (first + 1) // 2
            + (second - first - 1))
    return _rows_null_device(iscs, np.where(distinct, pair, 0),
                             distinct.astype(np.int8),
                             summary_statistic, device)


def _identity_rows(n_draws, n_rows):
    return np.broadcast_to(np.arange(n_rows), (n_draws, n_rows))


def _timeshift_lag_table(x):
    """All circular lags of every subject against its leave-one-out
    mean: x [S, T, V] → C [S, T, V] with C[s, k, v] the correlation of
    subject s rolled by k with the unshifted mean of the others."""
    import torch
    n_subjects, n_TRs, _ = x.shape
    loo = (x.sum(dim=0, keepdim=True) - x) / (n_subjects - 1)

    def unit(a):
        a = a - a.mean(dim=1, keepdim=True)
        return a / a.square().sum(dim=1, keepdim=True).sqrt()

    fx = torch.fft.rfft(unit(x), dim=1)
    fm = torch.fft.rfft(unit(loo), dim=1)
    # n_TRs may be odd: the output length has to be given
    return torch.fft.irfft(fx.conj() * fm, n=n_TRs, dim=1).contiguous()


def _timeshift_null_device(data, shifts, summary_statistic, device):
    """Leave-one-out time-shift null [shift, voxel] (numpy) from the
    per-draw subject shifts [shift, subject], in voxel chunks."""
    import torch
    dev = torch.device(device)
    n_TRs, n_voxels, n_subjects = data.shape
    n_shifts = shifts.shape[0]
    rows = _identity_rows(n_shifts, n_subjects)
    signs = np.ones((n_shifts, n_subjects), dtype=np.int8)
    per_voxel = n_subjects * n_TRs * 8 * _TIMESHIFT_CHUNK_COPIES
    chunk = max(64, _TIMESHIFT_CHUNK_BYTES // per_voxel // 64 * 64)
    distribution = np.empty((n_shifts, n_voxels))
    for a in range(0, n_voxels, chunk):
        b = min(n_voxels, a + chunk)
        x = torch.from_numpy(data[:, a:b, :]).to(
            device=dev, dtype=torch.float64)
        table = _timeshift_lag_table(x.permute(2, 0, 1).contiguous())
        del x
        out = _resample_stat(table, rows, shifts, signs,
                             summary_statistic)
        distribution[:, a:b] = out.cpu().numpy()
        del table, out
    return distribution


# --------------------------------------------------------------------------
# device path of the phase-randomisation null
#
# Phase randomisation multiplies bin f of a subject's spectrum by
# exp(i phi_f) (and the mirrored bin by its conjugate); it changes neither
# the mean nor the norm of the series.  With u the centred unit-norm
# series, w the centred unit-norm fixed series it is correlated with,
# U = rfft(u), W = rfft(w) and P = U conj(W), Parseval gives
#
#   r = sum_{f=1..F} (2/T) Re P_f cos phi_f - (2/T) Im P_f sin phi_f
#       + (1/T) Re P_{T/2}                    (even T: the Nyquist bin)
#
# with F = (T - 1) // 2 randomised bins and a zero DC term.  The pairwise
# test has P = U_a conj(U_b) and the phase difference phi_a - phi_b.  So
# a null value is the dot product of a fixed table column with the
# cosines and sines of the draw.
# --------------------------------------------------------------------------

def _phase_tables(x, pairwise):
    """Spectral table of the phase-shift null: x [S, T, V] -> fp64
    [R, K, V].  Rows: subjects against their unshifted leave-one-out
    mean (R = S), or subject pairs in ``combinations`` order (R =
    S (S - 1) / 2).  Columns: (2/T) Re P_f for f = 1..F, then
    -(2/T) Im P_f for f = 1..F, then (1/T) Re P_{T/2} for even T, so
    K = 2 F (+ 1).  All signs and factors of the formula live here; the
    coefficients are plain cosines, sines and ones."""
    import torch
    n_subjects, n_TRs, _ = x.shape
    F = (n_TRs - 1) // 2

    def unit(a):
        a = a - a.mean(dim=1, keepdim=True)
        return a / a.square().sum(dim=1, keepdim=True).sqrt()

    fx = torch.fft.rfft(unit(x), dim=1)                 # [S, T//2+1, V]
    if pairwise:
        iu = torch.triu_indices(n_subjects, n_subjects, offset=1,
                                device=x.device)
        P = fx[iu[0]] * fx[iu[1]].conj()
    else:
        loo = (x.sum(dim=0, keepdim=True) - x) / (n_subjects - 1)
        P = fx * torch.fft.rfft(unit(loo), dim=1).conj()
    parts = [P.real[:, 1:F + 1] * (2.0 / n_TRs),
             P.imag[:, 1:F + 1] * (-2.0 / n_TRs)]
    if n_TRs % 2 == 0:
        half = n_TRs // 2
        parts.append(P.real[:, half:half + 1] * (1.0 / n_TRs))
    return torch.cat(parts, dim=1).contiguous()


def _phase_coef(phases, pairwise, n_TRs):
    """Coefficient block of the phase-shift null: phases [I, F, S]
    (radians, a tensor on the compute device) -> fp64 [I, R, K] matching
    ``_phase_tables``: cos, then sin, of each row's phase (a subject's,
    or the difference first - second of a pair's), then a column of ones
    for the Nyquist row of an even ``n_TRs``."""
    import torch
    n_draws, _, n_subjects = phases.shape
    ph = phases.permute(0, 2, 1)                        # [I, S, F]
    if pairwise:
        iu = torch.triu_indices(n_subjects, n_subjects, offset=1,
                                device=phases.device)
        ph = ph[:, iu[0]] - ph[:, iu[1]]
    parts = [torch.cos(ph), torch.sin(ph)]
    if n_TRs % 2 == 0:
        parts.append(torch.ones((n_draws, ph.shape[1], 1),
                                dtype=ph.dtype, device=ph.device))
    return torch.cat(parts, dim=2).contiguous()


def _phase_stat_torch(table, coef, stat):
    """Torch twin of ``ops.isc_phase_stat`` on any device: a batched
    matmul over the rows, chunked over draws by the byte budget of the
    resampling twin, then the same statistic."""
    import torch
    R, K, V = table.shape
    n_draws = coef.shape[0]
    out = torch.full((n_draws, V), float("nan"), dtype=torch.float64,
                     device=table.device)
    if V == 0:
        return out
    per_draw = R * V * 8 * _RESAMPLE_CHUNK_COPIES
    chunk = max(1, _RESAMPLE_CHUNK_BYTES // per_draw)
    for a in range(0, n_draws, chunk):
        b = min(n_draws, a + chunk)
        # [R, c, K] @ [R, K, V] -> [R, c, V]
        x = torch.bmm(coef[a:b].transpose(0, 1), table)
        out[a:b] = _stat_over_rows(x.transpose(0, 1), stat)
    return out


def _phase_stat(table, coef, stat):
    """out[i, v] = stat over the r with a non-NaN
    x[i, r, v] = sum_k coef[i, r, k] * table[r, k, v].

    table : fp64 tensor [R, K, V]; coef : fp64 tensor [I, R, K] on the
    same device; R >= 1, K >= 1.
    stat : 'median' or 'mean', as in ``_resample_stat``.

    A GPU table goes through the HIP kernel ``ops.isc_phase_stat`` (for
    'median' while R is within ``ops.isc_phase_max_rows()``); everything
    else, and everything under ``BRAINIAK_ISC_RESAMPLE=torch``, takes
    the torch twin.  Returns an fp64 tensor [I, V] on the table's
    device.
    """
    import torch
    from . import ops
    if stat not in ('mean', 'median'):
        raise ValueError("Summary statistic must be 'mean' or 'median'")
    for t, name, dims in ((table, "table", "[R, K, V]"),
                          (coef, "coef", "[I, R, K]")):
        if not isinstance(t, torch.Tensor) or t.dim() != 3 \
                or t.dtype != torch.float64:
            raise ValueError(f"{name} must be an fp64 tensor {dims}")
    R, K, _ = table.shape
    if coef.shape[1:] != (R, K) or coef.device != table.device:
        raise ValueError("coef [I, R, K] must agree with table [R, K, V] "
                         "in R and K and share its device")
    if R < 1 or K < 1:
        raise ValueError("table needs at least one row and one column")
    table = table.contiguous()
    coef = coef.contiguous()
    if (table.is_cuda
            and os.environ.get("BRAINIAK_ISC_RESAMPLE", "") != "torch"
            and ops.require_hip()
            and (stat == 'mean' or R <= ops.isc_phase_max_rows())):
        return ops.isc_phase_stat(table, coef, stat)
    return _phase_stat_torch(table, coef, stat)


def _phaseshift_null_device(data, phases, pairwise, summary_statistic,
                            device):
    """Phase-shift null [shift, voxel] (numpy) from the drawn phases
    [shift, F, subject] (radians), in voxel chunks sized by the rows of
    the table (subjects, or pairs).  The coefficient block is built once,
    so every chunk sees the same draws."""
    import torch
    dev = torch.device(device)
    n_TRs, n_voxels, n_subjects = data.shape
    n_shifts = phases.shape[0]
    n_rows = n_subjects * (n_subjects - 1) // 2 if pairwise \
        else n_subjects
    coef = _phase_coef(
        torch.from_numpy(np.ascontiguousarray(phases, dtype=np.float64))
        .to(dev), pairwise, n_TRs)
    per_voxel = max(n_rows, n_subjects) * n_TRs * 8 \
        * _PHASESHIFT_CHUNK_COPIES
    chunk = max(64, _PHASESHIFT_CHUNK_BYTES // per_voxel // 64 * 64)
    distribution = np.empty((n_shifts, n_voxels))
    for a in range(0, n_voxels, chunk):
        b = min(n_voxels, a + chunk)
        x = torch.from_numpy(data[:, a:b, :]).to(
            device=dev, dtype=torch.float64)
        table = _phase_tables(x.permute(2, 0, 1).contiguous(), pairwise)
        del x
        out = _phase_stat(table, coef, summary_statistic)
        distribution[:, a:b] = out.cpu().numpy()
        del table, out
    return distribution


# --------------------------------------------------------------------------
# device path of the observed ISC
#
# Per voxel the work is one Pearson correlation per subject (against the
# leave-one-out mean) or per subject pair, each a centred two-pass
# r = sxy / sqrt(sxx * syy).  ``_isc_corr`` is that step with the voxel
# NaN policy applied: the HIP kernels ``ops.isc_loo`` / ``ops.isc_pairwise``
# on a GPU tensor, a torch twin of the same arithmetic anywhere else.  The
# summary statistic over the rows is ``_resample_stat`` with one identity
# draw.  Voxels are independent, so the array streams through in chunks.
# --------------------------------------------------------------------------

# byte budget of one voxel chunk of the observed ISC
_ISC_CHUNK_BYTES = 2 << 30
# chunk-sized tensors alive at the twin's peak (the fp64 series, the
# leave-one-out means, their centred forms, a product, a NaN mask)
_ISC_CHUNK_COPIES = 6


def _isc_min_clean(tolerate_nans, n_subjects):
    """NaN-free subjects a voxel needs under a float ``tolerate_nans``
    (the comparison of ``_drop_bad_voxels``); None without a threshold."""
    if tolerate_nans is True or not isinstance(tolerate_nans, float):
        return None
    if not 0.0 <= tolerate_nans <= 1.0:
        raise ValueError("If threshold to tolerate NaNs is a float, "
                         "it must be between 0.0 and 1.0; got "
                         f"{tolerate_nans}")
    return n_subjects * tolerate_nans


def _isc_corr_torch(x, pairwise, tolerant, min_clean):
    """Torch twin of ``ops.isc_loo`` / ``ops.isc_pairwise`` on any
    device: x fp64 [T, c, S] -> r [S or pairs, c]."""
    import torch
    n_TRs, _, n_subjects = x.shape
    nan_somewhere = torch.isnan(x).any(dim=0)           # [c, S]
    clean = (~nan_somewhere).sum(dim=1)
    keep = clean > 0
    if min_clean is not None:
        keep &= clean.to(torch.float64) >= min_clean
    if pairwise:
        xd = x - x.mean(dim=0)
        gram = torch.einsum("tvi,tvj->vij", xd, xd)     # [c, S, S]
        sxx = torch.diagonal(gram, dim1=1, dim2=2)      # [c, S]
        iu = torch.triu_indices(n_subjects, n_subjects, offset=1,
                                device=x.device)
        r = gram[:, iu[0], iu[1]] / torch.sqrt(sxx[:, iu[0]]
                                               * sxx[:, iu[1]])
    else:
        if tolerant:
            finite = torch.isfinite(x)
            zero = torch.zeros((), dtype=x.dtype, device=x.device)
            totals = torch.where(torch.isnan(x), zero, x).sum(
                dim=2, keepdim=True)
            counts = finite.sum(dim=2, keepdim=True)
            loo = (totals - torch.where(finite, x, zero)) \
                / (counts - finite.to(counts.dtype))
        else:
            loo = (x.sum(dim=2, keepdim=True) - x) / (n_subjects - 1)
        xd = x - x.mean(dim=0)
        ld = loo - loo.mean(dim=0)
        r = (xd * ld).sum(dim=0) / torch.sqrt((xd * xd).sum(dim=0)
                                              * (ld * ld).sum(dim=0))
    r = r.t().contiguous()
    r[:, ~keep] = float("nan")
    return r


def _isc_corr(x, v0, nv, pairwise, tolerant, min_clean):
    """Correlations of the voxels [v0, v0 + nv) of x (fp64 [T, V, S],
    contiguous) with the voxel NaN policy applied: rows are subjects
    against their leave-one-out mean (the NaN-skipping one if
    ``tolerant``), or subject pairs in ``combinations`` order.  A voxel
    without a NaN-free subject, or with fewer than ``min_clean`` of them
    (None: no threshold), is NaN in every row.

    A GPU tensor goes through the HIP kernels ``ops.isc_loo`` /
    ``ops.isc_pairwise`` (pairwise while S is within
    ``ops.isc_pairwise_max_subjects()``), which read the window in
    place; everything else, and everything under
    ``BRAINIAK_ISC_CORR=torch``, takes the torch twin.  Returns an fp64
    tensor [rows, nv] on x's device.
    """
    from . import ops
    if (x.is_cuda
            and os.environ.get("BRAINIAK_ISC_CORR", "") != "torch"
            and ops.require_hip()
            and (not pairwise
                 or x.shape[2] <= ops.isc_pairwise_max_subjects())):
        need = -1.0 if min_clean is None else float(min_clean)
        if pairwise:
            return ops.isc_pairwise(x, need, v0, nv)
        return ops.isc_loo(x, tolerant, need, v0, nv)
    return _isc_corr_torch(x[:, v0:v0 + nv, :], pairwise, tolerant,
                           min_clean)


class _PinnedStage:
    """One pinned host buffer that the voxel chunks of a host array pass
    through on their way to a GPU.  Gathering the strided window
    [T, a:b, S] into it is a threaded copy and the upload from it runs
    at the link's rate; torch's own strided host-to-device copy goes
    through a fresh pageable temporary per chunk (measured at 50k x 32 x
    200 in chunks of 6912 voxels: 4 + 6 ms a chunk against 80 ms)."""

    def __init__(self, x, chunk, dev):
        import torch
        n_TRs, n_voxels, n_subjects = x.shape
        self.dev = dev
        self.buf = torch.empty(
            n_TRs * min(chunk, n_voxels) * n_subjects, dtype=x.dtype,
            pin_memory=True)
        self.read = None                    # event: the last upload is done

    def upload(self, window):
        import torch
        if self.read is not None:
            self.read.synchronize()         # the buffer is free again
        staged = self.buf[:window.numel()].view(window.shape)
        staged.copy_(window)
        out = staged.to(self.dev, non_blocking=True)
        self.read = torch.cuda.Event()
        self.read.record(torch.cuda.current_stream(self.dev))
        return out


def _isc_chunk_to_device(x, a, b, dev, stage=None):
    """Voxels [a, b) of x [T, V, S] as (tensor, v0, nv) for ``_isc_corr``:
    x itself with the window when it already is an fp64 contiguous
    tensor on the compute device, a contiguous fp64 copy of the window
    there otherwise (through ``stage``, a ``_PinnedStage``, if given)."""
    import torch
    if x.device == dev and x.dtype == torch.float64 and x.is_contiguous():
        return x, a, b - a
    window = x[:, a:b, :]
    if stage is not None:
        window = stage.upload(window)
    xc = window.to(device=dev, dtype=torch.float64).contiguous()
    return xc, 0, b - a


def _isc_to_host(t):
    return t.cpu().numpy()


def _isc_device(data, pairwise, summary_statistic, tolerate_nans, device):
    """``isc`` on a torch device, in voxel chunks."""
    import torch
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    if isinstance(data, torch.Tensor):
        if data.dim() != 3:
            raise ValueError("Input tensor should have 3 dimensions "
                             f"(got {data.dim()})!")
        if data.dtype not in (torch.float32, torch.float64):
            raise ValueError("Input tensor should be fp32 or fp64")
        x = data.detach()
    else:
        data, _, _, _ = _check_timeseries_input(data)
        data = np.asarray(data)
        try:
            x = torch.from_numpy(data)
        except (TypeError, ValueError):     # e.g. negative strides
            x = torch.from_numpy(np.ascontiguousarray(data,
                                                      dtype=np.float64))
    n_TRs, n_voxels, n_subjects = x.shape
    if n_TRs < 1 or n_subjects < 2:
        raise ValueError("isc: the device path needs at least 1 TR and "
                         "2 subjects")
    if n_subjects == 2:
        logger.info("Only two subjects! Simply computing Pearson "
                    "correlation.")
        summary_statistic = None
        pairwise = True                     # the one pair is the result
    if summary_statistic and summary_statistic not in ('mean', 'median'):
        raise ValueError("Summary statistic must be 'mean' or 'median'")
    min_clean = _isc_min_clean(tolerate_nans, n_subjects)
    tolerant = bool(tolerate_nans)

    n_rows = n_subjects * (n_subjects - 1) // 2 if pairwise \
        else n_subjects
    per_voxel = 8 * (n_subjects * max(n_TRs, n_subjects)
                     * _ISC_CHUNK_COPIES + 4 * n_rows)
    chunk = max(64, _ISC_CHUNK_BYTES // per_voxel // 64 * 64)
    iscs = np.empty((1 if summary_statistic else n_rows, n_voxels))
    stage = None
    if dev.type == "cuda" and x.device.type == "cpu" and n_voxels:
        try:
            stage = _PinnedStage(x, chunk, dev)
        except RuntimeError:                # no pinned memory to be had
            stage = None
    for a in range(0, n_voxels, chunk):
        b = min(n_voxels, a + chunk)
        xc, v0, nv = _isc_chunk_to_device(x, a, b, dev, stage)
        rows = _isc_corr(xc, v0, nv, pairwise, tolerant, min_clean)
        del xc
        if summary_statistic:
            rows = _resample_stat(
                rows[:, None, :], np.arange(n_rows)[None, :], None,
                np.ones((1, n_rows), dtype=np.int8), summary_statistic)
        iscs[:, a:b] = _isc_to_host(rows)
        del rows
    return iscs[0] if iscs.shape[0] == 1 else iscs


def _expected_observed_shape(n_voxels, n_subjects, pairwise,
                             summary_statistic):
    """Shape of ``isc(data, pairwise, summary_statistic)``."""
    if n_subjects == 2 or summary_statistic:
        return (n_voxels,)
    n_rows = n_subjects * (n_subjects - 1) // 2 if pairwise \
        else n_subjects
    return (n_voxels,) if n_rows == 1 else (n_rows, n_voxels)


def _check_observed(observed, n_voxels, n_subjects, pairwise,
                    summary_statistic):
    """A caller's ``observed=`` as an array of the shape the internal
    ``isc`` call would return."""
    observed = np.asarray(observed)
    want = _expected_observed_shape(n_voxels, n_subjects, pairwise,
                                    summary_statistic)
    if observed.shape != want:
        raise ValueError(f"observed has shape {observed.shape}; "
                         f"isc() of this data returns {want}")
    return observed


def bootstrap_isc(iscs, pairwise=False, summary_statistic='median',
                  n_bootstraps=1000, ci_percentile=95, side='right',
                  random_state=None, device=None):
    """One-sample subject-level bootstrap with the Hall-Wilson shift.

    All ``n_bootstraps`` subject resamples are drawn up front and the
    summary statistic is applied to the whole [boot, subject, voxel]
    stack at once.  Resampled pairs of a subject with itself (pairwise
    mode) carry no information and are excluded as NaN.

    ``device`` (``"cpu"``, ``"cuda"``, a ``torch.device``): compute the
    bootstrap distribution on that device (``_resample_stat``) from the
    same draws; ``None`` keeps the numpy path.
    """
    iscs, n_subjects, n_voxels = _coerce_iscs(iscs, pairwise)
    if summary_statistic not in ('mean', 'median'):
        raise ValueError("Summary statistic must be 'mean' or 'median'")
    observed = compute_summary_statistic(
        iscs, summary_statistic=summary_statistic, axis=0)

    rng = _as_rng(random_state)
    draws = np.sort(rng.randint(0, n_subjects,
                                size=(n_bootstraps, n_subjects)), axis=1)

    if device is not None:
        distribution = _bootstrap_null_device(
            iscs, draws, n_subjects, pairwise, summary_statistic, device)
    elif pairwise:
        # square per-voxel matrices once, then each bootstrap is a
        # row/column gather + upper-triangle read
        V = n_voxels
        iu = np.triu_indices(n_subjects, k=1)
        sq = np.zeros((n_subjects, n_subjects, V))
        sq[iu[0], iu[1]] = iscs
        sq += np.transpose(sq, (1, 0, 2))
        gathered = sq[draws[:, :, None],
                      draws[:, None, :]]        # [boot, s, s, V]
        samples = gathered[:, iu[0], iu[1]]     # [boot, pair, V]
        self_pair = draws[:, iu[0]] == draws[:, iu[1]]
        samples[self_pair] = np.nan
    else:
        samples = iscs[draws]                   # [boot, subject, voxel]

    if device is None:
        distribution = compute_summary_statistic(
            samples, summary_statistic=summary_statistic, axis=1)

    half_alpha = (100 - ci_percentile) / 2
    ci = (np.percentile(distribution, half_alpha, axis=0),
          np.percentile(distribution, 100 - half_alpha, axis=0))
    p = p_from_null(observed, distribution - observed, side=side,
                    exact=False, axis=0)
    return observed, ci, p, distribution


class _GroupLayout:
    """Two-group bookkeeping for permutation_isc: label order, the
    pairwise label matrix, and the observed group selector."""

    def __init__(self, assignment, n_subjects, pairwise):
        self.assignment = assignment
        self.n_subjects = n_subjects
        uniques = np.unique(assignment) if assignment else np.array([])
        self.n_groups = max(1, len(uniques))
        if self.n_groups > 2:
            raise ValueError("This test is not valid for more than "
                             f"2 groups! (got {self.n_groups})")
        self.labels = uniques if self.n_groups == 2 else None
        self.matrix = None
        self.selector = None
        if self.n_groups == 2:
            a = np.asarray(assignment)
            if pairwise:
                # label matrix: within-group pairs carry the group
                # label, cross-group pairs are NaN
                lab = np.where(a[:, None] == a[None, :],
                               np.broadcast_to(a, (n_subjects,
                                                   n_subjects)),
                               np.nan).astype(float)
                np.fill_diagonal(lab, np.nan)
                self.matrix = lab
                self.selector = squareform(lab, checks=False)
            else:
                self.selector = a
        elif pairwise:
            self.matrix = np.ones((n_subjects, n_subjects))


def _normalize_assignment(group_assignment, n_subjects):
    if isinstance(group_assignment, np.ndarray):
        group_assignment = group_assignment.tolist()
    elif not isinstance(group_assignment, list):
        logger.info("No group assignment provided, "
                    "performing one-sample test.")
        group_assignment = None
    if group_assignment and len(group_assignment) != n_subjects:
        raise ValueError(
            f"Group assignments ({len(group_assignment)}) do not "
            f"match number of subjects ({n_subjects})!")
    return group_assignment


def _group_difference(iscs, selector, labels, summary_statistic):
    sel = np.asarray(selector)
    first = compute_summary_statistic(
        iscs[sel == labels[0]], summary_statistic=summary_statistic,
        axis=0)
    second = compute_summary_statistic(
        iscs[sel == labels[1]], summary_statistic=summary_statistic,
        axis=0)
    return first - second


def _sign_flip_rows(layout, flips, pairwise):
    """Per-permutation row multipliers from subject sign flips.

    flips [n_perm, n_subjects] → [n_perm, n_rows]: in pairwise mode a
    pair's sign is the product of its two subjects' signs.
    """
    if not pairwise:
        return flips
    iu = np.triu_indices(layout.n_subjects, k=1)
    return flips[:, iu[0]] * flips[:, iu[1]]


def permutation_isc(iscs, group_assignment=None, pairwise=False,
                    summary_statistic='median', n_permutations=1000,
                    side='right', random_state=None, device=None):
    """One-sample (sign-flip) / two-sample (label-shuffle) permutation
    test; exact enumeration when the permutation space fits in
    n_permutations.

    ``device`` (``"cpu"``, ``"cuda"``, a ``torch.device``): compute the
    permutation distribution on that device (``_resample_stat``) from
    the same flips / label orders; ``None`` keeps the numpy path."""
    iscs, n_subjects, n_voxels = _coerce_iscs(iscs, pairwise)
    if summary_statistic not in ('mean', 'median'):
        raise ValueError("Summary statistic must be 'mean' or 'median'")
    assignment = _normalize_assignment(group_assignment, n_subjects)
    layout = _GroupLayout(assignment, n_subjects, pairwise)
    rng = _as_rng(random_state)

    one_sample = layout.n_groups == 1
    space = 2 ** n_subjects if one_sample \
        else math.factorial(n_subjects)
    exact = n_permutations >= space

    if one_sample:
        observed = compute_summary_statistic(
            iscs, summary_statistic=summary_statistic, axis=0)[None, :]
        if exact:
            # every sign pattern via the bits of 0..2^n-1
            codes = np.arange(space)[:, None] >> np.arange(n_subjects)
            flips = 1.0 - 2.0 * (codes & 1)
            n_permutations = space
        else:
            flips = rng.choice([-1.0, 1.0],
                               size=(n_permutations, n_subjects))
        row_signs = _sign_flip_rows(layout, flips, pairwise)
        if device is not None:
            distribution = _rows_null_device(
                iscs, _identity_rows(*row_signs.shape),
                row_signs.astype(np.int8), summary_statistic, device)
        else:
            # [perm, row, voxel] in one broadcast multiply
            flipped = iscs[None] * row_signs[:, :, None]
            distribution = compute_summary_statistic(
                flipped, summary_statistic=summary_statistic, axis=1)
    else:
        observed = np.array(_group_difference(
            iscs, layout.selector, layout.labels, summary_statistic))
        if exact:
            orders = list(permutations(range(n_subjects)))
            n_permutations = space
        else:
            orders = [rng.permutation(n_subjects)
                      for _ in range(n_permutations)]
        rows = []
        base = np.asarray(layout.assignment)
        if device is not None:
            # the selector of every permutation at once: a row belongs
            # to a group's call where its (shuffled) label is that
            # group's; cross-group pairs (NaN labels) belong to neither
            orders = np.asarray(orders)
            if pairwise:
                iu = np.triu_indices(n_subjects, k=1)
                selectors = layout.matrix[orders[:, iu[0]],
                                          orders[:, iu[1]]]
            else:
                selectors = base[orders]
            groups = [_rows_null_device(
                iscs, _identity_rows(*selectors.shape),
                (selectors == label).astype(np.int8),
                summary_statistic, device) for label in layout.labels]
            distribution = groups[0] - groups[1]
        else:
            for order in orders:
                if pairwise:
                    shuffled_matrix = layout.matrix[np.ix_(order, order)]
                    selector = squareform(shuffled_matrix, checks=False)
                else:
                    selector = base[np.asarray(order)]
                rows.append(_group_difference(
                    iscs, selector, layout.labels, summary_statistic))
            distribution = np.array(rows)

    p = p_from_null(observed, distribution, side=side, exact=exact,
                    axis=0)
    return observed, p, distribution


def _null_from_resamples(data, observed, n_iter, side, draw_fn):
    """Shared shell of the timeshift/phaseshift tests: build the null
    distribution row by row from draw_fn(iteration) and convert to p."""
    rows = [np.asarray(draw_fn(i)).ravel() for i in range(n_iter)]
    distribution = np.vstack(rows)
    p = p_from_null(observed, distribution, side=side, exact=False,
                    axis=0)
    return observed, p, distribution


def _loo_null_isc(surrogate, data, summary_statistic, tolerate_nans):
    """Leave-one-out null: each surrogate subject vs the UNshifted
    mean of the others."""
    totals = data.sum(axis=2)
    n = data.shape[-1]
    cols = []
    for s in range(n):
        others_mean = (totals - data[..., s]) / (n - 1)
        cols.append(isc(np.dstack((surrogate[..., s], others_mean)),
                        pairwise=False, summary_statistic=None,
                        tolerate_nans=tolerate_nans))
    return compute_summary_statistic(
        np.dstack(cols), summary_statistic=summary_statistic, axis=2)


def timeshift_isc(data, pairwise=False, summary_statistic='median',
                  n_shifts=1000, side='right', tolerate_nans=True,
                  random_state=None, device=None, observed=None):
    """Circular time-shift null distribution for a one-sample ISC test.

    ``device`` (``"cpu"``, ``"cuda"``, a ``torch.device``): compute the
    null distribution on that device from the same shifts; ``None``
    keeps the numpy path.  Rolling subject s by k and correlating it
    with the unshifted leave-one-out mean is their circular
    cross-correlation at lag k, so all lags are tabulated once (by FFT,
    in voxel chunks) and every draw is a lookup (``_resample_stat``).
    Leave-one-out only: the pair-lag tables of the pairwise test would
    be n_subjects^2 / 2 times the data.

    The observed statistic comes from the host ``isc`` unless
    ``observed`` is given: an array of the shape that call returns
    (``ValueError`` otherwise), for instance the result of
    ``isc(data, ..., device="cuda")`` with the same ``pairwise``,
    ``summary_statistic`` and ``tolerate_nans``, which skips the host
    ISC, most of a device call's time.
    """
    if device is not None and pairwise:
        raise ValueError("timeshift_isc: the device path is "
                         "leave-one-out only; use device=None with "
                         "pairwise=True")
    data, n_TRs, n_voxels, n_subjects = _check_timeseries_input(data)
    if observed is None:
        observed = isc(data, pairwise=pairwise,
                       summary_statistic=summary_statistic,
                       tolerate_nans=tolerate_nans)
    else:
        observed = _check_observed(observed, n_voxels, n_subjects,
                                   pairwise, summary_statistic)
    rng = _as_rng(random_state)

    if device is not None:
        # one call draws what the numpy path's per-draw calls draw
        shifts = rng.randint(0, n_TRs, size=(n_shifts, n_subjects))
        distribution = _timeshift_null_device(
            data, shifts, summary_statistic, device)
        p = p_from_null(observed, distribution, side=side, exact=False,
                        axis=0)
        return observed, p, distribution

    def one_draw(_):
        shifts = rng.randint(0, n_TRs, size=n_subjects)
        rolled = np.dstack([np.roll(data[..., s], shifts[s], axis=0)
                            for s in range(n_subjects)])
        if pairwise:
            return isc(rolled, pairwise=True,
                       summary_statistic=summary_statistic,
                       tolerate_nans=tolerate_nans)
        return _loo_null_isc(rolled, data, summary_statistic,
                             tolerate_nans)

    return _null_from_resamples(data, observed, n_shifts, side, one_draw)


def phaseshift_isc(data, pairwise=False, summary_statistic='median',
                   n_shifts=1000, side='right', tolerate_nans=True,
                   random_state=None, device=None, observed=None):
    """FFT phase-randomization null distribution for an ISC test.

    ``device`` (``"cpu"``, ``"cuda"``, a ``torch.device``): compute the
    null distribution on that device from the same phase draws;
    ``None`` keeps the numpy path.  A phase-randomised subject keeps its
    mean and norm, so its correlation with a fixed series is linear in
    the cosines and sines of the drawn phases: the spectra are tabulated
    once (in voxel chunks) and every draw is a dot product with that
    table (``_phase_stat``), without a per-draw FFT.  Both leave-one-out
    and ``pairwise=True`` are supported; the observed statistic still
    comes from the host ``isc`` unless ``observed`` is given: an array
    of the shape that call returns (``ValueError`` otherwise), for
    instance the result of ``isc(data, ..., device="cuda")`` with the
    same ``pairwise``, ``summary_statistic`` and ``tolerate_nans``,
    which skips the host ISC, most of a device call's time.

    On the device path ``tolerate_nans`` acts as on the numpy path: with
    ``pairwise=True`` the voxels that its threshold drops are NaN in the
    distribution; for leave-one-out it cannot change the null, because a
    NaN in any subject makes every (plain) leave-one-out mean of that
    voxel NaN on either path.  A voxel that is constant in some subject
    is NaN on the device path (its unit-norm series is 0 / 0), where the
    numpy path correlates the rounding noise that the FFT round trip
    leaves in the surrogate.
    """
    data, n_TRs, n_voxels, n_subjects = _check_timeseries_input(data)
    if observed is None:
        observed = isc(data, pairwise=pairwise,
                       summary_statistic=summary_statistic,
                       tolerate_nans=tolerate_nans)
    else:
        observed = _check_observed(observed, n_voxels, n_subjects,
                                   pairwise, summary_statistic)
    rng = _as_rng(random_state)

    if device is not None:
        if summary_statistic not in ('mean', 'median'):
            raise ValueError("Summary statistic must be 'mean' or "
                             "'median'")
        if n_TRs < 2 or n_subjects < 2:
            raise ValueError("phaseshift_isc: the device path needs at "
                             "least 2 TRs and 2 subjects")
        # one call draws what the numpy path's per-draw
        # rand(F, 1, n_subjects) calls draw
        n_freq = (n_TRs - 1) // 2
        phases = rng.rand(n_shifts, n_freq, 1, n_subjects)[:, :, 0, :] \
            * 2 * np.pi
        distribution = _phaseshift_null_device(
            data, phases, pairwise, summary_statistic, device)
        if pairwise:
            _, keep = _drop_bad_voxels(data, tolerate_nans)
            distribution[:, ~keep] = np.nan
        p = p_from_null(observed, distribution, side=side, exact=False,
                        axis=0)
        return observed, p, distribution

    def one_draw(_):
        surrogate = phase_randomize(data, random_state=rng)
        if pairwise:
            return isc(surrogate, pairwise=True,
                       summary_statistic=summary_statistic,
                       tolerate_nans=tolerate_nans)
        return _loo_null_isc(surrogate, data, summary_statistic,
                             tolerate_nans)

    return _null_from_resamples(data, observed, n_shifts, side, one_draw)
