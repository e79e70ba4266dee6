"""Hand-written HIP/CDNA4 (gfx950) kernels and their torch bindings.

This package owns every hot-path device kernel in the toolkit — the
MI355X equivalent of the reference's entire native layer
(ref src/brainiak/fcma/src/fcma_extension.cc, fcma/cython_blas.pyx,
factoranalysis/tfa_extension.cpp, eventseg/_utils.pyx):

 - ``fcma_normalize_``  — fused Fisher-z + within-subject z-score (N1)
 - ``fcma_correlate``   — MFMA bf16 batched epoch-correlation GEMM (N2)
 - ``fcma_gram``        — MFMA per-voxel [E,E] Gram / syrk (N3)
 - ``fcma_fused_gram``  — chunk pipeline; single-kernel for E=64/P=4
 - ``batched_polar``    — batched K×K Jacobi eigensolve → Procrustes
                          polar factor for SRM (srm.py:595-606 class)
 - ``tfa_factor`` / ``tfa_recon`` — TFA RBF factor matrix + residual
                          (N8/N9)
 - ``hmm_forward_backward`` — single-launch log-space forward-backward
                          over EventSegment's event chains (N10)
 - ``hmm_viterbi``      — single-launch MAP event path (Viterbi) over
                          the same chains (N10)
 - ``isc_resample_stat`` — per-draw gather + NaN-skipping median /
                          Fisher mean: the null distributions of the
                          ISC bootstrap, permutation and time-shift
                          tests
 - ``isc_phase_stat``   — per-draw contraction of a cos/sin coefficient
                          block with a fixed spectral table + the same
                          median / Fisher mean: the null distribution of
                          the ISC phase-randomisation test
 - ``isc_loo`` / ``isc_pairwise`` — the observed ISC itself: per-voxel
                          leave-one-out and pairwise correlations from
                          the [T, V, S] layout, NaN policy included
 - ``searchlight_gram`` — per-centre [E,E] Gram of a searchlight's
                          activity vectors (gather + exact-fp32 MFMA
                          syrk), the front end of the activity-based
                          voxel selector

Build: ``python setup.py build_ext --inplace`` (hipcc, gfx950) or
``__graft_entry__.build()``.  The extension is REQUIRED whenever CUDA
(=ROCm) devices are visible: a GPU box silently falling back to eager
torch would invalidate every benchmark, so ``has_hip`` raises instead of
returning False there (set BRAINIAK_AMD_ALLOW_NO_HIP=1 to override for
debugging).
"""

import os

import torch

__all__ = [
    "batched_polar",
    "polar_invsqrt",
    "require_hip",
    "fcma_correlate",
    "fcma_fused_gram",
    "fcma_gram",
    "fcma_normalize_",
    "has_fused_gram",
    "has_hip",
    "hmm_fb_tile",
    "hmm_forward_backward",
    "hmm_viterbi",
    "hmm_viterbi_tile",
    "isc_loo",
    "isc_pairwise",
    "isc_pairwise_max_subjects",
    "isc_phase_max_rows",
    "isc_phase_stat",
    "isc_resample_max_rows",
    "isc_resample_stat",
    "isfc_accum_",
    "searchlight_gram",
    "searchlight_gram_kernel",
    "searchlight_gram_max_e",
    "searchlight_gram_torch",
    "stencil3d",
    "load_extension",
    "masked_log",
    "tfa_factor",
    "tfa_recon",
]

_EXT = None
_TRIED = False


def load_extension():
    """Import the compiled in-tree extension (brainiak_amd/ops/_hip_ops.so).

    Returns the module or None (CPU-only environments).
    """
    global _EXT, _TRIED
    if _TRIED:
        return _EXT
    _TRIED = True
    try:
        from . import _hip_ops  # type: ignore
        _EXT = _hip_ops
    except ImportError:
        _EXT = None
    return _EXT


def has_hip() -> bool:
    """Pure capability probe: True iff the HIP extension is importable.
    Never raises — CPU-only estimator use on a GPU box must not abort
    just for probing."""
    return load_extension() is not None


def require_hip() -> bool:
    """Dispatch-site gate: call when a CUDA tensor is about to run
    through a HIP kernel.  True if the extension is loaded; raises if a
    GPU is visible but the extension is missing — silently falling back
    to eager torch there would invalidate every benchmark.  Set
    BRAINIAK_AMD_ALLOW_NO_HIP=1 to get the eager fallback for
    debugging."""
    if load_extension() is not None:
        return True
    if torch.cuda.is_available() and not os.environ.get(
            "BRAINIAK_AMD_ALLOW_NO_HIP"):
        raise RuntimeError(
            "brainiak_amd.ops._hip_ops is not built but a GPU tensor "
            "reached a HIP dispatch site. Run `python setup.py "
            "build_ext --inplace` (hipcc, gfx950); refusing to fall "
            "back to eager torch on the GPU path.")
    return False


def has_fused_gram() -> bool:
    ext = load_extension()
    return ext is not None and hasattr(ext, "fcma_fused_gram")


def _ext():
    ext = load_extension()
    if ext is None:
        raise RuntimeError("HIP extension not built")
    return ext


# ---------------------------------------------------------------------------
# FCMA pipeline kernels
# ---------------------------------------------------------------------------

def fcma_normalize_(corr: torch.Tensor, epochs_per_subj: int) -> torch.Tensor:
    """In-place Fisher-z + within-subject z-score of corr [C, E, V] fp32."""
    _ext().fcma_normalize_(corr, int(epochs_per_subj))
    return corr


def fcma_correlate(data: torch.Tensor, data2: torch.Tensor,
                   start: int, count: int) -> torch.Tensor:
    """corr [count, E, V2] fp32 from stacked epochs data/data2 [E, L, V]
    (bf16 only — fp32 inputs use the CorrelationPipeline torch
    fallback)."""
    return _ext().fcma_correlate(data, data2, int(start), int(count))


def fcma_gram(corr_norm: torch.Tensor) -> torch.Tensor:
    """Per-voxel Gram [C, E, E] fp32 of corr_norm [C, E, V] fp32."""
    return _ext().fcma_gram(corr_norm)


def fcma_gram_fp8(Z: torch.Tensor) -> torch.Tensor:
    """Per-voxel Gram [C, E, E] fp32 of Z [C, E, V] float8_e4m3fn
    (E % 64 == 0, V % 16 == 0 — host pads both)."""
    return _ext().fcma_gram_fp8(Z)


def fcma_gram_bf16(Z: torch.Tensor, norm_P: int = 0) -> torch.Tensor:
    """Per-voxel Gram [C, E, E] fp32 of Z [C, E, V] bf16 (E % 64 == 0).

    norm_P in {2, 4}: Z holds RAW correlations; Fisher-z + the
    within-subject z-score over norm_P epochs are applied to each
    staged tile in LDS before the MFMAs (the corr kernel then skips
    its normalize epilogue — see CorrelationPipeline)."""
    return _ext().fcma_gram_bf16(Z, int(norm_P))


def fcma_fused_gram(data: torch.Tensor, data2: torch.Tensor, start: int,
                    count: int, epochs_per_subj: int) -> torch.Tensor:
    """Correlate→normalize→Gram for one voxel chunk.  On the single-
    kernel path (E=64, P=4 — see ``fcma_fused_gram_native``) the
    [C, E, V] intermediate never touches HBM; other shapes run the
    two-kernel corr_norm_z + gram_bf16 composite."""
    return _ext().fcma_fused_gram(data, data2, int(start), int(count),
                                  int(epochs_per_subj))


def fcma_corr_gram_fused_supported(E: int, P: int, L: int) -> bool:
    """True when ``fcma_corr_gram_fused`` covers E epochs, P epochs per
    subject and epoch length L (E <= 64, P in {2, 4})."""
    return bool(_ext().fcma_corr_gram_fused_supported(int(E), int(P),
                                                      int(L)))


def fcma_fused_operand(data: torch.Tensor) -> torch.Tensor:
    """Time-contiguous operand [64, V, LP] bf16 of stacked epochs
    data [E, L, V]: epoch rows past E and time steps past L are zero.
    The single-kernel ``fcma_corr_gram_fused`` reads both of its inputs
    in this layout; build it once per data set."""
    E, L, V = data.shape
    LP = int(_ext().fcma_corr_gram_fused_lp(int(L)))
    out = torch.zeros((64, V, LP), dtype=torch.bfloat16,
                      device=data.device)
    out[:E, :, :L] = data.permute(0, 2, 1)
    return out


def fcma_corr_gram_fused(At_all: torch.Tensor, B_t: torch.Tensor,
                         start: int, count: int, epochs_per_subj: int,
                         nsplit: int = 1, shrink: bool = True,
                         clamp: str = "auto",
                         schedule: str = "auto",
                         fisher: str = "auto") -> torch.Tensor:
    """Correlation + normalize + Gram in one kernel over the operands of
    ``fcma_fused_operand``: [count, 64, 64] fp32 Grams of selected voxels
    [start, start+count) of At_all against every column of B_t, with the
    [count, E, V] intermediate kept on chip.

    The operands must be finite (``stack_epochs`` zero-pads, callers
    z-score with a clamped std).  ``clamp="auto"`` applies the Fisher-z
    clamp only where a correlation reaches |r| >= 1; ``clamp="always"``
    applies it to every element.  Both give the same bits.

    ``schedule="ahead"`` issues each task's correlation MFMAs one task
    before its normalize, with the column prefetch two tasks deep;
    ``"phased"`` issues them at the head of the task itself, the order
    the kernel was first shipped with; ``"auto"`` (the default) is
    ``"ahead"``.  Epoch lengths above 32 have no ``"ahead"`` form
    (``fcma_corr_gram_fused_ahead``) and run phased whatever is asked.
    All give the same bits.

    ``fisher="table"`` takes the Fisher z of a bf16-rounded correlation
    from a table that every workgroup builds in LDS with the log path's
    own arithmetic; ``"log"`` computes it with ``v_log_f32``; ``"auto"``
    (the default) is the table where the instance has one
    (``fcma_corr_gram_fused_table``: epoch lengths up to 32) and
    ``clamp`` is ``"auto"``, the logs elsewhere.  ``"table"`` where there
    is none is an error.  Both give the same bits."""
    return _ext().fcma_corr_gram_fused(At_all, B_t, int(start), int(count),
                                       int(epochs_per_subj), int(nsplit),
                                       bool(shrink), str(clamp),
                                       str(schedule), str(fisher))


def fcma_corr_gram_fused_table(P: int, L: int) -> bool:
    """True when the ``fcma_corr_gram_fused`` instance for P epochs per
    subject and epoch length L has a Fisher-z table."""
    return bool(_ext().fcma_corr_gram_fused_table(int(P), int(L)))


def fcma_fused_image_layout(P: int):
    """Tests only: the layout of ``fcma_corr_gram_fused``'s z image in
    LDS for P epochs per subject, from the address functions the kernel
    runs, evaluated on the host (no launch).  Returns ``(stride,
    image_bytes, table_bytes, store, read)``: the bytes from one voxel to
    the next, the bytes of one image (two lie back to back, behind
    ``table_bytes`` of Fisher table in the table instances), the int32
    byte offsets ``store[wave, si, st, p, lane]`` of every 8-byte
    ``ds_write_b64`` and ``read[voxel, band, lane]`` of every 16-byte
    ``ds_read_b128`` of the Gram."""
    return _ext().fcma_fused_image_layout(int(P))


def fcma_corr_gram_fused_ahead(P: int, L: int) -> bool:
    """True when the ``fcma_corr_gram_fused`` instance for P epochs per
    subject and epoch length L has the ``"ahead"`` schedule."""
    return bool(_ext().fcma_corr_gram_fused_ahead(int(P), int(L)))


# ---------------------------------------------------------------------------
# SRM Procrustes
# ---------------------------------------------------------------------------

def isfc_fused_(acc: torch.Tensor, Zs: torch.Tensor,
                Zm: torch.Tensor) -> torch.Tensor:
    """acc += per-subject atanh(sym(Zs_b @ Zm_b^T)) with the [V, V]
    correlation matrices never materialized (bf16 MFMA tile pairs,
    fp32 accumulation).  Zs/Zm: bf16 [B, V, T] unit rows."""
    return _ext().isfc_fused_(acc, Zs, Zm)


def svm_cv(kernels: torch.Tensor, y: torch.Tensor, train_idx, test_idx,
           n_train, n_test, C: float = 1.0, tol: float = 1e-3,
           max_iter: int = 10000, max_n: int = -1,
           variant: str = "auto") -> torch.Tensor:
    """Batched precomputed-kernel SVC k-fold CV fully on device.

    One wavefront per (voxel, fold) dual QP (SMO, WSS1); returns
    correct-prediction counts [C, F] int32.  n_train/n_test <= 128.
    max_n > 0 skips the fold-size .item() sync (pass
    max(n_train.max(), n_test.max()) computed on the host) so the
    launch can be enqueued on a side stream without draining it.

    variant: ``"shared"`` runs one workgroup per voxel whose fold-waves
    share one staged [E, E] tile (E <= 128 and the tile within 64 KB of
    LDS; raises otherwise), ``"wave"`` one single-wave workgroup per
    (voxel, fold) with its own Q tile, ``"auto"`` the shared kernel
    wherever it fits.  The two give identical counts.
    """
    return _ext().svm_cv(kernels, y, train_idx, test_idx, n_train, n_test,
                         float(C), float(tol), int(max_iter), int(max_n),
                         str(variant))


def svm_cv_trace(kernels: torch.Tensor, y: torch.Tensor, train_idx,
                 test_idx, n_train, n_test, C: float = 1.0,
                 tol: float = 1e-3, max_iter: int = 10000, max_n: int = -1,
                 variant: str = "auto"):
    """``svm_cv`` through the trace instantiations of its kernels, for
    tests: same arguments, returns ``(correct, dec, n_iter)``.

    dec [C, F, E] fp32: the decision value of test sample v of fold f,
    the number the kernel compares with 0 (slots past n_test[f] are 0).
    n_iter [C, F] int32: SMO iterations run before the gap fell under
    tol, or max_iter when it never did.  ``correct`` equals ``svm_cv``'s.
    """
    correct, dec, n_iter = _ext().svm_cv_trace(
        kernels, y, train_idx, test_idx, n_train, n_test, float(C),
        float(tol), int(max_iter), int(max_n), str(variant))
    return correct, dec, n_iter


def jacobi_eigh(G: torch.Tensor):
    """Batched symmetric eigensolve of G [B, K, K] (K <= 64) → (evals,
    evecs), one wavefront per matrix."""
    return _ext().jacobi_eigh(G)


def polar_invsqrt(G: torch.Tensor) -> torch.Tensor:
    """G^{-1/2} [B, K, K] for a stack of SPD Gram matrices (batched
    one-workgroup Jacobi eigensolve; K <= 64).  The ragged-batch
    Procrustes building block: callers keep per-subject [V_i, K] GEMMs
    and batch only the K x K eigensolves."""
    return _ext().polar_invsqrt(G)


def batched_polar(A: torch.Tensor, perturb: float = 0.001) -> torch.Tensor:
    """Batched orthogonal Procrustes factor of A [B, V, K] → [B, V, K].

    W_b = U_b V_b^T computed as A (A^T A)^{-1/2} with a one-workgroup
    Jacobi eigensolver per K×K Gram matrix on device.
    """
    return _ext().batched_polar(A, float(perturb))


# ---------------------------------------------------------------------------
# TFA kernels (N8/N9)
# ---------------------------------------------------------------------------

def tfa_factor(centers: torch.Tensor, widths: torch.Tensor,
               coords: torch.Tensor) -> torch.Tensor:
    """RBF factor matrix F[v, k] = exp(-||coords_v - centers_k||² / widths_k)."""
    return _ext().tfa_factor(centers, widths, coords)


def tfa_recon(X: torch.Tensor, W: torch.Tensor, F: torch.Tensor,
              scale: float) -> torch.Tensor:
    """Flattened residual scale*(X - F·W) for TFA least-squares."""
    return _ext().tfa_recon(X, W, F, float(scale))


# ---------------------------------------------------------------------------
# EventSegment forward-backward and MAP path (N10)
# ---------------------------------------------------------------------------

def hmm_forward_backward(logprob: torch.Tensor, log_start: torch.Tensor,
                         log_end: torch.Tensor, log_self: torch.Tensor,
                         log_adv: torch.Tensor, pred: torch.Tensor,
                         succ: torch.Tensor):
    """Log-space HMM forward-backward over left-to-right event chains in
    one launch (one wavefront per sequence, lane k = event k; K <= 64).

    logprob [B, T, K] fp64 observation log-probabilities; log_start /
    log_end fp64 with at least K entries (a trailing sink entry is
    ignored); log_self / log_adv fp64 [K] (self-loop and advance
    log-probabilities); pred / succ int32 [K] (previous / next member of
    k's chain, -1 at a chain head / tail).  All on the GPU.

    Returns (log_gamma [B, T, K] row-normalized log posteriors, ll [B]).
    """
    lg, ll = _ext().hmm_forward_backward(logprob, log_start, log_end,
                                         log_self, log_adv, pred, succ)
    return lg, ll


def hmm_fb_tile() -> int:
    """Timesteps per streamed tile of the forward-backward kernel (the
    sizes around which its tile-tail paths switch)."""
    return int(_ext().hmm_fb_tile())


def hmm_viterbi(logprob: torch.Tensor, log_start: torch.Tensor,
                log_end: torch.Tensor, log_self: torch.Tensor,
                log_adv: torch.Tensor, pred: torch.Tensor,
                succ: torch.Tensor):
    """MAP state path (Viterbi) over left-to-right event chains in one
    launch; same layout and arguments as ``hmm_forward_backward``.

    Max-plus recursion in fp64 additions and comparisons only: a state
    advances from ``pred[k]`` only when that is strictly better than its
    self loop, and the final state is the lowest k at the maximum of
    ``d[T-1] + log_end``.  Bit-identical to the torch recursion of
    ``EventSegment._viterbi_batch``.

    Returns (path [B, T] int32, score [B] fp64 joint log-probability of
    that path; -inf when no path fits a chain into T steps, which only
    chain vectors built for a longer sequence allow).
    """
    path, score = _ext().hmm_viterbi(logprob, log_start, log_end,
                                     log_self, log_adv, pred, succ)
    return path, score


def hmm_viterbi_tile() -> int:
    """Timesteps per backtrace tile of the Viterbi kernel (its forward
    pass streams ``logprob`` in ``hmm_fb_tile()`` steps)."""
    return int(_ext().hmm_viterbi_tile())


# ---------------------------------------------------------------------------
# ISC resampling statistics
# ---------------------------------------------------------------------------

def isc_resample_stat(table: torch.Tensor, rows: torch.Tensor, lags,
                      signs: torch.Tensor, stat: str) -> torch.Tensor:
    """Per-draw gather and summary statistic in one launch (one lane per
    voxel, one wave per 64 voxels of a draw).

    table fp64 [N, L, V] contiguous; rows int32 [I, R] into N; lags
    int32 [I, R] into L or None (all zero); signs int8 [I, R]: +1 / -1
    multiply the value, 0 leaves the entry out; all on the GPU.  The
    index ranges are NOT checked here (``isc._resample_stat`` checks
    them on the host).

    out[i, v] = stat over the r with signs[i, r] != 0 and a non-NaN
    signs[i, r] * table[rows[i, r], lags[i, r], v]: 'median' is numpy's
    nanmedian, 'mean' is tanh(mean(atanh(x))); NaN when nothing
    survives.  'median' needs R <= ``isc_resample_max_rows()``.

    Returns out [I, V] fp64.
    """
    return _ext().isc_resample_stat(table, rows, lags, signs, str(stat))


def isc_resample_max_rows() -> int:
    """Largest R the 'median' path of ``isc_resample_stat`` takes (its
    per-lane sorted column lives in LDS)."""
    return int(_ext().isc_resample_max_rows())


def isc_phase_stat(table: torch.Tensor, coef: torch.Tensor,
                   stat: str) -> torch.Tensor:
    """Contraction and summary statistic of the phase-randomisation null
    in one launch (one lane per voxel, one wave per 64 voxels of a small
    tile of draws); the [I, R, V] intermediate stays in registers.

    table fp64 [R, K, V] contiguous; coef fp64 [I, R, K] contiguous;
    both on the same GPU, R >= 1, K >= 1.

    x[i, r, v] = sum_k coef[i, r, k] * table[r, k, v], and out[i, v] is
    the statistic over the r with a non-NaN x: 'median' is numpy's
    nanmedian, 'mean' is tanh(mean(atanh(x))) with NaN atanh results
    skipped and infinities kept; NaN when nothing survives.  A NaN in
    the table reaches x through the product.  'median' needs
    R <= ``isc_phase_max_rows()``.

    Returns out [I, V] fp64.
    """
    return _ext().isc_phase_stat(table, coef, str(stat))


def isc_phase_max_rows() -> int:
    """Largest R the 'median' path of ``isc_phase_stat`` takes (its
    per-lane sorted columns live in LDS)."""
    return int(_ext().isc_phase_max_rows())


# ---------------------------------------------------------------------------
# observed ISC
# ---------------------------------------------------------------------------

def isc_loo(data: torch.Tensor, tolerant: bool, min_clean: float = -1.0,
            v0: int = 0, nv: int = -1) -> torch.Tensor:
    """Leave-one-out ISC of every voxel of a window of the data, from the
    caller's layout (no transposed copy): ``k_isc_totals`` (sums over
    the subjects), ``k_isc_loo`` (one thread per voxel and subject, a
    centred two-pass correlation) and ``k_isc_drop`` (the voxel policy).

    data fp64 [T, V, S] contiguous on the GPU, T >= 1, S >= 2.  The
    window is the voxels [v0, v0 + nv) (``nv = -1``: up to V); it is
    addressed in place.  ``tolerant``: the leave-one-out mean skips
    NaNs (``np.nanmean``) instead of propagating them.  A voxel whose
    subjects all have a NaN somewhere, or that has fewer than
    ``min_clean`` NaN-free subjects (``min_clean < 0``: no threshold),
    is NaN in every row.

    Returns r [S, nv] fp64: r[s, v] is the correlation of subject s with
    the mean of the others.
    """
    return _ext().isc_loo(data, bool(tolerant), float(min_clean), int(v0),
                          int(nv))


def isc_pairwise(data: torch.Tensor, min_clean: float = -1.0, v0: int = 0,
                 nv: int = -1) -> torch.Tensor:
    """Pairwise ISC of every voxel of a window of the data
    (``k_isc_pairwise``: a block stages time slabs of a few voxels in
    LDS, a thread holds a 4 x 4 tile of a voxel's centred Gram; then
    ``k_isc_drop``).

    data, the window and ``min_clean`` as in ``isc_loo``;
    S <= ``isc_pairwise_max_subjects()``.

    Returns r [S (S - 1) / 2, nv] fp64, pairs in ``combinations`` order
    (row-major upper triangle).
    """
    return _ext().isc_pairwise(data, float(min_clean), int(v0), int(nv))


def isc_pairwise_max_subjects() -> int:
    """Largest S ``isc_pairwise`` takes (a voxel's Gram tiles fill one
    block)."""
    return int(_ext().isc_pairwise_max_subjects())


# ---------------------------------------------------------------------------
# small helpers
# ---------------------------------------------------------------------------

def stencil3d(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """Valid [K,K,K] stencil over [B,X,Y,Z] fp32 (K odd, <= 9) — the
    searchlight ball aggregation without MIOpen's im2col detour."""
    return _ext().stencil3d(x, w)


# ---------------------------------------------------------------------------
# activity-based searchlight Gram
# ---------------------------------------------------------------------------

# bytes of gathered rows the torch twin holds per chunk of centres
_SL_GRAM_TWIN_BYTES = 1 << 28


def searchlight_gram_max_e() -> int:
    """Largest epoch count E that ``searchlight_gram_kernel`` takes (its
    upper-triangular tile accumulators live in registers)."""
    return int(_ext().searchlight_gram_max_e())


def searchlight_gram_kernel(x: torch.Tensor, mask: torch.Tensor,
                            shape: torch.Tensor,
                            centres: torch.Tensor) -> torch.Tensor:
    """The HIP kernel behind ``searchlight_gram`` (one workgroup per
    centre, exact-fp32 MFMA).  x fp32 [B, X, Y, Z, E], mask uint8
    [B, X, Y, Z], shape uint8 [K, K, K], centres int64 [N]; all
    contiguous on one GPU, E <= ``searchlight_gram_max_e()``.  Centre
    positions are NOT checked here."""
    return _ext().searchlight_gram(x, mask, shape, centres)


def searchlight_gram_torch(x: torch.Tensor, mask: torch.Tensor,
                           shape: torch.Tensor,
                           centres: torch.Tensor) -> torch.Tensor:
    """Torch twin of ``searchlight_gram_kernel``: gathers each centre's
    K^3 neighbourhood (the offsets the shape keeps), zeroes the rows the
    mask drops and runs one ``bmm`` per chunk of centres.  Works in fp64
    on CPU tensors and in fp32 on the GPU; returns fp32 [N, E, E] with
    the lower triangle mirrored from the upper."""
    B, X, Y, Z, E = x.shape
    K = shape.shape[0]
    rad = K // 2
    dev = x.device
    work = torch.float32 if x.is_cuda else torch.float64
    ar = torch.arange(K, device=dev) - rad
    rel = ((ar[:, None, None] * Y + ar[None, :, None]) * Z
           + ar[None, None, :]).reshape(-1)
    rel = rel[shape.reshape(-1).to(torch.bool)]
    rows = x.reshape(-1, E)
    live = mask.reshape(-1).to(torch.bool)
    N = centres.shape[0]
    out = torch.empty((N, E, E), dtype=torch.float32, device=dev)
    per_centre = max(1, rel.numel()) * E * (4 if x.is_cuda else 8)
    step = max(1, _SL_GRAM_TWIN_BYTES // per_centre)
    for lo in range(0, N, step):
        idx = centres[lo:lo + step, None] + rel[None, :]
        a = rows[idx].to(work)
        a = torch.where(live[idx][:, :, None], a, torch.zeros_like(a))
        g = torch.bmm(a.transpose(1, 2), a)
        g = torch.triu(g) + torch.triu(g, 1).transpose(1, 2)
        out[lo:lo + step] = g.to(torch.float32)
    return out


def searchlight_gram(x: torch.Tensor, mask: torch.Tensor,
                     shape: torch.Tensor,
                     centres: torch.Tensor) -> torch.Tensor:
    """Gram matrices of the activity vectors of a list of searchlights:

        G[n, e, f] = sum over v in shape(c_n) & mask of x[v, e] * x[v, f]

    x [B, X, Y, Z, E] fp32 halo-padded block stack (epoch innermost);
    mask [B, X, Y, Z] bool or uint8; shape [K, K, K] bool or uint8 with
    K = 2 rad + 1 odd and at most 9; centres [N] int64 linear indices of
    the centre voxels in [B, X, Y, Z].  Returns G [N, E, E] fp32 with
    G == G^T bit for bit.

    Raises ValueError for a shape that is not such a cube and for a
    centre that is out of range or within rad of a block face.  GPU
    tensors with E <= ``searchlight_gram_max_e()`` run the HIP kernel;
    everything else, and everything under ``BRAINIAK_SL_GRAM=torch``,
    runs ``searchlight_gram_torch``.
    """
    if x.dim() != 5 or mask.shape != x.shape[:4]:
        raise ValueError("x must be [B, X, Y, Z, E] and mask [B, X, Y, Z]")
    K = shape.shape[0] if shape.dim() == 3 else 0
    if K == 0 or tuple(shape.shape) != (K, K, K) or K % 2 == 0 or K > 9:
        raise ValueError("shape must be a [K, K, K] cube with odd K <= 9")
    B, X, Y, Z, E = x.shape
    rad = K // 2
    if centres.dim() != 1:
        raise ValueError("centres must be a 1-D index list")
    centres = centres.to(device=x.device, dtype=torch.int64).contiguous()
    if centres.numel():
        k = centres % Z
        j = (centres // Z) % Y
        i = (centres // (Y * Z)) % X
        bad = (centres < 0) | (centres >= B * X * Y * Z)
        for pos, edge in ((i, X), (j, Y), (k, Z)):
            bad |= (pos < rad) | (pos >= edge - rad)
        if bool(bad.any()):
            raise ValueError(
                "searchlight centre out of range or within the radius "
                "of a block face")
    mask = mask.to(torch.uint8)
    shape = shape.to(device=x.device, dtype=torch.uint8)
    if (x.is_cuda and os.environ.get("BRAINIAK_SL_GRAM") != "torch"
            and require_hip() and E <= searchlight_gram_max_e()):
        return searchlight_gram_kernel(
            x.to(torch.float32).contiguous(), mask.contiguous(),
            shape.contiguous(), centres)
    return searchlight_gram_torch(x, mask, shape, centres)


def isfc_accum_(acc: torch.Tensor, M: torch.Tensor) -> torch.Tensor:
    """In-place acc += atanh(clamp((M + M^T)/2, +-(1-1e-7))) — the ISFC
    Fisher-mean accumulation fused into one HBM pass.  M may be a
    [B, V, V] subject stack: the batch streams through while the acc
    tile loads/stores once."""
    return _ext().isfc_accum_(acc, M)


def masked_log(x: torch.Tensor) -> torch.Tensor:
    """log(x) with x <= 0 → -inf (ref eventseg/_utils.pyx:27-54).

    Pure torch on both CPU and GPU — elementwise, never a bottleneck.
    """
    return torch.where(x > 0, torch.log(x.clamp_min(1e-300)),
                       torch.full_like(x, float("-inf")))
