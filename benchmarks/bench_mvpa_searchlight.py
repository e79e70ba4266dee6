#!/usr/bin/env python3
"""Activity-based voxel selection: ``MVPAVoxelSelector.run(device=...)``
on a whole-brain searchlight — 91x109x91 volume, synthetic ellipsoid
mask, radius-3 Ball, 64 epochs (16 subjects x 4), linear SVC, 4 folds.
One step = one full public call (block decomposition on the host, upload,
per-centre Gram matrices, batched cross-validation, stitch).  Metric:
searchlight centres per second.

The config block also reports
 - the time spent per step inside the Gram stage and inside the CV stage;
 - the Gram stage ALONE on the largest block stack, through the HIP
   kernel (k_sl_gram) and through its torch twin on the same device,
   alternating after warm-up and timed with device events, with the
   kernel's achieved bytes/s and FLOP/s from shapes over kernel time;
 - the host path (device=None: one sklearn fit per fold and centre) timed
   on a fixed seeded SAMPLE of centres at the same shape, labelled as
   such; a whole-brain host run is hours."""

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from benchmarks.common import dist_setup, emit, teardown, timed_steps  # noqa: E402

# MI355X peaks the achieved rates are set against
HBM_PEAK_TBS = 8.0
F32_MFMA_PEAK_TFLOPS = 157.3


def ellipsoid_mask(dims, frac):
    axes = [np.linspace(-1.0, 1.0, d) for d in dims]
    gx, gy, gz = np.meshgrid(*axes, indexing="ij")
    return (gx ** 2 + gy ** 2 + gz ** 2) <= (2.0 * frac) ** 2


def gram_stage_alone(ops, sl, device, reps, max_centres):
    """Kernel and twin on the largest resident block stack, alternating;
    per-call milliseconds from device events."""
    idxs, stacks, mask_stack = max(sl._device_group_cache[1],
                                   key=lambda g: g[1][0].numel())
    x = stacks[0].to(torch.float32).contiguous()
    msk = mask_stack.to(torch.bool)
    rad = sl.sl_rad
    shape = torch.as_tensor(sl.shape, device=device)
    B, bx, by, bz = msk.shape
    E = x.shape[-1]
    inner = torch.zeros_like(msk)
    inner[:, rad:bx - rad, rad:by - rad, rad:bz - rad] = True
    centres = (inner & msk).reshape(-1).nonzero()[:, 0][:max_centres]
    centres = centres.contiguous()
    N = int(centres.numel())
    counts = ops.stencil3d(msk.float().contiguous(),
                           shape.float().contiguous())
    nv_total = float(counts[(inner & msk)[:, rad:bx - rad, rad:by - rad,
                                         rad:bz - rad]][:N].sum())
    mask_u8 = msk.to(torch.uint8)
    shape_u8 = shape.to(torch.uint8)

    def timed(fn):
        start = torch.cuda.Event(enable_timing=True)
        stop = torch.cuda.Event(enable_timing=True)
        start.record()
        out = fn(x, mask_u8, shape_u8, centres)
        stop.record()
        stop.synchronize()
        del out
        return start.elapsed_time(stop)

    for _ in range(2):
        timed(ops.searchlight_gram_kernel)
        timed(ops.searchlight_gram_torch)
    kernel_ms, twin_ms = [], []
    for _ in range(reps):
        kernel_ms.append(timed(ops.searchlight_gram_kernel))
        twin_ms.append(timed(ops.searchlight_gram_torch))
    k_med = float(np.median(kernel_ms))
    # what the kernel must move and compute: every in-light row read
    # once per centre, every Gram written once; the full E x E products
    nbytes = nv_total * E * 4 + N * E * E * 4
    flops = 2.0 * nv_total * E * E
    tbs = nbytes / (k_med * 1e-3) / 1e12
    tflops = flops / (k_med * 1e-3) / 1e12
    frac_bw = tbs / HBM_PEAK_TBS
    frac_fl = tflops / F32_MFMA_PEAK_TFLOPS
    return {
        "gram_block_stack": [int(B), int(bx), int(by), int(bz), int(E)],
        "gram_centres": N,
        "gram_mean_voxels_per_centre": nv_total / max(N, 1),
        "gram_kernel_ms": k_med,
        "gram_kernel_ms_min_max": [min(kernel_ms), max(kernel_ms)],
        "gram_twin_ms": float(np.median(twin_ms)),
        "gram_twin_ms_min_max": [min(twin_ms), max(twin_ms)],
        "gram_reps": reps,
        "gram_kernel_tbytes_per_s": tbs,
        "gram_kernel_tflops": tflops,
        "gram_kernel_fraction_of_hbm_peak": frac_bw,
        "gram_kernel_fraction_of_f32_mfma_peak": frac_fl,
        "gram_kernel_nearer_bound": "memory" if frac_bw >= frac_fl
        else "compute",
    }


def host_path_sample(data, mask, shape_mask, rad, labels, folds, clf,
                     n_sample):
    """``device=None`` statistic on a fixed seeded sample of centres."""
    from brainiak_amd.fcma.mvpa_voxelselector import _sl_accuracy
    inner = np.zeros_like(mask)
    inner[rad:-rad, rad:-rad, rad:-rad] = True
    cand = np.argwhere(inner & mask)
    pick = np.random.RandomState(7).choice(
        len(cand), size=min(n_sample, len(cand)), replace=False)
    t0 = time.perf_counter()
    for i, j, k in cand[pick]:
        sl = np.s_[i - rad:i + rad + 1, j - rad:j + rad + 1,
                   k - rad:k + rad + 1]
        _sl_accuracy([data[sl]], mask[sl] * shape_mask, rad,
                     (labels, folds, clf))
    return len(pick), time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dims", type=int, nargs=3, default=[91, 109, 91])
    ap.add_argument("--mask-frac", type=float, default=0.36,
                    help="ellipsoid semi-axes as a fraction of the dims")
    ap.add_argument("--rad", type=int, default=3)
    ap.add_argument("--subjects", type=int, default=16)
    ap.add_argument("--epochs-per-subj", type=int, default=4)
    ap.add_argument("--folds", type=int, default=4)
    ap.add_argument("--max-blk-edge", type=int, default=32)
    ap.add_argument("--gram-reps", type=int, default=7)
    ap.add_argument("--gram-centres", type=int, default=65536)
    ap.add_argument("--host-sample", type=int, default=2000)
    ap.add_argument("--out", default=None,
                    help="also write the result JSON to this file")
    args = ap.parse_args()

    rank, world, device, _ = dist_setup()
    from sklearn import svm

    from brainiak_amd import ops
    from brainiak_amd.fcma import mvpa_voxelselector as mvs_mod
    from brainiak_amd.fcma import svm as svm_mod
    from brainiak_amd.fcma.mvpa_voxelselector import MVPAVoxelSelector
    from brainiak_amd.searchlight import Ball, Searchlight

    on_gpu = device.type == "cuda"
    dims = tuple(args.dims) if on_gpu else (14, 16, 14)
    host_sample = args.host_sample if on_gpu else 50
    E = args.subjects * args.epochs_per_subj
    rad = args.rad

    rng = np.random.default_rng(1234)
    mask = ellipsoid_mask(dims, args.mask_frac)
    labels = np.array([e % 2 for e in range(E)])
    data = rng.standard_normal((*dims, E), dtype=np.float32)
    centre = tuple(d // 2 for d in dims)
    data[centre] += 3.0 * labels
    clf = svm.SVC(kernel='linear', shrinking=False, C=1)

    sl = Searchlight(sl_rad=rad, max_blk_edge=args.max_blk_edge,
                     shape=Ball, pool_size=1)
    mvs = MVPAVoxelSelector(data, mask, labels, args.folds, sl)

    spent = {"gram": 0.0, "cv": 0.0}

    def timed(name, fn):
        def wrapper(*a, **kw):
            if on_gpu:
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **kw)
            if on_gpu:
                torch.cuda.synchronize()
            spent[name] += time.perf_counter() - t0
            return out
        return wrapper

    real_gram = ops.searchlight_gram
    ops.searchlight_gram = timed("gram", real_gram)
    svm_mod.svm_cv_device = timed("cv", svm_mod.svm_cv_device)
    svm_mod.cross_validate_voxels = timed("cv",
                                          svm_mod.cross_validate_voxels)

    scored = {}

    def step(i):
        if i == args.warmup:
            spent["gram"] = spent["cv"] = 0.0
        volume, ranked = mvs.run(clf, device=device)
        scored["n"] = int((~np.isnan(volume.astype(np.float64))).sum())

    elapsed = timed_steps(step, args.steps, args.warmup, world, device)
    ops.searchlight_gram = real_gram
    n_centres = scored["n"]
    centres_per_sec = float(n_centres) * args.steps / elapsed

    config = {
        "model": "mvpa_voxelselector_linear_svc",
        "path": "hip" if on_gpu else "cpu",
        "dims": list(dims), "mask_voxels": int(mask.sum()),
        "centres": n_centres, "rad": rad, "shape": "Ball",
        "epochs": E, "folds": args.folds,
        "max_blk_edge": args.max_blk_edge,
        "gram_stage_ms_per_step": spent["gram"] * 1000.0 / args.steps,
        "cv_stage_ms_per_step": spent["cv"] * 1000.0 / args.steps,
        "gram_chunk_bytes": mvs_mod._GRAM_CHUNK_BYTES,
        "global_batch": n_centres, "seq_len": E,
        "parallelism": "single device",
    }
    if on_gpu:
        config.update(gram_stage_alone(ops, sl, device, args.gram_reps,
                                       args.gram_centres))
    if host_sample > 0:
        n, secs = host_path_sample(data, mask, sl.shape, rad, labels,
                                   args.folds, clf, host_sample)
        config["host_path_sampled_centres"] = n
        config["host_path_sample_seconds"] = secs
        config["host_path_sample_centres_per_sec"] = n / secs

    emit(rank, "mvpa_searchlight_centres_per_sec", centres_per_sec,
         "centres/s", world, args.steps, args.warmup, elapsed, True,
         "none", "fp32", config)
    if args.out and rank == 0:
        with open(args.out, "w") as fh:
            json.dump({"metric": "mvpa_searchlight_centres_per_sec",
                       "value": centres_per_sec, "unit": "centres/s",
                       "steps": args.steps, "warmup": args.warmup,
                       "ms_per_step": elapsed * 1000.0 / args.steps,
                       "config": config}, fh, indent=1)
            fh.write("\n")
    teardown(world)


if __name__ == "__main__":
    main()
