#!/usr/bin/env python3
"""ISC phase-randomisation null distribution: ``phaseshift_isc`` at 50k
voxels x 32 subjects x 200 TRs with 1000 shifts, leave-one-out or
``--pairwise``.  One step = one full public call (host ISC of the observed
data, upload, spectral tables in voxel chunks, the per-draw contraction +
summary statistic, download, p-values).  Metric: null values per second
(n_shifts * V / time).

``--path hip`` runs the contraction + statistic in the HIP kernel
(k_isc_phase_stat), ``--path torch`` in its torch twin on the same device
(BRAINIAK_ISC_RESAMPLE=torch: a batched matmul, then the statistic),
``--path numpy`` is the host path (device=None) — give that one a small
shape, it takes an FFT pair of the whole array per draw.  The config block
also reports the time spent inside the null construction and inside the
contraction + statistic step (``_phase_stat``) alone.  With ``--pairwise``
the table has subjects * (subjects - 1) / 2 rows: 'median' stays on the
kernel up to ``ops.isc_phase_max_rows()`` rows (16 subjects)."""

import argparse
import os
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from benchmarks.common import dist_setup, emit, teardown, timed_steps  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--num-voxels", type=int, default=50000)
    ap.add_argument("--subjects", type=int, default=32)
    ap.add_argument("--trs", type=int, default=200)
    ap.add_argument("--shifts", type=int, default=1000)
    ap.add_argument("--stat", choices=["median", "mean"], default="median")
    ap.add_argument("--path", choices=["hip", "torch", "numpy"],
                    default="hip")
    ap.add_argument("--pairwise", action="store_true")
    args = ap.parse_args()

    if args.path == "torch":
        os.environ["BRAINIAK_ISC_RESAMPLE"] = "torch"
    else:
        os.environ.pop("BRAINIAK_ISC_RESAMPLE", None)

    rank, world, device, _ = dist_setup()
    from brainiak_amd import isc as isc_mod

    # on CPU smoke runs shrink the problem so it finishes in seconds
    on_gpu = device.type == "cuda"
    shrink = not on_gpu and args.path != "numpy"
    V = 512 if shrink else args.num_voxels
    subjects = 4 if shrink else args.subjects
    shifts = 20 if shrink else args.shifts

    rng = np.random.RandomState(1234)
    data = rng.randn(args.trs, V, 1) \
        + rng.randn(args.trs, V, subjects)

    # where the step spends its time: the null construction, and the
    # contraction + statistic inside it
    spent = {"null": 0.0, "phase_stat": 0.0}

    def timed(name, fn, sync):
        def wrapper(*a, **kw):
            if sync and on_gpu:
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **kw)
            if sync and on_gpu:
                torch.cuda.synchronize()
            spent[name] += time.perf_counter() - t0
            return out
        return wrapper

    isc_mod._phase_stat = timed("phase_stat", isc_mod._phase_stat, True)
    isc_mod._phaseshift_null_device = timed(
        "null", isc_mod._phaseshift_null_device, False)

    dev_arg = None if args.path == "numpy" else device

    def step(i):
        if i == args.warmup:
            spent["null"] = spent["phase_stat"] = 0.0
        isc_mod.phaseshift_isc(data, pairwise=args.pairwise,
                               summary_statistic=args.stat,
                               n_shifts=shifts, random_state=i,
                               device=dev_arg)

    elapsed = timed_steps(step, args.steps, args.warmup, world, device)
    values_per_sec = float(shifts) * V * args.steps / elapsed
    emit(rank, "isc_phaseshift_null_values_per_sec", values_per_sec,
         "values/s", world, args.steps, args.warmup, elapsed, True,
         "none", "fp64",
         {"model": "phaseshift_isc_pairwise" if args.pairwise
          else "phaseshift_isc_leave_one_out", "path": args.path,
          "stat": args.stat, "num_voxels": V, "subjects": subjects,
          "trs": args.trs, "n_shifts": shifts,
          "null_ms_per_step": spent["null"] * 1000.0 / args.steps,
          "phase_stat_ms_per_step":
              spent["phase_stat"] * 1000.0 / args.steps,
          "global_batch": shifts, "seq_len": args.trs,
          "parallelism": "single device"})
    teardown(world)


if __name__ == "__main__":
    main()
