#!/usr/bin/env python3
"""Observed ISC: ``isc()`` at 50k voxels x 32 subjects x 200 TRs, fp64.
One step = one full public call (upload in voxel chunks, the correlation
kernels, the summary statistic if asked for, download).  Metric: voxels
per second (V / time).

``--path hip`` runs the correlations in the HIP kernels (k_isc_totals /
k_isc_loo / k_isc_pairwise), ``--path torch`` in their torch twin on the
same device (BRAINIAK_ISC_CORR=torch), ``--path numpy`` is the host path
(device=None): run that one with ``--steps 1 --warmup 0`` at the full
shape, it is the baseline.  ``--resident`` hands the call a tensor that
already is on the device.  The config block reports where the device call
spends its time: upload (chunk to device), kernels (correlations and the
summary statistic) and download."""

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
    ap.add_argument("--pairwise", action="store_true")
    ap.add_argument("--stat", choices=["none", "median", "mean"],
                    default="none")
    ap.add_argument("--path", choices=["hip", "torch", "numpy"],
                    default="hip")
    ap.add_argument("--resident", action="store_true",
                    help="the data is a tensor on the device already")
    args = ap.parse_args()

    if args.path == "torch":
        os.environ["BRAINIAK_ISC_CORR"] = "torch"
    else:
        os.environ.pop("BRAINIAK_ISC_CORR", None)

    rank, world, device, _ = dist_setup()
    from brainiak_amd import isc as isc_mod

    # on CPU smoke runs shrink the problem so it finishes in seconds
    on_gpu = device.type == "cuda"
    shrink = not on_gpu
    V = 512 if shrink else args.num_voxels
    subjects = 4 if shrink else args.subjects
    stat = None if args.stat == "none" else args.stat

    rng = np.random.RandomState(1234)
    data = rng.randn(args.trs, V, 1) + rng.randn(args.trs, V, subjects)
    data += 100.0                           # un-demeaned, as fMRI is
    dev_arg = None if args.path == "numpy" else device
    resident = args.resident and dev_arg is not None
    arg = torch.from_numpy(data).to(device) if resident else data

    # where the device call spends its time
    spent = {"upload": 0.0, "kernels": 0.0, "download": 0.0}

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

    isc_mod._isc_chunk_to_device = timed("upload",
                                         isc_mod._isc_chunk_to_device)
    isc_mod._isc_corr = timed("kernels", isc_mod._isc_corr)
    isc_mod._resample_stat = timed("kernels", isc_mod._resample_stat)
    isc_mod._isc_to_host = timed("download", isc_mod._isc_to_host)

    def step(i):
        if i == args.warmup:
            for k in spent:
                spent[k] = 0.0
        isc_mod.isc(arg, pairwise=args.pairwise, summary_statistic=stat,
                    device=dev_arg)

    elapsed = timed_steps(step, args.steps, args.warmup, world, device)
    emit(rank, "isc_voxels_per_sec", float(V) * args.steps / elapsed,
         "voxels/s", world, args.steps, args.warmup, elapsed, True,
         "none", "fp64",
         {"model": "isc_pairwise" if args.pairwise else "isc_leave_one_out",
          "path": args.path, "stat": args.stat, "num_voxels": V,
          "subjects": subjects, "trs": args.trs, "resident": resident,
          "upload_ms_per_step": spent["upload"] * 1000.0 / args.steps,
          "kernels_ms_per_step": spent["kernels"] * 1000.0 / args.steps,
          "download_ms_per_step": spent["download"] * 1000.0 / args.steps,
          "global_batch": V, "seq_len": args.trs,
          "parallelism": "single device"})
    teardown(world)


if __name__ == "__main__":
    main()
