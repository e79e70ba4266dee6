#!/usr/bin/env python3
"""Flagship benchmark: FCMA voxel selection, whole-brain 34k voxels x 16
subjects, bf16 compute, on N MI355X GPUs (BASELINE.json config 2; the
driver's headline metric).

One *step* scores ``--voxels-per-step`` voxels PER GPU against all
``--num-voxels`` voxels: the full selection pipeline — fused HIP
correlation + Fisher-z normalization + per-voxel [E,E] SVM Gram
matrices (MFMA), then batched k-fold SVM cross-validation on device.
Per-GPU work is fixed as N grows (weak scaling): rank r scores its own
voxel slice, exactly how `VoxelSelector` shards whole-brain selection.

Metric: voxel-pairs/sec = (voxels_scored_per_step * num_voxels * N)
/ step_time, aggregated over the whole job.  Data is synthetic
(random-init, z-scored epochs of the named shape) — there is no network
for datasets; BASELINE.md documents that the reference publishes no
in-repo numbers, so `vs_baseline` is null.

Usage (driver contract):
    python bench.py --gpus N --steps K --warmup W
    torchrun --nproc-per-node N bench.py --gpus N ...   (N > 1)

A plain run sets up, warms up, times K steps and prints one JSON line;
``--dump-outputs DIR`` also saves what the last timed step computed,
and ``--full`` is the home of any secondary measurement (none today).
"""

import argparse
import json
import math
import os
import time

import numpy as np
import torch


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # defaults sized so the timed region is long enough for the
    # driver's gpu-busy sampling to land inside it (~2.6 s on MI355X
    # at the whole-brain step default)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--num-voxels", type=int, default=34470)
    ap.add_argument("--subjects", type=int, default=16)
    ap.add_argument("--epochs-per-subj", type=int, default=4)
    ap.add_argument("--epoch-len", type=int, default=12)
    ap.add_argument("--voxels-per-step", type=int, default=None,
                    help="default: the whole brain (--num-voxels) — one "
                         "step = one complete whole-brain selection "
                         "pass per GPU")
    ap.add_argument("--num-folds", type=int, default=4)
    ap.add_argument("--chunk", type=int, default=512,
                    help="pipeline chunk (voxels per kernel pass; "
                         "512 measured best on MI355X, profiles/)")
    ap.add_argument("--no-cv", action="store_true",
                    help="skip the SVM CV stage (pipeline only)")
    ap.add_argument("--fp8", action="store_true",
                    help="fp8(e4m3) Z tile between corr and Gram "
                         "(BRAINIAK_FP8=1 equivalent)")
    ap.add_argument("--device", default=None)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last "
                         "timed step computed to DIR/<name>.npy "
                         "(float32): accuracy.npy = per-voxel CV "
                         "accuracy [voxels_per_step]; with --no-cv "
                         "kernels.npy = the [n, E, E] Gram matrices "
                         "(a fixed seeded voxel sample when they "
                         "exceed 64 MB)")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beyond the headline "
                         "figure (secondary measurements and checks). "
                         "This benchmark currently has none, so the "
                         "flag changes nothing")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")
    return args


# 64 MB cap on everything --dump-outputs writes, with room for headers
DUMP_BUDGET_BYTES = 60 * 1000 * 1000


def dump_outputs(outputs, out_dir, rank):
    """Write {name: tensor/array} as float32 .npy files, at most
    DUMP_BUDGET_BYTES in all.  An oversized array is cut to a fixed
    seeded sample of its leading (voxel) axis, so two builds given the
    same arguments write the same rows."""
    os.makedirs(out_dir, exist_ok=True)
    budget = DUMP_BUDGET_BYTES // max(len(outputs), 1)
    for name, val in outputs.items():
        if not torch.is_tensor(val):
            val = torch.as_tensor(np.asarray(val))
        n = val.shape[0]
        row_bytes = 4 * max(val[0].numel(), 1)
        keep = budget // row_bytes
        if n > keep:
            idx = np.sort(np.random.default_rng(0).choice(
                n, size=keep, replace=False))
            val = val[torch.as_tensor(idx, device=val.device)]
        arr = val.detach().to(torch.float32).cpu().numpy()
        suffix = "" if rank == 0 else f".rank{rank}"
        np.save(os.path.join(out_dir, f"{name}{suffix}.npy"), arr)


def make_synthetic_epochs(rng, n_epochs, length, voxels, device):
    """Z-scored, 1/sqrt(n)-scaled epochs, generated on device."""
    g = torch.Generator(device="cpu").manual_seed(rng)
    out = []
    for _ in range(n_epochs):
        m = torch.randn((length, voxels), generator=g, dtype=torch.float32)
        m = m.to(device)
        m = (m - m.mean(dim=0)) / m.std(dim=0, unbiased=False).clamp_min(
            1e-12)
        out.append(m / math.sqrt(length))
    return out


def main():
    args = parse_args()
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    distributed = world > 1

    if torch.cuda.is_available():
        local_rank = int(os.environ.get("LOCAL_RANK", rank))
        device = torch.device("cuda", local_rank % torch.cuda.device_count())
        torch.cuda.set_device(device)
        backend = "nccl"
    else:  # CPU smoke path (no GPU in the dev container)
        device = torch.device("cpu")
        backend = "gloo"
    if args.device:
        device = torch.device(args.device)
        backend = "nccl" if device.type == "cuda" else "gloo"

    if distributed:
        import torch.distributed as dist
        dist.init_process_group(backend=backend)

    from brainiak_amd.fcma.core import CorrelationPipeline
    from brainiak_amd.fcma.svm import cross_validate_voxels

    E = args.subjects * args.epochs_per_subj
    V = args.num_voxels
    # epochs stacked directly on device; bf16 on GPU (BASELINE dtype)
    raw = make_synthetic_epochs(1234, E, args.epoch_len, V, device)
    labels = np.array([e % 2 for e in range(E)])
    pipeline = CorrelationPipeline(
        raw, None, args.epochs_per_subj, device=device,
        use_bf16=device.type == "cuda",
        z_fp8=args.fp8 if args.fp8 else None)
    del raw

    # overlapped CV: per-chunk SMO launches ride a side stream while
    # the duo sweep continues (same scheme as VoxelSelector.run)
    cv_plan = cv_stream = None
    if device.type == "cuda" and not args.no_cv             and pipeline._hip_path and pipeline._raw_split             and not os.environ.get("BRAINIAK_NO_DUO")             and not os.environ.get("BRAINIAK_NO_CV_OVERLAP"):
        from brainiak_amd.fcma.svm import FoldPlan, svm_cv_device
        cv_plan = FoldPlan(labels, args.num_folds, device)
        cv_stream = torch.cuda.Stream(
            device=device,
            priority=int(os.environ.get("BRAINIAK_CV_PRIO", "0")))

    # this rank's voxel range rotates so steps touch different voxels
    vps = min(args.voxels_per_step or V, V)
    chunk = min(args.chunk, vps)
    if device.type != "cuda":
        # CPU smoke path: the fp32 correlation chunk is [chunk, E, V]
        # (9 GB at the GPU defaults) — keep host invocations sane
        vps = min(vps, 256)
        chunk = min(chunk, 128)

    last = {}    # --dump-outputs: what the final timed step computed

    def one_step(step_idx, keep=False):
        # rank-interleaved rotation: ranks score disjoint voxel ranges
        # each step, exactly how VoxelSelector shards a whole-brain run
        start0 = ((step_idx * world + rank) * vps) % V
        chunks = []
        done = 0
        while done < vps:
            count = min(chunk, vps - done)
            start = (start0 + done) % V
            count = min(count, V - start)
            chunks.append((start, count))
            done += count
        if cv_plan is not None:
            cv_tol = 1e-2 if args.fp8 else 1e-3
            accs = []

            def consume(g, start, count):
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(device))
                with torch.cuda.stream(cv_stream):
                    cv_stream.wait_event(ev)
                    accs.append(svm_cv_device(g, cv_plan, 1.0, cv_tol))
                    g.record_stream(cv_stream)

            pipeline._duo_pipeline(chunks, consumer=consume)
            torch.cuda.current_stream(device).wait_stream(cv_stream)
            acc = torch.cat(accs)
            if keep:
                last["accuracy"] = acc
            return float(acc.mean().cpu())
        kernels = pipeline.pipelined_kernel_matrices(chunks)
        if not args.no_cv:
            if device.type == "cuda":
                # fp8 Z: the SMO's KKT gap cannot fall below the e4m3
                # quantization noise floor; tol 1e-2 matches it
                # (measured: accuracy churn == bf16@1e-2, CV 0.45 ms
                # vs 55 ms grinding at 1e-3 — profiles/fp8.md)
                accs = cross_validate_voxels(
                    kernels, labels, args.num_folds,
                    tol=1e-2 if args.fp8 else 1e-3)
            else:  # CPU smoke: tiny sklearn sample to keep runtime sane
                accs = cross_validate_voxels(kernels[:8], labels,
                                             args.num_folds)
            if keep:
                last["accuracy"] = accs
            return float(np.mean(accs))
        if keep:
            last["kernels"] = kernels
        return float(kernels[0].float().mean())

    def barrier_sync():
        if distributed:
            import torch.distributed as dist
            dist.barrier()
        if device.type == "cuda":
            torch.cuda.synchronize(device)

    for w in range(args.warmup):
        one_step(w)
    barrier_sync()

    t0 = time.perf_counter()
    sink = 0.0
    for k in range(args.steps):
        sink += one_step(args.warmup + k,
                         keep=bool(args.dump_outputs)
                         and k == args.steps - 1)
    barrier_sync()
    elapsed = time.perf_counter() - t0

    # MAX over ranks
    if distributed:
        import torch.distributed as dist
        t = torch.tensor([elapsed], dtype=torch.float64,
                         device=device if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t[0])

    if args.dump_outputs:
        dump_outputs(last, args.dump_outputs, rank)

    ms_per_step = elapsed * 1000.0 / args.steps
    pairs_per_sec = (vps * world * V) / (elapsed / args.steps)

    if rank == 0:
        result = {
            "metric": "fcma_voxel_pairs_per_sec",
            "value": pairs_per_sec,
            "unit": "voxel-pairs/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16" if device.type == "cuda" else "fp32",
            "data": "synthetic",
            "config": {
                "model": "fcma_voxel_selection",
                "num_voxels": V,
                "subjects": args.subjects,
                "epochs_per_subj": args.epochs_per_subj,
                "epoch_len": args.epoch_len,
                "voxels_per_step_per_gpu": vps,
                "num_folds": args.num_folds,
                "cv": not args.no_cv,
                "global_batch": vps * world,
                "seq_len": args.epoch_len,
                "parallelism": f"voxel-sharded dp{world}",
            },
            "_sink": sink,
        }
        del result["_sink"]
        print(json.dumps(result))

    if distributed:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
