#!/usr/bin/env python3
"""Event segmentation throughput: batched HMM forward-backward over
many searchlight-sized regions (the realistic whole-brain use: fit an
EventSegment per region).  Metric: region-fits/s.

One step = fitting ``--regions`` independent EventSegment models
(ragged lengths grouped by the batched forward-backward).

``--decode`` times inference instead: the models are fitted once outside
the timed steps and one step is ``decode_regions`` (MAP event paths) over
all regions; metric region-decodes/s.  ``--find-events`` times the
marginal route to hard labels (``find_events_regions`` + argmax) the same
way, for comparison."""

import argparse
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from benchmarks.common import dist_setup, emit, teardown, timed_steps  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--regions", type=int, default=64)
    ap.add_argument("--trs", type=int, default=200)
    ap.add_argument("--voxels", type=int, default=100)
    ap.add_argument("--events", type=int, default=8)
    ap.add_argument("--decode", action="store_true",
                    help="time decode_regions (MAP event paths) of "
                         "models fitted once outside the timed steps; "
                         "metric: region-decodes/s")
    ap.add_argument("--find-events", action="store_true",
                    help="like --decode, but time find_events_regions + "
                         "argmax, the marginal route to hard labels")
    args = ap.parse_args()

    rank, world, device, _ = dist_setup()
    from brainiak_amd.eventseg.event import EventSegment

    rng = np.random.RandomState(7 + rank)
    regions = args.regions if device.type == "cuda" else 8
    data = []
    for _ in range(regions):
        bounds = np.sort(rng.choice(
            np.arange(1, args.trs), args.events - 1, replace=False))
        means = rng.randn(args.events, args.voxels)
        seg = np.zeros((args.trs, args.voxels))
        prev = 0
        for e, b in enumerate(list(bounds) + [args.trs]):
            seg[prev:b] = means[e]
            prev = b
        data.append(seg + 0.5 * rng.randn(args.trs, args.voxels))

    dev = str(device) if device.type == "cuda" else "cpu"

    if args.decode or args.find_events:
        return bench_decode(args, data, regions, dev, rank, world, device)

    batched = not os.environ.get("BRAINIAK_EVENTSEG_SEQ")

    def step(i):
        if batched:
            EventSegment(args.events, n_iter=10,
                         device=dev).fit_regions(data)
        else:
            for d in data:
                EventSegment(args.events, n_iter=10,
                             device=dev).fit(d.copy())

    elapsed = timed_steps(step, args.steps, args.warmup, world, device)
    fits_per_sec = regions * world * args.steps / elapsed
    emit(rank, "eventseg_region_fits_per_sec", fits_per_sec, "fits/s",
         world, args.steps, args.warmup, elapsed, True, "weak", "fp64",
         {"model": "eventseg", "regions": regions, "trs": args.trs,
          "voxels": args.voxels, "events": args.events,
          "global_batch": regions, "seq_len": args.trs,
          "parallelism": f"region-sharded dp{world}"})
    teardown(world)


def bench_decode(args, data, regions, dev, rank, world, device):
    """One step = hard labels for every region from models fitted once
    up front: ``decode_regions`` (Viterbi), or with ``--find-events``
    the argmax of ``find_events_regions``'s marginals."""
    from brainiak_amd.eventseg.event import EventSegment

    proto = EventSegment(args.events, n_iter=10, device=dev)
    models = proto.fit_regions(data)

    if args.decode:
        def step(i):
            proto.decode_regions(models, data)
        metric = "eventseg_region_decodes_per_sec"
    else:
        def step(i):
            segments, _ = proto.find_events_regions(models, data)
            for seg in segments:
                seg.argmax(axis=1)
        metric = "eventseg_region_find_events_per_sec"

    elapsed = timed_steps(step, args.steps, args.warmup, world, device)
    per_sec = regions * world * args.steps / elapsed
    emit(rank, metric, per_sec, "regions/s",
         world, args.steps, args.warmup, elapsed, True, "weak", "fp64",
         {"model": "eventseg", "regions": regions, "trs": args.trs,
          "voxels": args.voxels, "events": args.events,
          "global_batch": regions, "seq_len": args.trs,
          "recursion": ("hip" if device.type == "cuda" and os.environ.get(
              "BRAINIAK_EVENTSEG_FB", "") != "torch" else "torch"),
          "parallelism": f"region-sharded dp{world}"})
    teardown(world)


if __name__ == "__main__":
    main()
