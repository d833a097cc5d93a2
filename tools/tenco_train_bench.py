#!/usr/bin/env python3
"""Temporal_tenco training step, wall time per step (synchronised), one process, one GPU, the full 11/10/3 model:
  (a) host draw + explicit masks : `draw_masks` + `train_step(masks=...)`                      -- what `run.py -t` runs by default
  (b) no masks, replayed         : `train_step(use_graph=True)`                                -- what `bench.py` times
  (c) device draws, eager        : `train_step(draws=(seed, step))`
  (d) device draws, replayed     : `train_step(draws=(seed, step), use_graph=True)`            -- `run.py -t --mask_draw device`
Medians over --reps alternating repetitions of --steps steps each, at every T of --lengths; the reserved bytes a cached graph adds.

    python tools/tenco_train_bench.py [--lengths 256 2000] [--reps 7] [--steps 5]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/tenco_train_bench.py --only d --lengths 2000 --reps 1 --steps 10
    python tools/tenco_train_bench.py --driver DIR [--frames 600] [--epochs 3]

--driver builds a synthetic CholecT45-shaped dataset of --frames frames per video under DIR and runs `Temporal_tenco/run.py -t --fpn --mask`
once with `--mask_draw host` and once with `--mask_draw device`: the epoch times of the `Traning |` lines (the fold's 31 training videos)."""
import argparse
import os
import re
import shutil
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from computervision_codes_amd import cholect, featfile, shapes, synth  # noqa: E402

HEADS = (("", 100), ("_i", 6), ("_v", 10), ("_t", 15))


def step_times(args):
    from computervision_codes_amd.tenco_train import TencoTrainer
    dev = torch.device("cuda:0")
    sd = synth.fill_from_shapes(shapes.tenco_shapes(), seed=47)
    for T in args.lengths:
        x = synth.synthetic_features(T, 512, seed=47).to(dev)
        tr = {m: TencoTrainer(lr=0.01, device=str(dev)).load_state_dict(sd) for m in args.only}
        z = next(iter(tr.values())).prepare_labels({s: torch.from_numpy((synth.uniform01(3, i, T * k) < 0.1).reshape(T, k).astype(np.int64))
                                                    for i, (s, k) in enumerate(HEADS)})
        gen = torch.Generator().manual_seed(47)
        count = [0]

        def one(m):
            count[0] += 1
            if m == "a":
                tr[m].train_step(x, z, masks=tr[m].draw_masks(T, gen))
            elif m == "b":
                tr[m].train_step(x, z, use_graph=True)
            else:
                tr[m].train_step(x, z, draws=(47, count[0]), use_graph=m == "d")
        for m in args.only:                                            # warm-up: lazy loading, allocator, graph capture
            for _ in range(2):
                one(m)
        times = {m: [] for m in args.only}
        for _ in range(args.reps):
            for m in args.only:                                        # alternating: a b c d a b c d ...
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    one(m)
                torch.cuda.synchronize()
                times[m].append((time.perf_counter() - t0) / args.steps * 1e3)
        for m in args.only:
            v = sorted(times[m])
            print(f"T {T} ({m}) ms/step median {statistics.median(v):.3f} min {v[0]:.3f} max {v[-1]:.3f} reps {' '.join(f'{t:.3f}' for t in times[m])}")
        for m in args.only:
            if tr[m]._graphs:
                print(f"T {T} ({m}) cached graphs {len(tr[m]._graphs)} reserved bytes added {tr[m].graph_reserved_bytes}")
        del tr
        torch.cuda.empty_cache()


def make_driver_tree(d, frames, root=ROOT):
    """a synthetic CholecT45-shaped dataset of `frames` frames per video and the Spatial_cnn feature file of run_S under d (emptied first), beside
    a copy of `root`'s MT4MTLKD/ scripts -> (tree, data)"""
    shutil.rmtree(d, ignore_errors=True)
    tree, data = os.path.join(d, "MT4MTLKD"), os.path.join(d, "CholecT45")
    shutil.copytree(os.path.join(root, "MT4MTLKD"), tree)
    rng = np.random.default_rng(3)
    vids = cholect.extraction_videos("cholect45-crossval", 1)
    for sub, k in (("triplet", 100), ("instrument", 6), ("verb", 10), ("target", 15)):
        os.makedirs(os.path.join(data, sub))
        for v in vids:
            lab = np.concatenate([np.arange(frames)[:, None], (rng.random((frames, k)) < 0.15).astype(int)], 1)
            np.savetxt(os.path.join(data, sub, v + ".txt"), lab, fmt="%d", delimiter=",")
    featfile.write_feats(os.path.join(tree, "0-5fold", "data_feats", "run_S", "k1_feats.pkl"),
                         {v[-2:]: rng.standard_normal((frames, 512)).astype(np.float32) for v in vids})
    return tree, data


def driver_times(args):
    d = os.path.abspath(args.driver)
    tree, data = make_driver_tree(d, args.frames)
    env = dict(os.environ, PYTHONPATH=ROOT)
    for mode in ("host", "device"):
        r = subprocess.run([sys.executable, "run.py", "-t", "--fpn", "--mask", "--mask_draw", mode, "--input_dim", "512", "--loss_type", "all", "--epochs",
                            str(args.epochs), "-l", "1e-2", "5e-3", "1e-2", "-w", "9", "18", "200", "--version", f"S_{mode}", "--version1", "S", "--data_dir", data,
                            "--kfold", "1", "--val_interval", "-1"], cwd=os.path.join(tree, "Temporal_tenco"), env=env, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit(r.stdout[-2000:] + r.stderr[-2000:])
        for ln in r.stdout.splitlines():
            if ln.startswith(("Traning |", "mask_draw")):
                print(f"driver --mask_draw {mode} frames {args.frames}: {ln}")
        secs = [float(s) for s in re.findall(r"\| ([0-9.]+) secs", "\n".join(ln for ln in r.stdout.splitlines() if ln.startswith("Traning |")))]
        print(f"driver --mask_draw {mode} frames {args.frames}: epoch secs {secs}")
    shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--lengths", type=int, nargs="+", default=[256, 2000])
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--only", type=str, nargs="+", default=["a", "b", "c", "d"], choices=["a", "b", "c", "d"])
    p.add_argument("--driver", type=str, default=None)
    p.add_argument("--frames", type=int, default=600)
    p.add_argument("--epochs", type=int, default=3)
    a = p.parse_args()
    driver_times(a) if a.driver else step_times(a)
