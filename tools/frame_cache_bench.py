#!/usr/bin/env python3
"""The frame cache (--frame_cache) against the run without it (GPU box).  Steps, each a command of its own (run every GPU step under its own
`timeout` and chain them with `&&`, see tools/README.md); the dataset comes from `tools/train_transform_bench.py make-data DIR 40`, the setup of
profiles/r06_prefetch_loader.txt (480 x 854 PNGs -> 256 x 448, batch 64, --png_decode device --train_transform device --prefetch 16):

  kernels [N H W]                 `mt4_put_frames_u8` / `mt4_take_frames_u8` alone: event-timed us per call and GB/s (bytes read + written) for N
                                  frames of H x W x 3 (default 1024 256 448) into / out of a pool of 4 N slots at scattered slots, 7 repetitions
  loader DIR [--frame_cache GB]   the loader alone: 3 passes ("epochs") of `loader.FrameLoader(prefetch=16)` over the training batches consumed as fast
                                  as it delivers, frames/s per pass; GB > 0 puts a `cholect.FrameCache` behind it (sealed after every pass) and
                                  adds the cache's counters and the HBM its pool reserves; 3 repetitions, a fresh cache each
  epoch DIR [--frame_cache GB]    `Spatial_cnn/run.py -t` for 3 epochs (ResNet-50, bf16 operands, --loss_type i, no validation before the last epoch):
                                  seconds and frames/s per epoch.  Without --frame_cache the flag is not passed at all, so the same command runs on
                                  a checkout that does not know it (the A/B baseline: alternate the two checkouts in one session)
  all DIR GB                      kernels, then loader and epoch without and with the cache, each a fresh child process under a time limit of its own,
                                  timed, the next one started only after exit status 0

Every step prints one JSON line."""
import json
import os
import random
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NAMES = ["original", "vflip", "hflip", "contrast", "rot90"]


def kernels(N=1024, H=256, W=448, reps=7, iters=10):
    import numpy as np
    import torch
    from computervision_codes_amd import ops
    fb = H * W * 3
    pool = torch.empty((4 * N, H, W, 3), dtype=torch.uint8, device="cuda")
    frames = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, device="cuda")
    out = torch.empty_like(frames)
    slots = np.random.default_rng(1).permutation(4 * N)[:N].astype(np.int32)
    dev_slots = torch.from_numpy(slots).cuda()
    from computervision_codes_amd._lib import check, lib
    stream = torch.cuda.current_stream().cuda_stream
    calls = {"put": lambda: check(lib.mt4_put_frames_u8(pool.data_ptr(), dev_slots.data_ptr(), frames.data_ptr(), N, fb, 4 * N, stream)),
             "take": lambda: check(lib.mt4_take_frames_u8(pool.data_ptr(), dev_slots.data_ptr(), out.data_ptr(), N, fb, 4 * N, stream))}
    ops.put_frames(pool, slots, frames)
    ops.take_frames(pool, slots, out)
    assert torch.equal(out, frames)
    us = {k: [] for k in calls}
    for r in range(reps + 1):                                  # (round 0 warms up)
        for k, fn in calls.items():
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            if r:
                us[k].append(a.elapsed_time(b) * 1e3 / iters)
    res = {"step": "kernels", "frames": N, "size": [H, W], "frame_bytes": fb, "pool_slots": 4 * N, "reps": reps, "calls_per_rep": iters}
    for k, v in us.items():
        med = statistics.median(v)
        res[k] = {"median_us": round(med, 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1), "GB_per_s_read_plus_write": round(2 * N * fb / med / 1e3, 1)}
    print(json.dumps(res))


def loader(d, gb=0.0, B=64, H=256, W=448, K=16, reps=3, passes=3):
    import argparse
    import torch
    from computervision_codes_amd import cholect
    from computervision_codes_amd.loader import FrameLoader, SampleTables
    vids, _, _ = cholect.split_videos("cholect45-crossval", 1)
    labels = {v: cholect.load_labels(d, v) for v in vids}
    samples = [(v, i) for v in vids for i in range(len(labels[v]["ivt"]))]
    tables = SampleTables(labels, videos=vids)
    F = argparse.Namespace(data_dir=d, augmentation_list=list(NAMES), png_decode="device", decode_workers=8, train_transform="device")
    frames = len(samples)
    pass_s, stats, cache_stats, reserved = [], [], None, None
    for r in range(reps + 1):                                  # (repetition 0 warms up: library load, table pools, file cache, pinned staging)
        torch.cuda.synchronize()
        before = torch.cuda.memory_reserved()
        kw = {"cache": cholect.FrameCache(int(gb * 1e9))} if gb > 0 else {}
        order_rng, rng, secs, st = random.Random(1), random.Random(r), [], []
        for p in range(passes):
            order = list(samples)
            order_rng.shuffle(order)
            batches = [order[k:k + B] for k in range(0, len(order), B)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with FrameLoader(F, batches, labels, tables, (H, W), rng, prefetch=K, **kw) as fl:
                for fb in fl:
                    pass
            if kw:
                kw["cache"].seal()
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
            st.append(dict(fl.stats))
        if r:
            pass_s.append(secs)
            stats = st
        if kw:
            cache_stats, reserved = dict(kw["cache"].stats), torch.cuda.memory_reserved() - before
            del kw
            torch.cuda.empty_cache()
    per_pass = list(zip(*pass_s))
    print(json.dumps({"step": "loader", "frame_cache_gb": gb, "batch": B, "size": [H, W], "prefetch": K, "png_decode": "device", "train_transform": "device",
                      "frames_per_pass": frames, "reps": reps,
                      "frames_per_s": [{"median": round(frames / statistics.median(t), 1), "min": round(frames / max(t), 1), "max": round(frames / min(t), 1)} for t in per_pass],
                      "pass_s": [[round(v, 4) for v in s] for s in pass_s], "loader_stats_per_pass": stats, "cache_stats": cache_stats,
                      "reserved_bytes_added": reserved}))


def epoch(d, gb=0.0, B=64, K=16):
    import torch
    from computervision_codes_amd import cholect, drivers
    vids, _, _ = cholect.split_videos("cholect45-crossval", 1)
    n = sum(len(cholect.load_labels(d, v)["ivt"]) for v in vids)
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as work:
        os.chdir(work)
        try:
            drivers.spatial_cnn_train(["-t", "--network", "resnet50", "--student_dim", "2048", "--loss_type", "i", "--operand_dtype", "bf16", "--epochs", "3",
                                       "--val_interval", "3", "--batch", str(B), "--version", "B", "--data_dir", d, "--kfold", "1", "--png_decode", "device",
                                       "--train_transform", "device", "--prefetch", str(K)] + (["--frame_cache", str(gb)] if gb > 0 else []))
            log = open(os.path.join(work, "__checkpoint__", "run_B", "rendezvous_lcholect45-crossval_cholect1.log")).read()
        finally:
            os.chdir(cwd)
    lines = [ln for ln in log.splitlines() if "Traning | lr:" in ln]
    secs = [float(ln.split("| loss")[1].split("|")[1].split()[0]) for ln in lines]
    print(json.dumps({"step": "epoch", "frame_cache_gb": gb, "prefetch": K, "batch": B, "frames_per_epoch": n, "epoch_s": secs,
                      "frames_per_s": [round(n / s, 1) for s in secs], "cache_notes": [ln.split("| cache ")[1].strip() if "| cache " in ln else None for ln in lines],
                      "reserved_bytes": torch.cuda.memory_reserved()}))


def run_all(d, gb):
    import subprocess
    me = [sys.executable, os.path.abspath(__file__)]
    steps = [(["kernels"], 120), (["loader", d], 300), (["loader", d, "--frame_cache", str(gb)], 300), (["epoch", d], 300),
             (["epoch", d, "--frame_cache", str(gb)], 300)]
    for args, limit in steps:
        print("== " + " ".join(args), flush=True)
        t0 = time.perf_counter()
        try:
            rc = subprocess.run(me + args, timeout=limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        print(json.dumps({"step": "all", "ran": args, "exit_status": rc, "wall_s": round(time.perf_counter() - t0, 1)}), flush=True)
        if rc != 0:                                            # nothing more is started on the GPU behind a step that failed or hung
            sys.exit(rc)


if __name__ == "__main__":
    cmd, a = (sys.argv[1] if len(sys.argv) > 1 else ""), sys.argv[2:]
    gb = 0.0
    if "--frame_cache" in a:
        i = a.index("--frame_cache")
        gb = float(a[i + 1])
        del a[i:i + 2]
    if cmd == "kernels":
        kernels(*[int(v) for v in a[:3]])
    elif cmd == "loader" and a:
        loader(a[0], gb)
    elif cmd == "epoch" and a:
        epoch(a[0], gb)
    elif cmd == "all" and len(a) >= 2:
        run_all(a[0], float(a[1]))
    else:
        sys.exit(__doc__)
