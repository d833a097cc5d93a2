#!/usr/bin/env python3
"""The validation metric on the host (`metrics.Recognition`, sklearn) against the device (`metrics_device.DeviceRecognition`, --metrics device).
One step per command, each GPU step under its own `timeout`, chained with `&&`:

    timeout -k 10 600 python3 tools/metrics_bench.py metric [--videos 5 --frames 2000] [--reps 7] [--host_reps 3]
    timeout -k 10 900 python3 tools/metrics_bench.py metric --videos 9 --frames cap
    timeout -k 10 900 python3 tools/metrics_bench.py driver DIR --metrics host [--root CHECKOUT] [--frames 2000] [--epochs 3]
    timeout -k 10 900 python3 tools/metrics_bench.py driver DIR --metrics device

metric: K = 100 random scores with 15 % positives; one `compute_video_AP()` per repetition after a warm-up call, the device side from
        `compute_video_AP()` entry to the numpy result (launch + the D2H of the [V, K] doubles), the host side on host copies of the same rows;
        medians.  Also the six components of a closing report (ivt + the five disentangled ones) together.  The device object keeps the
        concatenation of its videos from the warm-up call, so the device figures leave out the `torch.cat` a driver pays at every validation
        (it builds a new object each time); the disentangled components re-run `component_max` per call.  The driver step includes all of it.
driver: `Temporal_tenco/run.py -t --fpn --mask --mask_draw device --val_interval 1` on the synthetic 31 x --frames set of
        `tools/tenco_train_bench.py --driver`: seconds per epoch (`Traning |` lines) and per validation (`video-wise | eta`).  --root: run the
        scripts and the package of another checkout (the parent commit, which ignores the --metrics flag it does not know)."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def metric(a):
    import torch

    from computervision_codes_amd import metrics, ops
    from computervision_codes_amd.metrics_device import DeviceRecognition
    frames = ops.video_ap_max_rows() if a.frames == "cap" else int(a.frames)
    rng = np.random.default_rng(5)
    host, dev = metrics.Recognition(100), DeviceRecognition(100)
    for _ in range(a.videos):
        t, p = (rng.random((frames, 100)) < 0.15).astype(np.float32), rng.random((frames, 100)).astype(np.float32)
        host.update(t, p)
        host.video_end()
        dev.update(torch.from_numpy(t).cuda(), torch.from_numpy(p).cuda())
        dev.video_end()
    comps = ("ivt", "i", "v", "t", "iv", "it")

    def timed(fn, reps):
        fn()                                                       # warm-up: lazy loading, allocator, sklearn import
        out = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            out.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(out), min(out), max(out)
    rows = (("device ivt", lambda: dev.compute_video_AP(), a.reps), ("device six components", lambda: [dev.compute_video_AP(c) for c in comps], a.reps),
            ("host ivt", lambda: host.compute_video_AP(), a.host_reps), ("host six components", lambda: [host.compute_video_AP(c) for c in comps], a.host_reps))
    for name, fn, reps in rows:
        med, lo, hi = timed(fn, reps)
        print(f"{a.videos} videos x {frames} frames x 100 classes | {name}: median {med:.3f} ms min {lo:.3f} max {hi:.3f} ({reps} reps)", flush=True)
    h, d = host.compute_video_AP(), dev.compute_video_AP()
    print(f"mAP host {h['mAP']:.15f} device {d['mAP']:.15f} max |AP diff| {np.nanmax(np.abs(h['AP'] - d['AP'])):.2e}")


def driver(a):
    root = os.path.abspath(a.root)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from tenco_train_bench import make_driver_tree
    tree, data = make_driver_tree(os.path.abspath(a.dir), a.frames, root=root)
    r = subprocess.run([sys.executable, "run.py", "-t", "--fpn", "--mask", "--mask_draw", "device", "--metrics", a.metrics, "--input_dim", "512", "--loss_type", "all",
                        "--epochs", str(a.epochs), "-l", "1e-2", "5e-3", "1e-2", "-w", "9", "18", "200", "--version", "S_m", "--version1", "S", "--data_dir", data,
                        "--kfold", "1", "--val_interval", "1"], cwd=os.path.join(tree, "Temporal_tenco"), env=dict(os.environ, PYTHONPATH=root),
                       capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(r.stdout[-2000:] + r.stderr[-2000:])
    who = "THIS" if root == ROOT else "ROOT " + os.path.basename(root)              # (no absolute paths in a record)
    for ln in r.stdout.splitlines():
        if "Traning |" in ln or "video-wise" in ln:
            print(f"driver {who} --metrics {a.metrics} frames {a.frames}: {ln.strip()}")
    epoch = [float(s) for s in re.findall(r"\| ([0-9.]+) secs", "\n".join(ln for ln in r.stdout.splitlines() if ln.startswith("Traning |")))]
    val = [float(s) for s in re.findall(r"eta ([0-9.]+) secs", r.stdout)]
    print(f"driver {who} --metrics {a.metrics} frames {a.frames}: epoch secs {epoch} validation secs {val}")


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    sub = p.add_subparsers(dest="step", required=True)
    m = sub.add_parser("metric")
    m.add_argument("--videos", type=int, default=5)
    m.add_argument("--frames", type=str, default="2000")
    m.add_argument("--reps", type=int, default=7)
    m.add_argument("--host_reps", type=int, default=3)
    d = sub.add_parser("driver")
    d.add_argument("dir")
    d.add_argument("--metrics", choices=["host", "device"], default="host")
    d.add_argument("--root", type=str, default=ROOT)
    d.add_argument("--frames", type=int, default=2000)
    d.add_argument("--epochs", type=int, default=3)
    a = p.parse_args()
    {"metric": metric, "driver": driver}[a.step](a)
