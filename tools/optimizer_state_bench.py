#!/usr/bin/env python3
"""What --momentum and --optimizer adamw cost (GPU box): a trainer's whole step -- forward, losses and backward replayed as one hipGraph, then the
update launched behind it as `apply_update` does -- with the plain update, with momentum 0.9 and with AdamW.  Rows: `resnet50_bf16` = the student
step on 64 uint8 frames of 256 x 448, bf16 operands; `tenco` = the temporal step with the draws made on the device, full-size head (11 + 3 x 10
layers, 512 maps), at --length frames.  Modelled on tools/guarded_update_bench.py.

  python3 tools/optimizer_state_bench.py [--parent DIR] [--reps 7] [--steps 40] [--length 2000] [--workloads resnet50_bf16,tenco]
        every repetition starts one fresh child process per variant, alternating: the default step of the checkout at DIR (a built parent checkout
        carried in the tree, when given), the default step of this tree (the same launches: a difference beyond the parent's own spread means the
        default path changed), `--momentum 0.9` (mt4_sgd_momentum_step_f32: 20 bytes per parameter instead of 12) and `--optimizer adamw`
        (mt4_optim_advance + mt4_adamw_step_f32: 28 bytes).  A child times its steps with device events after a warm-up that includes the graph
        capture and reports the median step; the table gives, per variant, the median of the repetitions' medians and their spread (min .. max).
        Each child runs under a time limit of its own and the run stops at the first child that does not exit with status 0.
  python3 tools/optimizer_state_bench.py --child default|momentum|adamw --workload W [--root DIR] ...
        one such process: one JSON line.
  python3 tools/optimizer_state_bench.py --latest_write
        host seconds one `_latest` write of the ResNet-50 student takes under --resume without and with the optimizer file (momentum: one state
        buffer; AdamW: two), median of --reps writes into a temporary directory."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("default", "momentum", "adamw")


def _optim(mode):
    if mode == "default":
        return {}                                            # (no keyword -- the parent checkout does not know it)
    from computervision_codes_amd.flatparams import Optim
    return {"optim": Optim("sgd", 0.9) if mode == "momentum" else Optim("adamw")}


def _timed(step, steps, warmup):
    import torch
    ms = []
    for i in range(warmup + steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step(i)
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    return round(statistics.median(ms), 4)


def _student(net, op, kw):
    import torch
    from computervision_codes_amd import shapes, synth
    from computervision_codes_amd.spatial_cnn_train import SpatialCnnTrainer
    tr = SpatialCnnTrainer(net, lr=1e-3, weight_decay=1e-5, rates=(1.0, 0.0, 0.1), operand_dtype=torch.bfloat16 if op == "bf16" else torch.float32, **kw)
    return tr.load_state_dict(synth.fill_from_shapes(shapes.spatial_cnn_shapes(net), seed=1))


def child(workload: str, mode: str, root: str, steps: int, warmup: int, length: int, graph: bool = True):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from computervision_codes_amd import shapes, synth
    kw = _optim(mode)
    rng = np.random.default_rng(3)
    out = {"workload": workload, "mode": mode, "root": os.path.relpath(root, HERE), "steps": steps}
    if workload == "tenco":
        from computervision_codes_amd.tenco_train import TencoTrainer
        tr = TencoTrainer(11, 10, 3, 512, 512, lr=1e-3, weight_decay=1e-5, **kw)
        tr.load_state_dict(synth.fill_from_shapes(shapes.tenco_shapes(11, 10, 3, 512, 512, 100, fpn=True), seed=1))
        x = synth.synthetic_features(length, 512, seed=2).cuda()
        z = tr.prepare_labels({s: torch.from_numpy((rng.random((length, k)) < 0.1).astype(np.int64)) for s, k in (("", 100), ("_i", 6), ("_v", 10), ("_t", 15))})
        step = lambda i: tr.train_step(x, z, draws=(5, i), use_graph=graph)
    else:
        net, op = workload.split("_")
        batch, h, w = 64, 256, 448
        tr = _student(net, op, kw)
        frames = synth.synthetic_frames(batch, h, w, seed=2).cuda()
        z = torch.from_numpy((rng.random((batch, 131)) < 0.1).astype(np.float32)).cuda()
        tp = [torch.from_numpy(rng.standard_normal((batch, k)).astype(np.float32)).cuda() for k in (6, 10, 15)]
        tf = [torch.from_numpy(rng.standard_normal((batch, 1536)).astype(np.float32)).cuda() for _ in range(3)]
        step = lambda i: tr.train_step(frames, z, tp, tf, use_graph=graph)
    out["parameters"] = int(tr.P.numel())
    out["ms"] = _timed(step, steps, warmup)
    # the update alone, behind the same step: the launches `apply_update` makes on one unchanged gradient
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ups = []
    for _ in range(20):
        a.record()
        tr.apply_update()
        b.record()
        torch.cuda.synchronize()
        ups.append(a.elapsed_time(b))
    out["update_ms"] = round(statistics.median(ups), 4)
    print(json.dumps(out), flush=True)


def latest_write(reps: int):
    """host seconds of `trainloop._save_pair` for the ResNet-50 student: the checkpoint and sidecar alone, and with the optimizer file"""
    sys.path.insert(0, HERE)
    from computervision_codes_amd import trainloop
    for mode in MODES:
        tr = _student("resnet50", "bf16", _optim(mode))
        secs, export, size = [], [], 0
        with tempfile.TemporaryDirectory() as d:
            latest, older = os.path.join(d, "m_latest.pth"), []
            for epoch in range(reps):
                t0 = time.perf_counter()
                state, osd = tr.state_dict(), tr.optimizer_state_dict()
                t1 = time.perf_counter()
                rec = {"epoch": epoch, "top": 0.0, "generators": {}}
                trainloop._save_pair(state, latest, rec, older, 1, osd)
                secs.append(time.perf_counter() - t0)
                export.append(t1 - t0)
                older = [rec]
                if osd is not None:
                    size = os.path.getsize(trainloop.optim_file(latest, epoch))
        print(f"  {mode:10s} one `_latest` write under --resume: {statistics.median(secs):7.3f} s (min {min(secs):.3f}, of it {statistics.median(export):.3f} s "
              f"exporting to the host), optimizer file {size / 2 ** 20:7.1f} MiB", flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--child", choices=MODES)
    p.add_argument("--latest_write", action="store_true")
    p.add_argument("--workload", default="resnet50_bf16", choices=["tenco", "resnet50_bf16", "resnet50_fp32", "resnet18_bf16"])
    p.add_argument("--workloads", default="resnet50_bf16,tenco")
    p.add_argument("--root", default=HERE)
    p.add_argument("--parent", default=None)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--steps", type=int, default=40)
    p.add_argument("--warmup", type=int, default=8)
    p.add_argument("--length", type=int, default=2000)
    p.add_argument("--eager", action="store_true", help="(--child) launch the step's kernels one by one instead of replaying a graph: for a kernel trace")
    a = p.parse_args()
    if a.child:
        return child(a.workload, a.child, os.path.abspath(a.root), a.steps, a.warmup, a.length, not a.eager)
    if a.latest_write:
        return latest_write(a.reps)
    variants = ([("parent default", "default", os.path.abspath(a.parent))] if a.parent else []) + \
        [("default", "default", HERE), ("--momentum 0.9", "momentum", HERE), ("--optimizer adamw", "adamw", HERE)]
    for workload in a.workloads.split(","):
        res, ups = {name: [] for name, _, _ in variants}, {name: [] for name, _, _ in variants}
        for rep in range(a.reps):
            for name, mode, root in variants:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--workload", workload, "--root", root, "--steps", str(a.steps),
                                    "--warmup", str(a.warmup), "--length", str(a.length)], capture_output=True, text=True, timeout=240)
                if r.returncode != 0:
                    sys.exit(f"{workload} {name}: exit status {r.returncode}\n{r.stdout[-1000:]}{r.stderr[-2000:]}")
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
                print(f"rep {rep} {name}: {line}", flush=True)
                res[name].append(json.loads(line)["ms"])
                ups[name].append(json.loads(line)["update_ms"])
        what = f"temporal step (device draws), {a.length} frames" if workload == "tenco" else f"{workload} student step, 64 frames of 256 x 448"
        print(f"\n{what}; forward + backward replayed as a hipGraph + the update, ms: median of {a.reps} process medians (min .. max)")
        base = statistics.median(res["default"])
        for name, _, _ in variants:
            v = res[name]
            print(f"  {name:22s} {statistics.median(v):8.3f}  ({min(v):.3f} .. {max(v):.3f})  {100.0 * (statistics.median(v) / base - 1.0):+6.2f} % of default"
                  f" | the update's launches alone {statistics.median(ups[name]):.3f} ms")
        if a.parent:
            pv, dv = res["parent default"], statistics.median(res["default"])
            print(f"  default inside the parent's own spread ({min(pv):.3f} .. {max(pv):.3f}): {'yes' if min(pv) <= dv <= max(pv) else 'NO'}")
        print(flush=True)


if __name__ == "__main__":
    main()
