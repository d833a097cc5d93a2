#!/usr/bin/env python3
"""What localisation costs: `mt4_class_maps` beside its byte floor and beside a torch formulation of the same maps, and `MT4MTLKD/predict.py`
with and without `--localize`.  Measurement only; one step per command, each under its own `timeout`; every line is printed and appended to
--out (default profiles/r18_localize.txt):

    timeout -k 10 300 python3 tools/localize_timing.py kernel [--frames 512 --cells 8 14] [--reps 7]
    timeout -k 10 1100 python3 tools/localize_timing.py command DIR [--videos 9 --frames 2000] [--reps 7] [--parent TREE]

kernel:  `ops.class_maps` on --frames maps of --cells cells, C = 512 bf16 (ResNet-18) and C = 2048 fp32 (ResNet-50), for 6 and 100 columns, and
         `torch.einsum("byxk,jk->bjyx", map.float(), w)` (maps only: no range, peak or region) on the same tensors.  The variants alternate; a
         repetition is --calls calls between two device events on the current stream, over a ring of input maps larger than the 256 MB Infinity
         Cache (each call reads a map no earlier call of the repetition left in cache); microseconds per call, median / min / max over --reps
         repetitions after a warm-up repetition.  The byte floor: the map's bytes read once plus the three outputs written once, at 6.29 TB/s
         (the float4-copy rate MI355X_MICROARCH.md measures; 8.0 TB/s is the HBM3E figure on paper).
command: --videos directories of --frames 256 x 448 PNG files under DIR (16 distinct smooth frames, hard-linked), a synthetic ResNet-18 student
         and TCN; `predict.py --frames_dir ... --temporal_ckpt ...` without the flag, with `--localize i` and with `--localize ivt`, and -- with
         --parent TREE, a built checkout of the parent commit -- that tree's predict.py without the flag.  Alternating, --reps times after one
         warm-up round, each a fresh process; wall seconds (interpreter start and imports included): median, min, max, and the parent's own
         spread (max - min of its runs), which is the margin the run without the flag is held to."""
import argparse
import io
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

OUT = None
HBM_TBS = 6.29


def say(line):
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def _stat(xs, unit):
    return f"median {statistics.median(xs):.3f} {unit} min {min(xs):.3f} max {max(xs):.3f} ({len(xs)} reps)"


def kernel(a):
    import torch

    from computervision_codes_amd import ops
    h, w = a.cells
    g = torch.Generator().manual_seed(18)
    for c, dtype, what in ((512, torch.bfloat16, "C = 512 bf16"), (2048, torch.float32, "C = 2048 fp32")):
        map_bytes = a.frames * h * w * c * (2 if dtype == torch.bfloat16 else 4)
        ring = max(2, -(-(512 << 20) // map_bytes))                  # maps in rotation: more than twice the Infinity Cache between two reads of one
        feats = [torch.randn((a.frames, h, w, c), generator=g).to(dtype).cuda() for _ in range(ring)]
        rows = torch.randn((131, c), generator=g).cuda()
        for ncol in (6, 100):
            lo = 0 if ncol == 6 else 31
            wsel = rows[lo:lo + ncol].contiguous()
            got = ops.class_maps(feats[0], rows, lo, ncol, 0.5)[0]
            ref = torch.einsum("byxk,jk->bjyx", feats[0].double(), wsel.double())
            err = float((got.double() - ref).abs().max())
            runs = {"mt4_class_maps (maps, range, peak, region)": lambda i: ops.class_maps(feats[i % ring], rows, lo, ncol, 0.5),
                    "torch.einsum on map.float() (maps only)": lambda i: torch.einsum("byxk,jk->bjyx", feats[i % ring].float(), wsel)}
            times = {n: [] for n in runs}
            for rep in range(a.reps + 1):                            # (the first repetition warms up)
                for name, fn in runs.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    for i in range(a.calls):
                        fn(i)
                    e1.record()
                    e1.synchronize()
                    if rep:
                        times[name].append(e0.elapsed_time(e1) * 1e3 / a.calls)
            out_bytes = a.frames * ncol * (h * w + 8 + 2) * 4
            floor = (map_bytes + out_bytes) / (HBM_TBS * 1e12) * 1e6
            macs = a.frames * h * w * c * ncol
            say(f"{a.frames} maps of {h} x {w}, {what}, {ncol} columns | reads {map_bytes / 1e6:.1f} MB + writes {out_bytes / 1e6:.1f} MB: byte floor "
                f"{floor:.1f} us at {HBM_TBS} TB/s | {macs / 1e9:.2f} GMAC | max |m - m64| {err:.2e} | ring of {ring} maps, {a.calls} calls per repetition")
            for name, xs in times.items():
                med = statistics.median(xs)
                say(f"    {name}: {_stat(xs, 'us per call')} | {med / floor:.1f} x the byte floor | {macs / med / 1e6:.2f} TMAC/s")
        del feats


def _frames_png(n=16, h=256, w=448):
    from PIL import Image
    rng = np.random.default_rng(0)
    y, x = np.mgrid[0:h, 0:w]
    for i in range(n):
        base = np.stack([(x + 7 * i) % 256, (y * 2 + 3 * i) % 256, ((x + y) // 2) % 256], -1).astype(np.int32)
        wave = 40 * np.sin(x[..., None] / (17.0 + i) + np.arange(3)) * np.cos(y[..., None] / (23.0 + i))
        fr = np.clip(base * 0.5 + 60 + wave + rng.normal(0, 3.0, (h, w, 3)), 0, 255).astype(np.uint8)
        b = io.BytesIO()
        Image.fromarray(fr, "RGB").save(b, format="PNG")
        yield b.getvalue()


def command(a):
    import torch

    from computervision_codes_amd import shapes, synth
    work = os.path.abspath(a.dir)
    student, temporal = os.path.join(work, "student.pth"), os.path.join(work, "temporal.pth")
    dirs = [os.path.join(work, "videos", f"clip{v:02d}") for v in range(a.videos)]
    if not os.path.isfile(temporal):
        blobs = os.path.join(work, "blobs")
        os.makedirs(blobs)
        for i, b in enumerate(_frames_png()):
            with open(os.path.join(blobs, f"{i}.png"), "wb") as f:
                f.write(b)
        for d in dirs:
            os.makedirs(d)
            for i in range(a.frames):
                os.link(os.path.join(blobs, f"{i % 16}.png"), os.path.join(d, f"{i:06d}.png"))
        torch.save(synth.fill_from_shapes(shapes.spatial_cnn_shapes("resnet18"), seed=11), student)
        torch.save(synth.fill_from_shapes(shapes.tenco_shapes(11, 10, 3, 512, 512, 100, fpn=True), seed=12), temporal)
    common = [x for d in dirs for x in ("--frames_dir", d)] + ["--student_ckpt", student, "--temporal_ckpt", temporal, "--fpn", "--input_dim", "512",
                                                               "--out", os.path.join(work, "predictions")]

    def run(tree, extra):
        cmd = [sys.executable, os.path.join(tree, "MT4MTLKD", "predict.py")] + common + extra
        t0 = time.perf_counter()
        r = subprocess.run(cmd, cwd=tree, env=dict(os.environ, PYTHONPATH=tree), capture_output=True, text=True)
        secs = time.perf_counter() - t0
        if r.returncode != 0:
            raise SystemExit(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}")
        return secs
    variants = {"this tree, no flag": (ROOT, []), "this tree, --localize i": (ROOT, ["--localize", "i"]), "this tree, --localize ivt": (ROOT, ["--localize", "ivt"])}
    if a.parent:
        variants = {"parent tree, no flag": (os.path.abspath(a.parent), []), **variants}
    times = {n: [] for n in variants}
    for rep in range(a.reps + 1):                                    # (the first round is the warm-up: file cache, code-object cache)
        secs = {n: run(*v) for n, v in variants.items()}
        say(f"round {rep}{' (warm-up)' if not rep else ''}: " + " | ".join(f"{n} {s:.2f} s" for n, s in secs.items()))
        if rep:
            for n, s in secs.items():
                times[n].append(s)
    frames = a.videos * a.frames
    say(f"{a.videos} videos x {a.frames} frames of 256 x 448 PNG, ResNet-18 fp32 + TCN, --png_decode host; wall seconds of fresh processes:")
    for name, xs in times.items():
        say(f"  {name}: {_stat(xs, 's')} | {frames / statistics.median(xs):.0f} frames/s")
    base = times.get("parent tree, no flag") or times["this tree, no flag"]
    say(f"  margin: the spread of '{'parent tree, no flag' if a.parent else 'this tree, no flag'}' is {max(base) - min(base):.3f} s (max - min of its {len(base)} runs)")
    for name in ("this tree, no flag", "this tree, --localize i", "this tree, --localize ivt"):
        if times[name] is not base:
            say(f"  {name} - baseline: {statistics.median(times[name]) - statistics.median(base):+.3f} s (medians)")


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_localize.txt"))
    sub = p.add_subparsers(dest="step", required=True)
    s = sub.add_parser("kernel")
    s.add_argument("--frames", type=int, default=512)
    s.add_argument("--cells", type=int, nargs=2, default=[8, 14])
    s.add_argument("--calls", type=int, default=20)
    s.add_argument("--reps", type=int, default=7)
    s = sub.add_parser("command")
    s.add_argument("dir")
    s.add_argument("--videos", type=int, default=9)
    s.add_argument("--frames", type=int, default=2000)
    s.add_argument("--reps", type=int, default=7)
    s.add_argument("--parent", default="", help="a built checkout of the parent commit: its predict.py is timed too")
    a = p.parse_args()
    OUT = a.out
    {"kernel": kernel, "command": command}[a.step](a)
