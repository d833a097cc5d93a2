"""The train transform of the frame trainers (`Spatial_cnn/dataloader.py:89-100,153-162`: Resize -> vflip -> hflip -> autocontrast ->
rotation by a random angle with expand -> Resize) as a function of (frames, random draws) that runs on the device and returns the bytes
Pillow returns (`drivers.load_train_frames_u8`, the `--train_transform host` path).

`draw_params` consumes the `random.Random` of the host path draw for draw and does the float64 matrix work of `Image.rotate`;
`reference_u8` is the integer arithmetic in numpy (CPU tests, bug hunting); `train_transform_device` launches the three kernels of
csrc/augment_kernels.hip; `load_train_batch_device` is the loader `drivers._frame_batch` routes to.  This module imports without
libmt4hip.so: `ops` is imported where a launch happens."""
from __future__ import annotations

import math
import os
from typing import Dict, List, Sequence, Tuple

import numpy as np

NPARAMS = 12            # MT4_AUG_PARAMS (include/mt4hip.h): vflip, hflip, a0..a5, nw, nh, contrast, 0


def supported(names: Sequence[str]) -> bool:
    """the lists the device form covers: at most one `rot90`, at most one `contrast`, and no `contrast` after the `rot90` (the black fill of
    the rotation would enter the histogram).  A second autocontrast is NOT the identity: `int(hi * scale + offset)` is 254 for about 15 % of
    the (lo, hi) pairs, so the second one stretches again; the kernels hold one LUT per channel, so such a list keeps the host path.  Flips may
    stand anywhere; `original` and names `_augment` ignores are no-ops."""
    seen_rot = seen_contrast = False
    for n in names:
        if n == "rot90":
            if seen_rot:
                return False
            seen_rot = True
        elif n == "contrast":
            if seen_rot or seen_contrast:
                return False
            seen_contrast = True
    return True


class Params:
    """table int32 [B, NPARAMS] (the rows the kernels read), the frame size (h, w) it was built for, rotated = the list has `rot90`"""

    def __init__(self, table: np.ndarray, h: int, w: int, rotated: bool):
        self.table, self.h, self.w, self.rotated = table, h, w, rotated

    def __len__(self):
        return len(self.table)

    def sizes(self) -> List[Tuple[int, int]]:
        """(nh, nw) of every frame after the rotation"""
        return [(int(r[9]), int(r[8])) for r in self.table]


def _fix(v: float) -> int:
    return int(math.floor(v * 65536.0 + 0.5))


def rotation_row(angle: float, h: int, w: int) -> Tuple[List[int], int, int]:
    """`im.rotate(angle, NEAREST, expand=True)` of a w x h image -> ([a0..a5] in 16.16 fixed point, nw, nh): output pixel (X, Y) of the
    nw x nh result reads source ((a2 + X a0 + Y a1) >> 16, (a5 + X a3 + Y a4) >> 16), 0 outside.  float64 in Pillow's operation order."""
    angle = angle % 360.0
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]

    def T(x, y):
        return m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2], m[5] = T(-w / 2.0, -h / 2.0)
    m[2] += w / 2.0
    m[5] += h / 2.0
    xs, ys = zip(*(T(x, y) for x, y in ((0, 0), (w, 0), (w, h), (0, h))))
    nw = math.ceil(max(xs)) - math.floor(min(xs))
    nh = math.ceil(max(ys)) - math.floor(min(ys))
    m[2], m[5] = T(-(nw - w) / 2.0, -(nh - h) / 2.0)
    fx = [_fix(m[0]), _fix(m[1]), _fix(m[2] + 0.5 * m[0] + 0.5 * m[1]), _fix(m[3]), _fix(m[4]), _fix(m[5] + 0.5 * m[3] + 0.5 * m[4])]
    return fx, int(nw), int(nh)


def draw_params(rng, names: Sequence[str], n: int, h: int, w: int) -> Params:
    """the draws of `drivers._augment` for n frames of h x w, frame by frame in list order (`random() < 0.4` per vflip, `random() < 0.4`
    per hflip, `random() < 0.5` per contrast, `uniform(-90, 90)` per rot90): afterwards rng is in the state the host path leaves.  A flip
    listed after `rot90` acts on the rotated image; it is folded into the affine map (X -> nw-1-X, Y -> nh-1-Y), which is exact in integers."""
    if not supported(names):
        raise ValueError(f"augmentation list {list(names)}: 'contrast' after 'rot90' (or 'contrast' / 'rot90' twice) has no device form")
    table = np.zeros((n, NPARAMS), np.int32)
    for i in range(n):
        vflip = hflip = contrast = 0
        post_v = post_h = 0
        fx, nw, nh = [65536, 0, 32768, 0, 65536, 32768], w, h          # the identity map: (32768 + 65536 X) >> 16 = X
        rotated = False
        for name in names:
            if name == "vflip" and rng.random() < 0.4:
                if rotated:
                    post_v ^= 1
                else:
                    vflip ^= 1
            elif name == "hflip" and rng.random() < 0.4:
                if rotated:
                    post_h ^= 1
                else:
                    hflip ^= 1
            elif name == "contrast" and rng.random() < 0.5:
                contrast = 1                                             # (`supported`: the list names it once)
            elif name == "rot90":
                fx, nw, nh = rotation_row(rng.uniform(-90.0, 90.0), h, w)
                rotated = True
        a0, a1, a2, a3, a4, a5 = fx
        if post_h:
            a2, a5, a0, a3 = a2 + (nw - 1) * a0, a5 + (nw - 1) * a3, -a0, -a3
        if post_v:
            a2, a5, a1, a4 = a2 + (nh - 1) * a1, a5 + (nh - 1) * a4, -a1, -a4
        table[i] = (vflip, hflip, a0, a1, a2, a3, a4, a5, nw, nh, contrast, 0)
    return Params(table, h, w, "rot90" in names)


# ------------------------------------------------------------------------------------------------ resize tables
def resize_tables(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """`ops.pil_resize_tables` without the Python loops (the same float64 operations in the same order, on arrays)
    -> (bounds int32 [out, 2] = (lo, count), coeffs int32 [out, ksize])"""
    scale = float(in_size) / float(out_size)
    filterscale = scale if scale >= 1.0 else 1.0
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = 0.0 + (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)          # (int) of C: toward zero, as astype does
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    t = np.abs(((x + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss)
    wgt = np.where((t < 1.0) & (x < xmax[:, None]), 1.0 - t, 0.0)
    ww = np.zeros(out_size, np.float64)
    for j in range(ksize):                                                   # the running sum in Pillow's order
        ww = ww + wgt[:, j]
    v = np.where(ww[:, None] != 0.0, wgt / np.where(ww == 0.0, 1.0, ww)[:, None], wgt)
    kk = (0.5 + v * float(1 << 22)).astype(np.int64)                         # (the bilinear weights are >= 0)
    kk[x >= xmax[:, None]] = 0
    return np.stack([xmin, xmax], 1).astype(np.int32), kk.astype(np.int32)


class TablePool:
    """the (bounds, coeffs) tables of every (n_in, n_out) met so far in ONE int32 device buffer: a table is built (numpy) and uploaded the
    first time its key appears, `offsets` -> (bounds offset, coeffs offset, ksize).  The buffer doubles when it is full; offsets stay valid."""

    def __init__(self, device, capacity: int = 1 << 20):
        import torch
        self.device = device
        self.buf = torch.empty(capacity, dtype=torch.int32, device=device)
        self.used = 0
        self.index: Dict[Tuple[int, int], Tuple[int, int, int]] = {}

    def offsets(self, keys: Sequence[Tuple[int, int]]) -> List[Tuple[int, int, int]]:
        import torch
        new, at = [], self.used
        for key in keys:
            if key not in self.index:
                bd, kk = resize_tables(*key)
                self.index[key] = (at, at + bd.size, kk.shape[1])
                new += [bd.ravel(), kk.ravel()]
                at += bd.size + kk.size
        if new:
            if at > self.buf.numel():
                grown = torch.empty(max(at, 2 * self.buf.numel()), dtype=torch.int32, device=self.device)
                grown[:self.used] = self.buf[:self.used]
                self.buf = grown
            self.buf[self.used:at] = torch.from_numpy(np.concatenate(new)).to(self.device)       # one upload for all new tables
            self.used = at
        return [self.index[k] for k in keys]


_POOLS: Dict[object, TablePool] = {}


# ------------------------------------------------------------------------------------------------ the arithmetic in numpy
def reference_luts(frames: np.ndarray, params: Params) -> np.ndarray:
    """uint8 [B,3,256]: `ImageOps.autocontrast` tables of the frames whose contrast flag is set, the identity elsewhere"""
    b = len(frames)
    luts = np.tile(np.arange(256, dtype=np.uint8), (b, 3, 1))
    for i in range(b):
        if not params.table[i, 10]:
            continue
        for c in range(3):
            lo, hi = int(frames[i, :, :, c].min()), int(frames[i, :, :, c].max())
            if hi <= lo:
                continue
            scale = 255.0 / (hi - lo)
            offset = -lo * scale
            luts[i, c] = [min(255, max(0, int(ix * scale + offset))) for ix in range(256)]
    return luts


def canvas_dims(params: Params) -> Tuple[int, int]:
    """(Hc, Wc) of the padded canvas: the batch maxima of (nh, nw), the width rounded up to 4 pixels when a resize follows (its rows are then
    whole dwords)"""
    if not params.rotated:
        return params.h, params.w
    return int(params.table[:, 9].max()), (int(params.table[:, 8].max()) + 3) // 4 * 4


def reference_canvas(frames: np.ndarray, luts: np.ndarray, params: Params) -> np.ndarray:
    """uint8 [B,Hc,Wc,3]: flips + LUT + the fixed-point gather of every frame, zero outside its nw x nh"""
    b, h, w, _ = frames.shape
    hc, wc = canvas_dims(params)
    out = np.zeros((b, hc, wc, 3), np.uint8)
    for i in range(b):
        vflip, hflip, a0, a1, a2, a3, a4, a5, nw, nh = (int(v) for v in params.table[i, :10])
        X, Y = np.arange(nw, dtype=np.int64)[None, :], np.arange(nh, dtype=np.int64)[:, None]
        xin, yin = (a2 + X * a0 + Y * a1) >> 16, (a5 + X * a3 + Y * a4) >> 16
        ok = (xin >= 0) & (xin < w) & (yin >= 0) & (yin < h)
        xs, ys = np.clip(xin, 0, w - 1), np.clip(yin, 0, h - 1)
        if hflip:
            xs = w - 1 - xs
        if vflip:
            ys = h - 1 - ys
        px = frames[i][ys, xs]                                               # [nh, nw, 3]
        px = np.stack([luts[i, c][px[..., c]] for c in range(3)], -1)
        out[i, :nh, :nw] = np.where(ok[..., None], px, 0)
    return out


def reference_resize_pass(img: np.ndarray, n_out: int, axis: int) -> np.ndarray:
    """one pass of Pillow's 8-bit bilinear resize over one image [H,W,3]: axis 0 along the width, axis 1 along the height"""
    n_in = img.shape[1 - axis]
    bd, kk = resize_tables(n_in, n_out)
    idx = np.minimum(bd[:, :1].astype(np.int64) + np.arange(kk.shape[1])[None, :], n_in - 1)      # [out, ksize]; kk is 0 beyond the count
    src = img.astype(np.int64)
    if axis == 0:
        ss = (src[:, idx, :] * kk.astype(np.int64)[None, :, :, None]).sum(2)
    else:
        ss = (src[idx, :, :] * kk.astype(np.int64)[:, :, None, None]).sum(1)
    return np.clip(((1 << 21) + ss) >> 22, 0, 255).astype(np.uint8)


def reference_u8(frames: np.ndarray, params: Params, stages: bool = False):
    """the whole transform in numpy integers: uint8 [B,h,w,3] -> uint8 [B,h,w,3].  stages=True -> the dict of every stage: 'luts' [B,3,256],
    'canvas' [B,Hc,Wc,3], 'rotated' (the list of [nh,nw,3] images = what Pillow holds before the second Resize), 'hpass' (list of [nh,w,3]),
    'out'"""
    frames = np.ascontiguousarray(frames)
    b, h, w, _ = frames.shape
    assert (h, w) == (params.h, params.w) and b == len(params)
    luts = reference_luts(frames, params)
    canvas = reference_canvas(frames, luts, params)
    rotated = [canvas[i, :nh, :nw] for i, (nh, nw) in enumerate(params.sizes())]
    if params.rotated:
        hpass = [reference_resize_pass(im, w, 0) for im in rotated]
        out = np.stack([reference_resize_pass(im, h, 1) for im in hpass])
    else:
        hpass, out = rotated, canvas
    return {"luts": luts, "canvas": canvas, "rotated": rotated, "hpass": hpass, "out": out} if stages else out


# ------------------------------------------------------------------------------------------------ the device form
def channel_luts_device(frames, table_dev):
    """`mt4_aug_channel_luts`: uint8 [B,H,W,3] on the GPU, the parameter rows on the GPU -> uint8 [B,3,256]"""
    import torch
    from . import ops
    b, h, w, _ = frames.shape
    minmax = torch.empty((b, 3, 2), dtype=torch.int32, device=frames.device)
    luts = torch.empty((b, 3, 256), dtype=torch.uint8, device=frames.device)
    ops.check(ops.lib.mt4_aug_channel_luts(frames.data_ptr(), table_dev.data_ptr(), minmax.data_ptr(), luts.data_ptr(), b, h, w, ops._stream()),
              "mt4_aug_channel_luts")
    return luts


def flip_lut_rotate_device(frames, luts, table_dev, hc: int, wc: int):
    """`mt4_aug_flip_lut_rotate` -> the canvas uint8 [B,hc,wc,3]"""
    import torch
    from . import ops
    b, h, w, _ = frames.shape
    canvas = torch.empty((b, hc, wc, 3), dtype=torch.uint8, device=frames.device)
    ops.check(ops.lib.mt4_aug_flip_lut_rotate(frames.data_ptr(), luts.data_ptr(), table_dev.data_ptr(), canvas.data_ptr(), b, h, w, hc, wc,
                                              ops._stream()), "mt4_aug_flip_lut_rotate")
    return canvas


def frame_tables(params: Params, device):
    """the per-frame rows `mt4_aug_resize_pass_u8` reads ([B,8] int32 on the device), the table pool's buffer and the largest (h, v) ksize"""
    import torch
    # one pool per (device, stream): a pool's uploads and the kernels that read it are ordered by that stream alone, so loads that run on side
    # streams of their own (`loader.FrameLoader`) neither share a buffer across streams nor grow one under another thread's feet
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    pool = _POOLS.get(key)
    if pool is None:
        pool = _POOLS[key] = TablePool(device)
    sizes = params.sizes()
    offs = pool.offsets([(nw, params.w) for _, nw in sizes] + [(nh, params.h) for nh, _ in sizes])
    b = len(sizes)
    ft = np.array([[*offs[i], sizes[i][1], *offs[b + i], sizes[i][0]] for i in range(b)], np.int32)
    return torch.from_numpy(ft).to(device), pool.buf, (int(ft[:, 2].max()), int(ft[:, 6].max()))


def resize_pass_device(x, pool_buf, ft_dev, n_out: int, ksize_max: int, axis: int):
    """`mt4_aug_resize_pass_u8`: axis 0 [B,Hc,Wc,3] -> [B,Hc,n_out,3] (rows below a frame's nh are not written), axis 1 -> [B,n_out,W,3]"""
    import torch
    from . import ops
    b, hc, wc, _ = x.shape
    hout, wout = (hc, n_out) if axis == 0 else (n_out, wc)
    y = torch.empty((b, hout, wout, 3), dtype=torch.uint8, device=x.device)
    ops.check(ops.lib.mt4_aug_resize_pass_u8(x.data_ptr(), y.data_ptr(), pool_buf.data_ptr(), ft_dev.data_ptr(), b, hc, wc, hout, wout, ksize_max,
                                             axis, ops._stream()), "mt4_aug_resize_pass_u8")
    return y


def train_transform_device(frames, params: Params, stages: bool = False):
    """uint8 [B,h,w,3] on the GPU -> uint8 [B,h,w,3]: the bytes of `reference_u8` (= Pillow's).  Nothing is read back from the device: the canvas size
    and the tables come from `params`; the parameter rows and the frame-table rows go up as two small host-to-device copies per call.  stages=True -> the dict of 'luts', 'canvas', 'hpass', 'out' tensors."""
    import torch
    from . import ops
    ops._need_cuda(frames)
    assert frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3 and frames.is_contiguous()
    b, h, w, _ = frames.shape
    assert (h, w) == (params.h, params.w) and b == len(params) and b > 0
    table_dev = torch.from_numpy(params.table).to(frames.device)
    luts = channel_luts_device(frames, table_dev)
    hc, wc = canvas_dims(params)
    canvas = flip_lut_rotate_device(frames, luts, table_dev, hc, wc)
    hpass = out = canvas
    if params.rotated:
        ft_dev, pool_buf, (kh, kv) = frame_tables(params, frames.device)
        hpass = resize_pass_device(canvas, pool_buf, ft_dev, w, kh, 0)
        out = resize_pass_device(hpass, pool_buf, ft_dev, h, kv, 1)
    return {"luts": luts, "canvas": canvas, "hpass": hpass, "out": out} if stages else out


def load_train_batch_device(data_dir: str, samples: Sequence[Tuple[str, int]], height: int, width: int, rng, names: Sequence[str],
                            decode: str = "host", workers: int = 8, device="cuda"):
    """the (video, frame id) samples of a training batch -> uint8 [B,height,width,3] on the GPU, the bytes of
    `drivers.load_train_frames_u8` sample by sample with the same rng: the PNGs are decoded by `pngdec.decode_files` (decode = "device")
    or by Pillow threads and resized group by native size (`cholect.load_files_device`), then `train_transform_device`."""
    from . import cholect
    paths = [os.path.join(data_dir, "data", v, "{}.png".format(str(int(fid)).zfill(6))) for v, fid in samples]
    x = cholect.load_files_device(paths, height, width, device=device, workers=workers, decode=decode)
    return train_transform_device(x, draw_params(rng, names, len(paths), height, width))
