"""The train transform of the frame trainers (`Spatial_cnn/dataloader.py:89-100,153-162`: Resize -> vflip -> hflip -> autocontrast ->
sharpening (the list's 'brightness') -> rotation by a random angle with expand -> Resize) as a function of (frames, random draws) that runs on the device and returns the bytes
Pillow returns (`drivers.load_train_frames_u8`, the `--train_transform host` path).

`draw_params` consumes the `random.Random` of the host path draw for draw and does the float64 matrix work of `Image.rotate`;
`reference_u8` is the integer arithmetic in numpy (CPU tests, bug hunting); `train_transform_device` launches the kernels of
csrc/augment_kernels.hip; `load_train_batch_device` is the loader `drivers._frame_batch` routes to.  This module imports without
libmt4hip.so: `ops` is imported where a launch happens."""
from __future__ import annotations

import math
import os
from typing import Dict, List, Sequence, Tuple

import numpy as np

NPARAMS = 12            # MT4_AUG_PARAMS (include/mt4hip.h): vflip, hflip, a0..a5, nw, nh, contrast, sharpen
# column 11, the draw of 'brightness': 0 = not drawn (always, for a list without the name); 1 = sharpen the frame as it stands -- its autocontrast,
# if drawn, comes later and takes its range from the sharpened frame; 2 = the frame's autocontrast was drawn before it: the sharpening reads the
# frame through its LUTs, and the gather kernel does not apply them again
SHARP_ROWS, SHARP_COLS = 16, 64          # the tile of the sharpening kernel (AUG_SH_ROWS, AUG_SH_COLS of csrc/augment_kernels.hip)


def supported(names: Sequence[str]) -> bool:
    """the lists the device form covers: at most one `rot90`, at most one `contrast`, and no `contrast` after the `rot90` (the black fill of
    the rotation would enter the histogram).  A second autocontrast is NOT the identity: `int(hi * scale + offset)` is 254 for about 15 % of
    the (lo, hi) pairs, so the second one stretches again; the kernels hold one LUT per channel, so such a list keeps the host path.  Flips may
    stand anywhere; `original` and names `_augment` ignores are no-ops.  At most one `brightness`, before the `rot90`: after it the sharpening
    would act on the black fill and the rotated edge.  It may stand on either side of `contrast`, and anywhere among the flips: the stencil
    and its border rule are symmetric and the result depends on the integers alone, so it commutes with both flips exactly."""
    seen_rot = seen_contrast = seen_sharp = False
    for n in names:
        if n == "rot90":
            if seen_rot:
                return False
            seen_rot = True
        elif n == "contrast":
            if seen_rot or seen_contrast:
                return False
            seen_contrast = True
        elif n == "brightness":
            if seen_rot or seen_sharp:
                return False
            seen_sharp = True
    return True


class Params:
    """table int32 [B, NPARAMS] (the rows the kernels read), the frame size (h, w) it was built for, rotated = the list has `rot90`,
    sharpened = some frame drew the sharpening (column 11)"""

    def __init__(self, table: np.ndarray, h: int, w: int, rotated: bool):
        self.table, self.h, self.w, self.rotated = table, h, w, rotated
        self.sharpened = bool(table[:, 11].any())

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
    per hflip, `random() < 0.5` per contrast, `random() < 0.5` per brightness, `uniform(-90, 90)` per rot90): afterwards rng is in the state the host path leaves.  A flip
    listed after `rot90` acts on the rotated image; it is folded into the affine map (X -> nw-1-X, Y -> nh-1-Y), which is exact in integers."""
    if not supported(names):
        raise ValueError(f"augmentation list {list(names)}: 'contrast' or 'brightness' after 'rot90' (or 'contrast' / 'brightness' / 'rot90' twice) "
                         "has no device form")
    table = np.zeros((n, NPARAMS), np.int32)
    for i in range(n):
        vflip = hflip = contrast = sharpen = 0
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
            elif name == "brightness" and rng.random() < 0.5:
                sharpen = 2 if contrast else 1                           # (column 11, see NPARAMS)
            elif name == "rot90":
                fx, nw, nh = rotation_row(rng.uniform(-90.0, 90.0), h, w)
                rotated = True
        a0, a1, a2, a3, a4, a5 = fx
        if post_h:
            a2, a5, a0, a3 = a2 + (nw - 1) * a0, a5 + (nw - 1) * a3, -a0, -a3
        if post_v:
            a2, a5, a1, a4 = a2 + (nh - 1) * a1, a5 + (nh - 1) * a4, -a1, -a4
        table[i] = (vflip, hflip, a0, a1, a2, a3, a4, a5, nw, nh, contrast, sharpen)
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


def sharpen_u8(img: np.ndarray) -> np.ndarray:
    """`ImageEnhance.Sharpness(im).enhance(1.6)` of one image uint8 [H,W,C] in integers: N = the 3 x 3 neighbourhood sum + 4 x centre (SMOOTH is
    [1 1 1; 1 5 1; 1 1 1] / 13), deg = (2 N + 13) // 26 (Pillow's float32 `0.5 + N / 13` truncated: 13 is odd, so the sum is never within 1/26
    of an integer), out = clamp(trunc((5 deg + 8 (p - deg)) / 5)) (the blend p + 0.6 (p - deg), truncated toward zero); the one-pixel border is
    the source, an image with H < 3 or W < 3 comes back unchanged"""
    h, w = img.shape[:2]
    out = img.copy()
    if h < 3 or w < 3:
        return out
    a = img.astype(np.int64)
    n = 4 * a[1:-1, 1:-1]
    for dy in range(3):
        for dx in range(3):
            n = n + a[dy:h - 2 + dy, dx:w - 2 + dx]
    deg = (2 * n + 13) // 26
    t = 5 * deg + 8 * (a[1:-1, 1:-1] - deg)
    t = np.where(t >= 0, t // 5, -((-t) // 5))                              # toward zero
    out[1:-1, 1:-1] = np.clip(t, 0, 255).astype(np.uint8)
    return out


def _lut_first(params: Params) -> bool:
    """the call applies the autocontrast before the sharpening (some row has sharpen == 2).  A list has ONE order, so `draw_params` never puts
    such a row beside a row whose autocontrast follows its sharpening (sharpen == 1 with the contrast flag)"""
    t = params.table
    first = bool((t[:, 11] == 2).any())
    assert not (first and ((t[:, 11] == 1) & (t[:, 10] != 0)).any()), "rows of both autocontrast / sharpening orders in one table"
    return first


def reference_sharp(frames: np.ndarray, luts, params: Params) -> np.ndarray:
    """uint8 [B,h,w,3], what `mt4_aug_sharpen_u8` writes: the sharpened image of every frame whose sharpen column is set (of the frame read
    through its LUTs when the column is 2 and luts is given), a copy of the others"""
    out = frames.copy()
    for i in range(len(frames)):
        mode = int(params.table[i, 11])
        if mode:
            src = frames[i]
            if mode == 2 and luts is not None:
                src = np.stack([luts[i, c][src[..., c]] for c in range(3)], -1)
            out[i] = sharpen_u8(src)
    return out


def canvas_luts(luts: np.ndarray, params: Params) -> np.ndarray:
    """the tables the gather applies: `luts`, the identity for the frames whose LUTs the sharpening already applied"""
    done = params.table[:, 11] == 2
    if not done.any():
        return luts
    luts = luts.copy()
    luts[done] = np.arange(256, dtype=np.uint8)
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
    'out'; and, when a frame drew the sharpening, 'sharp' [B,h,w,3] = the frames after it (`reference_sharp`).  'luts' then holds the tables of
    the frames as stored when the autocontrast comes first, of the sharpened frames when it comes second."""
    frames = np.ascontiguousarray(frames)
    b, h, w, _ = frames.shape
    assert (h, w) == (params.h, params.w) and b == len(params)
    sharp = None
    if params.sharpened:
        if _lut_first(params):
            luts = reference_luts(frames, params)
            frames = sharp = reference_sharp(frames, luts, params)
        else:
            frames = sharp = reference_sharp(frames, None, params)
            luts = reference_luts(frames, params)
    else:
        luts = reference_luts(frames, params)
    canvas = reference_canvas(frames, canvas_luts(luts, params), params)
    rotated = [canvas[i, :nh, :nw] for i, (nh, nw) in enumerate(params.sizes())]
    if params.rotated:
        hpass = [reference_resize_pass(im, w, 0) for im in rotated]
        out = np.stack([reference_resize_pass(im, h, 1) for im in hpass])
    else:
        hpass, out = rotated, canvas
    if not stages:
        return out
    st = {"luts": luts, "canvas": canvas, "rotated": rotated, "hpass": hpass, "out": out}
    if sharp is not None:
        st["sharp"] = sharp
    return st


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


def sharpen_device(frames, luts, table_dev):
    """`mt4_aug_sharpen_u8`: uint8 [B,H,W,3] on the GPU, the LUTs [B,3,256] or None -> a new uint8 [B,H,W,3] (a stencil cannot run in place)"""
    import torch
    from . import ops
    b, h, w, _ = frames.shape
    out = torch.empty_like(frames)
    ops.check(ops.lib.mt4_aug_sharpen_u8(frames.data_ptr(), luts.data_ptr() if luts is not None else None, table_dev.data_ptr(), out.data_ptr(),
                                         b, h, w, ops._stream()), "mt4_aug_sharpen_u8")
    return out


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
    and the tables come from `params`; the parameter rows and the frame-table rows go up as two small host-to-device copies per call.  stages=True -> the dict of 'luts', 'canvas', 'hpass', 'out' tensors.
    When a frame of the call drew the sharpening, one more launch and one more [B,h,w,3] buffer ('sharp' under stages=True): LUTs of the frames
    as stored, then the sharpening through them, when the list has `contrast` first; the sharpening, then the LUTs of its output, otherwise."""
    import torch
    from . import ops
    ops._need_cuda(frames)
    assert frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3 and frames.is_contiguous()
    b, h, w, _ = frames.shape
    assert (h, w) == (params.h, params.w) and b == len(params) and b > 0
    table_dev = torch.from_numpy(params.table).to(frames.device)
    sharp = None
    if params.sharpened:
        if _lut_first(params):
            luts = channel_luts_device(frames, table_dev)
            frames = sharp = sharpen_device(frames, luts, table_dev)
        else:
            frames = sharp = sharpen_device(frames, None, table_dev)
            luts = channel_luts_device(frames, table_dev)
    else:
        luts = channel_luts_device(frames, table_dev)
    hc, wc = canvas_dims(params)
    canvas = flip_lut_rotate_device(frames, luts, table_dev, hc, wc)
    hpass = out = canvas
    if params.rotated:
        ft_dev, pool_buf, (kh, kv) = frame_tables(params, frames.device)
        hpass = resize_pass_device(canvas, pool_buf, ft_dev, w, kh, 0)
        out = resize_pass_device(hpass, pool_buf, ft_dev, h, kv, 1)
    if not stages:
        return out
    st = {"luts": luts, "canvas": canvas, "hpass": hpass, "out": out}
    if sharp is not None:
        st["sharp"] = sharp
    return st


def load_train_batch_device(data_dir: str, samples: Sequence[Tuple[str, int]], height: int, width: int, rng, names: Sequence[str],
                            decode: str = "host", workers: int = 8, device="cuda"):
    """the (video, frame id) samples of a training batch -> uint8 [B,height,width,3] on the GPU, the bytes of
    `drivers.load_train_frames_u8` sample by sample with the same rng: the PNGs are decoded by `pngdec.decode_files` (decode = "device")
    or by Pillow threads and resized group by native size (`cholect.load_files_device`), then `train_transform_device`."""
    from . import cholect
    paths = [os.path.join(data_dir, "data", v, "{}.png".format(str(int(fid)).zfill(6))) for v, fid in samples]
    x = cholect.load_files_device(paths, height, width, device=device, workers=workers, decode=decode)
    return train_transform_device(x, draw_params(rng, names, len(paths), height, width))
