"""The fused layer1 Bottleneck with unconditional (clamped) halo loads and its biases in LDS: all three forms of `bottleneck64_fused_kernel`
against conv1 -> conv2 -> conv3 (+ downsample, + the following conv1) through `conv_nhwc`, bit for bit, on inputs on which a clamped halo value
reaching conv2's zero padding, a read from the neighbouring image reaching a stored pixel, or a bias read from the wrong LDS slot changes the
result far beyond rounding."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [
    (2, 8, 14),      # one exact tile
    (1, 9, 15),      # ragged both ways; a second tile row and column of one pixel
    (1, 17, 29),     # 3 x 3 tiles; an interior tile with all four neighbours
    (1, 1, 1),       # single pixel: every halo load is clamped onto it
    (3, 56, 56),     # the bench geometry: 28 tiles per image; first, middle and last image
]
FORMS = ["identity", "downsample", "next"]
IMAGE_SCALE = (1.0, 3.0, 0.5)


def _biases(dev):
    """b1 | b2 | b3 | bds | bn: every value of every vector different from every other (multiples of 1 / 512, exact in fp32), none zero, signs mixed"""
    n = torch.arange(1, 64 + 64 + 256 + 256 + 128 + 1, dtype=torch.float32)
    v = n / 512 * torch.where(n.long() % 3 == 0, -1.0, 1.0)
    assert v.abs().unique().numel() == v.numel() and bool((v != 0).all())
    return [t.contiguous().to(dev) for t in v.split([64, 64, 256, 256, 128])]


@functools.lru_cache(maxsize=None)
def _case(form, b, h, w):
    """(x, packed block, packed following conv | None, reference outputs) -- built once, shared by the tests below and never written to"""
    from computervision_codes_amd import ops
    dev = torch.device("cuda:0")
    bf = torch.bfloat16
    cin = 64 if form == "downsample" else 256
    g = torch.Generator().manual_seed(100 * h + w + len(form))
    x = torch.randn((b, h, w, cin), generator=g)
    ring = torch.ones((h, w))
    ring[1:-1, 1:-1] = 0                                 # the outermost ring of pixels (all of a 1 x 1 or 2-pixel-wide image)
    x = x * (1 + 63 * ring)[None, :, :, None]
    x = x * torch.tensor([IMAGE_SCALE[i % 3] for i in range(b)])[:, None, None, None]
    # the batch stands between two images of NaN: a halo load that leaves the first or the last image shows in whatever it reaches
    buf = torch.full((b + 2, h, w, cin), float("nan"), dtype=bf, device=dev)
    buf[1:b + 1] = x.to(dev).to(bf)
    x = buf[1:b + 1]
    assert x.is_contiguous()

    def mk(cout, ci, k, s, bias):
        wt = (torch.randn((cout, ci, k, k), generator=g) * s).to(dev)
        return ops.pack_conv_weight(wt, None, bf), bias
    b1, b2, b3, bds, bn = _biases(dev)
    c1, c2, c3 = mk(64, cin, 1, cin ** -0.5, b1), mk(64, 64, 3, 1 / 24, b2), mk(256, 64, 1, 1 / 8, b3)
    cd = mk(256, cin, 1, cin ** -0.5, bds) if form == "downsample" else None
    cn = mk(128, 256, 1, 1 / 16, bn) if form == "next" else None
    idt = ops.conv_nhwc(x, cd[0], cd[1], kh=1, kw=1, relu=False) if cd is not None else x
    o = ops.conv_nhwc(x, c1[0], c1[1], kh=1, kw=1, relu=True)
    o = ops.conv_nhwc(o, c2[0], c2[1], kh=3, kw=3, pad=(1, 1), relu=True)
    ref = ops.conv_nhwc(o, c3[0], c3[1], kh=1, kw=1, residual=idt, relu=True)
    assert bool(torch.isfinite(ref.float()).all()) and float(ref.float().abs().max()) > 0.5
    refs = (ref,)
    if cn is not None:
        ref_t = ops.conv_nhwc(ref, cn[0], cn[1], kh=1, kw=1, relu=True)
        assert float(ref_t.float().abs().max()) > 0.5
        refs = (ref[:, ::2, ::2].contiguous(), ref_t)
    return x, ops.bottleneck_pack(c1, c2, c3, cd), (ops.bottleneck_pack_next(cn) if cn is not None else None), refs


def _launch(form, x, packed, packed_next):
    from computervision_codes_amd import ops
    if form == "next":
        return tuple(ops.bottleneck_fused_next(x, packed, packed_next))
    return (ops.bottleneck_fused(x, packed),)


@pytest.mark.parametrize("b,h,w", SHAPES)
@pytest.mark.parametrize("form", FORMS)
def test_fused_forms_bit_identical_to_separate_launches(cuda, form, b, h, w):
    """identity, downsample and `bottleneck_fused_next` (both outputs) == the separate launches, bit for bit.  The ring of every image is 64 x the
    interior and consecutive images differ in scale, so a clamped halo pixel that is not zeroed before conv2, or a pixel of the wrong image, moves
    the result by far more than a rounding; the biases are 768 different non-zero values, so no two LDS slots hold the same one."""
    x, packed, packed_next, refs = _case(form, b, h, w)
    got = _launch(form, x, packed, packed_next)
    assert len(got) == len(refs)
    for y, ref in zip(got, refs):
        assert y.shape == ref.shape
        assert torch.equal(y.view(torch.int16), ref.view(torch.int16)), float((y.float() - ref.float()).abs().max())


@pytest.mark.parametrize("b,h,w", SHAPES)
@pytest.mark.parametrize("form", FORMS)
def test_fused_forms_are_deterministic(cuda, form, b, h, w):
    """two launches on the same input give equal bytes"""
    x, packed, packed_next, _ = _case(form, b, h, w)
    first = _launch(form, x, packed, packed_next)
    second = _launch(form, x, packed, packed_next)
    for y0, y1 in zip(first, second):
        assert torch.equal(y0.view(torch.int16), y1.view(torch.int16))
