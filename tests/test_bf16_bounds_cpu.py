"""CPU: the per-element bf16 bound of `bf16_bounds` accepts a correct bf16 GEMM epilogue (fp32 accumulation, bias in fp32, one
round-to-nearest-even at the store) and rejects each of five subtly wrong ones, all emulated with torch's fp32 matmul on 2048 x 256 outputs;
and the single tolerance the bf16 GPU tests used before (1.2e-2 x max|ref|) accepts every one of the wrong ones."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bf16_bounds import check_bf16, check_f32, half_ulp_bf16, rne_bf16  # noqa: E402

M, N = 2048, 256


def _operands(k, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn((M, k), generator=g).bfloat16().float()
    w = (torch.randn((k, N), generator=g) * k ** -0.5).bfloat16().float()
    bias = torch.randn(N, generator=g)
    ref64 = a.double() @ w.double() + bias.double()
    acc64 = a.double().abs() @ w.double().abs() + bias.double().abs()
    return a, w, bias, ref64, acc64


def _trunc_bf16(t32):
    return (t32.contiguous().view(torch.int32) & -65536).view(torch.float32)


def _correct(a, w, bias):
    return (a @ w + bias).bfloat16()


def _truncating_store(a, w, bias):
    return _trunc_bf16(a @ w + bias)


def _bf16_partials(a, w, bias, chunk=256):
    acc = torch.zeros((M, N))
    for k0 in range(0, a.shape[1], chunk):
        acc += (a[:, k0:k0 + chunk] @ w[k0:k0 + chunk]).bfloat16().float()
    return (acc + bias).bfloat16()


def _rounded_before_bias(a, w, bias):
    return ((a @ w).bfloat16().float() + bias).bfloat16()


def _bf16_bias(a, w, bias):
    return (a @ w + bias.bfloat16().float()).bfloat16()


def _old_tolerance_accepts(got, ref64):
    return (got.double() - ref64).abs().max().item() < 1.2e-2 * max(1.0, ref64.abs().max().item())


def test_rne_and_half_ulp():
    x = torch.tensor([1.0, 1.0 + 2 ** -8, 1.0 + 3 * 2 ** -8, 1.0 + 2 ** -8 + 2 ** -40, -3.0, 0.0, 2 ** -130], dtype=torch.float64)
    assert rne_bf16(x).tolist() == [1.0, 1.0, 1.0 + 4 * 2 ** -8, 1.0 + 2 ** -7, -3.0, 0.0, 2 ** -130]   # ties to even; just above a tie rounds up
    assert half_ulp_bf16(x).tolist()[:5] == [2 ** -8, 2 ** -8, 2 ** -8, 2 ** -8, 2 ** -7]
    assert half_ulp_bf16(x)[5].item() == half_ulp_bf16(x)[6].item() == 2.0 ** -134                     # floored at the smallest normal
    r = torch.randn(10000, dtype=torch.float64) * 10.0 ** torch.randint(-3, 4, (10000,)).double()
    assert torch.equal(rne_bf16(r.float()), r.float().bfloat16().double())                              # == torch's fp32 -> bf16 RNE


@pytest.mark.parametrize("k", [64, 576, 4608])
def test_correct_kernel_passes(k):
    a, w, bias, ref64, acc64 = _operands(k, 100 + k)
    st = check_bf16(_correct(a, w, bias), ref64, acc64=acc64, k=k, what=f"correct K={k}")
    assert st["worst_ratio"] <= 1.0 and st["match"] >= 0.999 and abs(st["mean_signed_ulp"]) < 0.01
    check_f32(a @ w + bias, ref64, acc64=acc64, k=k, what=f"correct fp32 out K={k}")


@pytest.mark.parametrize("bug,k", [(_truncating_store, 576), (_bf16_partials, 576), (_bf16_partials, 4608), (_rounded_before_bias, 576),
                                   (_bf16_bias, 576)])
def test_emulated_bug_rejected_but_passes_old_tolerance(bug, k):
    a, w, bias, ref64, acc64 = _operands(k, 200 + k)
    got = bug(a, w, bias)
    assert _old_tolerance_accepts(got, ref64)
    with pytest.raises(AssertionError, match="bound exceeded or biased"):
        check_bf16(got, ref64, acc64=acc64, k=k, what=bug.__name__)


def test_three_outputs_one_ulp_off_rejected():
    k = 576
    a, w, bias, ref64, acc64 = _operands(k, 300)
    got = _correct(a, w, bias)
    bits = got.view(torch.int16).clone()
    for (i, j) in ((0, 0), (1000, 100), (2047, 255)):
        bits[i, j] += 1                                    # one bf16 ulp away from zero
    bad = bits.view(torch.bfloat16)
    assert _old_tolerance_accepts(bad, ref64)
    with pytest.raises(AssertionError, match="bound exceeded"):
        check_bf16(bad, ref64, acc64=acc64, k=k, what="3 elements one ulp off")


def test_failure_message_names_the_worst_element():
    ref64 = torch.linspace(-2.0, 2.0, 64, dtype=torch.float64).view(8, 8)
    got = rne_bf16(ref64).float().bfloat16()
    bits = got.view(torch.int16).clone()
    bits[3, 5] += 2
    with pytest.raises(AssertionError, match=r"worst element \(3, 5\)"):
        check_bf16(bits.view(torch.bfloat16), ref64, what="message")
