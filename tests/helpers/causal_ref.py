"""float64 reference of the CAUSAL temporal head for the tests, written from the formula
    y[t] = b + sum_k W_k x[t - (2 - k) d],  zeros before frame 0
with `F.pad` (2 d frames in front) + `F.conv1d`; everything else is the head's documented structure (stage stack, FPN at equal lengths, four
heads, BCE over the four levels, SGD without momentum).  `causal=False` pads d on both sides (the symmetric head), for tests that must show
they can tell the two apart."""
from typing import Dict, Optional

import torch
import torch.nn.functional as F

HEADS = (("", 100, 1.0), ("_i", 6, 0.1), ("_v", 10, 0.1), ("_t", 15, 0.1))


def dilated(z, w, b, d, causal=True):
    """z [1, C, T]; w [Cout, Cin, 3]"""
    return F.conv1d(F.pad(z, (2 * d, 0)) if causal else F.pad(z, (d, d)), w, b, dilation=d)


def forward(sd: Dict[str, torch.Tensor], x: torch.Tensor, num_layers_PG: int, num_layers_R: int, num_R: int, masks: Optional[dict] = None,
            causal: bool = True):
    """x [1, T, D] -> ({head suffix: [p1, p2, p3, p4] logits [1, K, T]}, [c1 .. p4 features]) in x's dtype (pass float64 tensors for float64)"""
    masks = masks or {}
    h = x.permute(0, 2, 1)
    if masks.get("input_mask") is not None:
        h = h * masks["input_mask"].to(h.dtype)
    if masks.get("channel_mask") is not None:
        h = h * masks["channel_mask"].to(h.dtype)
    lm = masks.get("layer_masks") or {}

    def stage(prefix, z, n):
        for i in range(n):
            p = f"{prefix}.layers.{i}"
            u = F.relu(dilated(z, sd[p + ".conv_dilated.weight"], sd[p + ".conv_dilated.bias"], 2 ** i, causal))
            o = F.conv1d(u, sd[p + ".conv_1x1.weight"], sd[p + ".conv_1x1.bias"])
            if p in lm:
                o = o * lm[p].to(o.dtype)
            z = z + o
        return z

    f = stage("PG", F.conv1d(h, sd["PG.conv_1x1.weight"], sd["PG.conv_1x1.bias"]), num_layers_PG)
    cs = [f]
    for r in range(num_R):
        f = stage(f"Rs.{r}", f, num_layers_R)
        cs.append(f)
    w, b = sd["fpn.latlayer1.weight"], sd["fpn.latlayer1.bias"]
    levels = [cs[-1]]
    for c in reversed(cs[:-1]):
        levels.insert(0, levels[0] + F.conv1d(c, w, b))
    return {s: [F.conv1d(l, sd[f"conv_out{s}.weight"], sd[f"conv_out{s}.bias"]) for l in levels] for s, _, _ in HEADS}, levels


def to64(sd):
    return {k: v.double() for k, v in sd.items()}


def train_step(sd, x, labels, lr, weight_decay=1e-5, masks=None, causal=True, **cfg):
    """one SGD step in float64 by autograd: -> (new_sd, loss, grads); a parameter without gradient is left untouched (torch.optim.SGD)"""
    params = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    logits, _ = forward(params, x.double(), masks=masks, causal=causal, **cfg)
    total = sum(wgt * sum(F.binary_cross_entropy_with_logits(l[0].transpose(0, 1), labels[s].double()) for l in logits[s]) for s, _, wgt in HEADS)
    names = list(params)
    grads = torch.autograd.grad(total, [params[k] for k in names], allow_unused=True)
    g = {k: gr for k, gr in zip(names, grads) if gr is not None}
    new = {k: (params[k].detach() - lr * (g[k] + weight_decay * params[k].detach())) if k in g else params[k].detach().clone() for k in names}
    return new, float(total.detach()), g
