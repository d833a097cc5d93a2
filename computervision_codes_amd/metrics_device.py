"""`metrics.Recognition` with the scores left where the model wrote them (`--metrics device`): the per-video, per-class average precision
is one `ops.video_ap` launch over all videos and classes of a head, component disentangling one `ops.component_max` launch per operand; the
[V, K] float64 APs come down in one copy and meet the nan-means of `metrics.video_mean`, the lines the host metric runs.  Top-K stays on
the host (`to_host()`)."""
from __future__ import annotations

from typing import List

import numpy as np
import torch

from . import ops
from .metrics import N_NULL_TRIPLETS, Recognition, component_table, video_mean


class DeviceRecognition:
    """the surface the drivers use of `metrics.Recognition`; `update` takes fp32 rows on the device (anything else is converted and uploaded)"""

    def __init__(self, num_class: int = 100, device="cuda"):
        self.num_class = num_class
        self.device = torch.device(device)
        self.reset_global()

    def reset(self):
        self.targets: List[torch.Tensor] = []
        self.predictions: List[torch.Tensor] = []

    def reset_global(self):
        self.global_targets: List[torch.Tensor] = []
        self.global_predictions: List[torch.Tensor] = []
        self._cat = None
        self.reset()

    def _rows(self, a) -> torch.Tensor:
        return torch.as_tensor(a).to(device=self.device, dtype=torch.float32).reshape(-1, self.num_class)

    def update(self, targets, predictions):
        self.targets.append(self._rows(targets))
        self.predictions.append(self._rows(predictions))

    def video_end(self):
        if self.targets:
            self.global_targets.append(torch.cat(self.targets, 0))
            self.global_predictions.append(torch.cat(self.predictions, 0))
            self._cat = None
        self.reset()

    def set_videos(self, vids):
        self.reset_global()
        for t, p in vids:
            self.global_targets.append(self._rows(t))
            self.global_predictions.append(self._rows(p))
        return self

    def _concatenated(self):
        """(targets [N, K], scores [N, K], row offsets) of all videos, built once per set of videos"""
        if self._cat is None:
            offs = np.concatenate([[0], np.cumsum([t.shape[0] for t in self.global_targets])]).astype(np.int64)
            self._cat = (torch.cat(self.global_targets, 0).contiguous(), torch.cat(self.global_predictions, 0).contiguous(), offs)
        return self._cat

    def compute_video_AP(self, component: str = "ivt", ignore_null: bool = False):
        if component != "ivt" and self.num_class != 100:
            raise ValueError("component disentangling needs the 100-way triplet scores")
        if not self.global_targets:
            return video_mean([], self.num_class)
        longest, cap = max(t.shape[0] for t in self.global_targets), ops.video_ap_max_rows()
        if longest > cap:
            print(f"[metrics] a video of {longest} frames exceeds the device AP's {cap} rows: this compute_video_AP runs on the host", flush=True)
            return self.to_host().compute_video_AP(component, ignore_null=ignore_null)
        t, p, offs = self._concatenated()
        k = t.shape[1]
        if component != "ivt":
            table, k = component_table(component)
            t, p = ops.component_max(t, table, k), ops.component_max(p, table, k)
        elif ignore_null and self.num_class == 100:
            k -= N_NULL_TRIPLETS                                       # the null triplets are the last columns: k of ld
        per_video = ops.video_ap(p, t, offs, k).cpu().numpy()
        return video_mean(per_video, self.num_class)

    def to_host(self) -> Recognition:
        """the same videos as float64 numpy in a `metrics.Recognition` (what the reports pickle, and what top-K runs on)"""
        return Recognition(self.num_class).set_videos([(t.cpu().numpy(), p.cpu().numpy()) for t, p in zip(self.global_targets, self.global_predictions)])

    def topK(self, k: int = 5, component: str = "ivt") -> float:
        return self.to_host().topK(k, component)


def device_recognition_from(scores, order):
    """`metrics.recognition_from` with device rows: {video -> {head -> (targets, predictions)}} -> {head -> DeviceRecognition}"""
    from .metrics import HEADS
    missing = [k for k in order if k not in scores]
    if missing:
        raise KeyError(f"videos without predictions: {missing[:4]}")
    heads = [h for h, _ in HEADS if all(h in scores[k] for k in order)]
    return {h: DeviceRecognition(dict(HEADS)[h]).set_videos([scores[k][h] for k in order]) for h in heads}
