"""`metrics.Recognition` with the scores left where the model wrote them (`--metrics device`): the per-video, per-class average precision
is one `ops.video_ap` launch over all videos and classes of a head, component disentangling one `ops.component_max` launch per operand
(kept per component: AP and top-K share the pair), top-K one `ops.rank_hist` launch per component that answers every k; the [V, K] float64
APs and the [K] int64 histograms come down and meet the nan-means of `metrics.video_mean` / one integer division, the lines the host metric
runs.  `to_host()` is for the pickled objects only.  Under several ranks those small arrays -- not the rows -- are what travels
(`summarize` / `gather_device_recognition`)."""
from __future__ import annotations

from typing import List

import numpy as np
import torch

from . import ops
from .metrics import HEADS, N_NULL_TRIPLETS, Recognition, component_table, video_mean

COMPONENTS = ("i", "v", "t", "iv", "it", "ivt")


def _components_of(num_class: int):
    return COMPONENTS if num_class == 100 else ("ivt",)


def _check_component(component: str, num_class: int):
    if component != "ivt" and num_class != 100:
        raise ValueError("component disentangling needs the 100-way triplet scores")


def _top_k(hist: np.ndarray, k: int) -> float:
    """`Recognition.topK` from the rank histogram: two Python integers divided once (k above the column count: everything counts, as the
    host's slice)"""
    total = int(hist.sum())
    return int(hist[:max(int(k), 0)].sum()) / (total if total else 1)


class DeviceRecognition:
    """the surface the drivers use of `metrics.Recognition`; `update` takes fp32 rows on the device (anything else is converted and uploaded)"""

    def __init__(self, num_class: int = 100, device="cuda"):
        self.num_class = num_class
        self.device = torch.device(device)
        self.reset_global()

    def reset(self):
        self.targets: List[torch.Tensor] = []
        self.predictions: List[torch.Tensor] = []

    def _forget(self):
        self._cat, self._comp, self._hist = None, {}, {}

    def reset_global(self):
        self.global_targets: List[torch.Tensor] = []
        self.global_predictions: List[torch.Tensor] = []
        self._forget()
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
            self._forget()
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

    def _component(self, component: str):
        """(targets [N, Kc], scores [N, Kc]) of a component of the 100-way rows: two `ops.component_max` launches per component and set of
        videos, shared by the AP and top-K"""
        if component == "ivt":
            return self._concatenated()[:2]
        if component not in self._comp:
            t, p, _ = self._concatenated()
            table, k = component_table(component)
            self._comp[component] = (ops.component_max(t, table, k), ops.component_max(p, table, k))
        return self._comp[component]

    def per_video_AP(self, component: str = "ivt", ignore_null: bool = False) -> np.ndarray:
        """float64 [V, K]: the rows `compute_video_AP` averages.  A video longer than `ops.video_ap_max_rows()`: on the host, with one line"""
        _check_component(component, self.num_class)
        if not self.global_targets:
            return np.zeros((0, self.num_class))
        longest, cap = max(t.shape[0] for t in self.global_targets), ops.video_ap_max_rows()
        if longest > cap:
            print(f"[metrics] a video of {longest} frames exceeds the device AP's {cap} rows: this compute_video_AP runs on the host", flush=True)
            return np.stack(self.to_host().per_video_AP(component, ignore_null), 0)
        t, p = self._component(component)
        k = t.shape[1]
        if component == "ivt" and ignore_null and self.num_class == 100:
            k -= N_NULL_TRIPLETS                                       # the null triplets are the last columns: k of ld
        return ops.video_ap(p, t, self._concatenated()[2], k).cpu().numpy()

    def compute_video_AP(self, component: str = "ivt", ignore_null: bool = False):
        _check_component(component, self.num_class)
        if not self.global_targets:
            return video_mean([], self.num_class)
        return video_mean(self.per_video_AP(component, ignore_null), self.num_class)

    def to_host(self) -> Recognition:
        """the same videos as float64 numpy in a `metrics.Recognition` (what the reports pickle)"""
        return Recognition(self.num_class).set_videos([(t.cpu().numpy(), p.cpu().numpy()) for t, p in zip(self.global_targets, self.global_predictions)])

    def rank_hist(self, component: str = "ivt") -> np.ndarray:
        """int64 [Kc] on the host: `metrics.rank_hist` of all frames seen, one `ops.rank_hist` launch per component and set of videos"""
        _check_component(component, self.num_class)
        if component not in self._hist:
            if not self.global_targets:
                self._hist[component] = np.zeros(self.num_class if component == "ivt" else component_table(component)[1], dtype=np.int64)
            else:
                t, p = self._component(component)
                self._hist[component] = ops.rank_hist(p, t).cpu().numpy()
        return self._hist[component]

    def topK(self, k: int = 5, component: str = "ivt") -> float:
        return _top_k(self.rank_hist(component), k)


def device_recognition_from(scores, order):
    """`metrics.recognition_from` with device rows: {video -> {head -> (targets, predictions)}} -> {head -> DeviceRecognition}"""
    missing = [k for k in order if k not in scores]
    if missing:
        raise KeyError(f"videos without predictions: {missing[:4]}")
    heads = [h for h, _ in HEADS if all(h in scores[k] for k in order)]
    return {h: DeviceRecognition(dict(HEADS)[h]).set_videos([scores[k][h] for k in order]) for h in heads}


# ------------------------------------------------------------------------------------------------ several ranks: the small arrays travel
class MergedRecognition:
    """the report's surface of `Recognition` over the per-video AP rows and the rank histograms of all ranks: `rows` = {component -> float64
    [V, Kc] in the single-process video order}, `hists` = {component -> int64 [Kc]}.  An AP column depends on nothing but its own (video,
    class) rows, so these are the numbers one process computes over all videos -- exactly."""

    def __init__(self, num_class: int, rows, hists):
        self.num_class, self.rows, self.hists = num_class, rows, hists

    def compute_video_AP(self, component: str = "ivt", ignore_null: bool = False):
        _check_component(component, self.num_class)
        rows = self.rows[component]
        if ignore_null and component == "ivt" and self.num_class == 100:
            rows = rows[:, :self.num_class - N_NULL_TRIPLETS]
        return video_mean(list(rows), self.num_class)

    def topK(self, k: int = 5, component: str = "ivt") -> float:
        _check_component(component, self.num_class)
        return _top_k(self.hists[component], k)


def summarize(m, keys):
    """{head -> DeviceRecognition} over the videos `keys` of THIS rank (in that order) -> what `gather_device_recognition` exchanges:
    {"ap": {video -> {head -> {component -> float64 [Kc]}}}, "hist": {head -> {component -> int64 [Kc]}}} -- for the 100-way head the six
    components, for a component head its own classes"""
    ap = {v: {} for v in keys}
    hist = {}
    for h, rec in m.items():
        hist[h] = {}
        for c in _components_of(rec.num_class):
            rows = rec.per_video_AP(c)
            for vi, v in enumerate(keys):
                ap[v].setdefault(h, {})[c] = np.asarray(rows[vi], dtype=np.float64)
            hist[h][c] = np.asarray(rec.rank_hist(c), dtype=np.int64)
    return {"ap": ap, "hist": hist}


def gather_device_recognition(local, order, group=None):
    """local: `summarize(...)` of THIS rank's videos.  Returns {head -> MergedRecognition} over the videos of ALL ranks in `order` (the
    single-process order), identical on every rank: per-video AP rows placed in `order`, histograms summed.  One host-side object gather of
    [K]-sized arrays, where `metrics.gather_recognition` sends every video's rows."""
    import torch.distributed as dist
    parts = [local]
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        parts = [None] * dist.get_world_size(group)
        dist.all_gather_object(parts, local, group=group)
    ap = {}
    for part in parts:
        for v, heads in part["ap"].items():
            if v in ap:
                raise ValueError(f"video {v} evaluated by two ranks")
            ap[v] = heads
    missing = [v for v in order if v not in ap]
    if missing:
        raise KeyError(f"videos without predictions: {missing[:4]}")
    merged = {}
    for h, n in HEADS:
        if not all(h in ap[v] for v in order):
            continue
        comps = _components_of(n)
        width = {c: n if c == "ivt" else component_table(c)[1] for c in comps}
        rows = {c: np.stack([ap[v][h][c] for v in order], 0) if len(order) else np.zeros((0, width[c])) for c in comps}
        hists = {c: sum((np.asarray(part["hist"][h][c], dtype=np.int64) for part in parts if h in part["hist"]), np.zeros(width[c], dtype=np.int64))
                 for c in comps}
        merged[h] = MergedRecognition(n, rows, hists)
    return merged
