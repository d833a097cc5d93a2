"""The nn.Module-like surface the four inference models share (`spatial_cnn.VideoNas`, `temporal_tenco.VideoNas`, `temporal_mstct.VideoNas`,
`spatial_transformer.Qeruy2Label`): `eval / cuda / state_dict / load_state_dict` over the model's shape table.  Host code only."""
from __future__ import annotations

from typing import Dict

import torch


class StateModule:
    """A subclass sets `self._table` ([(key, shape)] in registration order, `shapes.py`) and `self._sd = {}` and defines `_pack()`, which
    builds the device-side parameters from `self._sd`.  Three hooks carry what differs between the models."""

    def eval(self):
        self.training = False
        return self

    def cuda(self):
        return self

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return dict(self._sd)

    def _tolerated(self, key: str) -> bool:
        """an unexpected key that a strict load accepts all the same"""
        return False

    def _store(self, t: torch.Tensor) -> torch.Tensor:
        """the tensor kept in the state dict for a loaded one"""
        return t.detach().float()

    def _loaded(self):
        """after the tensors of a load are stored"""
        self._pack()

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        names = [k for k, _ in self._table]
        known = set(names)
        missing = [k for k in names if k not in sd]
        unexpected = [k for k in sd if k not in known and not self._tolerated(k)]
        if strict and (missing or unexpected):
            raise KeyError(f"state dict mismatch: missing {missing[:4]}, unexpected {unexpected[:4]}")
        for k, shp in self._table:
            if k in sd:
                if tuple(sd[k].shape) != tuple(shp):
                    raise ValueError(f"{k}: shape {tuple(sd[k].shape)} != {shp}")
                self._sd[k] = self._store(sd[k])
        self._loaded()
        return self
