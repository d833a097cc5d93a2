#!/usr/bin/env python3
"""MI355X entry point without a reference counterpart: frames of a video -> per-frame top-K triplet predictions in one pass
(student -> temporal head -> `mt4_topk_rows_f32`; see computervision_codes_amd/drivers.py `predict`).  One process; no label files.  `--causal --online [--online_chunk N] [--online_streams S]` answers frame by frame, S videos at once.  `--localize {i,ivt} [--localize_frac F] [--save_maps]` adds where in the frame each top-K triplet is
(class-activation maps of the student's heads, `mt4_class_maps`): `loc_*` arrays in the .npz and `<video>.loc.csv`."""
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from computervision_codes_amd.drivers import predict  # noqa: E402

if __name__ == "__main__":
    predict(sys.argv[1:])
