"""Stage drivers behind the reference's `Scripts/` entry points (SURVEY 8(b) "CLI"): same flag names, relative paths
(`./__checkpoint__/run_<version>/`, `../0-5fold/data_feats/run_<version>/`), checkpoint names and feature-file layout
as `Spatial_cnn/test.py`, `Spatial_transformer/test.py`, `Temporal_mstct/test.py` and `Temporal_tenco/run.py -e`.
Unknown flags are ignored like the reference's `parse_known_args`.  Two additions: `--dtype {fp32,bf16}` and, when
torch.distributed is initialised (torchrun), whole videos are sharded over ranks (extract.shard_videos)."""
from __future__ import annotations

import argparse
import sys
import os
import pickle
import time
from typing import Dict

import numpy as np
import torch

from . import cholect, extract, featfile
from .metrics import Recognition, final_report, gather_recognition, recognition_from
from .trainloop import LossMean, _barrier, _dist, _log, add_schedule_flags, deal, guard_flags, load_resume, run_epochs


def extraction_batch(img_size, device_batch):
    from .spatial_transformer import extraction_batch as f      # (the transformer stage loads on demand)
    return f(img_size, device_batch)


def _common(p: argparse.ArgumentParser):
    p.add_argument("--model", type=str, default="rendezvous")
    p.add_argument("--version", type=str, default="")
    p.add_argument("--version1", type=str, default="")
    p.add_argument("-t", "--train", action="store_true")
    p.add_argument("-e", "--test", action="store_true")
    p.add_argument("--data_dir", type=str, default="/home/shuangchun/Data/Video/CholecT45/CholecT45")
    p.add_argument("--dataset_variant", type=str, default="cholect45-crossval")
    p.add_argument("-k", "--kfold", type=int, default=1)
    p.add_argument("--image_width", type=int, default=448)
    p.add_argument("--image_height", type=int, default=256)
    p.add_argument("-b", "--batch", type=int, default=32)
    p.add_argument("--loss_type", type=str, default="all")
    p.add_argument("--test_ckpt", type=str, default=None)
    p.add_argument("--gpu", type=str, default="0")
    p.add_argument("--seed", type=int, default=47)
    p.add_argument("--dtype", type=str, default="fp32", choices=["fp32", "bf16"])
    p.add_argument("--device_batch", type=int, default=512, help="frames per extraction pass on the GPU (results do not depend on it)")
    p.add_argument("--decode_workers", type=int, default=8, help="host threads decoding PNGs")
    p.add_argument("--png_decode", type=str, default="host", choices=["host", "device"],
                   help="device: inflate + PNG unfiltering on the GPU (mt4_png_inflate / mt4_png_unfilter_rgb8), the host only reads the files")
    p.add_argument("--metrics", type=str, default="host", choices=["host", "device"],
                   help="device: the video-wise AP and top-K of the trainers' validation, of the temporal closing reports and of the spatial -e / test.py "
                        "passes on the GPU (mt4_video_ap_f32 / mt4_component_max_f32 / mt4_rank_hist_f32) from the fp32 scores where the model wrote them; "
                        "under torchrun the spatial passes exchange per-video AP rows and rank histograms instead of the rows.  The pickled metric "
                        "objects and the temporal drivers' N-rank gather (rank 0 alone runs those) stay on the host")


def _flag(*names, **kw):
    return names, kw


# the flags of the two frame trainers (`Spatial_cnn/run.py`, `Spatial_transformer/run.py`: --rates `:66`, --temp `:70`).  The reference's
# Spatial_transformer dataloader reads args.teacher_pred_version / teacher_feat_version (`dataloader.py:217-238`) though its run.py declares
# neither flag: same names and defaults as the student's `Spatial_cnn/run.py`
_OPERAND_DTYPE = _flag("--operand_dtype", type=str, default="fp32", choices=["fp32", "bf16"],
                       help="bf16: the GEMM operands of the training step in bf16 (Spatial_cnn: the convolutions' activations, gradients and weight copies; "
                            "the transformer stages: operand copies of the nn.Linear GEMMs), master weights, accumulation and sums fp32")
# --deterministic (not in the reference, which seeds torch and still sums with atomics): declared on EVERY trainer's parser -- the entry points read
# their flags with parse_known_args, so an undeclared flag would be ignored in silence -- honoured by the trainers named in `_DETERMINISTIC_STAGES`
# and refused by the others before any model is built (`_deterministic`)
_DETERMINISTIC = _flag("--deterministic", action="store_true",
                       help="reproducible training (Spatial_cnn, Temporal_tenco): every sum of the step that crosses workgroups (weight and bias gradients, "
                            "BatchNorm sums, the max-pool backward, loss sums) is taken from per-workgroup partials folded in a fixed order (mt4_*_det_* + "
                            "mt4_fold_parts_f32 / _f64) instead of float atomics -- the same seed and inputs give the same losses and the same checkpoint "
                            "bytes; the BatchNorm statistics come from the separate pass instead of the convolution's epilogue")
# --resume (not in the reference, whose drivers load `_latest` and start again at epoch 0): every trainer, `trainloop.run_epochs`
_RESUME = _flag("--resume", action="store_true",
                help="write resume state beside the `_latest` checkpoint whenever that is written (`<latest>.resume`, ranks > 0 `<latest>.resume.rank<r>`: "
                     "epoch, best score, world size, the digest of the `_latest` bytes, the host generators' states) and continue from it when it is there: "
                     "the epoch after the recorded one, with its learning rate, draws and best score.  The same command line can be issued again "
                     "after a kill; a `_latest` without matching resume state is refused.  `_latest.pth` itself stays the plain state dict")
# --clip_grad_norm / --skip_nonfinite (not in the reference, which applies whatever gradient it gets): every trainer, `FlatTrainer.apply_update`
_GUARD = [
    _flag("--clip_grad_norm", type=float, default=0.0,
          help="X > 0: the step's gradient (after the data-parallel exchange, weight decay not included) is scaled to the global L2 norm X when its "
               "norm is larger -- torch.nn.utils.clip_grad_norm_'s coefficient min(1, X / (norm + 1e-6)), the norm taken in float64 on the device "
               "(mt4_grad_norm_parts_f32 + mt4_grad_guard_finalize), no copy to the host; 0: off; negative: refused"),
    _flag("--skip_nonfinite", action="store_true",
          help="a step whose gradient holds a NaN or an Inf changes nothing: parameters and BatchNorm running statistics stay as they were "
               "(mt4_sgd_step_guarded_f32, mt4_restore_if_skipped_f32; num_batches_tracked still advances), the epoch's loss is the mean over the "
               "steps with a finite loss, and an epoch in which every step was skipped ends the run before a checkpoint is written"),
]
# --momentum / --nesterov / --optimizer / --adam_betas / --adam_eps: every trainer, `FlatTrainer.apply_update` (`flatparams.Optim`)
_OPTIM = [
    _flag("--momentum", type=float, default=0.0,
          help="SGD momentum M in [0, 1) (torch.optim.SGD, dampening 0; mt4_sgd_momentum_step_f32).  The default 0.0 is the reference's EFFECTIVE "
               "value: every driver of it declares --momentum with default 0.95 (Spatial_cnn/run.py:72, Spatial_transformer/run.py:72, "
               "Temporal_mstct/run.py:73, Temporal_tenco/run.py:66) and none hands it to torch.optim.SGD (:344, :360, :345, :346).  The clip of "
               "--clip_grad_norm scales the gradient before it enters the momentum buffer; without --skip_nonfinite a non-finite gradient "
               "poisons the buffer for good, as it does in torch"),
    _flag("--nesterov", action="store_true", help="the Nesterov form of the momentum update (needs --momentum > 0)"),
    _flag("--optimizer", type=str, default="sgd", choices=["sgd", "adamw"],
          help="the update rule: sgd (with --momentum / --nesterov) or adamw (torch.optim.AdamW, amsgrad off, decoupled --weight_decay; "
               "mt4_optim_advance + mt4_adamw_step_f32, the step count kept on the device).  Without --skip_nonfinite a non-finite gradient "
               "poisons the moments for good, as it does in torch.  The schedule flags -l, -w, --power, --decay_rate keep their meaning"),
    _flag("--adam_betas", type=float, nargs=2, default=[0.9, 0.999], metavar=("B1", "B2"), help="AdamW's betas, each in [0, 1)"),
    _flag("--adam_eps", type=float, default=1e-8, help="AdamW's epsilon (> 0)"),
]
# --ema_decay / --ema_warmup / --ema_eval (the reference ships `ModelEma`, Spatial_transformer/utils/misc.py:433-458, and no driver calls it): every
# trainer, `FlatTrainer._ema_update` (`flatparams.Ema`) and `trainloop.run_epochs`
_EMA = [
    _flag("--ema_decay", type=float, default=0.0,
          help="D in (0, 1): keep an exponential moving average of the weights on the device, E <- D E + (1 - D) P behind every applied update "
               "(mt4_ema_advance + mt4_ema_step_f32; the student's BatchNorm running statistics are averaged with it), validate IT and save IT "
               "as the best `.pth` -- a plain state dict, so extraction, test.py and predict.py need no flag; `_latest.pth` stays the raw weights "
               "and --resume keeps the average beside it (`<latest>.ema.e<epoch>`).  A step --skip_nonfinite skips does not enter the average; "
               "without --skip_nonfinite a non-finite parameter stays in it for good, as in the optimizer state.  0: off"),
    _flag("--ema_warmup", action="store_true",
          help="the decay of the t-th averaged step is min(D, (1 + t) / (10 + t)) (TensorFlow's ExponentialMovingAverage with num_updates): the "
               "average follows the weights closely at first (needs --ema_decay > 0)"),
    _flag("--ema_eval", type=str, default="ema", choices=["ema", "both"],
          help="both: validation also scores the raw weights and the `video-wise |` line shows it as `| raw => ...`; the best `.pth` is still "
               "chosen by, and holds, the averaged weights (needs --ema_decay > 0)"),
]
_DETERMINISTIC_STAGES = ("spatial_cnn", "tenco")
_NOT_DETERMINISTIC = {
    "spatial_transformer": "the sequence trainers' reductions are not covered yet (csrc/seq_train_kernels.hip: LayerNorm dgamma/dbeta, the "
                           "relative-position table gradient, the depth-wise conv gradient)",
    "mstct": "the sequence trainers' reductions are not covered yet (csrc/seq_train_kernels.hip: LayerNorm dgamma/dbeta, the "
             "relative-position table gradient, the depth-wise conv gradient)",
}
_FRAME_TRAIN = [
    _flag("--teacher_feat_version", type=str, default="Q2L"),
    _flag("--teacher_pred_version", type=str, default="Q2LMSTCT"),
    _flag("--augmentation_list", type=str, nargs="*", default=["original", "vflip", "hflip", "contrast", "rot90"]),
    _flag("--train_transform", type=str, default="host", choices=["host", "device"],
          help="device: flips, autocontrast, rotation and the second Resize of the train transform on the GPU (mt4_aug_*), the same bytes "
               "as Pillow for the same draws; the PNGs are decoded as --png_decode says"),
    _flag("--prefetch", type=int, default=0,
          help="K > 0: training batches come from `loader.FrameLoader` -- chunks of up to K batches (at most 1024 frames) decoded, transformed "
               "and gathered per call on helper threads and side streams while the step runs, labels and teacher rows resident on the device; "
               "the same batches as 0 (the synchronous loader), only faster"),
    _flag("--frame_cache", type=float, default=0,
          help="GB of HBM per rank for `cholect.FrameCache`: the decoded, resized uint8 frames stay on the device across epochs, so every epoch after "
               "the first (and every validation after the first) takes its frames from the pool (mt4_take_frames_u8) instead of reading, inflating "
               "and resizing the PNGs again; first come, first served, the same bytes; training frames are cached behind --train_transform device only; 0: off"),
    _flag("--rates", type=float, nargs="+", default=[1, 0, 0.1]),
    _flag("--temp", type=int, default=4),
    _flag("--pretrain_dir", type=str, default=""),
    _OPERAND_DTYPE,
    _DETERMINISTIC,
    _RESUME,
] + _GUARD + _OPTIM + _EMA
# stage -> (the flags every entry point of the stage parses, the flags of its trainer alone), on top of `_common` and -- the trainer --
# `add_schedule_flags`.  --teacher_dim: the student mixes in the 1536-wide Swin-L feature (`Spatial_cnn/run.py`), the transformer stage's
# `loss_type all` variant the 512-wide ResNet-18 one (`Spatial_transformer/run.py:82`, `test.py:82`)
_FLAGS = {
    "spatial_cnn": ([_flag("--network", type=str, default="resnet18"),
                     _flag("--student_dim", type=int, default=512),
                     _flag("--teacher_dim", type=int, default=1536)],
                    _FRAME_TRAIN + [_flag("--imagenet_trunk", type=str, default="",
                                          help="a torchvision ResNet-18 / -50 checkpoint (e.g. resnet50-0676ba61.pth) for the trunk, the reference's "
                                               "`pretrained=True` (`network.py:100,105`): loaded after the synthetic fill and before --pretrain_dir and "
                                               "`_latest`; a file that is not there or is another architecture's is an error")]),
    "spatial_transformer": ([_flag("--backbone", type=str, default="swin_L_384_22k"),
                             _flag("--img_size", type=int, default=384),
                             _flag("--hidden_dim", type=int, default=1536),
                             _flag("--teacher_dim", type=int, default=512)],
                            _FRAME_TRAIN + [_flag("--drop_path_rate", type=float, default=0.1)]),          # `swin_transformer.py:488`
    "mstct": ([_flag("--input_dim", type=int, default=1536),
               _flag("--final_embedding_dim", type=int, default=512)],
              [_flag("--num_clips", type=int, default=256, help="window length (the reference hard-codes 256, dataloader.py:237)"), _OPERAND_DTYPE,
               _DETERMINISTIC, _RESUME] + _GUARD + _OPTIM + _EMA),
    # --mask_draw / --subclip (not in the reference) device: the step's random pieces are drawn by HIP kernels from (seed, step) and whole-video
    # steps replay as hipGraphs; host: drawn with torch's generator and uploaded.  reference: `Temporal_tenco/dataloader.py:219-222` sub-clip sampling
    "tenco": ([_flag("--num_layers_PG", default=11, type=int),
               _flag("--num_layers_R", default=10, type=int),
               _flag("--num_R", default=3, type=int),
               _flag("--fpn", action="store_true"),
               _flag("--mask", action="store_true"),
               _flag("--output", default=False, type=bool),
               _flag("--hier", default=False, type=bool),
               _flag("--causal", action="store_true",
                     help="the causal temporal head (the reference's unused `DilatedResidualCausalLayer`, network.py:165-183): every dilated conv reads "
                          "frames t - 2d, t - d, t, so frame t's answer needs no later frame; same checkpoint keys -- train, evaluate and predict with it"),
               _flag("--input_dim", type=int, default=512)],
              [_flag("--mask_draw", choices=("host", "device"), default="host"),
               _flag("--subclip", choices=("off", "reference"), default="off"),
               _DETERMINISTIC, _RESUME] + _GUARD + _OPTIM + _EMA),
}
_LATEST = {"spatial_cnn": "_latest.pth", "spatial_transformer": "_latest.pth", "tenco": "_latest.pth",
           "mstct": "latest.pth"}                            # <stem> + this = the trainer's newest checkpoint; MS-TCT: no underscore (`Temporal_mstct/run.py:268`)
_MSTCT_ARCH = ((256, 384, 576, 864), 2, 8, 8)               # inter_channels, num_block, head, mlp_ratio (`Temporal_mstct/run.py`)


def _parser(stage: str, train: bool) -> argparse.ArgumentParser:
    """the parser of a stage's entry points (of its trainer with `train`); they read it with `parse_known_args`: unknown flags are ignored"""
    p = argparse.ArgumentParser()
    _common(p)
    if train:
        add_schedule_flags(p)
    own, train_only = _FLAGS[stage]
    for names, kw in own + (train_only if train else []):
        p.add_argument(*names, **kw)
    return p


def _deterministic(stage: str, F) -> bool:
    """--deterministic of a trainer: said once at start where the stage's trainer has the mode, refused (before any model is built) where not"""
    if not getattr(F, "deterministic", False):
        return False
    if stage not in _DETERMINISTIC_STAGES:
        raise NotImplementedError(f"--deterministic: {_NOT_DETERMINISTIC[stage]}")
    print("--deterministic: fixed-order sums (per-workgroup partials + mt4_fold_parts_f32 / _f64) in place of float atomics", flush=True)
    return True


def _causal(F) -> bool:
    """--causal of the temporal head, read before any model is built: refused with --hier True, said once at start"""
    if not getattr(F, "causal", False):
        return False
    if getattr(F, "hier", False):
        from .temporal_tenco import CAUSAL_HIER_REASON
        raise ValueError(CAUSAL_HIER_REASON)
    print("--causal: dilated convs read frames t - 2d, t - d, t (front padding 2d): frame t's logits depend on no later frame", flush=True)
    return True


def _guard(F) -> dict:
    """--clip_grad_norm / --skip_nonfinite of a trainer, read before any model is built: a negative norm is refused, the mode is said once at
    start; -> the trainer's keyword arguments"""
    clip, skip = guard_flags(F)
    if not clip >= 0:
        raise ValueError(f"--clip_grad_norm {clip}: 0 (off) or a positive global L2 norm")
    if clip > 0 or skip:
        print("guarded update:" + (f" --clip_grad_norm {clip:g} (global L2 norm of the exchanged gradient, float64, on the device)" if clip > 0 else "")
              + (" --skip_nonfinite (a step with a NaN / Inf gradient changes nothing)" if skip else ""), flush=True)
    return {"clip_grad_norm": clip, "skip_nonfinite": skip}


def _optim(F) -> dict:
    """--optimizer / --momentum / --nesterov / --adam_betas / --adam_eps of a trainer, read before any model is built: contradictions and values
    out of range are refused, a rule other than plain SGD is said once at start; -> the trainer's keyword argument"""
    from .flatparams import Optim
    kind, mom, nest = getattr(F, "optimizer", "sgd"), float(getattr(F, "momentum", 0.0)), bool(getattr(F, "nesterov", False))
    betas, eps = [float(b) for b in getattr(F, "adam_betas", (0.9, 0.999))], float(getattr(F, "adam_eps", 1e-8))
    if kind == "adamw":
        if mom != 0 or nest:
            raise ValueError("--momentum / --nesterov belong to --optimizer sgd; adamw takes --adam_betas")
        if not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError(f"--adam_betas {betas[0]:g} {betas[1]:g}: each in [0, 1)")
        if not eps > 0:
            raise ValueError(f"--adam_eps {eps:g}: a positive number")
        o = Optim("adamw", 0.0, False, betas[0], betas[1], eps)
    else:
        if not 0 <= mom < 1:
            raise ValueError(f"--momentum {mom:g}: in [0, 1)")
        if nest and mom == 0:
            raise ValueError("--nesterov needs --momentum > 0")
        o = Optim("sgd", mom, nest)
    o.check()
    if o.stateful:
        print("update rule: " + (f"adamw betas ({o.beta1:g}, {o.beta2:g}) eps {o.eps:g}, decoupled weight decay" if kind == "adamw" else
                                 f"sgd momentum {o.momentum:g}" + (" nesterov" if o.nesterov else ""))
              + " (state in flat fp32 buffers beside the parameters; --resume keeps it)", flush=True)
    return {"optim": o if o.stateful else None}


def _ema(F) -> dict:
    """--ema_decay / --ema_warmup / --ema_eval of a trainer, read before any model is built: a decay outside [0, 1) and --ema_warmup or
    --ema_eval both without a decay are refused, an average is said once at start; -> the trainer's keyword argument"""
    from .flatparams import Ema
    decay, warmup = float(getattr(F, "ema_decay", 0.0)), bool(getattr(F, "ema_warmup", False))
    if not 0 <= decay < 1:
        raise ValueError(f"--ema_decay {decay:g}: in [0, 1) (0: off)")
    if warmup and decay == 0:
        raise ValueError("--ema_warmup needs --ema_decay > 0")
    if getattr(F, "ema_eval", "ema") == "both" and decay == 0:
        raise ValueError("--ema_eval both needs --ema_decay > 0: without an average there is nothing beside the raw weights to validate")
    e = Ema(decay, warmup).check()
    if e.active:
        print(f"weight average: decay {decay:g}" + (" warmup" if warmup else ""), flush=True)
    return {"ema": e if e.active else None}


def _resume(F, latest: str, optim=None, ema=None):
    """--resume of a trainer, read before any model is built: what `trainloop.load_resume` finds beside `latest` for this rank (a fresh run,
    the state to continue from, or its ValueError -- also when the recorded optimizer state or weight average does not belong to the flags
    `optim` / `ema` were made from); None without the flag"""
    if not getattr(F, "resume", False):
        return None
    return load_resume(latest, *_dist(), optim=optim.config() if optim is not None else None, ema=ema.config() if ema is not None else None)


def _load_optim(tr, resume):
    """the optimizer state and the weight average `load_resume` read beside the checkpoint go into the trainer (after its `load_state_dict`)"""
    if resume is not None and resume.optim_state is not None:
        tr.load_optimizer_state_dict(resume.optim_state())
    if resume is not None and resume.ema_state is not None:
        tr.load_ema_export(resume.ema_state())


def _latest_state(latest: str, resume):
    """the state dict a trainer starts from when its newest checkpoint is on disk (else None); under --resume the tensors of the very bytes
    whose digest `load_resume` checked"""
    if resume is not None:
        return resume.state_dict()
    return torch.load(latest, map_location="cpu") if os.path.exists(latest) else None


def _dtype(name: str) -> torch.dtype:
    return torch.float32 if name == "fp32" else torch.bfloat16


def _chlg(F) -> bool:
    """`set_chlg_eval` of the reference's drivers (`Spatial_cnn/run.py:122`): the challenge evaluation protocol (null triplets left out of the
    100-way AP) for the `*challenge*` dataset variants"""
    return "challenge" in str(getattr(F, "dataset_variant", ""))


def _stem(F, kfold: int = None, task_dir: bool = False, model: str = None) -> str:
    """`./__checkpoint__/run_<version>[_<task>]/<modelname>`, the stem of a run's log and checkpoints.  modelname: the spatial drivers'
    `<model>_l<variant>_cholect<kfold>` when kfold is given, else the temporal drivers' `<model>_l8_cholect<variant>_k<kfold>_batchnorm_lowres`
    (`Temporal_tenco/run.py:137-142`); task_dir: the task suffix of single-task runs (`Spatial_transformer/run.py:86-88`, `Temporal_mstct/run.py:88-90`);
    model: instead of --model (the spatial `test.py` spell their checkpoint 'rendezvous' whatever --model says)"""
    model = model or F.model
    name = f"{model}_l{F.dataset_variant}_cholect{kfold}" if kfold is not None else f"{model}_l8_cholect{F.dataset_variant}_k{F.kfold}_batchnorm_lowres"
    return os.path.join(f"./__checkpoint__/run_{F.version}" + (f"_{F.loss_type}" if task_dir and F.loss_type != "all" else ""), name)


def _sigmoid(x: torch.Tensor) -> np.ndarray:
    return torch.sigmoid(x.float()).cpu().numpy()


def _device_metrics(F) -> bool:
    return getattr(F, "metrics", "host") == "device"


def _scores(x: torch.Tensor, device: bool):
    """sigmoid scores of logits x: the fp32 values `_sigmoid` copies down, left on the device for --metrics device"""
    return torch.sigmoid(x.float()) if device else _sigmoid(x)


def _label_rows(cache, v, lab, device: bool):
    """{head -> label rows [N,K] of video v} (`lab()` reads the label files): for --metrics device fp32 on the GPU, uploaded once per video
    and run -- `cache` outlives the epochs"""
    if not device:
        return {h: a[:, 1:] for h, a in lab().items() if h in ("i", "v", "t", "ivt")}
    if v not in cache:
        cache[v] = {h: torch.from_numpy(np.ascontiguousarray(a[:, 1:], dtype=np.float32)).cuda() for h, a in lab().items() if h in ("i", "v", "t", "ivt")}
    return cache[v]


def _spatial_recognition(F, scores_local, mine, order):
    """{head -> metric object} over the videos of ALL ranks in `order`, identical on every rank, from this rank's `scores_local` (its videos
    `mine`).  host: every video's (labels, scores) meet in `metrics.gather_recognition`.  --metrics device: the rows stay on the GPU; one
    rank reports from `DeviceRecognition` objects, N ranks exchange their per-video AP rows and rank histograms
    (`metrics_device.gather_device_recognition`) -- the same digits either way."""
    if not _device_metrics(F):
        return gather_recognition(scores_local, order)
    from .metrics_device import device_recognition_from, gather_device_recognition, summarize
    if _dist()[1] == 1:
        return device_recognition_from(scores_local, order)
    return gather_device_recognition(summarize(device_recognition_from(scores_local, mine), mine), order)


def _recognition(scores, order, device: bool):
    if device:
        from .metrics_device import device_recognition_from
        return device_recognition_from(scores, order)
    return recognition_from(scores, order)


def _write_report(logfile: str, m, loss_type: str, chlg: bool, style: str, pckl: str = None) -> Dict[str, float]:
    """the reference's closing report (`metrics.final_report`: per-category AP vectors, the mean-AP row with I / V / T disentangled from the
    triplet head, top-K rows) into the log file, and -- temporal drivers -- the pickled metric objects (`Temporal_tenco/run.py:529-533`:
    `{'ivt': mAP, 'i': mAPi, 'v': mAPv, 't': mAPt}`, here `metrics.Recognition` objects with ivtmetrics' attribute names)"""
    if pckl:
        os.makedirs(os.path.dirname(os.path.abspath(pckl)), exist_ok=True)
        with open(pckl, "wb") as f:
            pickle.dump({k: m[k].to_host() if hasattr(m[k], "to_host") else m[k] for k in ("ivt", "i", "v", "t")}, f)     # (--metrics device: the same type and arrays)
    lines, res = final_report(m, loss_type, chlg, style)
    for ln in lines:
        _log(logfile, ln)
    return res


def _eval_model(stage: str, F, src):
    """the inference model of `stage` built from F with a checkpoint loaded.  src = a list of checkpoint files: --test_ckpt instead of the
    first when given, then the first one on disk (the last if none is: the load names it), the model in --dtype; or a trainer's state dict
    (validation): the fp32 model.  Strict loads, except a Temporal_tenco FILE: the model's own keys of it (`Temporal_tenco/run.py:520`)"""
    from_file = not isinstance(src, dict)
    dtype = _dtype(F.dtype) if from_file else torch.float32
    if stage == "spatial_cnn":
        from .spatial_cnn import VideoNas
        model = VideoNas(args=argparse.Namespace(**{**vars(F), "train": False}), dtype=dtype)     # (args.train gates the KD branch, `network.py:47`)
    elif stage == "spatial_transformer":
        from .spatial_transformer import build_q2l
        model = build_q2l(F, dtype=dtype)
    elif stage == "mstct":
        from .temporal_mstct import VideoNas
        model = VideoNas(F, *_MSTCT_ARCH, F.input_dim, F.final_embedding_dim, dtype=dtype)
    else:
        from .temporal_tenco import VideoNas
        model = VideoNas(F, F.num_layers_PG, F.num_layers_R, F.num_R, 512, F.input_dim, 100,         # (fp32 whatever --dtype says)
                         causal=bool(getattr(F, "causal", False)))
    if from_file:
        files = [F.test_ckpt or src[0]] + list(src[1:])
        src = torch.load(next((f for f in files if os.path.exists(f)), files[-1]), map_location="cpu")
        if stage == "tenco":
            known = dict(model._table)
            return model.eval().load_state_dict({k: v for k, v in src.items() if k in known}, strict=False)
    return model.eval().load_state_dict(src, strict=True)


def _labelled_share(F, videos):
    """-> (the labels of `videos`, the videos of this rank under `extract.shard_videos` by frame count, in file order)"""
    labels = {v: cholect.load_labels(F.data_dir, v) for v in videos}
    mine = extract.shard_videos(videos, [len(labels[v]["ivt"]) for v in videos], *_dist())
    return labels, [videos[vi] for vi in mine]


def _on_rank0(fn):
    """fn() on rank 0 alone ({} on the others); every rank meets at the barrier behind it, whatever fn raised: what rank 0 wrote is on disk
    before any rank goes on to the next stage"""
    try:
        return fn() if _dist()[0] == 0 else {}
    finally:
        _barrier()


# ------------------------------------------------------------------------------------------------ Spatial_cnn/test.py
def _spatial_cnn_videos(F, model, vids, labels):
    """the per-video loop of `test_loop` (`Spatial_cnn/test.py:143-177`, `run.py:226-256`) over `vids`: -> ({video key -> feat [N,D]},
    {video -> {head -> (labels [N,K], sigmoid scores [N,K])}}); --metrics device: label rows and scores are fp32 tensors on the GPU, the
    sigmoid of the logits where the extractor left them"""
    feats_local: Dict[str, np.ndarray] = {}
    scores_local = {}
    dev_dec = F.png_decode == "device"
    dev_met, label_cache = _device_metrics(F), {}

    def loader(v):
        ids_all = labels[v]["ivt"][:, 0]                       # file order, no shuffle, drop_last False (`test.py:227-242`)
        return lambda s, e: cholect.load_frames_device(F.data_dir, v, ids_all[s:e], F.image_height, F.image_width,   # decode on the host (or
                                                       workers=F.decode_workers, decode=F.png_decode)          # device), Resize on the GPU
    # ONE loader pipeline over all videos (`extract.extract_videos_device`): the first loads of the next video are read and decoded while this
    # one's last passes run.  The device PNG decoder runs one wave per frame and takes 75-105 ms per call for 512-2048 frames: it is handed loads
    # of 1024 frames, two in flight on streams of their own (sweep: profiles/r04_png_pipeline_sweep.txt -- 9.7-10.2 k frames/s from 480 x 854 files
    # through ResNet-50; the host reader alone delivers > 100 k files/s, what bounds the loop is inflate time + extractor time, which share the CUs).
    plan = [(v, len(labels[v]["ivt"]), loader(v)) for v in vids]
    for v, feat, lgs, *dev_lgs in extract.extract_videos_device(model, plan, F.device_batch, prefetch=2 if dev_dec else 1,
                                                                    load_batch=(1023 // F.device_batch + 1) * F.device_batch if dev_dec else None,      # (>= 1024 frames per device decode)
                                                                    keep_device=dev_met):
        lab = labels[v]
        if dev_met:
            rows = _label_rows(label_cache, v, lambda: lab, True)
            scores_local[v] = {key: (rows[key], torch.sigmoid(lg)) for key, lg in zip(("i", "v", "t", "ivt"), dev_lgs[0])}
        else:
            scores_local[v] = {key: (lab[key][:, 1:], torch.sigmoid(torch.from_numpy(lg)).numpy())       # `test.py:162-169`
                               for key, lg in zip(("i", "v", "t", "ivt"), lgs)}
        feats_local[featfile.video_key(v)] = np.array(feat)    # (own copy: the pinned staging buffer is released)
    return feats_local, scores_local


def spatial_cnn_eval(argv=None) -> Dict[str, float]:
    """`Spatial_cnn/run.py -e` (:503-560): the TEST-split videos through the best checkpoint and the closing report -- per-category AP, the
    mean-AP row (I / V / T disentangled from the 100-way triplet head when --loss_type all, head-wise otherwise, `:518-525`), top-5 / 10 / 20
    per component.  Under torchrun whole videos are sharded over the ranks and their (labels, scores) -- --metrics device: their AP rows and
    rank histograms -- meet in one host-side gather, so N ranks log exactly the single-rank report; rank 0 writes it."""
    F = _parser("spatial_cnn", False).parse_known_args(argv)[0]
    kfold = F.kfold if "crossval" in F.dataset_variant else 0
    stem = _stem(F, kfold)
    model = _eval_model("spatial_cnn", F, [stem + ".pth"])
    _, _, videos = cholect.split_videos(F.dataset_variant, kfold)
    labels, mine = _labelled_share(F, videos)
    _, scores_local = _spatial_cnn_videos(F, model, mine, labels)
    m = _spatial_recognition(F, scores_local, mine, videos)
    return _on_rank0(lambda: _write_report(stem + ".log", m, F.loss_type, _chlg(F), "spatial_cnn"))


def spatial_cnn_test(argv=None) -> Dict[str, np.ndarray]:
    F = _parser("spatial_cnn", False).parse_known_args(argv)[0]
    rank, world = _dist()
    # `test.py:126-128`: --kfold as given (no crossval rule), the checkpoint spelled 'rendezvous' whatever --model says
    logfile = _stem(F, F.kfold) + ".log"
    model = _eval_model("spatial_cnn", F, [_stem(F, F.kfold, model="rendezvous") + ".pth"])
    videos = cholect.extraction_videos(F.dataset_variant, F.kfold)
    labels, mine = _labelled_share(F, videos)
    t0 = time.time()
    feats_local, scores_local = _spatial_cnn_videos(F, model, mine, labels)
    merged = extract.gather_feats(feats_local)
    m = _spatial_recognition(F, scores_local, mine, videos)    # the videos of ALL ranks in file order: N ranks log the 1-rank numbers
    all_feats = {featfile.video_key(v): merged[featfile.video_key(v)] for v in videos}
    if rank == 0:
        featfile.write_feats(featfile.feats_path("..", F.version, F.kfold, F.loss_type), all_feats)
        _log(logfile, f"save time:::::: : {time.time() - t0:.4f} secs")
        _log(logfile, " ".join(f"AP_{k}={m[k].compute_video_AP(ignore_null=_chlg(F))['mAP']:.4f}" for k in m) + f" (all {len(videos)} videos, world={world})")
    return all_feats


# ------------------------------------------------------------------------------------------------ Spatial_cnn/run.py -t
def _augment(im, rng, names):
    """the reference's PIL-side train augmentations (`Spatial_cnn/dataloader.py:89-100`; its dict lists 'contrast' twice, so the later
    RandomAutocontrast is the one in effect; its 'brightness' is RandomAdjustSharpness(1.6, p=0.5)), drawn from `rng` (python `random.Random`)"""
    from PIL import Image, ImageEnhance, ImageOps
    for n in names:
        if n == "vflip" and rng.random() < 0.4:
            im = ImageOps.flip(im)
        elif n == "hflip" and rng.random() < 0.4:
            im = ImageOps.mirror(im)
        elif n == "contrast" and rng.random() < 0.5:
            im = ImageOps.autocontrast(im)
        elif n == "brightness" and rng.random() < 0.5:
            im = ImageEnhance.Sharpness(im).enhance(1.6)
        elif n == "rot90":
            im = im.rotate(rng.uniform(-90.0, 90.0), resample=Image.NEAREST, expand=True)
    return im


def load_train_frames_u8(data_dir, video, frame_ids, height, width, rng, aug_names) -> np.ndarray:
    """`Resize -> augmentations -> Resize` of the train transform (`dataloader.py:153-162`) -> uint8 [N,H,W,3]"""
    from PIL import Image
    out = np.empty((len(frame_ids), height, width, 3), np.uint8)
    for i, fid in enumerate(frame_ids):
        with Image.open(os.path.join(data_dir, "data", video, "{}.png".format(str(int(fid)).zfill(6)))) as im:
            im = im.convert("RGB").resize((width, height), Image.BILINEAR)
            im = _augment(im, rng, aug_names)
            if im.size != (width, height):
                im = im.resize((width, height), Image.BILINEAR)
            out[i] = np.asarray(im)
    return out


def _teacher_files(F, kfold):
    """the teacher prediction / feature files of --loss_type all ({task: {video key: rows}} for i, v, t): the distillation losses read them
    (`dataloader.py:216-238` loads them regardless; a single-task run never uses them)"""
    if F.loss_type != "all":
        return {}, {}
    tdir = lambda ver, task, kind: featfile.feats_path("..", ver, kfold, task, kind)
    return ({t: featfile.read_feats(tdir(F.teacher_pred_version, t, "pred")) for t in "ivt"},
            {t: featfile.read_feats(tdir(F.teacher_feat_version, t, "feats")) for t in "ivt"})


_WARNED_TRANSFORM = False


def _device_transform(F) -> bool:
    """--train_transform device, unless the augmentation list has no device form ('contrast' or 'brightness' after 'rot90': the black fill of
    the rotation would enter the histogram or be sharpened; 'contrast', 'brightness' or 'rot90' named twice) -- such a run keeps the host
    transform; said once"""
    if getattr(F, "train_transform", "host") != "device":
        return False
    from . import augment
    if augment.supported(F.augmentation_list):
        return True
    global _WARNED_TRANSFORM
    if not _WARNED_TRANSFORM:
        print(f"[drivers] --train_transform device: the augmentation list {list(F.augmentation_list)} has no device form ('contrast' or "
              "'brightness' after 'rot90', or 'contrast' / 'brightness' / 'rot90' twice); the train transform runs in Pillow on the host", flush=True)
        _WARNED_TRANSFORM = True
    return False


def _frame_cache(F):
    """--frame_cache GB > 0: this rank's `cholect.FrameCache` (None for 0).  It sits behind the device transform only: with the host transform
    (the flag, or an augmentation list without a device form) Pillow decodes and augments in one go, the training side runs uncached -- said
    once -- and the cache serves the validation frames alone"""
    gb = float(getattr(F, "frame_cache", 0) or 0)
    if gb <= 0:
        return None
    if not _device_transform(F):
        print("[drivers] --frame_cache: the train transform runs in Pillow on the host, which decodes its own frames; training frames are not cached "
              "(validation frames are)", flush=True)
    return cholect.FrameCache(int(gb * 1e9))


def _cache_note(cache):
    """-> (mark, note): `mark()` at the start of a training epoch, `note()` = ' | cache <hits>/<frames>' of the requests since, for its `Traning |` line"""
    at = [0, 0]

    def mark():
        at[:] = [cache.stats["hits"], cache.stats["hits"] + cache.stats["misses"]]

    def note():
        return f" | cache {cache.stats['hits'] - at[0]}/{cache.stats['hits'] + cache.stats['misses'] - at[1]}"
    return mark, note


def _frame_batch(F, batch, labels, tpred, tfeat, size, rng, cache=None):
    """a training batch of (video, frame) samples -> (uint8 frames [B,H,W,3] on the GPU through the train transform at size = (H, W), the
    labels of the i, v, t, ivt heads, the teacher predictions and features of i, v, t -- empty without teacher files).  `cache` (--frame_cache):
    the frames ahead of the device transform go through `cholect.FrameCache.plan` + `fetch`"""
    if _device_transform(F) and cache is not None:
        from . import augment
        paths = [os.path.join(F.data_dir, "data", v, "{}.png".format(str(int(labels[v]["ivt"][i, 0])).zfill(6))) for v, i in batch]
        x = cache.fetch(paths, cache.plan(paths, size[0], size[1]),
                        lambda ps: cholect.load_files_device(ps, size[0], size[1], workers=F.decode_workers, decode=F.png_decode))
        frames = augment.train_transform_device(x, augment.draw_params(rng, F.augmentation_list, len(paths), size[0], size[1]))
    elif _device_transform(F):
        from . import augment
        frames = augment.load_train_batch_device(F.data_dir, [(v, labels[v]["ivt"][i, 0]) for v, i in batch], size[0], size[1], rng,
                                                 F.augmentation_list, decode=F.png_decode, workers=F.decode_workers)
    else:
        frames = torch.from_numpy(np.concatenate([load_train_frames_u8(F.data_dir, v, [labels[v]["ivt"][i, 0]], size[0], size[1], rng,
                                                                       F.augmentation_list) for v, i in batch])).cuda()
    lab = [torch.from_numpy(np.stack([labels[v][k][i, 1:] for v, i in batch])) for k in ("i", "v", "t", "ivt")]
    rows = lambda files: [torch.from_numpy(np.stack([files[t][featfile.video_key(v)][i] for v, i in batch]).astype(np.float32))
                          for t in "ivt"] if files else []
    return frames, lab, rows(tpred), rows(tfeat)


def _sample_tables(F, labels, tpred, tfeat, videos):
    """--prefetch K > 0: the label and teacher rows of the training videos on the device, built once per run (`loader.SampleTables`:
    N x (131 + 31 + 3 x teacher_dim) x 4 bytes with teacher files); None for --prefetch 0, which keeps the synchronous `_frame_batch` path"""
    if getattr(F, "prefetch", 0) <= 0:
        return None
    from .loader import SampleTables
    return SampleTables(labels, tpred, tfeat, videos=videos)


def _frame_validation(F, val_videos, labels, size, cap, forward, label_cache=None, cache=None):
    """validation mAP of the task's head (`run.py:416-451`; ivt for --loss_type all) over the validation videos' frames in device batches of
    max(--batch, min(--device_batch, cap)) (results do not depend on it); forward(uint8 frames) -> the head's logits.  --metrics device: the
    scores stay on the GPU, the label rows come from `label_cache` (the caller's, one per run).  `cache` (--frame_cache): the spans' frames go
    through the run's `cholect.FrameCache` (planned on this thread, span by span), which is sealed when the pass ends"""
    vt = F.loss_type if F.loss_type != "all" else "ivt"
    dev = _device_metrics(F)
    if dev:
        from .metrics_device import DeviceRecognition
    m = (DeviceRecognition if dev else Recognition)({"i": 6, "v": 10, "t": 15, "ivt": 100}[vt])
    vb = max(F.batch, min(F.device_batch, cap))
    label_cache = {} if label_cache is None else label_cache
    for v in val_videos:
        lv = labels[v][vt]
        zv = _label_rows(label_cache, v, lambda v=v: labels[v], dev)[vt]
        load = lambda s0, v=v, lv=lv: cholect.load_frames_device(F.data_dir, v, lv[s0:s0 + vb, 0], size[0], size[1], workers=F.decode_workers, decode=F.png_decode)
        prepare = None
        if cache is not None:
            files = lambda s0, v=v, lv=lv: [os.path.join(F.data_dir, "data", v, "{}.png".format(str(int(fid)).zfill(6))) for fid in lv[s0:s0 + vb, 0]]
            prepare = lambda s0, files=files: cache.plan(files(s0), size[0], size[1])
            load = lambda s0, plan, files=files: cache.fetch(files(s0), plan, lambda ps: cholect.load_files_device(
                ps, size[0], size[1], workers=F.decode_workers, decode=F.png_decode))
        spans = [(s0,) for s0 in range(0, len(lv), vb)]
        for (s0,), fr in zip(spans, extract.iter_chunks(spans, load, 1 if getattr(F, "prefetch", 0) > 0 else 0, prepare=prepare)):      # --prefetch: the next span loads meanwhile
            m.update(zv[s0:s0 + vb], _scores(forward(fr), dev))
        m.video_end()
    if cache is not None:
        cache.seal()
    score = float(m.compute_video_AP(ignore_null=_chlg(F))["mAP"]) if val_videos else 0.0
    return score, f"{vt}: [{score:.5f}]"


def student_start(F, latest: str, resume=None, say=None) -> Dict[str, torch.Tensor]:
    """the state dict `Spatial_cnn/run.py -t` starts from, in the reference's order; host only.  The synthetic fill (no torch.nn init here:
    deterministic synthetic start), then --imagenet_trunk (`BaseModel`'s `resnet18/50(pretrained=True)`, `network.py:100,105`: a torchvision
    file through `checkpoint.torchvision_resnet_to_student`; given but not there, or another architecture's: an error), then --pretrain_dir
    (`run.py:316-317`) and the newest checkpoint `latest` (`load_model`, `:272-278`: the keys present in the model, strict=False; a file that
    is not there is skipped).  A later source wins key by key.  `resume`: --resume's `trainloop.Resume`, whose bytes stand for `latest`;
    `say(line)` gets the one line about the trunk file"""
    from . import checkpoint, shapes, synth
    sd = synth.fill_from_shapes(shapes.spatial_cnn_shapes(F.network, F.student_dim, F.teacher_dim, F.loss_type), seed=F.seed)
    trunk = getattr(F, "imagenet_trunk", "")
    if trunk:
        if not os.path.isfile(trunk):
            raise FileNotFoundError(f"--imagenet_trunk {trunk}: no such file (leave the flag out for the synthetic start)")
        hit, ignored = checkpoint.torchvision_resnet_to_student(torch.load(trunk, map_location="cpu"), F.network)
        sd.update(hit)
        if say:
            say(f"--imagenet_trunk: {len(hit)} tensors from {trunk}, ignored {ignored}")
    if F.pretrain_dir and os.path.exists(F.pretrain_dir):
        sd.update({k: v for k, v in torch.load(F.pretrain_dir, map_location="cpu").items() if k in sd})
    state = _latest_state(latest, resume)
    if state is not None:
        sd.update({k: v for k, v in state.items() if k in sd})
    return sd


def spatial_cnn_train(argv=None) -> Dict[str, float]:
    """`Spatial_cnn/run.py -t` (:296-470): student distillation.  Shuffled frames of all training videos in batches of --batch; with
    torchrun every rank takes its own batch of a step (frame-DDP: global batch = world x --batch), BatchNorm statistics stay per
    GPU and the flat gradient buffer is all-reduced over RCCL once per step.  SGD without momentum, LinearLR warm-up ->
    ExponentialLR per epoch, validation mAP every --val_interval epochs with `_latest.pth` / best `.pth` like `weight_mgt` (:258-269)."""
    import random

    from .spatial_cnn_train import SpatialCnnTrainer
    F = _parser("spatial_cnn", True).parse_known_args(argv)[0]
    if F.loss_type not in ("all", "i", "v", "t"):
        raise ValueError("--loss_type all | i | v | t (`Spatial_cnn/run.py:165-192`)")
    single = F.loss_type != "all"
    guard = dict(_guard(F), **_optim(F), **_ema(F))
    rank, world = _dist()
    kfold = F.kfold if "crossval" in F.dataset_variant else 0
    stem = _stem(F, kfold)
    latest = stem + _LATEST["spatial_cnn"]
    resume = _resume(F, latest, guard["optim"], guard["ema"])
    sd = student_start(F, latest, resume, say=print if rank == 0 else None)
    tr = SpatialCnnTrainer(F.network, lr=F.initial_learning_rates[2], weight_decay=F.weight_decay, rates=F.rates, temp=float(F.temp),
                           teacher_dim=F.teacher_dim, loss_type=F.loss_type,
                           operand_dtype=_dtype(F.operand_dtype), deterministic=_deterministic("spatial_cnn", F), **guard)
    tr.load_state_dict(sd)
    _load_optim(tr, resume)
    train_videos, val_videos, _ = cholect.split_videos(F.dataset_variant, kfold)
    labels = {v: cholect.load_labels(F.data_dir, v) for v in train_videos + val_videos}
    tpred, tfeat = _teacher_files(F, kfold)
    samples = [(v, i) for v in train_videos for i in range(len(labels[v]["ivt"]))]
    order_rng, aug_rng = random.Random(F.seed), random.Random(F.seed * 1000003 + rank)
    size = (F.image_height, F.image_width)
    tables = _sample_tables(F, labels, tpred, tfeat, train_videos)
    cache = _frame_cache(F)                                  # (--frame_cache: this rank's resized frames, resident from their first use on)
    mark, note = _cache_note(cache) if cache is not None else (lambda: None, None)

    def train_epoch(epoch):
        order = list(samples)
        order_rng.shuffle(order)                             # the same permutation on every rank
        mine, tot = deal(order, F.batch, world, rank), LossMean(guard["skip_nonfinite"])
        mark()
        try:
            if tables is not None:                           # --prefetch K: the same batches, loaded ahead in chunks (`loader.FrameLoader`)
                from .loader import FrameLoader
                with FrameLoader(F, mine, labels, tables, size, aug_rng, prefetch=F.prefetch, cache=cache) as batches:
                    for fb in batches:
                        tot.add(tr.train_step(*fb)["loss"])
                batches.check_drained()                      # (--resume saves aug_rng's state behind this epoch: no chunk of it is still to draw)
                return tot.total, tot.steps
            for batch in mine:
                tot.add(tr.train_step(*_frame_batch(F, batch, labels, tpred, tfeat, size, aug_rng, cache))["loss"])
            return tot.total, tot.steps
        finally:
            if cache is not None:
                cache.seal()                                 # what this epoch stored is readable from the next one on

    val_labels = {}                                          # (--metrics device: the validation label rows on the GPU, uploaded once)

    def validate(state):
        model = _eval_model("spatial_cnn", F, state)
        gi = "ivt".index(F.loss_type) if single else 3
        return _frame_validation(F, val_videos, labels, size, 256, lambda fr: model.extract_u8(fr)[gi][1], val_labels, cache)

    return run_epochs(F, tr, rank, train_epoch, validate, stem + ".log", latest, stem + ".pth", score_key="val_mAP_ivt", epoch_note=note,
                      generators={"order_rng": order_rng, "aug_rng": aug_rng}, resume=resume)


# ------------------------------------------------------------------------------------------------ Temporal_tenco/run.py -e
def tenco_eval(argv=None) -> Dict[str, float]:
    F = _parser("tenco", True).parse_known_args(argv)[0]      # (this is the stage's `run.py`: -t trains first)
    _causal(F)
    if F.train:
        _tenco_train(F)
        if not F.test:
            return {}
    return _on_rank0(lambda: _tenco_eval_rank0(F))      # under torchrun the evaluation, its log lines and the mAP pickle belong to rank 0 alone


def _tenco_eval_rank0(F) -> Dict[str, float]:
    stem = _stem(F)
    logfile = stem + ".log"
    model = _eval_model("tenco", F, [stem + ".pth", stem + _LATEST["tenco"]])   # (the shipped scripts pass --test_ckpt ..._latest.pth, Scripts/test_fold1.sh)
    _, _, test_videos = cholect.split_videos(F.dataset_variant, F.kfold)
    feats = featfile.read_feats(featfile.feats_path("..", F.version1, F.kfold, "all"))
    t0 = time.time()
    dev = _device_metrics(F)
    m = _recognition(_tenco_scores(model, feats, test_videos, F.data_dir, dev), test_videos, dev)     # (rank 0 alone runs this pass)
    _log(logfile, f"eta {time.time() - t0:.3f} secs")
    # `run.py:529-570`: the pickled metric objects, then head-wise ('singletest') and disentangled per-category AP and both mean-AP rows
    return _write_report(logfile, m, F.loss_type, _chlg(F), "temporal_tenco", pckl=os.path.join(os.path.dirname(stem), f"mAPs_k{F.kfold}.pckl"))


def _tenco_scores(model, feats, vids, data_dir, device=False, label_cache=None):
    """`test_loop` of `Temporal_tenco/run.py:238-270`: whole video, batch 1, the finest FPN level's logits [K,T] -> sigmoid [T,K].
    device (--metrics device): scores and label rows are device tensors, the label rows uploaded once per video into `label_cache`"""
    out_scores = {}
    label_cache = {} if label_cache is None else label_cache
    for v in vids:
        lab = _label_rows(label_cache, v, lambda v=v: cholect.load_labels(data_dir, v), device)
        x = torch.from_numpy(feats[featfile.video_key(v)]).unsqueeze(0).cuda()
        out, out_i, out_v, out_t, _, _ = model(x, False)
        n = x.shape[1]
        out_scores[v] = {key: (lab[key][:n], _scores(lg[0][0].transpose(0, 1), device)) for key, lg in (("ivt", out), ("i", out_i), ("v", out_v), ("t", out_t))}
    return out_scores


def _tenco_train(F):
    """`Temporal_tenco/run.py -t` (:181-235, :341-348, :260-271): whole-video batch 1, SGD without momentum, LinearLR warm-up ->
    ExponentialLR per epoch, `_latest.pth` after every epoch.  With torchrun the shuffled videos of an epoch are dealt round-robin
    to the ranks (one video per rank per step) and the flat gradient buffer is all-reduced over RCCL each step.

    --mask_draw device: the draws of step i of an epoch are those of `tenco_draws.host_masks(F.seed + rank, epoch * steps_per_epoch + i, ...)`,
    made on the device (`TencoTrainer.train_step(draws=...)`); whole-video steps replay as one hipGraph per length.
    --subclip reference: a training item is `tenco_draws.tenco_clip` of the video (`dataloader.py:219-222`), drawn from a `random.Random(F.seed)`
    of its own for EVERY video of the epoch in shuffled order on every rank (a rank's clips do not depend on the world size); features and label
    rows are sliced on the device (row ranges: no copy) and a clipped step runs eagerly (its length is new almost every time).  Taken whole
    instead: videos of <= 10 frames (`tenco_clip`) and, with --hier, clips too short for the pooled levels (`TencoTrainer.level_lengths`)."""
    import random

    from .tenco_draws import tenco_clip

    from .tenco_train import TencoTrainer
    rank, world = _dist()
    stem = _stem(F)
    if not F.fpn:
        # the reference's own train loop cannot run a model without --fpn: `out_list_i / _v / _t` stay empty (`network.py:56-66`), so `loss_i`,
        # `loss_v`, `loss_t` stay the int 0 they start as (`run.py:190`) and `loss_i.item()` raises AttributeError at `run.py:214` in the first step
        raise NotImplementedError("Temporal_tenco training needs --fpn (Scripts/train_fold1.sh:28): without it the reference's train loop itself fails "
                                  "in its first step (run.py:190,214: .item() on the int 0 that loss_i stays when the model returns no per-component logits)")
    guard = dict(_guard(F), **_optim(F), **_ema(F))
    init = stem + _LATEST["tenco"]
    resume = _resume(F, init, guard["optim"], guard["ema"])
    tr = TencoTrainer(F.num_layers_PG, F.num_layers_R, F.num_R, 512, F.input_dim, lr=F.initial_learning_rates[2], weight_decay=F.weight_decay,
                      hier=bool(getattr(F, "hier", False)),      # --hier True: pooled refinement levels (`network.py:147,154-155`, `run.py:159-179`)
                      causal=bool(getattr(F, "causal", False)),
                      deterministic=_deterministic("tenco", F), **guard)
    from . import shapes, synth
    state = _latest_state(init, resume)
    if state is not None:
        tr.load_state_dict(state)
    else:   # no torch.nn init here: deterministic synthetic start (the reference starts from torch's default init)
        tr.load_state_dict(synth.fill_from_shapes(shapes.tenco_shapes(F.num_layers_PG, F.num_layers_R, F.num_R, 512, F.input_dim, 100, fpn=True),
                                                  seed=F.seed))
    _load_optim(tr, resume)
    train_videos, val_videos, _ = cholect.split_videos(F.dataset_variant, F.kfold)
    feats = featfile.read_feats(featfile.feats_path("..", F.version1, F.kfold, "all"))
    # features and labels of every training video are uploaded ONCE (a per-step pageable host->device copy stalls the step)
    xs, zs = {}, {}
    for v in train_videos:
        lab = cholect.load_labels(F.data_dir, v)
        xs[v] = torch.from_numpy(feats[featfile.video_key(v)]).unsqueeze(0).cuda()
        zs[v] = tr.prepare_labels({k: torch.from_numpy(lab[n][:, 1:]) for k, n in (("", "ivt"), ("_i", "i"), ("_v", "v"), ("_t", "t"))})
    rng = random.Random(F.seed)
    clip_rng = random.Random(F.seed)
    device_draw, subclip = F.mask_draw == "device", F.subclip == "reference"
    clipped = [0, 0]                                               # this rank's steps of the epoch: on a clip, all
    gen = torch.Generator().manual_seed(F.seed + rank)

    def clip(length):                                              # (start, frames) of a training item
        s, n = tenco_clip(clip_rng, length)
        if n != length and tr.hier:
            try:
                tr.level_lengths(n)
            except ValueError:
                return 0, length
        return s, n

    def train_epoch(epoch):
        order = list(train_videos)
        rng.shuffle(order)                                         # same permutation on every rank
        mine, tot = deal(order, 1, world, rank), LossMean(guard["skip_nonfinite"])
        clips = {v: clip(xs[v].shape[1]) for v in order} if subclip else {}
        clipped[:] = [0, len(mine)]
        for i, (v,) in enumerate(mine):
            x, z, whole = xs[v], zs[v], True
            if subclip:
                s, n = clips[v]
                whole = n == x.shape[1]
                clipped[0] += not whole
                x, z = x[:, s:s + n], z[s:s + n]
            if device_draw:                                        # Dropout2d + per-layer Dropout are always on in train mode
                tot.add(tr.train_step(x, z, draws=(F.seed + rank, epoch * len(mine) + i), input_mask=bool(F.mask), use_graph=whole)[0])
                continue
            masks = tr.draw_masks(x.shape[1], gen)
            if not F.mask:                                         # (`network.py:123-127,194-196`); --mask gates the 75 % input mask only
                masks["input_mask"] = None                         # (`network.py:43-48`)
            tot.add(tr.train_step(x, z, masks=masks)[0])
        return tot.total, tot.steps

    dev_metrics, val_labels = _device_metrics(F), {}

    def validate(state):                                           # (`run.py:416-452`): best `.pth` by the triplet mAP
        vmodel = _eval_model("tenco", F, state)
        vm = _recognition(_tenco_scores(vmodel, feats, val_videos, F.data_dir, dev_metrics, val_labels), val_videos, dev_metrics) if val_videos else None
        head = F.loss_type if F.loss_type in ("i", "v", "t") else "ivt"
        score = float(vm[head].compute_video_AP()["mAP"]) if vm else 0.0
        ivt = float(vm["ivt"].compute_video_AP("ivt", ignore_null=_chlg(F))["mAP"]) if vm else 0.0
        return score, f"ivt: [{ivt:.5f}]"

    run_epochs(F, tr, rank, train_epoch, validate, stem + ".log", init, stem + ".pth", latest_every_epoch=True,
               epoch_note=(lambda: f" | clips {clipped[0]}/{clipped[1]}") if subclip else None,
               generators={"rng": rng, "clip_rng": clip_rng, "gen": gen}, resume=resume)
    if rank == 0 and device_draw:
        _log(stem + ".log", f"mask_draw device | subclip {F.subclip} | cached graphs {len(tr._graphs)} | reserved bytes added {tr.graph_reserved_bytes}")


# ------------------------------------------------------------------------------------------------ Spatial_transformer/test.py
def _q2l_chunks(F, v, ids, min_load: int = 1, prefetch: int = 1):
    """the frames `ids` of video v in file order as device chunks of `extraction_batch(...)` frames (a frame's result does not depend on the
    chunk it rides in).  They are loaded -- decoded on --decode_workers threads or on the device -- in whole chunks of at least `min_load`
    frames, `prefetch` loads running ahead of the model (`extract.iter_chunks`)"""
    step = extraction_batch(F.img_size, F.device_batch)
    lb = ((min_load - 1) // step + 1) * step
    load = lambda s, e: cholect.load_frames_device(F.data_dir, v, ids[s:e], F.img_size, F.img_size, workers=F.decode_workers, decode=F.png_decode)
    for span in extract.iter_chunks([(s, min(len(ids), s + lb)) for s in range(0, len(ids), lb)], load, prefetch):
        for s in range(0, span.shape[0], step):
            yield span[s:s + step]


def spatial_transformer_test(argv=None) -> Dict[str, np.ndarray]:
    F = _parser("spatial_transformer", False).parse_known_args(argv)[0]
    # only the CHECKPOINT directory carries the task suffix (`test.py:93-95`; --kfold as given, spelled 'rendezvous'); the feature file goes to
    # run_<version as given> (`test.py:364-372`: `version1`), which is where Temporal_mstct and the student's dataloader look for it
    model = _eval_model("spatial_transformer", F, [_stem(F, F.kfold, task_dir=True, model="rendezvous") + ".pth"])
    labels, mine = _labelled_share(F, cholect.extraction_videos(F.dataset_variant, F.kfold))
    dev_dec = F.png_decode == "device"                         # (the device decoder wants >= 1024 frames per call; two loads run ahead)
    feats_local = {}
    for v in mine:
        # the video's features stay on the GPU until its end: one D2H per video instead of one synchronous copy per --batch frames (`test.py:357-376`)
        chunks = [model(fr)[3][0].float() for fr in _q2l_chunks(F, v, labels[v]["ivt"][:, 0], 1024 if dev_dec else 1, 2 if dev_dec else 1)]
        feats_local[featfile.video_key(v, "transformer")] = torch.vstack(chunks).cpu().numpy()
    merged = extract.gather_feats(feats_local)
    if _dist()[0] == 0:
        featfile.write_feats(featfile.feats_path("..", F.version, F.kfold, F.loss_type), merged)
    return merged


def _q2l_scores(F, model, vids, labels):
    """`test_loop` of `Spatial_transformer/run.py:231-262` over `vids`: device batches in file order (loads of one batch, one running ahead), the
    teacher features the loader hands a `loss_type all` model off the train split are zeros (`dataloader.py:240-246`) -> {video -> {head ->
    (labels, sigmoid scores)}}; heads the model does not have score sigmoid(0) like the reference's zero logits (`network.py:84-89`).
    --metrics device: label rows and scores are fp32 tensors on the GPU"""
    out_scores = {}
    single = F.loss_type != "all"
    dev_met, label_cache = _device_metrics(F), {}
    for v in vids:
        acc = {k: [] for k in ("i", "v", "t", "ivt")}
        for fr in _q2l_chunks(F, v, labels[v]["ivt"][:, 0]):
            zt = [] if single else [torch.zeros((fr.shape[0], F.teacher_dim), device=fr.device)] * 3
            o = model(fr, *zt)
            for gi, key in enumerate(("i", "v", "t", "ivt")):
                acc[key].append(_scores(o[gi][1], dev_met))
        if dev_met:
            rows = _label_rows(label_cache, v, lambda v=v: labels[v], True)
            out_scores[v] = {key: (rows[key], torch.cat(acc[key])) for key in acc}
        else:
            out_scores[v] = {key: (labels[v][key][:, 1:], np.concatenate(acc[key])) for key in acc}
    return out_scores


def spatial_transformer_eval(argv=None) -> Dict[str, float]:
    """`Spatial_transformer/run.py -e` (:482-527): the TEST-split videos through the best checkpoint of run_<version>[_<task>]/ and the closing
    report (per-category AP, mean-AP row; I / V / T from the component heads for a single-task teacher, disentangled from the triplet head for
    --loss_type all).  Videos sharded over the ranks, (labels, scores) gathered on the host (--metrics device: AP rows computed on the GPU),
    rank 0 writes: N ranks log the 1-rank report."""
    F = _parser("spatial_transformer", False).parse_known_args(argv)[0]
    kfold = F.kfold if "crossval" in F.dataset_variant else 0
    stem = _stem(F, kfold, task_dir=True)
    model = _eval_model("spatial_transformer", F, [stem + ".pth"])
    _, _, videos = cholect.split_videos(F.dataset_variant, kfold)
    labels, mine = _labelled_share(F, videos)
    m = _spatial_recognition(F, _q2l_scores(F, model, mine, labels), mine, videos)
    return _on_rank0(lambda: _write_report(stem + ".log", m, F.loss_type, _chlg(F), "spatial_transformer"))


# ------------------------------------------------------------------------------------------------ Temporal_mstct/test.py
def _mstct_windows(model, f: np.ndarray, full=None):
    """the feature matrix f [N,D] in non-overlapping 256-frame chunks, each an independent window, through `model.forward_btd` (`Temporal_mstct/
    test.py:146-174`, loader batch 256): yields its return per chunk.  `full(x)`, when given, runs the full chunks instead"""
    for s in range(0, f.shape[0], 256):
        x = torch.from_numpy(f[s:s + 256]).unsqueeze(0).cuda()
        yield full(x) if full is not None and x.shape[1] == 256 else model.forward_btd(x)


def mstct_test(argv=None):
    F = _parser("mstct", False).parse_known_args(argv)[0]
    # checkpoint directory: run_<version>_<task> for a single-task teacher (`test.py:88-90,131,326`); the feature / prediction files it
    # writes go to run_<version as given> (`test.py:342-366`) and its input comes from run_<version1> (`dataloader_test.py:220`)
    model = _eval_model("mstct", F, [_stem(F, task_dir=True) + _LATEST["mstct"]])
    feats = featfile.read_feats(featfile.feats_path("..", F.version1, F.kfold, F.loss_type))
    out_feats, out_preds = {}, {}
    gi = {"i": 0, "v": 1, "t": 2, "ivt": 3}[F.loss_type]
    graphed = []

    def full(x):                                                                           # full chunks: one hipGraph replay each (~100 launches, launch-bound)
        if not graphed:
            from .graph import GraphedForward
            graphed.append(GraphedForward(lambda xx: model.forward_btd(xx), [x]))
        return graphed[0](x)
    # under torchrun (`Scripts/train_fold1.sh` with NGPU > 1 runs `run.py -t -e`) whole videos are sharded over the ranks like the spatial
    # extractors' (no data-path collective), the per-rank dicts meet in one host-side gather and rank 0 alone writes the two files
    keys = list(feats.keys())
    for ki in extract.shard_videos(keys, [feats[k].shape[0] for k in keys], *_dist()):
        outs = [(o[3][1][0].transpose(0, 1).float().cpu(), o[gi][0][0].float().cpu()) for o in _mstct_windows(model, feats[keys[ki]], full)]
        out_feats[keys[ki]] = torch.vstack([fs for fs, _ in outs]).numpy()                 # concat feature [T,2048]
        out_preds[keys[ki]] = torch.vstack([ps for _, ps in outs]).numpy()                 # raw logits [T,K]
    out_feats, out_preds = extract.gather_feats(out_feats), extract.gather_feats(out_preds)
    out_feats, out_preds = {k: out_feats[k] for k in keys}, {k: out_preds[k] for k in keys}      # file order = input order, whatever the sharding

    def write():                                                                           # the files exist before any rank goes on to the next stage
        featfile.write_feats(featfile.feats_path("..", F.version, F.kfold, F.loss_type, "feats"), out_feats)
        featfile.write_feats(featfile.feats_path("..", F.version, F.kfold, F.loss_type, "pred"), out_preds)
    _on_rank0(write)
    return out_feats, out_preds


def _mstct_scores(model, feats, vids, data_dir, loss_type, device=False, label_cache=None):
    """`test_loop` of `Temporal_mstct/run.py:237-262` behind its batch-256 loaders (`:371,378`): non-overlapping 256-frame chunks, each an
    independent window; the heads the single-task model lacks are zero logits (`network.py:85-99`) = sigmoid 0.5.
    device (--metrics device): scores and label rows are device tensors, the label rows uploaded once per video into `label_cache`"""
    out_scores = {}
    gi = {"i": 0, "v": 1, "t": 2, "ivt": 3}[loss_type]
    label_cache = {} if label_cache is None else label_cache
    for v in vids:
        lab = _label_rows(label_cache, v, lambda v=v: cholect.load_labels(data_dir, v), device)
        key = featfile.video_key(v)
        parts = [_scores(o[gi][0][0], device) for o in _mstct_windows(model, feats[key] if key in feats else feats[v[3:]])]
        p_own = torch.cat(parts) if device else np.concatenate(parts)
        n = p_own.shape[0]                                          # (a feature file may hold fewer frames than the label file lists: the first n)
        half = (lambda a: torch.full(a.shape, 0.5, dtype=torch.float32, device=a.device)) if device else (lambda a: np.full(a.shape, 0.5))
        out_scores[v] = {h: (lab[h][:n], p_own if h == loss_type else half(lab[h][:n])) for h in ("i", "v", "t", "ivt")}
    return out_scores


def mstct_eval(argv=None) -> Dict[str, float]:
    """`Temporal_mstct/run.py -e` (:527-580): the TEST-split videos in 256-frame chunks through the checkpoint of run_<version>[_<task>]/ (best
    `.pth`, else `latest.pth`), the pickled metric objects (`mAPs.pckl` in the working directory, `:546-549`) and the closing report.  Rank 0
    alone (a window takes < 1 ms)."""
    F = _parser("mstct", False).parse_known_args(argv)[0]

    def rank0():
        stem = _stem(F, task_dir=True)
        model = _eval_model("mstct", F, [stem + ".pth", stem + _LATEST["mstct"]])
        feats = featfile.read_feats(featfile.feats_path("..", F.version1, F.kfold, F.loss_type))
        _, _, test_videos = cholect.split_videos(F.dataset_variant, F.kfold)
        dev = _device_metrics(F)
        m = _recognition(_mstct_scores(model, feats, test_videos, F.data_dir, F.loss_type, dev), test_videos, dev)
        return _write_report(stem + ".log", m, F.loss_type, _chlg(F), "temporal_mstct", pckl="mAPs.pckl")
    return _on_rank0(rank0)


def _mstct_train(F):
    """`Temporal_mstct/run.py -t` (:147-235, :345-420): every epoch one random 256-frame window per training video, windows shuffled into
    batches of --batch (31 in Scripts/train_fold1.sh), SGD without momentum under LinearLR warm-up -> ExponentialLR, checkpoint
    `..._lowreslatest.pth` (no underscore: `run.py:268`) in run_<version>[_<task>] after every epoch.  Under torchrun every rank takes its
    own batch of a step (window-DDP, global batch = world x --batch) and the flat gradient buffer is all-reduced over RCCL once per step."""
    import random

    from .mstct_train import NCLS, MstctTrainer, draw_windows
    from . import shapes, synth
    _deterministic("mstct", F)
    guard = dict(_guard(F), **_optim(F), **_ema(F))
    rank, world = _dist()
    lt = F.loss_type
    if lt not in NCLS:
        raise ValueError("Temporal_mstct trains one task at a time: --loss_type i | v | t | ivt (Scripts/train_fold1.sh:16)")
    stem = _stem(F, task_dir=True)
    latest = stem + _LATEST["mstct"]
    resume = _resume(F, latest, guard["optim"], guard["ema"])
    tr = MstctTrainer(*_MSTCT_ARCH, F.input_dim, F.final_embedding_dim, lt, lr=F.initial_learning_rates[2], weight_decay=F.weight_decay,
                      operand_dtype=_dtype(F.operand_dtype), **guard)
    state = _latest_state(latest, resume)
    if state is not None:
        tr.load_state_dict(state)
    else:   # no torch.nn init here: deterministic synthetic start (the reference starts from its trunc_normal_ init)
        tr.load_state_dict(synth.fill_from_shapes(shapes.mstct_shapes(F.input_dim, _MSTCT_ARCH[0], _MSTCT_ARCH[1], _MSTCT_ARCH[3], F.final_embedding_dim, lt), seed=F.seed))
    _load_optim(tr, resume)
    train_videos, val_videos, _ = cholect.split_videos(F.dataset_variant, F.kfold)
    feats = featfile.read_feats(featfile.feats_path("..", F.version1, F.kfold, lt))                # `dataloader.py:220-222`
    xs, zs = {}, {}
    for v in train_videos:                                                                        # uploaded ONCE; windows are device slices
        key = featfile.video_key(v)
        if key not in feats:
            key = v[3:]                                                                           # Spatial_transformer's key style
        xs[v] = torch.from_numpy(feats[key]).to(tr.dev)
        zs[v] = torch.from_numpy(cholect.load_labels(F.data_dir, v)[lt][:, 1:]).to(torch.float32).to(tr.dev)
    lengths = {v: int(xs[v].shape[0]) for v in train_videos}
    short = [v for v, n in lengths.items() if n <= F.num_clips]
    if short:
        raise ValueError(f"videos shorter than the {F.num_clips}-frame training window: {short[:3]} (the reference's sampler fails on them too)")
    order_rng, win_rng = random.Random(F.seed), random.Random(F.seed * 7919 + 1)

    def train_epoch(epoch):
        starts = draw_windows(lengths, win_rng, F.num_clips)                                       # same draw on every rank, before the shuffle
        order = list(train_videos)
        order_rng.shuffle(order)
        mine, tot = deal(order, F.batch, world, rank), LossMean(guard["skip_nonfinite"])
        for s, vids in enumerate(mine):
            x = torch.stack([xs[v][starts[v]:starts[v] + F.num_clips] for v in vids])             # [B,T,D] frame-major
            z = torch.cat([zs[v][starts[v]:starts[v] + F.num_clips] for v in vids])               # [B*T,K]
            tot.add(tr.train_step_btd(x, z, masks=tr.draw_masks_device(len(vids), F.num_clips, F.seed + rank, epoch * len(mine) + s)))
        return tot.total, tot.steps

    dev_metrics, val_labels = _device_metrics(F), {}

    def validate(state):                                                                          # (`run.py:416-452`): best `.pth` by the task's mAP
        vmodel = _eval_model("mstct", F, state)
        vm = _recognition(_mstct_scores(vmodel, feats, val_videos, F.data_dir, lt, dev_metrics, val_labels), val_videos, dev_metrics) if val_videos else None
        score = float(vm[lt].compute_video_AP(ignore_null=_chlg(F))["mAP"]) if vm else 0.0
        return score, f"{lt}: [{score:.5f}]"

    run_epochs(F, tr, rank, train_epoch, validate, stem + ".log", latest, stem + ".pth", latest_every_epoch=True,
               generators={"order_rng": order_rng, "win_rng": win_rng}, resume=resume)


# ------------------------------------------------------------------------------------------------ Spatial_transformer/run.py -t
# `Spatial_transformer/models/backbone.py:31-41` (get_model_path)
SWIN_PRETRAIN_FILES = {"swin_L_384_22k": "swin_large_patch4_window12_384_22k.pth", "swin_B_384_22k": "swin_base_patch4_window12_384_22k.pth",
                       "swin_T_224_1k": "swin_tiny_patch4_window7_224.pth"}


def spatial_transformer_train(argv=None) -> Dict[str, float]:
    """`Spatial_transformer/run.py -t` (:150-229, 296-470): the single-task teachers of the recipe (`Scripts/train_fold1.sh:12`, --loss_type
    i | v | t) and the four-decoder distillation variant (--loss_type all, `run.py:183-197`: hard + DistillKL + feature-MSE terms with --rates,
    teacher predictions / features from the files `dataloader.py:216-238` reads, zeros at validation `:240-246`).  Shuffled
    frames of all training videos in batches of --batch, the train transform at img_size x img_size (`dataloader.py:154-161`), DropPath and
    the transformer's dropout drawn per step on the device, SGD without momentum (`run.py:360`), LinearLR warm-up -> ExponentialLR per
    epoch, validation mAP of the task's head every --val_interval epochs with `_latest.pth` / best `.pth` (`weight_mgt`, :265-277).
    With torchrun every rank takes its own batch of a step and the flat gradient buffer is all-reduced over RCCL once per step."""
    import random

    from .q2l_train import Q2LTrainer
    from . import shapes, synth
    F = _parser("spatial_transformer", True).parse_known_args(argv)[0]
    _deterministic("spatial_transformer", F)
    guard = dict(_guard(F), **_optim(F), **_ema(F))
    if F.loss_type not in ("i", "v", "t", "all"):
        raise ValueError("--loss_type i | v | t | all (`Spatial_transformer/run.py:168-197`)")
    single = F.loss_type != "all"
    F.student_dim = F.hidden_dim                                             # `run.py:93`
    rank, world = _dist()
    kfold = F.kfold if "crossval" in F.dataset_variant else 0
    stem = _stem(F, kfold, task_dir=True)
    logfile, latest = stem + ".log", stem + _LATEST["spatial_transformer"]
    resume = _resume(F, latest, guard["optim"], guard["ema"])
    tr = Q2LTrainer(F.backbone, F.img_size, F.hidden_dim, F.loss_type, lr=F.initial_learning_rates[2], weight_decay=F.weight_decay,
                    drop_path_rate=F.drop_path_rate, operand_dtype=_dtype(F.operand_dtype),
                    teacher_dim=F.teacher_dim, rates=F.rates, temp=float(F.temp), **guard)
    table = shapes.q2l_param_shapes(F.backbone, F.img_size, F.hidden_dim, F.loss_type, teacher_dim=F.teacher_dim)
    sd = synth.fill_from_shapes(table, seed=F.seed)          # deterministic synthetic start when no pretrained file is on disk
    # `build_backbone` (`backbone.py:188-196`): the upstream Swin checkpoint ../Pretrain/<file> ('model' entry, `head.*` dropped) into the backbone
    swin_file = os.path.join("..", "Pretrain", SWIN_PRETRAIN_FILES.get(F.backbone, ""))
    if os.path.isfile(swin_file):
        up = torch.load(swin_file, map_location="cpu")
        up = up.get("model", up)
        hit = {"backbone.0." + k: v for k, v in up.items() if "head" not in k and ("backbone.0." + k) in sd and tuple(v.shape) == tuple(sd["backbone.0." + k].shape)}
        sd.update(hit)
        if rank == 0:
            _log(logfile, f"backbone: {len(hit)} tensors from {swin_file}")
    if F.pretrain_dir and os.path.exists(F.pretrain_dir):    # `load_model` (:280-287): keys present in the model, strict=False
        sd.update({k: v for k, v in torch.load(F.pretrain_dir, map_location="cpu").items() if k in sd})
    state = _latest_state(latest, resume)
    if state is not None:
        sd.update({k: v for k, v in state.items() if k in sd})
    tr.load_state_dict(sd)
    _load_optim(tr, resume)
    train_videos, val_videos, _ = cholect.split_videos(F.dataset_variant, kfold)
    labels = {v: cholect.load_labels(F.data_dir, v) for v in train_videos + val_videos}
    samples = [(v, i) for v in train_videos for i in range(len(labels[v]["ivt"]))]
    tpred, tfeat = _teacher_files(F, kfold)
    order_rng, aug_rng = random.Random(F.seed), random.Random(F.seed * 1000003 + rank)
    size = (F.img_size, F.img_size)
    tables = _sample_tables(F, labels, tpred, tfeat, train_videos)
    cache = _frame_cache(F)                                  # (--frame_cache: this rank's resized frames, resident from their first use on)
    mark, note = _cache_note(cache) if cache is not None else (lambda: None, None)

    def train_epoch(epoch):
        from contextlib import nullcontext
        order = list(samples)
        order_rng.shuffle(order)                             # the same permutation on every rank
        mine, tot = deal(order, F.batch, world, rank), LossMean(guard["skip_nonfinite"])
        mark()
        if tables is not None:                               # --prefetch K: the same batches, loaded ahead in chunks (`loader.FrameLoader`)
            from .loader import FrameLoader
            source = FrameLoader(F, mine, labels, tables, size, aug_rng, prefetch=F.prefetch, cache=cache)
        else:
            source = nullcontext(_frame_batch(F, batch, labels, tpred, tfeat, size, aug_rng, cache) for batch in mine)
        try:
            with source as loaded:
                for s, (batch, (frames, lab, tp, tf)) in enumerate(zip(mine, loaded)):
                    masks = tr.draw_masks_device(len(batch), F.seed * 1000003 + rank, epoch * len(mine) + s)     # (a running step count)
                    if single:
                        tot.add(tr.train_step(frames, lab["ivt".index(F.loss_type)], masks))
                    else:
                        tot.add(tr.train_step(frames, lab, masks, teacher_pred=tp, teacher_feat=tf)["loss"])
            if tables is not None:
                source.check_drained()                       # (--resume saves aug_rng's state behind this epoch: no chunk of it is still to draw)
        finally:
            if cache is not None:
                cache.seal()                                 # what this epoch stored is readable from the next one on
        return tot.total, tot.steps

    val_labels = {}                                          # (--metrics device: the validation label rows on the GPU, uploaded once)

    def validate(state):                                     # the task's head (:416-421, 443-450)
        model = _eval_model("spatial_transformer", F, state)
        gi = "ivt".index(F.loss_type) if single else 3
        zt = lambda fr: [] if single else [torch.zeros((fr.shape[0], F.teacher_dim), device=fr.device)] * 3   # (`dataloader.py:240-246`: zeros off the train split)
        return _frame_validation(F, val_videos, labels, size, 128, lambda fr: model(fr, *zt(fr))[gi][1], val_labels, cache)

    return run_epochs(F, tr, rank, train_epoch, validate, logfile, latest, stem + ".pth", epoch_note=note,
                      generators={"order_rng": order_rng, "aug_rng": aug_rng}, resume=resume)


# ------------------------------------------------------------------------------------------------ predict.py (no reference counterpart)
def _predict_parser() -> argparse.ArgumentParser:
    """the shared flags, the stage flags of the student (`spatial_cnn`) and of the temporal head (`tenco`), and predict.py's own"""
    p = argparse.ArgumentParser()
    _common(p)
    for stage in ("spatial_cnn", "tenco"):
        for names, kw in _FLAGS[stage][0]:
            p.add_argument(*names, **kw)
    p.add_argument("--student_ckpt", type=str, default="", help="the student's checkpoint (required)")
    p.add_argument("--temporal_ckpt", type=str, default="", help="a Temporal_tenco checkpoint; empty: the student's own heads are decoded")
    p.add_argument("--frames_dir", type=str, action="append", default=[], help="a directory of *.png, one video, frames in sorted name order; may be repeated")
    p.add_argument("--videos", type=str, nargs="*", default=[], help="videos read from <data_dir>/data/<video>")
    p.add_argument("--out", type=str, default="./predictions")
    p.add_argument("--topk", type=int, default=5)
    p.add_argument("--threshold", type=float, default=0.5)
    p.add_argument("--names", type=str, default="", help="one line per triplet id, with an optional `id:` prefix")
    p.add_argument("--save_scores", action="store_true", help="the four heads' full sigmoid score matrices into the .npz")
    p.add_argument("--segments", action="store_true", help="also <video>.segments.csv: runs of frames in which a triplet is above --threshold")
    p.add_argument("--online", action="store_true",
                   help="frame-by-frame mode (needs --causal and --temporal_ckpt): frames go through the student and `tenco_stream.TencoStream` "
                        "--online_chunk at a time, each answer computed from the frames seen so far; the log line adds per-chunk latencies")
    p.add_argument("--online_chunk", type=int, default=1, help="frames per step of --online, 1..32")
    p.add_argument("--online_streams", type=int, default=1,
                   help="videos answered at once by --online, 1..64: each tick takes --online_chunk frames of every open video through one "
                        "student pass and one `tenco_stream.StreamBank` push; the files are those of 1, a closing line reports the ticks")
    p.add_argument("--localize", type=str, default="off", choices=["off", "i", "ivt"],
                   help="where in the frame each top-K triplet is: class-activation maps of the student's instrument head (i: the column of the "
                        "triplet's instrument) or triplet head (ivt: the triplet's own column); adds loc_* arrays to the .npz and <video>.loc.csv")
    p.add_argument("--localize_frac", type=float, default=0.5,
                   help="the region around a map's peak: the connected cells with map >= min + frac * (max - min), 0..1")
    p.add_argument("--save_maps", action="store_true", help="with --localize: also the top-K maps themselves, loc_maps [T, k, h, w], into the .npz")
    return p


def _predict_inputs(F):
    """everything of predict.py's command line that can be wrong, looked at BEFORE any model is built -> ([(video name, frame paths)], triplet
    names or None); every message names its flag"""
    from . import ops, predict as P
    _causal(F)
    if not 1 <= F.online_streams <= ops.STREAM_MAX_SLOTS:
        raise ValueError(f"--online_streams {F.online_streams}: 1..{ops.STREAM_MAX_SLOTS} videos at once")
    if F.online_streams > 1 and not F.online:
        raise ValueError(f"--online_streams {F.online_streams} needs --online: only the frame-by-frame mode answers several videos at once")
    if F.online:
        if not F.causal:
            raise ValueError("--online needs --causal: a head that pads symmetrically needs frames that have not arrived yet")
        if not F.temporal_ckpt:
            raise ValueError("--online needs --temporal_ckpt FILE: it is the temporal head that streams")
        if not 1 <= F.online_chunk <= ops.STREAM_MAX_CHUNK:
            raise ValueError(f"--online_chunk {F.online_chunk}: 1..{ops.STREAM_MAX_CHUNK}")
        if _dtype(F.dtype) != torch.float32:
            raise ValueError(f"--online with --dtype {F.dtype}: the streaming step (mt4_tcn_stream_conv_f32) is fp32 only")
    if F.save_maps and F.localize == "off":
        raise ValueError("--save_maps needs --localize i or --localize ivt: there are no maps to save")
    if not 0.0 <= F.localize_frac <= 1.0:
        raise ValueError(f"--localize_frac {F.localize_frac}: a fraction of the map's range, 0..1")
    if F.localize != "off" and F.loss_type not in (F.localize, "all"):
        raise ValueError(f"--localize {F.localize} with --loss_type {F.loss_type}: that student has no {F.localize} head to map")
    if not F.student_ckpt:
        raise ValueError("--student_ckpt FILE is required")
    for flag, path in (("--student_ckpt", F.student_ckpt), ("--temporal_ckpt", F.temporal_ckpt), ("--names", F.names)):
        if path and not os.path.isfile(path):
            raise FileNotFoundError(f"{flag} {path}: no such file")
    if not 1 <= F.topk <= ops.TOPK_MAX_K:
        raise ValueError(f"--topk {F.topk}: 1..{ops.TOPK_MAX_K}")
    if not 0.0 < F.threshold < 1.0:
        raise ValueError(f"--threshold {F.threshold}: a score strictly between 0 and 1")
    dirs = [("--frames_dir", os.path.basename(os.path.normpath(d)) or "video", d) for d in F.frames_dir]
    dirs += [("--videos", v, os.path.join(F.data_dir, "data", v)) for v in F.videos]
    if not dirs:
        raise ValueError("nothing to predict: give --frames_dir DIR (may be repeated) or --videos VID ...")
    videos = []
    for flag, name, d in dirs:
        if not os.path.isdir(d):
            raise FileNotFoundError(f"{flag} {name}: {d} is not a directory")
        frames = sorted(f for f in os.listdir(d) if f.lower().endswith(".png"))
        if not frames:
            raise ValueError(f"{flag} {name}: no *.png in {d}")
        if name in [n for n, _ in videos]:
            raise ValueError(f"{flag} {name}: two videos of this name would write the same files in --out")
        videos.append((name, [os.path.join(d, f) for f in frames]))
    return videos, P.parse_names(F.names) if F.names else None


def predict(argv=None):
    """`MT4MTLKD/predict.py`: frames -> per-frame top-K triplets in one pass and one process.  Every video (a --frames_dir directory, or
    --videos under --data_dir/data) goes through `predict.Predictor`: PNG decode + Resize, the student in passes of --device_batch, the
    whole-video TCN of --temporal_ckpt on the features left on the device (without it: the student's own heads), `mt4_topk_rows_f32`, one D2H
    copy; --out/<video>.npz and .csv (`Prediction.save`), with --segments also <video>.segments.csv.  No label file is opened.
    --online: frame by frame (`Predictor._online_parts`); with --online_streams S > 1, S videos at once (`Predictor.predict_streams`), the same
    files and one closing line about the ticks.  -> {video -> Prediction}"""
    from . import predict as P
    F = _predict_parser().parse_known_args(argv)[0]
    videos, names = _predict_inputs(F)
    F.test_ckpt = None                                               # (the files are --student_ckpt / --temporal_ckpt, whatever --test_ckpt says)
    student = _eval_model("spatial_cnn", F, [F.student_ckpt])
    temporal = _eval_model("tenco", F, [F.temporal_ckpt]) if F.temporal_ckpt else None
    if temporal is None:
        print("no --temporal_ckpt: the student's own i / v / t / ivt heads are decoded, frame by frame", flush=True)
    pr = P.Predictor(student, temporal, height=F.image_height, width=F.image_width, device_batch=F.device_batch, png_decode=F.png_decode,
                     decode_workers=F.decode_workers, topk=F.topk, threshold=F.threshold, online_chunk=F.online_chunk if F.online else 0,
                     online_streams=F.online_streams, localize=None if F.localize == "off" else F.localize, localize_frac=F.localize_frac,
                     localize_maps=F.save_maps)
    if F.localize != "off":
        print(f"--localize {F.localize}: each top-K triplet is localised by the student's {'instrument' if F.localize == 'i' else 'triplet'} head "
              f"(class-activation maps, region at {F.localize_frac:g} of the map's range{', maps saved' if F.save_maps else ''})", flush=True)
    os.makedirs(F.out, exist_ok=True)
    out = {}

    def done(name, pred, lat, t0):
        pred.save(os.path.join(F.out, name), names)
        note = ""
        if F.segments:
            segs = P.segments(pred)
            P.save_segments(os.path.join(F.out, name + ".segments.csv"), segs, pred.frames, names)
            note = f" | {len(segs)} segments"
        if F.online:
            lat = np.asarray(lat)
            note += f" | online, {F.online_chunk} frames per chunk: median {float(np.median(lat)):.3f} ms, max {float(lat.max()):.3f} ms per chunk"
        print(f"{name}: {len(pred.frames)} frames | {float(pred.n_active.mean()):.2f} triplets above {F.threshold:g} per frame{note} | {time.time() - t0:.3f} s", flush=True)
        out[name] = pred

    if F.online_streams > 1:
        for name, pred, lat, t0 in pr.predict_streams(videos, keep_scores=F.save_scores):
            done(name, pred, lat, t0)
        lat = np.asarray(pr.tick_latencies_ms)
        print(f"online, {F.online_streams} streams: {len(lat)} ticks | median {float(np.median(lat)):.3f} ms, max {float(lat.max()):.3f} ms per tick | "
              f"median {float(np.median(pr.tick_frames)):g} frames per tick", flush=True)
        return {name: out[name] for name, _ in videos}
    for name, paths in videos:
        t0 = time.time()
        try:
            pred = pr.predict_paths(paths, keep_scores=F.save_scores)
        except ValueError as e:                                      # (--hier on a video too short for the pooled levels: the model's own words)
            raise ValueError(f"{name} ({len(paths)} frames): {e}") from e
        done(name, pred, pr.chunk_latencies_ms, t0)
    return out


# ------------------------------------------------------------------------------------------------ run.py: -t, then -e
def _run(argv, train, evaluate):
    """a stage's `run.py`: -t trains, -e evaluates the test split and writes the closing report; -> the evaluation's result, else the training's"""
    argv = list(sys.argv[1:] if argv is None else argv)
    last = train(argv) if "-t" in argv or "--train" in argv else None
    return evaluate(argv) if "-e" in argv or "--test" in argv else last


def spatial_cnn_run(argv=None):
    """`Spatial_cnn/run.py`: -t trains the student (`spatial_cnn_train`), -e evaluates the test split and writes the closing report
    (`spatial_cnn_eval`, `run.py:503-560`); the extraction pass over all videos is `test.py` (`spatial_cnn_test`)."""
    return _run(argv, spatial_cnn_train, spatial_cnn_eval)


def spatial_transformer_run(argv=None):
    """`Spatial_transformer/run.py`: -t trains the teacher (`spatial_transformer_train`), -e evaluates the test split and writes the closing
    report (`spatial_transformer_eval`, `run.py:482-527`); the extraction pass over all videos is `test.py` (`spatial_transformer_test`)."""
    return _run(argv, spatial_transformer_train, spatial_transformer_eval)


def mstct_run(argv=None):
    """`Temporal_mstct/run.py`: -t trains the MS-TCT teacher on random 256-frame windows (`run.py:147-235`), -e evaluates the test split and
    writes the closing report + `mAPs.pckl` (`mstct_eval`, `run.py:527-580`); features / raw predictions for the student come from `test.py`
    (`mstct_test`)."""
    return _run(argv, lambda a: _mstct_train(_parser("mstct", True).parse_known_args(a)[0]), mstct_eval)
