"""worker of tests/test_gpu_weight_ema_train.py: two DDP steps of the TCN trainer with a weight average, one video per rank (both ranks on
cuda:0, gloo transport).  The average is never exchanged: it must still be the same on both ranks.  Every step's exchanged gradient (the SUM
over ranks, as the all-reduce leaves it in G) is saved, so that a one-rank trainer can take the same steps from it."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
import torch.distributed as dist
from ddp_guarded_worker import trainer
from ddp_tenco_worker import video
from computervision_codes_amd.flatparams import Ema

EMA = Ema(0.9, True)

if __name__ == "__main__":
    out_dir = sys.argv[1]
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    tr = trainer(deterministic=True, ema=EMA)
    snaps = []
    for step in range(2):
        x, labels = video(rank, T=37 + 4 * step)
        tr.train_step(x.cuda(), labels)
        snaps.append({"G": tr.G.cpu().clone(), "P": tr.P.cpu().clone(), "E": tr.fp.S["ema"].cpu().clone(), "record": tr.ema_record()})
    torch.save({"snaps": snaps, "ema_state_dict": tr.ema_state_dict()}, os.path.join(out_dir, f"ddp_ema_rank{rank}.pth"))
    dist.barrier()
    dist.destroy_process_group()
