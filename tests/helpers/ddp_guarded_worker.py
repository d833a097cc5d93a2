"""worker of tests/test_gpu_guarded_train.py: two DDP steps of the TCN trainer under --skip_nonfinite, one video per rank (both ranks on
cuda:0, gloo transport).  Step 1: rank 1's video holds one +Inf -- every rank must skip.  Step 2: clean videos -- sgd of the mean gradient."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
import torch.distributed as dist
from ddp_tenco_worker import CFG, video
from computervision_codes_amd import shapes, synth
from computervision_codes_amd.tenco_train import TencoTrainer


def trainer(**kw):
    sd = synth.fill_from_shapes(shapes.tenco_shapes(CFG["num_layers_PG"], CFG["num_layers_R"], CFG["num_R"], CFG["num_f_maps"], CFG["dim"], 100, fpn=True), seed=8)
    return TencoTrainer(CFG["num_layers_PG"], CFG["num_layers_R"], CFG["num_R"], CFG["num_f_maps"], CFG["dim"], lr=0.05, weight_decay=1e-5, **kw).load_state_dict(sd)


def poisoned(rank):
    x, labels = video(rank)
    if rank == 1:
        x = x.clone()
        x.view(-1)[x.numel() // 2] = float("inf")
    return x, labels


if __name__ == "__main__":
    out_dir = sys.argv[1]
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    tr = trainer(skip_nonfinite=True, clip_grad_norm=1e9)
    before = tr.state_dict()
    x, labels = poisoned(rank)
    tr.train_step(x.cuda(), labels)
    after_bad, stats_bad, state_bad = tr.state_dict(), tr.guard_stats(), tr.guard_state()
    x, labels = video(rank)
    tr.train_step(x.cuda(), labels)
    torch.save({"before": before, "after_bad": after_bad, "stats_bad": stats_bad, "state_bad": state_bad, "after_clean": tr.state_dict(),
                "stats": tr.guard_stats()}, os.path.join(out_dir, f"ddp_guarded_rank{rank}.pth"))
    dist.barrier()
    dist.destroy_process_group()
