"""worker of tests/test_gpu_optimizer_train.py: three DDP steps of the TCN trainer with optimizer state under --skip_nonfinite, one video per
rank (both ranks on cuda:0, gloo transport), once with Nesterov momentum and once with AdamW.  Step 2: rank 1's video holds one +Inf -- every
rank must skip and keep P, the state buffers and the step count.  The state is never exchanged: it must still be the same on both ranks."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
import torch.distributed as dist
from ddp_guarded_worker import poisoned, trainer
from ddp_tenco_worker import video
from computervision_codes_amd.flatparams import Optim

RULES = {"nesterov": Optim("sgd", 0.9, True), "adamw": Optim("adamw")}

if __name__ == "__main__":
    out_dir = sys.argv[1]
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    out = {}
    for name, rule in RULES.items():
        tr = trainer(skip_nonfinite=True, optim=rule)
        snaps = []
        for step in range(3):
            x, labels = poisoned(rank) if step == 1 else video(rank)
            tr.train_step(x.cuda(), labels)
            snaps.append({"P": tr.P.cpu().clone(), "S": {k: v.cpu().clone() for k, v in tr.fp.S.items()}, "record": tr.optim_record(),
                          "skip": tr.guard_state()["skip"]})
        out[name] = {"snaps": snaps, "stats": tr.guard_stats(), "osd": tr.optimizer_state_dict()}
    torch.save(out, os.path.join(out_dir, f"ddp_optim_rank{rank}.pth"))
    dist.barrier()
    dist.destroy_process_group()
