"""Device time of the optimizer update kernels inside the training step, at the benchmark shape (256x256, batch 16, bf16).

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 scripts/prof_optimizers.py
  python3 scripts/prof_optimizers.py --summary DIR N        (N: the "elements per update" line the run printed)

The first form runs one warm and four eager train steps per optimizer (a Trainer each on one model); the second reads
rocprofv3's kernel_stats CSV and prints the update kernels with their bytes per element and the rate that implies."""
import csv
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# kernel-name fragment -> (label, HBM bytes per element: parameter and state read + written, gradient read)
KERNELS = [("adadelta_kernel", "Adadelta  isa_adadelta", 20), ("AdamOp", "Adam      isa_adam update", 28),
           ("adam_prepare_kernel", "Adam      isa_adam prepare", 0), ("RmspropOp", "RMSprop   isa_rmsprop", 20),
           ("SgdOp", "SGD       isa_sgd", 20), ("sqnorm_kernel", "all       isa_sqnorm", 4)]


def run():
    import torch
    import isa_amd  # noqa: F401
    from isa_amd.data import synth_batch
    from isa_amd.reseg import ReSeg
    from isa_amd.trainer import OPTIMIZERS, Trainer
    torch.manual_seed(1000)
    model = ReSeg(2, True, dtype=torch.bfloat16)
    model.reset_parameters(seed=23)
    model.train()
    x, sem, ins, n = synth_batch(16, 256, 256, seed=100)
    x, sem, ins = x.cuda(), sem.cuda(), ins.cuda()
    sel = [list(range(int(k))) for k in n.view(-1)]
    start = model.store.flat.clone()
    for name in OPTIMIZERS:
        model.store.flat.copy_(start)
        model.mark_weights_dirty()
        tr = Trainer(model, lr={"Adadelta": 1.0, "SGD": 1e-2}.get(name, 1e-3), optimizer=name)
        for _ in range(5):
            tr.train_step(x, sem, ins, n, selected_idx=sel)
        torch.cuda.synchronize()
        assert torch.isfinite(model.store.flat).all(), name
    print("elements per update: %d" % model.store.n_train)


def summary(path, n):
    files = glob.glob(path + "/**/*kernel_stats.csv", recursive=True)
    rows = list(csv.DictReader(open(files[0])))
    print("update kernels inside the eager train step, 256x256 batch 16 bf16, n = %d fp32 elements" % n)
    for frag, label, bpe in KERNELS:
        for r in rows:
            if frag in r["Name"]:
                avg = float(r["AverageNs"]) / 1e3
                rate = "  %4d B/element -> %5.2f TB/s" % (bpe, bpe * n / avg / 1e6) if bpe else ""
                print("%-28s calls %3s  avg %7.1f us  min %7.1f  max %7.1f%s" % (
                    label, r["Calls"], avg, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3, rate))


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "--summary":
        summary(sys.argv[2], int(sys.argv[3]))
    else:
        run()
