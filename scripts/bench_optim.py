"""Timing of one optimiser step over the flat state of ResNet-18 and of ViT-B, each with the default projector (8192 hidden, 256 out):
the fused flat LARS (sa_lars_flat_step, two launches), utils.LARS tensor by tensor (sa_lars_step, a memset and two launches per adapted
tensor) and the fused AdamW (sa_adamw_step_dev, two launches).  Device events around K steps after a warm-up; bytes per step are the
algorithmic traffic (LARS: 8 B / parameter in pass 1 + 22 B in pass 2; AdamW: 30 B), not a measurement.  For per-kernel times run it
under `rocprofv3 --kernel-trace --stats`."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from ssl_audio_amd import hyperparameters as hp, model, utils
from ssl_audio_amd.train import FlatState

STEPS = int(os.environ.get("SA_OPT_STEPS", "20"))
WARMUP = int(os.environ.get("SA_OPT_WARMUP", "5"))


def timeit(fn):
    for _ in range(WARMUP):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(STEPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / STEPS * 1e3                      # us per step


def bench(model_type, dev):
    cfg = hp.make_args(model_type=model_type, batch_size=128)
    torch.manual_seed(0)
    bb = model.ModelWrapper(cfg)
    net = utils.MultiCropWrapper(bb, model.BarlowTwinsHead(cfg, bb.feature_dim)).to(dev)
    flat = FlatState(list(net.named_parameters()), dev)
    flat.grads.normal_(0, 1e-3)
    n = sum(p.numel() for _, p in flat._trainable())
    flat.stage_hyper(0.1, lr_nodecay=0.001)
    skip = torch.zeros(1, dtype=torch.int32, device=dev)
    out = {"model": model_type, "params": n, "flat_elements": flat.n_train}
    out["lars_fused_us"] = timeit(lambda: flat.lars_staged(1e-5, skip_flag=skip))
    out["adamw_fused_us"] = timeit(lambda: flat.adamw_staged(0.05, skip_flag=skip))
    # the per-tensor form over the same (flat-backed) parameters, gradients bound as .grad views of the flat gradient buffer
    w = [p for p in net.parameters() if p.ndim != 1]
    b = [p for p in net.parameters() if p.ndim == 1]
    for name, p in flat._trainable():
        off, cnt = flat.offsets[name]
        p.grad = flat.grads[off:off + cnt].view(p.shape)
    opt = utils.LARS([{"params": w, "lr": 0.1}, {"params": b, "lr": 0.001}], lr=0, weight_decay=1e-5, weight_decay_filter=True,
                     lars_adaptation_filter=True)
    out["lars_per_tensor_us"] = timeit(opt.step)
    out["lars_bytes_per_step"] = n * (8 + 22)
    out["adamw_bytes_per_step"] = n * 30
    for k in ("lars_fused", "adamw_fused", "lars_per_tensor"):
        out[k + "_TBps"] = round(out["lars_bytes_per_step" if k.startswith("lars") else "adamw_bytes_per_step"] / out[k + "_us"] / 1e6, 3)
    out["lars_over_adamw"] = round(out["lars_fused_us"] / out["adamw_fused_us"], 3)
    return out


def main():
    dev = torch.device("cuda:0")
    for mt in ("resnet18", "vit_base"):
        print(json.dumps(bench(mt, dev)))


if __name__ == "__main__":
    main()
