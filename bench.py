#!/usr/bin/env python3
"""Headline benchmark: clips/sec of the Barlow Twins pre-training step (10 s @ 16 kHz -> 64-mel, ViT-B, BT loss).

  python bench.py --gpus N --steps K --warmup W

N > 1: one rank per GPU over RCCL.  Under a launcher (RANK / WORLD_SIZE in the environment, e.g. `python -m torch.distributed.run
--nproc-per-node N bench.py --gpus N ...`) this process IS a rank; without one it starts the ranks itself as a child
`torch.distributed.run` (before anything here touches a GPU), forwards rank 0's JSON line and returns the child's exit code.

One "step" = one pass of the whole hot path over one batch of synthetic waveforms already resident in HBM:
log-mel frontend -> 2 augmented views -> encoder+projector fwd -> BT loss -> bwd -> grad all-reduce -> AdamW.
Per-GPU batch is fixed (weak scaling): 128 clips/GPU, i.e. BASELINE config 3 (global batch 1024) at N = 8.
Rank 0 prints ONE JSON line (metric, value, roofline of the dominant kernel, CPU baseline).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

WORKLOADS = {
    # name: (model_type, seconds, clips per GPU, mode)
    "vit_base_bt_10s": ("vit_base", 10.0, 128, "bt"),        # BASELINE configs[2] per-GPU shard (metric's config)
    "vit_tiny_bt_10s": ("vit_tiny", 10.0, 256, "bt"),        # BASELINE configs[1]
    "vit_base_byol_10s": ("vit_base", 10.0, 128, "byol"),    # BASELINE configs[3]
    "vit_large_mae_10s": ("vit_large", 9.92, 256, "mae"),    # BASELINE configs[4]: ViT-L, 75 % masking + reconstruction, T = 992
}
GF_PER_CLIP = {"vit_base_bt_10s": 268.2, "vit_tiny_bt_10s": 19.5, "vit_base_byol_10s": 357.6,
               # config 5 as main.py runs it: view 1 masked (63 tokens) + decoder, view 2 UNMASKED ViT-L: 3 * (156.6 + 38.6 + 4.0) GF
               "vit_large_mae_10s": 597.6}
PEAK_BF16_TFLOPS = 2500.0      # MI355X dense bf16 MFMA (MI355X_MICROARCH.md)
PEAK_F32_VALU_TFLOPS = 157.3   # MI355X_MICROARCH.md: 256 CUs x 256 FLOP/clk x 2.4 GHz (fp32 vector, FMA)
PEAK_HBM_GBS = 8000.0          # HBM3E spec (MI355X_MICROARCH.md: 6.29 TB/s measured with a float4 copy)


def source_sha():
    """Hash of the GEMM kernel sources: profiles/rNN_gemm_traffic.json (HBM bytes of the GEMM launches) carries the hash it was collected
    at and is ignored when stale."""
    import hashlib
    h = hashlib.sha256()
    for f in ("gemm_bf16.hip", "gemm_phase.hip", "gemm_stream.hip", "gemm_common.h", "common.h"):
        h.update(open(os.path.join(ROOT, "ssl_audio_amd", "csrc", f), "rb").read())
    return h.hexdigest()[:16]


def executed_gflop_per_clip(model_type, mode, N):
    """Matmul FLOPs the step really EXECUTES per clip (2 views, forward + backward = 3 x forward).  Differs from the algorithmic
    GF_PER_CLIP (what `value`'s metric is priced in) where the engine skips work exactly: with CLS pooling the last
    block runs proj / MLP (and the attention queries) for the CLS row only (engine.block_forward_cls)."""
    size = model_type.split("_")[-1]
    d, L, H = {"tiny": (192, 12, 3), "small": (384, 12, 6), "base": (768, 12, 12), "large": (1024, 24, 16)}[size]
    if mode == "mae":
        return None                                  # masked + decoder passes: reported from the algorithmic figure only
    full = 24.0 * N * d * d + 4.0 * N * N * d        # one block, all rows: qkv 6, proj 2, fc1 8, fc2 8 (x N d^2) + attention
    pruned = 6.0 * N * d * d + 18.0 * d * d + 4.0 * N * d        # last block: qkv for all rows, the rest for the CLS row only
    view = (L - 1) * full + pruned + 2.0 * (N - 1) * 256 * d + 2.0 * (d * 8192 + 8192 * 256)
    passes = 8.0 if mode == "byol" else 6.0          # byol: online fwd+bwd (3) x 2 views + target fwd x 2 views
    return view * passes / 1e9


def cpu_baseline(workload, budget_clips=8, steps=16):
    """The oracle (CPU restatement of the reference path) timed on this box's host cores on a bounded sample of the SAME step the
    GPU leg runs: oracle.step.bt_step (bt), bt_byol_step with EMA target + predictor (byol), mae_step with 75 % masking (mae)."""
    from oracle import step as ostep, vit as ovit
    from ssl_audio_amd.selfcheck import synthetic_waveforms
    from oracle import frontend as ofe, augment as oaug
    import numpy as np
    model_type, seconds, _, mode = WORKLOADS[workload]
    size = model_type.split("_")[-1]
    avail = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    cores = min(avail, 32)                        # measured: 256 threads on this small batch is 50x SLOWER than 32 (oversubscription)
    torch.set_num_threads(cores)
    n_samples = int(seconds * 16000)
    T = n_samples // 160 + 1
    if mode == "mae":
        T = T // 16 * 16                          # whole patches (992), like the GPU leg
    heads = ovit.VIT_SIZES[size]["num_heads"]
    d = ovit.VIT_SIZES[size]["embed_dim"]
    grid = (4, T // 16) if mode == "mae" else (4, 6)
    enc = ovit.init_params(size, seed=0, use_decoder=(mode == "mae"), img_size=(64, T) if mode == "mae" else (64, 96))
    sd = {"backbone.encoder.encoder." + k: v for k, v in enc.items()}
    g = torch.Generator().manual_seed(1)
    sd["head.projector.0.weight"] = torch.randn(8192, d, generator=g) * 0.02
    sd["head.projector.1.weight"], sd["head.projector.1.bias"] = torch.ones(8192), torch.zeros(8192)
    sd["head.projector.1.running_mean"], sd["head.projector.1.running_var"] = torch.zeros(8192), torch.ones(8192)
    sd["head.projector.1.num_batches_tracked"] = torch.zeros((), dtype=torch.long)
    sd["head.projector.3.weight"] = torch.randn(256, 8192, generator=g) * 0.02
    target = {k: v.clone() for k, v in sd.items()} if mode == "byol" else None
    pred = None
    if mode == "byol":
        pred = {"predictor.0.weight": torch.randn(256, 256, generator=g) * 0.05, "predictor.1.weight": torch.ones(256),
                "predictor.1.bias": torch.zeros(256), "predictor.1.running_mean": torch.zeros(256), "predictor.1.running_var": torch.ones(256),
                "predictor.1.num_batches_tracked": torch.zeros((), dtype=torch.long), "predictor.3.weight": torch.randn(256, 256, generator=g) * 0.05}
    opt = ostep.AdamW(1e-4, 0.06)
    all_waves = synthetic_waveforms(budget_clips, n_samples).numpy()
    tfm = oaug.PairTransformOracle(crop_frames=T, seed=0)

    def one_step(n_clips=budget_clips):
        waves = all_waves[:n_clips]
        lms = ofe.crop_pad_normalize(ofe.logmel(waves, dtype=np.float32), T, 0, -0.8294, 4.6230)
        v = [[], []]
        for b in range(n_clips):
            c = tfm(lms[b][None])
            v[0].append(c[0]); v[1].append(c[1])
        views = [torch.from_numpy(np.stack(x)).float() for x in v]
        if mode == "byol":
            return ostep.bt_byol_step(sd, target, pred, views, heads, grid, opt, True, True)[0]
        if mode == "mae":
            return ostep.mae_step(sd, views, heads, grid, opt, noise=torch.rand(n_clips, grid[0] * grid[1], generator=g), mask_ratio=0.75)[0]
        return ostep.bt_step(sd, views, heads, grid, opt)[0]

    t0 = time.time()
    one_step(2)                                   # warm-up on 2 clips (also sizes the sample: about 15 s of CPU work)
    warm = (time.time() - t0) * budget_clips / 2
    print(f"[bench] cpu baseline warm-up: ~{warm:.1f}s per {budget_clips}-clip step on {cores} threads ({avail} cores visible)",
          file=sys.stderr, flush=True)
    steps = max(1, min(steps, int(15.0 / max(warm, 1e-3))))   # about 15 s of CPU work, never more than `steps` steps
    t0 = time.time()
    for _ in range(steps):
        one_step()
    dt = time.time() - t0
    return {"value": budget_clips * steps / dt, "unit": "clips/s", "cores": cores, "kind": "port",
            "sample": f"{budget_clips} clips x {steps} step(s) of the '{mode}' step after a 2-clip warm-up, {model_type}, {seconds:g} s clips, fp32 torch CPU, "
                      f"{torch.get_num_threads()} threads of {avail} visible cores (oracle/: frontend + augment + fwd/bwd + AdamW)"}


DUMP_MAX_ELEMENTS = 3 << 20      # per array: 12 MiB of float32, at most 4 arrays + the loss; a larger state is dumped as a fixed, seeded sample


def dump_outputs(trainer, loss, out_dir, max_elements=DUMP_MAX_ELEMENTS):
    """--dump-outputs: what a caller of trainer.step holds after the last timed step, as float32 .npy files under out_dir: the step's
    loss and the state the step updated -- the online network (parameters and BatchNorm buffers), the predictor and the EMA target
    (byol), the loss's BatchNorm buffers.  A module's floating-point state_dict entries are flattened in key order (the reference's
    key names, independent of the flat-buffer layout) and concatenated; past max_elements a sample at sorted indices drawn from a
    generator seeded 0 stands in for the whole, so two builds run with the same arguments are compared element for element."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"loss": loss.detach().float().reshape(()).cpu().numpy()}
    for name, module in (("online_state", trainer.online), ("predictor_state", trainer.predictor), ("target_state", trainer.target),
                         ("criterion_state", trainer.criterion)):
        if module is None:
            continue
        vals = [v.detach().reshape(-1).float() for v in module.state_dict().values() if v.is_floating_point()]
        flat = torch.cat(vals)
        if flat.numel() > max_elements:
            idx = np.sort(np.random.default_rng(0).choice(flat.numel(), max_elements, replace=False))
            flat = flat[torch.from_numpy(idx).to(flat.device)]
        arrays[name] = flat.cpu().numpy()
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return {name: a.shape for name, a in arrays.items()}


def profiler_in_environment():
    """The marker of a rocprofiler tool library injected into this process (rocprofv3 sets these for the program it starts), or None."""
    for k in ("ROCP_TOOL_LIBRARIES", "ROCPROFILER_REGISTER_FORCE_LOAD", "ROCPROF_OUTPUT_PATH", "ROCPROF_OUTPUT_FILE_NAME"):
        if os.environ.get(k):
            return f"{k} is set"
    for k in os.environ:
        if k.startswith("ROCPROFILER_") or k.startswith("ROCPROF_"):
            return f"{k} is set"
    if "rocprofiler" in os.environ.get("LD_PRELOAD", ""):
        return "LD_PRELOAD holds a rocprofiler library"
    return None


def self_launch(args):
    """`python bench.py --gpus N` with N > 1 and no launcher environment: start the N ranks as a CHILD process (never a re-exec), the
    way the reference is launched -- one process per GPU from torchrun's environment (utils/utils.py:335-361).  Nothing in THIS code has
    touched the GPU at that point (no torch.cuda call, no ops.lib()); a profiler that injected itself into the process has, which is
    why a profiled parent refuses (profiler_in_environment).  The child's stdout (rank 0's single JSON line) and stderr pass through."""
    import socket
    import subprocess
    prof = profiler_in_environment()
    if prof and not args.dry_launch:
        # Under rocprofv3 the profiler's preloaded library has ALREADY initialised the GPU in this process (always so with --pmc), so
        # starting the ranks from here is the fork + exec out of a GPU-initialised process that takes this pool's machines down.
        print(f"[bench] refusing to self-launch {args.gpus} ranks from a profiled process ({prof}): profile one rank per profiler "
              "(`torch.distributed.run ... rocprofv3 ... -- python3 bench.py` is NOT that either) or profile `--gpus 1`", file=sys.stderr, flush=True)
        return 3
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    argv = [a for a in sys.argv[1:] if a != "--dry_launch"]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + argv
    if args.dry_launch:
        print(json.dumps({"launch": cmd}), flush=True)
        return 0
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")              # dmabuf IPC: RCCL across processes needs it on this driver
    env.setdefault("OMP_NUM_THREADS", "8")
    env["SA_BENCH_PARENT"] = str(os.getpid())
    print(f"[bench] --gpus {args.gpus} without a launcher: starting {' '.join(cmd)}", file=sys.stderr, flush=True)
    return subprocess.run(cmd, env=env).returncode


def launcher_name():
    if os.environ.get("TORCHELASTIC_RUN_ID") is not None and os.environ.get("SA_BENCH_PARENT"):
        return "torch.distributed.run (self-launched child)"
    return "torch.distributed.run" if "RANK" in os.environ else "single process"


def dry_run(args):
    """The launch path of a real run without its GPU work: process group from the launcher's environment (dist.init_from_env, the same
    call), world-size check, one MAX all-reduce like the one that closes the timed region, rank 0 prints the launch fields.  No value."""
    from ssl_audio_amd import dist as sdist
    hsa_before = os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY")         # (dist's import has already set it when it was unset)
    rank, local, world = sdist.init_from_env(None if os.environ.get("SA_DIST_BACKEND") else "gloo")
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus}")
    t = torch.tensor([float(rank + 1)], dtype=torch.float64)
    if world > 1:
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        torch.distributed.barrier()
    if rank == 0:
        print(json.dumps({"metric": "clips/sec (10 s, 64-mel, ViT-B, BT loss) at 1/2/4/8 MI355X + CPU ref", "value": None, "dry_run": True,
                          "n_gpus": world, "config": {"workload": args.workload, "parallelism": f"dp{world}", "dist_world": sdist.get_world_size(),
                                                      "dist_backend": torch.distributed.get_backend() if sdist.is_dist_avail_and_initialized() else None,
                                                      "launcher": launcher_name(), "max_rank_plus_1": float(t),
                                                      "grad_dtype": args.grad_dtype or os.environ.get("SA_GRAD_DTYPE", "fp32"),
                                                      "env": {"HSA_ENABLE_IPC_MODE_LEGACY": hsa_before, "LOCAL_RANK": os.environ.get("LOCAL_RANK"),
                                                              "MASTER_ADDR": os.environ.get("MASTER_ADDR")}}}), flush=True)
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10, help="timed steps (at least 1)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="vit_base_bt_10s", choices=sorted(WORKLOADS))
    ap.add_argument("--batch_per_gpu", type=int, default=None)
    ap.add_argument("--global_batch", type=int, default=None, help="STRONG scaling: this many clips in all, split over the ranks "
                    "(BASELINE config 3's 1024); default is weak scaling at the workload's clips per GPU")
    ap.add_argument("--dispatch", default="auto", choices=["auto", "direct", "torch_ops"], help="torch_ops: every kernel call of the step goes "
                    "through torch.ops.ssl_audio.* (torch.library custom operators) instead of the direct ctypes call -- same kernels, same "
                    "bits, ~3 us more host time per launch.  Measured (DESIGN.md section 6): free where the step is GPU-bound (ViT-B 41.10 vs "
                    "41.10 ms), +12 %% where ~480 launches share 16 ms (ViT-T 16.1 -> 18.1 ms).  auto = torch_ops for the ViT-B / ViT-L "
                    "workloads, direct for ViT-T")
    ap.add_argument("--dry_launch", action="store_true", help="print the child launcher command of the self-launch path and exit")
    ap.add_argument("--no_cpu_baseline", action="store_true")
    ap.add_argument("--graph", action="store_true", help="replay the device part of the step as ONE HIP graph (BarlowTwinsTrainer.enable_graph); "
                    "default eager: measured on MI355X / ROCm 7.2 the replay of the ~600-node graph is 1-2 % SLOWER than the eager launches, "
                    "which already keep the GPU saturated (42.7 vs 43.3 ms per step)")
    ap.add_argument("--no_graph", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--profile_steps", type=int, default=3, help="eager steps with per-launch HIP events after the timed region (roofline)")
    ap.add_argument("--grad_dtype", default=None, choices=["fp32", "bf16"], help="what the gradient all-reduce carries (train.GradSync): fp32 "
                    "(default) or bf16 staging buckets at half the bytes, accumulated back into the fp32 gradients")
    ap.add_argument("--dry_run", action="store_true", help="rendezvous only: initialise the process group exactly as a real run does, "
                    "exchange one tensor, print the launch / environment fields of the JSON line with value null -- no GPU is touched "
                    "(CPU rehearsal of the N > 1 launch: SA_DIST_BACKEND=gloo)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the last one computed (loss, "
                    "updated model state; seeded samples of large states) as DIR/<name>.npy, float32 (dump_outputs)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if "RANK" not in os.environ and (args.gpus > 1 or args.dry_launch or os.environ.get("SA_BENCH_SELF_LAUNCH") == "1"):
        sys.exit(self_launch(args))
    if args.dry_run:
        sys.exit(dry_run(args))

    # stdout carries exactly ONE line (the JSON): RCCL prints a version banner to fd 1 when its first communicator comes up, so
    # the process-level stdout is parked on stderr until the result is ready
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    from ssl_audio_amd import dist as sdist, hyperparameters as hp, ops
    from ssl_audio_amd.selfcheck import synthetic_waveforms
    from ssl_audio_amd.train import BarlowTwinsTrainer

    t_start = time.perf_counter()
    rank, local, world = sdist.init_from_env("nccl")
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus}")
    local = local % max(torch.cuda.device_count(), 1)              # (lets several gloo ranks rehearse on a 1-GPU box)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    ops.lib()                                                      # fail loudly if the HIP library is missing
    if args.dispatch == "torch_ops" or (args.dispatch == "auto" and "tiny" not in WORKLOADS[args.workload][0]):
        ops.route_through_dispatcher(True)
    dist_backend = torch.distributed.get_backend() if sdist.is_dist_avail_and_initialized() else None
    try:
        rccl_version = ".".join(str(v) for v in torch.cuda.nccl.version())      # RCCL's version (backend "nccl" IS RCCL on ROCm)
    except Exception:  # noqa: BLE001
        rccl_version = None

    model_type, seconds, bpg, mode = WORKLOADS[args.workload]
    B = args.batch_per_gpu or bpg
    if args.global_batch:
        if args.global_batch % world:
            raise SystemExit(f"--global_batch {args.global_batch} does not divide over {world} ranks")
        B = args.global_batch // world
    n_samples = int(seconds * 16000)
    extra = dict(masked_recon=True, mask=True, mask_ratio=0.75) if mode == "mae" else {}
    frames = (n_samples // 160 + 1) // 16 * 16 if mode == "mae" else n_samples // 160 + 1      # MAE: whole patches (992)
    cfg = hp.make_args(model_type=model_type, batch_size=B * world, crop_frames=frames, dataset="audioset",
                       stop_gradient=(mode == "byol"), predictor=(mode == "byol"), **extra)
    trainer = BarlowTwinsTrainer(cfg, dev, mode=mode, batch_per_rank=B, clip_samples=n_samples, seed=0, grad_dtype=args.grad_dtype)

    # synthetic waveforms resident in HBM: 2 alternating batches, distinct per rank (cheap device-side recipe of the
    # same family as BASELINE.md §3: noise + 3 sinusoids)
    g = torch.Generator(device=dev).manual_seed(1234 + rank)
    t = torch.arange(n_samples, device=dev, dtype=torch.float32) / 16000.0
    pool = []
    for _ in range(2):
        w = 0.1 * torch.randn(B, n_samples, device=dev, generator=g)
        for _ in range(3):
            f = 100.0 + 6900.0 * torch.rand(B, 1, device=dev, generator=g)
            a = 0.05 + 0.45 * torch.rand(B, 1, device=dev, generator=g)
            w += a * torch.sin(2 * torch.pi * f * t)
        pool.append(w.contiguous())

    def note(msg):
        if rank == 0:
            print(f"[bench +{time.perf_counter() - t_start:7.1f}s] {msg}", file=sys.stderr, flush=True)

    def barrier():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    note(f"model + {2 * B} synthetic clips resident; warm-up x{args.warmup}")
    # (measured: vit_base 42.7 ms eager vs 43.3 ms replayed, vit_tiny 18.11 vs 18.13 -- every workload here is GPU-bound, so eager
    # is the default and --graph the option)
    use_graph = args.graph and not args.no_graph           # (round 5: the masked MAE step is capturable too: fixed mask ratio)
    for i in range(max(args.warmup, 1)):
        trainer.step(pool[i % 2])
        torch.cuda.synchronize()
        note(f"warm-up step {i} done (loss {float(trainer.last_loss):.4f})")
        if i == 0 and use_graph:
            # --graph: the device part of the step (forward, loss, backward, all-reduce, AdamW) becomes ONE HIP graph; the remaining warm-up
            # steps replay it.  A failed capture is fatal for this process (no silent eager fallback): rank 0 of a single-GPU run hands
            # over to a FRESH child process that runs eagerly (never a re-exec of a process that has touched the GPU).
            try:
                trainer.enable_graph()
                trainer.step(pool[1])                                  # first replay (untimed)
                torch.cuda.synchronize()
                note("device step captured into a HIP graph")
            except Exception as e:  # noqa: BLE001
                note(f"HIP graph capture FAILED: {e!r}")
                if world > 1:
                    raise
                import subprocess
                os.dup2(real_stdout, 1)
                child = subprocess.run([sys.executable, os.path.abspath(__file__)] + [a for a in sys.argv[1:] if a != "--graph"])
                sys.exit(child.returncode)
    barrier()
    t0 = time.perf_counter()
    for i in range(args.steps):
        loss = trainer.step(pool[i % 2])
    barrier()
    dt = time.perf_counter() - t0
    trainer.assert_finite()                                        # the step's device-side finite-loss counter, read once here
    note(f"timed region done: {args.steps} steps in {dt:.3f}s")
    loss_val = float(loss)
    if args.dump_outputs and rank == 0:
        shapes = dump_outputs(trainer, loss, args.dump_outputs)
        note(f"outputs of timed step {args.steps} written to {args.dump_outputs}: {shapes}")
    # roofline pass, OUTSIDE the timed region: a few eager steps of the same workload with HIP events (on the launch stream) around every
    # GEMM launch and around the HBM-bound frontend / augmentation / LayerNorm / AdamW launches
    psteps = max(args.profile_steps, 1)
    trainer.use_graph = False
    trainer.step(pool[0])                                          # (re-warms the eager allocator paths)
    barrier()
    ops.GEMM_PROFILE = []
    ops.STREAM_PROFILE = {}
    tp0 = time.perf_counter()
    for i in range(psteps):
        trainer.step(pool[i % 2])
    barrier()
    dtp = time.perf_counter() - tp0
    prof, ops.GEMM_PROFILE = ops.GEMM_PROFILE, None
    sprof, ops.STREAM_PROFILE = ops.STREAM_PROFILE, None
    trainer.use_graph = True
    note(f"profiled pass done: {psteps} eager steps in {dtp:.3f}s")
    tmax = torch.tensor([dt], device=dev, dtype=torch.float64)
    if world > 1:
        torch.distributed.all_reduce(tmax, op=torch.distributed.ReduceOp.MAX)
    dt = float(tmax)

    if rank == 0:
        clips_per_s = B * world * args.steps / dt
        gemm_ms = sum(e0.elapsed_time(e1) for e0, e1, *_ in prof)
        gemm_flop = sum(fl for _, _, fl, *_ in prof)
        n_launch = max(len(prof), 1)
        achieved = gemm_flop / (gemm_ms * 1e-3) / 1e12 if gemm_ms > 0 else 0.0
        by_kind, by_kernel, by_symbol = {}, {}, {}
        for e0, e1, fl, kind, nb, kname, symbol in prof:
            t = e0.elapsed_time(e1)
            ms, f = by_kind.get(kind, (0.0, 0.0))
            by_kind[kind] = (ms + t, f + fl)
            for table, key in ((by_kernel, kname), (by_symbol, symbol)):
                k = table.setdefault(key, [0.0, 0.0, 0.0, 0])
                k[0] += t; k[1] += fl; k[2] += nb; k[3] += 1
        # `dom` below groups launches by kernel FUNCTION (all template instances of one __global__); rocprofv3 lists every instance as its own
        # symbol, and by that grouping another kernel may lead (the split-K weight gradient): name it beside the family
        top_sym = max(by_symbol, key=lambda k: by_symbol[k][0])
        s_ms, s_fl, s_nb, s_n = by_symbol[top_sym]
        # the DOMINANT device kernel (most time in the timed region) carries the roofline object; names match rocprofv3's
        dom = max(by_kernel, key=lambda k: by_kernel[k][0])
        d_ms, d_fl, d_nb, d_n = by_kernel[dom]
        d_tflops = d_fl / (d_ms * 1e-3) / 1e12
        traffic, traffic_note = None, "no PMC summary for this workload"
        import glob
        tfiles = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_gemm_traffic.json")))
        tpath = tfiles[-1] if tfiles else ""                        # the newest round's PMC summary
        if os.path.exists(tpath) and B == bpg:
            # HBM bytes per launch of that kernel from rocprofv3 PMC passes of this same command (scripts/profile_round.sh), per
            # workload, valid only for the kernel sources it was collected with
            tj = json.load(open(tpath))
            if tj.get("source_sha") != source_sha():
                traffic_note = f"profiles/{os.path.basename(tpath)} is stale (kernel sources changed since it was collected): ignored"
            elif args.workload in tj.get("workloads", {}):
                traffic = tj["workloads"][args.workload].get("per_kernel", {}).get(dom, {}).get("hbm_bytes_per_launch")
                traffic_note = f"rocprofv3 PMC (FETCH_SIZE x 2 + WRITE_SIZE, separate passes) of this command, profiles/{os.path.basename(tpath)}"
        n_tok = (64 // 16) * (frames // 16) + 1
        exec_gf = executed_gflop_per_clip(model_type, mode, n_tok)
        hbm_kernels = {}
        for kname, recs in (sprof or {}).items():
            ms = sum(r[0].elapsed_time(r[1]) for r in recs)
            nb = sum(r[2] for r in recs)
            fl = sum(r[3] for r in recs)
            mfl = sum(r[4] for r in recs)
            if ms > 0:
                gbs = nb / (ms * 1e-3) / 1e9
                hbm_kernels[kname] = {"bound": "hbm", "achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(gbs / PEAK_HBM_GBS, 4),
                                      "launches": len(recs), "avg_launch_us": round(ms * 1e3 / len(recs), 2),
                                      "algorithmic_bytes_per_launch": round(nb / len(recs)), "share_of_step": round((ms / psteps) / (dt / args.steps * 1e3), 4)}
                if mfl > 0:    # the attention kernels: bf16 MFMA work next to their bytes (they sit under BOTH roofs: DESIGN.md section 6)
                    tf = mfl / (ms * 1e-3) / 1e12
                    hbm_kernels[kname]["mfma"] = {"achieved": round(tf, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": round(tf / PEAK_BF16_TFLOPS, 4),
                                                  "algorithmic_flop_per_launch": round(mfl / len(recs))}
                if fl > 0:     # arithmetic outweighs bytes (the FFT frontend: 87 flop per byte): the fp32 vector rate is the nearer bound
                    tf = fl / (ms * 1e-3) / 1e12
                    hbm_kernels[kname]["nearer_bound"] = {"bound": "valu_f32", "achieved": round(tf, 2), "peak": PEAK_F32_VALU_TFLOPS, "unit": "TFLOP/s",
                                                          "frac": round(tf / PEAK_F32_VALU_TFLOPS, 4), "algorithmic_flop_per_launch": round(fl / len(recs))}
        line = {
            "metric": "clips/sec (10 s, 64-mel, ViT-B, BT loss) at 1/2/4/8 MI355X + CPU ref",
            "value": round(clips_per_s, 2), "unit": "clips/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(dt / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "strong" if args.global_batch else "weak", "vs_baseline": None,
            "dtype": "bf16", "data": "synthetic",
            "config": {"workload": args.workload, "encoder": model_type, "clip_seconds": seconds, "n_mels": 64,
                       "clips_per_gpu": B, "global_batch": B * world, "step": "logmel+augment+fwd+bwd+allreduce+adamw" +
                       ("+ema" if mode == "byol" else ""), "hip_graph": trainer._graph is not None, "dispatch": ops.DISPATCH,
                       "profiled_ms_per_step": round(dtp / psteps * 1e3, 3), "parallelism": f"dp{world}", "gflop_per_clip": GF_PER_CLIP[args.workload],
                       "loss": round(loss_val, 4),
                       "dist_world": sdist.get_world_size(), "dist_backend": dist_backend, "rccl_version": rccl_version,
                       "launcher": launcher_name(), "grad_dtype": trainer.sync.grad_dtype,
                       "env": {"HSA_ENABLE_IPC_MODE_LEGACY": os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY")}},
            # which bound applies: the kernel's arithmetic intensity against the ridge (2 500 TFLOP/s / 8 TB/s = 312 flop/B).  ViT-B's GEMMs sit
            # above it (MFMA-bound); ViT-T's (d = 192: three K-tiles per output tile, weight gradients that read 245 MB for 38 GFLOP)
            # far below, so their roofline is HBM and `frac` is the fraction of 8 TB/s the algorithmic bytes move at
            "roofline": ({"bound": "mfma", "achieved": round(d_tflops, 2), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                          "frac": round(d_tflops / PEAK_BF16_TFLOPS, 4)} if d_fl / max(d_nb, 1.0) >= PEAK_BF16_TFLOPS * 1e3 / PEAK_HBM_GBS else
                         {"bound": "hbm", "achieved": round(d_nb / (d_ms * 1e-3) / 1e9, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                          "frac": round(d_nb / (d_ms * 1e-3) / 1e9 / PEAK_HBM_GBS, 4)}) | {
                         "kernel": dom + " (bf16 MFMA 16x16x32, sa_gemm_bf16; all template instances of the function)",
                         "largest_single_symbol": {"kernel": top_sym, "launches": s_n, "avg_launch_us": round(s_ms * 1e3 / s_n, 2),
                                                   "tflops": round(s_fl / (s_ms * 1e-3) / 1e12, 1), "frac": round(s_fl / (s_ms * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4),
                                                   "hbm_gbs_algorithmic": round(s_nb / (s_ms * 1e-3) / 1e9, 1),
                                                   "share_of_step": round((s_ms / psteps) / (dt / args.steps * 1e3), 4)},
                         "intensity_flop_per_byte": round(d_fl / max(d_nb, 1.0), 1), "ridge_flop_per_byte": round(PEAK_BF16_TFLOPS * 1e3 / PEAK_HBM_GBS, 1),
                         "mfma": {"achieved": round(d_tflops, 2), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": round(d_tflops / PEAK_BF16_TFLOPS, 4)},
                         "hbm": {"achieved": round(d_nb / (d_ms * 1e-3) / 1e9, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                                 "frac": round(d_nb / (d_ms * 1e-3) / 1e9 / PEAK_HBM_GBS, 4),
                                 "pmc_achieved": round(traffic / (d_ms / d_n * 1e-3) / 1e9, 1) if traffic else None},
                         "traffic": traffic, "traffic_unit": "HBM bytes per launch (PMC)", "traffic_note": traffic_note,
                         "algorithmic_flop_per_launch": round(d_fl / d_n), "algorithmic_bytes_per_launch": round(d_nb / d_n),
                         "launches": d_n, "avg_launch_us": round(d_ms * 1e3 / d_n, 2),
                         "share_of_step": round((d_ms / psteps) / (dt / args.steps * 1e3), 4),
                         "timing": f"HIP events on the launch stream around every sa_gemm_bf16 launch of {psteps} steps of the same workload run right "
                                   "after the timed region (the timed region itself carries no events: 2 x 160 of them per step cost 5 % of it)",
                         "all_gemm": {"achieved": round(achieved, 2), "frac": round(achieved / PEAK_BF16_TFLOPS, 4), "launches": len(prof),
                                      "share_of_step": round((gemm_ms / psteps) / (dt / args.steps * 1e3), 4),
                                      "hbm_gbs_algorithmic": round(sum(v[2] for v in by_kernel.values()) / (gemm_ms * 1e-3) / 1e9, 1) if gemm_ms > 0 else None,
                                      "by_kernel": {k: {"tflops": round(v[1] / (v[0] * 1e-3) / 1e12, 1), "launches": v[3],
                                                        "avg_launch_us": round(v[0] * 1e3 / v[3], 2),
                                                        "hbm_gbs_algorithmic": round(v[2] / (v[0] * 1e-3) / 1e9, 1)} for k, v in by_kernel.items() if v[0] > 0},
                                      "by_layout_tflops": {k: round(f / (ms * 1e-3) / 1e12, 1) for k, (ms, f) in by_kind.items() if ms > 0}},
                         "hbm_kernels": hbm_kernels,
                         "whole_step_tflops_algorithmic": round(clips_per_s / world * GF_PER_CLIP[args.workload] / 1e3, 2),
                         "executed_gflop_per_clip": round(exec_gf, 1) if exec_gf else None,
                         "whole_step_tflops": round(clips_per_s / world * (exec_gf or GF_PER_CLIP[args.workload]) / 1e3, 2)},
        }
        if not args.no_cpu_baseline and world == 1:          # the CPU leg is timed at N = 1 only (rank 0 is the only rank)
            note("timing the CPU baseline (oracle on host cores) ...")
            try:
                line["cpu_baseline"] = cpu_baseline(args.workload)
                note("CPU baseline done")
            except Exception as e:  # noqa: BLE001  -- the GPU result is never lost to a failure of the CPU leg
                line["cpu_baseline"] = None
                note(f"CPU baseline FAILED: {e!r}")
        sys.stdout.flush()
        os.dup2(real_stdout, 1)
        print(json.dumps(line), flush=True)
        os.dup2(2, 1)          # anything printed from here on (RCCL's banner when its first communicator only comes up at the barrier below:
                               # one-rank runs) goes to stderr: stdout stays the ONE JSON line
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
