"""bench.py's launcher contract, CPU side: `python bench.py --gpus N` with no launcher environment starts its own
ranks as a CHILD `torch.distributed.run` (the reference is launched one process per GPU from torchrun's environment,
utils/utils.py:335-361) before anything touches a GPU, and hands the child's exit code back."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env():
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    return e


def test_dry_launch_prints_the_child_command():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "8", "--steps", "7", "--warmup", "2", "--dry_launch"], env=_env(), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    cmd = json.loads(r.stdout.strip().splitlines()[-1])["launch"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node=8" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and int(cmd[cmd.index("--master-port") + 1]) > 0
    i = cmd.index(BENCH)
    assert cmd[i + 1:] == ["--gpus", "8", "--steps", "7", "--warmup", "2"]           # the ranks get the same arguments, minus --dry_launch


def test_under_a_launcher_the_process_is_a_rank_and_world_must_match():
    """With RANK / WORLD_SIZE present nothing is spawned; a --gpus that disagrees with WORLD_SIZE is refused before any GPU call."""
    e = dict(_env(), RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29431", SA_DIST_BACKEND="gloo")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "1"], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "WORLD_SIZE=1" in (r.stderr + r.stdout)


def test_self_launch_returns_the_childs_exit_code():
    """No GPU in the build container: every rank of the self-launched child fails loudly (no CPU fallback), and the parent's exit code
    is the launcher's -- non-zero, with no JSON line on stdout."""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "1", "--warmup", "1", "--no_cpu_baseline"], env=_env(),
                       capture_output=True, text=True, timeout=600)
    import torch
    if torch.cuda.is_available():
        return                                                                       # (on a GPU box this would be a real 2-rank run)
    assert r.returncode != 0
    assert "starting" in r.stderr and "torch.distributed.run" in r.stderr
    assert not any(l.startswith("{") for l in r.stdout.splitlines())


def test_external_launcher_dry_run_two_gloo_ranks():
    """VERDICT r4 #2 iv: bench.py under an EXTERNAL `torch.distributed.run` (the driver's way of launching N > 1) with nothing prepared
    beyond torchrun's own variables: the ranks rendezvous through dist.init_from_env, which also sets HSA_ENABLE_IPC_MODE_LEGACY=0 (RCCL
    across processes needs dmabuf IPC on this driver; bench.py's own child launcher used to be the only place that set it), rank 0 prints
    one JSON line with the launch fields and no value.  gloo on CPU: no GPU is touched."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    e = {k: v for k, v in _env().items() if k != "HSA_ENABLE_IPC_MODE_LEGACY"}
    e.update(SA_DIST_BACKEND="gloo", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           BENCH, "--gpus", "2", "--steps", "3", "--warmup", "1", "--dry_run", "--grad_dtype", "bf16"]
    r = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout                                                    # rank 0 only
    j = json.loads(lines[0])
    c = j["config"]
    assert j["dry_run"] is True and j["value"] is None and j["n_gpus"] == 2
    assert c["dist_world"] == 2 and c["dist_backend"] == "gloo" and c["launcher"] == "torch.distributed.run" and c["parallelism"] == "dp2"
    assert c["max_rank_plus_1"] == 2.0                                                  # the MAX all-reduce really crossed the ranks
    assert c["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0" and c["env"]["MASTER_ADDR"] == "127.0.0.1" and c["grad_dtype"] == "bf16"


def test_a_user_value_of_the_ipc_variable_is_kept_and_world_mismatch_is_refused_in_dry_run():
    e = dict(_env(), HSA_ENABLE_IPC_MODE_LEGACY="1")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--dry_run"], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and json.loads(r.stdout.strip().splitlines()[-1])["config"]["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "1"
    e = dict(_env(), RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29433", SA_DIST_BACKEND="gloo")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dry_run"], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "WORLD_SIZE=1" in (r.stderr + r.stdout)


def test_self_launch_is_refused_from_a_profiled_process():
    """under rocprofv3 the profiler's injected library has already initialised the GPU in the parent, so starting the ranks from
    there is the forbidden fork + exec out of a GPU-initialised process: bench.py detects the profiler's environment and exits non-zero
    before spawning anything (`--dry_launch` still only prints)."""
    for marker in ({"ROCP_TOOL_LIBRARIES": "/opt/rocm/lib/rocprofiler-sdk/librocprofiler-sdk-tool.so"}, {"ROCPROFILER_SOMETHING": "1"},
                   {"LD_PRELOAD": "/opt/rocm/lib/librocprofiler-sdk-tool.so.1"}):
        e = dict(_env(), **marker)
        if "LD_PRELOAD" in marker:
            e.pop("LD_PRELOAD")                       # (a non-existent preload would only make the loader complain; the check reads the variable)
            e["ROCPROF_OUTPUT_PATH"] = "/tmp/x"
        r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "1", "--no_cpu_baseline"], env=e, capture_output=True, text=True, timeout=300)
        assert r.returncode == 3 and "refusing to self-launch" in r.stderr and "starting" not in r.stderr, (marker, r.stderr[-500:])
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dry_launch"], env=dict(_env(), ROCPROF_OUTPUT_PATH="/tmp/x"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "launch" in r.stdout


def test_steps_below_one_are_refused():
    """--steps sets the number of timed steps: zero steps time nothing and are refused before any GPU call."""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "0"], env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--steps" in r.stderr


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_writes_the_step_state_and_a_fixed_sample(tmp_path):
    """--dump-outputs on CPU stand-ins for the trainer's modules: float32 files, the whole state in state_dict key order while it fits,
    a sample at fixed sorted indices past the cap (identical from call to call), and a bound of 64 MB on everything written."""
    import numpy as np
    import torch
    from types import SimpleNamespace
    bench = _bench_module()
    torch.manual_seed(0)
    online = torch.nn.Sequential(torch.nn.Linear(32, 16), torch.nn.BatchNorm1d(16))
    crit = torch.nn.BatchNorm1d(4, affine=False)
    tr = SimpleNamespace(online=online, predictor=None, target=None, criterion=crit)
    loss = torch.tensor(1.25)
    shapes = bench.dump_outputs(tr, loss, str(tmp_path / "a"))
    assert sorted(shapes) == ["criterion_state", "loss", "online_state"]
    full = np.concatenate([v.detach().reshape(-1).float().numpy() for v in online.state_dict().values() if v.is_floating_point()])
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in shapes}
    assert all(a.dtype == np.float32 for a in got.values())
    assert got["loss"].shape == () and float(got["loss"]) == 1.25
    np.testing.assert_array_equal(got["online_state"], full)
    np.testing.assert_array_equal(got["criterion_state"], np.concatenate([np.zeros(4), np.ones(4)]).astype(np.float32))
    cap = 100
    bench.dump_outputs(tr, loss, str(tmp_path / "b"), max_elements=cap)
    bench.dump_outputs(tr, loss, str(tmp_path / "c"), max_elements=cap)
    b, c = np.load(tmp_path / "b" / "online_state.npy"), np.load(tmp_path / "c" / "online_state.npy")
    idx = np.sort(np.random.default_rng(0).choice(full.size, cap, replace=False))
    np.testing.assert_array_equal(b, full[idx])
    np.testing.assert_array_equal(b, c)
    assert 4 * bench.DUMP_MAX_ELEMENTS * 4 + 4 <= 64 << 20           # at most four sampled states and the loss, float32
