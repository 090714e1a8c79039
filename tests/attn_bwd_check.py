"""Child process of tests/test_attention_gpu.py::test_persistent_backward_is_bit_identical: one attention forward + backward per shape on
seeded inputs, printing a digest of dqkv.  The library reads SA_ATTN_BWD_PERSIST once per process, so each setting runs in its own."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from ssl_audio_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
# more (sequence, head) units than the persistent grid's workgroups (two per CU at N <= 256, one above): a workgroup walks several
for S, H, N in [(64, 12, 249), (32, 12, 501), (48, 12, 100)]:
    g = torch.Generator(device=dev).manual_seed(N)
    C = 64 * H
    qkv = (torch.randn(S * N, 3 * C, device=dev, generator=g) * 1.4).to(torch.bfloat16)
    dout = torch.randn(S * N, C, device=dev, generator=g).to(torch.bfloat16)
    out = torch.empty(S * N, C, device=dev, dtype=torch.bfloat16)
    lse = torch.empty(S * H, N, device=dev)
    dqkv = torch.full((S * N, 3 * C), float("nan"), device=dev, dtype=torch.bfloat16)
    ops.attention_fwd(qkv, H, N, 0.125, out, lse)
    ops.attention_bwd(qkv, H, N, 0.125, out, dout, lse, dqkv)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dqkv.float()).all()), (S, H, N)
    print(f"dqkv {S}x{H}x{N} {hashlib.sha256(dqkv.cpu().view(torch.int16).numpy().tobytes()).hexdigest()}")
