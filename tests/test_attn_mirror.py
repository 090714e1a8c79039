"""CPU checks of the attention rounding mirror (tests/attn_mirror.py) that tests/test_attention_gpu.py compares the kernels with:
with its roundings off it is fp64 softmax attention and its autograd gradients, with them on it stays inside the norm bounds
tests/test_kernels_gpu.py::test_attention_fwd_bwd holds the kernels to."""
import pytest
import torch

import attn_mirror as am


def _inputs(S, H, N, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(S * N, 3 * 64 * H, generator=g, dtype=torch.float64) * 1.4).to(torch.bfloat16)
    dout = torch.randn(S * N, 64 * H, generator=g, dtype=torch.float64).to(torch.bfloat16)
    return qkv, dout


def _autograd(q, k, v, dout, scale, nq):
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    s = (q[..., :nq, :] @ k.transpose(-1, -2)) * scale
    out = s.softmax(-1) @ v
    out.backward(dout[..., :nq, :])
    return out.detach(), torch.logsumexp(s, -1).detach(), q.grad, k.grad, v.grad


def _pad(x, N):
    return torch.cat([x, x.new_zeros(x.shape[:-2] + (N - x.shape[-2],) + x.shape[-1:])], -2)


@pytest.mark.parametrize("S,H,N,nq,scale", [(2, 2, 37, 37, 0.125), (3, 1, 40, 17, 0.125), (2, 3, 16, 1, 0.2)])
def test_mirror_without_rounding_is_fp64_attention(S, H, N, nq, scale):
    qkv, dout = _inputs(S, H, N, 5)
    q, k, v = am.split_heads(qkv, H, N)
    do = am.split_rows(dout, H, N)
    out, lse, gq, gk, gv = _autograd(q, k, v, do, scale, nq)
    f = am.forward(q, k, v, scale, n_query=nq, rounding=False)
    b = am.backward(q, k, v, _pad(out, N), do, _pad(lse[..., None], N)[..., 0], scale, n_query=nq, rounding=False)
    for name, got, ref in [("out", f["out"], out), ("lse", f["lse"], lse), ("dq", b["dq"], gq), ("dk", b["dk"], gk), ("dv", b["dv"], gv)]:
        err = float((got - ref).abs().max()) / max(1.0, float(ref.abs().max()))
        assert err <= 1e-12, (name, err)


@pytest.mark.parametrize("S,H,N,nq", [(2, 2, 249, 249), (1, 2, 501, 501), (3, 1, 40, 17)])
def test_mirror_with_rounding_stays_inside_the_fp64_norm_bounds(S, H, N, nq):
    qkv, dout = _inputs(S, H, N, 6)
    q, k, v = am.split_heads(qkv, H, N)
    do = am.split_rows(dout, H, N)
    out, lse, gq, gk, gv = _autograd(q, k, v, do, 0.125, nq)
    f = am.forward(q, k, v, 0.125, n_query=nq)
    b = am.backward(q, k, v, _pad(f["out"], N), do, am.f32(_pad(f["lse"][..., None], N)[..., 0]), 0.125, n_query=nq)

    def rel(a, r):
        return float((a - r).norm() / r.norm())

    assert torch.equal(f["out"], am.bf16(f["out"])) and torch.equal(b["dq"], am.bf16(b["dq"]))      # the results are bf16 values
    assert rel(f["out"], out) < 1e-2 and float((f["lse"] - lse).abs().max()) < 2e-2
    for name in ("dq", "dk", "dv"):
        assert rel(b[name], {"dq": gq, "dk": gk, "dv": gv}[name]) < 2e-2, name
    assert rel(f["out"], out) > 1e-4 and rel(b["dk"], gk) > 1e-4                # the roundings are real: not secretly exact


def test_round_spread_is_zero_away_from_a_rounding_boundary():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.0], dtype=torch.float64)
    e = torch.full_like(x, 2.0 ** -18)
    assert am.round_spread(x, e).tolist() == [0.0, 2.0 ** -7, 2.0 ** -7, 0.0]
    assert am.ulp_bf16(torch.tensor([1.0, 1.99, 2.0, 0.0], dtype=torch.float64)).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -133]
