"""Rounding mirror of the fused attention kernels (ssl_audio_amd/csrc/attention.hip), in fp64 PyTorch.

The mirror restates the kernels' arithmetic and rounds to bf16 (RNE, like `torch.Tensor.to(torch.bfloat16)`) at exactly the points where
the kernels round; everything else is carried in fp64.  With `rounding=False` every rounding is switched off and the mirror is plain
softmax attention and its gradients (tests/test_attn_mirror.py checks both).  Next to each result it derives a per-element bound on
|kernel - mirror| from its own magnitudes, so that a GPU test can compare every element instead of a norm:

  * the kernels' fp32 accumulations: a chain of n fp32 additions is off by at most n * 2^-24 * (sum of the magnitudes it adds);
  * the bf16 roundings of intermediates (bf16(p), dS): the kernel and the mirror round slightly different values, and where the two
    straddle a rounding boundary the kernel's intermediate is one bf16 ulp away from the mirror's.  That can only happen where the value
    lies within its own fp32-level error of a boundary; the bound charges bf16(x + e) - bf16(x - e) per intermediate, which is zero
    everywhere else, so a mask or coverage bug cannot hide inside a blanket 2^-8 * sum |p| |v| allowance;
  * one bf16 rounding of the result: one bf16 ulp of |m| (2^-8 .. 2^-7 of |m|).
`lse` is fp32 and gets an fp32-level bound.

The kernels' rounding points (attention.hip):
  forward   s = q.k (fp32 sums of exact bf16 products); p = exp2(c2 s - fp32(c2 max_s)), c2 = fp32(scale log2 e); the denominator sums the
            unrounded p; the P.V operand is bf16(p); out = bf16((bf16(p).V) / sum p); lse = scale max_s + log(sum p).
  backward  pass A (dQ) prescales Q: bf16(fp32(q c2)); pass B (dK, dV) prescales K: bf16(fp32(k c2)) -- the two passes see slightly
            different P.  Both start the score chain from -fp32(lse * fp32(log2 e)); delta = rowsum(dO * O) over the stored bf16 O;
            dS = bf16(p (dP - delta)); dQ = bf16(scale dS.K); dK = bf16(scale dS^T.Q); dV = bf16(bf16(p)^T.dO).  Queries >= n_query
            contribute nothing (p = 0).

Plain torch: imports without a GPU, runs on whatever device its inputs live on; never imported by the package.
"""
import math

import torch

LOG2E = math.log2(math.e)
LN2 = math.log(2.0)
U = 2.0 ** -24          # fp32 unit roundoff
SAFE = 2.0              # margin on every fp32-level error estimate (the hardware's exp2 and MFMA summation are not specified to the ulp)
FLOOR = 2.0 ** -120     # absolute floor: fp32 flush-to-zero of denormal intermediates


def bf16(x):
    return x.to(torch.bfloat16).to(x.dtype)


def f32(x):
    return x.to(torch.float32).to(x.dtype)


def ulp_bf16(x):
    """One bf16 ulp at |x| (the spacing of bf16 values around x)."""
    _, e = torch.frexp(x.abs())                 # |x| = m 2^e, m in [0.5, 1): ulp = 2^(e - 1 - 7); frexp(0) has e = 0
    return torch.ldexp(torch.ones_like(x), torch.where(x == 0, -133, torch.clamp(e - 8, min=-133)))


def round_spread(x, e):
    """Largest |bf16(y) - bf16(x)| over |y - x| <= e: zero unless x lies within e of a bf16 rounding boundary."""
    return bf16(x + e) - bf16(x - e)


def result_bound(m, e):
    """|kernel - mirror| of a bf16 result whose pre-rounding values differ by at most e: e plus one ulp of the result."""
    return e + ulp_bf16(m.abs() + e) + FLOOR


def split_heads(qkv, H, N):
    """[S*N, >=3C] packed rows -> q, k, v as [S, H, N, 64] fp64."""
    rows = qkv.shape[0]
    C = 64 * H
    x = qkv[:, :3 * C].double().reshape(rows // N, N, 3, H, 64)
    return x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2), x[:, :, 2].transpose(1, 2)


def split_rows(x, H, N):
    """[S*N, >=C] rows -> [S, H, N, 64] fp64."""
    rows = x.shape[0]
    return x[:, :64 * H].double().reshape(rows // N, N, H, 64).transpose(1, 2)


def forward(q, k, v, scale, n_query=None, rounding=True):
    """q, k, v: [..., N, 64] fp64 (bf16 values).  Returns dict(out [..., nq, 64], lse [..., nq], out_bound, lse_bound)."""
    N = k.shape[-2]
    nq = N if not n_query else min(int(n_query), N)
    q = q[..., :nq, :]
    r = rounding
    c2 = f32(torch.tensor(scale * LOG2E, dtype=torch.float64)).item() if r else scale * LOG2E
    s = q @ k.transpose(-1, -2)
    mx = s.amax(-1, keepdim=True)
    mb = f32(mx * c2) if r else mx * c2
    arg = s * c2 - mb
    p = torch.exp2(arg)
    den = p.sum(-1, keepdim=True)
    pb = bf16(p) if r else p
    x = (pb @ v) / den
    out = bf16(x) if r else x
    lse = (scale * mx + torch.log(den)).squeeze(-1)

    # bounds: relative error of each p from the fp32 score chain (64 products), the shared max, the exp2 argument and v_exp itself
    es = 64 * U * (q.abs() @ k.abs().transpose(-1, -2))
    es_max = es.amax(-1, keepdim=True)
    ep = SAFE * p * (scale * (es + es_max) + LN2 * U * (arg.abs() + mb.abs()) + 4 * U)
    dpb = round_spread(p, ep)
    av = v.abs()
    e_num = dpb @ av + N * U * (pb @ av)
    rel_den = ep.sum(-1, keepdim=True) / den + N * U
    e_x = e_num / den + x.abs() * rel_den + 2 * U * x.abs()
    out_bound = result_bound(out, e_x)
    lse_bound = (scale * es_max + rel_den).squeeze(-1) + 1e-6 * (1 + lse.abs())
    return dict(out=out, lse=lse, out_bound=out_bound, lse_bound=lse_bound)


def backward(q, k, v, o, dout, lse, scale, n_query=None, rounding=True):
    """Gradients of the kernels' backward, given the forward's stored o (bf16 values) and lse (fp32 values), all [..., N, *] fp64.
    Rows >= n_query of o, dout and lse are never used.  Returns dict(dq, dk, dv and their *_bound), each [..., N, 64]."""
    N = k.shape[-2]
    nq = N if not n_query else min(int(n_query), N)
    r = rounding
    l2 = f32(torch.tensor(LOG2E, dtype=torch.float64)).item() if r else LOG2E
    c2 = f32(torch.tensor(scale * LOG2E, dtype=torch.float64)).item() if r else scale * LOG2E
    live = torch.arange(N, device=q.device) < nq
    zq = torch.zeros((), dtype=q.dtype, device=q.device)
    o = torch.where(live[:, None], o, zq)
    dout = torch.where(live[:, None], dout, zq)
    lse = torch.where(live, lse, zq)
    nl = -(f32(lse * l2) if r else lse * l2)                      # -lse in log2 units: the initial accumulator of both score chains
    delta = (dout * o).sum(-1)
    D = dout @ v.transpose(-1, -2) - delta[..., None]             # dP - delta, [.., query, key]
    lmask = live[:, None].to(q.dtype)

    # pass A: dQ (prescaled Q)
    qa = bf16(f32(q * c2)) if r else q * c2
    sA = qa @ k.transpose(-1, -2) + nl[..., None]
    pA = torch.exp2(sA) * lmask
    xA = f32(pA * D) if r else pA * D
    dSA = bf16(xA) if r else xA
    gq = (dSA @ k) * scale
    dq = bf16(f32(gq)) if r else gq

    # pass B: dK, dV (prescaled K)
    kb = bf16(f32(k * c2)) if r else k * c2
    sB = q @ kb.transpose(-1, -2) + nl[..., None]
    pB = torch.exp2(sB) * lmask
    xB = f32(pB * D) if r else pB * D
    dSB = bf16(xB) if r else xB
    pBb = bf16(pB) if r else pB
    gk = (dSB.transpose(-1, -2) @ q) * scale
    dk = bf16(f32(gk)) if r else gk
    gv = pBb.transpose(-1, -2) @ dout
    dv = bf16(gv) if r else gv

    # bounds.  dP - delta: a 64-product fp32 chain started at -delta, delta itself a 64-term fp32 sum
    adO = dout.abs()
    ad = (adO * o.abs()).sum(-1)
    e_D = 65 * U * (adO @ v.abs().transpose(-1, -2) + ad[..., None]) + 64 * U * ad[..., None]

    def p_err(p, s_abs):                                           # score chain: 64 products + the -lse start, then v_exp
        return SAFE * p * (LN2 * 65 * U * (s_abs + nl.abs()[..., None]) + 4 * U)

    ak, aq = k.abs(), q.abs()
    e_pA = p_err(pA, qa.abs() @ ak.transpose(-1, -2))
    e_xA = SAFE * (e_pA * D.abs() + pA * e_D) + 2 * U * xA.abs()
    e_gq = scale * (round_spread(xA, e_xA) @ ak + N * U * (dSA.abs() @ ak)) + 2 * U * gq.abs()
    e_pB = p_err(pB, aq @ kb.abs().transpose(-1, -2))
    e_xB = SAFE * (e_pB * D.abs() + pB * e_D) + 2 * U * xB.abs()
    e_gk = scale * (round_spread(xB, e_xB).transpose(-1, -2) @ aq + N * U * (dSB.abs().transpose(-1, -2) @ aq)) + 2 * U * gk.abs()
    e_gv = round_spread(pB, e_pB).transpose(-1, -2) @ adO + N * U * (pBb.transpose(-1, -2) @ adO)
    return dict(dq=dq, dk=dk, dv=dv, dq_bound=result_bound(dq, e_gq), dk_bound=result_bound(dk, e_gk), dv_bound=result_bound(dv, e_gv))
