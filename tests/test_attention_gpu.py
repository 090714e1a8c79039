"""The fused attention kernels (ssl_audio_amd/csrc/attention.hip) element by element against their rounding mirror (tests/attn_mirror.py).

Every element of out / lse / dq / dk / dv is held to a bound the mirror derives from its own magnitudes: one bf16 ulp of the result,
the fp32 accumulation terms, and a one-ulp flip of a rounded intermediate only where that intermediate lies within its fp32-level error
of a bf16 rounding boundary.  Each check prints its worst error / bound ratio (pytest -s shows them); a ratio just under 1 is a one-ulp
disagreement of the result's own rounding, which the bound allows; two ulps without the error to explain them fail.  The lengths
cover every 16-key tile, 32-key step and FULL-dispatch edge of both instantiations; the probes turn a mask or coverage bug into an
O(1) error."""
import math
import os
import subprocess
import sys

import pytest
import torch

import attn_mirror as am

pytestmark = pytest.mark.gpu

from ssl_audio_amd import ops  # noqa: E402

BF16 = torch.bfloat16
SCALE = 0.125
SENTINEL = 0x7FA5            # a bf16 NaN with a payload no arithmetic produces: outputs are pre-filled with it


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    ops.lib()
    return torch.device("cuda:0")


def sentinel(rows, cols, dev):
    return torch.full((rows, cols), SENTINEL, dtype=torch.int16, device=dev).view(BF16)


def untouched(x):
    return bool((x.contiguous().view(torch.int16) == SENTINEL).all())


def qk_sd(scale, score_sd=2.0):
    """Standard deviation of q and k entries that gives scaled scores of standard deviation score_sd (head_dim 64)."""
    return math.sqrt(score_sd / (8.0 * scale))


def randn(shape, seed, dev, sd=1.0):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(shape, generator=g, device=dev) * sd


def make_qkv(S, H, N, seed, dev, scale=SCALE, ld=None):
    """bf16 qkv rows; with ld > 3C a view into a wider buffer whose other columns are NaN (read nowhere)."""
    C = 64 * H
    x = randn((S * N, 3 * C), seed, dev)
    x[:, :2 * C] *= qk_sd(scale)
    return widen(x.to(BF16), ld)


def widen(x, ld):
    if ld is None or ld == x.shape[1]:
        return x
    buf = torch.full((x.shape[0], ld), float("nan"), dtype=x.dtype, device=x.device)
    buf[:, :x.shape[1]] = x
    return buf[:, :x.shape[1]]


def worst(name, group, got, ref, bound):
    """Every element finite and inside its bound; returns the worst error / bound ratio."""
    got = got.double()
    assert bool(torch.isfinite(got).all()), f"{group} {name}: non-finite output"
    ratio = float(((got - ref).abs() / bound).max()) if got.numel() else 0.0
    assert ratio <= 1.0, f"{group} {name}: worst error / bound {ratio:.3f}"
    return ratio


def chunks(S, H, N):
    step = max(1, (1 << 26) // (H * N * N))          # mirror intermediates of <= 512 MiB each
    return [(s0, min(S, s0 + step)) for s0 in range(0, S, step)]


def check_fwd(group, qkv, H, N, scale, nq, out, lse):
    """out [S*N, >=C] and lse [S*H, N] of the kernel against the mirror on the first nq rows of every sequence."""
    S = qkv.shape[0] // N
    nq = nq or N
    r = {"out": 0.0, "lse": 0.0}
    for s0, s1 in chunks(S, H, N):
        q, k, v = am.split_heads(qkv[s0 * N:s1 * N], H, N)
        m = am.forward(q, k, v, scale, n_query=nq)
        o = am.split_rows(out[s0 * N:s1 * N], H, N)[:, :, :nq]
        ls = lse[s0 * H:s1 * H].double().view(s1 - s0, H, N)[:, :, :nq]
        r["out"] = max(r["out"], worst("out", group, o, m["out"], m["out_bound"]))
        r["lse"] = max(r["lse"], worst("lse", group, ls, m["lse"], m["lse_bound"]))
    return r


def check_bwd(group, qkv, H, N, scale, nq, out, dout, lse, dqkv):
    S = qkv.shape[0] // N
    C = 64 * H
    r = {"dq": 0.0, "dk": 0.0, "dv": 0.0}
    for s0, s1 in chunks(S, H, N):
        rows = slice(s0 * N, s1 * N)
        q, k, v = am.split_heads(qkv[rows], H, N)
        m = am.backward(q, k, v, am.split_rows(out[rows], H, N), am.split_rows(dout[rows], H, N),
                        lse[s0 * H:s1 * H].double().view(s1 - s0, H, N), scale, n_query=nq or N)
        for i, name in enumerate(("dq", "dk", "dv")):
            got = am.split_rows(dqkv[rows, i * C:(i + 1) * C], H, N)
            r[name] = max(r[name], worst(name, group, got, m[name], m[name + "_bound"]))
    return r


def launch(qkv, H, N, scale=SCALE, nq=0, ldo=None, dout=None):
    """Forward then backward into sentinel-filled outputs (out, dout as views with leading dimension ldo; dqkv with qkv's)."""
    rows, C, ld = qkv.shape[0], 64 * H, qkv.stride(0)
    dev = qkv.device
    out = sentinel(rows, ldo or C, dev)[:, :C]
    lse = torch.full(((rows // N) * H, N), float("nan"), device=dev)
    ops.attention_fwd(qkv, H, N, scale, out, lse, n_query=nq)
    if 0 < nq < N:
        rest = (torch.arange(rows, device=dev) % N) >= nq
        assert untouched(out[rest]), "the forward wrote out rows >= n_query"
        out[rest] = 0                                    # rows the backward reads but must not use: finite, as the engine leaves them
    if dout is None:
        dout = randn((rows, C), 7, dev).to(BF16)
    dout = widen(dout, ldo)
    dqkv = sentinel(rows, ld, dev)[:, :3 * C]
    ops.attention_bwd(qkv, H, N, scale, out, dout, lse, dqkv, n_query=nq)
    torch.cuda.synchronize()
    return out, lse, dout, dqkv


def full_check(group, qkv, H, N, scale=SCALE, nq=0, ldo=None, dout=None):
    out, lse, dout, dqkv = launch(qkv, H, N, scale, nq, ldo, dout)
    # every element the header says is written came back: the sentinel is a NaN, and `worst` requires finite values
    rf = check_fwd(group, qkv, H, N, scale, nq or N, out, lse)
    rb = check_bwd(group, qkv, H, N, scale, nq, out, dout, lse, dqkv)
    r = {**rf, **rb}
    print(f"[{group}] worst error/bound " + "  ".join(f"{k} {v:.3f}" for k, v in r.items()))
    return r


# ------------------------------------------------------------------------------------------------ length sweep
# every tile / step / FULL edge: NMAX = 256 (FULL for N > 240) and NMAX = 512 (FULL for N > 496); N > 128 / 256: a wave loops over
# more than one 16-query tile
LENGTHS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 225, 233, 240, 241, 248, 249, 255, 256,
           257, 258, 272, 288, 383, 384, 496, 497, 500, 501, 511, 512]


@pytest.mark.parametrize("N", LENGTHS)
def test_length_sweep(dev, N):
    """Three sequences (the padded rows of the first two read the next sequence, those of the last the buffer's zero-filled end)."""
    full_check(f"sweep N={N}", make_qkv(3, 2, N, 100 + N, dev), 2, N)


@pytest.mark.parametrize("N", [40, 249, 501])
def test_strided_views(dev, N):
    """ld > 3C and ldo > C: views into wider buffers.  The input columns outside the window are NaN (a read of them would show), the
    output columns outside it must come back untouched."""
    H = 2
    C = 64 * H
    qkv = make_qkv(3, H, N, 200 + N, dev, ld=3 * C + 64)
    out, lse, dout, dqkv = launch(qkv, H, N, ldo=C + 64)
    assert untouched(out.as_strided((out.shape[0], 64), (out.stride(0), 1), out.storage_offset() + C))
    assert untouched(dqkv.as_strided((dqkv.shape[0], 64), (dqkv.stride(0), 1), dqkv.storage_offset() + 3 * C))
    r = {**check_fwd("strided", qkv, H, N, SCALE, N, out, lse), **check_bwd("strided", qkv, H, N, SCALE, 0, out, dout, lse, dqkv)}
    print(f"[strided N={N}] worst error/bound " + "  ".join(f"{k} {v:.3f}" for k, v in r.items()))


# ------------------------------------------------------------------------------------------------ n_query
@pytest.mark.parametrize("N", [249, 501])
@pytest.mark.parametrize("nq_of", [lambda N: 1, lambda N: 15, lambda N: 16, lambda N: 17, lambda N: N - 1], ids=["1", "15", "16", "17", "N-1"])
def test_n_query(dev, N, nq_of):
    """Only the first n_query rows of each sequence are queries.  The forward writes exactly those rows of out (and lse), equal to the
    full launch's bit for bit; the backward's rows >= n_query of out and dout only have to be finite: large junk there gives the same
    dqkv, bit for bit, as zeros -- and as the full launch fed with a dout that is zero outside the queried rows."""
    S, H = 3, 2
    C = 64 * H
    nq = nq_of(N)
    qkv = make_qkv(S, H, N, 300 + nq, dev)
    full = torch.empty(S * N, C, device=dev, dtype=BF16)
    lse_full = torch.empty(S * H, N, device=dev)
    ops.attention_fwd(qkv, H, N, SCALE, full, lse_full)
    part = sentinel(S * N, C, dev)
    lse = torch.full((S * H, N), float("nan"), device=dev)
    ops.attention_fwd(qkv, H, N, SCALE, part, lse, n_query=nq)
    torch.cuda.synchronize()
    q_rows = (torch.arange(S * N, device=dev) % N) < nq
    assert torch.equal(part[q_rows], full[q_rows]) and untouched(part[~q_rows])
    assert torch.equal(lse[:, :nq], lse_full[:, :nq]) and bool(torch.isnan(lse[:, nq:]).all())
    r = check_fwd(f"n_query {nq} N={N}", qkv, H, N, SCALE, nq, part, lse)

    dout = randn((S * N, C), 301, dev).to(BF16)
    junk = randn((S * N, C), 302, dev, 1e3).to(BF16)
    zero = torch.zeros_like(dout)
    sel = q_rows[:, None]
    results = {}
    for tag, o_rest, d_rest in [("junk", junk, junk.flip(0)), ("zero", zero, zero)]:
        dq = sentinel(S * N, 3 * C, dev)
        ops.attention_bwd(qkv, H, N, SCALE, torch.where(sel, part, o_rest), torch.where(sel, dout, d_rest), lse, dq, n_query=nq)
        results[tag] = dq
    ref = sentinel(S * N, 3 * C, dev)
    ops.attention_bwd(qkv, H, N, SCALE, full, torch.where(sel, dout, zero), lse_full, ref)
    torch.cuda.synchronize()
    assert torch.equal(results["junk"], results["zero"])
    assert torch.equal(results["zero"], ref)
    r.update(check_bwd(f"n_query {nq} N={N}", qkv, H, N, SCALE, nq, torch.where(sel, part, zero), torch.where(sel, dout, zero), lse, results["junk"]))
    print(f"[n_query {nq} N={N}] worst error/bound " + "  ".join(f"{k} {v:.3f}" for k, v in r.items()))


# ------------------------------------------------------------------------------------------------ probes
def direction(dev):
    return torch.full((64,), 1.0 / 8.0, device=dev)             # a unit vector


@pytest.mark.parametrize("N", LENGTHS)
def test_leak_probe(dev, N):
    """Neighbouring sequences get opposite key directions: a sequence's own scaled scores are all ~ -40, a key of the next sequence
    scores ~ +40 and a zero-filled row past the end 0 -- one such key past N takes over the softmax instead of moving it by a rounding."""
    S, H = 3, 2
    C = 64 * H
    a = math.sqrt(40.0 / SCALE)
    sign = torch.tensor([1.0, -1.0, 1.0], device=dev).repeat_interleave(N)[:, None, None]
    u = direction(dev)
    q = sign * a * u + randn((S * N, H, 64), 400 + N, dev, 0.5)
    k = -sign * a * u + randn((S * N, H, 64), 401 + N, dev, 0.5)
    v = randn((S * N, H, 64), 402 + N, dev)
    qkv = torch.cat([q.reshape(S * N, C), k.reshape(S * N, C), v.reshape(S * N, C)], 1).to(BF16)
    full_check(f"leak N={N}", qkv, H, N)


@pytest.mark.parametrize("N", [17, 64, 241, 249, 256, 257, 497, 501, 512])
def test_coverage_probe(dev, N):
    """One dominant key per (sequence, head), its position swept over 0 .. N-1 across the batch: every output row is that key's V, and
    its dV row carries the whole dO of the sequence's queries.  The dominant key scores ~0 and every other key ~ -30 (scaled): with a
    dominant score near 0 the backward's bf16 prescale of Q / K (a relative 2^-9 of the score) leaves its p at 1."""
    H = 3
    S = -(-N // H)
    C = 64 * H
    a = math.sqrt(30.0 / SCALE)
    u = direction(dev)
    q = a * u + randn((S, N, H, 64), 500 + N, dev, 0.2)
    k = -a * u + randn((S, N, H, 64), 501 + N, dev, 0.2)
    v = randn((S, N, H, 64), 502 + N, dev)
    pos = torch.arange(S * H, device=dev).view(S, H) % N
    si, hi = torch.arange(S, device=dev)[:, None].expand(S, H), torch.arange(H, device=dev)[None, :].expand(S, H)
    k[si, pos, hi] = randn((S, H, 64), 504 + N, dev, 0.2)
    qkv = torch.cat([q.reshape(S * N, C), k.reshape(S * N, C), v.reshape(S * N, C)], 1).to(BF16)
    dout = randn((S * N, C), 503 + N, dev).to(BF16)
    full_check(f"coverage N={N}", qkv, H, N, dout=dout)
    out, _, _, dqkv = launch(qkv, H, N, dout=dout)
    vd = am.split_rows(qkv[:, 2 * C:], H, N)                    # [S, H, N, 64]
    vdom = vd[si, hi, pos]                                       # [S, H, 64]
    o = am.split_rows(out, H, N)
    assert float((o - vdom[:, :, None]).abs().max()) <= 2.0 ** -8 * float(vdom.abs().max())
    dv = am.split_rows(dqkv[:, 2 * C:], H, N)[si, hi, pos]
    dsum = am.split_rows(dout, H, N).sum(2)
    assert float((dv - dsum).abs().max()) <= 2.0 ** -6 * float(dsum.abs().max())


@pytest.mark.parametrize("N", [33, 249, 501])
def test_extremes(dev, N):
    """Flat rows (q = 0: every p = 1, out = the mean of V) and very peaked rows (scaled scores of standard deviation 50, so around +-100:
    most p underflow in exp2) -- the max subtraction and the underflow."""
    H = 2
    C = 64 * H
    flat = make_qkv(2, H, N, 600 + N, dev)
    flat[:, :C] = 0
    full_check(f"flat N={N}", flat, H, N)
    peak = randn((2 * N, 3 * C), 601 + N, dev)
    peak[:, :2 * C] *= qk_sd(SCALE, 50.0)
    full_check(f"peaked N={N}", peak.to(BF16), H, N)


# ------------------------------------------------------------------------------------------------ step shapes
@pytest.mark.parametrize("name,S,H,N,nq", [("ViT-B bench", 256, 12, 249, 0), ("ViT-T", 64, 3, 249, 0), ("ConvStem 16x8 10 s", 16, 12, 501, 0),
                                           ("MAE encoder, masked", 256, 12, 63, 0), ("CLS-only last block", 256, 12, 249, 1)])
def test_step_shapes(dev, name, S, H, N, nq):
    dout = None
    if nq:
        dout = randn((S * N, 64 * H), 700, dev).to(BF16)
        dout.view(S, N, -1)[:, nq:] = 0                          # what the engine passes (dao is zero-filled)
    full_check(name, make_qkv(S, H, N, 701, dev), H, N, nq=nq, dout=dout)


# ------------------------------------------------------------------------------------------------ determinism and variants
@pytest.mark.parametrize("S,H,N", [(8, 4, 249), (4, 3, 501), (5, 2, 100)])
def test_two_launches_are_bit_identical(dev, S, H, N):
    qkv = make_qkv(S, H, N, 800, dev)
    a = launch(qkv, H, N)
    b = launch(qkv, H, N)
    for x, y in zip(a, b):
        assert torch.equal(x.contiguous().view(torch.int16), y.contiguous().view(torch.int16))


def test_persistent_backward_is_bit_identical(dev):
    """SA_ATTN_BWD_PERSIST=1 (the library reads it once: one child process per setting, one after the other) gives the default dqkv
    bit for bit, with more heads than the persistent grid has workgroups so that a workgroup walks several."""
    script = os.path.join(os.path.dirname(__file__), "attn_bwd_check.py")
    digests = {}
    for flag in ("0", "1"):
        env = dict(os.environ, SA_ATTN_BWD_PERSIST=flag)
        r = subprocess.run([sys.executable, script], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        digests[flag] = [line for line in r.stdout.splitlines() if line.startswith("dqkv ")]
    assert len(digests["0"]) == 3 and digests["0"] == digests["1"], digests


@pytest.mark.parametrize("scale", [0.2, 0.0625])
@pytest.mark.parametrize("N", [249, 501])
def test_other_scale(dev, scale, N):
    full_check(f"scale {scale} N={N}", make_qkv(3, 2, N, 900 + N, dev, scale=scale), 2, N, scale=scale)
