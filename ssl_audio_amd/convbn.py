"""The conv + BatchNorm2d (+ ReLU) unit that ResNet, the ConvStem and AudioNTT are built from, on channel-last maps ([B*H*W, C]).

`_conv_bn_fwd` runs one convolution (optional bias) and the BatchNorm statistics and returns a `_ConvBN` record; `_bn_relu_out`
applies the BatchNorm; `_conv_bn_bwd` walks a record backwards.  Convolutions: the single-channel first layer is a direct kernel, a
3x3 is im2col + bf16 GEMM (dgrad GEMM + col2im, wgrad on the recomputed im2col), a strided 1x1 is row subsampling + GEMM.  Training-
mode BatchNorm exchanges its statistics and backward sums across data-parallel ranks (SyncBN, utils/utils.py:411)."""
import torch

from . import dist as sdist
from . import ops
from .engine import BF16_WEIGHTS, _wgrad, grad_target

BF16 = torch.bfloat16
BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def _bn_forward(h, bn, training=True):
    """Training: batch statistics of a tall [M, C] map (SyncBN over ranks) -> mean, rstd; running buffers updated like nn.BatchNorm2d.
    Eval (`bn.eval()`, nn.BatchNorm2d's inference form): the running statistics -- no column pass, no collective, buffers untouched."""
    M, Cn = h.shape
    dev = h.device
    if not training:
        return bn.running_mean.detach(), torch.rsqrt(bn.running_var.detach() + bn.eps)
    stats = torch.empty(2, Cn, device=dev)
    ops.bn_colstats_tall(h, stats[0], stats[1])
    allst = sdist.all_gather_rows(stats)
    mean, rstd = torch.empty(Cn, device=dev), torch.empty(Cn, device=dev)
    ops.bn_finalize(allst, M, BN_EPS, BN_MOMENTUM, mean, rstd, bn.running_mean, bn.running_var)
    with torch.no_grad():
        bn.num_batches_tracked += 1
    return mean, rstd


def bn_bwd_sums(s, training):
    """The two sums the BatchNorm input gradient subtracts: the cross-rank totals in training; zeros in eval, where the layer is the
    fixed affine map of its running statistics and dx = gamma * rstd * dy (the parameter gradients are the local sums either way)."""
    if training:
        sdist.all_reduce_sum_(s)
        return s
    return torch.zeros_like(s)


def _pack_conv_weight(w, kpad, rows=None):
    """[C_out, C_in, 3, 3] fp32 master -> bf16 [rows >= C_out, kpad] in im2col order (ky, kx, c_in), zero padded (the dgrad GEMM
    reduces over C_out, which the k-major operand rule wants as a multiple of 64).  Data movement + one cast."""
    co, ci = w.shape[0], w.shape[1]
    packed = torch.zeros(rows or co, kpad, device=w.device)
    packed[:co, :9 * ci] = w.detach().permute(0, 2, 3, 1).reshape(co, 9 * ci)
    return ops.cast_bf16(packed)


def _kpad(ci):
    return (9 * ci + 63) // 64 * 64


class _ConvBN:
    """One convolution + BatchNorm2d of the forward, with what its backward needs."""
    __slots__ = ("conv", "bn", "k", "stride", "relu", "S", "H", "W", "Ci", "Ho", "Wo", "Co", "a_in", "x_img", "h", "mean", "rstd", "train")


def _conv_bn_fwd(conv, bn, a16, S, H, W, Ci, relu, x_img=None, training=True):
    """a16 bf16 [S*H*W, Ci] (or x_img fp32 [S,1,H,W] for the single-channel first layer) -> record with h = conv output (fp32, + the
    conv's bias when it has one) and the batch statistics.  3x3 (pad 1) through im2col + GEMM, 1x1 through row subsampling + GEMM."""
    r = _ConvBN()
    r.conv, r.bn, r.relu = conv, bn, relu
    r.k = conv.kernel_size[0]
    r.stride = tuple(conv.stride)
    r.S, r.H, r.W, r.Ci = S, H, W, Ci
    sh, sw = r.stride
    r.Co = conv.weight.shape[0]
    dev = conv.weight.device
    if r.k == 3:
        r.Ho, r.Wo = ops.conv_out_size(H, sh), ops.conv_out_size(W, sw)
    else:
        r.Ho, r.Wo = (H - 1) // sh + 1, (W - 1) // sw + 1
    M = S * r.Ho * r.Wo
    r.h = torch.empty(M, r.Co, device=dev)
    r.x_img, r.a_in = x_img, a16
    bias = conv.bias.detach() if conv.bias is not None else None
    if x_img is not None:
        ops.conv3x3_c1_fwd(x_img, conv.weight.detach().reshape(r.Co, 9).contiguous(), bias, r.stride, r.h)
    elif r.k == 3:
        kp = _kpad(Ci)
        P = torch.empty(M, kp, dtype=BF16, device=dev)
        ops.im2col3x3(a16, S, H, W, Ci, r.stride, P)
        ops.gemm(P, _pack_conv_weight(conv.weight, kp), bias=bias, out_f32=r.h)
        del P
    else:
        xs = a16
        if r.stride != (1, 1):
            xs = torch.empty(M, Ci, dtype=BF16, device=dev)
            ops.subsample_fwd(a16, S, H, W, Ci, r.stride, xs)
        r.a_in = xs                                              # the 1x1 convolution's GEMM operand (already subsampled)
        ops.gemm(xs, BF16_WEIGHTS.get(conv.weight), bias=bias, out_f32=r.h)
    r.train = training
    r.mean, r.rstd = _bn_forward(r.h, bn, training)
    return r


def _conv_bn_bwd(r, dz, grads, dx_out=None, need_dx=True):
    """dz fp32 [M, Co]: gradient at the BatchNorm output (after the ReLU when r.relu).  Accumulates the parameter gradients into `grads`
    (id -> autograd value) and returns the gradient at the convolution's input: fp32 [S*H*W, Ci] written by col2im for a 3x3, or, for a
    1x1, ADDED into dx_out at the sampled pixels; None for the single-channel first layer."""
    conv, bn = r.conv, r.bn
    dev = dz.device
    M, Co, Ci = r.h.shape[0], r.Co, r.Ci
    W_ = sdist.get_world_size()
    gamma, beta = bn.weight, bn.bias
    s = torch.empty(2, Co, device=dev)
    ops.bn_bwd_stats_tall(dz, r.h, r.mean, r.rstd, gamma, beta, r.relu, s[0], s[1])
    dgb, grads[id(gamma)] = grad_target(gamma)
    dbb, grads[id(beta)] = grad_target(beta)
    ops.axpy(dbb, s[0])
    ops.axpy(dgb, s[1])
    s = bn_bwd_sums(s, r.train)
    cpad = (Co + 63) // 64 * 64 if r.x_img is None else Co            # zero columns up to the dgrad GEMM's K granule
    dh_full = torch.zeros(M, cpad, dtype=BF16, device=dev) if cpad != Co else torch.empty(M, Co, dtype=BF16, device=dev)
    dh = dh_full[:, :Co]
    ops.bn_bwd_apply(dz, r.h, r.mean, r.rstd, gamma, beta, r.relu, s[0], s[1], 1.0 / (M * W_), dx_bf16=dh)
    dwbuf, grads[id(conv.weight)] = grad_target(conv.weight)
    dbias = None
    if conv.bias is not None:
        dbias, grads[id(conv.bias)] = grad_target(conv.bias)
    if r.x_img is not None:
        ops.conv3x3_c1_wgrad(r.x_img, dh, r.stride, dwbuf.view(Co, 9), dbias)
        return None
    if dbias is not None:
        ops.colsum_bf16(dh, dbias, accumulate=True)
    if r.k == 1:
        _wgrad(dh, r.a_in, dwbuf.view(Co, Ci))
        if not need_dx:
            return None
        dxs = torch.empty(M, Ci, dtype=BF16, device=dev)
        w16 = BF16_WEIGHTS.get(conv.weight)
        if cpad != Co:
            wp = torch.zeros(cpad, Ci, dtype=BF16, device=dev)
            wp[:Co] = w16
            w16 = wp
        ops.gemm(dh_full, w16, b_kmajor=False, out_bf16=dxs)
        if r.stride == (1, 1):
            raise NotImplementedError("1x1 convolution without stride is not part of the BasicBlock networks")
        ops.subsample_bwd_add(dxs, r.S, r.H, r.W, Ci, r.stride, dx_out)
        return dx_out
    kp = _kpad(Ci)
    P = torch.empty(M, kp, dtype=BF16, device=dev)
    ops.im2col3x3(r.a_in, r.S, r.H, r.W, Ci, r.stride, P)            # recomputed: cheaper than keeping 9x the activations
    dwp = torch.zeros(Co, kp, device=dev)
    _wgrad(dh, P, dwp)
    del P
    # back to the parameter's [C_out, C_in, 3, 3] layout: a permuted copy (data movement), accumulated by the axpy kernel
    ops.axpy(dwbuf.view(-1), dwp[:, :9 * Ci].reshape(Co, 3, 3, Ci).permute(0, 3, 1, 2).contiguous().view(-1))
    if not need_dx:
        return None
    dP = torch.empty(M, kp, dtype=BF16, device=dev)
    ops.gemm(dh_full, _pack_conv_weight(conv.weight, kp, rows=cpad), b_kmajor=False, out_bf16=dP)
    da = torch.empty(r.S * r.H * r.W, Ci, device=dev)
    ops.col2im3x3(dP, r.S, r.H, r.W, Ci, r.stride, da)
    return da


def _bn_relu_out(r):
    """BN (+ ReLU) of a record -> bf16 activation for the next convolution."""
    a = torch.empty(r.h.shape[0], r.Co, dtype=BF16, device=r.h.device)
    ops.bn_apply(r.h, r.mean, r.rstd, r.bn.weight.detach(), r.bn.bias.detach(), r.relu, y_bf16=a)
    return a
