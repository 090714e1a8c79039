"""ResNet-18 encoders of the reference (models/resnet.py: `resnet18`, `resnet18_ReGP_NRF`; BASELINE config 1) on the MI355X kernels.

`ResNet` owns the parameters under the reference's names (`conv1.{0,3,6}.weight`, `conv1.{1,4,7}.*`, `layer<i>.<b>.conv{1,2}.weight`,
`layer<i>.<b>.bn{1,2}.*`, `layer<i>.<b>.downsample.{0,1}.*`; `fc` is the Identity model.py:74-81 installs), so checkpoints carry over.
Compute is one autograd Function with a hand-written schedule, everything channel-last (a feature map IS the [B*H*W, C] matrix):

  x [B,1,F,T] --3x3 conv (C_in = 1, direct kernel)--> BN+ReLU --[im2col -> bf16 MFMA GEMM -> BN+ReLU] x2--> MaxPool(3, 2, 1)
     --> 8 BasicBlocks: [im2col -> GEMM -> BN+ReLU -> im2col -> GEMM -> BN] + identity (or subsample -> 1x1 GEMM -> BN) -> ReLU
     --> global average pool (resnet18) or max + mean over time of the (mel x channel) stack (ReGP, resnet18_ReGP_NRF)

Only BasicBlock networks are built: the Bottleneck variants (`resnet50*`) raise NotImplementedError in `ModelWrapper`.
BatchNorm2d statistics are exchanged across data-parallel ranks like the projector's (SyncBN, utils/utils.py:411).
"""
import torch
import torch.nn as nn

from . import ops
from .convbn import _bn_relu_out, _conv_bn_bwd, _conv_bn_fwd

BF16 = torch.bfloat16


def _pair(s):
    return tuple(s) if isinstance(s, (tuple, list)) else (s, s)


def conv3x3(in_planes, out_planes, stride=1):
    return nn.Conv2d(in_planes, out_planes, kernel_size=3, stride=_pair(stride), padding=1, bias=False)


def conv1x1(in_planes, out_planes, stride=1):
    return nn.Conv2d(in_planes, out_planes, kernel_size=1, stride=_pair(stride), bias=False)


class BasicBlock(nn.Module):
    """Parameter holder, models/resnet.py:33-80 (forward lives in ResNetFn)."""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = conv3x3(inplanes, planes, stride)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = conv3x3(planes, planes)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample
        self.stride = _pair(stride)


class ResNet(nn.Module):
    """models/resnet.py:141-274 for BasicBlock, the ResNet-C stem (C=True) and D=False -- what the reference's factories build."""

    def __init__(self, layers, strides, ReGP=False):
        super().__init__()
        self.ReGP = ReGP
        self.inplanes = 64
        self.stem_stride = _pair(strides[0])
        self.conv1 = nn.Sequential(
            nn.Conv2d(1, 32, kernel_size=3, stride=self.stem_stride, padding=1, bias=False), nn.BatchNorm2d(32), nn.ReLU(inplace=True),
            nn.Conv2d(32, 32, kernel_size=3, stride=1, padding=1, bias=False), nn.BatchNorm2d(32), nn.ReLU(inplace=True),
            nn.Conv2d(32, 64, kernel_size=3, stride=1, padding=1, bias=False), nn.BatchNorm2d(64), nn.ReLU(inplace=True))
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(64, layers[0], strides[1])
        self.layer2 = self._make_layer(128, layers[1], strides[2])
        self.layer3 = self._make_layer(256, layers[2], strides[3])
        self.layer4 = self._make_layer(512, layers[3], strides[4])
        if not ReGP:
            self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Identity()                                   # model.py:74-81 replaces the classifier by Identity
        for m in self.modules():                                   # models/resnet.py:199-204
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def _make_layer(self, planes, blocks, stride):
        downsample = None
        if _pair(stride) != (1, 1) or self.inplanes != planes:
            downsample = nn.Sequential(conv1x1(self.inplanes, planes, stride), nn.BatchNorm2d(planes))
        layers = [BasicBlock(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes
        for _ in range(1, blocks):
            layers.append(BasicBlock(self.inplanes, planes))
        return nn.Sequential(*layers)

    def blocks(self):
        return [b for layer in (self.layer1, self.layer2, self.layer3, self.layer4) for b in layer]

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError("ssl_audio_amd.resnet: CUDA (ROCm) tensors only -- there is no CPU path")
        return ResNetFn.apply(x, self, *self.parameters())


def resnet18():
    """models/resnet.py:277-292."""
    return ResNet([2, 2, 2, 2], [2, 1, 2, 2, 2])


def resnet18_ReGP_NRF():
    """models/resnet.py:349-360: ReGP + narrow receptive field (no stem stride, time-only stride in the last stage)."""
    return ResNet([2, 2, 2, 2], [1, 1, 2, 2, [1, 2]], ReGP=True)


# ---------------------------------------------------------------------------------------------------------------------------------
class ResNetFn(torch.autograd.Function):
    """x [S,1,F,T] fp32 -> embedding [S, 512] (average pool) or [S, C * F'] (ReGP).  Gradients: every parameter (the input gets none)."""

    @staticmethod
    def forward(ctx, x, net, *params):
        S, _, F_, T_ = x.shape
        dev = x.device
        x = x.contiguous()
        tape = []
        # ---- ResNet-C stem (models/resnet.py:177-188)
        tr = net.training
        r = _conv_bn_fwd(net.conv1[0], net.conv1[1], None, S, F_, T_, 1, True, x_img=x, training=tr)
        a = _bn_relu_out(r)
        stem = [r]
        for l in (1, 2):
            r = _conv_bn_fwd(net.conv1[3 * l], net.conv1[3 * l + 1], a, S, stem[-1].Ho, stem[-1].Wo, stem[-1].Co, True, training=tr)
            a = _bn_relu_out(r)
            stem.append(r)
        H, W, C = stem[-1].Ho, stem[-1].Wo, stem[-1].Co
        # ---- MaxPool2d(3, 2, 1)
        Hp, Wp = ops.pool_out_size(H), ops.pool_out_size(W)
        p16 = torch.empty(S * Hp * Wp, C, dtype=BF16, device=dev)
        p32 = torch.empty(S * Hp * Wp, C, device=dev)
        pidx = torch.empty(S * Hp * Wp, C, dtype=torch.uint8, device=dev)
        ops.maxpool3s2_fwd(a, S, H, W, C, p16, p32, pidx)
        pool = (H, W, C, pidx)
        del a
        # ---- BasicBlocks (models/resnet.py:62-80)
        y16, y32, H, W = p16, p32, Hp, Wp
        for blk in net.blocks():
            r1 = _conv_bn_fwd(blk.conv1, blk.bn1, y16, S, H, W, C, True, training=tr)
            a1 = _bn_relu_out(r1)
            r2 = _conv_bn_fwd(blk.conv2, blk.bn2, a1, S, r1.Ho, r1.Wo, r1.Co, False, training=tr)
            z = torch.empty(r2.h.shape[0], r2.Co, device=dev)
            ops.bn_apply(r2.h, r2.mean, r2.rstd, blk.bn2.weight.detach(), blk.bn2.bias.detach(), False, y_f32=z)
            rd = None
            idn = y32
            if blk.downsample is not None:
                rd = _conv_bn_fwd(blk.downsample[0], blk.downsample[1], y16, S, H, W, C, False, training=tr)
                idn = torch.empty(rd.h.shape[0], rd.Co, device=dev)
                ops.bn_apply(rd.h, rd.mean, rd.rstd, blk.downsample[1].weight.detach(), blk.downsample[1].bias.detach(), False, y_f32=idn)
            out32 = torch.empty_like(z)
            out16 = torch.empty(z.shape, dtype=BF16, device=dev)
            ops.add_relu_fwd(z, idn, out32, out16)
            tape.append((r1, r2, rd, out32))
            y16, y32, H, W, C = out16, out32, r2.Ho, r2.Wo, r2.Co
        # ---- head
        if net.ReGP:                                             # models/resnet.py:260-265: (B, T, mel * ch), max + mean over time
            fr = torch.empty(S, W, H * C, device=dev)
            ops.nhwc_to_frames(y16, S, H, W, C, frames_f32=fr.view(S * W, H * C))
            out = torch.empty(S, H * C, device=dev)
            arg = torch.empty(S, H * C, dtype=torch.int32, device=dev)
            ops.meanmax_time_fwd(fr, out, arg)
            ctx.head = (arg,)
        else:
            out = torch.empty(S, C, device=dev)
            ops.avgpool_fwd(y32, S, H * W, C, out)
            ctx.head = ()
        ctx.net, ctx.stem, ctx.pool, ctx.tape, ctx.last = net, stem, pool, tape, (S, H, W, C)
        ctx.params = params
        return out

    @staticmethod
    def backward(ctx, dout):
        net, stem, tape = ctx.net, ctx.stem, ctx.tape
        S, H, W, C = ctx.last
        dev = dout.device
        dout = dout.contiguous()
        grads = {}
        # ---- head
        dy = torch.empty(S * H * W, C, device=dev)
        if net.ReGP:
            dfr = torch.empty(S, W, H * C, device=dev)
            ops.meanmax_time_bwd(dout, ctx.head[0], dfr)
            ops.frames_to_nhwc(dfr.view(S * W, H * C), None, S, H, W, C, dy)
        else:
            ops.avgpool_bwd(dout, S, H * W, C, dy)
        # ---- blocks, last to first
        for r1, r2, rd, out32 in reversed(tape):
            ds = torch.empty_like(out32)
            ops.relu_bwd(dy, None, out32, ds)                    # through the block's final ReLU
            da1 = _conv_bn_bwd(r2, ds, grads)                    # bn2 + conv2  -> gradient at relu(bn1(.))
            dx = _conv_bn_bwd(r1, da1, grads)                    # bn1 (+ReLU) + conv1 -> gradient at the block input (written by col2im)
            if rd is not None:
                _conv_bn_bwd(rd, ds, grads, dx_out=dx)           # identity path: BN + strided 1x1 convolution, added at the sampled pixels
            else:
                ops.axpy(dx.view(-1), ds.view(-1))
            dy = dx
        # ---- MaxPool backward, stem
        Hs, Ws, Cs, pidx = ctx.pool
        da = torch.empty(S * Hs * Ws, Cs, device=dev)
        ops.maxpool3s2_bwd(dy, pidx, S, Hs, Ws, Cs, da)
        for r in reversed(stem):
            da = _conv_bn_bwd(r, da, grads)
        return (None, None) + tuple(grads.get(id(p)) for p in ctx.params)
