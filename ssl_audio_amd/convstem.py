"""ConvStem patch embedding of the `vitc_*` encoders (models/mae.py:46-99) on the MI355X kernels.

`ConvStem` owns the parameters with the reference's names (`proj.0.weight`, `proj.1.{weight,bias,running_*}`, ...,
`proj.<3n>.{weight,bias}`), so checkpoints carry over; its forward is never called.  Compute is `ConvStemTokensFn`:

  x [S,1,F,T] --conv3x3 s2 (C_in = 1: direct kernel)--> BN2d(batch stats) + ReLU --> [im2col -> bf16 MFMA GEMM -> BN2d + ReLU] x (n-1)
     --> 1x1 conv GEMM (+ bias + interpolated positional rows, scattered past the CLS row) --> CLS fill [--> keep-gather]

Feature maps are channel-last: a map IS the [B*H*W, C] matrix of the GEMM and of the BatchNorm kernels, and its row order is
the token order of `x.flatten(2).transpose(1, 2)`.  Unlike PatchEmbed the stem is TRAINED (models/mae.py:186-192 freezes only
the plain patch projection), so the Function has a backward.  Each conv + BatchNorm2d + ReLU layer is a convbn.py unit (forward and
backward, SyncBN statistics / sums exchanged across data-parallel ranks exactly like the projector's, utils/utils.py:411).
"""
import torch
import torch.nn as nn

from . import ops
from .convbn import _bn_relu_out, _conv_bn_bwd, _conv_bn_fwd
from .engine import BF16_WEIGHTS, _wgrad, grad_target
from .functional import pos_table_grad


def to_2tuple(x):
    return tuple(x) if isinstance(x, (list, tuple)) else (x, x)


def stem_strides(patch_size):
    """models/mae.py:58-67."""
    patch_size = tuple(patch_size)
    table = {(16, 16): [(2, 2)] * 4, (16, 8): [(2, 2)] * 3 + [(2, 1)], (8, 8): [(2, 2)] * 3 + [(1, 1)], (64, 2): [(2, 2)] + [(2, 1)] * 5}
    if patch_size not in table:
        raise ValueError(f'Patch size {patch_size[0]}x{patch_size[1]} is not supported by ConvStem')
    return table[patch_size]


class ConvStem(nn.Module):
    """Parameter holder with the reference's constructor and attribute names (models/mae.py:51-87)."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768, norm_layer=None, flatten=True):
        super().__init__()
        if in_chans != 1:
            raise NotImplementedError("audio spectrogram input only (in_chans=1)")
        if norm_layer is not None or not flatten:
            raise NotImplementedError("ConvStem: the reference call site uses norm_layer=None, flatten=True (models/mae.py:187)")
        self.img_size, self.patch_size = to_2tuple(img_size), to_2tuple(patch_size)
        self.strides = stem_strides(self.patch_size)
        assert embed_dim % 8 == 0, 'Embed dimension must be divisible by 8 for ConvStem'
        if (embed_dim // 8) % 8 != 0:
            raise NotImplementedError("ConvStem on the MI355X path needs embed_dim % 64 == 0 (channel counts are multiples of 8)")
        self.grid_size = (self.img_size[0] // self.patch_size[0], self.img_size[1] // self.patch_size[1])
        self.num_patches = self.grid_size[0] * self.grid_size[1]
        self.flatten = flatten
        stem = []
        input_dim, output_dim = 1, embed_dim // 8
        for l in range(len(self.strides)):
            stem.append(nn.Conv2d(input_dim, output_dim, kernel_size=3, stride=self.strides[l], padding=1, bias=False))
            stem.append(nn.BatchNorm2d(output_dim))
            stem.append(nn.ReLU(inplace=True))
            input_dim = output_dim
            if output_dim < embed_dim:
                output_dim *= 2
        stem.append(nn.Conv2d(input_dim, embed_dim, kernel_size=1))
        self.proj = nn.Sequential(*stem)
        self.norm = nn.Identity()

    def engine_params(self):
        """(conv weights, BN gammas, BN betas, final 1x1 weight, final bias) + the BatchNorm modules (for their buffers)."""
        n = len(self.strides)
        convs = [self.proj[3 * l] for l in range(n)]
        bns = [self.proj[3 * l + 1] for l in range(n)]
        return convs, bns, self.proj[3 * n]


class ConvStemTokensFn(torch.autograd.Function):
    """imgs [S,1,F,T] -> tokens [S, 1 + L (or keep), d] fp32: the conv stem, + positional rows, CLS row, optional keep-gather
    (prepare_tokens, models/mae.py:349-365 with patch_embed = ConvStem).  Gradients: every stem parameter, the CLS token and -- with
    `--use_learned_pos_embd` (:198-199; `pos_param` = the live nn.Parameter, `pos_A` = its resampling matrix or None) -- the positional table."""

    @staticmethod
    def forward(ctx, imgs, cls_token, pos, ids_keep, stem, pos_param, pos_A, *params):
        convs, bns, last = stem.engine_params()
        S, _, F_, T_ = imgs.shape
        dev = imgs.device
        x = imgs.contiguous()
        recs = []
        a, H, W, C = None, F_, T_, 1
        for conv, bn in zip(convs, bns):
            r = _conv_bn_fwd(conv, bn, a, S, H, W, C, True, x_img=None if recs else x, training=stem.training)
            a = _bn_relu_out(r)
            recs.append(r)
            H, W, C = r.Ho, r.Wo, r.Co
        L = H * W
        d = last.weight.shape[0]
        if pos.shape[-2] != 1 + L:
            raise ValueError(f"ConvStem produced {L} patch tokens but the positional table has {pos.shape[-2] - 1}: the input length must "
                             f"give floor(T / patch) columns through every stride-2 stage (T % {stem.patch_size[1]} == 0)")
        tok = torch.empty(S, 1 + L, d, device=dev)
        pos2 = pos.detach().reshape(1 + L, d)
        ops.gemm(a, BF16_WEIGHTS.get(last.weight), bias=last.bias.detach(), residual=pos2[1:], res_mod=L, row_group=L, out_f32=tok.view(S * (1 + L), d))
        ops.fill_cls(tok, S, (1 + L) * d, d, cls_token.detach().reshape(-1), pos2[0])
        ctx.keep_rows = None
        if ids_keep is not None:
            keep = ids_keep.shape[1]
            out = torch.empty(S, 1 + keep, d, device=dev)
            rows = torch.cat([torch.zeros(S, 1, dtype=torch.int32, device=dev), ids_keep + 1], dim=1).contiguous()
            ops.gather_rows(tok, (1 + L) * d, 0, rows, out, (1 + keep) * d, 0, S, d)
            ctx.keep_rows = rows
            tok = out
        ctx.stem, ctx.recs, ctx.a_last = stem, recs, a
        ctx.cls_param = cls_token
        ctx.pos_param = pos_param if (pos_param is not None and pos_param.requires_grad) else None
        ctx.pos_A = pos_A
        ctx.L = L
        return tok

    @staticmethod
    def backward(ctx, dtok):
        stem, recs = ctx.stem, ctx.recs
        last = stem.engine_params()[2]
        S = dtok.shape[0]
        L = ctx.L
        dev = dtok.device
        dtok = dtok.contiguous()
        d = dtok.shape[-1]
        if ctx.keep_rows is not None:                       # un-gather: rows that were dropped by the masking get zero gradient
            full = torch.zeros(S, 1 + L, d, device=dev)
            keep1 = ctx.keep_rows.shape[1]
            ops.scatter_add_rows(dtok, keep1 * d, 0, ctx.keep_rows, full, (1 + L) * d, 0, S, d)
            dtok = full
        dcls = None
        if ctx.needs_input_grad[1]:
            buf, dcls = grad_target(ctx.cls_param)
            ops.cls_grad(dtok, S, (1 + L) * d, d, buf.view(-1))
        dpos = pos_table_grad(dtok, ctx.pos_param, ctx.pos_A) if ctx.pos_param is not None else None
        dy16 = ops.cast_bf16(dtok[:, 1:].contiguous().view(S * L, d))
        # 1x1 conv
        grads = {}
        dwb, grads[id(last.weight)] = grad_target(last.weight)
        _wgrad(dy16, ctx.a_last, dwb.view(d, -1))
        dbb, grads[id(last.bias)] = grad_target(last.bias)
        ops.colsum_bf16(dy16, dbb, accumulate=True)
        da = torch.empty(S * L, recs[-1].Co, device=dev)
        ops.gemm(dy16, BF16_WEIGHTS.get(last.weight), b_kmajor=False, out_f32=da)
        for r in reversed(recs):
            da = _conv_bn_bwd(r, da, grads)
        return (None, dcls, None, None, None, dpos, None, *(grads[id(p)] for p in stem_flat_params(stem)))


def stem_flat_params(stem):
    convs, bns, last = stem.engine_params()
    flat = []
    for c, b in zip(convs, bns):
        flat += [c.weight, b.weight, b.bias]
    return flat + [last.weight, last.bias]
