"""ResNet-50 backbone for config 1 ("Co-DINO 5-scale R50").  The reference cannot instantiate it
(``CoDETR.__init__`` asserts a Swin backbone, reference codetr/codetr.py:51); the R50 model exists
there only as config (configs lsj:30-39: mmdet ``ResNet`` depth 50, ``style='pytorch'``, frozen BN,
out_indices 0-3).  Restated from mmdet v3.3.0 / torchvision semantics with their parameter names
(``conv1``, ``bn1``, ``layer{1..4}.{b}.conv{1,2,3}/bn{1,2,3}/downsample.{0,1}``).  Inference only:
BatchNorm always uses its running statistics.

Two routes.  ``forward`` (NCHW, ATen / MIOpen convolutions) is the parity route: fp32, CPU-free GPU tests and
``route="nchw"``.  ``forward_tokens`` is the native 16-bit route (fp16 / bf16 on HIP, ``hip_ops.R50_NATIVE``): every
frozen BN is folded into its conv, maps stay token-major [B, H, W, C], and each layer is one libcodetr_hip.so launch --
stem window gather + GEMM (ReLU), max pool, and per bottleneck 1x1 GEMM (ReLU) -> 3x3 implicit-GEMM conv (ReLU) -> 1x1
GEMM with the ReLU after the residual (the identity, or the downsample conv's output)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import hip_ops

_STEM_KPAD = 192   # 3 x 7 x 7 = 147 columns of the stem's GEMM, padded to a multiple of 64


def _folded(conv, bn, kpad=None):
    """(weight, bias) of conv followed by frozen BN, folded in fp32 and rounded once to the conv's dtype:
    w * gamma / sqrt(var + eps) and beta - mean * gamma / sqrt(var + eps).  The weight is permuted to the
    [Cout, (ky, kx, c)] GEMM layout, or -- with kpad -- flattened in (c, ky, kx) order and zero-padded to kpad columns
    (the stem).  Cached on the conv weight (hip_ops.derived): rebuilt when a checkpoint is loaded or the model moves."""
    w = conv.weight
    srcs = (w, bn.weight, bn.bias, bn.running_mean, bn.running_var)

    def build():
        scale = bn.weight.float() / torch.sqrt(bn.running_var.float() + bn.eps)
        wf = w.detach().float() * scale[:, None, None, None]
        bias = (bn.bias.float() - bn.running_mean.float() * scale).to(w.dtype).contiguous()
        if kpad is not None:
            wk = torch.zeros((w.shape[0], kpad), dtype=w.dtype, device=w.device)
            wk[:, :wf[0].numel()] = wf.reshape(w.shape[0], -1).to(w.dtype)
        else:
            wk = wf.permute(0, 2, 3, 1).reshape(w.shape[0], -1).to(w.dtype).contiguous()
        return wk, bias

    return hip_ops.derived(srcs, "_codetr_bn_folded", build)


class _Bottleneck(nn.Module):
    def __init__(self, cin, planes, stride, downsample):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)  # style='pytorch': stride on the 3x3
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.downsample = downsample
        self.stride = stride

    @staticmethod
    def _bn(bn, x):
        return F.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)

    def forward(self, x):
        idt = x
        y = F.relu(self._bn(self.bn1, hip_ops.conv2d(x, self.conv1.weight)))
        y = F.relu(self._bn(self.bn2, hip_ops.conv2d(y, self.conv2.weight, None, self.stride, 1)))
        y = self._bn(self.bn3, hip_ops.conv2d(y, self.conv3.weight))
        if self.downsample is not None:
            idt = self._bn(self.downsample[1], hip_ops.conv2d(x, self.downsample[0].weight, None, self.stride, 0))
        return F.relu(y + idt)

    def forward_tokens(self, x):
        """x [B, H, W, Cin] token-major -> [B, Ho, Wo, 4 planes]"""
        B, H, W, _ = x.shape
        w1, b1 = _folded(self.conv1, self.bn1)
        w2, b2 = _folded(self.conv2, self.bn2)
        w3, b3 = _folded(self.conv3, self.bn3)
        y = hip_ops.linear(x, w1, b1, act="relu")
        y = hip_ops.conv_tokens(y, w2, b2, 3, self.stride, 1, act="relu")
        idt = x
        if self.downsample is not None:
            wd, bd = _folded(self.downsample[0], self.downsample[1])
            if self.stride == 1:
                idt = hip_ops.linear(x, wd, bd)
            else:
                idt = hip_ops.conv_tokens(x, wd, bd, 1, self.stride, 0)
        return hip_ops.linear(y, w3, b3, act="relu_res", residual=idt)


class ResNet(nn.Module):
    def __init__(self, depth=50, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=-1, norm_cfg=None,
                 norm_eval=True, style="pytorch", init_cfg=None, **kwargs):
        super().__init__()
        if depth != 50 or style != "pytorch" or num_stages != 4:
            raise NotImplementedError("only ResNet-50, style='pytorch' (the Co-DETR R50 config)")
        self.out_indices = tuple(out_indices)
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        cin = 64
        for li, (planes, n) in enumerate(zip((64, 128, 256, 512), (3, 4, 6, 3))):
            blocks = []
            for b in range(n):
                stride = 2 if (b == 0 and li > 0) else 1
                down = None
                if b == 0:
                    down = nn.Sequential(nn.Conv2d(cin, planes * 4, 1, stride, bias=False), nn.BatchNorm2d(planes * 4))
                blocks.append(_Bottleneck(cin, planes, stride, down))
                cin = planes * 4
            self.add_module(f"layer{li + 1}", nn.Sequential(*blocks))

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")

    def tokens_supported(self, x):
        """True when forward_tokens serves x: 16-bit HIP tensors, inference, hip_ops.R50_NATIVE.  fp32 / CPU / autograd
        calls keep the NCHW route (the parity route, bit for bit as before the native backbone)."""
        return (hip_ops.R50_NATIVE and x.is_cuda and x.dim() == 4 and x.shape[1] == 3
                and x.dtype in (torch.float16, torch.bfloat16) and self.conv1.weight.dtype == x.dtype
                and not torch.is_grad_enabled())

    def forward_tokens(self, x):
        """x [B, 3, H, W] -> [(tokens [B, H_i*W_i, C_i], (H_i, W_i))] for out_indices (as SwinTransformer.forward_tokens)"""
        if not self.tokens_supported(x):
            raise RuntimeError("ResNet.forward_tokens: 16-bit HIP inputs only, with hip_ops.R50_NATIVE "
                               "(fp32 / CPU / autograd run the NCHW route, ResNet.forward)")
        w, b = _folded(self.conv1, self.bn1, kpad=_STEM_KPAD)
        x = hip_ops.stem_conv_tokens(x, w, b, 7, 2, 3)
        x = hip_ops.maxpool_tokens(x)
        outs = []
        for i in range(4):
            for blk in getattr(self, f"layer{i + 1}"):
                x = blk.forward_tokens(x)
            if i in self.out_indices:
                B, H, W, C = x.shape
                outs.append((x.view(B, H * W, C), (H, W)))
        return outs

    def forward(self, x):
        x = F.relu(_Bottleneck._bn(self.bn1, hip_ops.conv2d(x, self.conv1.weight, None, 2, 3)))
        x = F.max_pool2d(x, 3, 2, 1)
        outs = []
        for i in range(4):
            x = getattr(self, f"layer{i + 1}")(x)
            if i in self.out_indices:
                outs.append(x)
        return outs
