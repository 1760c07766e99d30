"""A plain float64 reference of the conv engine's one layer (csrc/conv.hip, conv_dma.hip):
im2col + matmul, the fused epilogue in conv_epilogue's order, the output routing, and
MaxPool2d(k, s, ceil_mode=True).  torch float64, NHWC, on whatever device the inputs are on; it
shares no code with the kernels.  tests/test_conv_ref.py pins it to torch.nn.functional on the CPU.

Every function takes an optional `absolute=True` twin where it matters: conv2d(|x|, |w|) and
epilogue(..., absolute=True) propagate magnitudes instead of values, which gives the scale
S = sum |a||w| + |epilogue terms| the GPU tests measure errors against."""
import math

import torch


def out_size(L, k, s, p):
    return (L + 2 * p - k) // s + 1


def im2col(x, Cin, KH, KW, stride=(1, 1), pad=(0, 0)):
    """x [N,H,W,C>=Cin] -> [N,OH,OW,KH*KW*Cin] (k = (kh, kw, ci)), zero padding."""
    N, H, W, _ = x.shape
    (sh, sw), (ph, pw) = stride, pad
    OH, OW = out_size(H, KH, sh, ph), out_size(W, KW, sw, pw)
    xp = torch.zeros((N, H + 2 * ph, W + 2 * pw, Cin), dtype=torch.float64, device=x.device)
    xp[:, ph:ph + H, pw:pw + W] = x[..., :Cin].to(torch.float64)
    taps = [xp[:, kh:kh + sh * (OH - 1) + 1:sh, kw:kw + sw * (OW - 1) + 1:sw] for kh in range(KH) for kw in range(KW)]
    return torch.stack(taps, dim=3).reshape(N, OH, OW, KH * KW * Cin)


def conv2d(x, w, stride=(1, 1), pad=(0, 0)):
    """x [N,H,W,C>=Cin] (the first Cin channels are read: in_cstride), w [Cout,KH,KW,Cin] ->
    float64 [N,OH,OW,Cout]."""
    Cout, KH, KW, Cin = w.shape
    a = im2col(x, Cin, KH, KW, stride, pad)
    return a @ w.to(torch.float64).reshape(Cout, -1).T


def up2(v):
    """nearest x2 upsample of [N,H,W,C] (F.interpolate(scale_factor=2))."""
    return v.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def epilogue(v, bias=None, alpha=None, beta=None, scale=1.0, res=None, res_post=False, res_up2=False, relu=False,
             leaky=False, slope=0.0, prelu=None, gelu=False, absolute=False):
    """conv_epilogue's order on v [N,OH,OW,Cout]: bias, v*alpha+beta, scale, residual (pre),
    relu / leaky / prelu / erf-GELU, residual (post).  absolute=True: the same walk on magnitudes
    (an upper bound of |value| at every step; an activation multiplies by its Lipschitz constant:
    1, max(1, |slope|), or GELU's 1.13), the error scale S."""
    f = (lambda t: t.to(torch.float64).abs()) if absolute else (lambda t: t.to(torch.float64))
    v = v.to(torch.float64)
    if res is not None:
        r = f(res)
        if res_up2:
            r = up2(r)
    if bias is not None:
        v = v + f(bias)
    if alpha is not None:
        v = v * f(alpha) + f(beta)
    if scale != 1.0:
        v = v * abs(scale) if absolute else v * scale
    if res is not None and not res_post:
        v = v + r
    if absolute:
        # Lipschitz constants of the activations (all map 0 to 0)
        if leaky:
            v = v * max(1.0, abs(slope))
        if prelu is not None:
            v = v * f(prelu).clamp_min(1.0)
        if gelu:
            v = v * 1.13
    else:
        if relu:
            v = v.clamp_min(0)
        if leaky:
            v = torch.where(v > 0, v, v * slope)
        if prelu is not None:
            v = torch.where(v > 0, v, v * f(prelu))
        if gelu:
            v = 0.5 * v * (1.0 + torch.erf(v * (1.0 / math.sqrt(2.0))))
    if res is not None and res_post:
        v = v + r
    return v


def route(v, out, out_coff=0, upsample=False, n_split=0, out2=None, out2_coff=0):
    """Write v [N,OH,OW,Cout] into copies of the pre-filled buffers: channels [0, n_split or Cout)
    to out[..., out_coff:], the rest to out2[..., out2_coff:]; upsample = the up2 replication.
    Returns (out, out2)."""
    out = out.clone().to(torch.float64)
    if upsample:
        v = up2(v)
    C = v.shape[-1]
    n1 = n_split if n_split else C
    out[..., out_coff:out_coff + n1] = v[..., :n1]
    if n_split:
        out2 = out2.clone().to(torch.float64)
        out2[..., out2_coff:out2_coff + C - n1] = v[..., n1:]
    return out, out2


def pool_out_size(L, k, s):
    o = -((L - k) // -s) + 1  # ceil((L - k) / s) + 1
    if (o - 1) * s >= L:
        o -= 1
    return o


def maxpool_ceil(v, k, s):
    """MaxPool2d(k, s, ceil_mode=True), no padding, on [N,H,W,C]: windows clipped at the border."""
    N, H, W, C = v.shape
    OH, OW = pool_out_size(H, k, s), pool_out_size(W, k, s)
    out = torch.empty((N, OH, OW, C), dtype=v.dtype, device=v.device)
    for oy in range(OH):
        for ox in range(OW):
            out[:, oy, ox] = v[:, oy * s:min(oy * s + k, H), ox * s:min(ox * s + k, W)].amax(dim=(1, 2))
    return out


# ---- the two deliberate faults of the looseness guard (applied to the accumulator) ----------
def fault_dropped_chunk(x, w, stride, pad, n=0, oh=0, ow=0, tap=None, chunk=0):
    """The change of conv2d's output row (n, oh, ow) [Cout] when one 8-channel chunk of one tap is
    read as zero.  tap defaults to the centre tap (always inside the image for pad <= k // 2)."""
    Cout, KH, KW, Cin = w.shape
    kh, kw = tap if tap is not None else (KH // 2, KW // 2)
    ih, iw = oh * stride[0] - pad[0] + kh, ow * stride[1] - pad[1] + kw
    assert 0 <= ih < x.shape[1] and 0 <= iw < x.shape[2]
    c = slice(8 * chunk, 8 * chunk + 8)
    return -(w[:, kh, kw, c].to(torch.float64) @ x[n, ih, iw, c].to(torch.float64))


def fault_clamped_border(x, w, stride, pad):
    """The change of output row (0, 0, 0) when its padded corner tap (0, 0) reads the clamped
    neighbour pixel (0, 0) instead of zero (pad > 0 in both directions, or in the one padded)."""
    Cout, KH, KW, Cin = w.shape
    assert pad[0] > 0 or pad[1] > 0
    return w[:, 0, 0, :].to(torch.float64) @ x[0, 0, 0, :Cin].to(torch.float64)
