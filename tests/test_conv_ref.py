"""CPU: tests/conv_ref.py (the float64 reference the conv-engine GPU tests rest on) against
torch.nn.functional conv2d / max_pool2d / interpolate in float64, at small shapes that cover
every option of the reference."""
import pytest
import torch
import torch.nn.functional as F

import conv_ref as cr


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


# N, H, W, Cin, Cout, KH, KW, stride, pad, extra input channels (in_cstride - Cin)
CONV_SHAPES = [
    (1, 1, 1, 8, 8, 1, 1, (1, 1), (0, 0), 0),
    (2, 5, 7, 8, 15, 3, 3, (1, 1), (1, 1), 0),
    (1, 9, 6, 16, 18, 1, 7, (1, 1), (0, 3), 0),
    (1, 6, 9, 16, 8, 7, 1, (1, 1), (3, 0), 0),
    (3, 7, 9, 8, 40, 3, 3, (2, 2), (1, 1), 0),
    (2, 8, 5, 8, 24, 3, 3, (2, 1), (2, 2), 8),
    (1, 6, 6, 24, 72, 2, 2, (1, 1), (0, 0), 16),
    (2, 11, 13, 8, 16, 5, 3, (3, 2), (2, 0), 0),
]


@pytest.mark.parametrize('case', CONV_SHAPES)
def test_conv2d_matches_torch(case):
    N, H, W, Cin, Cout, KH, KW, stride, pad, extra = case
    x = _rand((N, H, W, Cin + extra), 1)
    w = _rand((Cout, KH, KW, Cin), 2)
    got = cr.conv2d(x, w, stride, pad)
    ref = _nhwc(F.conv2d(_nchw(x[..., :Cin]), w.permute(0, 3, 1, 2), stride=stride, padding=pad))
    assert got.shape == ref.shape == (N, cr.out_size(H, KH, stride[0], pad[0]), cr.out_size(W, KW, stride[1], pad[1]), Cout)
    torch.testing.assert_close(got, ref, rtol=0, atol=1e-12)


def _torch_epilogue(v, o):
    """The same epilogue written with torch.nn.functional building blocks on NCHW."""
    v = _nchw(v)
    ch = lambda t: t.view(1, -1, 1, 1)  # noqa: E731
    res = None
    if o.get('res') is not None:
        res = _nchw(o['res'])
        if o.get('res_up2'):
            res = F.interpolate(res, scale_factor=2, mode='nearest')
    if o.get('bias') is not None:
        v = v + ch(o['bias'])
    if o.get('alpha') is not None:
        v = v * ch(o['alpha']) + ch(o['beta'])
    v = v * o.get('scale', 1.0)
    if res is not None and not o.get('res_post'):
        v = v + res
    if o.get('relu'):
        v = F.relu(v)
    if o.get('leaky'):
        v = F.leaky_relu(v, o['slope'])
    if o.get('prelu') is not None:
        v = F.prelu(v, o['prelu'])
    if o.get('gelu'):
        v = F.gelu(v)
    if res is not None and o.get('res_post'):
        v = v + res
    return _nhwc(v)


N_, OH_, OW_, C_ = 2, 4, 6, 16
EPILOGUES = {
    'plain': {},
    'bias': dict(bias=_rand((C_,), 3)),
    'bn_scale': dict(alpha=_rand((C_,), 4), beta=_rand((C_,), 5), scale=0.17),
    'relu': dict(relu=True),
    'leaky': dict(leaky=True, slope=0.1),
    'prelu': dict(prelu=_rand((C_,), 6)),
    'gelu': dict(gelu=True),
    'res_pre': dict(bias=_rand((C_,), 7), scale=0.2, res=_rand((N_, OH_, OW_, C_), 8), relu=True),
    'res_post': dict(alpha=_rand((C_,), 9), beta=_rand((C_,), 10), res=_rand((N_, OH_, OW_, C_), 11), res_post=True,
                     leaky=True, slope=0.1),
    'res_up2': dict(res=_rand((N_, OH_ // 2, OW_ // 2, C_), 12), res_up2=True, relu=True),
    'res_up2_post': dict(res=_rand((N_, OH_ // 2, OW_ // 2, C_), 13), res_up2=True, res_post=True, gelu=True),
}


@pytest.mark.parametrize('name', sorted(EPILOGUES))
def test_epilogue_matches_torch(name):
    o = EPILOGUES[name]
    v = _rand((N_, OH_, OW_, C_), 20)
    torch.testing.assert_close(cr.epilogue(v, **o), _torch_epilogue(v, o), rtol=0, atol=1e-12)
    # the magnitude walk bounds the value walk at every element
    S = cr.epilogue(v.abs(), absolute=True, **o)
    assert bool((S + 1e-12 >= cr.epilogue(v, **o).abs()).all())


def test_route_slices_and_upsample():
    v = _rand((2, 3, 5, 24), 30)
    out = torch.full((2, 3, 5, 40), 7.0, dtype=torch.float64)
    got, _ = cr.route(v, out, out_coff=8)
    assert bool((got[..., :8] == 7).all()) and bool((got[..., 32:] == 7).all())
    torch.testing.assert_close(got[..., 8:32], v, rtol=0, atol=0)
    # n_split: the channels from n_split on go to out2 at out2_coff
    out2 = torch.full((2, 3, 5, 16), -3.0, dtype=torch.float64)
    got, got2 = cr.route(v, out, out_coff=16, n_split=16, out2=out2, out2_coff=8)
    torch.testing.assert_close(got[..., 16:32], v[..., :16], rtol=0, atol=0)
    torch.testing.assert_close(got2[..., 8:16], v[..., 16:], rtol=0, atol=0)
    assert bool((got[..., :16] == 7).all()) and bool((got[..., 32:] == 7).all()) and bool((got2[..., :8] == -3).all())
    # up2 = F.interpolate(scale_factor=2) nearest, into a slice of a (2 OH, 2 OW) buffer
    big = torch.zeros((2, 6, 10, 32), dtype=torch.float64)
    got, _ = cr.route(v, big, out_coff=8, upsample=True)
    ref = _nhwc(F.interpolate(_nchw(v), scale_factor=2, mode='nearest'))
    torch.testing.assert_close(got[..., 8:], ref, rtol=0, atol=0)
    assert bool((got[..., :8] == 0).all())


@pytest.mark.parametrize('H,W,k,s', [(4, 4, 2, 2), (5, 5, 2, 2), (9, 9, 3, 2), (10, 7, 3, 2), (22, 22, 3, 2), (21, 21, 2, 2),
                                     (3, 8, 3, 2)])
def test_maxpool_ceil_matches_torch(H, W, k, s):
    v = _rand((2, H, W, 8), 40)
    ref = _nhwc(F.max_pool2d(_nchw(v), k, s, ceil_mode=True))
    got = cr.maxpool_ceil(v, k, s)
    assert got.shape == ref.shape
    torch.testing.assert_close(got, ref, rtol=0, atol=0)


def test_faults_are_what_they_say():
    """The looseness guard's two faults against a conv recomputed with the fault built in."""
    x, w = _rand((1, 5, 6, 16), 50), _rand((8, 3, 3, 16), 51)
    good = cr.conv2d(x, w, (1, 1), (1, 1))
    # output (0, 2, 3): the centre tap reads pixel (2, 3); zero its channels 8..15
    xz = x.clone()
    xz[0, 2, 3, 8:16] = 0
    wz = w.clone()
    wz[:, 0, :, :] = 0
    wz[:, 2, :, :] = 0
    wz[:, 1, 0, :] = 0
    wz[:, 1, 2, :] = 0  # only the centre tap: the zeroed pixel is seen by that tap alone
    d = cr.fault_dropped_chunk(x, w, (1, 1), (1, 1), 0, 2, 3, chunk=1)
    torch.testing.assert_close(d, (cr.conv2d(xz, wz, (1, 1), (1, 1)) - cr.conv2d(x, wz, (1, 1), (1, 1)))[0, 2, 3], rtol=0,
                               atol=1e-12)
    # replicate padding instead of zeros changes output (0, 0, 0) through tap (0, 0) by w[:,0,0] . x[0,0,0]
    w00 = torch.zeros_like(w)
    w00[:, 0, 0, :] = w[:, 0, 0, :]
    xr = _nhwc(F.pad(_nchw(x), (1, 1, 1, 1), mode='replicate'))
    bad = cr.conv2d(xr, w00, (1, 1), (0, 0))
    torch.testing.assert_close(cr.fault_clamped_border(x, w, (1, 1), (1, 1)), bad[0, 0, 0], rtol=0, atol=1e-12)
    assert float(good.abs().max()) > 0
