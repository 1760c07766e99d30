"""GPU: the implicit-GEMM conv engine (csrc/conv.hip, conv_dma.hip, conv_dev.hpp) kernel by kernel
through vtf_conv2d, against the float64 reference of tests/conv_ref.py (pinned to
torch.nn.functional by tests/test_conv_ref.py; computed here on the device in float64).

Every case names the kernel configuration it means to hit and asserts it on the plan vtf_conv2d
returns (kernel id, tile, whole tiles, slices per tail tile, split-K factor), so a shape that
lands on another branch fails.  Shapes that depend on the grid filling the chip are derived from
multi_processor_count.  Every case runs twice and must give identical bits (fixed slice order,
workspace reuse), and is checked with two kinds of data:

exact   inputs are integers in [-4, 4], weights in [-2, 2], epilogue terms small integers or
        powers of two: exact in bf16, in fp16 and in both split layouts, every partial sum below
        2^24, so every operand mode must equal the float64 reference bit for bit (rounded once to
        bf16 where the output is bf16).  Pre-filled channels outside the written slice must come
        back unchanged.

random  inputs N(0, 1), weights 0.05 N(0, 1).  |got - ref| <= rel * S + out_round, with
        S = sum |a||w| + |epilogue terms| (conv_ref.epilogue(absolute=True): the magnitude walk
        through the same epilogue, an activation counting with its Lipschitz constant).  The
        bounds are derived, u = 2^-24 being fp32's unit roundoff:
          fp32  rel = (K + 32) u.  A K-term fp32 sum errs by at most K u sum|a||w| whatever the
                order (MFMA chains, split-K slices); 32 covers the epilogue: at most 7 roundings
                (bias, fma, scale, residual, slope, two for GELU's products), erff within 4 ulp,
                the up to 16 slice additions of a split tile, and the final acc + accx.
          f16x, sp  rel = (K + 32) u + 3 * 2^-22.  x is carried as x0 + x1 2^-11 with x0 = fp16(x)
                (|x - x0| <= 2^-11 |x|) and x1 = fp16((x - x0) 2^11) (relative 2^-11 again): each
                operand is off by 2^-22 relative, and the product x1 w1 2^-22 is dropped: three
                terms of 2^-22 |x||w| per product.  (fp16 parts below 2^-14 are subnormal with an
                absolute step of 2^-25: that adds at most K 2^-36 (max|x| + max|w|), included as
                an absolute term.)  The GEMM test's 2e-6 is this bound at K ~ 100.
          s3    rel = (K + 32) u + 3 u.  b0 + b1 + b2 is exact; the three products b1 w2, b2 w1,
                b2 w2 (each <= 2^-8 2^-16 |x||w|) are dropped.
          bf16  the reference is computed on bf16-rounded operands (products of two bf16 are exact
                in fp32), so rel = (K + 32) u.
        out_round is the one rounding of the stored value: half a bf16 ulp of ref for a bf16 output,
        2^-22 |ref| for a split-pair output, 0 for fp32 and split triples.  bf16 carries 8
        significant bits, so half an ulp of a value in [2^e, 2^(e+1)) is 2^(e-8): between 2^-9 |ref|
        (top of the binade) and 2^-8 |ref| (bottom).  A flat 2^-9 |ref| is not a bound of a correct
        round-to-nearest (1.0039 stores as 1.0: 2^-8.04 relative), so the half ulp itself is used.
        Measured worst |got - ref| / (rel S + out_round) per mode is printed (DESIGN.md records it).

looseness guard (random data, on the reference alone): the reference with one 8-channel chunk of
one tap read as zero in one output row, and with one padded corner tap reading its clamped
neighbour, must both violate the case's bound; otherwise the bound could not see such a fault.
"""
import ctypes
import os
import types
import zlib

import pytest
import torch

import conv_ref as cr

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
E_ARG = -1
# ConvKernel ids (include/vtf.h, `path`): id -> (BM, BN)
K_TILES = {1: (128, 32), 2: (128, 64), 3: (64, 32), 4: (64, 64), 5: (32, 32), 6: (32, 64)}
K_BK = {1: 32, 2: 32, 3: 64, 4: 64, 5: 64, 6: 64}
# id -> (mode, BM, BN, workgroups per CU, k per step)
DMA = {10: ('bf16', 256, 32, 2, 64), 11: ('bf16', 256, 64, 2, 64), 12: ('bf16', 128, 128, 2, 64),
       13: ('bf16', 64, 64, 3, 64), 20: ('sp', 128, 64, 3, 32), 21: ('sp', 128, 128, 2, 32),
       40: ('s3', 128, 64, 2, 32), 41: ('s3', 64, 128, 2, 32)}
SPAN, SPOOL = 30, 31
WORST = {}


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ------------------------------------------------------------------------------- the call
def conv2d(x, w, stride=(1, 1), pad=(0, 0), mode='fp32', path=0, out=None, **o):
    """vtf_conv2d on CUDA fp32 tensors x [N,H,W,ics], w [Cout,KH,KW,Cin]; `out` is the pre-filled
    buffer (written in place).  Returns rc, ovf, plan and the buffers."""
    from videotofaces import _native as nat
    N, H, W, ics = x.shape
    Cout, KH, KW, Cin = w.shape
    op = nat.Conv2dOpts()
    op.scale = 1.0
    keep = []
    fields = {f[0] for f in nat.Conv2dOpts._fields_}
    for k, v in o.items():
        assert k in fields, k
        if isinstance(v, torch.Tensor):
            assert v.is_cuda and v.dtype == torch.float32 and v.is_contiguous()
            keep.append(v)
            v = v.data_ptr()
        setattr(op, k, v)
    op.mode = nat.CONV_MODES[mode]
    op.path = path
    if ics != Cin:
        op.in_cstride = ics
    if out is not None and not op.out_cstride:
        op.out_cstride = out.shape[-1]
    ovf = ctypes.c_int32(-1)
    plan = (ctypes.c_int32 * 8)(*([-1] * 8))
    assert x.is_contiguous() and w.is_contiguous() and (out is None or out.is_contiguous())
    rc = nat.lib().vtf_conv2d(x.data_ptr(), w.data_ptr(), N, H, W, Cin, Cout, KH, KW, stride[0], stride[1], pad[0],
                              pad[1], ctypes.byref(op), out.data_ptr() if out is not None else None,
                              ctypes.byref(ovf), plan, torch.cuda.current_stream().cuda_stream)
    return types.SimpleNamespace(rc=rc, ovf=ovf.value, plan=list(plan), out=out, out2=o.get('out2'),
                                 pool=o.get('pool_out'))


# ------------------------------------------------------------------------------- data
def _ints(gen, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


def _prefill(shape):
    n = 1
    for s in shape:
        n *= s
    return ((torch.arange(n) % 13) - 6).float().reshape(shape)  # exact in bf16 and in both split layouts


EPI = {
    'plain': {},
    'bias': dict(bias=1),
    'relu': dict(bias=1, relu=1),
    'leaky': dict(bias=1, leaky=1),
    'prelu': dict(bias=1, prelu=1),
    'gelu': dict(bias=1, gelu=1),
    'bn_res_pre': dict(bn=1, scale=1, res=1, relu=1),
    'bn_res_post': dict(bn=1, scale=1, res=1, res_post=1, leaky=1),
    'res_up2': dict(bias=1, res=1, res_up2=1, relu=1),
}


def _make(c, data):
    """Inputs, options and the float64 reference (values, allowed error, fault deltas) of case c."""
    gen = torch.Generator().manual_seed(zlib.crc32(repr(sorted(c.items(), key=str)).encode()) & 0x7fffffff)
    exact = data == 'exact'
    N, H, W, Cin, Cout = c['N'], c['H'], c['W'], c['Cin'], c['Cout']
    KH, KW = c.get('k', (1, 1))
    stride, pad = c.get('stride', (1, 1)), c.get('pad', (0, 0))
    mode = c['mode']
    ics = Cin + c.get('in_extra', 0)
    OH, OW = cr.out_size(H, KH, stride[0], pad[0]), cr.out_size(W, KW, stride[1], pad[1])
    e = EPI[c.get('epi', 'plain')]
    if exact:
        x, w = _ints(gen, (N, H, W, ics), -4, 4), _ints(gen, (Cout, KH, KW, Cin), -2, 2)
    else:
        x, w = torch.randn((N, H, W, ics), generator=gen), 0.05 * torch.randn((Cout, KH, KW, Cin), generator=gen)
    o, eo = {}, {}
    if e.get('bias'):
        o['bias'] = _ints(gen, (Cout,), -8, 8) if exact else torch.randn((Cout,), generator=gen)
    if e.get('bn'):
        o['alpha'] = (_ints(gen, (Cout,), 0, 1) * 3 - 1) if exact else 1 + 0.1 * torch.randn((Cout,), generator=gen)
        o['beta'] = _ints(gen, (Cout,), -8, 8) if exact else torch.randn((Cout,), generator=gen)
    if e.get('scale'):
        o['scale'] = 0.5 if exact else 0.17000000178813934  # (float)0.17
    if e.get('res'):
        rs = (N, OH // 2, OW // 2, Cout) if e.get('res_up2') else (N, OH, OW, Cout)
        o['res'] = _ints(gen, rs, -16, 16) if exact else torch.randn(rs, generator=gen)
    if e.get('prelu'):
        o['prelu'] = (_ints(gen, (Cout,), 1, 2) * 0.25) if exact else 0.25 + 0.1 * torch.rand((Cout,), generator=gen)
    if e.get('leaky'):
        o['leaky'], o['slope'] = 1, (0.5 if exact else 0.10000000149011612)  # (float)0.1
    for f in ('relu', 'gelu', 'res_post', 'res_up2'):
        if e.get(f):
            o[f] = 1
    for f in ('up2', 'out_coff', 'n_split', 'out2_coff', 'out_f32', 'split_fp32', 'out_sp'):
        if c.get(f):
            o[f] = c[f]
    ocs = c.get('out_cstride', Cout)
    o['out_cstride'] = ocs
    up = 2 if c.get('up2') else 1
    out0 = _prefill((N, OH * up, OW * up, ocs))
    out20 = None
    if c.get('n_split'):
        o['out2_cstride'] = c['out2_cstride']
        out20 = _prefill((N, OH, OW, c['out2_cstride'])) + 1
    dev = 'cuda'
    x, w, out0 = x.to(dev), w.to(dev), out0.to(dev)
    o = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in o.items()}
    if out20 is not None:
        out20 = out20.to(dev)

    # ---- the reference, float64 on the device
    rnd = (lambda t: t.to(torch.bfloat16).to(torch.float64)) if mode == 'bf16' else (lambda t: t.to(torch.float64))
    xr, wr = rnd(x), rnd(w)
    eo = {k: o[k] for k in ('bias', 'alpha', 'beta', 'prelu') if k in o}
    for f in ('relu', 'leaky', 'gelu', 'res_post', 'res_up2'):
        eo[f] = bool(o.get(f))
    eo['scale'], eo['slope'] = o.get('scale', 1.0), o.get('slope', 0.0)
    if 'res' in o:
        eo['res'] = rnd(o['res'])
    acc = cr.conv2d(xr, wr, stride, pad)
    S = cr.epilogue(cr.conv2d(xr.abs(), wr.abs(), stride, pad), absolute=True, **eo)
    rt = dict(out_coff=c.get('out_coff', 0), upsample=bool(c.get('up2')), n_split=c.get('n_split', 0),
              out2_coff=c.get('out2_coff', 0))

    def routed(v, base, base2):
        return cr.route(v, base, out2=base2, **rt)

    ref, ref2 = routed(cr.epilogue(acc, **eo), out0, out20)
    K = KH * KW * Cin
    rel = (K + 32) * U + {'fp32': 0.0, 'bf16': 0.0, 'f16x': 3 * 2.0 ** -22, 'sp': 3 * 2.0 ** -22, 's3': 3 * U}[mode]
    bf16_out = mode == 'bf16' and not c.get('out_f32')

    def out_round(t):
        if bf16_out:  # half a bf16 ulp: |t| = m 2^e with m in [0.5, 1) -> ulp 2^(e - 8)
            return torch.ldexp(torch.full_like(t, 0.5), torch.frexp(t)[1] - 8) * (t != 0)
        return 2.0 ** -22 * t.abs() if c.get('out_sp') else torch.zeros_like(t)
    sub = 0.0
    if mode in ('f16x', 'sp'):
        amp = float(S.max() / cr.conv2d(xr.abs(), wr.abs(), stride, pad).max().clamp_min(1e-30))  # epilogue gain
        sub = K * 2.0 ** -36 * float(xr.abs().max() + wr.abs().max()) * max(1.0, amp)
    z, z2 = torch.zeros_like(out0, dtype=torch.float64), None if out20 is None else torch.zeros_like(out20, dtype=torch.float64)
    allow, allow2 = routed(rel * S + sub, z, z2)  # zero outside the written slice: untouched channels are exact
    allow = allow + out_round(ref) * (allow > 0)
    if allow2 is not None:
        allow2 = allow2 + out_round(ref2) * (allow2 > 0)

    # ---- the looseness guard's faulty references (row (0, 0, 0) of the accumulator)
    faulty = []
    if not exact:
        # the first output row whose tap (0, 0) lies inside the image loses that tap's last chunk;
        # output (0, 0, 0) reads its padded corner tap from the clamped neighbour
        fo = (-(-pad[0] // stride[0]), -(-pad[1] // stride[1]))
        deltas = [(fo, cr.fault_dropped_chunk(xr, wr, stride, pad, 0, fo[0], fo[1], tap=(0, 0), chunk=(Cin // 8) - 1))]
        if pad[0] or pad[1]:
            deltas.append(((0, 0), cr.fault_clamped_border(xr, wr, stride, pad)))
        for (fy, fx), dl in deltas:
            bad = acc.clone()
            bad[0, fy, fx] += dl
            faulty.append(routed(cr.epilogue(bad, **eo), out0, out20))
    return types.SimpleNamespace(x=x, w=w, o=o, out0=out0, out20=out20, ref=ref, ref2=ref2, allow=allow, allow2=allow2,
                                 faulty=faulty, stride=stride, pad=pad, mode=mode, bf16_out=bf16_out, exact=exact)


def _launch(c, d):
    o = dict(d.o)
    out = d.out0.clone()
    if d.out20 is not None:
        o['out2'] = d.out20.clone()
    return conv2d(d.x, d.w, d.stride, d.pad, d.mode, c.get('path', 0), out, **o)


def _check_plan(r, expect):
    names = ['kernel', 'BM', 'BN', 'dp_tiles', 'tail_split', 'split', 'parts', 'cg']
    got = dict(zip(names, r.plan))
    for k, v in expect.items():
        assert got[k] == v, ('plan', k, got, expect)


def _compare(d, got, ref, allow, label):
    if d.exact:
        want = ref.to(torch.float32)
        if d.bf16_out:
            want = want.to(torch.bfloat16).to(torch.float32)
        assert torch.equal(got, want), (label, 'max abs diff', float((got.double() - want.double()).abs().max()))
        return
    err = (got.to(torch.float64) - ref).abs()
    assert bool(torch.isfinite(got).all())
    assert bool((err[allow == 0] == 0).all()), (label, 'a channel outside the written slice changed')
    m = allow > 0
    worst = float((err[m] / allow[m]).max())
    key = d.mode + ('/bf16 out' if d.bf16_out else '')
    WORST[key] = max(WORST.get(key, 0.0), worst)
    print('%s %s: worst |got - ref| / allowed = %.4f (worst so far for %s: %.4f)' % (label, d.mode, worst, key, WORST[key]))
    assert worst <= 1.0, (label, worst)


def run_case(c, data):
    d = _make(c, data)
    r1 = _launch(c, d)
    assert r1.rc == 0, r1.rc
    _check_plan(r1, c['expect'])
    assert r1.ovf == 0
    r2 = _launch(c, d)
    assert r2.rc == 0 and r2.plan == r1.plan
    assert torch.equal(r1.out, r2.out), 'two runs differ'
    _compare(d, r1.out, d.ref, d.allow, 'out')
    if d.out20 is not None:
        assert torch.equal(r1.out2, r2.out2)
        _compare(d, r1.out2, d.ref2, d.allow2, 'out2')
    for bad, bad2 in d.faulty:  # the looseness guard
        viol = bool(((bad - d.ref).abs() > d.allow).any())
        if bad2 is not None:
            viol = viol or bool(((bad2 - d.ref2).abs() > d.allow2).any())
        assert viol, 'the bound would not see a dropped chunk / a clamped border tap'


def _params(cases):
    ps = []
    for name, c in cases.items():
        for data in ('exact', 'random'):
            if data == 'exact' and 'gelu' in c.get('epi', ''):
                continue
            ps.append(pytest.param(name, data, id='%s-%s' % (name, data)))
    return ps


# ------------------------------------------------------------------------------- k_conv
def _kconv_cases():
    cs = {}
    for path, modes in ((1, ('fp32', 'f16x')), (2, ('fp32', 'f16x')), (3, ('bf16',)), (4, ('bf16',)), (5, ('bf16',)),
                        (6, ('bf16',))):
        BM, BN = K_TILES[path]
        ex = dict(kernel=path, BM=BM, BN=BN, split=1)
        for mode in modes:
            t = 'k%dx%d-%s-' % (BM, BN, mode)
            base = dict(mode=mode, path=path, expect=ex)
            # M = 1 and K = 8 < BK
            cs[t + 'm1'] = dict(base, N=1, H=1, W=1, Cin=8, Cout=8)
            # M < BM, K = 72 (a K tail), Cout = 15 (scalar epilogue)
            cs[t + 'm_lt_bm'] = dict(base, N=1, H=3, W=5, Cin=8, Cout=15, k=(3, 3), pad=(1, 1))
            # M = 2 BM + 1, K = 40, Cout = 18
            cs[t + 'm_qbm1'] = dict(base, N=1, H=1, W=2 * BM + 1, Cin=40, Cout=18, epi='bias')
            # three images of 63 pixels: tiles straddle images; Cout = 40
            cs[t + 'straddle'] = dict(base, N=3, H=7, W=9, Cin=16, Cout=40, k=(3, 3), pad=(1, 1), epi='relu')
            cs[t + '1x7'] = dict(base, N=2, H=5, W=11, Cin=8, Cout=72, k=(1, 7), pad=(0, 3))
            cs[t + '7x1'] = dict(base, N=2, H=11, W=5, Cin=8, Cout=8, k=(7, 1), pad=(3, 0))
            cs[t + 'pad2'] = dict(base, N=1, H=6, W=7, Cin=8, Cout=40, k=(3, 3), pad=(2, 2))
            cs[t + 'stride2'] = dict(base, N=2, H=9, W=11, Cin=16, Cout=24, k=(3, 3), stride=(2, 2), pad=(1, 1))
    # layout and epilogue branches: one fp32, one f16x and two bf16 tiles
    for path, mode in ((2, 'fp32'), (1, 'f16x'), (4, 'bf16'), (5, 'bf16')):
        BM, BN = K_TILES[path]
        t = 'k%dx%d-%s-' % (BM, BN, mode)
        g = dict(mode=mode, path=path, expect=dict(kernel=path, split=1), N=3, H=6, W=8, Cin=16, Cout=40, k=(3, 3), pad=(1, 1))
        cs[t + 'in_cstride'] = dict(g, in_extra=8)
        cs[t + 'concat'] = dict(g, Cout=16, out_cstride=40, out_coff=8, epi='bias')
        cs[t + 'concat_scalar'] = dict(g, Cout=15, out_cstride=21, out_coff=3, epi='bias')
        cs[t + 'n_split'] = dict(g, n_split=16, out_cstride=24, out_coff=8, out2_cstride=32, out2_coff=8, epi='relu')
        cs[t + 'n_split_scalar'] = dict(g, n_split=16, out_cstride=19, out_coff=3, out2_cstride=27, out2_coff=3)
        for e in ('relu', 'leaky', 'prelu', 'gelu', 'bn_res_pre', 'bn_res_post', 'res_up2'):
            cs[t + e] = dict(g, epi=e)
        cs[t + 'bn_res_pre_scalar'] = dict(g, Cout=15, epi='bn_res_pre')
        cs[t + 'res_up2_scalar'] = dict(g, Cout=18, epi='res_up2')
        cs[t + 'up2'] = dict(g, up2=1, out_cstride=56, out_coff=16, epi='leaky')
        cs[t + 'up2_scalar'] = dict(g, Cout=15, up2=1, out_cstride=20, out_coff=5)
        if mode == 'bf16':
            cs[t + 'out_f32'] = dict(g, out_f32=1, epi='bias')
            cs[t + 'out_f32_scalar'] = dict(g, Cout=18, out_f32=1, epi='bias')
    # split-K: bf16 below 192 tiles with KT >= 8; fp32 / f16x with split_fp32 below 160 tiles
    sk = dict(N=1, H=10, W=13, Cin=512, Cout=72, epi='bn_res_post', out_cstride=88, out_coff=8)  # 3 x 2 tiles, KT = 8
    cs['k64x64-bf16-split_kt4_cap'] = dict(sk, mode='bf16', path=4, expect=dict(kernel=4, split=2))  # min(8, KT / 4 = 2)
    # 50 x 2 tiles, K = 2088 (KT = 33): ceil(512 / 100) = 6 slices
    cs['k64x64-bf16-split6'] = dict(N=2, H=40, W=40, Cin=232, Cout=72, k=(3, 3), pad=(1, 1), mode='bf16', path=4,
                                    epi='relu', expect=dict(kernel=4, split=6))
    cs['k32x32-bf16-split'] = dict(sk, mode='bf16', path=5, Cout=24, out_cstride=24, out_coff=0,
                                   expect=dict(kernel=5, split=2))
    sf = dict(N=3, H=10, W=10, Cin=512, Cout=72, epi='bn_res_pre')  # 3 x 2 tiles of 128 x 64, KT = 16: min(8, 16 / 4)
    for mode in ('fp32', 'f16x'):
        cs['k128x64-%s-split_fp32' % mode] = dict(sf, mode=mode, path=2, split_fp32=1, expect=dict(kernel=2, split=4))
        cs['k128x64-%s-no_split' % mode] = dict(sf, mode=mode, path=2, expect=dict(kernel=2, split=1))
    cs['k128x32-fp32-split_fp32'] = dict(sf, Cout=24, mode='fp32', path=1, split_fp32=1, expect=dict(kernel=1, split=4))
    return cs


KCONV = _kconv_cases()


@pytest.mark.parametrize('name,data', _params(KCONV))
def test_k_conv(name, data):
    run_case(KCONV[name], data)


def test_k_conv_auto_dispatch():
    """path 0 = launch_conv's own choice: fp32 by Cout; bf16 32-row tiles below 3 workgroups per
    CU, 64-row tiles above (K < 256 keeps bf16 on k_conv)."""
    big = 64 * 3 * _cus()
    for mode, Cout, M, kernel in (('fp32', 24, 50, 1), ('fp32', 40, 50, 2), ('f16x', 40, 50, 2), ('bf16', 24, 50, 5),
                                  ('bf16', 40, 50, 6), ('bf16', 24, big, 3), ('bf16', 40, big, 4)):
        BM, BN = K_TILES[kernel]
        c = dict(mode=mode, path=0, N=1, H=1, W=M, Cin=8, Cout=Cout, epi='bias',
                 expect=dict(kernel=kernel, BM=BM, BN=BN, split=1))
        run_case(c, 'exact')


def test_k_conv_split_workspace_growth():
    """A split call, a larger split call (the per-stream workspace grows), then an unsplit one,
    back to back on one stream: each exact."""
    for name in ('k64x64-bf16-split_kt4_cap', 'k64x64-bf16-split6', 'k64x64-bf16-straddle', 'k64x64-bf16-split_kt4_cap'):
        run_case(KCONV[name], 'exact')


@pytest.mark.parametrize('path', [1, 2])
def test_f16x_range_flag(path):
    """f16x: an operand of magnitude >= 2^14 raises ovf, 16383 does not (either operand)."""
    x = torch.ones((1, 4, 5, 8), device='cuda')
    w = torch.ones((16, 1, 1, 8), device='cuda')
    for xv, wv, want in ((16383.0, 1.0, 0), (16384.0, 1.0, 1), (-16384.0, 1.0, 1), (1.0, 16383.0, 0), (1.0, 16384.0, 1)):
        x[0, 3, 4, 7], w[15, 0, 0, 7] = xv, wv
        r = conv2d(x, w, mode='f16x', path=path, out=torch.zeros((1, 4, 5, 16), device='cuda'))
        assert r.rc == 0 and r.plan[0] == path and r.ovf == want, (xv, wv, r.ovf)
    r = conv2d(x, w, mode='fp32', path=path, out=torch.zeros((1, 4, 5, 16), device='cuda'))
    assert r.rc == 0 and r.ovf == 0  # the flag belongs to the split modes


# ------------------------------------------------------------------------------- k_conv_dma, k_conv_dma3
def _rows(gx, BM):
    """N = 2 images of H x 13 whose M = 26 H needs exactly gx row tiles, the last one partial
    (rows past M) and one straddling the two images."""
    H = ((gx - 1) * BM) // 26 + 1
    assert -(-26 * H // BM) == gx
    return dict(N=2, H=H, W=13)


def _factor(T, prefs):
    for gy in prefs:
        if T % gy == 0:
            return T // gy, gy
    return T, 1


def _dma_case(path, regime, cus):
    """Grid regimes of launch_dma_t / launch_dma3_t on `cus` CUs: 3x3 pad 1 convs of Cin = 56
    (K = 504: a K tail in the last k-step, padded corners, rows past M)."""
    mode, BM, BN, occ, KS = DMA[path]
    slots = occ * cus
    c = dict(mode=mode, path=path, Cin=56, k=(3, 3), pad=(1, 1))
    KT = -(-504 // KS)
    if mode != 'bf16':
        c['split_fp32'] = 1  # bf16 splits on its own; the fp32-grade modes when the caller allows it
    if regime == 'below':  # T = 6 < slots: every tile split, S = min(slots / T, KT / 4, 16); a Cout tail
        gx, gy = 3, 2
        S = min(slots // 6, KT // 4, 16)
        c.update(_rows(gx, BM), Cout=gy * BN - 8, epi='relu', out_cstride=gy * BN + 8, out_coff=8)
        ex = dict(dp_tiles=0, tail_split=S)
        assert S >= 2
    elif regime == 'cap16':  # one tile, KT / 4 = 18 (bf16) or 36: S capped at 16
        c.update(N=2, H=3, W=13, Cin=4608, k=(1, 1), pad=(0, 0), Cout=BN, epi='bias')
        ex = dict(dp_tiles=0, tail_split=16)
    elif regime == 'round':  # exactly one round: whole tiles only
        gx, gy = _factor(slots, (4, 2, 1))
        c.update(_rows(gx, BM), Cout=gy * BN)
        ex = dict(dp_tiles=slots, tail_split=1)
    elif regime == 'tail':  # one round + 3 tiles: those 3 run as min(slots / 3, KT / 4) slices each
        gx, gy = _factor(slots + 3, (5, 3, 2, 1))
        c.update(_rows(gx, BM), Cout=gy * BN, epi='bn_res_post')
        ex = dict(dp_tiles=slots, tail_split=min(slots // 3, KT // 4))
        assert ex['tail_split'] >= 2
    elif regime == 'wide':  # a remainder above half the slots: no split
        T = -(-(slots + slots // 2 + 1) // 4) * 4
        assert T < 2 * slots
        c.update(_rows(T // 4, BM), Cout=4 * BN)
        ex = dict(dp_tiles=T, tail_split=1)
    if mode == 'sp' and regime in ('below', 'tail'):
        c['out_sp'] = 1
    c['expect'] = dict(ex, kernel=path, BM=BM, BN=BN)
    return c


DMA_REGIMES = [(p, r) for p in (10, 11, 12, 13, 20, 21) for r in ('below', 'cap16', 'round', 'tail', 'wide')] + \
              [(p, r) for p in (40, 41) for r in ('below', 'round', 'tail', 'wide')]


@pytest.mark.parametrize('data', ['exact', 'random'])
@pytest.mark.parametrize('path,regime', DMA_REGIMES)
def test_conv_dma_grid_regimes(path, regime, data):
    run_case(_dma_case(path, regime, _cus()), data)


def _dma_small_cases():
    cs = {}
    g = dict(N=3, H=6, W=8, Cin=16, Cout=40, k=(3, 3), pad=(1, 1))
    for path in (13, 10, 12, 20, 21, 40, 41):
        mode, BM, BN = DMA[path][:3]
        t = 'dma%d-%s-' % (path, mode)
        b = dict(g, mode=mode, path=path, expect=dict(kernel=path, BM=BM, BN=BN, tail_split=1))
        cs[t + 'm1'] = dict(b, N=1, H=1, W=1, Cin=8, Cout=8, k=(1, 1), pad=(0, 0))
        cs[t + 'stride2_in_cstride'] = dict(b, N=2, H=9, W=11, stride=(2, 2), in_extra=8, epi='bias')
        cs[t + '1x7'] = dict(b, N=2, H=5, W=11, Cin=8, Cout=72, k=(1, 7), pad=(0, 3))
        cs[t + '7x1_pad2'] = dict(b, N=2, H=11, W=5, Cin=8, Cout=8, k=(7, 1), pad=(3, 2))
        cs[t + 'concat'] = dict(b, Cout=16, out_cstride=40, out_coff=8, epi='bias')
        for e in ('prelu', 'gelu', 'bn_res_pre', 'bn_res_post', 'res_up2'):
            cs[t + e] = dict(b, epi=e)
        cs[t + 'up2'] = dict(b, up2=1, out_cstride=56, out_coff=16, epi='leaky')
        if mode != 's3':
            cs[t + 'n_split'] = dict(b, n_split=16, out_cstride=24, out_coff=8, out2_cstride=32, out2_coff=8, epi='relu')
        if mode in ('bf16', 's3'):
            cs[t + 'out_f32'] = dict(b, out_f32=1, epi='bias')
        if mode == 'sp':
            cs[t + 'out_sp'] = dict(b, out_sp=1, out_cstride=48, out_coff=8, epi='prelu')
            cs[t + 'no_split_fp32'] = dict(b, Cin=128, expect=dict(kernel=path, dp_tiles=2 if BM == 128 else 1, tail_split=1))
            cs[t + 'split_fp32'] = dict(b, Cin=128, split_fp32=1, expect=dict(kernel=path, dp_tiles=0, tail_split=9))
    return cs


DMA_SMALL = _dma_small_cases()


@pytest.mark.parametrize('name,data', _params(DMA_SMALL))
def test_conv_dma_small(name, data):
    run_case(DMA_SMALL[name], data)


def test_conv_dma_auto_dispatch():
    """path 0: the split-pair and bf16x3 modes pick their tile by Cout; a bf16 conv of Cout = 192
    and K >= 256 on a grid of at least 2 tiles per CU takes the 256 x 64 tiles."""
    g = dict(N=3, H=6, W=8, Cin=16, k=(3, 3), pad=(1, 1), path=0, epi='bias')
    for mode, Cout, kernel in (('sp', 56, 20), ('sp', 72, 21), ('s3', 64, 40), ('s3', 72, 41)):
        run_case(dict(g, mode=mode, Cout=Cout, expect=dict(kernel=kernel, BM=DMA[kernel][1], BN=DMA[kernel][2])), 'exact')
    cus = _cus()
    T = (128 * cus // 256) * 3
    c = dict(mode='bf16', path=0, N=1, H=1, W=128 * cus, Cin=256, Cout=192, epi='relu',
             expect=dict(kernel=11, BM=256, BN=64, dp_tiles=T, tail_split=1))
    run_case(c, 'exact')
    run_case(c, 'random')


def test_split_pair_range_flags():
    """sp mode: an input >= 2^14 raises ovf in the packer; an out_sp value >= 2^14 raises it in the
    conv epilogue (whole tiles and the tail kernel); just below does not."""
    x = torch.zeros((1, 4, 5, 8), device='cuda')
    w = torch.ones((16, 1, 1, 8), device='cuda')
    for path in (20, 21):
        for split in (0, 1):
            xx = torch.zeros((1, 4, 5, 512), device='cuda') if split else x
            ww = torch.ones((16, 1, 1, 512), device='cuda') if split else w
            for b, want in ((16383.0, 0), (16384.0, 1), (-20000.0, 1)):
                bias = torch.zeros(16, device='cuda')
                bias[5] = b
                r = conv2d(xx, ww, mode='sp', path=path, out=torch.zeros((1, 4, 5, 16), device='cuda'), bias=bias,
                           out_sp=1, split_fp32=split)
                assert r.rc == 0 and r.plan[0] == path and (r.plan[4] > 1) == bool(split) and r.ovf == want, (path, b, r.plan)
                r = conv2d(xx, ww, mode='sp', path=path, out=torch.zeros((1, 4, 5, 16), device='cuda'), bias=bias,
                           split_fp32=split)
                assert r.rc == 0 and r.ovf == 0  # an fp32 output has no range
    x[0, 1, 2, 3] = 16384.0
    r = conv2d(x, w, mode='sp', path=20, out=torch.zeros((1, 4, 5, 16), device='cuda'))
    assert r.rc == 0 and r.ovf == 1


# ------------------------------------------------------------------------------- k_conv_span
SPAN_CASES = {
    'span-cin32-3x3': dict(N=7, H=10, W=10, Cin=32, Cout=48, k=(3, 3), epi='prelu'),
    'span-cin32-2x3-out_sp': dict(N=5, H=9, W=12, Cin=32, Cout=64, k=(2, 3), epi='prelu', out_sp=1),
    'span-cin64-3x3': dict(N=7, H=10, W=10, Cin=64, Cout=64, k=(3, 3), epi='bias'),
    'span-cin64-4x1-concat': dict(N=3, H=12, W=9, Cin=64, Cout=24, k=(4, 1), epi='relu', out_cstride=40, out_coff=16),
    'span-cin32-m1': dict(N=1, H=2, W=3, Cin=32, Cout=8, k=(2, 3)),
}


@pytest.mark.parametrize('name,data', _params(SPAN_CASES))
def test_conv_span(name, data):
    """k_conv_span (auto dispatch of the split-pair mode on stride-1 unpadded Cin 32 / 64 convs,
    KH KW >= 4, odd KW) against the reference, and bit for bit against the implicit-GEMM gather:
    the forced 128 x 64 MODE 1 tiles and the VTF_CONV_SPAN=0 dispatch (neither splits K here)."""
    c = dict(SPAN_CASES[name], mode='sp', path=0)
    BMs = -(-(c['N'] * (c['H'] - c['k'][0] + 1) * (c['W'] - c['k'][1] + 1)) // 128)
    c['expect'] = dict(kernel=SPAN, BM=128, BN=64, dp_tiles=BMs, tail_split=1)
    run_case(c, data)
    d = _make(c, data)
    span = _launch(c, d)
    gather = _launch(dict(c, path=20), d)
    assert gather.rc == 0 and gather.plan[0] == 20 and gather.plan[4] == 1
    assert torch.equal(span.out, gather.out)
    forced = _launch(dict(c, path=SPAN), d)
    assert forced.rc == 0 and forced.plan[0] == SPAN and torch.equal(span.out, forced.out)
    os.environ['VTF_CONV_SPAN'] = '0'
    try:
        env = _launch(c, d)
    finally:
        del os.environ['VTF_CONV_SPAN']
    assert env.rc == 0 and env.plan[0] == 20 and torch.equal(span.out, env.out)


def test_conv_span_refuses_what_does_not_fit():
    """path = k_conv_span on a conv it cannot run (padding, even KW, 16 input channels): an
    error, nothing launched."""
    for kw in (dict(Cin=32, k=(3, 3), pad=(1, 1)), dict(Cin=32, k=(2, 2)), dict(Cin=16, k=(3, 3))):
        x = torch.ones((2, 8, 8, kw['Cin']), device='cuda')
        w = torch.ones((16,) + kw['k'] + (kw['Cin'],), device='cuda')
        out = torch.full((2, 8, 8, 16), 3.0, device='cuda')
        r = conv2d(x, w, pad=kw.get('pad', (0, 0)), mode='sp', path=SPAN, out=out)
        assert r.rc == E_ARG and r.plan == [0] * 8 and bool((out == 3).all())


# ------------------------------------------------------------------------------- k_conv_span_pool
#   name: N, H, Cout, conv k, pool k -> parts, cg   (Cin = 32, stride-2 pool)
SPOOL_CASES = {
    'rnet-cg3-k3': (7, 11, 48, 3, 3, 1, 3),           # OH = 9: 3 images per tile, 7 = 2 tiles + 1; Cout <= 48
    'cg3-k2-partial': (7, 11, 64, 3, 2, 1, 3),         # OH = 9, k = 2: ceil_mode adds a 1-wide window; Cout > 48
    'cg2-k3-partial': (5, 12, 48, 3, 3, 1, 2),         # OH = 10, k = 3: a 2-wide last window; N = 2 tiles + 1
    'onet-parts2-k3': (3, 23, 64, 3, 3, 2, 1),         # OH = 21: two bands per image
    'parts2-k2-cout40': (2, 19, 40, 2, 2, 2, 1),       # a 2 x 3 conv (KW must be odd): OH x OW = 18 x 17, two bands
}


@pytest.mark.parametrize('name', sorted(SPOOL_CASES))
@pytest.mark.parametrize('data', ['exact', 'random'])
def test_conv_span_pool(name, data):
    """The fused conv + MaxPool2d(k, 2, ceil_mode) against pool(reference conv) within the
    split-pair bound, and bit for bit against the unfused conv + launch_maxpool_ks_sp."""
    N, H, Cout, ck, pk, parts, cg = SPOOL_CASES[name]
    kk = (ck, ck) if ck % 2 else (ck, 3)
    c = dict(N=N, H=H, W=H, Cin=32, Cout=Cout, k=kk, mode='sp', epi='prelu')
    d = _make(c, data)
    OH, OW = H - kk[0] + 1, H - kk[1] + 1
    POH, POW = cr.pool_out_size(OH, pk, 2), cr.pool_out_size(OW, pk, 2)
    if 'partial' in name:
        assert (POH - 1) * 2 + pk > OH  # ceil_mode's clipped last window
    runs = []
    for fused in (1, 1, 0):
        pool = _prefill((N, POH, POW, Cout)).cuda()
        r = conv2d(d.x, d.w, mode='sp', out=None if fused else d.out0.clone(), pool_out=pool, pool_k=pk, pool_s=2,
                   pool_fused=fused, **d.o)
        assert r.rc == 0 and r.ovf == 0
        runs.append(r)
    _check_plan(runs[0], dict(kernel=SPOOL, parts=parts, cg=cg, dp_tiles=-(-N // cg) if parts == 1 else N * parts))
    assert runs[2].plan[0] in (20, SPAN) and runs[2].plan[4] == 1
    assert torch.equal(runs[0].pool, runs[1].pool), 'two runs differ'
    assert torch.equal(runs[0].pool, runs[2].pool), 'fused and unfused pooled maps differ'
    ref = cr.maxpool_ceil(d.ref, pk, 2)
    allow = cr.maxpool_ceil(d.allow, pk, 2) + 2.0 ** -22 * ref.abs()  # |max a - max b| <= max |a - b|; split-pair store
    _compare(types.SimpleNamespace(exact=d.exact, bf16_out=False, mode='sp'), runs[0].pool, ref, allow, 'pooled')
    if not d.exact:  # looseness guard through the pool: the faulty row must surface in some pooled value
        for bad, _ in d.faulty:
            assert bool(((cr.maxpool_ceil(bad, pk, 2) - ref).abs() > allow).any()) or \
                bool(((bad - d.ref).abs() > d.allow).any())


def test_conv_span_pool_refuses():
    """Shapes the fused kernel cannot take return false: nothing launched, the plan is empty and
    the pooled buffer untouched."""
    for N, H, W, Cin, kk in ((1, 9, 100, 32, (3, 3)),   # a 98-wide conv row: no band of <= 256 rows holds a pool row
                             (2, 11, 11, 64, (3, 3)),   # 64 input channels
                             (2, 11, 11, 32, (2, 2))):  # even KW
        x = torch.ones((N, H, W, Cin), device='cuda')
        w = torch.ones((16,) + kk + (Cin,), device='cuda')
        OH, OW = H - kk[0] + 1, W - kk[1] + 1
        pool = torch.full((N, cr.pool_out_size(OH, 3, 2), cr.pool_out_size(OW, 3, 2), 16), 5.0, device='cuda')
        r = conv2d(x, w, mode='sp', out=None, pool_out=pool, pool_k=3, pool_s=2, pool_fused=1, out_cstride=16)
        assert r.rc == 0 and r.plan == [0] * 8 and bool((pool == 5).all())


# ------------------------------------------------------------------------------- refusals
def _refused(r, out, fill):
    assert r.rc == E_ARG, r.rc
    assert r.plan == [0] * 8, r.plan
    assert bool((out == fill).all()), 'a refused call wrote the output'


@pytest.mark.parametrize('mode,path', [('fp32', 0), ('f16x', 2), ('bf16', 0), ('bf16', 4), ('bf16', 13)])
def test_launch_conv_refusals(mode, path):
    """Every VTF_CHECK of launch_conv returns VTF_E_ARG and launches nothing."""
    def call(Cin=16, ics=None, Cout=16, H=6, **o):
        x = torch.ones((1, H, 6, ics or Cin), device='cuda')  # ics != Cin is passed on as in_cstride
        w = torch.ones((Cout, 1, 1, Cin), device='cuda')
        out = torch.full((1, H, 6, Cout), 9.0, device='cuda')
        return conv2d(x, w, mode=mode, path=path, out=out, **o), out

    _refused(*call(Cin=12), 9)                                           # Cin % 8
    _refused(*call(Cin=16, ics=20), 9)                                   # in_cstride % 8
    _refused(*call(Cin=16, in_cstride=8), 9)                             # in_cstride < Cin
    res = torch.ones((1, 2, 3, 16), device='cuda')
    _refused(*call(H=5, res=res, res_up2=1), 9)                          # res_up2 with odd OH
    out2 = torch.ones((1, 6, 6, 16), device='cuda')
    _refused(*call(n_split=16, out2=out2, out2_cstride=16), 9)           # n_split == Cout
    _refused(*call(n_split=8, out2=out2, out2_cstride=16, out_f32=1), 9)  # n_split with out_f32
    big = torch.full((1, 12, 12, 16), 9.0, device='cuda')
    x = torch.ones((1, 6, 6, 16), device='cuda')
    w = torch.ones((16, 1, 1, 16), device='cuda')
    r = conv2d(x, w, mode=mode, path=path, out=big, n_split=8, out2=out2, out2_cstride=16, up2=1)  # n_split with up2
    _refused(r, big, 9)
    r, out = call()  # and the same call without a fault runs
    assert r.rc == 0 and r.plan[0] != 0 and bool((out == 16).all())


@pytest.mark.parametrize('mode,path', [('bf16', 13), ('bf16', 11), ('sp', 0), ('sp', 21), ('s3', 0)])
def test_launch_conv_dma_refusals(mode, path):
    """conv_dma on channel counts / strides / offsets that are not multiples of 8: VTF_E_ARG,
    nothing launched."""
    x = torch.ones((1, 6, 6, 16), device='cuda')
    for Cout, ocs, coff in ((12, 12, 0), (16, 20, 0), (16, 24, 4)):
        w = torch.ones((Cout, 1, 1, 16), device='cuda')
        out = torch.full((1, 6, 6, ocs), 9.0, device='cuda')
        o = dict(out_f32=1) if mode == 's3' else {}  # an fp32 output: the refusal is conv_dma_ok's, not the packer's
        _refused(conv2d(x, w, mode=mode, path=path, out=out, out_coff=coff, **o), out, 9)
    if mode != 's3':
        out = torch.full((1, 6, 6, 16), 9.0, device='cuda')
        out2 = torch.ones((1, 6, 6, 12), device='cuda')
        w = torch.ones((24, 1, 1, 16), device='cuda')
        _refused(conv2d(x, w, mode=mode, path=path, out=out, n_split=16, out2=out2, out2_cstride=12), out, 9)
    w = torch.ones((16, 1, 1, 16), device='cuda')
    out = torch.full((1, 6, 6, 16), 9.0, device='cuda')
    r = conv2d(x, w, mode=mode, path=path, out=out)
    assert r.rc == 0 and r.plan[0] != 0 and bool((out == 16).all())
