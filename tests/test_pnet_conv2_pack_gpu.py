"""k_pnet's packed pooled map (sub-planes A[cell][ch 0..7] and C[cell] = [c8 c9 | c8 c9 of the next
column]) and conv2's K packing on it: every conv2 operand is one 16-byte read, the second pair of a
C cell is written by conv1's lanes 10, 11 into the previous cell, and conv2's fragments are
row-aligned.  Tiny frames, so that tile edges, row ends and level changes fall inside a handful of
tiles; the pyramids hold upsampled levels (exact-levels kernel) and downsampled ones whose PNet maps
are smaller than a tile, one tile, and one cell more than a tile.

Reference: oracle.mtcnn (CPU), through test_pnet_tile_loop_gpu's helpers and cache: face counts
exact, boxes 2e-3 px, stage-1 keys equal to the oracle's except within 2e-5 of the 0.6 gate (at
most 1 % of the oracle's keys lie there: asserted by the helper).  Dense outputs: atol 2e-5.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT
from test_pnet_tile_loop_gpu import ONE, SMALL, _check_vs_oracle, _model, _oracle, _run, _same

gpu = pytest.mark.gpu
SHAPES = SMALL + [ONE]  # (3, 57, 83), (2, 90, 160), (1, 200, 120) at min_face_size 5


@gpu
@pytest.mark.parametrize('shape', SHAPES)
def test_small_frames_vs_oracle(shape):
    m = _model()
    keys, res = _run(m, torch.from_numpy(_oracle(shape)[0]).cuda(), shape[4])
    plan = m.pnet_plan().tolist()
    assert 1 in plan and 0 in plan, ('both k_pnet launches must take levels', shape, plan)
    _check_vs_oracle(shape, keys, res)


@gpu
@pytest.mark.parametrize('env', [{'VTF_PNET_PR': '0'}, {'VTF_PNET_X': '0'}, {'VTF_PNET_VR': '1'}, {'VTF_PNET_C1K': '0'}],
                         ids=lambda e: ','.join('%s=%s' % kv for kv in e.items()))
def test_plan_variants(env, monkeypatch):
    """The general kernel instead of PR / of the exact-levels kernel, vertical reuse (pooled rows
    carried through the slot as byte ranges of A and C) and the 32x32 conv1 on the exact levels:
    every conv1 path that writes the packed map, every reader.  Same counts, boxes within
    test_mtcnn_b16_pnet_variants' tolerance of the default plan, same keys outside the band."""
    base = _model()
    for shape in SHAPES:
        frames = torch.from_numpy(_oracle(shape)[0]).cuda()
        near = _oracle(shape)[3]
        with monkeypatch.context() as mp:
            one = _run(base, frames, shape[4])
            for k, v in env.items():
                mp.setenv(k, v)
            alt = _run(_model(), frames, shape[4])  # (VTF_PNET_C1K is read when the model is made)
        assert [r.shape[0] for r in alt[1]] == [r.shape[0] for r in one[1]]
        np.testing.assert_allclose(np.concatenate(alt[1]), np.concatenate(one[1]), rtol=1e-5, atol=2e-3)
        diff = np.setxor1d(alt[0], one[0])
        assert np.isin(diff, near).all(), (shape, env, diff[~np.isin(diff, near)][:8])
        _check_vs_oracle(shape, *alt)


@gpu
@pytest.mark.parametrize('shape', SHAPES)
def test_independent_of_tile_assignment(shape, monkeypatch):
    """Which tiles a workgroup takes one after the other changes nothing: identical keys and rows.
    A duplicate pair left over from the previous tile and read by this one shows up here."""
    m = _model()
    frames = torch.from_numpy(_oracle(shape)[0]).cuda()
    base = _run(m, frames, shape[4])
    for chunk in (1, 3, 64):
        for quota in (0, 1):
            monkeypatch.setenv('VTF_PNET_CHUNK', str(chunk))
            monkeypatch.setenv('VTF_PNET_QUOTA', str(quota))
            _same(_run(m, frames, shape[4]), base)


def _loud_params():
    """The synthetic parameters with conv1's channels 8 and 9 -- the ones the pooled map stores
    twice -- made large and distinct: a duplicate that lands in the wrong cell or meets a nonzero
    weight moves the outputs far outside the tolerance.  (Slopes stay in [0, 1], weights below 16:
    the default conv1 paths.)"""
    from videotofaces import synth
    p = {k: np.array(v, copy=True) for k, v in synth.make_params('mtcnn').items()}
    w, b, a = list(p)[:3]
    assert p[w].shape == (10, 3, 3, 3) and p[b].shape == (10,) and p[a].shape == (10,), (w, b, a)
    p[w][8] *= 3.0
    p[w][9] *= -2.0
    p[b][8], p[b][9] = 0.5, -0.4
    p[a][8], p[a][9] = 0.75, 0.5
    return p


@gpu
@pytest.mark.parametrize('loud', [False, True], ids=['synthetic', 'loud_ch8_ch9'])
def test_dense_levels_vs_oracle(loud):
    """pnet_level (the general kernel's split conv1 / conv2, dense outputs) on maps of several
    tiles, a few tiles and less than one."""
    from oracle import mtcnn as om
    from videotofaces import synth
    from videotofaces.detectors.mtcnn import MTCNN
    params = _loud_params() if loud else synth.make_params('mtcnn')
    m = MTCNN('cuda:0', params=params)
    fr = synth.make_frames(2, 90, 160, seed=9)
    x = om.preprocess(list(fr))
    dev = torch.from_numpy(fr).cuda()
    for (lh, lw) in [(217, 385), (54, 97), (12, 21), (13, 12)]:
        reg, prob = m.pnet_level(dev, lh, lw)
        rref, pref = om.pnet(params, F.adaptive_avg_pool2d(x, (lh, lw)))
        ep = np.abs(prob.cpu().numpy() - pref.numpy()).max()
        er = np.abs(reg.cpu().numpy() - rref.numpy()).max()
        print('level', (lh, lw), 'loud' if loud else 'synthetic', 'max |prob err| %.3g  max |reg err| %.3g' % (ep, er))
        np.testing.assert_allclose(prob.cpu().numpy(), pref.numpy(), rtol=0, atol=2e-5)
        np.testing.assert_allclose(reg.cpu().numpy(), rref.numpy(), rtol=0, atol=2e-5)


def test_lds_bank_model_tool(monkeypatch, capsys):
    """scripts/lds_bank_model.py reproduces the figures the re-packing started from ([cell][12] map:
    208 / 168 LDS cycles for k-steps 0 and 1, 379 / 168 for k-step 2's dword gathers) and prints the
    packed layout's."""
    monkeypatch.syspath_prepend(os.path.join(ROOT, 'scripts'))
    monkeypatch.setattr(sys, 'argv', ['lds_bank_model.py'])
    import lds_bank_model
    p = lds_bank_model.model('parent', 'linear')
    assert (p['steps01'], p['free01'], p['step2'], p['free2']) == (208, 168, 379, 168)
    lds_bank_model.main()
    out = capsys.readouterr().out
    lines = [' '.join(l.split()) for l in out.splitlines()]
    assert 'k-steps 0, 1 (two 16-byte reads) 208 (168)' in lines, out
    assert 'k-step 2 (eight ds_read_b32) 379 (168)' in lines, out
    packed = [l for l in lines if l.startswith('packed, mean of the planes: total ')]
    assert len(packed) == 1, out
    total = float(packed[0].split('total ')[1].split(',')[0])
    assert 168 + 84 <= total < 587, out  # from conflict-free up to the parent's 587
