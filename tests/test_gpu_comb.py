"""The comb stage on the GPU (csrc/xm_fx.hip k_comb_wide / k_comb_narrow):
bit for bit scipy lfilter in float32 (tests/golden/comb.npz), tests/comb_ref.py
and the CPU backend, through host and device memory, in and out of place,
whole clips and streams, in mixed chains, per-track in a mixer and over a
multi-device chain."""
import numpy as np
import pytest

from conftest import bits_equal

import comb_cases as K
from comb_ref import comb_f32

pytestmark = pytest.mark.gpu
N = 4100
WIDE_MIN = 256   # XMG_COMB_WIDE_MIN (csrc/xm_gpu.h): lags of that many samples and more run k_comb_wide
DS = sorted({1, 2, 3, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513, 1000, 1001, 2047, 4099, 4100,
             5000, WIDE_MIN - 1, WIDE_MIN, WIDE_MIN + 1, WIDE_MIN // 2 - 1, WIDE_MIN // 2, WIDE_MIN // 2 + 1})


def make(xm):
    return lambda C, rate=44100: xm.Effects(rate, C)


def run_device(e, x, inplace):
    """x [B, N, C] through a device-memory chain."""
    import torch
    xd = torch.from_numpy(np.array(x, np.float32)).cuda()
    yd = xd if inplace else torch.full_like(xd, float("nan"))
    torch.cuda.synchronize()
    e.process_ptrs([xd[b].data_ptr() for b in range(x.shape[0])], [yd[b].data_ptr() for b in range(x.shape[0])],
                   x.shape[1])
    torch.cuda.synchronize()
    return yd.cpu().numpy()


def test_gpu_comb_golden(xm, gpu):
    for name, D, coef, x, want in K.golden_cases():
        e = xm.Effects(44100, x.shape[1])
        e.add_comb(D, *coef)
        assert bits_equal(e.process(x[None].copy())[0], want), name
        ed = xm.Effects(44100, x.shape[1], mem="device")
        ed.add_comb(D, *coef)
        assert bits_equal(run_device(ed, x[None], True)[0], want), name


@pytest.mark.parametrize("D", DS)
def test_gpu_comb_vs_ref(xm, gpu, D):
    """mono and stereo (so the mono lags D and the stereo lags 2D samples fall
    on both sides of the regime switch), 1, 3 and 17 clips, in and out of
    place, host and device memory"""
    for C in (1, 2):
        want = K.comb_ref_clips(C, N, D)
        x = K.clips(C, N)
        eh, ed = xm.Effects(44100, C), xm.Effects(44100, C, mem="device")
        for e in (eh, ed):
            e.add_comb(D, *K.COEF)
        for B, inplace in ((1, False), (3, True), (17, False), (17, True)):
            assert bits_equal(eh.process(x[:B].copy(), inplace=inplace), want[:B]), (C, B, inplace, "host")
            assert bits_equal(run_device(ed, x[:B], inplace), want[:B]), (C, B, inplace, "device")


@pytest.mark.parametrize("D", [5, 700])
def test_gpu_comb_short_clips(xm, gpu, D):
    """frames around the lag: the block is all zero padding, one block, two"""
    for C in (1, 2):
        e = xm.Effects(44100, C, mem="device")
        e.add_comb(D, *K.ECHO)
        for F in (1, D - 1, D, D + 1, 2 * D, 2 * D + 1):
            x = K.clips(C, N)[:3, :F]
            want = K.comb_batch(x, D, K.ECHO)
            assert bits_equal(run_device(e, x, False), want), (C, F)
            assert bits_equal(run_device(e, x, True), want), (C, F, "in place")


def _v4_clips(xm, C, Ds):
    """Enough clips that the launcher gives a lane 4 positions (k_comb_wide<4, 4>):
    (Ds / 4) * clips >= CUs * 2048 (xmg_launch_fx_comb)."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = -(-cus * 2048 // (Ds // 4)) + 3
    assert (Ds // 4) * B >= cus * 2048
    return B


def _synth_clips(xm, B, F, C, base):
    """gen_f32 clips base .. base+B-1, generated on the device (k_synth is np_oracle.gen_f32's twin)."""
    import torch
    xd = torch.empty((B, F, C), dtype=torch.float32, device="cuda")
    xm.synth(xd.data_ptr(), "f32", K.SEED, base, B, C, F, 0)
    torch.cuda.synchronize()
    return xd


# (channels, D, frames): the lag D*C is 2 and 3 past a multiple of 4 (the last
# lane of the range owns 2 or 3 positions) and a multiple of 4 that is no
# multiple of a workgroup's 1024 positions; frames give 3 blocks with a ragged
# 3-frame tail, 2 whole blocks and a long ragged one, and 9 blocks (whole
# rounds of 4 blocks in straight-line code, then the bounded rest)
V4_CASES = [(2, 16385, 2 * 16385 + 3), (1, 32771, 40001 * 2), (2, 16390, 40001), (2, 16385, 8 * 16385 + 5),
            (1, 32771, 9 * 32771 + 2)]


@pytest.mark.parametrize("C,D,F", V4_CASES)
def test_gpu_comb_wide_four_positions_per_lane(xm, gpu, C, D, F):
    """shapes large enough for k_comb_wide<4, 4>: 16-B accesses on 4-B aligned
    block starts, partial lanes, ragged blocks, in and out of place"""
    import torch
    B = _v4_clips(xm, C, D * C)
    xd = _synth_clips(xm, B, F, C, 7300)
    x = xd.cpu().numpy()
    assert bits_equal(x[B - 1], K.O.gen_f32(K.SEED, 7300 + B - 1, C, F))
    want = K.comb_batch(x, D, K.COEF)
    e = xm.Effects(44100, C, mem="device")
    e.add_comb(D, *K.COEF)
    yd = torch.full_like(xd, float("nan"))
    torch.cuda.synchronize()
    e.process_ptrs([xd[b].data_ptr() for b in range(B)], [yd[b].data_ptr() for b in range(B)], F)
    torch.cuda.synchronize()
    assert bits_equal(yd.cpu().numpy(), want), "out of place"
    assert bits_equal(xd.cpu().numpy(), x), "the input was written"
    e.process_ptrs([xd[b].data_ptr() for b in range(B)], [xd[b].data_ptr() for b in range(B)], F)
    torch.cuda.synchronize()
    assert bits_equal(xd.cpu().numpy(), want), "in place"


@pytest.mark.parametrize("C,D", [(2, 16385), (1, 32771)])
def test_gpu_comb_wide_four_positions_streaming(xm, gpu, C, D):
    """k_comb_wide<4, 4, true>: the history rotation (p - n) mod Ds for 4
    positions per lane, blocks shorter and longer than D, in place on the device"""
    import torch
    F = 2 * D + 7001
    B = _v4_clips(xm, C, D * C)
    xd = _synth_clips(xm, B, F, C, 7600)
    want = K.comb_batch(xd.cpu().numpy(), D, K.COEF)
    e = xm.Effects(44100, C, mem="device")
    e.add_comb(D, *K.COEF)
    e.stream_reset(B)
    p = 0
    for n in K.splits(F, [0, 1, 5, 137, 0, 1000, 3, D + 2, 17, D - 1], rest=20011):
        if n:
            blk = xd[:, p:p + n].contiguous()
            ptrs = (xm.C.c_void_p * B)(*[blk[b].data_ptr() for b in range(B)])
            torch.cuda.synchronize()
            xm._check(xm._lib.xm_effects_process_stream(e._h, ptrs, ptrs, B, n), "process_stream")
            torch.cuda.synchronize()
            xd[:, p:p + n] = blk
        p += n
    assert bits_equal(xd.cpu().numpy(), want)


def test_gpu_comb_signed_zeros(xm, gpu):
    K.check_signed_zeros(make(xm))


def test_gpu_comb_mixed_chains(xm, gpu):
    K.check_mixed_chains(make(xm))


def test_gpu_comb_streaming(xm, gpu):
    K.check_streaming(make(xm))


def test_gpu_comb_streaming_device_in_place(xm, gpu):
    import torch
    B, F = 3, 3100
    for C, D in ((2, 1), (1, 100), (2, 700)):
        x = K.clips(C, F)[:B]
        want = K.comb_ref_clips(C, F, D)[:B]
        e = xm.Effects(44100, C, mem="device")
        e.add_comb(D, *K.COEF)
        e.stream_reset(B)
        outs, p = [], 0
        for n in K.splits(F, K.RAGGED):
            if n:
                blk = torch.from_numpy(np.ascontiguousarray(x[:, p:p + n])).cuda()
                ptrs = (xm.C.c_void_p * B)(*[blk[b].data_ptr() for b in range(B)])
                torch.cuda.synchronize()
                xm._check(xm._lib.xm_effects_process_stream(e._h, ptrs, ptrs, B, n), "process_stream")
                torch.cuda.synchronize()
                outs.append(blk.cpu().numpy())
            p += n
        assert bits_equal(np.concatenate(outs, axis=1), want), (C, D)


def test_gpu_comb_equals_cpu_backend(xm, gpu):
    """one case per regime: narrow (2 samples) and wide (1400 samples)"""
    x = K.clips(2, N)[:3]
    for D in (1, 700):
        g, c = xm.Effects(44100, 2), xm.Effects(44100, 2, device="cpu")
        for e in (g, c):
            e.add_echo(1000.0 * D / 44100, 0.45, 0.5)
            assert e.comb(0)[0] == D
        assert bits_equal(g.process(x.copy()), c.process(x.copy())), D


def test_gpu_mixer_track_effects_with_comb(xm, gpu):
    K.check_mixer(xm)


def test_gpu_comb_multi_device_chain(xm, gpu):
    x = K.clips(2, N)[:5]
    one, two = xm.Effects(44100, 2), xm.Effects(44100, 2, devices=[0, 0])
    assert two.n_devices() == 2
    for e in (one, two):
        e.add_biquad(K.mixed_chain_parts()[0][0])
        e.add_comb(3, *K.COEF)
        e.add_allpass(10.0, 0.6)
    assert two.comb(1)[0] == 3 and two.comb(2)[0] == 441
    want = one.process(x.copy())
    assert bits_equal(two.process(x.copy()), want)
    assert bits_equal(K.stream(two, x, K.splits(N, K.RAGGED)), want)
    assert bits_equal(want[0], comb_f32(comb_f32(K.O.biquad_f32(x[0], K.mixed_chain_parts()[0][:1]), 3, *K.COEF),
                                        441, *(-np.float32(0.6), 1.0, -np.float32(0.6))))
