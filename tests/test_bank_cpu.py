"""The comb bank and the reverb preset (include/xm_effects.h) on the CPU backend,
and their host-side API: bit for bit the sum of scipy lfilter branches in
float32 (tests/golden/bank.npz) and tests/bank_ref.py.  No GPU."""
import numpy as np
import pytest

from conftest import bits_equal, ulp_diff

import bank_cases as BK
import comb_cases as K
from bank_ref import bank_f32, reverb_taps
from comb_ref import comb_f32

N = 1200


def make(xm):
    return lambda C, rate=44100: xm.Effects(rate, C, device="cpu")


def test_bank_golden_manifest():
    """bank.npz is the file tools/gen_golden_bank.py wrote (its own manifest), smaller than comb.npz"""
    import hashlib
    import json
    import os
    from conftest import GOLDEN
    with open(os.path.join(GOLDEN, "MANIFEST_bank.json")) as fh:
        want = json.load(fh)["files"]["bank.npz"]
    with open(os.path.join(GOLDEN, "bank.npz"), "rb") as fh:
        data = fh.read()
    assert len(data) == want["bytes"] and hashlib.sha256(data).hexdigest() == want["sha256"]
    assert len(data) < os.path.getsize(os.path.join(GOLDEN, "comb.npz"))


def test_cpu_bank_golden(xm):
    BK.check_golden(make(xm))


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("lags", [(1,), (1, 2, 3), (15, 16, 17, 16), (100, 1001), (N, 7), (N + 300, N - 1, 64),
                                  (5, 9, 13, 17, 21, 25, 29, 33)])
def test_cpu_bank_vs_ref(xm, C, lags):
    """1 to 8 branches, lags from 1 to past the clip, 1, 3 and 17 clips, out of place and in place"""
    taps = BK.with_lags(lags)
    want = BK.bank_ref_clips(C, N, taps)
    e = xm.Effects(44100, C, device="cpu")
    e.add_comb_bank(taps, BK.DRY)
    for B in (1, 3, 17):
        x = K.clips(C, N)[:B]
        assert bits_equal(e.process(x.copy()), want[:B]), (B, "out of place")
        assert bits_equal(e.process(x.copy(), inplace=True), want[:B]), (B, "in place")


def test_cpu_bank_signed_zeros(xm):
    """a zero coefficient still forms its product: the zero's sign is part of the contract"""
    for C in (1, 2):
        x = K.zeros_input(C)[None]
        for taps, dry in (([(3, 0.0, 1.0, -0.5, 0.3), (7, -0.0, 0.0, 0.5, -0.3)], 0.0),
                          ([(1, -1.0, -0.0, 0.0, 0.0), (200, 0.0, -1.0, -0.0, 1.0)], -0.0)):
            e = xm.Effects(44100, C, device="cpu")
            e.add_comb_bank(taps, dry)
            r = bank_f32(x[0], taps, dry)
            y = e.process(x.copy())[0]
            assert bits_equal(y, r), (C, taps, int(np.sum(y.view(np.uint32) != r.view(np.uint32))))


def test_cpu_bank_streaming(xm):
    BK.check_streaming(make(xm), [BK.PRESET, BK.GENERAL, BK.with_lags((3100, 700, 4000))])


def test_cpu_bank_mixed_chain(xm):
    BK.check_mixed_chain(make(xm))


def test_comb_bank_round_trip(xm):
    e = xm.Effects(44100, 2, device="cpu")
    e.add_biquad([1.0, 0.0, 0.0, 1.0, 0.0, 0.0])
    e.add_comb_bank(BK.GENERAL, -0.8)
    e.add_comb(10, 1.0, 0.5, 0.5)
    e.add_comb_bank(BK.with_lags((xm.XM_MAX_DELAY,) * xm.XM_MAX_BANK), 0.25)
    assert e.count() == 4
    taps, dry = e.comb_bank(1)
    assert dry == np.float32(-0.8) and taps == BK.f32taps(BK.GENERAL)
    taps, dry = e.comb_bank(3)
    assert dry == np.float32(0.25) and taps == BK.f32taps(BK.with_lags((xm.XM_MAX_DELAY,) * 8))
    for f in (lambda: e.comb_bank(0), lambda: e.comb_bank(2), lambda: e.comb_bank(4), lambda: e.comb_bank(-1),
              lambda: e.comb(1), lambda: e.biquad(1)):
        with pytest.raises(xm.XmError) as err:
            f()
        assert err.value.code == xm.XM_EINVAL


def test_comb_bank_argument_errors(xm):
    e = xm.Effects(44100, 2, device="cpu")
    t = (10, 1.0, 0.5, 0.5, 0.5)
    nan, inf = float("nan"), float("inf")
    bad = [lambda: e.add_comb_bank([], 1.0), lambda: e.add_comb_bank([t] * 9, 1.0),
           lambda: e.add_comb_bank([t, (0, 1.0, 0.5, 0.5, 0.5)], 1.0),
           lambda: e.add_comb_bank([(-1, 1.0, 0.5, 0.5, 0.5)], 1.0),
           lambda: e.add_comb_bank([t, (xm.XM_MAX_DELAY + 1, 1.0, 0.5, 0.5, 0.5)], 1.0),
           lambda: e.add_comb_bank([(10, nan, 0.5, 0.5, 0.5)], 1.0), lambda: e.add_comb_bank([(10, 1.0, inf, 0.5, 0.5)], 1.0),
           lambda: e.add_comb_bank([t, (10, 1.0, 0.5, nan, 0.5)], 1.0), lambda: e.add_comb_bank([(10, 1.0, 0.5, 0.5, -inf)], 1.0),
           lambda: e.add_comb_bank([t], nan),
           lambda: e.add_reverb(0.0, 1.0, 0.3), lambda: e.add_reverb(-1.0, 1.0, 0.3), lambda: e.add_reverb(nan, 1.0, 0.3),
           lambda: e.add_reverb(inf, 1.0, 0.3), lambda: e.add_reverb(1.0, nan, 0.3), lambda: e.add_reverb(1.0, 1.0, inf)]
    for f in bad:
        with pytest.raises(xm.XmError) as err:
            f()
        assert err.value.code == xm.XM_EINVAL
    assert e.count() == 0
    # a rate at which a preset delay rounds to 0 frames (1.7 ms * 200 Hz = 0.34) or past XM_MAX_DELAY
    for rate in (200, 30_000_000):
        lo = xm.Effects(rate, 1, device="cpu")
        with pytest.raises(xm.XmError) as err:
            lo.add_reverb(1.0, 1.0, 0.3)
        assert err.value.code == xm.XM_EINVAL and lo.count() == 0
    # 128 effects at most; the reverb needs room for all three or adds none
    for _ in range(126):
        e.add_comb_bank([t], 1.0)
    with pytest.raises(xm.XmError) as err:
        e.add_reverb(1.0, 1.0, 0.3)
    assert err.value.code == xm.XM_ENOMEM and e.count() == 126
    e.add_comb_bank([t], 1.0)
    e.add_comb_bank([t], 1.0)
    with pytest.raises(xm.XmError) as err:
        e.add_comb_bank([t], 1.0)
    assert err.value.code == xm.XM_ENOMEM and e.count() == 128


@pytest.mark.parametrize("rate,rt60", [(44100, 1.8), (48000, 0.6), (96000, 3.0), (8000, 0.25)])
def test_reverb_preset(xm, rate, rt60):
    """exactly 3 effects: the bank of four combs, then the two all-passes; each
    loop gain within 1 fp32 ulp of numpy's (an fp64 pow that differs in its
    last bit can move the fp32 cast by that much at most); the output is
    checked with the coefficients read back from the handle"""
    e = xm.Effects(rate, 2, device="cpu")
    e.add_eq_band(xm.XM_EQ_PEAKING, 1500.0, 2.5, 1.2)
    e.add_reverb(rt60, 0.75, 0.3)
    assert e.count() == 4
    taps, dry = e.comb_bank(1)
    want = reverb_taps(rate, rt60, 0.3)
    assert dry == np.float32(0.75) and len(taps) == 4
    for (D, b0, bd, ad, mix), (wD, _, _, wad, wmix) in zip(taps, want):
        assert D == wD and D == int(np.rint(D)) and bits_equal(np.float32([b0, bd, mix]), np.float32([0.0, 1.0, wmix]))
        assert ad < 0 and ulp_diff(np.float32([ad]), np.float32([wad])) <= 1, (D, ad, wad)
    for i, ms in ((2, 5.0), (3, 1.7)):
        d, c = e.comb(i)
        g = np.float32(0.7)
        assert d == int(np.rint(ms * rate / 1000.0)) and bits_equal(c, np.array([-g, 1.0, -g], np.float32)), (i, d, c)
    x = K.clips(2, 6000)[:2]
    y = e.process(x.copy())
    sos = e.biquad(0)[None]
    for b in range(2):
        r = K.O.biquad_f32(x[b], sos)
        r = bank_f32(r, taps, dry)
        for i in (2, 3):
            d, c = e.comb(i)
            r = comb_f32(r, d, *c)
        assert bits_equal(y[b], r), b


def test_cpu_mixer_track_effects_with_reverb(xm):
    BK.check_mixer(xm, device="cpu")
