"""Cases shared by tests/test_bank_cpu.py and tests/test_gpu_bank.py: lag sets,
references (computed once per shape and kept unchanged) and the checks that
both backends must pass bit for bit.  Not a test module."""
import functools

import numpy as np

from conftest import bits_equal, golden

import np_oracle as O
import comb_cases as K
from bank_ref import bank_f32
from comb_ref import comb_f32

SEED = O.SEED
# (D, b0, bd, ad, mix) per branch
PRESET = ((1310, 0.0, 1.0, -0.84, 0.3), (1636, 0.0, 1.0, -0.80, 0.3), (1813, 0.0, 1.0, -0.78, 0.3),
          (1927, 0.0, 1.0, -0.77, 0.3))          # the reverb's lags at 44.1 kHz
GENERAL = ((333, 0.5, -0.25, 0.4, 0.6), (1, -0.3, 0.2, -0.5, -0.35), (333, 1.0, 0.5, -0.45, 0.2),
           (64, -0.7, 1.0, -0.7, 0.5))           # b0, bd != 0, equal lags, a lag of 1
DRY = 0.7


def with_lags(lags):
    """GENERAL-like coefficients (every product live) on the given lags."""
    c = ((0.5, -0.25, 0.4, 0.6), (-0.3, 1.0, -0.5, -0.35), (1.0, 0.5, -0.45, 0.2), (0.0, 1.0, -0.7, 0.5),
         (0.25, 0.75, 0.6, -0.1), (0.0, 1.0, 0.8, 0.15), (-1.0, 0.3, -0.3, 0.3), (0.6, -1.0, 0.2, 0.25))
    return tuple((int(D),) + c[k] for k, D in enumerate(lags))


def f32taps(taps):
    return [(int(t[0]),) + tuple(np.float32(v) for v in t[1:]) for t in taps]


def bank_batch(x, taps, dry):
    """x [B, N, C]: clips are as independent as channels (comb_cases.as_channels)."""
    return K.from_channels(bank_f32(K.as_channels(x), f32taps(taps), np.float32(dry)), x.shape[0])


@functools.lru_cache(maxsize=None)
def bank_ref_clips(C, N, taps, dry=DRY, B=K.BMAX):
    y = bank_batch(K.clips(C, N)[:B], taps, dry)
    y.setflags(write=False)
    return y


def golden_cases():
    z = golden("bank.npz")
    for name in z["names"]:
        name = str(name)
        C, N, clip = (int(v) for v in z[f"{name}__meta"])
        taps = [(int(d),) + tuple(c) for d, c in zip(z[f"{name}__delays"], z[f"{name}__coef"])]
        yield name, taps, z[f"{name}__dry"][0], O.gen_f32(SEED, clip, C, N), z[f"{name}__y"]


def chain_ref(e, x):
    """Reference of a chain of combs and banks as read back from the handle; x one clip."""
    for i in range(e.count()):
        try:
            taps, dry = e.comb_bank(i)
            x = bank_f32(x, taps, dry)
        except Exception:
            d, c = e.comb(i)
            x = comb_f32(x, d, *c)
    return x


def check_golden(make):
    n = 0
    for name, taps, dry, x, want in golden_cases():
        e = make(x.shape[1])
        e.add_comb_bank(taps, dry)
        assert bits_equal(e.process(x[None].copy())[0], want), name
        assert bits_equal(e.process(x[None].copy(), inplace=True)[0], want), (name, "in place")
        assert bits_equal(bank_f32(x, taps, dry), want), name
        n += 1
    assert n >= 5


def check_streaming(make, lag_sets, N=3100, B=3, patterns=(K.RAGGED, K.SINGLES, [10 ** 9])):
    for C in (1, 2):
        x = K.clips(C, N)[:B]
        for taps in lag_sets:
            e = make(C)
            e.add_comb_bank(taps, DRY)
            want = bank_ref_clips(C, N, tuple(taps))[:B]
            assert bits_equal(e.process(x.copy()), want), (C, taps)
            for pat in patterns:
                assert bits_equal(K.stream(e, x, K.splits(N, pat)), want), (C, taps, pat[:4])


def check_mixed_chain(make, N=900, B=3):
    """biquad x2 -> bank -> all-pass -> FIR, in and out of place, whole and streamed"""
    sos, h63, _ = K.mixed_chain_parts()
    ap = (-np.float32(0.6), 1.0, -np.float32(0.6))
    for C in (1, 2):
        x = K.clips(C, N)[:B]
        e = make(C)
        for s in sos:
            e.add_biquad(s)
        e.add_comb_bank(GENERAL, DRY)
        e.add_comb(75, *ap)
        e.add_fir(h63)
        r = O.biquad_f32(K.as_channels(x), sos)
        r = O.fir_f32(comb_f32(bank_f32(r, f32taps(GENERAL), np.float32(DRY)), 75, *ap), h63)
        r = K.from_channels(r, B)
        assert bits_equal(e.process(x.copy()), r), ("bq-bank-ap-fir", C)
        assert bits_equal(e.process(x.copy(), inplace=True), r), ("bq-bank-ap-fir in place", C)
        assert bits_equal(K.stream(e, x, K.splits(N, K.RAGGED, rest=211)), r), ("bq-bank-ap-fir streamed", C)


def check_mixer(xm, **mixer_kw):
    """2 tracks, 48k -> 44.1k, per-track chain = the reverb preset, against the
    oracle composition with the coefficients read back from the handle."""
    import c_oracle as CO
    N = 4000
    ramps = [dict(gain0=0.5), dict(gain0=0.25, gain1=0.8, ramp_start=100, ramp_len=900)]
    x = np.stack([O.gen_f32(SEED, 7250 + t, 2, N) for t in range(2)])[None]
    e = xm.Effects(44100, 2, **mixer_kw)
    e.add_reverb(1.2, 0.8, 0.25)
    m = xm.Mixer(48000, 44100, 2, "f32", **mixer_kw)
    m.set_tracks(ramps)
    m.set_track_effects(e)
    y = m.process(x)[0]
    r = [chain_ref(e, CO.resample_f32(t, 147, 160)) for t in x[0]]
    assert bits_equal(y, CO.mix_f32(r, ramps))
