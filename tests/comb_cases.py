"""Cases shared by tests/test_comb_cpu.py and tests/test_gpu_comb.py: inputs,
references (computed once per shape and kept unchanged) and the checks that
both backends must pass bit for bit.  Not a test module."""
import functools

import numpy as np

from conftest import bits_equal, golden

import np_oracle as O
from comb_ref import comb_f32

SEED = O.SEED
COEF = (0.75, -0.5, 0.4)        # negative bd, positive ad
ECHO = (1.0, 0.5, -0.45)
BMAX = 17                       # the largest batch; smaller batches are its first clips


@functools.lru_cache(maxsize=None)
def clips(C, N, B=BMAX, base=7000):
    x = np.stack([O.gen_f32(SEED, base + b, C, N) for b in range(B)])
    x.setflags(write=False)
    return x


def as_channels(x):
    """[B, N, C] -> [N, B*C]: clips are as independent as channels, so a
    batch runs through the per-clip references in one pass."""
    B, N, C = x.shape
    return np.ascontiguousarray(x.transpose(1, 0, 2)).reshape(N, B * C)


def from_channels(y, B):
    N = y.shape[0]
    return np.ascontiguousarray(y.reshape(N, B, -1).transpose(1, 0, 2))


def comb_batch(x, D, coef):
    return from_channels(comb_f32(as_channels(x), D, *coef), x.shape[0])


@functools.lru_cache(maxsize=None)
def comb_ref_clips(C, N, D, coef=COEF):
    y = comb_batch(clips(C, N), D, coef)
    y.setflags(write=False)
    return y


def golden_cases():
    z = golden("comb.npz")
    for name in z["names"]:
        name = str(name)
        D, C, N, clip = (int(v) for v in z[f"{name}__meta"])
        yield name, D, z[f"{name}__coef"], O.gen_f32(SEED, clip, C, N), z[f"{name}__y"]


def zeros_input(C, N=600):
    """+0.0, -0.0, runs of zeros and a few samples: the sign of every zero
    the recurrence produces is part of the contract."""
    x = O.gen_f32(SEED, 7100, C, N).copy()
    x[::3] = 0.0
    x[1::7] = -0.0
    x[40:140] = 0.0
    x[200:260] = -0.0
    x[300:330] = 0.0
    return x


def stream(e, x, sizes, inplace_every=3):
    """x [B, N, C] through process_stream in blocks of `sizes` frames."""
    e.stream_reset(x.shape[0])
    outs, p = [], 0
    for i, n in enumerate(sizes):
        blk = x[:, p:p + n].copy()
        outs.append(e.process_stream(blk, inplace=(i % inplace_every == inplace_every - 1)))
        p += n
    assert p == x.shape[1]
    return np.concatenate(outs, axis=1)


def splits(N, pattern, rest=997):
    out, left = [], N
    for b in pattern:
        b = min(b, left)
        out.append(b)
        left -= b
    while left > 0:
        out.append(min(rest, left))
        left -= out[-1]
    return out


RAGGED = [0, 1, 5, 137, 0, 1000, 17, 2, 33, 1, 1, 700]
SINGLES = [1] * 45 + [0, 3]


def check_signed_zeros(make):
    for C in (1, 2):
        x = zeros_input(C)[None]
        for D, coef in ((1, (-0.5, -0.25, -0.75)), (3, (-1.0, -0.5, 0.5)), (200, (-0.5, -0.25, -0.75)),
                        (700, (-0.0, -1.0, 0.0))):
            e = make(C)
            e.add_comb(D, *coef)
            y = e.process(x.copy())
            r = comb_f32(x[0], D, *coef)
            assert bits_equal(y[0], r), (C, D, coef, int(np.sum(y[0].view(np.uint32) != r.view(np.uint32))))


def mixed_chain_parts():
    z = golden("effects.npz")
    h5 = np.array([0.5, -0.25, 0.125, 0.3, -0.1], np.float32)
    return z["sos"][:2], z["h63"], h5


def check_mixed_chains(make, N=900, B=3):
    sos, h63, h5 = mixed_chain_parts()
    for C in (1, 2):
        x = clips(C, N)[:B]
        xc = as_channels(x)
        # biquad x2 -> comb -> FIR -> comb
        e = make(C)
        for s in sos:
            e.add_biquad(s)
        e.add_comb(5, *COEF)
        e.add_fir(h63)
        e.add_comb(300, *ECHO)
        r = comb_f32(O.fir_f32(comb_f32(O.biquad_f32(xc, sos), 5, *COEF), h63), 300, *ECHO)
        r = from_channels(r, B)
        assert bits_equal(e.process(x.copy()), r), ("bq-comb-fir-comb", C)
        assert bits_equal(e.process(x.copy(), inplace=True), r), ("bq-comb-fir-comb in place", C)
        # FIR -> comb -> FIR, in place
        e = make(C)
        e.add_fir(h5)
        e.add_comb(130, *COEF)
        e.add_fir(h63)
        r = from_channels(O.fir_f32(comb_f32(O.fir_f32(xc, h5), 130, *COEF), h63), B)
        assert bits_equal(e.process(x.copy(), inplace=True), r), ("fir-comb-fir in place", C)
        assert bits_equal(e.process(x.copy()), r), ("fir-comb-fir", C)
        # comb -> comb (two stages of their own) and comb last after a FIR
        e = make(C)
        e.add_comb(2, *ECHO)
        e.add_comb(64, *COEF)
        r = from_channels(comb_f32(comb_f32(xc, 2, *ECHO), 64, *COEF), B)
        assert bits_equal(e.process(x.copy(), inplace=True), r), ("comb-comb in place", C)
        assert bits_equal(e.process(x.copy()), r), ("comb-comb", C)


def check_streaming(make, N=3100, B=3):
    sos, h63, _ = mixed_chain_parts()
    for C in (1, 2):
        x = clips(C, N)[:B]
        for D in (1, 100, 700):
            e = make(C)
            e.add_comb(D, *COEF)
            want = comb_ref_clips(C, N, D)[:B]
            assert bits_equal(e.process(x.copy()), want), (C, D)
            for pat in (RAGGED, SINGLES, [10 ** 9]):
                assert bits_equal(stream(e, x, splits(N, pat)), want), (C, D, pat[:4])
        # a mixed chain streamed: biquad -> comb -> FIR -> comb
        e = make(C)
        e.add_biquad(sos[0])
        e.add_comb(37, *COEF)
        e.add_fir(h63)
        e.add_comb(700, *ECHO)
        want = e.process(x.copy())
        xc = as_channels(x)
        r = comb_f32(O.fir_f32(comb_f32(O.biquad_f32(xc, sos[:1]), 37, *COEF), h63), 700, *ECHO)
        assert bits_equal(want, from_channels(r, B)), C
        assert bits_equal(stream(e, x, splits(N, RAGGED)), want), C
        # adding an effect ends the streams until the next reset
        e.add_comb(3, *ECHO)
        try:
            e.process_stream(x[:, :10].copy())
        except Exception as err:
            assert getattr(err, "code", None) == -22, err
        else:
            raise AssertionError("process_stream after add_comb must fail until reset")
        e.stream_reset(B)
        assert bits_equal(e.process_stream(x.copy()), e.process(x.copy())), C


def check_mixer(xm, **mixer_kw):
    """2 tracks, 48k -> 44.1k, chain = EQ band + comb, against the oracle composition."""
    import c_oracle as CO
    N = 2000
    ramps = [dict(gain0=0.5), dict(gain0=0.25, gain1=0.8, ramp_start=100, ramp_len=900)]
    x = np.stack([O.gen_f32(SEED, 7200 + t, 2, N) for t in range(2)])[None]
    e = xm.Effects(44100, 2, **mixer_kw)
    e.add_eq_band(xm.XM_EQ_PEAKING, 1500.0, 2.5, 1.2)
    e.add_comb(441, *ECHO)
    sos = e.biquad(0)[None]
    m = xm.Mixer(48000, 44100, 2, "f32", **mixer_kw)
    m.set_tracks(ramps)
    m.set_track_effects(e)
    y = m.process(x)[0]
    r = [comb_f32(CO.biquad_f32(CO.resample_f32(t, 147, 160), sos), 441, *ECHO) for t in x[0]]
    assert bits_equal(y, CO.mix_f32(r, ramps))
