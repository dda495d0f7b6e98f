"""Reference of the comb bank (include/xm_effects.h, effect kind 4), numpy float32.

    c_k[i] = b0_k*x[i] + ( bd_k*x[i-Ds_k] - ad_k*c_k[i-Ds_k] ),   Ds_k = D_k * channels
    acc = dry*x[i];  for k ascending:  m = mix_k*c_k[i];  acc = acc + m;   y[i] = acc

Every branch is comb_ref.comb_f32 (scipy lfilter in float32 bit for bit:
tools/gen_golden_bank.py asserts that per branch before it writes
tests/golden/bank.npz); the sum is formed in the order written, every product
and every sum rounded to float32 on its own.  The tests, the golden generator
and the bench lines share this one function.
"""
import numpy as np

from comb_ref import comb_f32


def reverb_taps(rate, rt60, wet):
    """The bank of xm_effects_add_reverb: [(D, b0, bd, ad, mix)] with the gains as numpy computes them."""
    taps = []
    for ms in (29.7, 37.1, 41.1, 43.7):
        D = int(np.rint(ms * rate / 1000.0))
        taps.append((D, 0.0, 1.0, -np.float32(10.0 ** (-3.0 * D / (rate * rt60))), np.float32(wet)))
    return taps


def bank_f32(x, taps, dry, hist=None):
    """x: [frames] or [frames, C] float32 (one clip); taps: [(D, b0, bd, ad, mix), ...].  Returns y, shaped as x.

    hist: None (zero history), or (hx, [hc_0, hc_1, ...]): the max D frames of
    the stage's input and the D_k frames of every branch's output before x;
    then returns (y, (hx', [hc_k'])), the history after x.
    """
    x = np.ascontiguousarray(x, np.float32)
    Dmax = max(int(t[0]) for t in taps)
    acc = np.float32(dry) * x
    hc_out = []
    for k, (D, b0, bd, ad, mix) in enumerate(taps):
        D = int(D)
        if hist is None:
            c = comb_f32(x, D, b0, bd, ad)
        else:
            hx = np.asarray(hist[0], np.float32)
            c, (_, hc) = comb_f32(x, D, b0, bd, ad, hist=(hx[Dmax - D:], hist[1][k]))
            hc_out.append(hc)
        m = np.float32(mix) * c
        acc = acc + m
    assert acc.dtype == np.float32
    if hist is None:
        return acc
    hx = np.concatenate([np.asarray(hist[0], np.float32), x], axis=0)[-Dmax:] if Dmax else x[:0]
    return acc, (hx, hc_out)
