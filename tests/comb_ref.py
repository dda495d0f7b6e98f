"""Reference of the comb stage (include/xm_effects.h), numpy float32.

    y[i] = b0*x[i] + ( bd*x[i-Ds] - ad*y[i-Ds] ),   Ds = D * channels

on the interleaved sample stream of one clip, every operation rounded
separately to float32: p = b0*x, q = bd*x[i-Ds], r = ad*y[i-Ds], t = q - r,
y = p + t.  Position p of [0, Ds) depends only on position p of the previous
block of Ds samples, so the restatement is vectorised over a block.  It equals
scipy.signal.lfilter([b0, 0.., bd], [1, 0.., ad], x) in float32 bit for bit
(tools/gen_golden_comb.py asserts that before it writes tests/golden/comb.npz).
The tests, the golden generator and the bench line share this one function.
"""
import numpy as np


def comb_f32(x, D, b0, bd, ad, hist=None):
    """x: [frames] or [frames, C] float32 (one clip).  Returns y, shaped as x.

    hist: None (zero history), or (hx, hy): the D frames of the stage's input
    and of its output before x, each shaped [D] / [D, C]; then returns
    (y, (hx', hy')), the history after x (the last D frames of hist ++ x).
    """
    x = np.ascontiguousarray(x, np.float32)
    b0, bd, ad = np.float32(b0), np.float32(bd), np.float32(ad)
    C = 1 if x.ndim == 1 else x.shape[1]
    Ds = int(D) * C
    s = x.reshape(-1)
    n = s.size
    if hist is None:
        px, py = np.zeros(Ds, np.float32), np.zeros(Ds, np.float32)
    else:
        px = np.array(hist[0], np.float32).reshape(-1)
        py = np.array(hist[1], np.float32).reshape(-1)
        assert px.size == Ds and py.size == Ds
    y = np.empty(n, np.float32)
    for s0 in range(0, n, Ds):
        m = min(Ds, n - s0)
        xv = s[s0:s0 + m]
        p = b0 * xv
        q = bd * px[:m]
        r = ad * py[:m]
        t = q - r
        o = p + t
        px[:m] = xv
        py[:m] = o
        y[s0:s0 + m] = o
    y = y.reshape(x.shape)
    if hist is None:
        return y
    # position p holds its chain's newest sample: slot (p - n) mod Ds of the history
    hshape = (int(D),) if x.ndim == 1 else (int(D), C)
    return y, (np.roll(px, -(n % Ds)).reshape(hshape), np.roll(py, -(n % Ds)).reshape(hshape))
