"""The comb stage (echo, feedback comb, all-pass; include/xm_effects.h) on the
CPU backend, and its host-side API: bit for bit scipy lfilter in float32
(tests/golden/comb.npz) and tests/comb_ref.py.  No GPU."""
import numpy as np
import pytest

from conftest import bits_equal

import comb_cases as K
from comb_ref import comb_f32

N = 1200


def make(xm):
    return lambda C, rate=44100: xm.Effects(rate, C, device="cpu")


def test_comb_golden_manifest():
    """comb.npz is the file tools/gen_golden_comb.py wrote (its own manifest)."""
    import hashlib
    import json
    import os
    from conftest import GOLDEN
    with open(os.path.join(GOLDEN, "MANIFEST_comb.json")) as fh:
        want = json.load(fh)["files"]["comb.npz"]
    with open(os.path.join(GOLDEN, "comb.npz"), "rb") as fh:
        data = fh.read()
    assert len(data) == want["bytes"] and hashlib.sha256(data).hexdigest() == want["sha256"]


def test_cpu_comb_golden(xm):
    n = 0
    for name, D, coef, x, want in K.golden_cases():
        e = xm.Effects(44100, x.shape[1], device="cpu")
        e.add_comb(D, *coef)
        assert bits_equal(e.process(x[None].copy())[0], want), name
        assert bits_equal(comb_f32(x, D, *coef), want), name
        n += 1
    assert n >= 12


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("D", [1, 2, 3, 15, 16, 17, 100, 1001, N, N + 300])
def test_cpu_comb_vs_ref(xm, C, D):
    """every lag on 1, 3 and 17 clips, out of place and in place (D == frames
    and D > frames: the block is all zero padding or carried history)"""
    want = K.comb_ref_clips(C, N, D)
    e = xm.Effects(44100, C, device="cpu")
    e.add_comb(D, *K.COEF)
    for B in (1, 3, 17):
        x = K.clips(C, N)[:B]
        assert bits_equal(e.process(x.copy()), want[:B]), (B, "out of place")
        assert bits_equal(e.process(x.copy(), inplace=True), want[:B]), (B, "in place")


def test_cpu_comb_signed_zeros(xm):
    K.check_signed_zeros(make(xm))


def test_cpu_comb_mixed_chains(xm):
    K.check_mixed_chains(make(xm))


def test_cpu_comb_streaming(xm):
    K.check_streaming(make(xm))


def test_echo_and_allpass_map_to_comb(xm):
    e = xm.Effects(32000, 2, device="cpu")
    # delay_ms * 32 lands on k + 0.5 exactly: llrint rounds ties to even
    for ms, D in ((0.046875, 2), (0.078125, 2), (0.109375, 4), (250.0, 8000)):
        i = e.count()
        e.add_echo(ms, 0.45, 0.5)
        d, c = e.comb(i)
        assert d == D and bits_equal(c, np.array([1.0, np.float32(0.5), -np.float32(0.45)], np.float32)), (ms, d, c)
        e.add_allpass(ms, 0.7)
        d, c = e.comb(i + 1)
        assert d == D and bits_equal(c, np.array([-np.float32(0.7), 1.0, -np.float32(0.7)], np.float32)), (ms, d, c)
    e.add_comb(xm.XM_MAX_DELAY, 1.0, 0.5, 0.25)
    d, c = e.comb(e.count() - 1)
    assert d == xm.XM_MAX_DELAY and bits_equal(c, np.array([1.0, 0.5, 0.25], np.float32))
    # what add_echo documents is what runs
    x = K.clips(2, N)[:2]
    e2 = xm.Effects(32000, 2, device="cpu")
    e2.add_echo(0.109375, 0.45, 0.5)
    assert bits_equal(e2.process(x.copy()), K.comb_batch(x, 4, (1.0, np.float32(0.5), -np.float32(0.45))))


def test_comb_argument_errors(xm):
    e = xm.Effects(44100, 2, device="cpu")
    bad = [lambda: e.add_comb(0, 1.0, 0.5, 0.5), lambda: e.add_comb(-3, 1.0, 0.5, 0.5),
           lambda: e.add_comb(xm.XM_MAX_DELAY + 1, 1.0, 0.5, 0.5),
           lambda: e.add_comb(10, float("nan"), 0.5, 0.5), lambda: e.add_comb(10, 1.0, float("inf"), 0.5),
           lambda: e.add_comb(10, 1.0, 0.5, float("nan")),
           lambda: e.add_echo(0.0, 0.5, 0.5), lambda: e.add_echo(0.01, 0.5, 0.5),      # D = llrint(0.441) = 0
           lambda: e.add_echo(1e9, 0.5, 0.5), lambda: e.add_echo(float("nan"), 0.5, 0.5),
           lambda: e.add_echo(10.0, float("nan"), 0.5), lambda: e.add_allpass(0.0, 0.5),
           lambda: e.add_allpass(1e9, 0.5), lambda: e.add_allpass(10.0, float("inf"))]
    for f in bad:
        with pytest.raises(xm.XmError) as err:
            f()
        assert err.value.code == xm.XM_EINVAL
    assert e.count() == 0
    e.add_biquad([1.0, 0.0, 0.0, 1.0, 0.0, 0.0])
    e.add_comb(10, 1.0, 0.5, 0.5)
    with pytest.raises(xm.XmError) as err:
        e.comb(0)                                  # effect 0 is a biquad
    assert err.value.code == xm.XM_EINVAL
    with pytest.raises(xm.XmError):
        e.biquad(1)                                # effect 1 is a comb
    with pytest.raises(xm.XmError):
        e.comb(2)
    for _ in range(126):
        e.add_comb(3, 1.0, 0.5, 0.5)
    assert e.count() == 128
    for f in (lambda: e.add_comb(3, 1.0, 0.5, 0.5), lambda: e.add_echo(10.0, 0.5, 0.5),
              lambda: e.add_allpass(10.0, 0.5)):
        with pytest.raises(xm.XmError) as err:     # the 129th effect
            f()
        assert err.value.code == xm.XM_ENOMEM


def test_cpu_mixer_track_effects_with_comb(xm):
    K.check_mixer(xm, device="cpu")
