/*
 * xm_effects.h — biquad / FIR / comb / comb-bank effects chain over batches of clips (C ABI).
 *
 * BUILD-OWNED ABI (reference has no headers: /root/reference/README.md:1;
 * prefix xm_effects_* from BASELINE.json:5, signatures from SURVEY.md §8(b)).
 *
 * Arithmetic (pinned to scipy 1.15.3 float32):
 *  biquad section (b0,b1,b2,1,a1,a2), transposed direct form II, state zero at
 *  clip start, per channel, sections applied in insertion order:
 *      y  = b0*x + z0;  z0 = (b1*x - a1*y) + z1;  z1 = b2*x - a2*y;  x = y
 *  (scipy sosfilt, _signaltools.py:4601 / _sosfilt.pyx)
 *  FIR of K taps, causal, output length = input length:
 *      acc=+0; for t=0..K-1: acc = acc + x[n-K+1+t]*h[K-1-t]   (x<0 := 0)
 *  (scipy upfirdn(h, x)[:N], _upfirdn.py:107)
 *  comb (delay line: echo, feedback comb, Schroeder all-pass) of D frames,
 *  coefficients (b0, bd, ad), per clip on the interleaved sample stream of
 *  frames*C samples with lag Ds = D*C, so channels never mix:
 *      y[i] = b0*x[i] + ( bd*x[i-Ds] - ad*y[i-Ds] )
 *      p = b0*x[i];  q = bd*x[i-Ds];  r = ad*y[i-Ds];  t = q - r;  y[i] = p + t
 *  every operation fp32, round-to-nearest-even, separately rounded (no
 *  contraction), denormals preserved; x[i] = y[i] = +0 for i < 0 (when
 *  streaming: the carried history).  The operations are carried out as written
 *  also where an operand is the zero padding: the sign of a zero result is
 *  part of the contract.
 *  (scipy lfilter(b, a, x) in float32 with b = [b0, 0, ..., bd] and
 *  a = [1, 0, ..., ad], both of length D+1)
 *  comb bank (parallel combs: the body of a Schroeder reverberator) of n
 *  branches (D_k, b0_k, bd_k, ad_k, mix_k) and a dry weight, per clip on the
 *  interleaved sample stream with lags Ds_k = D_k*C, so channels never mix.
 *  Branch k is exactly the comb above, applied to the stage's input x:
 *      c_k[i] = b0_k*x[i] + ( bd_k*x[i-Ds_k] - ad_k*c_k[i-Ds_k] )
 *  (the same five separately rounded operations, zero history before the
 *  clip, denormals kept, signed zeros as computed; every product is formed,
 *  also one with a zero coefficient), and the output sums the branches in
 *  ascending order:
 *      acc = dry*x[i];  for k = 0 .. n-1:  m = mix_k*c_k[i];  acc = acc + m
 *      y[i] = acc
 *  every multiply and add rounded to fp32 separately, no contraction.
 *  (c_k = scipy lfilter in float32 as above; the sum in the order written)
 *  Effects run in insertion order; consecutive biquads form one cascade; a
 *  comb and a comb bank are stages of their own and never merge with their
 *  neighbours.
 */
#ifndef XM_EFFECTS_H
#define XM_EFFECTS_H

#include "xm_audio_common.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct XmEffects XmEffects;

typedef enum XmEqBand {
    XM_EQ_PEAKING   = 0,
    XM_EQ_LOWSHELF  = 1,
    XM_EQ_HIGHSHELF = 2,
    XM_EQ_LOWPASS   = 3,
    XM_EQ_HIGHPASS  = 4
} XmEqBand;

typedef struct XmEffectsConfig {
    int32_t rate;        /* Hz */
    int32_t channels;    /* 1 or 2 */
    int32_t mem_kind;    /* XmMemKind of in/out pointers */
    int32_t device;      /* HIP device ordinal, or XM_DEVICE_CPU (the host CPU backend) */
} XmEffectsConfig;

XM_API XmEffects *xm_effects_create_ex(const XmEffectsConfig *cfg, int *status);
/* Host-memory chain (SURVEY.md §8(b) form): n_devices == 0 on the host CPU
 * backend (XM_DEVICE_CPU), n_devices == 1 on GPU 0, n_devices > 1 over GPUs
 * 0 .. n_devices-1 (xm_effects_create_multi); NULL if n_devices is out of
 * [0, 16] or names a device that is not there. */
XM_API XmEffects *xm_effects_create(int rate, int channels, int n_devices);

/* Multi-device chain over an explicit device list (n_devices in [1, 16]; a
 * device may repeat).  One single-device chain and one host worker thread per
 * entry ("one host worker thread per GPU, joined before
 * process_batch returns").  Effects added to the handle reach every device.
 * process_batch / process_stream cut the clips into contiguous blocks, block
 * d (the first batch % n blocks one clip longer) on device d, and return when
 * every device is done; clips are independent, so the result equals the
 * one-device result bit for bit.  With XM_MEM_DEVICE, block d's pointers must
 * be on device d.  cfg->device is ignored; set_stream returns XM_ENOSYS.
 * Such a chain attaches to multi-device mixers (copied per device), not to a
 * single-device mixer (XM_EINVAL there).  A list of one device returns the
 * plain single-device chain on it.  An effect that cannot be added to every
 * device's chain is added to none. */
XM_API XmEffects *xm_effects_create_multi(const XmEffectsConfig *cfg, const int *devices, int n_devices,
                                          int *status);

/* Devices a chain runs on (1 for a single-device chain). */
XM_API int xm_effects_n_devices(const XmEffects *e);

/* sos = {b0, b1, b2, a0, a1, a2}; a0 must be 1 (as scipy sosfilt requires).
 * A chain holds up to 128 effects (XM_ENOMEM beyond); consecutive biquads run
 * as one cascade of up to 64 sections per pass over the clip. */
XM_API int xm_effects_add_biquad(XmEffects *e, const float sos[6]);

/* RBJ audio-EQ-cookbook section designed in fp64 and cast to fp32.
 * q is Q (peaking / pass filters) or shelf slope S (shelves). */
XM_API int xm_effects_add_eq_band(XmEffects *e, int band, double f0_hz, double gain_db, double q);

/* FIR with K taps (1 <= K <= 4096), copied. */
XM_API int xm_effects_add_fir(XmEffects *e, const float *h, int K);

/* Comb stage y[n] = b0*x[n] + (bd*x[n-D] - ad*y[n-D]) per channel (the
 * arithmetic above), 1 <= delay_frames <= XM_MAX_DELAY, finite coefficients
 * (XM_EINVAL otherwise; XM_ENOMEM beyond 128 effects).  Stability (|ad| < 1)
 * is not checked: the contract covers the arithmetic only. */
#define XM_MAX_DELAY (1 << 20)
XM_API int xm_effects_add_comb(XmEffects *e, int64_t delay_frames, float b0, float bd, float ad);

/* Echo y[n] = x[n] + wet*x[n-D] + feedback*y[n-D]: add_comb(D, 1, (float)wet,
 * -(float)feedback) with D = llrint(delay_ms * rate / 1000.0) in fp64, ties
 * to even; XM_EINVAL if D is outside [1, XM_MAX_DELAY]. */
XM_API int xm_effects_add_echo(XmEffects *e, double delay_ms, double feedback, double wet);

/* Schroeder all-pass y[n] = -g*x[n] + x[n-D] + g*y[n-D]: add_comb(D,
 * -(float)g, 1, -(float)g), D as for add_echo. */
XM_API int xm_effects_add_allpass(XmEffects *e, double delay_ms, double g);

/* Comb bank (the arithmetic above): n combs in parallel on the stage's input,
 * summed with weights mix_k onto dry*x.  1 <= n <= XM_MAX_BANK, every delay in
 * [1, XM_MAX_DELAY], every coefficient and dry finite (XM_EINVAL otherwise;
 * XM_ENOMEM beyond 128 effects).  Equal lags in several branches are legal;
 * stability is not checked.  taps is copied. */
#define XM_MAX_BANK 8
typedef struct XmCombTap {
    int64_t delay_frames;   /* 1 .. XM_MAX_DELAY */
    float b0, bd, ad;       /* the comb stage's coefficients */
    float mix;              /* weight of this branch in the sum */
} XmCombTap;
XM_API int xm_effects_add_comb_bank(XmEffects *e, const XmCombTap *taps, int n, float dry);

/* Schroeder reverberator: appends three effects, all or none.  A bank of four
 * feedback combs of 29.7, 37.1, 41.1 and 43.7 ms (D_k = llrint(ms * rate /
 * 1000.0), as add_echo), each b0 = 0, bd = 1, ad = -(float)pow(10.0,
 * -3.0 * D_k / (rate * rt60_s)) (the loop gain that decays by 60 dB in
 * rt60_s seconds), mix = (float)wet, the bank's dry = (float)dry; then
 * add_allpass(5.0 ms, 0.7) and add_allpass(1.7 ms, 0.7).  XM_EINVAL unless
 * rt60_s is finite and > 0, dry and wet are finite and every delay rounds into
 * [1, XM_MAX_DELAY]; XM_ENOMEM when the chain has no room for three effects.
 * The dry signal passes the two all-passes too (their magnitude response is
 * flat, their phase is not): for an untouched dry path run the reverb with
 * dry = 0 on a send track and sum it with the dry track in the mixer. */
XM_API int xm_effects_add_reverb(XmEffects *e, double rt60_s, double dry, double wet);

/* Number of effects and the coefficients of biquad i (for inspection). */
XM_API int xm_effects_count(const XmEffects *e);
XM_API int xm_effects_get_biquad(const XmEffects *e, int index, float sos[6]);
/* Delay and coef = {b0, bd, ad} of comb i; XM_EINVAL when effect i is not a comb. */
XM_API int xm_effects_get_comb(const XmEffects *e, int index, int64_t *delay_frames, float coef[3]);
/* Taps, their number and the dry weight of comb bank i; XM_EINVAL when effect
 * i is not a bank (get_comb on a bank returns XM_EINVAL as well). */
XM_API int xm_effects_get_comb_bank(const XmEffects *e, int index, XmCombTap taps[XM_MAX_BANK], int *n, float *dry);

/* Install a caller-owned hipStream_t (NULL: the chain's own stream, which is
 * created blocking: ordered after the legacy default stream's work, as a
 * synchronous caller expects).  A CPU chain accepts and ignores it. */
XM_API int xm_effects_set_stream(XmEffects *e, void *hip_stream);

/* in/out: batch pointers of frames*channels float32 samples (in == out allowed). */
XM_API int xm_effects_process_batch(XmEffects *e, const float *const *in, float *const *out,
                             size_t batch, size_t frames);

/* ---- streaming (build-owned) ----------------------
 * n_clips long signals fed in blocks.  xm_effects_stream_reset() (re)starts
 * n_clips streams at zero state for the chain as it is now; every
 * xm_effects_process_stream() call filters the next `frames` frames of each
 * stream (in[i] / out[i] as process_batch, in == out allowed), carrying on
 * the device the biquad state (z0, z1 per section and channel), the last
 * K-1 input frames of every FIR stage, the last D input and D output
 * frames of every comb stage and, of every comb bank, the last D_k output
 * frames of each branch and the last max D_k input frames.  Any split of a signal into blocks (ragged,
 * 1-frame or empty blocks, longer or shorter than D) gives, bit for bit, the output of one
 * process_batch() over the whole signal.  Adding an effect ends the streams:
 * process_stream then fails with XM_EINVAL until the next reset, as it does
 * for an n_clips other than the reset's. */
XM_API int xm_effects_stream_reset(XmEffects *e, size_t n_clips);
XM_API int xm_effects_process_stream(XmEffects *e, const float *const *in, float *const *out,
                              size_t n_clips, size_t frames);

XM_API void xm_effects_freep(XmEffects **e);

#ifdef __cplusplus
}
#endif
#endif /* XM_EFFECTS_H */
