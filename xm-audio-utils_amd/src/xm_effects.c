/*
 * xm_effects.c — the xm_effects_* C API: chain construction (biquad sections,
 * RBJ EQ bands designed in fp64, FIR taps, comb / delay-line stages, comb
 * banks and the reverb preset built from them), staging and dispatch of the
 * gfx950 effects kernels (csrc/xm_fx.hip).  Build-owned API (reference has
 * none: /root/reference/README.md:1); contract in include/xm_effects.h.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "xm_internal.h"

struct XmEffects {
    XmEffectsConfig cfg;
    int n_effects;
    struct {
        int kind;          /* 1 biquad section, 2 FIR, 3 comb, 4 comb bank */
        int n;             /* taps for FIR, branches for a bank */
        float sos[6];      /* comb: b0, bd, ad in sos[0..2]; bank: dry in sos[0] */
        float *fir;        /* host copy */
        int64_t delay;     /* comb: D frames */
        XmCombTap *bank;   /* bank: host copy of the n branches */
    } fx[XM_MAX_EFFECTS];
    XmFxStage stages[XM_MAX_EFFECTS];
    int n_stages;
    int dirty;
    void *own_stream, *stream;
    int user_stream;
    void *d_buf[2];
    size_t d_cap[2];
    void **d_ptrs;
    void **h_ptrs;
    size_t ptr_cap;
    /* streaming state (xm_effects_stream_reset): per stage, biquad
     * [clip][section][z0,z1][ch] in st[s][0]; FIR [clip][K-1][ch] history
     * ping-ponging between st[s][0] and st[s][1] (st_cur[s] = current); comb
     * [clip][x,y][D][ch] history (the last D frames of the stage's input and
     * of its output), ping-ponging the same way; comb bank [clip] the last
     * D_k frames of every branch's output, k ascending, then the last max D_k
     * frames of the stage's input (csrc/xm_shim.h bank_hist_in), ping-ponging
     * as well */
    float *st[XM_MAX_EFFECTS][2];
    int st_cur[XM_MAX_EFFECTS];
    size_t st_clips;
    int st_ready;
    /* delay lines of comb banks too long for the LDS (csrc/xm_fx_bank.hip):
     * one buffer, shared by the chain's bank stages, which run in stream order */
    void *bank_scr;
    size_t bank_scr_cap;
    /* multi-device chain (xm_effects_create_multi / n_devices > 1): one
     * single-device chain per entry of devs, a worker thread per device
     * (src/xm_pool.c); a batch's clips are cut into contiguous blocks, block
     * d on devs[d].  Clips are independent, so the result is the one-device
     * result bit for bit.  The parent keeps the effect list (fx[]) and no
     * device resources of its own. */
    int n_sub;
    int devs[XM_MAX_DEVICES];
    XmEffects *sub[XM_MAX_DEVICES];
    XmPool *pool;
    size_t st_first[XM_MAX_DEVICES], st_cnt[XM_MAX_DEVICES];
};

XmEffects *xm_effects_create_ex(const XmEffectsConfig *cfg, int *status)
{
    int rc = XM_OK;
    XmEffects *e = NULL;
    if (!cfg || cfg->rate <= 0 || (cfg->channels != 1 && cfg->channels != 2) ||
        (cfg->mem_kind != XM_MEM_HOST && cfg->mem_kind != XM_MEM_DEVICE) ||
        (cfg->device < 0 && cfg->device != XM_DEVICE_CPU)) {
        rc = XM_EINVAL;
        goto out;
    }
    if (cfg->device != XM_DEVICE_CPU && cfg->device >= xmh_device_count()) {
        rc = XM_EDEVICE;
        goto out;
    }
    e = calloc(1, sizeof *e);
    if (!e) {
        rc = XM_ENOMEM;
        goto out;
    }
    e->cfg = *cfg;
    if (cfg->device == XM_DEVICE_CPU) e->cfg.mem_kind = XM_MEM_DEVICE;   /* host memory is the CPU's: no staging */
    if ((rc = xmh_set_device(cfg->device))) goto out;
    if ((rc = xmh_stream_create(&e->own_stream))) goto out;
    e->stream = e->own_stream;
out:
    if (rc) xm_effects_freep(&e);
    if (status) *status = rc;
    return e;
}

XmEffects *xm_effects_create_multi(const XmEffectsConfig *cfg, const int *devices, int n_devices, int *status)
{
    int rc = XM_OK;
    XmEffects *e = NULL;
    if (!cfg || !devices || n_devices < 1 || n_devices > XM_MAX_DEVICES || cfg->rate <= 0 ||
        (cfg->channels != 1 && cfg->channels != 2) || (cfg->mem_kind != XM_MEM_HOST && cfg->mem_kind != XM_MEM_DEVICE)) {
        rc = XM_EINVAL;
        goto out;
    }
    for (int d = 0; d < n_devices; ++d)
        if (devices[d] < 0 || devices[d] >= xmh_device_count()) {
            rc = XM_EDEVICE;
            goto out;
        }
    if (n_devices == 1) {   /* one device: the plain single-device chain (set_stream, single-device mixers) */
        XmEffectsConfig c = *cfg;
        c.device = devices[0];
        return xm_effects_create_ex(&c, status);
    }
    e = calloc(1, sizeof *e);
    if (!e) {
        rc = XM_ENOMEM;
        goto out;
    }
    e->cfg = *cfg;
    e->cfg.device = devices[0];
    e->n_sub = n_devices;
    for (int d = 0; d < n_devices && !rc; ++d) {
        XmEffectsConfig c = *cfg;
        c.device = e->devs[d] = devices[d];
        e->sub[d] = xm_effects_create_ex(&c, &rc);
    }
    if (!rc) e->pool = xm_pool_create(n_devices, e, &rc);
out:
    if (rc) xm_effects_freep(&e);
    if (status) *status = rc;
    return e;
}

XmEffects *xm_effects_create(int rate, int channels, int n_devices)
{
    XmEffectsConfig c = {rate, channels, XM_MEM_HOST, 0};
    if (n_devices < 0 || n_devices > XM_MAX_DEVICES) return NULL;
    if (n_devices == 0) c.device = XM_DEVICE_CPU;   /* 0 = the host CPU backend */
    if (n_devices <= 1) return xm_effects_create_ex(&c, NULL);
    int devs[XM_MAX_DEVICES];
    for (int d = 0; d < n_devices; ++d) devs[d] = d;
    return xm_effects_create_multi(&c, devs, n_devices, NULL);
}

int xm_effects_n_devices(const XmEffects *e)
{
    if (!e) return XM_EINVAL;
    return e->n_sub ? e->n_sub : 1;
}

int xm_effects_is_multi(const XmEffects *e) { return e && e->n_sub > 0; }

static void free_stream_state(XmEffects *e)
{
    for (int i = 0; i < XM_MAX_EFFECTS; ++i)
        for (int k = 0; k < 2; ++k) {
            xmh_free(e->st[i][k]);
            e->st[i][k] = NULL;
        }
    e->st_ready = 0;
    e->st_clips = 0;
}

static void free_stages(XmEffects *e)
{
    for (int i = 0; i < e->n_stages; ++i) xmh_free(e->stages[i].coef_dev);
    e->n_stages = 0;
    free_stream_state(e);   /* streams belong to the chain they were started on */
}

void xm_effects_freep(XmEffects **pe)
{
    if (!pe || !*pe) return;
    XmEffects *e = *pe;
    if (e->n_sub) {
        xm_pool_free(&e->pool);
        for (int d = 0; d < e->n_sub; ++d) xm_effects_freep(&e->sub[d]);
        for (int i = 0; i < e->n_effects; ++i) {
            free(e->fx[i].fir);
            free(e->fx[i].bank);
        }
        free(e);
        *pe = NULL;
        return;
    }
    xmh_set_device(e->cfg.device);
    if (e->own_stream) xmh_stream_sync(e->own_stream);
    free_stages(e);
    free_stream_state(e);
    for (int i = 0; i < e->n_effects; ++i) {
        free(e->fx[i].fir);
        free(e->fx[i].bank);
    }
    xmh_free(e->bank_scr);
    xmh_free(e->d_buf[0]);
    xmh_free(e->d_buf[1]);
    xmh_free(e->d_ptrs);
    xmh_host_free(e->h_ptrs);
    xmh_stream_destroy(e->own_stream);
    free(e);
    *pe = NULL;
}

/* undo the effect just added to sub-chains 0 .. n-1 of a multi-device chain */
static void drop_last(XmEffects *e, int n)
{
    for (int d = 0; d < n; ++d) {
        XmEffects *s = e->sub[d];
        if (s->n_effects == 0) continue;
        s->n_effects--;
        free(s->fx[s->n_effects].fir);
        s->fx[s->n_effects].fir = NULL;
        free(s->fx[s->n_effects].bank);
        s->fx[s->n_effects].bank = NULL;
        s->dirty = 1;
    }
}

int xm_effects_add_biquad(XmEffects *e, const float sos[6])
{
    if (!e || !sos) return XM_EINVAL;
    if (sos[3] != 1.0f) return XM_EINVAL;   /* scipy sosfilt requires a0 == 1 */
    for (int i = 0; i < 6; ++i)
        if (!isfinite(sos[i])) return XM_EINVAL;
    if (e->n_effects >= XM_MAX_EFFECTS) return XM_ENOMEM;
    /* a cascade longer than XM_MAX_SOS sections is split by the stager */
    for (int d = 0; d < e->n_sub; ++d) {   /* multi-device: every device's chain */
        const int rc = xm_effects_add_biquad(e->sub[d], sos);
        if (rc) {
            drop_last(e, d);   /* every device keeps the same chain */
            return rc;
        }
    }
    e->fx[e->n_effects].kind = 1;
    e->fx[e->n_effects].fir = NULL;
    e->fx[e->n_effects].bank = NULL;
    memcpy(e->fx[e->n_effects].sos, sos, sizeof(float) * 6);
    e->n_effects++;
    e->dirty = 1;
    return XM_OK;
}

/* RBJ audio-EQ-cookbook (R. Bristow-Johnson), fp64, normalised by a0, cast to
 * fp32.  Mirrored by oracle/np_oracle.py:rbj_section for the parity tests. */
int xm_effects_add_eq_band(XmEffects *e, int band, double f0, double gain_db, double q)
{
    if (!e || f0 <= 0.0 || f0 >= 0.5 * e->cfg.rate || q <= 0.0 || !isfinite(gain_db)) return XM_EINVAL;
    const double A = pow(10.0, gain_db / 40.0);
    const double w0 = 2.0 * 3.141592653589793 * f0 / (double)e->cfg.rate;
    const double cw = cos(w0), sw = sin(w0);
    double alpha, b[3], a[3];
    if (band == XM_EQ_LOWSHELF || band == XM_EQ_HIGHSHELF)
        alpha = sw / 2.0 * sqrt((A + 1.0 / A) * (1.0 / q - 1.0) + 2.0);
    else
        alpha = sw / (2.0 * q);
    switch (band) {
    case XM_EQ_PEAKING:
        b[0] = 1 + alpha * A; b[1] = -2 * cw; b[2] = 1 - alpha * A;
        a[0] = 1 + alpha / A; a[1] = -2 * cw; a[2] = 1 - alpha / A;
        break;
    case XM_EQ_LOWSHELF: {
        const double sa = 2 * sqrt(A) * alpha;
        b[0] = A * ((A + 1) - (A - 1) * cw + sa); b[1] = 2 * A * ((A - 1) - (A + 1) * cw);
        b[2] = A * ((A + 1) - (A - 1) * cw - sa);
        a[0] = (A + 1) + (A - 1) * cw + sa; a[1] = -2 * ((A - 1) + (A + 1) * cw);
        a[2] = (A + 1) + (A - 1) * cw - sa;
        break;
    }
    case XM_EQ_HIGHSHELF: {
        const double sa = 2 * sqrt(A) * alpha;
        b[0] = A * ((A + 1) + (A - 1) * cw + sa); b[1] = -2 * A * ((A - 1) + (A + 1) * cw);
        b[2] = A * ((A + 1) + (A - 1) * cw - sa);
        a[0] = (A + 1) - (A - 1) * cw + sa; a[1] = 2 * ((A - 1) - (A + 1) * cw);
        a[2] = (A + 1) - (A - 1) * cw - sa;
        break;
    }
    case XM_EQ_LOWPASS:
        b[0] = (1 - cw) / 2; b[1] = 1 - cw; b[2] = (1 - cw) / 2;
        a[0] = 1 + alpha; a[1] = -2 * cw; a[2] = 1 - alpha;
        break;
    case XM_EQ_HIGHPASS:
        b[0] = (1 + cw) / 2; b[1] = -(1 + cw); b[2] = (1 + cw) / 2;
        a[0] = 1 + alpha; a[1] = -2 * cw; a[2] = 1 - alpha;
        break;
    default:
        return XM_EINVAL;
    }
    const float sos[6] = {(float)(b[0] / a[0]), (float)(b[1] / a[0]), (float)(b[2] / a[0]), 1.0f,
                          (float)(a[1] / a[0]), (float)(a[2] / a[0])};
    return xm_effects_add_biquad(e, sos);
}

int xm_effects_add_fir(XmEffects *e, const float *h, int K)
{
    if (!e || !h || K < 1 || K > XM_MAX_FIR) return XM_EINVAL;
    if (e->n_effects >= XM_MAX_EFFECTS) return XM_ENOMEM;
    float *c = malloc(sizeof(float) * (size_t)K);   /* the parent's copy first: nothing to undo if it fails */
    if (!c) return XM_ENOMEM;
    for (int d = 0; d < e->n_sub; ++d) {   /* multi-device: every device's chain */
        const int rc = xm_effects_add_fir(e->sub[d], h, K);
        if (rc) {
            drop_last(e, d);   /* every device keeps the same chain */
            free(c);
            return rc;
        }
    }
    memcpy(c, h, sizeof(float) * (size_t)K);
    e->fx[e->n_effects].kind = 2;
    e->fx[e->n_effects].n = K;
    e->fx[e->n_effects].fir = c;
    e->fx[e->n_effects].bank = NULL;
    e->n_effects++;
    e->dirty = 1;
    return XM_OK;
}

int xm_effects_add_comb(XmEffects *e, int64_t delay_frames, float b0, float bd, float ad)
{
    if (!e || delay_frames < 1 || delay_frames > XM_MAX_DELAY) return XM_EINVAL;
    if (!isfinite(b0) || !isfinite(bd) || !isfinite(ad)) return XM_EINVAL;
    if (e->n_effects >= XM_MAX_EFFECTS) return XM_ENOMEM;
    for (int d = 0; d < e->n_sub; ++d) {   /* multi-device: every device's chain */
        const int rc = xm_effects_add_comb(e->sub[d], delay_frames, b0, bd, ad);
        if (rc) {
            drop_last(e, d);   /* every device keeps the same chain */
            return rc;
        }
    }
    e->fx[e->n_effects].kind = 3;
    e->fx[e->n_effects].n = 0;
    e->fx[e->n_effects].fir = NULL;
    e->fx[e->n_effects].bank = NULL;
    e->fx[e->n_effects].delay = delay_frames;
    e->fx[e->n_effects].sos[0] = b0;
    e->fx[e->n_effects].sos[1] = bd;
    e->fx[e->n_effects].sos[2] = ad;
    e->n_effects++;
    e->dirty = 1;
    return XM_OK;
}

/* D = llrint(delay_ms * rate / 1000) in fp64, ties to even (the default
 * rounding mode); 0 when that is outside [1, XM_MAX_DELAY] */
static int64_t delay_frames_of(const XmEffects *e, double delay_ms)
{
    const double d = delay_ms * (double)e->cfg.rate / 1000.0;
    if (!(d >= 0.5 && d <= (double)XM_MAX_DELAY + 0.5)) return 0;   /* NaN too */
    const long long D = llrint(d);
    return D >= 1 && D <= XM_MAX_DELAY ? (int64_t)D : 0;
}

int xm_effects_add_echo(XmEffects *e, double delay_ms, double feedback, double wet)
{
    if (!e) return XM_EINVAL;
    const int64_t D = delay_frames_of(e, delay_ms);
    if (!D) return XM_EINVAL;
    return xm_effects_add_comb(e, D, 1.0f, (float)wet, -(float)feedback);
}

int xm_effects_add_allpass(XmEffects *e, double delay_ms, double g)
{
    if (!e) return XM_EINVAL;
    const int64_t D = delay_frames_of(e, delay_ms);
    if (!D) return XM_EINVAL;
    return xm_effects_add_comb(e, D, -(float)g, 1.0f, -(float)g);
}

int xm_effects_add_comb_bank(XmEffects *e, const XmCombTap *taps, int n, float dry)
{
    if (!e || !taps || n < 1 || n > XM_MAX_BANK || !isfinite(dry)) return XM_EINVAL;
    for (int k = 0; k < n; ++k) {
        if (taps[k].delay_frames < 1 || taps[k].delay_frames > XM_MAX_DELAY) return XM_EINVAL;
        if (!isfinite(taps[k].b0) || !isfinite(taps[k].bd) || !isfinite(taps[k].ad) || !isfinite(taps[k].mix))
            return XM_EINVAL;
    }
    if (e->n_effects >= XM_MAX_EFFECTS) return XM_ENOMEM;
    XmCombTap *c = malloc(sizeof(XmCombTap) * (size_t)n);   /* the parent's copy first: nothing to undo if it fails */
    if (!c) return XM_ENOMEM;
    for (int d = 0; d < e->n_sub; ++d) {   /* multi-device: every device's chain */
        const int rc = xm_effects_add_comb_bank(e->sub[d], taps, n, dry);
        if (rc) {
            drop_last(e, d);   /* every device keeps the same chain */
            free(c);
            return rc;
        }
    }
    memcpy(c, taps, sizeof(XmCombTap) * (size_t)n);
    e->fx[e->n_effects].kind = 4;
    e->fx[e->n_effects].n = n;
    e->fx[e->n_effects].fir = NULL;
    e->fx[e->n_effects].bank = c;
    e->fx[e->n_effects].sos[0] = dry;
    e->n_effects++;
    e->dirty = 1;
    return XM_OK;
}

/* undo the last effect of the chain (and of every sub-chain) */
static void pop_effect(XmEffects *e)
{
    drop_last(e, e->n_sub);
    e->n_effects--;
    free(e->fx[e->n_effects].fir);
    e->fx[e->n_effects].fir = NULL;
    free(e->fx[e->n_effects].bank);
    e->fx[e->n_effects].bank = NULL;
    e->dirty = 1;
}

int xm_effects_add_reverb(XmEffects *e, double rt60_s, double dry, double wet)
{
    static const double comb_ms[4] = {29.7, 37.1, 41.1, 43.7}, ap_ms[2] = {5.0, 1.7};
    if (!e || !isfinite(rt60_s) || !(rt60_s > 0.0) || !isfinite(dry) || !isfinite(wet)) return XM_EINVAL;
    XmCombTap t[4];
    for (int k = 0; k < 4; ++k) {
        const int64_t D = delay_frames_of(e, comb_ms[k]);
        if (!D) return XM_EINVAL;
        t[k].delay_frames = D;
        t[k].b0 = 0.0f;
        t[k].bd = 1.0f;
        t[k].ad = -(float)pow(10.0, -3.0 * (double)D / ((double)e->cfg.rate * rt60_s));
        t[k].mix = (float)wet;
    }
    for (int k = 0; k < 2; ++k)
        if (!delay_frames_of(e, ap_ms[k])) return XM_EINVAL;
    if (!isfinite((float)dry) || !isfinite((float)wet)) return XM_EINVAL;   /* finite in fp64, not in fp32 */
    if (e->n_effects + 3 > XM_MAX_EFFECTS) return XM_ENOMEM;
    int rc = xm_effects_add_comb_bank(e, t, 4, (float)dry);
    if (rc) return rc;
    for (int k = 0; k < 2; ++k) {
        rc = xm_effects_add_allpass(e, ap_ms[k], 0.7);
        if (rc) {   /* all or none */
            for (int u = 0; u <= k; ++u) pop_effect(e);
            return rc;
        }
    }
    return XM_OK;
}

int xm_effects_count(const XmEffects *e) { return e ? e->n_effects : XM_EINVAL; }

int xm_effects_get_comb_bank(const XmEffects *e, int i, XmCombTap taps[XM_MAX_BANK], int *n, float *dry)
{
    if (!e || !taps || !n || !dry || i < 0 || i >= e->n_effects || e->fx[i].kind != 4) return XM_EINVAL;
    memcpy(taps, e->fx[i].bank, sizeof(XmCombTap) * (size_t)e->fx[i].n);
    *n = e->fx[i].n;
    *dry = e->fx[i].sos[0];
    return XM_OK;
}

int xm_effects_get_comb(const XmEffects *e, int i, int64_t *delay_frames, float coef[3])
{
    if (!e || !delay_frames || !coef || i < 0 || i >= e->n_effects || e->fx[i].kind != 3) return XM_EINVAL;
    *delay_frames = e->fx[i].delay;
    memcpy(coef, e->fx[i].sos, sizeof(float) * 3);
    return XM_OK;
}

int xm_effects_get_biquad(const XmEffects *e, int i, float sos[6])
{
    if (!e || !sos || i < 0 || i >= e->n_effects || e->fx[i].kind != 1) return XM_EINVAL;
    memcpy(sos, e->fx[i].sos, sizeof(float) * 6);
    return XM_OK;
}

int xm_effects_set_stream(XmEffects *e, void *s)
{
    if (!e) return XM_EINVAL;
    if (e->n_sub) return XM_ENOSYS;   /* one stream per device, owned by the sub-chains */
    if (e->cfg.device == XM_DEVICE_CPU) return XM_OK;   /* CPU calls are synchronous */
    e->stream = s ? s : e->own_stream;
    e->user_stream = s != NULL;
    return XM_OK;
}

/* the chain's device (XM_DEVICE_CPU for a CPU chain); a multi-device chain has none */
int xm_effects_device(const XmEffects *e) { return e && !e->n_sub ? e->cfg.device : XM_DEVICE_NONE_; }

XmEffects *xm_effects_clone_on(const XmEffects *src, int device, int *status)
{
    XmEffectsConfig c = src->cfg;
    c.device = device;
    int rc = XM_OK;
    XmEffects *e = xm_effects_create_ex(&c, &rc);
    for (int i = 0; e && !rc && i < src->n_effects; ++i) {
        if (src->fx[i].kind == 1) rc = xm_effects_add_biquad(e, src->fx[i].sos);
        else if (src->fx[i].kind == 2) rc = xm_effects_add_fir(e, src->fx[i].fir, src->fx[i].n);
        else if (src->fx[i].kind == 4) rc = xm_effects_add_comb_bank(e, src->fx[i].bank, src->fx[i].n, src->fx[i].sos[0]);
        else rc = xm_effects_add_comb(e, src->fx[i].delay, src->fx[i].sos[0], src->fx[i].sos[1], src->fx[i].sos[2]);
    }
    if (rc) xm_effects_freep(&e);
    if (status) *status = rc;
    return e;
}

/* Group consecutive biquads into cascades (<= XM_MAX_SOS sections each) and
 * upload coefficients.  A comb is a stage of its own (no device buffer: its
 * coefficients travel in the job). */
static int build_stages(XmEffects *e)
{
    if (!e->dirty) return XM_OK;
    xmh_set_device(e->cfg.device);
    free_stages(e);
    int rc = XM_OK;
    for (int i = 0; !rc && i < e->n_effects;) {
        XmFxStage *s = &e->stages[e->n_stages];
        if (e->fx[i].kind == 1) {
            float buf[6 * XM_MAX_SOS];
            int n = 0;
            while (i < e->n_effects && e->fx[i].kind == 1 && n < XM_MAX_SOS) {
                memcpy(buf + 6 * n, e->fx[i].sos, sizeof(float) * 6);
                ++n;
                ++i;
            }
            s->kind = 1;
            s->n = n;
            rc = xmh_malloc((void **)&s->coef_dev, sizeof(float) * 6 * (size_t)n);
            if (!rc) rc = xmh_memcpy_h2d(s->coef_dev, buf, sizeof(float) * 6 * (size_t)n, e->stream);
        } else if (e->fx[i].kind == 3) {
            s->kind = 3;
            s->n = 0;
            s->coef_dev = NULL;
            s->delay = e->fx[i].delay;
            memcpy(s->comb, e->fx[i].sos, sizeof(float) * 3);
            ++i;
        } else if (e->fx[i].kind == 4) {
            s->kind = 4;
            s->n = e->fx[i].n;
            s->coef_dev = NULL;
            s->bank_dry = e->fx[i].sos[0];
            memcpy(s->bank, e->fx[i].bank, sizeof(XmCombTap) * (size_t)s->n);
            ++i;
        } else {
            s->kind = 2;
            s->n = e->fx[i].n;
            /* at least 16 floats, zero past the taps: the FIR kernel loads
             * coefficients in 14-tap blocks (csrc/xm_fx.hip k_fir_rb) */
            const size_t nc = s->n < 16 ? 16 : (size_t)s->n;
            float *hc = calloc(nc, sizeof(float));
            if (!hc) rc = XM_ENOMEM;
            if (!rc) {
                memcpy(hc, e->fx[i].fir, sizeof(float) * (size_t)s->n);
                rc = xmh_malloc((void **)&s->coef_dev, sizeof(float) * nc);
            }
            if (!rc) rc = xmh_memcpy_h2d(s->coef_dev, hc, sizeof(float) * nc, e->stream);
            if (!rc) rc = xmh_stream_sync(e->stream);   /* hc is pageable host memory */
            free(hc);
            ++i;
        }
        if (!rc) e->n_stages++;
    }
    if (!rc) rc = xmh_stream_sync(e->stream);
    if (!rc) e->dirty = 0;
    return rc;
}

int xm_effects_stages(const XmEffects *ce, const XmFxStage **stages, int *n)
{
    XmEffects *e = (XmEffects *)ce;   /* lazily built cache */
    if (e->n_sub) return XM_EINVAL;   /* a multi-device chain has no stages of its own */
    int rc = build_stages(e);
    if (rc) return rc;
    *stages = e->stages;
    *n = e->n_stages;
    return XM_OK;
}

static int grow(void **p, size_t *cap, size_t need)
{
    if (*cap >= need) return XM_OK;
    xmh_free(*p);
    *p = NULL;
    *cap = 0;
    int rc = xmh_malloc(p, need);
    if (!rc) *cap = need;
    return rc;
}

int xm_effects_bank_job(const XmEffects *ce, const XmFxStage *s, XmhFxJob *j)
{
    XmEffects *e = (XmEffects *)ce;   /* the scratch is a lazily grown cache, like the stages */
    j->bank_n = s->n;
    j->bank_dry = s->bank_dry;
    for (int k = 0; k < s->n; ++k) {
        j->bank_taps[k].delay = s->bank[k].delay_frames;
        j->bank_taps[k].b0 = s->bank[k].b0;
        j->bank_taps[k].bd = s->bank[k].bd;
        j->bank_taps[k].ad = s->bank[k].ad;
        j->bank_taps[k].mix = s->bank[k].mix;
    }
    if (e->cfg.device == XM_DEVICE_CPU || xmh_bank_ring_floats(j) <= XMH_BANK_LDS_FLOATS) return XM_OK;
    /* sized by batch: a slot per clip up to the workgroups a launch runs at once */
    const int slots = j->n_clips < XMH_BANK_SCRATCH_SLOTS ? j->n_clips : XMH_BANK_SCRATCH_SLOTS;
    const size_t need = (size_t)slots * (size_t)xmh_bank_ring_floats(j) * sizeof(float);
    if (e->bank_scr_cap < need) {
        /* an earlier stage's kernel may still run on the old buffer */
        int rc = xmh_stream_sync(e->stream);
        if (!rc) rc = grow(&e->bank_scr, &e->bank_scr_cap, need);
        if (rc) return rc;
    }
    j->bank_scratch = e->bank_scr;
    j->bank_scratch_slots = slots;
    return XM_OK;
}

static int ensure_ptrs(XmEffects *e, size_t n)
{
    if (e->ptr_cap >= n) return XM_OK;
    xmh_free(e->d_ptrs);
    xmh_host_free(e->h_ptrs);
    e->d_ptrs = NULL;
    e->h_ptrs = NULL;
    e->ptr_cap = 0;
    int rc = xmh_malloc((void **)&e->d_ptrs, n * sizeof(void *));
    if (!rc) rc = xmh_host_alloc((void **)&e->h_ptrs, n * sizeof(void *));
    if (!rc) e->ptr_cap = n;
    return rc;
}

/* Runs every stage; ping-pong through two device buffers so FIR never reads
 * what it writes.  src/dst: device pointer tables (n clips each). */
static int run_chain(XmEffects *e, size_t batch, size_t frames, float **src, float **dst, int streaming,
                     size_t clip0)
{
    const int C = e->cfg.channels;
    const size_t per = frames * (size_t)C;
    int rc = grow(&e->d_buf[0], &e->d_cap[0], batch * per * sizeof(float) + 16);
    if (!rc) rc = grow(&e->d_buf[1], &e->d_cap[1], batch * per * sizeof(float) + 16);
    if (!rc) rc = ensure_ptrs(e, batch * 6);
    if (rc) return rc;
    rc = xmh_stream_sync(e->stream);
    if (rc) return rc;
    /* table layout: [0,b) src  [b,2b) dst  [2b,3b) buf0  [3b,4b) buf1 */
    for (size_t i = 0; i < batch; ++i) {
        e->h_ptrs[i] = src[i];
        e->h_ptrs[batch + i] = dst[i];
        e->h_ptrs[2 * batch + i] = (float *)e->d_buf[0] + i * per;
        e->h_ptrs[3 * batch + i] = (float *)e->d_buf[1] + i * per;
    }
    rc = xmh_memcpy_h2d(e->d_ptrs, e->h_ptrs, 4 * batch * sizeof(void *), e->stream);
    if (rc) return rc;
    void **T_src = e->d_ptrs, **T_dst = e->d_ptrs + batch;
    void **T_b[2] = {e->d_ptrs + 2 * batch, e->d_ptrs + 3 * batch};
    int launches = 0;
    if (e->n_stages == 0) {
        for (size_t i = 0; !rc && i < batch; ++i)
            if (src[i] != dst[i]) rc = xmh_memcpy_d2d(dst[i], src[i], per * sizeof(float), e->stream);
        return rc;
    }
    /* FIR reads neighbours of the samples it writes: never run it in place.
     * If any clip is processed in place and the chain has a FIR stage, first
     * copy the inputs to buf0.  A biquad cascade runs in place (each chunk is
     * read into LDS before its outputs are stored), and so does a comb (the
     * owner of a sample reads it before it writes it; a bank likewise, with
     * the inputs it needs again kept in its own delay line): all take whatever
     * (cur, nxt) pair the FIR bookkeeping hands them, equal or not. */
    int inplace = 0, off = 0, has_fir = 0;
    for (int s = 0; s < e->n_stages; ++s) has_fir |= e->stages[s].kind == 2;
    for (size_t i = 0; has_fir && i < batch; ++i) inplace |= src[i] == dst[i];
    void **cur = T_src;
    if (inplace) {
        for (size_t i = 0; !rc && i < batch; ++i)
            rc = xmh_memcpy_d2d((float *)e->d_buf[0] + i * per, src[i], per * sizeof(float), e->stream);
        cur = T_b[0];
        off = 1;
    }
    for (int s = 0; !rc && s < e->n_stages; ++s) {
        const int last = s == e->n_stages - 1;
        void **nxt = last ? T_dst : T_b[(s + off) & 1];
        XmhFxJob j;
        memset(&j, 0, sizeof j);
        j.channels = C;
        j.n_clips = (int32_t)batch;
        j.frames = (int64_t)frames;
        j.in_ptrs = (const float *const *)cur;
        j.out_ptrs = (float *const *)nxt;
        const size_t C2 = (size_t)C;
        if (e->stages[s].kind == 1) {
            j.sos = e->stages[s].coef_dev;
            j.n_sos = e->stages[s].n;
            if (streaming) j.state = e->st[s][0] + clip0 * (size_t)j.n_sos * 2 * C2;
        } else if (e->stages[s].kind == 3) {
            j.comb_delay = e->stages[s].delay;
            memcpy(j.comb_coef, e->stages[s].comb, sizeof(float) * 3);
            if (streaming) {
                const size_t hoff = clip0 * 2 * (size_t)j.comb_delay * C2;
                j.comb_hist_in = e->st[s][e->st_cur[s]] + hoff;
                j.comb_hist_out = e->st[s][e->st_cur[s] ^ 1] + hoff;
            }
        } else if (e->stages[s].kind == 4) {
            rc = xm_effects_bank_job(e, &e->stages[s], &j);
            if (rc) break;
            if (streaming) {
                const size_t hoff = clip0 * (size_t)xmh_bank_hist_floats(&j);
                j.bank_hist_in = e->st[s][e->st_cur[s]] + hoff;
                j.bank_hist_out = e->st[s][e->st_cur[s] ^ 1] + hoff;
            }
        } else {
            j.fir = e->stages[s].coef_dev;
            j.fir_len = e->stages[s].n;
            if (streaming && j.fir_len > 1) {
                const size_t off = clip0 * (size_t)(j.fir_len - 1) * C2;
                j.hist_in = e->st[s][e->st_cur[s]] + off;
                j.hist_out = e->st[s][e->st_cur[s] ^ 1] + off;
            }
        }
        rc = xmh_launch_fx(&j, e->stream, &launches);
        cur = nxt;
    }
    return rc;
}

static int process(XmEffects *e, const float *const *in, float *const *out, size_t batch, size_t frames,
                   int streaming)
{
    int rc = XM_OK;
    const size_t bytes = frames * (size_t)e->cfg.channels * sizeof(float);
    if (e->cfg.mem_kind == XM_MEM_DEVICE) {
        /* FIR stages must not run in place: route through scratch when in == out */
        float **src = malloc(sizeof(float *) * batch), **dst = malloc(sizeof(float *) * batch);
        if (!src || !dst) rc = XM_ENOMEM;
        for (size_t i = 0; !rc && i < batch; ++i) {
            src[i] = (float *)in[i];
            dst[i] = out[i];
        }
        if (!rc) rc = run_chain(e, batch, frames, src, dst, streaming, 0);
        free(src);
        free(dst);
    } else {
        /* host: stage through a device buffer (chunks of <= 1 GiB) */
        size_t chunk = bytes ? ((size_t)1 << 30) / bytes : batch;
        if (chunk < 1) chunk = 1;
        if (chunk > batch) chunk = batch;
        void *d_io = NULL;
        rc = xmh_malloc(&d_io, chunk * bytes * 2);
        float **src = malloc(sizeof(float *) * chunk), **dst = malloc(sizeof(float *) * chunk);
        if (!src || !dst) rc = XM_ENOMEM;
        for (size_t b0 = 0; !rc && b0 < batch; b0 += chunk) {
            size_t nb = batch - b0 < chunk ? batch - b0 : chunk;
            for (size_t i = 0; !rc && i < nb; ++i) {
                src[i] = (float *)d_io + i * (bytes / sizeof(float));
                dst[i] = (float *)d_io + (chunk + i) * (bytes / sizeof(float));
                rc = xmh_memcpy_h2d(src[i], in[b0 + i], bytes, e->stream);
            }
            if (!rc) rc = run_chain(e, nb, frames, src, dst, streaming, b0);
            for (size_t i = 0; !rc && i < nb; ++i) rc = xmh_memcpy_d2h(out[b0 + i], dst[i], bytes, e->stream);
            if (!rc) rc = xmh_stream_sync(e->stream);
        }
        free(src);
        free(dst);
        xmh_stream_sync(e->stream);
        xmh_free(d_io);
    }
    if (!rc && !e->user_stream) rc = xmh_stream_sync(e->stream);
    return rc;
}

/* ---- multi-device dispatch: block d of the clips on sub-chain d ---------- */
typedef struct {
    const float *const *in;
    float *const *out;
    size_t batch, frames;
    int stream;   /* 0 process_batch, 1 process_stream (blocks of stream_reset) */
} XmFxArg;

static int t_fx(void *ctx, int d, void *p)
{
    XmEffects *e = ctx;
    const XmFxArg *a = p;
    size_t f, c;
    if (a->stream) {
        f = e->st_first[d];
        c = e->st_cnt[d];
    } else {
        xm_block(a->batch, e->n_sub, d, &f, &c);
    }
    if (!c) return XM_OK;
    return a->stream ? xm_effects_process_stream(e->sub[d], a->in + f, a->out + f, c, a->frames)
                     : xm_effects_process_batch(e->sub[d], a->in + f, a->out + f, c, a->frames);
}

int xm_effects_process_batch(XmEffects *e, const float *const *in, float *const *out, size_t batch, size_t frames)
{
    if (!e || (batch && (!in || !out))) return XM_EINVAL;
    if (batch == 0 || frames == 0) return XM_OK;
    if (batch > (size_t)INT32_MAX / 2) return XM_EINVAL;
    if (e->n_sub) {
        XmFxArg a = {in, out, batch, frames, 0};
        return xm_pool_run(e->pool, t_fx, &a);
    }
    int rc = xmh_set_device(e->cfg.device);
    if (!rc) rc = build_stages(e);
    if (rc) return rc;
    return process(e, in, out, batch, frames, 0);
}

/* ---- streaming ---------------------------------- */
int xm_effects_stream_reset(XmEffects *e, size_t n_clips)
{
    if (!e || n_clips == 0 || n_clips > (size_t)INT32_MAX / 2) return XM_EINVAL;
    if (e->n_sub) {   /* device d streams block d of the clips */
        int rc = XM_OK;
        e->st_ready = 0;
        for (int d = 0; d < e->n_sub && !rc; ++d) {
            xm_block(n_clips, e->n_sub, d, &e->st_first[d], &e->st_cnt[d]);
            if (e->st_cnt[d]) rc = xm_effects_stream_reset(e->sub[d], e->st_cnt[d]);
        }
        if (rc) return rc;
        e->st_clips = n_clips;
        e->st_ready = 1;
        e->dirty = 0;
        return XM_OK;
    }
    int rc = xmh_set_device(e->cfg.device);
    if (!rc) rc = build_stages(e);
    if (rc) return rc;
    xmh_stream_sync(e->stream);   /* a previous block may still use the old state */
    free_stream_state(e);
    const size_t C = (size_t)e->cfg.channels;
    for (int s = 0; !rc && s < e->n_stages; ++s) {
        size_t per = e->stages[s].kind == 1   ? (size_t)e->stages[s].n * 2 * C
                     : e->stages[s].kind == 3 ? 2 * (size_t)e->stages[s].delay * C
                                              : (size_t)(e->stages[s].n - 1) * C;
        if (e->stages[s].kind == 4) {   /* every branch's D_k frames, then max D_k frames of input */
            size_t sum = 0, mx = 0;
            for (int k = 0; k < e->stages[s].n; ++k) {
                const size_t D = (size_t)e->stages[s].bank[k].delay_frames;
                sum += D;
                mx = D > mx ? D : mx;
            }
            per = (sum + mx) * C;
        }
        if (per == 0) continue;   /* 1-tap FIR: no history */
        const size_t bytes = n_clips * per * sizeof(float);
        const int nbuf = e->stages[s].kind == 1 ? 1 : 2;
        for (int k = 0; !rc && k < nbuf; ++k) {
            rc = xmh_malloc((void **)&e->st[s][k], bytes);
            if (!rc) rc = xmh_memset(e->st[s][k], 0, bytes, e->stream);
        }
        e->st_cur[s] = 0;
    }
    if (!rc) rc = xmh_stream_sync(e->stream);
    if (rc) {
        free_stream_state(e);
        return rc;
    }
    e->st_clips = n_clips;
    e->st_ready = 1;
    return XM_OK;
}

int xm_effects_process_stream(XmEffects *e, const float *const *in, float *const *out, size_t n_clips,
                              size_t frames)
{
    if (!e || (n_clips && (!in || !out))) return XM_EINVAL;
    if (e->dirty || !e->st_ready || n_clips != e->st_clips) return XM_EINVAL;   /* reset first */
    if (frames == 0) return XM_OK;
    if (e->n_sub) {
        XmFxArg a = {in, out, n_clips, frames, 1};
        return xm_pool_run(e->pool, t_fx, &a);
    }
    int rc = xmh_set_device(e->cfg.device);
    if (rc) return rc;
    rc = process(e, in, out, n_clips, frames, 1);
    if (!rc)
        for (int s = 0; s < e->n_stages; ++s)
            if (e->stages[s].kind != 1) e->st_cur[s] ^= 1;   /* hist_out becomes the history */
    return rc;
}
