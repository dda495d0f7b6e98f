#!/usr/bin/env python3
"""Secondary benchmarks: BASELINE.json configs 2-4 on one GPU (the per-GPU
shard of each), one JSON line per config.  bench.py stays the headline.

  python tools/bench_configs.py [c2 c3 c4 ...] [--steps K] [--warmup W]

c2  48k->44.1k resample, 4096 stereo 10 s fp32 clips (1-track mixes, unity gain)
c3  8-track s16 Q15 gain-ramp + crossfade mix, 1024 mixes x 10 s stereo 48 kHz
c4  per-GPU shard of config 4: 1024 clips = 128 mixes x 8 tracks, resample ->
    5-band RBJ EQ (biquad cascade) -> gain -> mix (8192 clips over 8 GPUs)
c5  config 5 on this GPU: 512 mixes x 8 of their 64 s16 tracks -> int32 partial
    -> reduce-scatter over RCCL when launched with torchrun -> saturate
Headline-shaped C-API variants (512 mixes x 8 stereo tracks x ~10 s, gain
ramps, the kernel each one lands on in "kernel"):
odd     frames_in 480001 (fused kernel, odd-length path)
ptrs    irregular pointer table (tracks in scattered order: fused kernel)
up      44.1k -> 48k fp32 (fused kernel, UP)
far     headline through a pointer table whose mixes' tracks lie ~7.9 GB apart (FAR kernel)
mono8   1024 mixes x 8 mono f32 tracks, 48k -> 44.1k (the headline's input bytes; MONO kernel)
mono1   8192 mono 10 s f32 clips 44.1k -> 48k at unity gain (config 1's shape, batched; MONO kernel)
c1s16   the same in config 1's own s16 form (generic kernel)
s16rs   48k -> 44.1k s16 Q15 (fused kernel, IO 2)
planar  48k -> 44.1k fp32, planar tracks and mixes (fused kernel, PL)
conv    48k -> 44.1k, s16 tracks into the fp32 mix (fused kernel, IO 1)
stream  the headline pushed in 8 blocks through stream_push (fused bulk straight from the block + generic heads)
oconv   the headline with XM_MIXER_OUT_CONVERT: s16 output (fused kernel epilogue)
comb    comb stage alone, D = 11025 frames (250 ms echo), 1024 stereo 10 s fp32 clips in place (k_comb_wide)
comb1   the same with D = 1 (k_comb_narrow); both report vs_copy against a torch device copy of the same bytes
bank4   comb bank alone (k_bank), the reverb preset's four combs of 29.7-43.7 ms, the same clips in place, delay lines in LDS
bank8   eight branches of 25-45 ms with b0 and bd live, still in LDS
bankfar four branches of 200-350 ms, delay lines in device scratch; the three report vs_copy and vs_serial
        (time over N x the single comb stage at the bank's median lag), each the minimum of three timings
Unit: input samples (frames x channels x tracks) per second; roofline
fraction = algorithmic bytes (inputs once + output once) / kernel time / 8 TB/s.
Inputs are synthetic PCM generated in HBM (xm_synth_pcm), outside the timing.
After timing, every line bit-checks the first and the last mix (or clip) of
its batch against the C oracle (oracle/xm_oracle.c) and reports
parity_check (--no-check skips it).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xm-audio-utils_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import xmaudio as xm  # noqa: E402
from bench import RAMPS, SEED, HBM_PEAK_GBS  # noqa: E402
import c_oracle as CO  # noqa: E402

Q15_RAMPS = [dict(gain0_q15=29491), dict(gain0_q15=0, gain1_q15=26214, ramp_start=0, ramp_len=48000),
             dict(gain0_q15=22938, gain1_q15=6554, ramp_start=240000, ramp_len=96000), dict(gain0_q15=16384),
             dict(mode=1, ramp_start=144000, ramp_len=96000),
             dict(gain0_q15=0, gain1_q15=32768, ramp_start=144000, ramp_len=96000),
             dict(gain0_q15=32768, gain1_q15=0, ramp_start=432000, ramp_len=48000),
             dict(gain0_q15=9830, gain1_q15=19661, ramp_start=300000, ramp_len=0)]
EQ5 = [(xm.XM_EQ_LOWSHELF, 100.0, 3.0, 0.7), (xm.XM_EQ_PEAKING, 400.0, -2.0, 1.0),
       (xm.XM_EQ_PEAKING, 1500.0, 2.5, 1.2), (xm.XM_EQ_PEAKING, 5000.0, -3.0, 0.9),
       (xm.XM_EQ_HIGHSHELF, 10000.0, 4.0, 0.7)]


_SAMPLER = None   # (process, file) of the clock sampler (start_sampler)
_LAST_WINDOW = None   # wall-clock window of the last timed loop (time.time())


def start_sampler():
    """A child process that never touches HIP polls rocm-smi's current clocks
    every ~0.3 s into a file (started before any device work: the box refuses
    an exec from a GPU-initialised process, and rocm-smi re-execs its
    interpreter).  report() attaches the clocks sampled during each line's
    timed loop."""
    global _SAMPLER
    import subprocess
    import tempfile
    f = tempfile.NamedTemporaryFile(prefix="xm_clk_", suffix=".jsonl", delete=False)
    f.close()
    code = ("import json,subprocess,time,sys\n"
            "while True:\n"
            "    t=time.time()\n"
            "    try:\n"
            "        r=subprocess.run(['rocm-smi','--showclocks','--json'],capture_output=True,text=True,timeout=10)\n"
            "        d=json.loads(r.stdout) if r.stdout.strip().startswith('{') else {}\n"
            "    except Exception:\n"
            "        d={}\n"
            "    c=next((v for v in d.values() if isinstance(v,dict)),{})\n"
            "    open(sys.argv[1],'a').write(json.dumps({'t':(t+time.time())/2,**{k.split()[0]:v for k,v in c.items() if 'speed' in k}})+'\\n')\n"
            "    time.sleep(0.3)\n")
    try:
        p = subprocess.Popen([sys.executable, "-c", code, f.name], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        _SAMPLER = (p, f.name)
    except Exception:  # pragma: no cover - box dependent
        _SAMPLER = None


def stop_sampler():
    if _SAMPLER:
        _SAMPLER[0].kill()
        try:
            os.unlink(_SAMPLER[1])
        except OSError:
            pass


def clocks_during(window):
    """Median of each clock rocm-smi reported inside `window` (wall seconds)."""
    if not _SAMPLER or not window:
        return None
    rows = []
    try:
        for line in open(_SAMPLER[1]):
            d = json.loads(line)
            if window[0] <= d.get("t", 0) <= window[1]:
                rows.append(d)
    except (OSError, ValueError):
        return None
    out = {"samples": len(rows)}
    for k in ("sclk", "mclk", "fclk", "socclk"):
        v = sorted(int("".join(ch for ch in str(r[k]) if ch.isdigit()) or 0) for r in rows if k in r)
        if v:
            out[k + "_mhz"] = v[len(v) // 2]
    return out


def timed(step, steps, warmup, stream):
    global _LAST_WINDOW
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    w0 = time.time()
    e0.record(stream)
    for _ in range(steps):
        step()
    e1.record(stream)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / steps
    _LAST_WINDOW = (w0, time.time())
    return wall * 1e3, e0.elapsed_time(e1) / steps


def beq(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def to_s16(y):
    return np.clip(np.rint(y.astype(np.float32) * np.float32(32768.0)), -32768, 32767).astype(np.int16)


def ends(n):
    return sorted({0, n - 1})


def parity(args, fn):
    """fn() -> bool, run after timing unless --no-check (None then)."""
    return None if args.no_check else bool(fn())


_BOX = None


def box_info():
    """Identifiers of the box and its GPU state, attached to every line
    (config 2 runs 6.5 ms on some boxes, 8.7 on others).
    rocm-smi's current clocks (sclk, mclk, fclk, socclk), compute and memory
    partition modes, board serial / unique id and PCI bus; the device's CU
    count and arch.  Best effort: a missing tool leaves the field out."""
    global _BOX
    if _BOX is not None:
        return _BOX
    import subprocess
    box = {}
    # rocm-smi first, from a process that has not touched the GPU yet (main()
    # calls this before any device work): the box refuses an exec from a
    # GPU-initialised process, and rocm-smi re-execs its interpreter
    # (round 6, VERDICT r5 item 3: the HBM vendor and the board's part and
    # VBIOS, the identifiers that commonly differ between MI355X boards)
    for flag in ("--showclocks", "--showcomputepartition", "--showmemorypartition", "--showserial", "--showuniqueid",
                 "--showbus", "--showpower", "--showmaxpower", "--showmemvendor", "--showvbios", "--showproductname"):
        try:
            r = subprocess.run(["rocm-smi", flag, "--json"], capture_output=True, text=True, timeout=20)
            d = json.loads(r.stdout) if r.returncode == 0 and r.stdout.strip().startswith("{") else {}
            for card, kv in d.items():
                if not isinstance(kv, dict):
                    continue
                for k, v in kv.items():
                    box[k] = v
                break   # the first card: the one this process uses on a 1-GPU box
        except Exception as e:  # pragma: no cover
            box[flag.strip("-") + "_error"] = str(e)[:60]
    try:   # amd-smi's static VRAM record (vendor, type, size), where the tool exists
        r = subprocess.run(["amd-smi", "static", "--vram", "--json"], capture_output=True, text=True, timeout=30)
        d = json.loads(r.stdout) if r.returncode == 0 and r.stdout.strip()[:1] in "[{" else None
        if isinstance(d, list) and d:
            d = d[0]
        if isinstance(d, dict):
            v = d.get("vram", d)
            if isinstance(v, dict):
                for k in ("type", "vendor", "size", "bit_width", "max_bandwidth"):
                    if k in v:
                        box[f"vram_{k}"] = v[k]
    except Exception as e:  # pragma: no cover
        box["amd_smi_error"] = str(e)[:60]
    _BOX = box
    return box


def box_props():
    """The device's CU count, arch and memory (after the GPU is up)."""
    box = box_info()
    if "cus" not in box:
        try:
            p = torch.cuda.get_device_properties(0)
            box.update(name=p.name, cus=p.multi_processor_count, arch=getattr(p, "gcnArchName", ""),
                       mem_gb=round(p.total_memory / 2**30, 1))
        except Exception as e:  # pragma: no cover - box dependent
            box["props_error"] = str(e)[:80]
    return box


def report(name, workload, samples, alg_bytes, wall_ms, ker_ms, mixer, launches=None, **extra):
    line = {"config": name, "workload": workload, "value": round(samples / (wall_ms * 1e-3) / 1e6, 1),
            "unit": "Msamples/s", "ms_per_step": round(wall_ms, 4), "kernel_ms": round(ker_ms, 4),
            "launches_per_step": mixer.timing().n_launches if launches is None else launches,
            "roofline": {"bound": "hbm", "alg_bytes": alg_bytes,
                         "achieved_GBps": round(alg_bytes / (ker_ms * 1e-3) / 1e9, 1),
                         "frac": round(alg_bytes / (ker_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}}
    line.update(extra)
    line["box"] = box_props()
    clk = clocks_during(_LAST_WINDOW)
    if clk:
        line["clocks_during"] = clk
    print(json.dumps(line), flush=True)


def c2(a):
    B, N = a.clips, 480000
    m = xm.Mixer(48000, 44100, 2, "f32", mem="device")
    F = m.out_frames(N)
    x = torch.empty((B, N, 2), dtype=torch.float32, device="cuda")
    y = torch.empty((B, F, 2), dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream()
    xm.synth(x.data_ptr(), "f32", SEED, 0, B, 2, N, 0, s.cuda_stream)
    m.set_stream(s.cuda_stream)
    w, k = timed(lambda: m.process_strided(x.data_ptr(), N * 2, N * 2, y.data_ptr(), F * 2, B, N), a.steps, a.warmup, s)
    ok = parity(a, lambda: all(beq(y[b].cpu().numpy(), CO.resample_f32(x[b].cpu().numpy(), 147, 160))
                               for b in ends(B)))
    report("c2", f"48k->44.1k resample, {B} stereo 10 s fp32 clips", B * N * 2, B * N * 8 + B * F * 8, w, k, m,
           parity_check=ok, fast_launches=m.timing().fast_launches)


def c3(a):
    B, ntr, N = a.mixes3, 8, 480000
    m = xm.Mixer(48000, 48000, 2, "s16", mem="device")
    m.set_tracks(Q15_RAMPS)
    x = torch.empty((B, ntr, N, 2), dtype=torch.int16, device="cuda")
    y = torch.empty((B, N, 2), dtype=torch.int16, device="cuda")
    s = torch.cuda.current_stream()
    xm.synth(x.data_ptr(), "s16", SEED, 0, B * ntr, 2, N, 0, s.cuda_stream)
    m.set_stream(s.cuda_stream)
    w, k = timed(lambda: m.process_strided(x.data_ptr(), N * 2, ntr * N * 2, y.data_ptr(), N * 2, B, N),
                 a.steps, a.warmup, s)
    ok = parity(a, lambda: beq(y[ends(B)].cpu().numpy(), CO.batch_mix_s16(x[ends(B)].cpu().numpy(), Q15_RAMPS,
                                                                               threads=8)[0]))
    report("c3", f"8-track s16 Q15 ramp/crossfade mix, {B} mixes x 10 s stereo 48 kHz", B * ntr * N * 2,
           B * ntr * N * 4 + B * N * 4, w, k, m, parity_check=ok)


def c4(a):
    B, ntr, N = a.mixes4, 8, 480000
    fx = xm.Effects(44100, 2, mem="device")
    for band in EQ5:
        fx.add_eq_band(*band)
    m = xm.Mixer(48000, 44100, 2, "f32", mem="device")
    m.set_tracks(RAMPS)
    m.set_track_effects(fx)
    F = m.out_frames(N)
    x = torch.empty((B, ntr, N, 2), dtype=torch.float32, device="cuda")
    y = torch.empty((B, F, 2), dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream()
    xm.synth(x.data_ptr(), "f32", SEED, 0, B * ntr, 2, N, 0, s.cuda_stream)
    m.set_stream(s.cuda_stream)
    w, k = timed(lambda: m.process_strided(x.data_ptr(), N * 2, ntr * N * 2, y.data_ptr(), F * 2, B, N),
                 a.steps, a.warmup, s)
    sos = np.stack([fx.biquad(i) for i in range(len(EQ5))])

    def chk():
        for b in ends(B):
            xb = x[b].cpu().numpy()
            r = [CO.biquad_f32(CO.resample_f32(xb[t], 147, 160), sos) for t in range(ntr)]
            if not beq(y[b].cpu().numpy(), CO.mix_f32(r, RAMPS)):
                return False
        return True
    report("c4", f"resample + 5-band EQ + 8-track mix, {B * ntr} clips per GPU (config 4 shard of 8192/8)",
           B * ntr * N * 2, B * ntr * N * 8 + B * F * 8, w, k, m, parity_check=parity(a, chk))


def fir(a):
    """FIR effect alone: K-tap filter over 1024 stereo 10 s clips @ 44.1 kHz,
    device memory, out of place (k_fir_rb); one line per K of --fir-k."""
    for K in [int(k) for k in str(a.fir_k).split(",")]:
        _fir(a, K)
        torch.cuda.empty_cache()


def _fir(a, K):
    B, N = a.clips_fx, 441000
    h = (np.sin(np.arange(K, dtype=np.float64) * 0.37) / (1 + np.arange(K))).astype(np.float32)
    e = xm.Effects(44100, 2, mem="device")
    e.add_fir(h)
    x = torch.empty((B, N, 2), dtype=torch.float32, device="cuda")
    y = torch.empty_like(x)
    s = torch.cuda.current_stream()
    xm.synth(x.data_ptr(), "f32", SEED, 0, B, 2, N, 0, s.cuda_stream)
    e.set_stream(s.cuda_stream)
    ins, outs = [x[b].data_ptr() for b in range(B)], [y[b].data_ptr() for b in range(B)]
    w, k = timed(lambda: e.process_ptrs(ins, outs, N), a.steps, a.warmup, s)
    ok = parity(a, lambda: all(beq(y[b].cpu().numpy(), CO.fir_f32(x[b].cpu().numpy(), h)) for b in ends(B)))
    alg = 2 * B * N * 2 * 4
    line = {"config": "fir" if K == 63 else f"fir{K}", "taps": K, "workload": f"{K}-tap FIR (upfirdn order), {B} stereo 10 s fp32 clips @ 44.1 kHz",
            "value": round(B * N * 2 / (w * 1e-3) / 1e6, 1), "unit": "Msamples/s", "ms_per_step": round(w, 4),
            "kernel_ms": round(k, 4),
            "roofline": {"bound": "hbm", "alg_bytes": alg, "achieved_GBps": round(alg / (k * 1e-3) / 1e9, 1),
                         "frac": round(alg / (k * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                         "valu_floor_note": "2K separately rounded fp32 ops per output sample"},
            "parity_check": ok}
    print(json.dumps(line), flush=True)


def bq(a):
    """Config 4's biquad stage alone: the 5-band EQ cascade over 1024 stereo
    10 s clips @ 44.1 kHz, device memory, in place (k_biquad_pc)."""
    B, N = a.clips_fx, 441000
    e = xm.Effects(44100, 2, mem="device")
    for band in EQ5:
        e.add_eq_band(*band)
    sos = np.stack([e.biquad(i) for i in range(len(EQ5))])
    x = torch.empty((B, N, 2), dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream()
    xm.synth(x.data_ptr(), "f32", SEED, 0, B, 2, N, 0, s.cuda_stream)
    x0 = x[ends(B)].clone()
    e.set_stream(s.cuda_stream)
    ptrs = [x[b].data_ptr() for b in range(B)]
    # one checked pass, then timed passes (in place: each pass filters the previous output)
    e.process_ptrs(ptrs, ptrs, N)
    torch.cuda.synchronize()
    ok = parity(a, lambda: all(beq(x[b].cpu().numpy(), CO.biquad_f32(x0[i].cpu().numpy(), sos))
                               for i, b in enumerate(ends(B))))
    w, k = timed(lambda: e.process_ptrs(ptrs, ptrs, N), a.steps, a.warmup, s)
    alg = 2 * B * N * 2 * 4
    line = {"config": "bq", "workload": f"5-section biquad cascade (sosfilt order), {B} stereo 10 s fp32 clips",
            "value": round(B * N * 2 / (w * 1e-3) / 1e6, 1), "unit": "Msamples/s", "ms_per_step": round(w, 4),
            "kernel_ms": round(k, 4),
            "roofline": {"bound": "serial recurrence (latency per wave), HBM roofline quoted", "alg_bytes": alg,
                         "achieved_GBps": round(alg / (k * 1e-3) / 1e9, 1),
                         "frac": round(alg / (k * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)},
            "parity_check": ok}
    print(json.dumps(line), flush=True)


def comb(a): _comb(a, "comb", 11025)   # 250 ms echo: the wide-lag kernel (k_comb_wide)
def comb1(a): _comb(a, "comb1", 1)     # 1-frame lag: the narrow-lag kernel (k_comb_narrow)


def _comb(a, name, D):
    """Comb stage alone: echo coefficients over 1024 stereo 10 s clips @ 44.1
    kHz, device memory, in place; vs_copy = its time over a torch
    device-to-device copy of the same bytes, timed the same way."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from comb_ref import comb_f32
    B, N = a.clips_fx, 441000
    coef = (1.0, 0.5, -0.45)
    e = xm.Effects(44100, 2, mem="device")
    e.add_comb(D, *coef)
    x = torch.empty((B, N, 2), dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream()
    xm.synth(x.data_ptr(), "f32", SEED, 0, B, 2, N, 0, s.cuda_stream)
    x0 = x[ends(B)].clone()
    e.set_stream(s.cuda_stream)
    ptrs = [x[b].data_ptr() for b in range(B)]
    # one checked pass, then timed passes (in place: each pass filters the previous output)
    e.process_ptrs(ptrs, ptrs, N)
    torch.cuda.synchronize()
    ok = parity(a, lambda: all(beq(x[b].cpu().numpy(), comb_f32(x0[i].cpu().numpy(), D, *coef))
                               for i, b in enumerate(ends(B))))
    xm.synth(x.data_ptr(), "f32", SEED, 0, B, 2, N, 0, s.cuda_stream)   # timed passes start from bounded input again
    w, k = timed(lambda: e.process_ptrs(ptrs, ptrs, N), a.steps, a.warmup, s)
    y = torch.empty_like(x)
    _, kc = timed(lambda: y.copy_(x), a.steps, a.warmup, s)
    alg = 2 * B * N * 2 * 4
    line = {"config": name, "delay_frames": D,
            "workload": f"comb D={D} (echo), {B} stereo 10 s fp32 clips @ 44.1 kHz, in place",
            "value": round(B * N * 2 / (w * 1e-3) / 1e6, 1), "unit": "Msamples/s", "ms_per_step": round(w, 4),
            "kernel_ms": round(k, 4), "copy_ms": round(kc, 4), "vs_copy": round(k / kc, 3),
            "roofline": {"bound": "hbm", "alg_bytes": alg, "achieved_GBps": round(alg / (k * 1e-3) / 1e9, 1),
                         "frac": round(alg / (k * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)},
            "parity": ok, "parity_check": ok}
    print(json.dumps(line), flush=True)


def _bank_taps(ms, b0, bd):
    """Feedback combs of the given delays at 44.1 kHz with loop gains of a 1.8 s decay, equal weights."""
    out = []
    for m in ms:
        D = int(np.rint(m * 44100 / 1000.0))
        out.append((D, b0, bd, -float(np.float32(10.0 ** (-3.0 * D / (44100 * 1.8)))), 1.0 / len(ms)))
    return out


def bank4(a):   # the reverb preset's bank alone (delay lines in LDS)
    _bank(a, "bank4", _bank_taps((29.7, 37.1, 41.1, 43.7), 0.0, 1.0), 0.7)


def bank8(a):   # eight branches of 25-45 ms, b0 and bd live (still in LDS)
    _bank(a, "bank8", _bank_taps((25.0, 27.9, 30.7, 33.6, 36.4, 39.3, 42.1, 45.0), 0.25, 0.75), 0.7)


def bankfar(a):   # four branches of 200-350 ms: delay lines in device scratch
    _bank(a, "bankfar", _bank_taps((200.0, 250.0, 300.0, 350.0), 0.0, 1.0), 0.7)


def _bank(a, name, taps, dry):
    """Comb bank alone over 1024 stereo 10 s clips @ 44.1 kHz, device memory, in
    place, the minimum of three timings.  vs_copy = that over a torch
    device-to-device copy of the same bytes; vs_serial = that over N times the
    single comb stage at the bank's median lag on the same clips (N passes are
    the least an unfused route costs, before its summing passes), each the
    minimum of three timings in this process."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from bank_ref import bank_f32
    B, N = a.clips_fx, 441000
    e = xm.Effects(44100, 2, mem="device")
    e.add_comb_bank(taps, dry)
    rtaps, rdry = e.comb_bank(0)
    dmed = int(np.median([t[0] for t in taps]))
    ec = xm.Effects(44100, 2, mem="device")
    ec.add_comb(dmed, 0.0, 1.0, taps[0][3])
    x = torch.empty((B, N, 2), dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream()
    synth = lambda: xm.synth(x.data_ptr(), "f32", SEED, 0, B, 2, N, 0, s.cuda_stream)
    synth()
    x0 = x[ends(B)].clone()
    e.set_stream(s.cuda_stream)
    ec.set_stream(s.cuda_stream)
    ptrs = [x[b].data_ptr() for b in range(B)]
    # one checked pass, then timed passes (in place: each pass filters the previous output)
    e.process_ptrs(ptrs, ptrs, N)
    torch.cuda.synchronize()
    ok = parity(a, lambda: all(beq(x[b].cpu().numpy(), bank_f32(x0[i].cpu().numpy(), rtaps, rdry))
                               for i, b in enumerate(ends(B))))
    y = torch.empty_like(x)
    ks, kss, kcs, w = [], [], [], 0.0
    for _ in range(3):   # every timing starts from bounded input again
        synth()
        w, k = timed(lambda: e.process_ptrs(ptrs, ptrs, N), a.steps, a.warmup, s)
        ks.append(k)
        synth()
        kss.append(timed(lambda: ec.process_ptrs(ptrs, ptrs, N), a.steps, a.warmup, s)[1])
        kcs.append(timed(lambda: y.copy_(x), a.steps, a.warmup, s)[1])
    k, ksingle, kc = min(ks), min(kss), min(kcs)
    alg = 2 * B * N * 2 * 4
    line = {"config": name, "delays_frames": [t[0] for t in taps], "branches": len(taps),
            "workload": f"comb bank of {len(taps)}, {B} stereo 10 s fp32 clips @ 44.1 kHz, in place",
            "value": round(B * N * 2 / (k * 1e-3) / 1e6, 1), "unit": "Msamples/s", "ms_per_step": round(w, 4),
            "kernel_ms": round(k, 4), "kernel_ms_all": [round(v, 4) for v in ks],
            "copy_ms": round(kc, 4), "vs_copy": round(k / kc, 3),
            "single_comb_ms": round(ksingle, 4), "single_comb_delay": dmed,
            "vs_serial": round(k / (len(taps) * ksingle), 3),
            "roofline": {"bound": "hbm", "alg_bytes": alg, "achieved_GBps": round(alg / (k * 1e-3) / 1e9, 1),
                         "frac": round(alg / (k * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)},
            "parity": ok, "parity_check": ok}
    print(json.dumps(line), flush=True)


def c5(a):
    """Config 5 per GPU: 8 of the 64 s16 tracks of every mix live here; int32
    partial -> RCCL reduce-scatter (torchrun, N > 1) -> saturate."""
    from xmaudio import dist as xd
    rk = xd.from_env()
    dev = rk.local
    torch.cuda.set_device(dev)
    xd.init(rk, "nccl", torch.device("cuda", dev))
    B, ntr, N = a.mixes5, 8, 480000
    m = xm.Mixer(48000, 48000, 2, "s16", mem="device", device=dev)
    m.set_tracks(Q15_RAMPS)
    s = torch.cuda.current_stream()
    m.set_stream(s.cuda_stream)
    x = torch.empty((B, ntr, N, 2), dtype=torch.int16, device="cuda")
    xm.synth(x.data_ptr(), "s16", SEED, rk.rank * B * ntr, B * ntr, 2, N, dev, s.cuda_stream)
    y = torch.empty((B // rk.world, N, 2), dtype=torch.int16, device="cuda")
    w, k = timed(lambda: xd.mix_spanning_s16(rk, m, x, out=y), a.steps, a.warmup, s)
    w = xd.max_over_ranks(rk, w, device="cuda")
    ok = None
    if rk.world == 1:   # one rank: the partial over its 8 tracks is the whole mix
        ok = parity(a, lambda: beq(y[ends(B)].cpu().numpy(),
                                   CO.batch_mix_s16(x[ends(B)].cpu().numpy(), Q15_RAMPS, threads=8)[0]))
    if rk.rank == 0:
        report("c5", f"64-track s16 mixdown, {B} mixes x 10 s stereo 48 kHz, 8 tracks per GPU, "
                     f"{rk.world} GPU(s) (partial + reduce-scatter + saturate)",
               rk.world * B * ntr * N * 2, B * ntr * N * 4 + (B // rk.world) * N * 4, w, k, m,
               note="per-GPU HBM bytes: this GPU's tracks once + its finished mixes once; bench.py --config c5 "
                    "is the full 64-track line", parity_check=ok)
    xd.finish(rk)


def _shape(a, name, fi=48000, fo=44100, fmt="f32", N=480000, ptrs=False, planar=False, conv=False,
           stream=False, oconv=False, far=False, ntr=8):
    B = a.mixes
    q15, ramps = Q15_RAMPS[:ntr], RAMPS[:ntr]
    m = xm.Mixer(fi, fo, 2, fmt, mem="device", planar=planar, convert_in=conv, convert_out=oconv)
    m.set_tracks(q15 if fmt == "s16" else ramps)
    F = m.out_frames(N)
    ifmt = "s16" if (fmt == "s16") != conv else "f32"
    isz = 2 if ifmt == "s16" else 4
    ofmt = "s16" if (fmt == "s16") != oconv else "f32"
    osz = 2 if ofmt == "s16" else 4
    x = torch.empty((B, ntr, N, 2), dtype=torch.int16 if ifmt == "s16" else torch.float32, device="cuda")
    y = torch.empty((B, F, 2), dtype=torch.int16 if ofmt == "s16" else torch.float32, device="cuda")
    s = torch.cuda.current_stream()
    xm.synth(x.data_ptr(), ifmt, SEED, 0, B * ntr, 2, N, 0, s.cuda_stream)
    m.set_stream(s.cuda_stream)
    perm = [(5 * t + 3) % ntr for t in range(ntr)]
    half = B * ntr // 2
    fidx = lambda b, t: (b * ntr + t) // 2 + (half if t % 2 else 0)   # noqa: E731
    if far:
        # even tracks of every mix from the first half of the batch tensor,
        # odd ones from the second: a mix's tracks lie ~7.9 GB apart (FAR kernel)
        xf_ = x.view(B * ntr, N, 2)
        ins = [xf_[fidx(b, t)].data_ptr() for b in range(B) for t in range(ntr)]
        outs = [y[b].data_ptr() for b in range(B)]
        step = lambda: m.process_ptrs(ins, outs, B, N)   # noqa: E731
    elif ptrs:
        # every mix's tracks in a scattered order: no common stride
        ins = [x[b, perm[t]].data_ptr() for b in range(B) for t in range(ntr)]
        outs = [y[b].data_ptr() for b in range(B)]
        step = lambda: m.process_ptrs(ins, outs, B, N)   # noqa: E731
    elif stream:
        nb = 8
        blk = (N + nb - 1) // nb
        ys = torch.empty((B, F + 64, 2), dtype=y.dtype, device="cuda")

        counts = [0, 0]    # fused / all launches of the last step (timing() covers one call)

        def step():
            counts[:] = [0, 0]

            def tally():
                counts[0] += m.timing().fast_launches
                counts[1] += m.timing().n_launches
            m.stream_begin(B)
            got = 0
            for i in range(nb):
                lo, hi = i * blk, min(N, (i + 1) * blk)
                got += m.stream_push_strided(x[0, 0, lo:].data_ptr(), N * 2, ntr * N * 2, hi - lo,
                                             ys[0, got:].data_ptr(), (F + 64) * 2, F + 64 - got)
                tally()
            m.stream_flush_strided(ys[0, got:].data_ptr(), (F + 64) * 2, F + 64 - got)
            tally()
    else:
        step = lambda: m.process_strided(x.data_ptr(), N * 2, ntr * N * 2, y.data_ptr(), F * 2, B, N)  # noqa: E731
    w, k = timed(step, a.steps, a.warmup, s)
    fast, launches = counts if stream else (m.timing().fast_launches, m.timing().n_launches)

    def chk():
        from math import gcd
        g = gcd(fi, fo)
        L, M = fo // g, fi // g
        for b in ends(B):
            xb = x[b].cpu().numpy()                     # [ntr][N][2] (planar: [ntr][2][N] in memory order)
            if far:
                xb = np.stack([x.view(B * ntr, N, 2)[fidx(b, t)].cpu().numpy() for t in range(ntr)])
            elif ptrs:
                xb = xb[perm]                           # slot t of the table holds track perm[t]
            if planar:
                xb = np.ascontiguousarray(xb.reshape(ntr, 2, N).swapaxes(1, 2))
            if fmt == "s16":
                want = CO.resample_mix_s16(list(xb), q15, L, M)
            else:
                xf = xb.astype(np.float32) * np.float32(2.0 ** -15) if conv else xb
                want = CO.resample_mix_f32(list(xf), ramps, L, M)
                if oconv:
                    want = to_s16(want)
            got = (ys[b, :F] if stream else y[b]).cpu().numpy()
            if planar:
                got = np.ascontiguousarray(got.reshape(2, F).T)
            if not beq(got, want):
                return False
        return True
    report(name, f"{name}: {B} mixes x {ntr} stereo {ifmt} tracks x {N} frames, {fi}->{fo} {fmt} mix"
           + (f", {ofmt} out" if oconv else ""),
           B * ntr * N * 2, B * ntr * N * 2 * isz + B * F * 2 * osz, w, k, m, launches=launches,
           kernel="k_rs147_mix" if fast == launches else ("generic" if not fast else f"{fast}/{launches} fused"),
           parity_check=parity(a, chk))


def _mono(a, name, ntr, B, fi, fo, N):
    """Mono f32 on the fused kernel (MONO): B mixes x ntr mono tracks."""
    m = xm.Mixer(fi, fo, 1, "f32", mem="device")
    ramps = RAMPS[:ntr] if ntr > 1 else [dict(gain0=1.0)]
    m.set_tracks(ramps)
    F = m.out_frames(N)
    x = torch.empty((B, ntr, N), dtype=torch.float32, device="cuda")
    y = torch.empty((B, F), dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream()
    xm.synth(x.data_ptr(), "f32", SEED, 0, B * ntr, 1, N, 0, s.cuda_stream)
    m.set_stream(s.cuda_stream)
    w, k = timed(lambda: m.process_strided(x.data_ptr(), N, ntr * N, y.data_ptr(), F, B, N), a.steps, a.warmup, s)
    fast, launches = m.timing().fast_launches, m.timing().n_launches

    def chk():
        from math import gcd
        g = gcd(fi, fo)
        L, M = fo // g, fi // g
        for b in ends(B):
            xb = x[b].cpu().numpy()[:, :, None]         # [ntr][N][1]
            want = CO.resample_mix_f32(list(xb), ramps, L, M)
            if not beq(y[b].cpu().numpy()[:, None], want):
                return False
        return True
    report(name, f"{name}: {B} mixes x {ntr} mono f32 tracks x {N} frames, {fi}->{fo} f32 mix",
           B * ntr * N, B * ntr * N * 4 + B * F * 4, w, k, m, launches=launches,
           kernel="k_rs147_mix MONO" if fast == launches else ("generic" if not fast else f"{fast}/{launches} fused"),
           parity_check=parity(a, chk))


def c1s16(a, name="c1s16", N=441000):
    """Config 1's own form (mono s16 44.1k -> 48k, unity Q15 gain), batched:
    8192 clips through Mixer(44100, 48000, 1, "s16"): the fused kernel's mono
    s16 (M16) 1-track rows."""
    B = 16 * a.mixes
    m = xm.Mixer(44100, 48000, 1, "s16", mem="device")
    ramps = [dict(gain0_q15=32768)]
    m.set_tracks(ramps)
    F = m.out_frames(N)
    x = torch.empty((B, N), dtype=torch.int16, device="cuda")
    y = torch.empty((B, F), dtype=torch.int16, device="cuda")
    s = torch.cuda.current_stream()
    xm.synth(x.data_ptr(), "s16", SEED, 0, B, 1, N, 0, s.cuda_stream)
    m.set_stream(s.cuda_stream)
    w, k = timed(lambda: m.process_strided(x.data_ptr(), N, N, y.data_ptr(), F, B, N), a.steps, a.warmup, s)
    fast, launches = m.timing().fast_launches, m.timing().n_launches

    def chk():
        for b in ends(B):
            want = CO.resample_mix_s16([x[b].cpu().numpy()[:, None]], ramps, 160, 147)
            if not beq(y[b].cpu().numpy()[:, None], want):
                return False
        return True
    report(name, f"{name}: {B} mono s16 clips x {N} frames, 44100->48000 s16 (config 1's form)",
           B * N, B * N * 2 + B * F * 2, w, k, m, launches=launches,
           kernel="k_rs147_mix" if fast == launches else ("generic" if not fast else f"{fast}/{launches} fused"),
           parity_check=parity(a, chk))


def c1odd(a): c1s16(a, "c1odd", N=441001)   # odd N: every other clip 2 B off a dword (round 5: fused)


def r32to48(a): _shape(a, "r32to48", fi=32000, fo=48000, N=320000)
def r48to32(a): _shape(a, "r48to32", fi=48000, fo=32000, N=480000)
def r96to44(a): _shape(a, "r96to44", fi=96000, fo=44100, N=960000, )
def r96to48(a): _shape(a, "r96to48", fi=96000, fo=48000, N=960000)
def r24to48(a): _shape(a, "r24to48", fi=24000, fo=48000, N=240000)
def r16to48(a): _shape(a, "r16to48", fi=16000, fo=48000, N=160000)
def m22to48(a): _mono(a, "m22to48", 1, 16 * a.mixes, 22050, 48000, 220500)
def r22to48(a): _shape(a, "r22to48", fi=22050, fo=48000, N=220500)   # fused kernel (round 5: RID_U2, L/M = 320/147)
def r44to96(a): _shape(a, "r44to96", fi=44100, fo=96000, N=441000)   # fused kernel (round 5: RID_U2)
def s22to48(a): _shape(a, "s22to48", fi=22050, fo=48000, N=220500, ntr=1)   # stereo 1-track rows at 320/147 (round 5)
def m44to96(a): _mono(a, "m44to96", 1, 16 * a.mixes, 44100, 96000, 441000)   # mono 1-track rows at 320/147 (round 5)
def m24to48(a): _mono(a, "m24to48", 1, 16 * a.mixes, 24000, 48000, 240000)   # mono 1-track rows at 2/1 (round 5)
def m16to48(a): _mono(a, "m16to48", 1, 16 * a.mixes, 16000, 48000, 160000)   # mono 1-track rows at 3/1 (round 5)
def s24to48(a): _shape(a, "s24to48", fi=24000, fo=48000, N=240000, ntr=1)   # stereo 1-track rows at 2/1 (round 5)
def s96to44(a): _shape(a, "s96to44", fi=96000, fo=44100, N=960000, ntr=1)   # stereo 1-track rows at 147/320 (round 5)
def s44to48(a): _shape(a, "s44to48", fi=44100, fo=48000, N=441000, ntr=1)   # stereo 1-track rows at 160/147 (round 6)
def s32to48(a): _shape(a, "s32to48", fi=32000, fo=48000, N=320000, ntr=1)   # ... at 3/2
def s48to32(a): _shape(a, "s48to32", fi=48000, fo=32000, N=480000, ntr=1)   # ... at 2/3
def s96to48(a): _shape(a, "s96to48", fi=96000, fo=48000, N=960000, ntr=1)   # ... at 1/2
# f32 mixes of 2 and 4 tracks (4 and 2 mixes per wave: split mode's plain stores)
def t2(a): _shape(a, "t2", ntr=2)
def t4(a): _shape(a, "t4", ntr=4)
def t2up(a): _shape(a, "t2up", fi=44100, fo=48000, N=441000, ntr=2)
def t4up(a): _shape(a, "t4up", fi=44100, fo=48000, N=441000, ntr=4)
def t2odd(a): _shape(a, "t2odd", N=480001, ntr=2)
def t4odd(a): _shape(a, "t4odd", N=480001, ntr=4)
def mono8(a): _mono(a, "mono8", 8, 2 * a.mixes, 48000, 44100, 480000)
def mono1(a): _mono(a, "mono1", 1, 16 * a.mixes, 44100, 48000, 441000)
def hl(a): _shape(a, "hl")   # the headline's workload through the C API (bench.py's line, here for PMC passes)
def odd(a): _shape(a, "odd", N=480001)
def ptrs(a): _shape(a, "ptrs", ptrs=True)
def far(a): _shape(a, "far", far=True)
def up(a): _shape(a, "up", fi=44100, fo=48000, N=441000)
def s16rs(a): _shape(a, "s16rs", fmt="s16")
def planar(a): _shape(a, "planar", planar=True)
def conv(a): _shape(a, "conv", conv=True)
# stereo s16 / planar mixes of fewer than 4 tracks (the same mixes count, so
# 1/8 .. 3/8 of the input bytes)
def s16rs1(a): _shape(a, "s16rs1", fmt="s16", ntr=1)
def s16rs2(a): _shape(a, "s16rs2", fmt="s16", ntr=2)
def s16rs3(a): _shape(a, "s16rs3", fmt="s16", ntr=3)
def planar2(a): _shape(a, "planar2", planar=True, ntr=2)
def conv2(a): _shape(a, "conv2", conv=True, ntr=2)
# stereo s16 Q15 mixes at 2/1, 3/1 and 320/147 (round 6: fused IO kernels; the generic kernel before)
def s16r24to48(a): _shape(a, "s16r24to48", fi=24000, fo=48000, fmt="s16", N=240000)
def s16r16to48(a): _shape(a, "s16r16to48", fi=16000, fo=48000, fmt="s16", N=160000)
def s16r22to48(a): _shape(a, "s16r22to48", fi=22050, fo=48000, fmt="s16", N=220500)
def stream(a): _shape(a, "stream", stream=True)
def oconv(a): _shape(a, "oconv", oconv=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("which", nargs="*", default=["c2", "c3", "c4"])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--clips", type=int, default=4096)
    ap.add_argument("--mixes3", type=int, default=1024)
    ap.add_argument("--mixes4", type=int, default=128)
    ap.add_argument("--mixes5", type=int, default=512)
    ap.add_argument("--mixes", type=int, default=512, help="headline-shaped variants")
    ap.add_argument("--no-check", action="store_true", help="skip the post-timing oracle checks")
    ap.add_argument("--clips-fx", type=int, default=1024, help="fir / bq: clips")
    ap.add_argument("--fir-k", default="63", help="fir: taps (a comma list: one line each)")
    ap.add_argument("--no-box", action="store_true",
                    help="no rocm-smi box identifiers (under rocprofv3, whose preload initialises the GPU first)")
    a = ap.parse_args()
    global _BOX
    if a.no_box or any(k.startswith(("ROCPROF", "ROCP_")) for k in os.environ):   # under rocprofv3: no rocm-smi
        _BOX = {}
    box_info()   # before any device work (see box_info)
    if _BOX:
        start_sampler()
    try:
        for w in a.which:
            globals()[w](a)
            torch.cuda.empty_cache()
    finally:
        stop_sampler()


if __name__ == "__main__":
    main()
