"""bench.py's launch plan: `--gpus N` drives N devices in
one process through the library's multi-device handle, or fails loudly; under
torchrun --gpus must equal WORLD_SIZE.  CPU-only: no device is touched."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _plan(argv, world=1, visible=8):
    return bench.plan(bench.parse(argv), world, visible)


def test_default_is_one_gpu():
    assert _plan([]) == ("local", [0])


def test_gpus_n_in_one_process():
    assert _plan(["--gpus", "8"]) == ("local", list(range(8)))
    assert _plan(["--gpus", "2"], visible=2) == ("local", [0, 1])


def test_gpus_beyond_visible_fails_loudly():
    with pytest.raises(SystemExit) as e:
        _plan(["--gpus", "2"], visible=1)
    assert "visible" in str(e.value)


def test_devices_list_dev_flag():
    assert _plan(["--devices", "0,0"], visible=1) == ("local", [0, 0])
    with pytest.raises(SystemExit):
        _plan(["--devices", "0,1"], visible=2)          # 2 distinct GPUs but --gpus 1
    assert _plan(["--devices", "0,1", "--gpus", "2"], visible=2) == ("local", [0, 1])


def test_torchrun_world_must_match():
    assert _plan(["--gpus", "4"], world=4)[0] == "ranked"
    with pytest.raises(SystemExit):
        _plan(["--gpus", "1"], world=4)
    with pytest.raises(SystemExit):
        _plan(["--gpus", "2", "--devices", "0,1"], world=2)


def test_torchrun_ranks_beyond_visible(monkeypatch):
    """More ranks than GPUs fails loudly, unless the dev rehearsal switch
    (ranks share one GPU, gloo coordination, lines marked "rehearsal")."""
    monkeypatch.delenv("XM_BENCH_REHEARSE", raising=False)
    with pytest.raises(SystemExit):
        _plan(["--gpus", "2"], world=2, visible=1)
    monkeypatch.setenv("XM_BENCH_REHEARSE", "1")
    assert _plan(["--gpus", "2"], world=2, visible=1)[0] == "ranked"


def test_config5_ramps_and_shards():
    assert len(bench.RAMPS64) == 64
    args = bench.parse(["--config", "c5"])
    assert args.tracks5 % 8 == 0 and args.mixes5 % 8 == 0


def test_plain_run_is_the_headline_only():
    """Without --full the CPU baseline and the parity check are off; --full
    turns them on and --no-cpu / --no-check still switch each off."""
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.no_cpu, a.no_check, a.dump_outputs) == (7, 2, False, True, True, "")
    a = bench.parse(["--full"])
    assert (a.full, a.no_cpu, a.no_check) == (True, False, False)
    a = bench.parse(["--full", "--no-cpu"])
    assert (a.no_cpu, a.no_check) == (True, False)
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


@pytest.mark.parametrize("shape,dtype,shards", [((5, 300, 2), "float32", 1), ((3, 100, 2), "int16", 2),
                                                ((1, 50, 1), "float32", 1), ((40, 20000, 2), "float32", 1)])
def test_dump_outputs_sample(tmp_path, monkeypatch, shape, dtype, shards):
    """--dump-outputs: float32 .npy files holding the buffer's own values, the
    same choice on every call, within the shard's share of the budget."""
    import numpy as np
    import torch

    monkeypatch.setattr(bench, "DUMP_BUDGET", 4 * 400000)   # a budget the largest case exceeds
    B, F, C = shape
    y = torch.from_numpy((np.arange(B * F * C) % 30011 - 15000).astype(dtype).reshape(shape))
    got = []
    for d in ("a", "b"):
        args = bench.parse(["--dump-outputs", str(tmp_path / d)])
        bench.dump_outputs(args, y, "out", shards)
        files = sorted(os.listdir(tmp_path / d))
        assert files == ["out_mixes.npy", "out_windows.npy"]
        got.append([np.load(tmp_path / d / f) for f in files])
    (mixes, win), again = got
    assert all(np.array_equal(p, q) for p, q in zip(got[0], again))
    assert mixes.dtype == win.dtype == np.float32
    assert mixes.nbytes + win.nbytes <= bench.DUMP_BUDGET // shards or mixes.shape == tuple(shape)
    yn = y.numpy().astype(np.float32)
    assert win.shape[0] == B and mixes.shape[1:] == (F, C)
    assert np.array_equal(mixes[0], yn[0]) and (len(mixes) < 2 or np.array_equal(mixes[-1], yn[-1]))
    W = win.shape[1]
    for b in range(B):   # every window is a contiguous run of its own mix
        s = np.flatnonzero((yn[b, :F - W + 1] == win[b, 0]).all(axis=1))
        assert any(np.array_equal(yn[b, i:i + W], win[b]) for i in s)


def test_allotted_cores_reports_affinity():
    n, host = bench.allotted_cores()
    assert 1 <= n <= host
    if hasattr(os, "sched_getaffinity") and not os.environ.get("OMP_NUM_THREADS"):
        assert n == len(os.sched_getaffinity(0))
