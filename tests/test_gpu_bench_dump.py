"""bench.py's plain run, ``--dump-outputs`` and ``--full`` on a small trainer (ngf=8, batch 2), in this process.

A plain run prints the headline line only (no roofline run, no parity / other-config / CPU-baseline legs);
``--dump-outputs DIR`` writes the last timed step's loss scalars and the seeded state sample as float32 ``.npy``
files, identical from run to run with the same arguments (the step has no atomics in a result path: the same
inputs and weights give the same bits); ``--full`` still produces every section of the line.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ARGS = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2", "--ngf", "8"]
LOSSES = ("D1", "D2", "D", "G1", "G2", "data1", "data2", "G")
NETS = ("G1", "G2", "D1", "D2")


def _bench(monkeypatch, capsys, extra):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"] + ARGS + extra)
    capsys.readouterr()
    with torch.random.fork_rng(devices=[0]):  # (bench seeds the global generators)
        bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def _load(d):
    return {f: np.load(os.path.join(d, f), allow_pickle=False) for f in sorted(os.listdir(d))}


def test_plain_run_dumps_identical_outputs(monkeypatch, capsys, tmp_path):
    import bench
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 4096)  # below every network's size at ngf=8: the sampled path
    out = _bench(monkeypatch, capsys, ["--dump-outputs", str(tmp_path / "a")])
    assert out["metric"] == bench.METRIC and out["unit"] == "images/s" and out["higher_is_better"] is True
    assert out["dtype"] == "bf16" and out["steps"] == 2 and out["warmup"] == 1
    assert out["ms_per_step"] > 0
    assert abs(out["value"] - 2 / (out["ms_per_step"] * 1e-3)) <= 1e-3 * out["value"]
    # nothing but the timed steps: the sections with runs of their own are --full's
    assert out["cpu_baseline"] is None and "parity" not in out and "configs" not in out
    assert set(out["roofline"]) == {"whole_step", "whole_step_frac"}
    a = _load(tmp_path / "a")
    assert set(a) == {f"loss_{k}.npy" for k in LOSSES} | {f"state_{n}.npy" for n in NETS}
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for name, v in a.items():
        assert v.dtype == np.float32 and np.isfinite(v).all(), name
        assert v.shape == ((1,) if name.startswith("loss_") else (4096,)), (name, v.shape)
    _bench(monkeypatch, capsys, ["--dump-outputs", str(tmp_path / "b")])
    b = _load(tmp_path / "b")
    assert set(a) == set(b)
    for name in a:
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)


def test_full_run_keeps_every_section(monkeypatch, capsys):
    out = _bench(monkeypatch, capsys, ["--full", "--no-cpu-baseline"])
    assert out["ms_per_step"] > 0 and out["cpu_baseline"] is None
    roof = out["roofline"]
    for key in ("kernel", "frac", "g1g2_forward_frac", "per_kernel", "dominant_in_situ", "whole_step_frac"):
        assert key in roof, key
    assert out["parity"]["pass_fp32"] is True
    assert any(k.startswith("C2_") for k in out["configs"]) and any(k.startswith("C3_") for k in out["configs"])
