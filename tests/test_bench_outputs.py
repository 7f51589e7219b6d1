"""bench.py's plain / --full split and --dump-outputs: the dump's arrays and their sizes on the CPU twin of the trainer, the JSON
line of a real run on the MI355X and the same dump from two runs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from deepinpainting_amd.options import Option  # noqa: E402
from oracle import cpu_model  # noqa: E402

DUMP_NAMES = {"input_A"} | {t + "_" + f for t in ("ref", "gt") for f in ("relu1_2", "relu2_2", "relu3_3", "relu4_3")}
FULL_ONLY = ("ipsr_layer_ms", "ipsr_layer_ms_bf16corr", "ipsr_layer_ms_other_configs", "roofline", "conv_roofline", "step_roofline",
             "alt_arithmetic", "new_mask_each_step", "innercos_roofline", "strict_reference", "losses_last_step")


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_outputs_on_the_cpu_twin(tmp_path, monkeypatch):
    """One training step of the CPU twin, dumped twice: the same names, float32, the same sampled positions, under 64 MB, and the
    numbers are the step's own input and VGG features."""
    opt = Option(gpu_ids=[], batchSize=1, use_dropout=True, quiet=True, allow_random_vgg=True, checkpoints_dir=str(tmp_path / "ckpt"))
    torch.manual_seed(1234)
    model = bench.quiet(cpu_model.create_cpu_model, opt)
    img, mask, ref = bench.synthetic_batch(torch.device("cpu"), 1, 1234)
    bench.train_step(model, img, mask, ref)
    bench.dump_outputs(model, str(tmp_path / "a"))
    bench.dump_outputs(model, str(tmp_path / "b"))
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert set(a) == DUMP_NAMES
    for k in a:
        assert a[k].dtype == np.float32 and np.array_equal(a[k], b[k]), k
    np.testing.assert_array_equal(a["input_A"], model.input_A.numpy())
    np.testing.assert_array_equal(a["gt_relu4_3"], model._gt_latent.relu4_3.numpy())
    assert sum(x.nbytes for x in a.values()) <= 64 * 2 ** 20
    monkeypatch.setitem(bench.DUMP_CAP, "features", 1000)                               # longer arrays: the same seeded sample
    bench.dump_outputs(model, str(tmp_path / "c"))
    bench.dump_outputs(model, str(tmp_path / "d"))
    c, d = _load(tmp_path / "c"), _load(tmp_path / "d")
    assert c["ref_relu1_2"].shape == (1000,) and np.array_equal(c["ref_relu1_2"], d["ref_relu1_2"])
    assert np.isin(c["ref_relu1_2"], model.ref_latent.relu1_2.numpy()).all()


def _bench(argv, timeout):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=timeout, text=True, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_plain_run_prints_the_headline_and_two_runs_dump_the_same_arrays(tmp_path):
    args = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2", "--dump-outputs"]
    out = _bench(args + [str(tmp_path / "a")], 420)
    assert out["metric"] == bench.METRIC and out["unit"] == "images/sec" and out["higher_is_better"] is True
    assert out["dtype"] == "f32" and out["steps"] == 3 and out["warmup"] == 1
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert abs(out["value"] - 2 * 3 / (out["ms_per_step"] * 3e-3)) <= 1e-3 * out["value"]
    assert out["losses_finite"] is True
    assert not [k for k in FULL_ONLY + ("cpu_baseline",) if k in out]
    _bench(args + [str(tmp_path / "b")], 420)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert set(a) == set(b) == DUMP_NAMES and all(x.dtype == np.float32 for x in a.values())
    assert sum(x.nbytes for x in a.values()) <= 64 * 2 ** 20
    assert a["input_A"].shape == (2, 3, bench.FINE, bench.FINE)
    for k in a:
        assert np.isfinite(a[k]).all() and np.array_equal(a[k], b[k]), k


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_full_run_carries_the_measurements_beyond_the_headline():
    out = _bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline"], 840)
    assert out["value"] > 0 and out["ms_per_step"] > 0 and out["steps"] == 3
    assert all(out.get(k) is not None for k in FULL_ONLY), [k for k in FULL_ONLY if out.get(k) is None]
    assert out["ipsr_layer_ms"]["in_step"]["calls_timed"] == [3, 3]
    assert out["roofline"]["launches_timed"] == 3 and out["conv_roofline"]["launches_timed"] > 0
