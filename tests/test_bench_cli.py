"""bench.py's command line: a plain run is the headline alone, `--full` adds the extra measurements, `--dump-outputs DIR`
writes what the last timed step returned (host logic on CPU tensors here; one plain run on the GPU)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_cli_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_plain_run_is_the_default(bench):
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = bench.parse_args(["--full", "--no-cpu-baseline", "--dump-outputs", "out"])
    assert a.full and a.no_cpu_baseline and a.dump_outputs == "out"


def test_dump_outputs_types_and_sample(bench, tmp_path):
    g = torch.Generator().manual_seed(3)
    big = torch.rand(3, 1000, 1001, generator=g)                     # 12 MB of float32: above the whole-array limit
    data = {"image0": torch.zeros(2, 1, 8, 8), "image1": torch.zeros(2, 1, 8, 8), "bs": 2, "hw0_i": torch.Size([8, 8]),
            "conf_matrix": big, "mconf": torch.rand(5, generator=g), "b_ids": torch.tensor([0, 1, 1, 2**40 + 3]),
            "gt_mask": torch.tensor([True, False]), "expec_f": torch.rand(4, 3, generator=g, dtype=torch.float64),
            "_match_counts": torch.tensor([3, 1, 2], dtype=torch.int32)}
    shapes = bench.dump_outputs(data, str(tmp_path / "a"))
    assert set(shapes) == {"conf_matrix.npy", "conf_matrix.sample_index.npy", "mconf.npy", "b_ids.npy", "gt_mask.npy", "expec_f.npy",
                           "_match_counts.npy"}
    ld = lambda d, k: np.load(str(tmp_path / d / (k + ".npy")))
    assert ld("a", "mconf").dtype == np.float32 and np.array_equal(ld("a", "mconf"), data["mconf"].numpy())
    assert ld("a", "expec_f").dtype == np.float64 and np.array_equal(ld("a", "expec_f"), data["expec_f"].numpy())
    assert ld("a", "b_ids").dtype == np.float64 and ld("a", "b_ids")[-1] == 2**40 + 3
    assert ld("a", "gt_mask").tolist() == [1.0, 0.0] and ld("a", "_match_counts").tolist() == [3.0, 1.0, 2.0]
    idx, val = ld("a", "conf_matrix.sample_index"), ld("a", "conf_matrix")
    assert 0.8 * bench.DUMP_SAMPLE < len(idx) <= bench.DUMP_SAMPLE and np.all(np.diff(idx) > 0) and idx[-1] < big.numel()
    assert np.array_equal(val, big.reshape(-1).numpy()[idx.astype(np.int64)])
    assert sum(os.path.getsize(str(tmp_path / "a" / f)) for f in shapes) <= bench.DUMP_LIMIT_BYTES
    # the same entries of the same shape in every run: two builds compare output for output
    bench.dump_outputs({"conf_matrix": big * 2}, str(tmp_path / "b"))
    assert np.array_equal(ld("b", "conf_matrix.sample_index"), idx) and np.array_equal(ld("b", "conf_matrix"), 2 * val)


def test_dump_outputs_refuses_more_than_the_limit(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1000)
    with pytest.raises(RuntimeError, match="limit"):
        bench.dump_outputs({"x": torch.zeros(1000)}, str(tmp_path))
    assert not os.listdir(str(tmp_path))


@pytest.mark.gpu
def test_plain_bench_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    """A plain run (2 pairs, 2 timed steps) prints one JSON line with the headline fields and none of the --full extras, and
    --dump-outputs holds the matches of the last timed step."""
    out = tmp_path / "outputs"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2",
                        "--dump-outputs", str(out)], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    lines = p.stdout.decode().strip().splitlines()
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r["metric"] == "image-pairs/sec @640x480 indoor-ds" and r["unit"] == "image-pairs/s" and r["higher_is_better"] is True
    assert r["dtype"] == "f32" and r["steps"] == 2 and r["ms_per_step"] > 0
    assert abs(r["value"] - 2 * 1e3 / r["ms_per_step"]) <= 0.01 * r["value"]
    for k in ("roofline", "kernels", "stage_ms", "other_configs", "cpu_baseline"):
        assert k not in r, k
    mk0, mk1, mconf, m_bids = (np.load(str(out / f"{k}.npy")) for k in ("mkpts0_f", "mkpts1_f", "mconf", "m_bids"))
    assert mk0.dtype == np.float32 and mk0.shape == mk1.shape == (len(mconf), 2) and len(mconf) > 100
    assert set(np.unique(m_bids).tolist()) <= {0.0, 1.0} and np.isfinite(mk1).all()
    assert len(np.load(str(out / "conf_matrix.npy"))) == len(np.load(str(out / "conf_matrix.sample_index.npy")))
    assert not (out / "image0.npy").exists()
