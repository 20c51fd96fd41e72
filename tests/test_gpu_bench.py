"""GPU: bench.py's command line. A plain run prints one result line for exactly
--steps timed steps and nothing that takes a run of its own (roofline and
cpu_baseline null); --dump-outputs writes the last timed step's loss and
tables as float32 .npy within 64 MB, the same from run to run (seeded inputs)."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, R, D, B = 14505, 237, 200, 1024   # FB15k-237, the default C2 workload


@pytest.fixture(autouse=True)
def _gpu(hiplib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _bench(*extra):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
                          "--warmup", "1"] + list(extra), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def _load(path):
    assert sorted(os.listdir(path)) == ["ent_emb.npy", "loss.npy", "rel_emb.npy"]
    assert sum(os.path.getsize(os.path.join(path, f)) for f in os.listdir(path)) <= 64_000_000
    return {f[:-4]: np.load(os.path.join(path, f)) for f in os.listdir(path)}


@pytest.fixture(scope="module")
def first_run(hiplib, tmp_path_factory):
    """(result line, dumped arrays) of one plain run, shared by the tests."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    path = str(tmp_path_factory.mktemp("dump_a"))
    return _bench("--dump-outputs", path), _load(path)


def test_plain_run_line_and_dump(first_run):
    line, a = first_run
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "positive-triples/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["roofline"] is None and line["cpu_baseline"] is None
    ms = line["ms_per_step"]
    assert ms > 0
    # value = B / seconds per step; ms_per_step is rounded to 1e-5 ms on the line
    assert abs(line["value"] - B / (ms * 1e-3)) <= B / (ms * 1e-3) * (1e-5 / ms)
    assert a["ent_emb"].shape == (E, D) and a["rel_emb"].shape == (R, D) and a["loss"].shape == (1,)
    for v in a.values():
        assert v.dtype == np.float32 and np.isfinite(v).all()
    assert a["loss"][0] > 0


def test_dump_repeats_from_run_to_run(first_run, tmp_path):
    """The same arguments again: the same inputs, so the same outputs up to the
    order of fp32 sums (elements below 1 in magnitude: a few ulp of 1.0; 4 steps)."""
    a = first_run[1]
    _bench("--dump-outputs", str(tmp_path / "b"))
    b = _load(str(tmp_path / "b"))
    assert np.abs(a["ent_emb"] - b["ent_emb"]).max() <= 1e-6
    assert np.abs(a["rel_emb"] - b["rel_emb"]).max() <= 1e-6
    assert abs(a["loss"][0] - b["loss"][0]) <= 1e-5 * abs(a["loss"][0])
