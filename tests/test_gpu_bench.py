"""The bench.py contract on a small config (run with -m gpu): one JSON line with the fields
the driver reads, the roofline and (--full) cpu_baseline objects, sane magnitudes; a plain run
measures only the headline, and --dump-outputs writes the last timed step's outputs."""
import json
import os
import subprocess
import sys

import pytest

from helpers import ROOT

pytestmark = pytest.mark.gpu


def test_bench_json_contract_c2():
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "C2", "--rounds", "2",
                          "--steps", "1", "--warmup", "1", "--full"], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout
    j = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in j, k
    assert j["n_gpus"] == 1 and j["steps"] == 1 and j["warmup"] == 1 and j["higher_is_better"] is True
    assert j["vs_baseline"] is None and j["data"] == "synthetic" and "workload" in j["config"]
    assert j["value"] > 1e9 and j["sgns"]["value"] > 1e7
    r = j["roofline"]
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and r["unit"] == "GB/s"
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and 0 < r["frac"] < 2
    c = j["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] == 1 and c["value"] > 0 and c["unit"] == "walk-steps/s"
    assert j["walk"]["steps_per_step_global"] == 100000 * 2 * 79
    assert j["walk_reference_exact"]["value"] > 0 and j["walk_on_the_fly"]["value"] > 0
    assert j["sgns_shared_negatives"]["value"] > 0 and j["preprocess_seconds_second_call"] > 0


def _plain_run(out_dir):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "C2", "--rounds", "2",
                          "--steps", "2", "--warmup", "0", "--dump-outputs", str(out_dir)],
                         capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_bench_plain_run_and_dump_outputs(tmp_path):
    """Without --full the line carries the headline only; --steps sets the timed steps; --dump-outputs writes the last
    timed step's walks (a seeded sample of rows, with their lengths: those of an independent walk with that step's seed)
    and the pairs the timed SGNS passes trained, and a second run with the same arguments writes the same files bit for
    bit.  The racing SGNS tables are checked by the bench, not written."""
    import numpy as np
    import torch
    import bench
    import node2vec
    from n2v_hip import synth
    j = _plain_run(tmp_path / "a")
    assert j["steps"] == 2 and j["warmup"] == 0 and j["ms_per_step"] > 0 and j["value"] > 1e9
    assert j["walk"]["steps_per_step_global"] == 100000 * 2 * 79
    assert j["sgns"]["pairs_per_step_global"] > 0 and j["preprocess_seconds_second_call"] > 0
    assert "cpu_baseline" not in j and j["walk_reference_exact"] is None and j["walk_on_the_fly"] is None
    assert j["sgns_shared_negatives"] is None
    names = sorted(os.listdir(str(tmp_path / "a")))
    assert names == ["sgns_pairs.npy", "walk_lens.npy", "walks.npy"], names
    a = {n: np.load(str(tmp_path / "a" / n)) for n in names}
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    w, n = a["walks.npy"], a["walk_lens.npy"]
    assert w.dtype == np.float64 and w.shape == (65536, 80) and n.dtype == np.float64 and n.shape == (65536,)
    assert n.min() >= 1 and n.max() <= 80 and w.min() >= -1 and w.max() < 100000
    assert a["sgns_pairs.npy"].tolist() == [j["sgns"]["pairs_per_step_global"] * 2]
    _plain_run(tmp_path / "b")
    assert sorted(os.listdir(str(tmp_path / "b"))) == names
    for name in names:
        assert np.array_equal(a[name], np.load(str(tmp_path / "b" / name))), name
    # the rows come from the LAST timed step: bench.py walks step s with seed 1000 + s (warm-up 0, steps 2)
    cg, _ = synth.make_config_graph("C2")
    g = node2vec.Graph.from_csr(cg, 1.0, 1.0, device="cuda:0", rng="philox", seed=1)
    g.preprocess_transition_probs()
    eng, N = g._engine, cg.n_nodes
    rows = torch.from_numpy(bench.row_sample(2 * N, 65536)).cuda()
    ws = torch.empty((2 * N, 80), dtype=torch.int32, device="cuda:0")
    ls = torch.empty(2 * N, dtype=torch.int32, device="cuda:0")
    for seed, same in ((1001, True), (1000, False)):
        eng.walk(eng.start_order, 2, 80, rng="philox", seed=seed, pos_begin=0, pos_count=N, out=(ws, ls))
        assert np.array_equal(ws[rows].cpu().numpy(), w) == same, seed
        assert np.array_equal(ls[rows].cpu().numpy(), n) or not same, seed
