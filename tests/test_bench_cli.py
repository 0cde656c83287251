"""bench.py's command line: on the CPU (no GPU call is reached), and one plain run on the GPU."""
from __future__ import annotations

import os

import pytest


def test_bench_rejects_gpus_not_world_size():
    """--gpus N under a launcher whose WORLD_SIZE differs is an error (exit 2), before any GPU work."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, WORLD_SIZE="3", RANK="0", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2"], cwd=root, env=env,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 2, out.stderr[-2000:]


def test_dump_outputs_sample_is_fixed_and_within_budget(tmp_path, monkeypatch):
    """--dump-outputs keeps every array whole under the byte budget; over it, every kind keeps the same
    seeded sample of its rows from call to call, in float64, and the files together stay under the budget."""
    import sys
    import types

    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    from visual_inertial_bundle_adjustment_amd.kinds import NUM_VAR_KINDS, VAR_DATA

    class Engine:
        nvars = [4001, 301, 301] + [0] * (NUM_VAR_KINDS - 3)

        def get_vars(self, k):
            return np.arange(self.nvars[k] * VAR_DATA[k], dtype=np.float64).reshape(-1, VAR_DATA[k]) + k

    summary = types.SimpleNamespace(initial_cost=3.0, final_cost=2.0, num_iterations=5, num_rescaled=1,
                                    num_troubled_seqs=0, largest_troubled_seq=0)
    e = Engine()
    whole = bench.dump_outputs(e, summary, str(tmp_path / "whole"))
    assert whole == {"vars_point": [4001, 3], "vars_pose": [301, 7], "vars_vel": [301, 3], "summary": [6]}
    assert np.array_equal(np.load(tmp_path / "whole" / "vars_pose.npy"), e.get_vars(1))
    assert np.load(tmp_path / "whole" / "summary.npy").tolist() == [3.0, 2.0, 5.0, 1.0, 0.0, 0.0]
    total = sum(e.get_vars(k).nbytes for k in range(3)) + 48
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", total // 3)
    a = bench.dump_outputs(e, summary, str(tmp_path / "a"))
    b = bench.dump_outputs(e, summary, str(tmp_path / "b"))
    assert a == b and a["summary"] == [6] and 0 < a["vars_point"][0] < 4001 and 0 < a["vars_pose"][0] < 301
    size = 0
    for name in a:
        x, y = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert x.dtype == np.float64 and np.array_equal(x, y)
        size += x.nbytes
    assert size <= total // 3
    pts = np.load(tmp_path / "a" / "vars_point.npy")
    assert np.all(np.diff(pts[:, 0]) > 0) and np.all(pts[:, 0] % 3 == 0)  # whole rows of the input, in order


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    """A plain `bench.py --gpus 1 --steps 3 --warmup 1` (config A) times exactly 3 iterations, carries
    ms_per_step = 1e3 / value, and runs none of --full's legs (roofline, CPU baseline null);
    --dump-outputs writes the variables and the summary the timed optimize call left: the same costs as the
    engine driven in-process over the same warmup + timed iterations (bounds of test_bench_two_ranks_line),
    and every kind's variables in the engine's shape."""
    import json
    import subprocess
    import sys

    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dump = tmp_path / "out"
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--config", "A", "--steps", "3",
           "--warmup", "1", "--dump-outputs", str(dump)]
    out = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 1, lines
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "LM iterations/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["value"] > 0 and abs(line["ms_per_step"] * line["value"] - 1e3) <= 1e-6 * 1e3
    assert line["roofline"] is None and line["cpu_baseline"] is None and "vs_fp64" not in line
    assert "cpu baseline" not in out.stderr and "profiled pass" not in out.stderr
    from visual_inertial_bundle_adjustment_amd import synth
    from visual_inertial_bundle_adjustment_amd.engine import HipEngine, Settings
    from visual_inertial_bundle_adjustment_amd.kinds import NUM_VAR_KINDS, VAR_NAMES
    p = synth.generate(synth.config("A"))
    e = HipEngine(imu_calib_options=p.imu_calib_options)
    synth.load_into(e, p, rs_device=True)

    def settings(n):
        return Settings.default(max_num_iterations=n, stop_if_no_improvement_for=10**6,
                                distance_from_troubled_iteration=0)
    e.optimize(settings(1))
    s = e.optimize(settings(3))
    shapes = {f"vars_{VAR_NAMES[k]}": e.get_vars(k).shape for k in range(NUM_VAR_KINDS) if e.nvars[k]}
    e.close()
    assert sorted(f.name for f in dump.iterdir()) == sorted([f"{n}.npy" for n in shapes] + ["summary.npy"])
    for name, shape in shapes.items():
        a = np.load(dump / f"{name}.npy")
        assert a.dtype == np.float64 and a.shape == shape and np.isfinite(a).all(), name
    c0, c1, its = np.load(dump / "summary.npy")[:3]
    assert its == 3
    assert abs(c0 - s.initial_cost) <= 1e-10 * s.initial_cost
    assert abs(c1 - s.final_cost) <= 1e-9 * s.final_cost


def test_pmc_traffic_only_from_this_trees_sources(tmp_path):
    """roofline.traffic comes from profiles/pmc_summary.json only when that summary was measured on the
    HIP sources this tree builds (its recorded sources digest): a summary of other code is reported as
    stale with traffic None, not passed off as this binary's bytes."""
    import json
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    from visual_inertial_bundle_adjustment_amd.build import sources_digest
    good = tmp_path / "good.json"
    good.write_text(json.dumps({"fanin_kernel": {"hbm_bytes_per_launch": 123.0},
                                "_meta": {"sources_sha256": sources_digest(), "commit": "abc"}}))
    t, prov = bench.pmc_traffic("fanin_kernel", str(good))
    assert t == 123.0 and prov["measured_at_commit"] == "abc" and prov["status"].startswith("measured")
    stale = tmp_path / "stale.json"
    stale.write_text(json.dumps({"fanin_kernel": {"hbm_bytes_per_launch": 123.0},
                                 "_meta": {"sources_sha256": "0" * 64, "commit": "old"}}))
    t, prov = bench.pmc_traffic("fanin_kernel", str(stale))
    assert t is None and prov["status"].startswith("stale")
