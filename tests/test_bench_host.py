"""Host-side pieces of bench.py that need no GPU."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_bare_gpus_n_becomes_a_torchrun_job(monkeypatch):
    """`python bench.py --gpus 4` without WORLD_SIZE replaces itself by the documented launcher command (one rank per GPU,
    rendezvous on 127.0.0.1, the same bench arguments)."""
    b = _bench()
    seen = {}

    def fake_execve(path, argv, env):
        seen.update(path=path, argv=list(argv), env=dict(env))
        raise SystemExit(0)

    monkeypatch.setattr(os, "execve", fake_execve)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "5", "--warmup", "2"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    try:
        b.main()
    except SystemExit:
        pass
    a = seen["argv"]
    assert seen["path"] == sys.executable and a[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nnodes=1" in a and "--nproc-per-node=4" in a
    assert a[a.index("--master-addr") + 1] == "127.0.0.1" and 1024 < int(a[a.index("--master-port") + 1]) < 65536
    i = a.index(os.path.join(ROOT, "bench.py"))
    assert a[i + 1:] == ["--gpus", "4", "--steps", "5", "--warmup", "2"]
    assert seen["env"].get("HSA_ENABLE_IPC_MODE_LEGACY") == "0"


def test_ldlt_chain_length():
    b = _bench()
    assert b.ldlt_chain(12000, 2597) == 73 + 42
    assert b.ldlt_chain(640, 600) == 10          # too short for the two-ended form


def test_dump_outputs_writes_float64_arrays(tmp_path):
    b = _bench()
    poses = np.arange(36.0).reshape(3, 12)
    row = {k: float(i) for i, k in enumerate(b.LM_STEP_FIELDS)}
    b.dump_outputs(str(tmp_path / "out"), poses, row)
    p, r = np.load(tmp_path / "out" / "poses.npy"), np.load(tmp_path / "out" / "lm_step.npy")
    assert p.dtype == np.float64 and np.array_equal(p, poses)
    assert r.dtype == np.float64 and np.array_equal(r, np.arange(len(b.LM_STEP_FIELDS), dtype=np.float64))
