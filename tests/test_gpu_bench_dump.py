"""bench.py --dump-outputs on the GPU: the dumped y of the headline (config 2) is the render of the seeded inputs, the same in every run, and
stays right when the last timed step rendered into a gather slot (two ranks sharing cuda:0 over gloo, the IPC gather, which frees its array
when a timed window ends)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHORT = ["--steps", "2", "--warmup", "1", "--no-secondary", "--cpu-seconds", "0", "--windows", "1", "--event-windows", "1"]


def _bench(out_dir, extra=(), env_extra=None):
    env = dict(os.environ, BENCH_DETAIL_DIR=str(out_dir), **(env_extra or {}))
    return subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), *SHORT, *extra, "--dump-outputs", str(out_dir / "dump")],
                            cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _wait(procs):
    outs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(o)
    assert [p.returncode for p in procs] == [0] * len(procs), "\n".join(o[-3000:] for o in outs)
    return outs


@pytest.fixture(scope="module")
def single_dump(gpu, tmp_path_factory):
    d = tmp_path_factory.mktemp("bench_a")
    out, = _wait([_bench(d)])
    head = json.loads(out.strip().splitlines()[-1])
    assert head["steps"] == 2 and head["ms_per_step"] > 0
    return np.load(d / "dump" / "y.npy")


def test_dump_is_the_render_of_the_seeded_inputs(gpu, single_dump, tmp_path):
    import torch

    from sonicsim_amd import ops, synth
    sc = synth.make_scene("cfg2", scene=0)
    assert single_dump.dtype == np.float32 and single_dump.shape == (sc.C, sc.T) and np.isfinite(single_dump).all()
    _wait([_bench(tmp_path)])
    assert np.array_equal(single_dump, np.load(tmp_path / "dump" / "y.npy"))                     # the same bits in a second process
    ops.set_task_queue(True)                                                                       # bench.py's default
    seg = synth.scene_segments(sc, 0)
    bank, peak = ops.rir_bank_synth(sc.delay, sc.dgain, sc.L, sc.fs, sc.rt60, sc.bank_seed, device=gpu, return_peak=True)
    ops.divide_by_(bank, peak)
    y = ops.convolve_moving_seg(torch.from_numpy(sc.x).to(gpu), bank, seg)
    assert np.array_equal(single_dump, y.cpu().numpy())                                            # what a caller of the timed path receives


def test_dump_survives_the_ipc_gather_closing(gpu, single_dump, tmp_path):
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = [_bench(tmp_path / f"r{r}", ["--gpus", "2", "--gather", "ipc", "--gather-every", "1"],
                    dict(RANK=str(r), LOCAL_RANK="0", WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), SS_DIST_BACKEND="gloo",
                         HSA_ENABLE_IPC_MODE_LEGACY="0"))
             for r in range(2)]
    _wait(procs)
    assert not os.path.exists(tmp_path / "r1" / "dump")                                          # rank 0 dumps, the other ranks do not
    assert np.array_equal(np.load(tmp_path / "r0" / "dump" / "y.npy"), single_dump)              # rank 0 renders scene 0, like one rank
