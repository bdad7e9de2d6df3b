"""The cubed-sphere bulk exchange between real processes: six ranks, one cube tile each, all on
cuda:0, putting rotated halos into each other's fields through IPC mappings under device-side
epochs. The workers are started as child processes (never exec'd over this one) and are bounded
by a timeout."""
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_six_processes_put_into_each_others_halos():
    """c = 6, halos (1, 2, 0, 3), an f32 2-vector (x stride-1) and an f64 scalar (y stride-1) per
    rank, one bulk object per process, 3 exchanges with the interiors rewritten before each:
    every cell of every rank holds the expectation expanded from the recorded fixture."""
    world, port = 6, _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), LOCAL_RANK="0")
        procs.append(subprocess.Popen(
            [sys.executable, os.path.join(HERE, "mp_cs_put_worker.py"), "3"],
            env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs, codes = [], []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=120)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(out)
        codes.append(p.returncode)
    assert codes == [0] * world, "\n".join(outs)
    assert "bad cells 0" in outs[0]
