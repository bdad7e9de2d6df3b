"""A real two-process cubed-sphere adjoint exchange with the self messages fused: two ranks (separate
processes, both on cuda:0, gloo, staging="host") hold three tiles of the c = 6 configuration each
and run make_communication_object(adjoint_rotated=True, fuse_adjoint_rotated=True).adjoint_exchange
beside an unfused object on equal inputs, an fp64 scalar and an f32 3-vector per domain
(tests/mp_cs_get_worker.py). Fused and unfused fields must agree bit for bit. The workers are started
as fresh child processes (never exec'd over this one), each is bounded by a time limit of its own,
and once one has failed or run out of time the other is ended and nothing more runs."""
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


def test_fused_and_unfused_cubed_sphere_adjoint_between_two_processes():
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), LOCAL_RANK="0")
        procs.append(subprocess.Popen(
            [sys.executable, os.path.join(HERE, "mp_cs_get_worker.py"), "4"],
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
        if p.returncode != 0:
            for q in procs:
                if q.poll() is None:
                    q.kill()
    assert codes == [0, 0], "\n".join(outs)
    assert "forms [2, 0] bad cells 0" in outs[0]
