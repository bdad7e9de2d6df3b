"""A real two-process fused adjoint exchange of unstructured fields: two ranks (separate processes,
both on cuda:0) hold two domains of the known-answer case each, so every rank's exchange has self
and peer messages (form 2 of ghx_uexchange_adjoint_self_*). Each rank runs a fused object
(fuse_adjoint_lists=True) and an unfused one on copies of the same fields and compares them byte
for byte, and with the known answer, after each of three exchanges (tests/mp_uget_worker.py). The
workers are started as fresh child processes (never exec'd over this one), each bounded by one time
limit; after a failure nothing more is started."""
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


_FAILED = []      # a case that failed: the cases after it start no process


@pytest.mark.parametrize("levels", [1, 3])
def test_fused_adjoint_exchange_between_two_processes(levels):
    assert not _FAILED, f"not started: the case levels = {_FAILED[0]} failed before"
    _FAILED.append(levels)
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), LOCAL_RANK="0")
        procs.append(subprocess.Popen(
            [sys.executable, os.path.join(HERE, "mp_uget_worker.py"), str(levels), "3"],
            env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs, codes = [], []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=120)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            for q in procs:
                q.wait()
            raise
        outs.append(out)
        codes.append(p.returncode)
    assert codes == [0, 0], "\n".join(outs)
    assert "bad cells 0" in outs[0]
    _FAILED.clear()
