"""Two real processes (gloo, both on cuda:0, host staging) run the adjoint exchange of
cubed-sphere fields: three tiles of the c = 6 configuration per rank, so every rank has self
messages, peer sends and peer receives. k_pack_x and the ordinary reverse pack gather the halo
cells, rotated and negated, into the receive buffers, gloo carries the peer receive buffers back
into the peers' send buffers (the forward routing with the roles swapped), k_accum_s sums from the
send buffers. Every cell of every rank is checked after each of two adjoint exchanges from
rewritten fields, then after a forward exchange of the same object
(tests/mp_cs_adjoint_worker.py). The workers are started as fresh child processes (never exec'd
over this one) and are bounded by a timeout."""
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


@pytest.mark.parametrize("zero_halos", [1, 0], ids=["zero", "keep"])
def test_adjoint_exchange_between_two_processes(zero_halos):
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), LOCAL_RANK="0")
        procs.append(subprocess.Popen(
            [sys.executable, os.path.join(HERE, "mp_cs_adjoint_worker.py"), "2", str(zero_halos)],
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
    assert codes == [0, 0], "\n".join(outs)
    assert "bad cells 0" in outs[0]
