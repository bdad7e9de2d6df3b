"""Real multi-process bulk exchanges of an unstructured field: 2 and 4 ranks (separate
processes, all on cuda:0), zero-copy index-list puts (ghx_uput_create, k_put_u) into the peers'
fields through IPC mappings, ordered by the device epochs; and two emulated hosts, where the puts
stay inside a host and the host-staged buffered exchange carries the rest. Every cell of every
rank is checked after each of three exchanges from rewritten fields (tests/mp_ubulk_worker.py).
The workers are started as child processes (never exec'd over this one), one bulk object each,
and are bounded by a timeout."""
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


def _run(world, cells, levels, mode, reps=3):
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), LOCAL_RANK="0")
        procs.append(subprocess.Popen(
            [sys.executable, os.path.join(HERE, "mp_ubulk_worker.py"), str(cells), str(levels),
             str(reps), mode],
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


@pytest.mark.parametrize("world,levels", [(2, 1), (4, 3)])
def test_bulk_unstructured_multi_process(world, levels):
    """3000 cells per rank in a random storage order, 750 halo cells drawn from every other rank:
    levels 1 (8-byte rows: the run path) on 2 ranks, levels 3 (24-byte rows) on 4."""
    _run(world, 3000, levels, "bulk")


def test_bulk_unstructured_two_emulated_hosts():
    """4 ranks on two emulated hosts: puts between the two ranks of a host, the host-staged
    buffered exchange of the pattern's remote part between the hosts, one exchange()."""
    _run(4, 3000, 2, "mixed")
