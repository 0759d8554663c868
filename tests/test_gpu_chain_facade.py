"""The reference API of the Markov chain on the GPU: in a child process, c3control_simulate_chain_batch (the device walk through
libc3sc.so) against the host twin c3control_simulate_chain on 32 trajectories in lock-step (tests/chain_facade_child.py has the
rules)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_batch_against_the_host_twin_in_a_child_process(oracle):
    r = subprocess.run([sys.executable, os.path.join(HERE, "chain_facade_child.py")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "held to the host twin's whole walk" in r.stdout
