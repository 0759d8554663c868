"""ISA checks of the closed-loop integration kernels (kernel_rollout_ode.hpp, inst_rollout_ode_*.hip): test_rollout_isa.py's
invariants applied to k_rollout_ode.  Every core, grid and table read is a global load (no FLAT); the only cross-lane reads are
v_readlane of SGPR spill slots (VGPRs nothing but v_writelane writes), with no DPP, permute or swizzle; and the instantiations
the tests and the benchmark run keep the whole RK4 step (x, the running stage sum and the stage state next to k_rollout's
registers) without scratch."""
import os
import re

import pytest

from test_rollout_isa import CROSS_LANE, HIPCC, _instr, _vregs
from test_rollout_isa import _kernels as _rollout_kernels

SOURCES = ["inst_rollout_ode_a.hip", "inst_rollout_ode_b.hip", "inst_rollout_ode_c.hip"]
# dubins3d 4 / 6 / 8, lqg2d 4 / 8, car7d 4 / 10, tprob3d 4 / 12, cothrust6d 4 / 8
NO_SCRATCH = ("Dubins3DELi4E", "Dubins3DELi6E", "Dubins3DELi8E", "LqgNdILi2EEELi4E", "LqgNdILi2EEELi8E", "Car7DELi4E", "Car7DELi10E",
              "Tprob3DELi4E", "Tprob3DELi12E", "Cothrust6DELi4E", "Cothrust6DELi8E")


def _ode_kernels(tmp_path, src):
    bodies, meta = _rollout_kernels(tmp_path, src)
    return {k: v for k, v in bodies.items() if "k_rollout_ode" in k}, meta


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("src", SOURCES)
def test_rollout_ode_kernels_global_loads_and_no_spills(tmp_path, src):
    bodies, meta = _ode_kernels(tmp_path, src)
    assert len(bodies) >= 4
    for name, body in bodies.items():
        flat = [l for l in body if re.search(r"\bflat_load", l)]
        assert not flat, f"{name}: {len(flat)} FLAT loads (cores / tables must be read with global_load)"
        assert any("global_load_dwordx2" in l for l in body), name
        if any(t in name for t in NO_SCRATCH):
            scratch = [l for l in body if re.search(r"\bscratch_(load|store)", l)]
            assert not scratch, f"{name}: {len(scratch)} scratch accesses (spills)"
            assert meta.get(name, 0) == 0, f"{name}: private segment of {meta.get(name)} bytes"


def test_rollout_ode_no_scratch_list_covers_its_instantiations(tmp_path):
    """every rank of the no-scratch list is instantiated (the check above is not vacuous)"""
    names = []
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    for src in SOURCES:
        names += list(_ode_kernels(tmp_path, src)[0])
    for t in NO_SCRATCH:
        assert any(t in n for n in names), t


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("src", SOURCES)
def test_rollout_ode_cross_lane_reads_are_sgpr_spill_slots_only(tmp_path, src):
    bodies, _ = _ode_kernels(tmp_path, src)
    assert len(bodies) >= 4
    for name, body in bodies.items():
        slots = set()
        for l in body:
            op, args = _instr(l)
            if op and op.startswith("v_readlane"):
                slots |= _vregs(args[1])
            assert not (op and CROSS_LANE.search(l)), f"{name}: cross-lane operation {l.strip()}"
        for l in body:
            op, args = _instr(l)
            if not op or op.startswith(("v_writelane", "v_readlane", "v_cmp", "v_readfirstlane")) or "store" in op or not args:
                continue
            assert not (_vregs(args[0]) & slots), f"{name}: {l.strip()} writes a VGPR that v_readlane reads"
