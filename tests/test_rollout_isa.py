"""ISA checks of the rollout kernels (kernel_rollout.hpp).  Their candidate table lives in LDS and is read with wave-uniform
addresses (CandLds), and the device libm they call for the models' tables at off-grid states (cos / sin / tan) may branch per
lane; what must not happen is a register spilled and reloaded under a partial EXEC mask, and a core or table read through a
FLAT address (DESIGN.md's FLAT-access notes).  What a partial EXEC mask can corrupt is data one lane reads from another: a
VGPR written under a partial mask and then read with v_readlane.  The kernels keep no such table (the candidates are in LDS), so
the invariant checked here is that every v_readlane of every rollout kernel reads a VGPR that nothing but v_writelane writes --
the compiler's SGPR spill slots, which v_writelane fills whatever EXEC is -- and that no other cross-lane operation (DPP,
permute, swizzle) occurs.  Per-lane VGPR spills (scratch) of the rank-16 / 20 instantiations are per-lane data and outside that
hazard (the benchmark's ranks have none; tests/test_gpu_sim_kernels.py runs the spilling ones against the oracle).  And no flat_load in any rollout or off-grid stencil kernel."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "c3sc_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _kernels(tmp_path, src):
    out = tmp_path / "k.s"
    subprocess.run([HIPCC, "-std=c++20", "-O3", "-fPIC", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"),
                    "-S", "--cuda-device-only", os.path.join(CSRC, src), "-o", str(out)], check=True, cwd=CSRC,
                   stderr=subprocess.DEVNULL)
    bodies, name, body = {}, None, []
    meta = {}
    text = open(out).read()
    for line in text.splitlines():
        m = re.match(r"^(_ZN4c3sc\w*k_rollout\S*|_ZN4c3sc\w*k_stencil_points\S*):", line)
        if m:
            name, body = m.group(1), []
        elif name and line.startswith(".Lfunc_end"):
            bodies[name] = body
            name = None
        elif name:
            body.append(line)
    for m in re.finditer(r"\.name:\s+(_ZN4c3sc\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", text):
        meta[m.group(1)] = int(m.group(2))
    return bodies, meta


# instantiations whose registers hold the whole step (no scratch): every k_rollout but Dubins3D 20, LqgNd<2> 20, Car7D 16 / 20
# and Cothrust6D 16 / 20 (the test prints each kernel's private segment size; test_gpu_sim_kernels.py runs all of them)
NO_SCRATCH = ("Dubins3DELi4E", "Dubins3DELi6E", "Dubins3DELi8E", "Dubins3DELi12E", "Dubins3DELi16E", "Car7DELi4E", "Car7DELi10E",
              "Car7DELi12E", "LqgNdILi2EEELi4E", "LqgNdILi2EEELi8E", "LqgNdILi2EEELi12E", "Cothrust6DELi4E", "Cothrust6DELi8E",
              "Cothrust6DELi12E")
CROSS_LANE = re.compile(r"\bdpp|row_|quad_perm|ds_swizzle|permlane|ds_bpermute|ds_permute")


def _short(name):
    """k_rollout<Car7D,16> from the mangled name (the model's type and the padded rank; LqgNdILi2EE is LqgNd<2>)"""
    kind = "k_stencil_points" if "k_stencil_points" in name else "k_rollout"
    m = re.search(r"k_stencil_pointsILi(\d+)ELi(\d+)E", name)
    if m:
        return f"{kind}<{m.group(1)},{m.group(2)}>"
    m = re.search(r"NS_\d+([A-Za-z]\w*?)(?:ILi(\d+)EE)?ELi(\d+)ELb", name)
    if not m:
        return name
    model = m.group(1) + (f"<{m.group(2)}>" if m.group(2) else "")
    return f"{kind}<{model},{m.group(3)}>"


def _vregs(op):
    m = re.match(r"v\[(\d+):(\d+)\]", op)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r"v(\d+)$", op)
    return {int(m.group(1))} if m else set()


def _instr(line):
    t = line.strip().split(None, 1)
    if len(t) < 2 or t[0].startswith((";", ".", "s_")) or t[0].endswith(":"):
        return None, []
    return t[0], [o.strip() for o in t[1].split(";")[0].split(",")]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("src", ["inst_rollout_a.hip", "inst_rollout_b.hip"])
def test_rollout_kernels_global_loads_and_no_spills(tmp_path, src):
    bodies, meta = _kernels(tmp_path, src)
    assert len(bodies) >= 10
    seen = 0
    for name in sorted(bodies):  # informational: which instantiations spill, as this compiler builds them (not asserted)
        print(f"{src}: {_short(name)}: private_segment_fixed_size {meta.get(name, 'n/a')} bytes per lane")
    for name, body in bodies.items():
        flat = [l for l in body if re.search(r"\bflat_load", l)]
        assert not flat, f"{name}: {len(flat)} FLAT loads (cores / tables must be read with global_load)"
        assert any("global_load_dwordx2" in l for l in body), name
        if "k_rollout" in name and any(t in name for t in NO_SCRATCH):
            seen += 1
            scratch = [l for l in body if re.search(r"\bscratch_(load|store)", l)]
            assert not scratch, f"{name}: {len(scratch)} scratch accesses (spills)"
    assert seen >= 2


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("src", ["inst_rollout_a.hip", "inst_rollout_b.hip"])
def test_rollout_cross_lane_reads_are_sgpr_spill_slots_only(tmp_path, src):
    bodies, _ = _kernels(tmp_path, src)
    seen = 0
    for name, body in bodies.items():
        if "k_rollout" not in name:
            continue
        seen += 1
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
    assert seen >= 10
