"""Build-level checks of the Markov-chain kernels (kernel_chain_walk.hpp, inst_mcwalk_*.hip), no GPU: the C ABI, the
registrations, the compiler's resource remarks of the new kernels, and that no kernel the library had before them changed.

tests/golden/kernel_resources_before_chain.json is tools/kernel_resources.py's table of the build just before the chain kernels
were added (same compiler): build that commit (make -C c3sc_amd/csrc) and copy its c3sc_amd/csrc/kernel_resources.json there.
Only what the compiler allocates per kernel is compared -- registers, spills, scratch, static LDS -- not occupancy.  A change
that reshapes an existing kernel on purpose, or a compiler upgrade, regenerates the file from the build before that change; the
chain kernels themselves must not be the reason.  The chain kernels' own table is c3sc_amd/csrc/chain_res/kernel_resources.json."""
import glob
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

from c3sc_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "c3sc_amd", "csrc")
NEW = ["c3sc_hip_chain_transitions", "c3sc_hip_chain_transitions_host", "c3sc_hip_simulate_chain", "c3sc_hip_simulate_chain_host"]

# No chain kernel keeps a private segment: at the top classes (Dubins3D 16 / 20, LqgNd<2> 20, Car7D 12 / 16 / 20, Cothrust6D
# 16 / 20) the walks spill four VGPRs, to AGPRs.  k_rollout spills to scratch at Car7D 16 / 20 and Cothrust6D 16 / 20.
WALK_SCRATCH_EXCEPTIONS = set()
BENCH_CLASSES = [("Car7D", 10), ("Dubins3D", 6)]


def test_new_symbols_are_exported_with_c_names():
    out = subprocess.run(["nm", "-D", "--defined-only", E.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for n in NEW:
        assert n in names and n in E.EXPORTS
    L = E.load_library()
    assert all(hasattr(L, n) for n in NEW)


def test_headers_still_compile_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "c3sc_hip.h"\n#include "c3sc/bellman.h"\n'
                   "int f(void) { c3sc_hip_chain_args a; a.n = 0; return (int)a.n + (int)C3SC_CHAIN_STUCK(3) + 5; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "t.o")])


def test_the_struct_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "c3sc_hip.h")).read()
    body = re.search(r"typedef struct c3sc_hip_chain_args \{(.*?)\} c3sc_hip_chain_args;", hdr, re.S).group(1)
    fields = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f[0] for f in E.ChainArgs._fields_]


def _registrations(pattern, macro):
    got = set()
    for f in glob.glob(os.path.join(CSRC, pattern)):
        for m in re.finditer(r"^" + macro + r"\(([^()]*)\)", open(f).read(), re.M):
            a = [s.strip() for s in m.group(1).split(",")]
            got.add((a[0], int(a[1]), ",".join(a[3:] if macro == "C3SC_REG_ROLLOUT" else a[2:])))
    return got


def test_every_rollout_pair_has_a_walk_and_a_transitions_registration():
    rollout = _registrations("inst_rollout_[ab].hip", "C3SC_REG_ROLLOUT")
    chain = _registrations("inst_mcwalk_*.hip", "C3SC_CHAIN_KERNELS")
    assert len(rollout) == 20 and chain == rollout
    macro = open(os.path.join(CSRC, "kernel_chain_walk.hpp")).read()
    assert "VARIANT_CHAIN_WALK" in macro and "VARIANT_CHAIN_TRANSITIONS" in macro  # one macro registers both kernels
    srcs = re.search(r"^SRCS\s*=(.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1).split()
    assert {os.path.basename(f) for f in glob.glob(os.path.join(CSRC, "inst_mcwalk_*.hip"))} <= set(srcs)


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    """the compiler's resource remarks of this build, regenerated from the *.res files"""
    tmp = tmp_path_factory.mktemp("res")
    res = glob.glob(os.path.join(CSRC, "*.res")) + glob.glob(os.path.join(CSRC, "chain_res", "*.res"))
    assert len(res) > 3, "the build keeps the compiler's resource remarks next to the objects, the chain kernels' in chain_res/"
    for f in res:
        shutil.copy(f, tmp)
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), str(tmp)], check=True, capture_output=True)
    return json.load(open(tmp / "kernel_resources.json"))


def _chain_entries(resources, kind):
    out = {}
    for name, r in resources.items():
        m = re.match(r"k_chain_" + kind + r"<\d+, (.+), (\d+)>$", name)
        if m:
            out[(m.group(1), int(m.group(2)))] = r
    return out


def test_new_kernels_and_their_private_segments(resources):
    walk, trans = _chain_entries(resources, "walk"), _chain_entries(resources, "transitions")
    assert len(walk) == 20 and set(walk) == set(trans)
    for key in BENCH_CLASSES:
        for r in (walk[key], trans[key]):
            assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spill"] == 0, (key, r)
    for key, r in trans.items():
        assert r["scratch_bytes_per_lane"] == 0, (key, r)
    assert {k for k, r in walk.items() if r["scratch_bytes_per_lane"] != 0} <= WALK_SCRATCH_EXCEPTIONS
    assert all(r["static_lds_bytes"] == 0 for r in list(walk.values()) + list(trans.values()))  # the candidate table is dynamic LDS


def test_no_earlier_kernel_changed(resources):
    before = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_resources_before_chain.json")))
    assert len(before) > 600
    fields = ("vgprs", "agprs", "sgprs", "vgpr_spill", "sgpr_spill", "scratch_bytes_per_lane", "static_lds_bytes")
    pick = lambda r: None if r is None else {f: r.get(f) for f in fields}  # noqa: E731
    changed = {n: (pick(before[n]), pick(resources.get(n))) for n in before if pick(resources.get(n)) != pick(before[n])}
    assert not changed, changed
    assert {n for n in resources if n not in before} == {n for n in resources if n.startswith("k_chain_")}
