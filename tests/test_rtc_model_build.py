"""Run-time compiled device models, compile side (c3sc_hip_model_compile / c3sc_hip_model_code_object): no GPU
is needed.  The code object of a user's model holds the kernels the spec asks for, for gfx950, without scratch at the small
ranks; its rollout kernels keep the cross-lane rule of tests/test_rollout_isa.py (restated here for a code object); errors
come back as codes with the compiler's log; a spec compiled twice is one model; and the library compiles from its embedded
headers alone."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import textwrap

import pytest

from c3sc_amd import engine as E
from rtc_models import DUBINS3D, DUBINS3D_MASKS, PENDULUM, PENDULUM_MASKS, build_example

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.path.join(os.path.dirname(os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))), "..", "llvm", "bin")
OBJDUMP, READELF = os.path.join(LLVM, "llvm-objdump"), os.path.join(LLVM, "llvm-readelf")
ERR_ARG = 1  # C3SC_ERR_ARG


@pytest.fixture(scope="module")
def dubins_co(tmp_path_factory):
    co = E.code_object(DUBINS3D, 3, 1, ranks=(4, 8, 12), name="dubins_rtc", **DUBINS3D_MASKS)
    p = tmp_path_factory.mktemp("co") / "dubins.co"
    p.write_bytes(co)
    return p


@pytest.fixture(scope="module")
def pendulum_co(tmp_path_factory):
    co = E.code_object(PENDULUM, 2, 1, ranks=(4, 8), box=True, name="pendulum_rtc", **PENDULUM_MASKS)
    p = tmp_path_factory.mktemp("co") / "pendulum.co"
    p.write_bytes(co)
    return p


def _meta(path):
    text = subprocess.run([READELF, "--notes", str(path)], check=True, capture_output=True, text=True).stdout
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", text):
        meta[m.group(1)] = int(m.group(2))
    return meta


def _bodies(path):
    text = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", str(path)], check=True, capture_output=True, text=True).stdout
    bodies, name = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(_Z\S+)>:", line)
        if m:
            name = m.group(1)
            bodies[name] = []
        elif re.match(r"^[0-9a-f]+ <", line):
            name = None
        elif name and line.strip():
            bodies[name].append(line.split("//")[0].strip())
    return bodies


def _vregs(op):
    m = re.match(r"v\[(\d+):(\d+)\]", op)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r"v(\d+)$", op)
    return {int(m.group(1))} if m else set()


def _instr(line):
    t = line.split(None, 1)
    if len(t) < 2 or t[0].startswith("s_"):
        return None, []
    return t[0], [o.strip() for o in t[1].split(",")]


CROSS_LANE = re.compile(r"\bdpp|row_|quad_perm|ds_swizzle|permlane|ds_bpermute|ds_permute")


def test_code_object_is_gfx950(dubins_co):
    hdr = subprocess.run([READELF, "-h", str(dubins_co)], check=True, capture_output=True, text=True).stdout
    assert "EM_AMDGPU" in hdr and "gfx950" in hdr


def test_code_object_holds_every_kernel(dubins_co, pendulum_co):
    m = _meta(dubins_co)
    fpw = [k for k in m if "k_fiber_per_wave" in k and "RtcModel" in k]
    # ranks 4, 8: NPL 1 / 2, staged; rank 12: staged and the L2 form launch_fpw falls back to
    assert len(fpw) == 2 + 2 + 4, sorted(fpw)
    for rp in (4, 8, 12):
        assert any(f"Li{rp}ELi1ELb0ELb0ELb1E" in k for k in fpw), rp
        assert any(f"Li{rp}ELi2ELb0ELb0ELb1E" in k for k in fpw), rp
        assert sum("k_rollout_ode" in k and f"Li{rp}ELb0E" in k for k in m) == 1, rp
        assert sum("k_rolloutI" in k and f"Li{rp}ELb0E" in k for k in m) == 1, rp
    assert any("Li12ELi1ELb0ELb0ELb0E" in k for k in fpw)
    mp = _meta(pendulum_co)
    box = [k for k in mp if "k_fiber_per_wave" in k and "RtcModel" in k and "ELb0ELb1ELb1E" in k]
    assert len(box) == 4, sorted(mp)  # the box minimiser at both ranks and both NPL
    assert sum("k_rollout_ode" in k for k in mp) == 2 and all("ELb1EEEvNS_5KArgs" in k for k in mp if "k_rollout" in k)


def test_no_scratch_at_small_ranks(dubins_co, pendulum_co):
    for co in (dubins_co, pendulum_co):
        for name, priv in _meta(co).items():
            if re.search(r"ELi(4|8)E", name):
                assert priv == 0, f"{name}: private segment of {priv} bytes"


def test_rollout_kernels_keep_the_cross_lane_rule(dubins_co, pendulum_co):
    seen = 0
    for co in (dubins_co, pendulum_co):
        for name, body in _bodies(co).items():
            if "k_rollout" not in name:
                continue
            seen += 1
            assert not any(re.search(r"\bflat_load", l) for l in body), f"{name}: FLAT loads"
            assert any("global_load_dwordx2" in l for l in body), name
            slots = set()
            for l in body:
                op, args = _instr(l)
                if op and op.startswith("v_readlane"):
                    slots |= _vregs(args[1])
                assert not (op and CROSS_LANE.search(l)), f"{name}: cross-lane operation {l}"
            for l in body:
                op, args = _instr(l)
                if not op or op.startswith(("v_writelane", "v_readlane", "v_cmp", "v_readfirstlane")) or "store" in op or not args:
                    continue
                assert not (_vregs(args[0]) & slots), f"{name}: {l} writes a VGPR that v_readlane reads"
    assert seen == 3 * 2 + 2 * 2


def test_syntax_error_is_an_argument_error_with_the_line():
    bad = PENDULUM.replace("b[0] = x[1];", "b[0] = x[1] +* ;")
    line = next(i for i, l in enumerate(bad.splitlines(), 1) if "+* ;" in l)
    with pytest.raises(E.C3scHipError) as ei:
        E.code_object(bad, 2, 1, name="broken")
    assert ei.value.args[1] == ERR_ARG
    assert f"broken:{line}:" in ei.value.args[0], ei.value.args[0][:2000]


@pytest.mark.parametrize("kw", [dict(d=1), dict(d=11), dict(du=0), dict(du=5), dict(ranks=(6,)), dict(ranks=(4, 24)),
                                dict(udep_mask=1 << 2), dict(udep_mask=1, uconst_mask=2)])
def test_bad_spec_is_rejected(kw):
    args = dict(d=2, du=1, ranks=(4,))
    args.update(kw)
    with pytest.raises(E.C3scHipError) as ei:
        E.compile_model(PENDULUM, **args)
    assert ei.value.args[1] == ERR_ARG


def test_compile_twice_is_one_model_and_max_rank():
    L = E.load_library()
    a = E.compile_model(PENDULUM, 2, 1, ranks=(4, 12), name="pend_twice", **PENDULUM_MASKS)
    b = E.compile_model(PENDULUM, 2, 1, ranks=(12, 4), name="pend_twice", **PENDULUM_MASKS)
    assert a == b and a >= E.MODEL_USER
    assert L.c3sc_hip_max_rank(a, 2) == 12
    assert L.c3sc_hip_max_rank(a, 3) == 0
    c = E.compile_model(PENDULUM, 2, 1, ranks=(4,), name="pend_twice", **PENDULUM_MASKS)
    assert c != a and L.c3sc_hip_max_rank(c, 2) == 4
    unnamed = [E.compile_model(PENDULUM, 2, 1, ranks=(4,), **PENDULUM_MASKS) for _ in range(2)]
    assert unnamed[0] == unnamed[1] != c
    # a compiled spec's code object is the one its model loads, whatever was compiled since (its id is in the kernel names)
    co = E.code_object(PENDULUM, 2, 1, ranks=(4,), **PENDULUM_MASKS)
    E.compile_model(PENDULUM, 2, 1, ranks=(8,), **PENDULUM_MASKS)
    assert E.code_object(PENDULUM, 2, 1, ranks=(4,), **PENDULUM_MASKS) == co
    assert f"k_rolloutILi{unnamed[0]}E".encode() in co


def test_library_compiles_from_its_embedded_headers(tmp_path):
    lib = tmp_path / "lib" / "libc3sc_hip.so"
    lib.parent.mkdir()
    shutil.copy(E.LIB_PATH, lib)
    work = tmp_path / "elsewhere"
    work.mkdir()
    prog = textwrap.dedent(f"""
        import ctypes as C, sys
        class Spec(C.Structure):
            _fields_ = [("source", C.c_char_p), ("name", C.c_char_p), ("d", C.c_int), ("du", C.c_int), ("udep_mask", C.c_uint),
                        ("uconst_mask", C.c_uint), ("stage_udep", C.c_int), ("box", C.c_int), ("nranks", C.c_int),
                        ("ranks", C.POINTER(C.c_int))]
        L = C.CDLL({str(lib)!r})
        L.c3sc_hip_model_log.restype = C.c_char_p
        s = Spec({PENDULUM!r}.encode(), b"alone", 2, 1, 0, 0, 1, 0, 0, None)
        mid = C.c_int(0)
        rc = L.c3sc_hip_model_compile(C.byref(s), C.byref(mid))
        print(rc, mid.value, L.c3sc_hip_model_log().decode()[:2000])
        sys.exit(rc)
    """)
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    r = subprocess.run([sys.executable, "-c", prog], cwd=work, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert int(r.stdout.split()[1]) >= 1000


def test_example_compiles(tmp_path):
    assert os.path.exists(build_example(tmp_path))
