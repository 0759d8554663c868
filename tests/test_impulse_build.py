"""Impulse control, compile side (c3sc_hip_model_compile_ic / c3sc_hip_model_code_object_ic): no GPU is needed.
The new symbols are exported; an impulse model's code object is for gfx950 and holds the impulse forms of the per-wave kernels
(at rank 12 the L2 form too) and of k_rollout for the plain model and, with njump > 0, for the jump model, next to the forms
without interventions, never a k_rollout_ode form, with the rollouts' cross-lane rule and no scratch at ranks 4 and 8;
nimpulse = 0 yields the _jd code object instruction for instruction and needs no impulse function in the source; nimpulse
outside 0..8 is an argument error, interventions with a game, the box, horizon or stop are refused; the library itself holds no
impulse kernel and keeps its 666 entries; KArgs keeps its size."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from c3sc_amd import engine as E
import impulse_lib as IL
import jump_lib as JL
from test_rtc_model_build import CROSS_LANE, READELF, _bodies, _instr, _meta, _vregs

ERR_ARG, ERR_UNSUPPORTED = 1, 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (source, d, du, masks, njump, nimpulse)
MODELS = {"lqr": (IL.LQR, 2, 2, IL.LQR_MASKS, 0, IL.LQR_NIMPULSE), "lqr_jump": (IL.LQR_JUMP, 2, 2, IL.LQR_MASKS, JL.LQR_NJUMP, IL.LQR_NIMPULSE),
          "lqr3": (IL.LQR3, 3, 3, IL.LQR3_MASKS, JL.LQR3_NJUMP, IL.LQR3_NIMPULSE)}


def _co(tmp_path_factory, model, tag, **kw):
    src, d, du, masks, nj, ni = MODELS[model]
    co = E.code_object(src, d, du, name=f"{model}_{tag}", njump=nj, nimpulse=ni, **masks, **kw)
    p = tmp_path_factory.mktemp("co") / f"{model}_{tag}.co"
    p.write_bytes(co)
    return p


def test_new_symbols_are_exported_with_plain_c_names():
    L = E.load_library()
    for n in ("c3sc_hip_model_compile_ic", "c3sc_hip_model_code_object_ic", "c3sc_hip_set_impulses"):
        assert hasattr(L, n), n
        assert n in E.EXPORTS, n
    assert E.IMPULSE_MAX == IL.IMPULSE_MAX == 8


def test_decode_action():
    import numpy as np

    assert E.decode_action(3, 25) == ("control", 3)
    assert E.decode_action(25, 25) == ("stop", 0)
    assert E.decode_action(26, 25) == ("impulse", 0) and E.decode_action(28, 25) == ("impulse", 2)
    assert E.decode_action(-1, 25) == ("absorbed", -1)
    kind, idx = E.decode_action(np.array([0, 24, 25, 26, 33, -1]), 25)
    assert list(kind) == ["control", "control", "stop", "impulse", "impulse", "absorbed"] and list(idx) == [0, 24, 0, 0, 7, -1]


def _impulse(m, jump):
    """the impulse kernels of the plain (ImpulseOf<RtcModel>) or the jump (ImpulseOf<JumpOf<RtcModel>>) model"""
    inner = "9ImpulseOfINS_" + ("6JumpOfINS_" if jump else "") + "8RtcModel"
    return [k for k in m if inner in k]


def _expect_forms(names, ranks):
    for rp in ranks:
        for npl in (1, 2):
            for staged in ((1,) if rp < 12 else (0, 1)):
                n = sum("k_fiber_per_wave" in k and f"ELi{rp}ELi{npl}ELb0ELb0ELb{staged}E" in k for k in names)
                assert n == 1, (rp, npl, staged, n)
        assert sum("k_rolloutI" in k and f"ELi{rp}ELb0E" in k for k in names) == 1, rp
    assert not any("k_rollout_ode" in k for k in names), "integrate has no impulse form"
    assert len(names) == sum((2 if rp < 12 else 4) + 1 for rp in ranks), names


def _check_lane_rule(co, expect):
    """the rollouts' lane rule of DESIGN.md 4.8 on the impulse rollouts: global loads only, no cross-lane operation, v_readlane
    of SGPR spill slots alone"""
    seen = 0
    for name, body in _bodies(co).items():
        if "k_rollout" not in name or "ImpulseOf" not in name:
            continue
        seen += 1
        assert not any("flat_load" in l for l in body), f"{name}: FLAT loads"
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
    assert seen == expect, (seen, expect)


@pytest.mark.parametrize("model", ["lqr", "lqr_jump"])
def test_impulse_code_object_holds_the_impulse_forms(tmp_path_factory, model):
    jump = model == "lqr_jump"
    co = _co(tmp_path_factory, model, "ic", ranks=(4, 8))
    hdr = subprocess.run([READELF, "-h", str(co)], check=True, capture_output=True, text=True).stdout
    assert "EM_AMDGPU" in hdr and "gfx950" in hdr
    m = _meta(co)
    _expect_forms(_impulse(m, False), (4, 8))
    if jump:
        _expect_forms(_impulse(m, True), (4, 8))
    else:
        assert not _impulse(m, True)
    assert len([k for k in m if "ImpulseOf" in k]) == (2 if jump else 1) * 2 * 3
    _check_lane_rule(co, (2 if jump else 1) * 2)
    # the forms without interventions are all there as the _jd spec gives them
    assert len([k for k in m if "RtcModel" in k and "ImpulseOf" not in k and "JumpOf" not in k]) == 2 * 4
    assert len([k for k in m if "JumpOf" in k and "ImpulseOf" not in k]) == (2 * 3 if jump else 0)
    for name, priv in m.items():
        if "k_fiber_per_wave" in name:
            assert priv == 0, f"{name}: private segment of {priv} bytes at ranks 4 and 8"


def test_impulse_forms_at_rank_12_include_the_l2_per_wave_kernel(tmp_path_factory):
    m = _meta(_co(tmp_path_factory, "lqr_jump", "ic_r12", ranks=(12,)))
    _expect_forms(_impulse(m, False), (12,))
    _expect_forms(_impulse(m, True), (12,))
    m3 = _meta(_co(tmp_path_factory, "lqr3", "ic_r12", ranks=(12,)))
    _expect_forms(_impulse(m3, False), (12,))
    _expect_forms(_impulse(m3, True), (12,))


@pytest.mark.parametrize("njump", [0, 3])
def test_spec_with_nimpulse_0_yields_the_jd_code_object(tmp_path, njump):
    """... and needs no impulse function in the source"""
    src, masks = (JL.LQR, JL.LQR_MASKS)
    name = f"lqr_ic0_{njump}"
    ref = E.code_object(src, 2, 2, ranks=(4, 8), name=name, njump=njump, **masks)
    L = E.load_library()
    spec = E._model_spec(src, 2, 2, (4, 8), False, masks["udep_mask"], masks["uconst_mask"], True, name)
    ic = E.ModelSpecIc(E.ModelSpecJd(E.ModelSpecOs(E.ModelSpecFh(E.ModelSpecEx(spec, 0), 0), 0), njump), 0)
    size = C.c_size_t(len(ref) + 1024)
    buf = C.create_string_buffer(size.value)
    assert L.c3sc_hip_model_code_object_ic(C.byref(ic), buf, C.byref(size)) == 0
    assert b"ImpulseOf" not in ref
    a, b = tmp_path / "jd.co", tmp_path / "ic.co"
    a.write_bytes(ref)
    b.write_bytes(buf.raw[:size.value])
    assert _meta(a) == _meta(b) and _bodies(a) == _bodies(b)  # equal metadata and equal bodies


def test_source_without_the_impulse_function_compiles_only_with_nimpulse_0():
    with pytest.raises(E.C3scHipError) as ei:
        E.compile_model(JL.LQR, 2, 2, ranks=(4,), name="lqr_noimpulsefn", nimpulse=2, **JL.LQR_MASKS)
    assert ei.value.args[1] == ERR_ARG
    assert "impulse" in str(ei.value)


def test_nimpulse_out_of_range_is_an_argument_error():
    L = E.load_library()
    spec = E._model_spec(IL.LQR, 2, 2, (4,), False, 0, 0, True, "lqr_ic_bad")
    mid = C.c_int(0)
    for ni in (-1, 9, 100):
        ic = E.ModelSpecIc(E.ModelSpecJd(E.ModelSpecOs(E.ModelSpecFh(E.ModelSpecEx(spec, 0), 0), 0), 0), ni)
        assert L.c3sc_hip_model_compile_ic(C.byref(ic), C.byref(mid)) == ERR_ARG
        size = C.c_size_t(0)
        assert L.c3sc_hip_model_code_object_ic(C.byref(ic), None, C.byref(size)) == ERR_ARG
    assert L.c3sc_hip_model_compile_ic(None, C.byref(mid)) == ERR_ARG
    size = C.c_size_t(0)
    assert L.c3sc_hip_model_code_object_ic(None, None, C.byref(size)) == ERR_ARG
    with pytest.raises(E.C3scHipError) as ei:
        E.compile_model(IL.LQR, 2, 2, ranks=(4,), nimpulse=9, **IL.LQR_MASKS)
    assert ei.value.args[1] == ERR_ARG


@pytest.mark.parametrize("kw", [dict(game=True), dict(box=True), dict(horizon=True), dict(stop=True)])
def test_interventions_with_game_box_horizon_or_stop_are_refused(kw):
    with pytest.raises(E.C3scHipError) as ei:
        E.compile_model(IL.LQR, 2, 2, ranks=(4,), nimpulse=3, **kw)
    assert ei.value.args[1] == ERR_UNSUPPORTED


def test_a_model_with_eight_interventions_compiles(tmp_path):
    src = IL.KNOWN.replace("prm[5 + m]", "prm[5 + (m % 3)]")
    co = E.code_object(src, 2, 2, ranks=(4,), name="known_ic8", nimpulse=8, **IL.KNOWN_MASKS)
    p = tmp_path / "k8.co"
    p.write_bytes(co)
    assert len([k for k in _meta(p) if "ImpulseOf" in k]) == 3


def test_library_kernels_have_no_impulse_form(tmp_path):
    """the compiler's resource remarks of this build, regenerated from the *.res files: no library kernel is an impulse
    instantiation, and the library still has its 666 entries"""
    import glob
    import json
    import shutil

    res = glob.glob(os.path.join(ROOT, "c3sc_amd", "csrc", "*.res"))
    assert res, "the build keeps the compiler's resource remarks next to the objects"
    for f in res:
        shutil.copy(f, tmp_path)
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), str(tmp_path)], check=True, capture_output=True)
    names = json.load(open(tmp_path / "kernel_resources.json"))
    assert len(names) == 666
    assert not any("ImpulseOf" in n for n in names)


def test_kargs_keeps_its_size(tmp_path):
    """whether a launch takes the impulse form is host state (the FORM_IMPULSE bit of LaunchIO::form): the kernels' argument block is the old one"""
    src = tmp_path / "kargs.hip"
    src.write_text('#include "kernel_common.hpp"\nstatic_assert(sizeof(c3sc::KArgs) == 1368);\nstruct M0 {};\n'
                   "static_assert(c3sc::model_impulse<c3sc::ImpulseOf<c3sc::JumpOf<M0>>>());\n"
                   "static_assert(c3sc::model_jump<c3sc::ImpulseOf<c3sc::JumpOf<M0>>>());\n"
                   "static_assert(!c3sc::model_impulse<c3sc::JumpOf<M0>>());\n")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "-std=c++20", "-x", "hip", "--offload-arch=gfx950", "-fsyntax-only",
                        "-I", os.path.join(ROOT, "c3sc_amd", "csrc"), "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_ctypes_spec_has_the_c_struct_layout(tmp_path):
    """engine.ModelSpecIc against struct c3sc_hip_model_spec_ic of include/c3sc_hip.h: size and the offset of nimpulse, checked
    by the C compiler"""
    src = tmp_path / "spec.c"
    src.write_text('#include <stddef.h>\n#include "c3sc_hip.h"\n'
                   f"_Static_assert(sizeof(c3sc_hip_model_spec_ic) == {C.sizeof(E.ModelSpecIc)}, \"size\");\n"
                   f"_Static_assert(offsetof(c3sc_hip_model_spec_ic, nimpulse) == {E.ModelSpecIc.nimpulse.offset}, \"nimpulse\");\n"
                   f"_Static_assert(offsetof(c3sc_hip_model_spec_ic, jd.njump) == {E.ModelSpecJd.njump.offset}, \"njump\");\n"
                   f"_Static_assert(C3SC_IMPULSE_MAX == {E.IMPULSE_MAX}, \"max\");\n")
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
